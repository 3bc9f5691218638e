// kg_regex_dev.h — what the two -E scans share (kg_regex.hip: one class sequence; kg_regex_alt.hip: an alternation of them).  Each
// file keeps its walk over a lane's 16 bytes and what it reads off the walk; everything around the walk stands here, once:
//   the program a plan holds (RegexProg: the kind the compilers said, that kind's payload — for a line walk the RegexWalk of
//     kg_regex_compile.h as it stands — and the table on the device), the unit size, the launch modes and RxOut, the tail of both kernels' argument structs;
//   device: the LDS table fill, the loader of a round (with the newline behind the text), a lane's range and newline masks, the -c
//     line state of a unit (RxLineCarry), the wave prefix sum and the record store of the emitting launch, the end of a unit;
//   host: the grid of a launch, and the declarations of the window driver (rx_window, rx_drive: defined in kg_regex.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <functional>

#include "../../include/krep_gpu.h"
#include "kg_common.h"
#include "kg_device.h"
#include "kg_internal.h"
#include "kg_plan.h"

namespace kg {

struct RegexProg
{
    RegexCompiled::Kind kind = RegexCompiled::kSeq; // which scan runs it: kg_regex.hip | kg_regex_alt.hip | kg_regex_loops.hip
    u32 *d_table = nullptr;                         // the kind's table (rx_seq_table, rx_alt_table, RegexWalk::table) on the device
    krep_gpu_regex_anchored_t info{};               // kSeq
    // kAlt (the alternation or the expanding compiler took the search; the filter of a line walk): alt_bol / alt_eol say the place
    // { '\n' } in front of / behind every branch's classes; init and fin as rx_alt_table() gives them
    krep_gpu_regex_alt_t alt{};
    u32 alt_bol = 0, alt_eol = 0;
    u32 init = 0, fin = 0;
    // kWalk (the loops or the groups compiler took the search): the line walk's program, and the inner plans and the scratch of its
    // scan, made by the plan's first scan
    RegexWalk walk{};
    struct RxLoopsWork *work = nullptr;
};
void rx_loops_work_free(RxLoopsWork *w); // kg_regex_loops.hip

constexpr u32 kRxUnitBytes = kRoundsBig * kSegBytes; // 32 KiB of coordinates per wave unit

// the three launches of a scan: count the owned hits of every unit | write their records behind offsets[unit] | -c
constexpr int kRxCount = 0, kRxEmit = 1, kRxLines = 2;

// the last member of both kernels' argument structs: what the window driver sets between the launches of one scan
struct RxOut
{
    u64 *unitinfo;      // counting launches: per-unit info words (nullptr: only the total is wanted)
    const u64 *offsets; // emit: exclusive index of each unit's first record
    u64 *positions;
    u64 pos_cap;
    Counters *ctr;
};

// ------------------------------------------------------------------------------------------------ device
// T in LDS once per bank: entry b of copy k at dword b * 32 + k, a lane reads copy lane % 32
static __device__ __forceinline__ void rx_fill_table(u32 *s_T, const u32 *table)
{
    for (u32 i = threadIdx.x; i < 256u * 32u; i += kBlock)
        s_T[i] = table[i >> 5];
    __syncthreads();
}
// 16 bytes from `off`, bytes at or past text_len read as 0
static __device__ __noinline__ uint4 rx_load_guarded(const uint8_t *text, u64 text_len, u64 off)
{
    u32 v[4];
#pragma unroll
    for (int w = 0; w < 4; ++w)
    {
        u32 x = 0;
        for (int b = 0; b < 4; ++b)
        {
            const u64 o = off + (u64)(w * 4 + b);
            if (o < text_len)
                x |= (u32)text[o] << (8 * b);
        }
        v[w] = x;
    }
    return make_uint4(v[0], v[1], v[2], v[3]);
}
// $: the newline behind the last byte of the text, put into the 16 bytes from q when they hold offset text_len
static __device__ __forceinline__ void rx_put_eot(uint4 &d, u64 q, u64 text_len)
{
    const u64 rel = text_len - q;
    if (rel < 16u)
    {
        const u32 nl = 0x0au << (8u * ((u32)rel & 3u)), w = (u32)rel >> 2;
        d.x |= w == 0u ? nl : 0u;
        d.y |= w == 1u ? nl : 0u;
        d.z |= w == 2u ? nl : 0u;
        d.w |= w == 3u ? nl : 0u;
    }
}
// a round: the lane's 16 bytes of each of the 8 cells from `seg`.  fast (the round lies inside the text): nontemporal vector loads;
// else guarded loads, nothing of a cell at or behind cov_hi, and with eot the newline behind the text.  a: the kernel's arguments
// (text, text_len, cov_hi), read where they are used: handed over as three values they cost regex_scan scalar registers
// (its emitting instantiation 106 for 104, 69 VGPRs for 68)
template <class Args>
static __device__ __forceinline__ void rx_load_round(uint4 (&d)[kCells], const Args &a, u64 seg, u32 lane, bool fast, bool eot)
{
    const uint8_t *text = a.text;
    const u64 text_len = a.text_len, cov_hi = a.cov_hi;
    if (fast)
    {
        const uint4 *src = reinterpret_cast<const uint4 *>(text + seg) + lane;
#pragma unroll
        for (int j = 0; j < kCells; ++j)
        {
            typedef u32 u32x4 __attribute__((ext_vector_type(4)));
            const u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(src + j * kWave));
            d[j] = make_uint4(v.x, v.y, v.z, v.w);
        }
        return;
    }
#pragma unroll
    for (int j = 0; j < kCells; ++j)
    {
        const u64 cb = seg + (u64)j * kCellBytes;
        d[j] = cb < cov_hi ? rx_load_guarded(text, text_len, cb + (u64)lane * 16u) : make_uint4(0u, 0u, 0u, 0u);
    }
    if (eot)
    {
#pragma unroll
        for (int j = 0; j < kCells; ++j)
            rx_put_eot(d[j], seg + (u64)j * kCellBytes + (u64)lane * 16u, text_len);
    }
}
// bit k set iff lo <= q + k < hi, k = 0..15
static __device__ __forceinline__ u32 rx_range(u64 q, u64 lo, u64 hi)
{
    const u32 lk = lo > q ? (u32)min(lo - q, (u64)16) : 0u, hk = hi > q ? (u32)min(hi - q, (u64)16) : 0u;
    return ((1u << hk) - 1u) & ~((1u << lk) - 1u);
}
static __device__ __forceinline__ u32 rx_newlines(const uint4 &d)
{
    return movemask4(eq_bytes(d.x, 0x0a0a0a0au)) | (movemask4(eq_bytes(d.y, 0x0a0a0a0au)) << 4) |
           (movemask4(eq_bytes(d.z, 0x0a0a0a0au)) << 8) | (movemask4(eq_bytes(d.w, 0x0a0a0a0au)) << 12);
}

// -c: the line state of a unit, carried from cell to cell.  cell() is the carry arithmetic over the 64 lanes of a cell from four
// ballots, whatever a lane holds; lane16() makes them for a lane of 16 coordinates.  The same cell() arithmetic also stands in
// kg_literal.hip, kg_ac_tiny.hip and kg_ac_common.h (ac_line_pass): those kernels have register budgets tuned one by one and keep
// their copies; the ballot interface is the one they could take over.
struct RxLineCarry
{
    u32 cnt = 0;   // per lane: matches that are the first of their line within the lane's coordinates
    u32 fresh = 0; // uniform: lanes whose first match stands on a line that held none when it entered the lane
    bool open = false, seen = false, head = false; // uniform: the line that leaves the cell holds a match | a newline so far | a match in front of the first

    // B_nl: lanes with a newline; B_any: with a match; B_head: whose lowest flag is a match; B_tail: with a match behind their last newline
    __device__ __forceinline__ void cell(u64 B_nl, u64 B_any, u64 B_head, u64 B_tail)
    {
        const u64 G = B_tail, P = ~(B_nl | B_any);
        const unsigned __int128 sum = (unsigned __int128)(G | P) + G + (open ? 1u : 0u);
        const u64 O = (u64)sum ^ P; // bit l: the line entering lane l already holds a match
        fresh += (u32)__popcll(B_head & ~O);
        if (!seen && B_nl)
        {
            const int f = __builtin_ctzll(B_nl);
            head = (((O | B_head) >> f) & 1ull) != 0ull;
            seen = true;
        }
        open = (u64)(sum >> 64) != 0ull;
    }
    // H: the lane's owned matches at its 16 coordinates; nl, nl_prev: the raw newline masks of its and of the previous lane's 16 bytes,
    // which stand sh coordinates further up
    __device__ __forceinline__ void lane16(u32 H, u32 nl, u32 nl_prev, u32 sh)
    {
        const u32 N = ((nl << sh) | (nl_prev >> (16u - sh))) & 0xffffu, Hs = H | N;
        cnt += (u32)__popc(H & ~(Hs - ((N << 1) & 0xffffu)));
        // head: the lowest flag is a match (one ON a newline belongs to the line it ends); tail: a match behind the last newline
        cell(__ballot(N != 0u), __ballot(H != 0u), __ballot((H & (Hs ^ (Hs - 1u))) != 0u), __ballot((H >> (32 - __clz((int)N))) != 0u));
    }
    // t: cnt summed over the wave
    __device__ __forceinline__ LineState state(u32 t) const { return LineState{t + fresh, seen, seen ? head : open, open}; }
};

// emit: the inclusive prefix sum of c over the lanes of the wave
static __device__ __forceinline__ u32 rx_wave_incl(u32 c, u32 lane)
{
    u32 incl = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1)
    {
        const u32 t = __shfl_up(incl, o);
        if (lane >= (u32)o)
            incl += t;
    }
    return incl;
}
// emit: record idx = (s0, e0), one 16-byte store
static __device__ __forceinline__ void rx_store_record(u64 *positions, u64 idx, u64 s0, u64 e0)
{
    *reinterpret_cast<uint4 *>(positions + 2 * idx) = make_uint4((u32)s0, (u32)(s0 >> 32), (u32)e0, (u32)(e0 >> 32));
}
// the end of a unit in a counting launch: the lanes' hits summed over the wave (returned, uniform) and the unit's info word
template <bool LINES>
static __device__ __forceinline__ u32 rx_unit_end(u32 l_hits, const RxLineCarry &lc, u64 *unitinfo, u64 unit, u32 lane)
{
    u32 h = l_hits, t = lc.cnt;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1)
    {
        h += __shfl_xor(h, o);
        if (LINES)
            t += __shfl_xor(t, o);
    }
    if (unitinfo && lane == 0)
    {
        u64 info = (u64)h;
        if (LINES)
        {
            const LineState ls = lc.state(t);
            info |= line_bits(ls) | ((u64)(ls.cnt & kUiLineMask) << kUiLineShift);
        }
        else if (h)
            info |= kLnHead | kLnTail;
        unitinfo[unit] = info;
    }
    return h;
}

// ------------------------------------------------------------------------------------------------ host
// one launch over n_units wave units: at most wg_per_cu workgroups per compute unit, a wave takes unit after unit
template <class Args>
static hipError_t rx_launch_grid(void (*kernel)(const Args), const Args &a, u64 n_units, int num_cu, u32 wg_per_cu, hipStream_t st)
{
    const u64 blocks = (n_units + kWavesPerBlk - 1) / kWavesPerBlk;
    u32 grid = (u32)std::max<u64>(1, std::min<u64>(blocks, (u64)num_cu * wg_per_cu));
    if (const int force = g_rx_force_grid.load(); force > 0) // test hook: a starved grid (krep_gpu_debug_force_regex_grid)
        grid = std::min<u32>(grid, (u32)force);
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), 0, st, a);
    return hipGetLastError();
}

// The window driver (kg_regex.hip).  A scan names its pattern in an RxSpec, rx_window() checks the window against it and says
// what is to do, the scan fills its kernel's arguments from that, rx_drive() runs the launches and fills *out.
struct RxSpec
{
    const u32 *lens;       // the occurrence lengths: one L, or the branches'
    u32 n_lens, Lmin;
    bool bol, eol;         // ^ / $: the byte in front of / behind an occurrence decides it
    bool overlap;          // two occurrences can share a byte: without -c the matches are a greedy selection over one window
    const char *one_window; // ... and the refusal of any other window
    WalkSpec walk;         // the greedy pass over the occurrence list, which is put into start order first when `sort`
    bool sort;
};
struct RxWindow
{
    bool empty;     // the window owns nothing that can match: the zeroed *out is the answer, no launch
    u64 own_hi;     // min(w.own_hi, text_len)
    u64 hi_match;   // starts at or behind it hold no occurrence: min(own_hi, text_len - Lmin + 1)
    bool lines, greedy;
    u32 entry0;     // ^ and the buffer begins the text: a newline stands in front of byte 0
    u32 eot;        // $ and the buffer ends the text: a newline stands behind the last byte (not under -i)
    u64 want;       // records the caller takes
};
// 0, or 2 with the error set: a window this pattern cannot be scanned in
int rx_window(const krep_gpu_plan *pl, const Window &w, const match_position_t *d_pos, uint64_t cap, const RxSpec &sp, RxWindow *g);
// launch(mode): one of kRxCount / kRxEmit / kRxLines over n_units units, with what *o holds at that moment
int rx_drive(krep_gpu_plan *pl, const Window &w, const RxSpec &sp, const RxWindow &g, match_position_t *d_pos, uint64_t cap, hipStream_t st,
             int time_it, RxOut *o, u64 n_units, const std::function<hipError_t(int)> &launch, krep_gpu_scan_out_t *out);
// the result of one window from its totals, as every -E scan reports it: the line bits of `summary`, count under max_count and its 0
// corner, stored / overflow for a caller that takes `want` of the records
void rx_fill_out(const krep_gpu_plan *pl, bool lines, uint64_t total, uint64_t nlines, unsigned long long summary, const match_position_t *d_pos,
                 uint64_t cap, uint64_t want, krep_gpu_scan_out_t *out);

// kg_regex_alt.hip: the scan of a window for an alternation (scan_regex hands over when the program is one)
int scan_regex_alt(krep_gpu_plan *pl, const Window &w, match_position_t *d_pos, uint64_t cap, hipStream_t st, int time_it,
                   krep_gpu_scan_out_t *out);
// kg_regex_loops.hip: the scan of the whole text for places that may repeat (scan_regex hands over when the program is of that kind)
int scan_regex_loops(krep_gpu_plan *pl, const Window &w, match_position_t *d_pos, uint64_t cap, hipStream_t st, int time_it,
                     krep_gpu_scan_out_t *out);
} // namespace kg
