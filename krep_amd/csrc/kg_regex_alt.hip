// kg_regex_alt.hip — krep -E for an ALTERNATION of fixed-length class sequences (include/krep_gpu.h, krep_gpu_regex_compile_alt and
// krep_gpu_regex_compile_ext): ERROR|WARN|FATAL, cat|d[oi]g|b.rd, every -E run with several -e, colou?r, ^(ERROR|WARN).  The multi-branch shift-and scan kernel and its scan
// kg::scan_regex_alt; kg_regex.hip keeps the single sequence and hands over when the plan's program is an alternation.  The scan
// names its pattern and fills the kernel's arguments; the window checks, the launches and the result are the window driver's
// (rx_window / rx_drive, kg_regex.hip).  What the kernel does around its walks comes from kg_regex_dev.h.
//
// The kernel.  Branch i lives in bits [o_i, o_i + L_i) of a 32-bit state; T[byte] has bit o_i + j set when byte is in C[i][j]
// (in LDS once per bank, rx_fill_table: 32 KiB); INIT holds every o_i, FIN every o_i + L_i - 1, and
// one step is S = ((S << 1) | INIT) & T[b].  The bit a branch shifts out of its top lands on the next branch's INIT bit (set
// anyway) or on a bit T never holds, so the branches do not disturb each other.
// A lane takes 16 bytes.  (1) It walks its last Lmax - 1 bytes from the all-ones state: with every L_i <= 16 the state behind them
// is exact in every bit a later step can use, and one cross-lane move hands it to the next lane as that lane's TRUE entry state
// (lane 0: the exit of lane 63 of the cell before, kept in a scalar; the first cell of a unit: the 16 bytes in front of it).
// (2) It walks its 16 bytes from the true entry state and keeps the 16-bit mask of the bytes behind which any FIN bit is set.
// Bytes at or behind text_len are masked out of it before anything else: guarded loads read 0 there and a class may hold NUL.
// (3) A wave without a hit is done with the cell; in the others the lanes that hold hits walk again and read off, byte by byte,
// which branches end there: the branch of FIN bit f begins at the highest INIT bit at or below f, which gives its length.
// A hit of length L behind byte e is the occurrence (e - L + 1, e + 1), owned when its START lies in [own_lo, own_hi).
//   count / records: one unit per (end, branch) pair, in end order and within an end in branch order.  When no two occurrences
//     can share a byte (cross_overlap == 0) there is at most one pair per end, end order is start order and every occurrence is a
//     match; a cell whose ends all lie in [own_lo + Lmax - 1, own_hi) owns whatever ends in it and is counted from the mask alone.
//     The counting and the emitting launch count a lane with the same function (the two-pass offsets scheme of kg_post.hip).
//   cross_overlap == 1 without -c: every pair goes to post.d_occ, the device sort orders them by start (it is stable and equal
//     starts leave the kernel in end order, so the last record of a run of equal starts is the longest) and the greedy pass of
//     kg_greedy.hip (kWalkAlt) takes the longest record of each visited start and consumes its length.  One window only.
//   -c: every owned hit moves to the common coordinate start + Lmax - 1, that is up by Lmax - L < 16 places: the low 16 bits of
//     the shifted mask stay in the lane, the spill goes to the next lane (lane 63's to a scalar for the next cell; a unit rebuilds
//     it from the 16 bytes in front of it: an occurrence that spills out of them starts inside them).  From there on the newline
//     mask shifted by Lmax - 1, the line-state arithmetic and the info words are the shared ones (RxLineCarry, rx_unit_end).
// Line anchors (krep_gpu_regex_compile_ext: ^(ERROR|WARN), (jpg|png)$, and what ?, {n,m} and inner groups expand into): the
// instantiations with ANCH.  Every branch gets the place { '\n' } in front of (^) and / or behind ($) its classes, so branch i takes
// Lx_i = L_i + bol + eol bits and everything above holds with the places Lx in the role of the lengths: the lookback is Lxmax - 1
// <= 15 bytes, a hit of Lx places behind byte e is the occurrence (e + 1 - Lx + bol, e + 1 - eol), the common coordinate of -c is
// start + Lmax - 1 + eol.  Two newlines stand in no buffer: the one in front of byte 0 of the text is the entry state INIT of the unit
// at coordinate 0, the one behind the last byte is OR-ed into the one lane of a guarded load that holds offset text_len, in a
// case-sensitive search only (so with $ the coordinates reach text_len: one more cell or unit when the length is a multiple of
// one).  Neither is a newline of -c.  Sets without anchors run the instantiations without ANCH: the code they always ran.
// The anchor-byte fast path of kg_regex.hip is not taken: DESIGN §4.9 measured no gain from it on sparse text.
// Reads: no byte outside [0, text_len) — whole 8-KiB rounds inside the text are vector loads, everything else is guarded per byte.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/krep_gpu.h"
#include "kg_common.h"
#include "kg_device.h"
#include "kg_internal.h"
#include "kg_plan.h"
#include "kg_regex_dev.h"

namespace kg {

struct RaArgs
{
    const uint8_t *text;
    u64 text_len;
    u64 anchor;         // grid origin: a multiple of 16, <= own_lo
    u64 own_lo, own_hi; // starts in [own_lo, own_hi) are owned (own_hi <= text_len); -c: so are the newlines of these bytes
    u64 cov_hi;         // ends (-c: coordinates start + Lmax - 1) >= cov_hi hold nothing
    u64 n_units;
    u64 global_base;
    u32 init, fin;
    // One word for the geometry (every further uniform value costs scalar registers):
    //   bits 0-7  Lxmax: the places of the longest branch, Lmax + bol + eol (the lookback of the exit state is Lxmax - 1 bytes)
    //   bit 8     cross_overlap
    //   bit 9     bol, bit 10 eol: every branch has the place { '\n' } in front of / behind its classes (anchored instantiations only)
    //   bit 11    the entry state of the unit at coordinate 0 is INIT: ^ and the buffer begins the text
    //   bit 12    a guarded load holds '\n' at offset text_len: $ in the buffer that ends the text (not under -i)
    u32 geom;
    const u32 *table;
    RxOut o;            // what the window driver sets (kg_regex_dev.h)
};

static __device__ __forceinline__ u32 ra_byte(const uint4 &d, int i)
{
    const u32 w = (i >> 2) == 0 ? d.x : (i >> 2) == 1 ? d.y : (i >> 2) == 2 ? d.z : d.w;
    return (w >> (8 * (i & 3))) & 0xffu;
}
// the state behind a lane's 16 bytes, exact in bits 0 .. Lmax - 2 of every branch: bytes `first` = 17 - Lmax .. 15 from all-ones
static __device__ __forceinline__ u32 ra_exit(const u32 *T, const uint4 &d, u32 init, u32 first)
{
    u32 S = 0xffffffffu;
#pragma unroll
    for (int i = 1; i < 16; ++i)
        if ((u32)i >= first)
            S = ((S << 1) | init) & T[ra_byte(d, i) << 5];
    return S;
}
// the walk from the true entry state E: bit k of the result = some branch ends behind byte k
static __device__ __forceinline__ u32 ra_walk(const u32 *T, const uint4 &d, u32 init, u32 fin, u32 E)
{
    u32 S = E, H = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i)
    {
        S = ((S << 1) | init) & T[ra_byte(d, i) << 5];
        H |= ((S & fin) != 0u ? 1u : 0u) << i;
    }
    return H;
}
// the same walk again for a lane that holds hits: f(k, L) for every branch that ends behind a byte k of H, L its places
template <class F> static __device__ __forceinline__ void ra_hits(const u32 *T, const uint4 &d, u32 init, u32 fin, u32 E, u32 H, F &&f)
{
    u32 S = E;
#pragma unroll
    for (int i = 0; i < 16; ++i)
    {
        if ((H >> i) == 0u)
            break;
        S = ((S << 1) | init) & T[ra_byte(d, i) << 5];
        if ((H >> i) & 1u)
        {
            u32 fm = S & fin;
            while (fm)
            {
                const u32 fb = (u32)__builtin_ctz(fm);
                fm &= fm - 1u;
                const u32 o = 31u - (u32)__clz((int)(init & ((2u << fb) - 1u))); // the branch's lowest bit
                f((u32)i, fb - o + 1u);
            }
        }
    }
}
// the (end, branch) pairs of a lane whose occurrence starts in [own_lo, own_hi): the unit both launches count.  A hit of Lx places
// behind byte k starts at q + k + 1 - Lx + bol: the ^ place lies in front of the start.
template <bool ANCH>
static __device__ __forceinline__ u32 ra_count_lane(const u32 *T, const uint4 &d, const RaArgs &a, u32 E, u32 H, u64 q, bool all_owned)
{
    if (all_owned)
        return (u32)__popc(H); // (no two occurrences share a byte: one pair per end)
    const u32 bol = ANCH ? (a.geom >> 9) & 1u : 0u;
    u32 c = 0;
    if (H)
        ra_hits(T, d, a.init, a.fin, E, H, [&](u32 k, u32 L) {
            const u64 s = q + k + 1u + bol - L;
            c += (s >= a.own_lo && s < a.own_hi) ? 1u : 0u;
        });
    return c;
}
// -c: the owned hits of a lane at the common coordinate (the end a branch of Lmax places would have), relative to q (bits 16..30: the
// spill into the next lane)
template <bool ANCH>
static __device__ __forceinline__ u32 ra_starts(const u32 *T, const uint4 &d, const RaArgs &a, u32 E, u32 H, u64 q, u32 Lmax)
{
    const u32 bol = ANCH ? (a.geom >> 9) & 1u : 0u;
    u32 M = 0;
    if (H)
        ra_hits(T, d, a.init, a.fin, E, H, [&](u32 k, u32 L) {
            const u64 s = q + k + 1u + bol - L;
            if (s >= a.own_lo && s < a.own_hi)
                M |= 1u << (k + Lmax - L);
        });
    return M;
}

// ANCH: the branches stand between line anchors (krep_gpu_regex_compile_ext); without it the code is the unanchored alternation's
template <int MODE, bool ANCH>
__global__ __launch_bounds__(kBlock) void regex_alt_scan(const RaArgs a)
{
    constexpr bool LINES = MODE == kRxLines, EMIT = MODE == kRxEmit;
    __shared__ u32 s_T[256 * 32];
    rx_fill_table(s_T, a.table);
    const u32 lane = lane_id(), wave = threadIdx.x >> 6;
    const u32 *T = s_T + (lane & 31u);
    // Lmax: the places of the longest branch; a start p is seen, or for -c put, at coordinate p + sh = p + Lmax - 1 - bol
    const u32 bol = ANCH ? (a.geom >> 9) & 1u : 0u, eol = ANCH ? (a.geom >> 10) & 1u : 0u;
    const u32 Lmax = a.geom & 0xffu, sh = Lmax - 1u - bol, first = 17u - Lmax;
    const bool cross = ((a.geom >> 8) & 1u) != 0u;
    const bool eot = ANCH && ((a.geom >> 12) & 1u) != 0u;
    const u64 end_hi = ANCH ? a.text_len + (eot ? 1u : 0u) : a.text_len; // an end is a byte of the text, or the newline behind it
    const u64 in_lo = a.own_lo + sh; // a cell of ends in [in_lo, own_hi) owns every occurrence that ends in it
    const u64 n_waves = (u64)gridDim.x * kWavesPerBlk;
    u64 acc_total = 0;

    for (u64 unit = (u64)blockIdx.x * kWavesPerBlk + wave; unit < a.n_units; unit += n_waves)
    {
        const u64 ubase = a.anchor + unit * kRxUnitBytes;
        // the 16 bytes in front of the unit give lane 0 its entry state and, for -c, the spill and the newlines that shift into the unit
        u32 x63 = 0; // exit state of the 16 bytes in front of the next cell (uniform)
        u32 y63 = 0; // -c: their spill | their raw newline mask << 16 (uniform)
        if constexpr (ANCH)
            x63 = ((a.geom >> 11) & 1u) != 0u ? a.init : 0u; // ^: the newline in front of byte 0 of the text
        if (ubase != 0)
        {
            const u64 pq = ubase - 16u;
            uint4 p = rx_load_guarded(a.text, a.text_len, pq);
            if constexpr (ANCH)
                if (eot)
                    rx_put_eot(p, pq, a.text_len);
            x63 = __builtin_amdgcn_readfirstlane(ra_exit(T, p, a.init, first));
            if (LINES)
            {
                // (an occurrence whose coordinate start + sh lies in the unit and whose end does not starts behind the first of these 16
                //  bytes, its ^ place inside them: the entry state of the walk does not reach it)
                const u32 Hp = ra_walk(T, p, a.init, a.fin, 0u) & rx_range(pq, 0, end_hi);
                const u32 M = ra_starts<ANCH>(T, p, a, 0u, Hp, pq, Lmax);
                y63 = __builtin_amdgcn_readfirstlane((M >> 16) | ((rx_newlines(p) & rx_range(pq, a.own_lo, a.own_hi)) << 16));
            }
        }
        u32 l_hits = 0;                           // per lane
        u64 out_idx = EMIT ? a.o.offsets[unit] : 0; // uniform
        RxLineCarry lc;                           // -c: the line state of the unit

        for (int r = 0; r < kRoundsBig; ++r)
        {
            const u64 seg = ubase + (u64)r * kSegBytes;
            if (seg >= a.cov_hi)
                break;
            const bool fast = seg + kSegBytes <= a.text_len;
            uint4 d[kCells];
            rx_load_round(d, a, seg, lane, fast, eot);
#pragma unroll
            for (int j = 0; j < kCells; ++j)
            {
                const u64 cbase = seg + (u64)j * kCellBytes;
                if (cbase >= a.cov_hi)
                    break;
                const u64 q = cbase + (u64)lane * 16u;
                const u32 X = ra_exit(T, d[j], a.init, first);
                u32 E = __shfl_up(X, 1);
                if (lane == 0)
                    E = x63;
                x63 = __builtin_amdgcn_readlane(X, 63);
                u32 H = ra_walk(T, d[j], a.init, a.fin, E);
                if (!fast)
                    H &= rx_range(q, 0, end_hi);
                if (LINES)
                {
                    const u32 M = ra_starts<ANCH>(T, d[j], a, E, H, q, Lmax);
                    const u32 mine = (M >> 16) | ((rx_newlines(d[j]) & rx_range(q, a.own_lo, a.own_hi)) << 16);
                    u32 prev = __shfl_up(mine, 1);
                    if (lane == 0)
                        prev = y63;
                    y63 = __builtin_amdgcn_readlane(mine, 63);
                    const u32 Hc = (M | prev) & 0xffffu; // the owned starts at coordinates q .. q + 15
                    l_hits += (u32)__popc(Hc);
                    lc.lane16(Hc, mine >> 16, prev >> 16, sh);
                }
                else if (__ballot(H != 0u))
                {
                    const bool all_owned = !cross && cbase >= in_lo && cbase + kCellBytes <= a.own_hi;
                    const u32 c = ra_count_lane<ANCH>(T, d[j], a, E, H, q, all_owned);
                    l_hits += c;
                    if (EMIT)
                    {
                        const u32 incl = rx_wave_incl(c, lane);
                        if (c)
                        {
                            u64 idx = out_idx + (incl - c);
                            ra_hits(T, d[j], a.init, a.fin, E, H, [&](u32 k, u32 L) {
                                const u64 s = q + k + 1u + bol - L;
                                if (s >= a.own_lo && s < a.own_hi)
                                {
                                    if (idx < a.o.pos_cap)
                                    {
                                        const u64 s0 = s + a.global_base;
                                        rx_store_record(a.o.positions, idx, s0, s0 + (L - bol - eol));
                                    }
                                    ++idx;
                                }
                            });
                        }
                        out_idx += (u32)__builtin_amdgcn_readlane(incl, 63);
                    }
                }
            }
        }
        if (EMIT)
            continue;
        acc_total += rx_unit_end<LINES>(l_hits, lc, a.o.unitinfo, unit, lane);
    }
    if (!EMIT && lane == 0 && acc_total)
        atomicAdd(&a.o.ctr->total, acc_total);
}

template <int MODE> static hipError_t ra_launch(const RaArgs &a, int num_cu, hipStream_t st)
{
    // (32 KiB of LDS each would let five workgroups into a CU, but the kernel holds 112 to 126 VGPRs: four waves per SIMD, four workgroups)
    return ((a.geom >> 9) & 3u) ? rx_launch_grid(regex_alt_scan<MODE, true>, a, a.n_units, num_cu, 4, st)
                                : rx_launch_grid(regex_alt_scan<MODE, false>, a, a.n_units, num_cu, 4, st);
}
static hipError_t ra_run(const RaArgs &a, int mode, int num_cu, hipStream_t st)
{
    return mode == kRxLines ? ra_launch<kRxLines>(a, num_cu, st) : mode == kRxEmit ? ra_launch<kRxEmit>(a, num_cu, st) : ra_launch<kRxCount>(a, num_cu, st);
}

// ------------------------------------------------------------------------------------------------ the scan of a window
int scan_regex_alt(krep_gpu_plan *pl, const Window &w, match_position_t *d_pos, uint64_t cap, hipStream_t st, int time_it,
                   krep_gpu_scan_out_t *out)
{
    const RegexProg &rx = *pl->rx;
    const u32 Lmax = rx.alt.Lmax, bol = rx.alt_bol, eol = rx.alt_eol;
    u32 lens[8]; // (n_branches <= 8, include/krep_gpu.h)
    for (u32 i = 0; i < rx.alt.n_branches; ++i)
        lens[i] = rx.alt.branch[i].L;
    RxSpec sp{};
    sp.lens = lens; sp.n_lens = rx.alt.n_branches; sp.Lmin = rx.alt.Lmin;
    sp.bol = bol; sp.eol = eol;
    sp.overlap = rx.alt.cross_overlap;
    sp.one_window = "two occurrences of this regex alternation can overlap, its matches are the greedy selection over the whole occurrence "
                    "list: scan the whole text in one window (krep_gpu_split_mode() == KREP_GPU_SPLIT_WHOLE)";
    // every (end, branch) pair ordered by start: the longest record of a visited start is the match, consume = its own length
    sp.walk.mode = kWalkAlt; sp.walk.m = Lmax;
    sp.sort = true;
    RxWindow g;
    if (const int rc = rx_window(pl, w, d_pos, cap, sp, &g); rc || g.empty)
        return rc;

    RaArgs a{};
    a.text = w.d_text; a.text_len = w.text_len;
    a.anchor = w.own_lo & ~(u64)15;
    a.own_lo = w.own_lo; a.own_hi = g.own_hi;
    const u32 sh = Lmax - 1 + eol; // a start p is seen at p + L_i - 1 + eol and, for -c, put at p + sh
    a.cov_hi = g.lines ? g.own_hi + sh : std::min<u64>(g.own_hi + sh, w.text_len + g.eot); // (with $ this reaches text_len + 1)
    a.n_units = (a.cov_hi - a.anchor + kRxUnitBytes - 1) / kRxUnitBytes;
    a.global_base = w.global_base;
    a.init = rx.init; a.fin = rx.fin;
    a.geom = (Lmax + bol + eol) | ((rx.alt.cross_overlap ? 1u : 0u) << 8) | (bol << 9) | (eol << 10) | (g.entry0 << 11) | (g.eot << 12);
    a.table = rx.d_table;
    return rx_drive(pl, w, sp, g, d_pos, cap, st, time_it, &a.o, a.n_units,
                    [&](int mode) { return ra_run(a, mode, pl->num_cu, st); }, out);
}
} // namespace kg
