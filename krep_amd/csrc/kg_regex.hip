// kg_regex.hip — krep -E for fixed-length class sequences (include/krep_gpu.h, krep_gpu_regex_compile): the six exported pattern
// compilers (kg_regex_compile.h, one body), the bit-parallel shift-and scan kernel and its scan kg::scan_regex.  An alternation of such
// sequences (krep_gpu_regex_compile_alt, and what krep_gpu_regex_compile_ext expands into one, line anchors included) has its own
// kernel and scan in kg_regex_alt.hip, a line walk (krep_gpu_regex_compile_loops, _groups) in kg_regex_loops.hip: regex_prog_create
// makes the program of each of the three kinds here (the tables are kg_regex_compile.h's), scan_regex hands over.
// Both scans go through the one window driver of this file (rx_window: the window checks and refusals; rx_drive: the launches, the
// greedy pass, the read-back and the krep_gpu_scan_out_t), and both kernels are built around their walk from the device helpers of
// kg_regex_dev.h (table fill, round loader, -c line state, record store, unit end, grid).
//
// The kernel.  T[byte] is a 16-bit mask, bit j set when byte is in class Cj.  It sits in LDS once per bank (entry b of copy k at
// dword b * 32 + k, a lane reads copy lane % 32), so the 64 lookups of a wave instruction never meet in a bank whatever the
// text holds.  A lane takes 16 bytes and runs S = ((S << 1) | 1) & T[b] over them from the optimistic state 0xFFFF.  Because
// L <= 16 its EXIT state is exact from its own bytes; one cross-lane move hands it to the next lane as that lane's true entry
// state E (lane 0: the exit of lane 63 of the cell before, kept in a scalar).  The optimistic walk already knows everything
// about a match that ends at the lane's byte k except the part in front of the lane: for k >= L - 1 nothing is in front, for
// k < L - 1 the match is real iff bit L - 2 - k of E is set.  So the hits are H & ((0xFFFF << (L-1)) | reverse(E's low L-1 bits)):
// one walk, no second pass over the bytes.
// Coordinates: a match is seen at its END byte e = start + L - 1, so the whole kernel works in end coordinates: start s is at
// coordinate s + L - 1, and for -c a newline at byte n is put at coordinate n + L - 1 as well (its mask shifted across the lane
// boundary the same way).  Ownership is by START in [own_lo, hi_match); a unit is 32 KiB of coordinates, units are contiguous
// and in order, so their info words compose in kg_post.hip like those of every other scan.
// Anchor fast path (patterns whose smallest class holds 1..4 bytes, no -c): a cell is walked only when it or the cell in front of
// it holds an anchor byte (a match that ends in the cell has its anchor byte in one of the two); after skipped cells the entry
// state of lane 0 is rebuilt from the 16 bytes in front of the cell (kept in scalars), once.
// Line anchors (krep_gpu_regex_compile_anchored).  ^ and $ are one more place each in the sequence, the class { '\n' }: the walk runs
// over the EXTENDED sequence [\n] C0..C(L-1) [\n] of Lx = L + bol + eol <= 16 places, so the 16-bit state, the exact exit state and the
// entry-state mask hold with Lx in place of L.  Two shifts follow from it: a hit is seen at the extended end, text byte
// p + L - 1 + eol, so a START p is at coordinate p + sh with sh = L - 1 + eol (not Lx - 1: the ^ place lies in front of p), and that
// is the shift of the -c newline mask, of the ownership range and of the records.  Two newlines exist in no buffer: the one in front
// of byte 0 of the text (global_base == 0) is the entry state 1 of unit 0 instead of 0, the one behind the last byte is OR-ed into
// the lane of a guarded round that holds offset text_len when the buffer ends the text and the search is case-sensitive (so with
// $ the coordinates reach text_len itself: one more cell, round or unit when text_len is a multiple of one).  Neither is a
// newline of -c.  The anchor bytes come from the real classes, and the cell behind one that holds them is always walked: the
// cell that holds nothing but the newline behind the text is reached that way.
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
#include "kg_regex_compile.h"
#include "kg_regex_dev.h"

namespace kg {

struct RxArgs
{
    const uint8_t *text;
    u64 text_len;
    u64 anchor;          // grid origin: a multiple of 16, <= own_lo
    u64 own_lo, hi_match; // starts in [own_lo, hi_match) are matches; hi_match + L - 1 <= text_len
    u64 nl_hi;           // -c: the newlines of bytes [own_lo, nl_hi) take part (nl_hi <= text_len)
    u64 cov_hi;          // coordinates >= cov_hi hold nothing
    u64 n_units;
    u64 global_base;
    // One word for the geometry (the kernels run at the limit of their scalar registers: every further uniform value is spilled):
    //   bits 0-7   L: the real classes, a record is (p, p + L)
    //   bits 8-15  Lx: places of the walk, L + bol + eol
    //   bits 16-23 sh: start p is at coordinate p + sh, L - 1 + eol
    //   bit 24     entry state of the unit at coordinate 0: 1 when ^ and the buffer begins the text, else 0
    //   bit 25     a guarded round holds '\n' at offset text_len: $ in the buffer that ends the text (not under -i)
    u32 geom;
    u32 n_anchor;
    u32 ab[4];           // the anchor bytes, each in every byte lane
    const u32 *table;
    RxOut o;             // what the window driver sets (kg_regex_dev.h)
};

// the optimistic walk over a lane's 16 bytes: bit k of the result = bit L-1 of the state behind byte k; X = the exit state
static __device__ __forceinline__ u32 rx_walk(const u32 *T, const uint4 &d, u32 Lm1, u32 &X)
{
    const u32 w[4] = {d.x, d.y, d.z, d.w};
    u32 S = 0xffffu, H = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i)
    {
        const u32 b = (w[i >> 2] >> (8 * (i & 3))) & 0xffu;
        S = ((S << 1) | 1u) & T[b << 5];
        H = (H >> 1) | ((S >> Lm1) << 31);
    }
    X = S;
    return H >> 16;
}
template <bool ANCH, bool LINES, bool EMIT>
__global__ __launch_bounds__(kBlock) void regex_scan(const RxArgs a)
{
    static_assert(!(ANCH && LINES) && !(LINES && EMIT), "-c walks every cell and writes no records");
    __shared__ u32 s_T[256 * 32];
    rx_fill_table(s_T, a.table);
    const u32 lane = lane_id(), wave = threadIdx.x >> 6;
    const u32 *T = s_T + (lane & 31u);
    const u32 Lm1 = ((a.geom >> 8) & 0xffu) - 1u, sh = (a.geom >> 16) & 0xffu;

    const u64 c_lo = a.own_lo + sh, c_hi = a.hi_match + sh; // the coordinates of the owned starts
    const u64 n_waves = (u64)gridDim.x * kWavesPerBlk;
    u64 acc_total = 0;

    for (u64 unit = (u64)blockIdx.x * kWavesPerBlk + wave; unit < a.n_units; unit += n_waves)
    {
        const u64 ubase = a.anchor + unit * kRxUnitBytes;
        // the 16 bytes in front of the unit give lane 0 its entry state (and, for -c, the newlines that shift into the unit)
        u32 x63 = (a.geom >> 24) & 1u; // exit state | raw newline mask << 16 of the 16 bytes in front of the next cell (uniform)
        if (ubase != 0)
        {
            const uint4 p = rx_load_guarded(a.text, a.text_len, ubase - 16); // (ubase <= text_len: the newline behind the text is not among them)
            u32 X;
            (void)rx_walk(T, p, Lm1, X);
            x63 = X;
            if (LINES)
                x63 |= (rx_newlines(p) & rx_range(ubase - 16, a.own_lo, a.nl_hi)) << 16;
            x63 = __builtin_amdgcn_readfirstlane(x63);
        }
        bool have_state = true, prev_anch = true; // ANCH: x63 is valid | the cell in front holds an anchor byte (unknown: yes)
        u32 p63[4] = {0, 0, 0, 0};                // ANCH: lane 63's bytes of the last skipped cell
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
            rx_load_round(d, a, seg, lane, fast, ((a.geom >> 25) & 1u) != 0u);
#pragma unroll
            for (int j = 0; j < kCells; ++j)
            {
                const u64 cbase = seg + (u64)j * kCellBytes;
                if (cbase >= a.cov_hi)
                    break;
                const u64 q = cbase + (u64)lane * 16u;
                bool anch = true;
                if (ANCH)
                {
                    u32 f = 0;
                    for (u32 i = 0; i < a.n_anchor; ++i)
                        f |= eq_bytes(d[j].x, a.ab[i]) | eq_bytes(d[j].y, a.ab[i]) | eq_bytes(d[j].z, a.ab[i]) | eq_bytes(d[j].w, a.ab[i]);
                    anch = __ballot(f != 0u) != 0ull;
                    if (!anch && !prev_anch)
                    {
                        // no match ends here: keep only what the next walked cell needs for its entry state
                        have_state = false;
                        p63[0] = __builtin_amdgcn_readlane(d[j].x, 63);
                        p63[1] = __builtin_amdgcn_readlane(d[j].y, 63);
                        p63[2] = __builtin_amdgcn_readlane(d[j].z, 63);
                        p63[3] = __builtin_amdgcn_readlane(d[j].w, 63);
                        prev_anch = false;
                        continue;
                    }
                    if (!have_state)
                    {
                        u32 X;
                        (void)rx_walk(T, make_uint4(p63[0], p63[1], p63[2], p63[3]), Lm1, X);
                        x63 = __builtin_amdgcn_readfirstlane(X);
                        have_state = true;
                    }
                    prev_anch = anch;
                }
                u32 X;
                u32 H = rx_walk(T, d[j], Lm1, X);
                u32 mine = X;
                if (LINES)
                    mine |= (rx_newlines(d[j]) & rx_range(q, a.own_lo, a.nl_hi)) << 16;
                u32 prev = __shfl_up(mine, 1);
                if (lane == 0)
                    prev = x63;
                x63 = __builtin_amdgcn_readlane(mine, 63);
                const u32 E = prev & 0xffffu;
                H &= (0xffffu << Lm1) | (Lm1 ? (__brev(E) >> (32u - Lm1)) : 0u);
                if (!(cbase >= c_lo && cbase + kCellBytes <= c_hi))
                    H &= rx_range(q, c_lo, c_hi);
                l_hits += (u32)__popc(H);
                if (LINES)
                    lc.lane16(H, mine >> 16, prev >> 16, sh);
                if (EMIT)
                {
                    if (__ballot(H != 0u))
                    {
                        const u32 c = (u32)__popc(H), incl = rx_wave_incl(c, lane);
                        u64 idx = out_idx + (incl - c);
                        while (H)
                        {
                            const u32 k = (u32)__builtin_ctz(H);
                            H &= H - 1u;
                            if (idx < a.o.pos_cap)
                            {
                                const u64 s0 = q + k - sh + a.global_base;
                                rx_store_record(a.o.positions, idx, s0, s0 + (a.geom & 0xffu));
                            }
                            ++idx;
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

template <bool ANCH, bool LINES, bool EMIT> static hipError_t rx_launch(const RxArgs &a, int num_cu, hipStream_t st)
{
    return rx_launch_grid(regex_scan<ANCH, LINES, EMIT>, a, a.n_units, num_cu, 5, st); // 32 KiB of LDS each: five workgroups fit a CU
}
static hipError_t rx_run(const RxArgs &a, int mode, int num_cu, hipStream_t st)
{
    if (mode == kRxLines)
        return rx_launch<false, true, false>(a, num_cu, st);
    const bool emit = mode == kRxEmit;
    if (a.n_anchor)
        return emit ? rx_launch<true, false, true>(a, num_cu, st) : rx_launch<true, false, false>(a, num_cu, st);
    return emit ? rx_launch<false, false, true>(a, num_cu, st) : rx_launch<false, false, false>(a, num_cu, st);
}

// ------------------------------------------------------------------------------------------------ plan side
// The program of a plan: what the compilers said (kg_regex_compile.h, which also builds the tables) and its table on the device
static RegexProg *rx_upload(RegexProg *rx, const u32 table[256])
{
    if (hipMalloc(&rx->d_table, 256 * sizeof(u32)) != hipSuccess ||
        hipMemcpy(rx->d_table, table, 256 * sizeof(u32), hipMemcpyHostToDevice) != hipSuccess)
    {
        fail("regex plan: device allocation failed");
        regex_prog_free(rx);
        return nullptr;
    }
    return rx;
}
// the program of an alternation between line anchors: a search's, or with neither anchor the filter of a line walk (kg_regex_loops.hip)
RegexProg *regex_prog_create_alt(const krep_gpu_regex_alt_t &alt, u32 bol, u32 eol)
{
    auto *rx = new RegexProg();
    u32 table[256];
    rx->kind = RegexCompiled::kAlt;
    rx->alt = alt;
    rx->alt_bol = bol;
    rx->alt_eol = eol;
    rx_alt_table(alt, bol, eol, table, &rx->init, &rx->fin);
    return rx_upload(rx, table);
}
RegexProg *regex_prog_create(const search_params_t &sp)
{
    RegexCompiled rc;
    if (const char *why = regex_compile_cached(&sp, &rc))
    {
        fail("%s", why);
        return nullptr;
    }
    if (rc.kind == RegexCompiled::kAlt)
        return regex_prog_create_alt(rc.alt, rc.alt_bol ? 1u : 0u, rc.alt_eol ? 1u : 0u);
    auto *rx = new RegexProg();
    rx->kind = rc.kind;
    if (rc.kind == RegexCompiled::kWalk)
    { // test hook (krep_gpu_debug_force_regex_general, with both switches on): a loops program through the general step
        const bool force = !rc.walk.general && g_rl_force_general.load() && g_regex_loops.load(std::memory_order_relaxed) &&
                           g_regex_groups.load(std::memory_order_relaxed);
        rx->walk = force ? regex_walk_as_general(rc.walk) : rc.walk;
        return rx_upload(rx, rx->walk.table);
    }
    u32 table[256];
    rx->info = rc.seq;
    rx_seq_table(rc.seq, table);
    return rx_upload(rx, table);
}
void regex_prog_free(RegexProg *rx)
{
    if (!rx)
        return;
    rx_loops_work_free(rx->work);
    if (rx->d_table) (void)hipFree(rx->d_table);
    delete rx;
}

// ------------------------------------------------------------------------------------------------ the window driver of both scans
int rx_window(const krep_gpu_plan *pl, const Window &w, const match_position_t *d_pos, uint64_t cap, const RxSpec &sp, RxWindow *g)
{
    *g = RxWindow{};
    g->empty = true;
    if (w.global_len < sp.Lmin || w.text_len < sp.Lmin || w.own_lo >= w.own_hi)
        return 0; // (text_len == 0 included: no occurrence is empty)
    g->own_hi = std::min(w.own_hi, w.text_len);
    g->hi_match = std::min<u64>(g->own_hi, w.text_len - sp.Lmin + 1);
    g->lines = pl->lines;
    g->greedy = sp.overlap && !g->lines;
    const bool whole = w.global_base == 0 && w.own_lo == 0 && g->own_hi + sp.Lmin > w.text_len && w.global_len == w.text_len;
    if (g->greedy && !whole)
        return fail("%s", sp.one_window);
    if (g->own_hi <= w.own_lo || (!g->lines && g->hi_match <= w.own_lo))
        return 0;
    // an anchor needs the byte in front of, or behind, every occurrence the window owns
    const bool ends_text = w.global_base + w.text_len == w.global_len;
    if (sp.bol && w.own_lo == 0 && w.global_base > 0)
        return fail("regex with ^: the window owns buffer byte 0, which is not the start of the text (global_base > 0), and the byte in "
                    "front of it decides a match there: start the buffer at least one byte in front of own_lo");
    if (sp.eol && !ends_text)
        for (u32 i = 0; i < sp.n_lens; ++i)
            if (const u32 L = sp.lens[i]; w.own_lo + L <= w.text_len && g->own_hi + L > w.text_len)
                return fail("regex with $: the window owns a start whose occurrence ends on the last byte of a buffer that does not end the "
                            "text, and the byte behind it decides the match: end own_hi at least L bytes in front of the buffer's end");
    g->empty = false;
    g->entry0 = sp.bol && w.global_base == 0 ? 1u : 0u;
    // (regex_search ORs REG_ICASE into regexec's eflags, where that bit is REG_NOTEOL: under -i the end of the text ends no line)
    g->eot = sp.eol && ends_text && pl->sp.case_sensitive ? 1u : 0u;
    g->want = (d_pos && cap && !g->lines && pl->track) ? std::min<u64>(pl->max_count, cap) : 0;
    return 0;
}

int rx_drive(krep_gpu_plan *pl, const Window &w, const RxSpec &sp, const RxWindow &g, match_position_t *d_pos, uint64_t cap, hipStream_t st,
             int time_it, RxOut *o, u64 n_units, const std::function<hipError_t(int)> &launch, krep_gpu_scan_out_t *out)
{
    const bool lines = g.lines, greedy = g.greedy;
    const u64 want = g.want;
    o->ctr = pl->d_ctr;
    HIPCHK(hipSetDevice(pl->device));
    if (time_it) HIPCHK(hipEventRecord(pl->ev0, st));
    const bool chain = lines || want || greedy;
    PostScratch &post = pl->post;
    if (chain)
    {
        if (post_reserve(post, n_units, 0))
            return 2;
        o->unitinfo = post.d_unitinfo;
        o->offsets = (const u64 *)post.d_offsets;
    }
    HIPCHK(hipMemsetAsync(pl->d_ctr, 0, sizeof(Counters), st));
    HIPCHK(launch(lines ? kRxLines : kRxCount));
    if (pl->rx_emit_limit)
    { // an inner scan of kg_regex_loops.hip: a text that holds more occurrences than its caller has room for gets the number alone
        HIPCHK(hipMemcpyAsync(pl->h_ctr, pl->d_ctr, sizeof(Counters), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (pl->h_ctr->total > pl->rx_emit_limit)
        {
            out->total_matches = pl->h_ctr->total;
            return 0;
        }
    }
    if (chain && post_offsets_pass(post, n_units, lines, pl->d_ctr, st))
        return 2;
    uint64_t total = 0, nlines = 0;
    unsigned long long summary = 0;
    if (greedy)
    {
        // all occurrences into post.d_occ (sized once their number is known; an alternation's in start order), then the greedy pass
        // of kg_greedy.hip
        HIPCHK(hipMemcpyAsync(pl->h_ctr, pl->d_ctr, sizeof(Counters), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        const uint64_t n_occ = pl->h_ctr->total;
        HIPCHK(grow_scratch(post.occ_cap, n_occ, n_occ, {dev_buf(post.d_occ, n_occ * 2 * sizeof(uint64_t))}));
        if (n_occ)
        {
            o->positions = (u64 *)post.d_occ;
            o->pos_cap = n_occ;
            HIPCHK(launch(kRxEmit));
            if (sp.sort && order_records((match_position_t *)post.d_occ, n_occ, w.global_base + w.text_len + 1, st, false))
                return 2;
            HIPCHK(hipMemsetAsync(pl->d_ctr, 0, sizeof(Counters), st));
            if (const int rc = post_walk(post, w.d_text, w.text_len, w.global_base, sp.walk, n_occ, (uint64_t *)d_pos, want, pl->d_ctr,
                                         pl->h_ctr, st, &total, &nlines, nullptr))
                return rc;
        }
        summary = total ? (kLnHead | kLnTail) : 0;
    }
    else
    {
        if (want)
        {
            o->positions = (u64 *)d_pos;
            o->pos_cap = want;
            HIPCHK(launch(kRxEmit));
        }
        HIPCHK(hipMemcpyAsync(pl->h_ctr, pl->d_ctr, sizeof(Counters), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        total = pl->h_ctr->total;
        nlines = pl->h_ctr->lines;
        summary = lines ? pl->h_ctr->summary : (total ? (kLnHead | kLnTail) : 0);
    }
    if (time_it && stop_clock(pl, true, st, out))
        return 2;
    rx_fill_out(pl, lines, total, nlines, summary, d_pos, cap, want, out);
    return 0;
}
void rx_fill_out(const krep_gpu_plan *pl, bool lines, uint64_t total, uint64_t nlines, unsigned long long summary, const match_position_t *d_pos,
                 uint64_t cap, uint64_t want, krep_gpu_scan_out_t *out)
{
    out->total_matches = total;
    out->line_count = nlines;
    out->has_newline = (summary & kLnNl) != 0;
    out->head_line_hit = (summary & kLnHead) != 0;
    out->tail_line_hit = (summary & kLnTail) != 0;
    // regex_search's return value (krep.c:1395, :1533): max_count == 0 answers 0 with -c or positions, else 1 on the first occurrence
    const size_t maxc = pl->max_count;
    uint64_t store = 0;
    if (maxc == 0)
        out->count = (lines || pl->track) ? 0 : (total ? 1 : 0);
    else if (lines)
        out->count = std::min<uint64_t>(nlines, maxc);
    else
    {
        out->count = std::min<uint64_t>(total, maxc);
        store = (pl->track && d_pos) ? out->count : 0;
    }
    if (d_pos && cap && pl->track && !lines)
    {
        out->overflow = store > cap;
        out->stored = std::min<uint64_t>(store, std::min<uint64_t>(total, want));
    }
}

// ------------------------------------------------------------------------------------------------ the scan of a window
int scan_regex(krep_gpu_plan *pl, const Window &w, match_position_t *d_pos, uint64_t cap, hipStream_t st, int time_it,
               const krep_gpu_seq_carry_t *carry_in, krep_gpu_seq_carry_t *carry_out, krep_gpu_scan_out_t *out)
{
    memset(out, 0, sizeof *out);
    if (carry_out)
        *carry_out = carry_in ? *carry_in : krep_gpu_seq_carry_t{};
    if (!pl->rx)
        return fail("scan_device: the regex plan holds no program");
    if (pl->rx->kind == RegexCompiled::kWalk)
        return scan_regex_loops(pl, w, d_pos, cap, st, time_it, out);
    if (pl->rx->kind == RegexCompiled::kAlt)
        return scan_regex_alt(pl, w, d_pos, cap, st, time_it, out);
    const krep_gpu_regex_info_t &info = pl->rx->info.seq;
    const u32 L = info.L, bol = pl->rx->info.bol ? 1u : 0u, eol = pl->rx->info.eol ? 1u : 0u;
    RxSpec sp{};
    sp.lens = &L; sp.n_lens = 1; sp.Lmin = L;
    sp.bol = bol; sp.eol = eol;
    sp.overlap = info.self_overlap;
    sp.one_window = "this regex can overlap itself, its matches are the greedy selection over the whole occurrence list: scan the whole "
                    "text in one window (krep_gpu_split_mode() == KREP_GPU_SPLIT_WHOLE)";
    sp.walk.mode = kWalkGreedy; sp.walk.m = L; // consume = L
    RxWindow g;
    if (const int rc = rx_window(pl, w, d_pos, cap, sp, &g); rc || g.empty)
        return rc;

    RxArgs a{};
    a.text = w.d_text; a.text_len = w.text_len;
    a.anchor = w.own_lo & ~(u64)15;
    a.own_lo = w.own_lo; a.hi_match = std::max<u64>(g.hi_match, w.own_lo);
    a.nl_hi = g.own_hi;
    const u32 sh = L - 1 + eol;
    a.cov_hi = (g.lines ? g.own_hi : a.hi_match) + sh; // (with $ in the buffer that ends the text this reaches text_len + 1)
    a.n_units = (a.cov_hi - a.anchor + kRxUnitBytes - 1) / kRxUnitBytes;
    a.global_base = w.global_base;
    a.geom = L | ((L + bol + eol) << 8) | (sh << 16) | (g.entry0 << 24) | (g.eot << 25);
    a.n_anchor = g.lines ? 0 : info.n_anchor;
    for (u32 i = 0; i < 4; ++i)
        a.ab[i] = 0x01010101u * info.anchor_bytes[i < info.n_anchor ? i : 0];
    a.table = pl->rx->d_table;
    return rx_drive(pl, w, sp, g, d_pos, cap, st, time_it, &a.o, a.n_units,
                    [&](int mode) { return rx_run(a, mode, pl->num_cu, st); }, out);
}
// the body of every exported compiler: the compiler's reason is the error
template <class Out> static int rx_export(const char *(*compile)(const search_params_t *, Out *), const search_params_t *params, Out *out)
{
    krep_gpu_clear_error();
    if (const char *why = compile(params, out))
        return fail("%s", why);
    return 0;
}
} // namespace kg

extern "C" int krep_gpu_regex_compile(const search_params_t *p, krep_gpu_regex_info_t *out) { return kg::rx_export(kg::regex_compile, p, out); }
extern "C" int krep_gpu_regex_compile_anchored(const search_params_t *p, krep_gpu_regex_anchored_t *out) { return kg::rx_export(kg::regex_compile_anchored, p, out); }
extern "C" int krep_gpu_regex_compile_alt(const search_params_t *p, krep_gpu_regex_alt_t *out) { return kg::rx_export(kg::regex_compile_alt, p, out); }
extern "C" int krep_gpu_regex_compile_ext(const search_params_t *p, krep_gpu_regex_ext_t *out) { return kg::rx_export(kg::regex_compile_ext, p, out); }
extern "C" int krep_gpu_regex_compile_loops(const search_params_t *p, krep_gpu_regex_loops_t *out) { return kg::rx_export(kg::regex_compile_loops, p, out); }
extern "C" int krep_gpu_regex_compile_groups(const search_params_t *p, krep_gpu_regex_groups_t *out) { return kg::rx_export(kg::regex_compile_groups, p, out); }
