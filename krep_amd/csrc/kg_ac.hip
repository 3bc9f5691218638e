// kg_ac.hip — multi-pattern literal scan for gfx950, replacing aho_corasick_search
// (aho_corasick.c:299-466) behind the same search_func_t boundary.
//
// What the reference computes: for every text index i (ascending), every pattern that ENDS at i,
// longest first (it walks the goto/fail automaton and then the whole fail chain,
// aho_corasick.c:353-431), duplicates of a pattern string once per copy.  That set is a pure
// function of the bytes text[i-Lmax+1 .. i], so the sequential automaton walk is not needed to
// reproduce it.  MI355X-first formulation:
//   * FILTER (every byte): one bit table in LDS, indexed by the 5-bit classes (b & 31) of the last four bytes
//     (2^20 bits = 128 KiB; a pattern shorter than 4 bytes sets every class of the bytes in front of it).  A lane
//     turns its 20 bytes into a 100-bit class stream once; a position then costs a funnel shift, the dword address,
//     one ds_read_b32 and two shifts.  With STRIDE == 2 only the even positions are looked up (see below).
//     Positions whose bit is clear cannot end a pattern.  The haystack is read once with the same coalesced
//     16 B/lane loads as the literal scan, the next round streaming into the registers the current one vacates.
//   * VERIFY (candidates only, ~0.2 % of positions for 1000 random patterns): one candidate per lane, 64 at a time
//     from the unit's candidate bitmap in LDS.  The exact last 4 bytes select an entry of a sparse hash table that carries the
//     next <= 12 bytes of the reversed-trie chain and the depths at which patterns end (kg_ac_common.h); 1-3-byte
//     patterns are exact bitmap lookups.  Two dependent accesses per candidate; the level-by-level walk of the
//     REVERSED-pattern trie (edges in an open-addressing table, L2-resident) remains for what that cannot express.
//     The reference order (longest first at one end index) is the depth mask read from the top.
//   * ORDER: same as the literal kernel — unit-local ranks, staging slot, info word, post-pass.
// -w, -c (line counting), max_count and start-offset ownership are applied exactly as in the literal
// kernel.  A dense DFA in LDS is impossible for the benchmark set (8605 states x 256 x 2 B = 4.4 MB
// against 160 KiB), which is why the LDS holds the filter, not the automaton.
// The kernel below is the set-up, the ticket, unit and round loops, and calls; its stages are in kg_ac_scan_dev.h (AcWave: what a wave's
// stages share).  stage: in -> out [instantiations]
//   ac_round_before: text, have, carry -> the 4 bytes in front of the round, scalar [all]
//   ac_pair_round (ac_pair_issue, ac_pair_finish): the round in d[] -> cbits, 8 bits per lane-cell; the next round into d[] [stride 2 without -c]
//   ac_cell_round -> ac_filter_cell: the round in d[], windows -> cbits, 16 bits per lane-cell; nlmap [stride 1, -c]
//   ac_ragged_round -> ac_filter_cell: text bytes, bounds-checked -> cbits, nlmap [all: the round at the text's end]
//   ac_anchor_stage2 (ac_anchor_locate, _fetch, _gram, _pick, _mark): cbits, text windows, anchor buckets -> ebits [ANCH 1, 2]
//   ac_verify_ends: one END pair per lane -> counts, depth masks or the level walk's verdict [all]
//   ac_rank_and_emit (ac_emit_write): a verified batch -> staged words or final records, the -c hit bitmap, wcnt [all]
//   ac_pend_unit (ac_pend_flush, ac_pend_recount, ac_pend_pos): ebits, pend, npend, ucnt -> verify batches of 64 over the ticket's units [ANCH 1, 2]
//   ac_verify_count, ac_verify_batch: cbits -> the unit's candidate ranks; one verify batch of the kernel's loop [ANCH 0]
//   ac_unit_lines [-c]; ac_unit_info | ac_ticket_info | ac_ticket_unpark: bitmap, nlmap -> LineState; wcnt | ucnt | park_* -> info words, overflow report, parked stores
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <unordered_map>
#include <vector>

#include "../../include/krep_gpu.h"
#include "kg_ac_common.h"
#include "kg_ac_scan_dev.h"
#include "kg_ac_tables.h"
#include "kg_internal.h"

namespace kg {

// SHORT: the dictionary holds 1-3-byte patterns (wildcard-expanded in the filter table, exact bitmaps in the verifier).
// STRIDE == 2: the filter tests the EVEN text positions only.  The table then holds, besides every
// pattern's final 4-gram (a match ends at the tested position t), the 4-gram one byte earlier (the match ends at t + 1;
// for a 4-byte pattern that gram has an unknown first byte: all 32 classes are set).  Half the LDS lookups — the
// bank-conflict wall of 4.2 — and half the lookup VALU; a candidate verifies both ends, with both probes in flight.
// ANCH (round 6, kg_ac_anchor.hip; only with STRIDE == 2, no short patterns, no -c): the table holds rarity-chosen ANCHOR grams.
// A candidate's exact anchor gram names the offsets k at which patterns END behind it; those ends are marked in a second bitmap
// of the unit — same layout as the candidate bitmap: bit b <-> the END pair (2b + 1, 2b + 2), in the KiB that otherwise parks a
// ticket's stores — and the marked pairs, not the candidates, are what the end-anchored verifier looks at, in position order:
// ranking, staging and emission as before.
// ANCH == 2: the filter's index holds FIVE classes — the class of the byte in front of the 4-gram is multiplied out over the class
// fields of the pair register (ac_mix5) before the slot address is formed, three VALU per tested position — for dictionaries (almost)
// without patterns of 4 or 5 bytes: a 5-gram window of a word is several times rarer than its rarest 4-gram (kg_ac_anchor.hip).
template <bool CI, bool LINES, bool SHORT, int STRIDE, int ANCH = 0, bool WW = false>
__global__ __launch_bounds__(kAcBlock) void ac_scan_kernel(const AcArgs a)
{
    // WW: -w with the neighbour filter of the depth masks compiled in (stride-2 instantiations without short patterns).  A flag tested at run
    // time cost the plain scans 1.5-3 % — the filter's code in the verifier moved BASELINE config 4 from 6.27 to 6.38-6.46 ms in one process —
    // so the eight instantiations it applies to exist twice; every other instantiation sends -w through the level walk as before.
    static_assert(!WW || (STRIDE == 2 && !SHORT), "the -w filter of the depth masks: pair filter, no short patterns");
    static_assert(!ANCH || (STRIDE == 2 && !LINES && !SHORT), "anchored scan: pair filter, records / counts only");
    extern __shared__ __attribute__((aligned(16))) u32 s_mem[]; // filter table | per wave: candidate bitmap (+ hit and newline bitmaps for -c)
    const u32 lane = lane_id();
    const u32 wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if ((u32)(size_t)((__attribute__((address_space(3))) u32 *)s_mem) != 0u)
        __builtin_trap(); // the table lookups address LDS absolutely (no static __shared__ in this kernel)
    for (u32 w = threadIdx.x; w < a.filter_words; w += kAcBlock)
        s_mem[w] = a.filter[w];
    const u32 fw = (a.filter_words + 3u) & ~3u;
    constexpr u32 kPerWave = kAcBitmapWords + (LINES ? 2u * kAcBitmapWords : 0u); // candidate | hit | newline bitmaps
    constexpr bool PIPE = STRIDE == 2 && !LINES; // pair-layout table with the table reads software-pipelined over the cells of a round
    constexpr bool kPend = ac_pends(LINES, SHORT, STRIDE, ANCH);
    constexpr int kRoll = ac_roll_cells(LINES, STRIDE, ANCH);
    // PIPE: the pair filter only ever sets the even bits of a lane's 16-bit result, so it stores EIGHT bits per lane and cell
    // (bit q <-> tested position 2q + 1): the bitmap is 1 KiB, lane L owns 4 dwords, and the other KiB of the wave's bitmap
    // area parks the info words and staging slots of a ticket's units until the ticket's end (store
    // placement: the waves store nothing while they stream)
    AcWave wv;
    wv.cbits = s_mem + fw + wave * kPerWave;
    wv.park_slots = wv.cbits + 256;
    wv.park_info = reinterpret_cast<u64 *>(wv.cbits + 256 + kAcUnitsPerTicketMax * 16);
    wv.bitmap = wv.cbits + kAcBitmapWords;
    wv.nlmap = reinterpret_cast<unsigned short *>(wv.bitmap + kAcBitmapWords);
    wv.ebits = wv.cbits + 256;
    if (LINES)
        for (u32 w = lane; w < kAcBitmapWords; w += 64)
            wv.bitmap[w] = 0u;
    if (ANCH)
        *reinterpret_cast<uint4 *>(wv.ebits + lane * 4u) = make_uint4(0u, 0u, 0u, 0u);
    const bool want_pos = (a.flags & F_POS) != 0;
    const bool chain = want_pos || LINES;
    const bool emit_final = a.emit_mode != 0;

    u64 acc_total = 0;
    u32 acc_cand = 0; // (wave-uniform, an SGPR: a wave's share of a text holds far fewer than 2^32 tested positions)
    __syncthreads(); // filter tables are in LDS from here on; the waves never synchronise again

    // Waves are autonomous: each draws its own ticket for a.upt consecutive 16-KiB units (128 KiB on large texts:
    // ~25 fetch-adds/us on the single ticket word at 3 TB/s).  A per-tile workgroup barrier (one block per CU
    // because of the table) made every wave wait for the slowest verifier of its tile.
    for (;;)
    {
        const u64 tk = wave_fetch_add(&a.ctr->ticket, 1ull, lane);
        // (emit mode with a list: ticket k is the k-th unit that has to be scanned again — the launch no longer walks the info words of all
        //  units, one dependent load each: 0.7 ms per 8 GiB whenever a single unit had overflowed its slot)
        const bool listed = emit_final && a.redo_list != nullptr;
        if (listed && tk >= (u64)a.n_redo)
            break;
        const u64 u_begin = listed ? (u64)a.redo_list[tk] : tk * (u64)a.upt;
        if (u_begin >= a.num_tiles)
            break;
        const u64 u_end = listed ? u_begin + 1 : ((u_begin + a.upt < a.num_tiles) ? u_begin + a.upt : a.num_tiles);
        // Rolling prefetch: as soon as cell j of a round has been copied out of d[j], the same registers receive cell j
        // of the NEXT round (the rounds of a ticket are contiguous), so a wave always has 8 KiB in flight while it
        // filters and verifies — no second buffer (1024-thread blocks cap a wave at 128 VGPRs).
        uint4 d[kCells];
        bool have = false; // d[] holds (or is receiving) the round about to be processed (uniform)
        u32 carry = 0;     // the 4 bytes in front of that round (valid when have)
        // the deferred verify of the ticket (ac_pend_unit): pending pairs, their number, the units' counts
        const bool defer = kPend && !emit_final && !(a.flags & ((1u << 27) | (1u << 28) | (1u << 30) | (1u << 31))) && a.upt <= kAcUnitsPerTicketMax &&
                           (ANCH == 0 || a.xtab != nullptr);
        u32 pend = 0, npend = 0, ucnt = 0;
        for (u64 unit = u_begin; unit < u_end; ++unit)
        {
            const u64 useg = a.anchor + unit * (u64)kAcUnitBytes; // the unit = kAcRounds load rounds of 8 KiB
            if (emit_final && (u32)(a.unitinfo[unit] & kUiCountMask) <= a.stage_cap)
                continue;
            // (parks: the ticket's info words and slots wait in LDS.  Per unit: formed at the kernel's start these flags cost config 4 6.44 -> 6.46 ms)
            const bool parks = PIPE && !ANCH && !emit_final && chain && a.stage_cap == 16u && a.upt <= kAcUnitsPerTicketMax;
            wv.do_final = emit_final && want_pos;
            wv.do_stage = !emit_final && want_pos;
            wv.e_useg = useg;
            wv.e_fbase = wv.do_final ? a.offsets[unit] : 0ull;
            wv.e_slot = parks ? wv.park_slots + (u32)(unit - u_begin) * 16u
                              : reinterpret_cast<u32 *>(a.stage) + unit * (u64)a.stage_cap; // 32-bit staged words, see ac_emit_write
            wv.wcnt = 0;
#pragma unroll
            for (int r = 0; r < kAcRounds; ++r)
            {
                const u64 seg = useg + (u64)r * kSegBytes;
                const bool fast_now = seg + kSegBytes <= a.text_len;
                const bool interior = seg >= a.end_lo && seg + kSegBytes <= a.end_hi;
                const uint4 *src = reinterpret_cast<const uint4 *>(a.text + seg) + lane;
                u32 before = ac_round_before(a, seg, have, carry);
                if (fast_now) // what the round before did not prefetch (ac_roll_cells)
                {
#pragma unroll
                    for (int j = 0; j < kCells; ++j)
                        if (!have || j >= kRoll)
                            d[j] = src[j * kWave]; // (temporal on purpose: non-temporal stream loads measured 7.45 vs 6.87 ms, the verifier's text windows hit in cache)
                }
                // the next round of this ticket, if it is a full one, streams in behind this one
                const bool pf_next = kRoll > 0 && fast_now && !emit_final && seg + 2 * (u64)kSegBytes <= a.text_len &&
                                     (r + 1 < kAcRounds || unit + 1 < u_end);
                // always issued in the fast path (a uniform address select, not a branch: the s_waitcnt counts stay static);
                // without a next round every lane re-reads the first bytes of this one (one cached line per load, dropped)
                const uint4 *nsrc = pf_next ? src + kSegBytes / 16 : reinterpret_cast<const uint4 *>(a.text + seg);
                if (PIPE && fast_now)
                    ac_pair_round<ANCH>(wv.cbits, lane, r, d, nsrc, before);
                else if (fast_now) // (ANCH implies PIPE: see the static_assert at the kernel's head)
                    ac_cell_round<LINES, STRIDE>(a, wv, lane, r, seg, interior, d, nsrc, before);
                else
                    ac_ragged_round<LINES, STRIDE, ANCH>(a, wv, lane, r, seg, interior);
                have = pf_next;
                carry = before;
            }

            if constexpr (ANCH != 0)
                ac_anchor_stage2<CI, ANCH>(a, wv, lane, useg, acc_cand);
            // (ANCH: what follows is stage 3 — the same verify, over the END-pair bitmap instead of the candidate bitmap)
            const u32 *vbits = ANCH ? wv.ebits : wv.cbits;
            if constexpr (kPend)
                ac_pend_unit<CI, LINES, SHORT, STRIDE, ANCH, WW>(a, wv, lane, vbits, unit, u_begin, u_end, defer, parks, pend, npend, ucnt, acc_cand);
            else
            { // the plain verify loop of a unit
                static_assert(ANCH == 0, "the anchored instantiations pend");
                u32 mycnt, incl, n, n_tot;
                ac_verify_count<LINES, STRIDE>(a, vbits, lane, useg, mycnt, incl, n, n_tot);
                acc_cand += (u32)__builtin_amdgcn_readfirstlane((int)n);
                for (u32 b0 = 0; b0 < n_tot; b0 += 64)
                    ac_verify_batch<CI, LINES, SHORT, STRIDE, WW>(a, wv, lane, vbits, useg, mycnt, incl, n, n_tot, b0);
            }
            LineState wls{0, false, false, false};
            if (LINES)
                wls = ac_unit_lines(wv, lane);

            acc_total += wv.wcnt; // (deferred stage 3: zero here — the ticket's counts are added below)
            if (chain && !emit_final && lane == 0 && !(kPend && defer))
                ac_unit_info<LINES>(a, wv, unit, u_begin, parks, want_pos, wls);
        }
        const u32 nun = (u32)(u_end - u_begin);
        if (kPend && defer)
            acc_total += ac_ticket_info<PIPE && !ANCH>(a, wv, lane, u_begin, nun, ucnt, chain, want_pos);
        if (PIPE && !ANCH && !emit_final && chain && a.stage_cap == 16u && a.upt <= kAcUnitsPerTicketMax)
            ac_ticket_unpark(a, wv, lane, u_begin, nun, want_pos);
    }
    if (lane == 0 && acc_total && !a.emit_mode)
        atomicAdd(&a.ctr->total, acc_total);
    if (lane == 0 && acc_cand && !a.emit_mode)
        atomicAdd(&a.ctr->candidates, (unsigned long long)acc_cand);
}

// the units of a scan whose matches did not fit their staging slot, compacted (any order: an emitted unit writes at its own offset)
__global__ void ac_redo_list_kernel(const u64 *__restrict__ info, u64 n_units, u32 cap, u32 *__restrict__ list, u32 list_cap, unsigned long long *counter)
{
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_units && (u32)(info[i] & kUiCountMask) > cap)
    {
        const u64 at = atomicAdd(counter, 1ull);
        if (at < list_cap)
            list[at] = (u32)i;
    }
}

// ---------------------------------------------------------------------------------------------- host: launches and the scan driver
// (the tables: kg_ac_tables.h, built by kg_ac_build.hip)

static u32 ac_lds_bytes(u32 filter_words, bool lines)
{
    const u32 per_wave = kAcBitmapWords + (lines ? 2u * kAcBitmapWords : 0u);
    return (((filter_words + 3u) & ~3u) + kAcWaves * per_wave) * (u32)sizeof(u32);
}

constexpr u32 kAcMaxLds = 160u * 1024u; // LDS of a gfx950 CU: the most a launch of the scan kernel can ask for
template <bool CI, bool LN, bool SHORT, int STRIDE, int ANCH = 0, bool WW = false>
static hipError_t ac_launch3(const AcArgs &a, u32 grid, u32 lds, hipStream_t st)
{
    if constexpr (!WW && STRIDE == 2 && !SHORT)
        if (a.flags & F_WW)
            return ac_launch3<CI, LN, SHORT, STRIDE, ANCH, true>(a, grid, lds, st);
    // (always the MOST this kernel can ask for, the whole 160 KiB of a CU: no later, larger request can find a stale grant)
    if (const hipError_t e = grant_dynamic_lds<&ac_scan_kernel<CI, LN, SHORT, STRIDE, ANCH, WW>>((int)kAcMaxLds); e != hipSuccess)
        return e;
    hipLaunchKernelGGL((ac_scan_kernel<CI, LN, SHORT, STRIDE, ANCH, WW>), dim3(grid), dim3(kAcBlock), lds, st, a);
    return hipGetLastError();
}
template <bool CI, bool LN>
static hipError_t ac_launch2(const AcArgs &a, u32 grid, u32 lds, hipStream_t st)
{
    const bool shorts = a.has1 || a.has2 || a.has3;
    if constexpr (!LN)
        if (a.anch && a.stride == 2 && !shorts)
        {
            g_ac_anchored_launches.fetch_add(1, std::memory_order_relaxed);
            return a.anch_five ? ac_launch3<CI, false, false, 2, 2>(a, grid, lds, st) : ac_launch3<CI, false, false, 2, 1>(a, grid, lds, st);
        }
    if (a.stride == 2)
        return shorts ? ac_launch3<CI, LN, true, 2>(a, grid, lds, st) : ac_launch3<CI, LN, false, 2>(a, grid, lds, st);
    return shorts ? ac_launch3<CI, LN, true, 1>(a, grid, lds, st) : ac_launch3<CI, LN, false, 1>(a, grid, lds, st);
}
static hipError_t ac_launch(const AcArgs &a, u32 grid, u32 lds, hipStream_t st)
{
    const bool ci = a.flags & F_CI, ln = a.flags & F_LINES;
    if (ci && ln) return ac_launch2<true, true>(a, grid, lds, st);
    if (ci) return ac_launch2<true, false>(a, grid, lds, st);
    if (ln) return ac_launch2<false, true>(a, grid, lds, st);
    return ac_launch2<false, false>(a, grid, lds, st);
}

// one ac_scan call as its steps see it (kAcNext: a step hands the scan on to the next)
struct AcRun
{
    AcArgs a{};
    size_t own_hi = 0; // the caller's own range ends here (clipped to the text); a.own_* is the whole buffer for END-owned records
    u64 want = 0;      // records wanted: min(cap, max_count) (0: counts or -c)
    bool lines_on_list = false; // AcOwn::LinesOnList
    int fsc = 0;       // krep_gpu_debug_force_stage_cap (0: the dictionary's own slot)
    bool tiny = false; // the staged road: the register-compare kernel (kg_ac_tiny.hip), else the general one
    // for krep_gpu_debug_ac_last_scan (ac_report): the road as krep_gpu_debug_ac_scan_t numbers it, a one-pass road's ticket, the emit pass
    u32 road = 0, one_pass_upt = 0, emit = 0;
};
constexpr int kAcNext = -1;
// max_count 0, the empty text (its one empty match), an empty own range, -c with a newline inside a pattern
static int ac_early_out(const AcScan &c, size_t own_hi, krep_gpu_scan_out_t *out)
{
    if (c.max_count == 0) // aho_corasick.c:316
        return 0;
    if (c.text_len == 0)
    {
        // the empty pattern matches the empty text once (aho_corasick.c:441-463)
        if (c.t->has_empty)
            out->count = out->total_matches = 1;
        if (c.t->has_empty && c.d_pos && c.cap && c.track)
        {
            const match_position_t z{c.global_base, c.global_base};
            HIPCHK(hipMemcpyAsync(c.d_pos, &z, sizeof z, hipMemcpyHostToDevice, c.st));
            HIPCHK(hipStreamSynchronize(c.st));
            out->stored = 1;
        }
        return 0;
    }
    if (c.own_lo >= own_hi || c.t->lmax == 0)
        return 0;
    if (c.lines && c.t->has_nl)
        return fail("-c with a pattern containing a newline is not supported by the multi-pattern scan");
    return kAcNext;
}
// the scan kernel's arguments: ownership and the END range, the unit grid, the anchor decision, the exact dictionary, the hooks
static int ac_args(const AcScan &c, AcRun &r)
{
    AcTables *t = c.t;
    AcArgs &a = r.a;
    const size_t own_lo = c.own_lo, own_hi = r.own_hi, text_len = c.text_len;
    const bool own_by_end = c.own != AcOwn::Start;
    r.lines_on_list = c.own == AcOwn::LinesOnList;
    r.fsc = g_force_stage_cap.load(std::memory_order_relaxed);
    a.text = c.d_text; a.text_len = text_len; a.global_base = c.global_base;
    a.own_lo = own_lo; a.own_hi = own_hi;
    // END indices to examine.  Positions/counts own a match by its START (start-offset ownership), so ends
    // run up to own_hi + Lmax - 2.  -c owns by END index instead (a pattern without '\n' starts and ends
    // on the same line), which keeps the line bookkeeping inside the owned window.
    a.end_lo = own_lo;
    a.end_hi = (c.lines || own_by_end) ? own_hi : std::min<u64>(text_len, (u64)own_hi + t->lmax - 1);
    if (own_by_end)
    {
        // the record list -c is counted on (kg_scan_ac.hip scan_ac_lines_on_list) owns by END like the in-kernel -c road does: two
        // neighbouring pieces / shards may take different roads, and a match across their cut must belong to exactly one of them
        // (ADVICE r04).  No start clip: every start the buffer holds is in.
        a.own_lo = 0, a.own_hi = text_len;
    }
    // (END-owned records: a unit verifies the ends behind its first byte, so the end AT own_lo belongs to the unit in front —
    //  which has to exist; round 6)
    a.anchor = ((own_by_end && !c.lines && own_lo && !getenv("KREP_GPU_AC_R05_ANCHOR")) ? own_lo - 1 : own_lo) & ~(u64)15; // (the hook: the round-5 grid, for the regression test's own check)
    a.num_tiles = (a.end_hi - a.anchor + kAcUnitBytes - 1) / kAcUnitBytes;
    a.flags = (t->ci ? F_CI : 0) | (c.ww ? F_WW : 0) | (c.lines ? F_LINES : 0);
    a.flags |= getenv("KREP_GPU_AC_NOVERIFY") ? 1u << 31 : 0u; // measurement hook: filter cost only (wrong results by design)
    a.flags |= getenv("KREP_GPU_AC_NOSTAGE3") ? 1u << 28 : 0u; // measurement hook (anchored scan): candidates -> END pairs, no verify; a count-only scan returns the number of marked pairs
    a.flags |= getenv("KREP_GPU_AC_NODEFER") ? 1u << 27 : 0u;  // A/B hook (anchored scan): stage 3 at every unit's end, as first built
    a.flags |= getenv("KREP_GPU_AC_NOPROBE") ? 1u << 30 : 0u;  // measurement hook: filter + candidate enumeration, no probes: a count-only scan returns the number of candidates
    a.lmax = t->lmax; a.has1 = t->has1; a.has2 = t->has2; a.has3 = t->has3; a.has4 = t->has4;
    a.stride = 1;
    a.filter = c.lines ? t->d_filterx19 : t->d_filterx20;
    a.filter_words = (1u << (c.lines ? kXBitsLines : kXBitsBig)) / 32;
    if (t->d_filters20)
    {
        a.filter = c.lines ? t->d_filters19 : t->d_filters20;
        a.stride = 2;
    }
    // anchors (kg_ac_anchor.hip): decided once per dictionary on the first text of >= 1 MiB; every launch without in-kernel -c then
    // filters on the anchor grams and verifies the ends they name
    if (t->anch_state == 0 && text_len >= (1u << 20) && own_hi - own_lo >= (1u << 19))
    {
        HIPCHK(hipSetDevice(t->device));
        if (ac_anchor_prepare(t, c.d_text, text_len, own_lo, own_hi, c.st) == 2)
            (void)hipGetLastError(); // (the end grams stay; a failed sample is not a failed scan)
    }
    if (t->anch_state == 2 && !c.lines && a.stride == 2 && !getenv("KREP_GPU_AC_NO_ANCHOR"))
    {
        a.filter = t->d_filtera20;
        a.anch = t->d_anch; a.anch_mask = t->anch_mask; a.anch_mul = t->anch_mul; a.anch_five = t->anch_five;
    }
    if (t->d_xtab && !getenv("KREP_GPU_AC_NO_EXACT")) // the exact dictionary: stage 3 of the anchored scan, the slow path of the others
    {
        a.xlen = t->d_xlen; a.xtab = t->d_xtab; a.xmask = t->xmask; a.xmul = t->xmul;
    }
    a.s1 = t->d_s1; a.s2 = t->d_s2; a.s3 = t->d_s3;
    if (t->short_dup)
        a.flags |= F_AC_SHORT_DUP;
    a.edges = t->d_edges; a.emask = t->emask; a.copies = t->d_copies;
    a.gram4 = t->d_gram4; a.g4x = t->d_g4x; a.g4mask = t->g4mask;
    a.g4x_mode = t->g4x_mode; a.g4x_mask = t->g4x_mask; a.g4x_mul = t->g4x_mul;
    a.ctr = c.d_ctr;
    r.want = (c.d_pos && c.cap && !c.lines) ? std::min<u64>(c.cap, (u64)c.max_count) : 0;
    if (r.want)
        a.flags |= F_POS;
    a.positions = (u64 *)c.d_pos; a.pos_cap = r.want;
    return 0;
}
// from the counters in *c.h_ctr (a one-pass road, !staged, recorded every match and counts no lines; ~0 lines: the list -c is
// counted on overflowed a staging slot or its cap, and the caller counts again)
static int ac_result(const AcScan &c, const AcRun &r, bool staged, krep_gpu_scan_out_t *out)
{
    const Counters &h = *c.h_ctr;
    if (c.time_it)
    {
        float ms = 0;
        HIPCHK(hipEventElapsedTime(&ms, c.ev0, c.ev1));
        out->kernel_ms = ms;
    }
    const u64 total = h.total;
    out->total_matches = total;
    out->line_count = staged ? h.lines : 0;
    if (r.lines_on_list)
        out->line_count = (r.want && !h.overflow_units && total <= r.want) ? h.lines : ~0ull;
    const u64 summary = (staged && (r.want || c.lines)) ? h.summary : (total ? (kLnHead | kLnTail) : 0);
    out->has_newline = (summary & kLnNl) != 0;
    out->head_line_hit = (summary & kLnHead) != 0;
    out->tail_line_hit = (summary & kLnTail) != 0;
    out->count = std::min<u64>(c.lines ? h.lines : total, (u64)c.max_count);
    if (r.want && c.track)
    {
        out->stored = std::min<u64>(out->count, r.want);
        out->overflow = out->count > c.cap;
    }
    return 0;
}
// ---- a dictionary of single bytes, records wanted: memchr_search's one-pass kernel with a needle set (kg_single.hip).  The
// matches of aho_corasick_search for such a dictionary are one (i, i + 1) per matching position in text order
// (aho_corasick.c:383-437) — exactly that kernel's records.  Its shape rules: kg_single.hip single_fused_run.
static int ac_byte_set(const AcScan &c, AcRun &r, krep_gpu_scan_out_t *out)
{
    AcTables *t = c.t;
    if (!(t->set_n && r.want && !c.ww && c.own == AcOwn::Start && t->set_ok && c.text_len >= (size_t)16 * kSegBytes && !r.fsc &&
          !getenv("KREP_GPU_NO_FUSED1") && !getenv("KREP_GPU_AC_NO_TINY")))
        return kAcNext;
    LitArgs la{};
    la.text = c.d_text; la.text_len = c.text_len; la.global_base = c.global_base;
    la.own_lo = c.own_lo; la.own_hi = r.own_hi;
    la.anchor = c.own_lo & ~(u64)15;
    la.rounds = kRoundsBig;
    const u64 tile_bytes = (u64)kRoundsBig * kSegBytes * kWavesPerBlk;
    la.num_tiles = (r.own_hi - la.anchor + tile_bytes - 1) / tile_bytes;
    la.ww_exempt_left = ~0ull;
    la.m = 1;
    la.flags = (t->ci ? F_CI : 0) | F_POS;
    la.ctr = c.d_ctr; la.positions = (uint64_t *)c.d_pos; la.pos_cap = r.want;
    la.set_n = t->set_n;
    for (u32 k = 0; k < t->set_n; ++k)
    {
        la.set_p[k] = 0x01010101u * t->set_b[k];
        la.set_l[k] = (t->ci && t->set_b[k] >= 'a' && t->set_b[k] <= 'z') ? 0x20202020u : 0u;
    }
    la.p0 = la.set_p[0]; la.l0 = la.set_l[0]; la.k0 = 0xffu;
    HIPCHK(hipSetDevice(t->device));
    if (c.time_it) HIPCHK(hipEventRecord(c.ev0, c.st));
    const int rc = single_fused_run(la, la.num_tiles * kWavesPerBlk, r.own_hi - la.anchor, *c.post, c.d_ctr, c.h_ctr, (u32)c.num_cu, &t->set_shape,
                                    c.time_it ? c.ev1 : nullptr, c.st, false); // (not counted as krep_gpu_debug_single_launches)
    if (rc == 2)
        return 2;
    if (rc != kFusedGaveUp)
        return ac_result(c, r, false, out);
    t->set_ok = false; // denser than the largest rings hold: the register-compare kernel below, for good
    return kAcNext;
}
// ---- the tiny dictionary's density rules: its one-pass flavours (ac_tiny_one_pass) and their re-opening behind a staged scan
// tickets of the DENSE flavour for e matches per unit: two consecutive tickets share the ring, a quarter is left for clustering
static u32 tiny_dense_upt(double e)
{
    if (e <= 0.0)
        return 4u;
    const double u = (double)ac_tiny_dense_ring() / (2.5 * e);
    return u >= 4.0 ? 4u : (u32)u;
}
// behind a staged scan of a tiny dictionary that counted `total` matches in `n_units` units
static void tiny_reopen(AcTables *t, u64 total, u64 n_units)
{
    if (!t->tiny_fused_ok && total < n_units * 20) // (a 128-KiB ticket's ring holds ~1000: 125 per unit)
        t->tiny_fused_ok = true;
    if (!t->tiny_dense_ok && total < n_units * 20)
        t->tiny_dense_ok = true;
    // a dense text through the staging road (a dictionary with a long length starts here: the item flavour of the one-pass
    // writer does not take it): its next scans take the DENSE flavour, in tickets sized by the density just counted
    if (!t->tiny.five && t->tiny_dense_ok && !t->tiny_dense_upt && total >= n_units * 48)
        t->tiny_dense_upt = tiny_dense_upt((double)total / (double)n_units);
}
// ---- a tiny dictionary, records wanted: ONE pass (kg_ac_tiny.hip FUSED, round 5) — matches ranked into an LDS ring per
// 128-KiB ticket, the tickets' counts resolved into prefixes by one wave, records written at their final index: no masks kept,
// no staging, no info words, no post-pass.  A ticket with more matches than its ring holds (~0.6 % of the bytes) is counted,
// not recorded; the count gives the density, and the density the ticket size (1..4 units) of the DENSE flavour — 16-bit ring
// entries, matches decoded where they are found — which takes the scan again and the dictionary's next ones (up to ~15 % of
// the bytes; a long length included, which the item flavour does not take).  Beyond that, and for 4-byte patterns beside a long
// length, the staging road; every decision is re-evaluated by the following scans.
static int ac_tiny_one_pass(const AcScan &c, AcRun &r, krep_gpu_scan_out_t *out)
{
    AcTables *t = c.t;
    Counters *h_ctr = c.h_ctr;
    const bool one_pass_ok = t->tiny.ok && !t->tiny.five && r.want && !c.ww && c.own != AcOwn::End && c.track && !r.fsc &&
                             c.text_len >= (size_t)64 * kAcUnitBytes && !getenv("KREP_GPU_AC_NO_TINY_FUSED") && !getenv("KREP_GPU_AC_NO_TINY");
    const bool dense_first = getenv("KREP_GPU_AC_TINY_DENSE_FIRST") != nullptr; // measurement hook: the DENSE flavour at any density
    if (dense_first && one_pass_ok && !t->tiny_dense_upt && t->tiny_dense_ok)
        t->tiny_dense_upt = 4;
    for (int attempt = 0; one_pass_ok && attempt < 3; ++attempt)
    {
        const bool dense = t->tiny_dense_upt != 0 && !getenv("KREP_GPU_AC_NO_TINY_DENSE");
        if (!dense && (!t->tiny_fused_ok || t->tiny.llong))
            break;
        AcArgs f = r.a;
        f.upt = dense ? t->tiny_dense_upt : (u32)std::min<u64>(kAcUnitsPerTicketMax, std::max<u64>(1, f.num_tiles / ((u64)c.num_cu * kTinyWaves * 4)));
        const u64 n_tk = (f.num_tiles + f.upt - 1) / f.upt;
        const size_t tk_bytes = 2 * n_tk * sizeof(unsigned long long); // counts | prefixes
        HIPCHK(grow_scratch(c.post->tk_cap, n_tk, n_tk, {dev_buf(c.post->d_tk, tk_bytes)}));
        f.tk_agg = c.post->d_tk; f.tk_pref = c.post->d_tk + n_tk; f.n_tk = n_tk; f.stage_cap = 0;
        HIPCHK(hipSetDevice(t->device));
        if (c.time_it) HIPCHK(hipEventRecord(c.ev0, c.st));
        HIPCHK(hipMemsetAsync(c.d_ctr, 0, sizeof(Counters), c.st));
        HIPCHK(hipMemsetAsync(c.post->d_tk, 0, tk_bytes, c.st));
        HIPCHK(ac_tiny_launch_fused(f, t->tiny, n_tk, (u32)c.num_cu, c.st, dense));
        // (the record list -c is counted on: its line gaps behind the scan on the same stream, skipped by the kernel itself when
        //  a ticket overflowed its ring)
        if (r.lines_on_list && tail_launch_line_gaps(c.d_text, c.text_len, c.global_base, (const uint64_t *)c.d_pos, &c.d_ctr->total,
                                                     &c.d_ctr->overflow_units, r.want, &c.d_ctr->lines, c.st))
            return 2;
        if (c.time_it) HIPCHK(hipEventRecord(c.ev1, c.st));
        HIPCHK(hipMemcpyAsync(h_ctr, c.d_ctr, sizeof(Counters), hipMemcpyDeviceToHost, c.st));
        HIPCHK(hipStreamSynchronize(c.st));
        const double per_unit = (double)h_ctr->total / (double)f.num_tiles;
        if (getenv("KREP_GPU_DEBUG"))
            fprintf(stderr, "krep-gpu: tiny one-pass (%s, %u units per ticket): %llu matches, %.1f per unit, %llu waves overflowed\n",
                    dense ? "dense" : "items", f.upt, (unsigned long long)h_ctr->total, per_unit, (unsigned long long)h_ctr->overflow_units);
        if (!h_ctr->overflow_units)
        {
            r.road = dense ? 3u : 2u;
            r.one_pass_upt = f.upt;
            if (ac_result(c, r, false, out)) // (track: one_pass_ok asks for it)
                return 2;
            if (dense)
            {
                // re-evaluated by every scan: the ticket size follows the density, and a text with fewer than 24 matches per unit
                // goes back to the item flavour (or, with a long length, to the staging road)
                if (per_unit < 24.0 && !dense_first)
                    t->tiny_dense_upt = 0, t->tiny_fused_ok = true;
                else
                    t->tiny_dense_upt = std::max(1u, tiny_dense_upt(per_unit));
            }
            return 0;
        }
        // counted, not recorded (the resolver's running sum is the total — unless the spin-limit safety net fired: total 0)
        u32 nu = (t->tiny_dense_ok && h_ctr->total) ? tiny_dense_upt(per_unit) : 0u;
        if (dense && nu >= t->tiny_dense_upt)
            nu = t->tiny_dense_upt - 1u; // (clustered matches: the next smaller ticket)
        if (!dense)
            t->tiny_fused_ok = false; // (re-opened by tiny_reopen, by a text sparse enough for the rings)
        t->tiny_dense_upt = nu;
        if (!nu)
        {
            t->tiny_dense_ok = false; // (re-opened like tiny_fused_ok)
            break;
        }
    }
    return kAcNext;
}
// a launch of the staged road (its scan or its emit pass): the register-compare kernel over the tickets, else the general one
static hipError_t ac_staged_launch(const AcScan &c, const AcRun &r, const AcArgs &a)
{
    const u64 n_tickets = (a.num_tiles + a.upt - 1) / a.upt;
    if (r.tiny)
        return ac_tiny_launch(a, c.t->tiny, n_tickets, (u32)c.num_cu, c.st);
    const u32 lds = ac_lds_bytes(a.filter_words, c.lines), per_cu = lds <= 80 * 1024 ? 2u : 1u;
    return ac_launch(a, (u32)std::min<u64>((n_tickets + kAcWaves - 1) / kAcWaves, (u64)c.num_cu * per_cu), lds, c.st);
}
// ---- the staged road: the scan kernel stages every unit's matches, the post-pass orders them into the record list (and counts
// -c's lines), the line gaps of the record list -c is counted on behind it; the counters are read back
static int ac_staged(const AcScan &c, AcRun &r)
{
    AcArgs &a = r.a;
    const bool chain = r.want || c.lines;
    const u64 n_units = a.num_tiles;
    // 16 staged matches (32-bit words: unit-relative start + length) = one 64-byte slot per 16 KiB unit; BASELINE config 4 puts 5.3
    // matches in a unit.  Units that hold more are re-scanned in emit mode, and a scan in which more than 1 in 64 units did
    // raises the dictionary's slot to 64 for its next scans.  (Small slots keep the store stream dense: kg_scan.hip, lit_args.)
    a.stage_cap = r.want ? (r.fsc ? (u32)r.fsc : c.t->stage_cap) : 0u;
    if (chain)
    {
        if (post_reserve(*c.post, n_units, (n_units * a.stage_cap + 1) / 2))
            return 2;
        a.unitinfo = c.post->d_unitinfo; a.stage = (u64 *)c.post->d_stage; a.offsets = (const u64 *)c.post->d_offsets;
    }
    HIPCHK(hipSetDevice(c.t->device));
    // tiny dictionaries run in kg_ac_tiny.hip (same units, staging, info words and post-pass); -w takes the general kernel
    // (4-byte patterns beside a long length — AcTiny::five: only the case-sensitive COUNT runs in the register-compare kernel, every
    //  other mode of such a dictionary measured faster here)
    r.tiny = c.t->tiny.ok && !c.ww && (!c.t->tiny.five || (!r.want && !c.lines && !c.t->ci));
    const u32 waves = r.tiny ? (u32)kTinyWaves : (u32)kAcWaves;
    // ticket size by text size: >= ~4 tickets per resident wave before tickets grow (small host buffers keep every
    // CU busy), 8 units (128 KiB) on large texts
    a.upt = (u32)std::min<u64>(kAcUnitsPerTicketMax, std::max<u64>(1, a.num_tiles / ((u64)c.num_cu * waves * 4)));
    if (const char *e = getenv("KREP_GPU_AC_UPT")) // test hook: the ticket size large texts get (the anchored scan defers its verify stage over a ticket's units)
    {
        const int v = atoi(e);
        if (v >= 1 && v <= (int)kAcUnitsPerTicketMax)
            a.upt = (u32)v;
    }
    if (c.time_it) HIPCHK(hipEventRecord(c.ev0, c.st));
    // KREP_GPU_SYNC_DEBUG=1: synchronise behind every launch of this function and say which one faulted
    const bool dbg_sync = getenv("KREP_GPU_SYNC_DEBUG") != nullptr;
    auto dbg = [&](const char *what) -> int {
        if (!dbg_sync)
            return 0;
        const hipError_t e = hipStreamSynchronize(c.st);
        return e == hipSuccess ? 0 : fail("ac_scan: %s faulted: %s (tiny=%d stride=%u units=%llu stage_cap=%u lines=%d list=%d own=[%llu,%llu) end=[%llu,%llu) n=%llu)", what,
                                          hipGetErrorString(e), (int)r.tiny, a.stride, (unsigned long long)n_units, a.stage_cap, (int)c.lines, (int)r.lines_on_list,
                                          (unsigned long long)a.own_lo, (unsigned long long)a.own_hi, (unsigned long long)a.end_lo,
                                          (unsigned long long)a.end_hi, (unsigned long long)c.text_len);
    };
    HIPCHK(hipMemsetAsync(c.d_ctr, 0, sizeof(Counters), c.st));
    HIPCHK(ac_staged_launch(c, r, a));
    if (dbg("scan kernel")) return 2;
    if (chain && post_order(*c.post, n_units, a.stage_cap, 0, a.anchor + c.global_base, kAcUnitBytes, c.lines, (uint64_t *)c.d_pos, r.want, c.d_ctr,
                            c.num_cu, c.st))
        return 2;
    if (dbg("post-pass")) return 2;
    // lines_on_list (kg_scan_ac.hip scan_ac_lines_on_list): the distinct lines of the record list just gathered, counted by the
    // newline gaps between neighbours, behind the post-pass on the same stream — valid when no unit overflowed its staging
    // slot and the list fitted (ac_result checks both; the caller repeats otherwise)
    if (r.lines_on_list && r.want && tail_launch_line_gaps(c.d_text, c.text_len, c.global_base, (const uint64_t *)c.d_pos, &c.d_ctr->total,
                                                           &c.d_ctr->overflow_units, r.want, &c.d_ctr->lines, c.st))
        return 2;
    if (dbg("line-gap kernel")) return 2;
    if (c.time_it) HIPCHK(hipEventRecord(c.ev1, c.st));
    HIPCHK(hipMemcpyAsync(c.h_ctr, c.d_ctr, sizeof(Counters), hipMemcpyDeviceToHost, c.st));
    HIPCHK(hipStreamSynchronize(c.st));
    return 0;
}
// behind a staged scan: what its counters teach the dictionary for the next scans
static void ac_learn(const AcScan &c, const AcRun &r)
{
    AcTables *t = c.t;
    const AcArgs &a = r.a;
    const Counters &h = *c.h_ctr;
    const size_t own_lo = c.own_lo, own_hi = r.own_hi;
    const u64 n_units = a.num_tiles;
    // The anchor decision follows the TEXT, and a dictionary meets more than one: the kernel counts the positions its filter passed, and a
    // scan whose measured rate is both one that matters (the decision's own 0.8 % bar) and more than twice what the decision estimated for
    // the filter it chose re-opens the decision, so that the next scan samples the text it is given (an i.i.d. text first, a word-like
    // one after it: 0.04 of the roofline without this, 0.49 with).  Matches are candidates too, so a text dense with matches can ask as
    // well; the repeats are bounded, and a repeat on the same kind of text decides as before.
    if (!r.tiny && !c.lines && a.stride == 2 && own_hi > own_lo)
    {
        const double tested = 0.5 * (double)(own_hi - own_lo);
        t->anch_measured = (double)h.candidates / tested;
        const double est = t->anch_state == 2 ? t->anch_rate : t->anch_rate0;
        if (t->anch_state != 0 && t->anch_resamples < kAnchResamples && c.text_len >= (1u << 20) && own_hi - own_lo >= (1u << 19) &&
            t->anch_measured > 0.008 && t->anch_measured > 2.0 * est + 0.002 && !getenv("KREP_GPU_AC_ANCHOR") && !getenv("KREP_GPU_AC_NO_RESAMPLE"))
        {
            if (getenv("KREP_GPU_DEBUG"))
                fprintf(stderr, "krep-gpu: anchors: measured %.3f %% candidates per tested position against %.3f %% estimated (%s): the next scan decides again\n",
                        100.0 * t->anch_measured, 100.0 * est, t->anch_state == 2 ? "anchored" : "end grams");
            t->anch_state = 0;
            ++t->anch_resamples;
        }
    }
    if (!r.want || r.fsc)
        return;
    // a dense dictionary / text: the next scans stage 64 matches per unit — or, when most units of a tiny dictionary hold more
    // than that and the average is beyond 256 (`-e e -e t`: a thousand per unit), none at all: the first launch only counts (no masks kept, nothing staged)
    // and the emit-mode launch writes every record
    if (r.tiny && h.overflow_units * 2 > n_units && h.total > n_units * 256)
        t->stage_cap = 0;
    else if (t->stage_cap && h.overflow_units * 64 > n_units)
        t->stage_cap = 64;
    else if (!t->stage_cap && h.total < n_units * 32)
        t->stage_cap = 64; // the dense road (count pass + emit pass) is left again when a text holds < 32 matches per unit
    if (r.tiny)
        tiny_reopen(t, h.total, n_units);
    // a byte-set dictionary that proved too dense for the one-pass rings gets them back on a text half as dense as they hold
    if (t->set_n && !t->set_ok && own_hi > a.anchor && single_fused_reopens(h.total, own_hi - a.anchor))
        t->set_ok = true;
}
// ---- the units whose matches did not fit their staging slot: scanned again in emit mode, each writing at its own offset
static int ac_emit(const AcScan &c, AcRun &r)
{
    AcTables *t = c.t;
    const u64 n_units = r.a.num_tiles;
    AcArgs e = r.a;
    e.emit_mode = 1;
    HIPCHK(hipMemsetAsync(&c.d_ctr->ticket, 0, sizeof(unsigned long long), c.st));
    if (!r.tiny && !getenv("KREP_GPU_AC_NO_REDO_LIST"))
    {
        // the overflowed units as a list (their number is known: the scan counted them), one ticket each
        const u64 n_over = c.h_ctr->overflow_units;
        const u64 redo_cap = n_over + n_over / 4 + 64;
        if (grow_scratch(t->redo_cap, n_over, redo_cap, {dev_buf(t->d_redo, redo_cap * sizeof(u32))}) != hipSuccess)
            (void)hipGetLastError(); // (no list: the emit pass walks every unit)
        if (t->d_redo && n_over <= 0xffffffffull)
        {
            HIPCHK(hipMemsetAsync(&c.d_ctr->pad[3], 0, sizeof(unsigned long long), c.st));
            hipLaunchKernelGGL(ac_redo_list_kernel, dim3((u32)((n_units + 255) / 256)), dim3(256), 0, c.st, (const u64 *)e.unitinfo, n_units, e.stage_cap,
                               t->d_redo, (u32)t->redo_cap, &c.d_ctr->pad[3]);
            e.redo_list = t->d_redo, e.n_redo = (u32)n_over;
        }
    }
    r.emit = e.redo_list ? 1u : 2u;
    HIPCHK(ac_staged_launch(c, r, e));
    if (c.time_it) HIPCHK(hipEventRecord(c.ev1, c.st));
    HIPCHK(hipStreamSynchronize(c.st));
    return 0;
}
// test hook (krep_gpu_debug_ac_last_scan): what the scan that just ended ran with, as the launch rules above decided it
static void ac_report(const AcScan &c, const AcRun &r)
{
    const AcArgs &a = r.a;
    krep_gpu_debug_ac_scan_t &o = c.t->last;
    const uint64_t scans = o.scans + 1;
    o = krep_gpu_debug_ac_scan_t{};
    o.scans = scans;
    o.road = r.road;
    o.next_stage_cap = c.t->stage_cap;
    o.short_lens = (c.t->has1 ? 1u : 0u) | (c.t->has2 ? 2u : 0u) | (c.t->has3 ? 4u : 0u);
    o.shorts = o.short_lens != 0;
    o.ci = c.t->ci;
    if (r.road == 0)
        return;
    const bool general = r.road == 5;
    o.lines = c.lines;
    o.stride = a.stride;
    // (ac_launch2 / ac_launch3: the anchored and the WW instantiations)
    const bool anchored = general && !c.lines && a.anch && a.stride == 2 && !o.shorts;
    o.anch = anchored ? (a.anch_five ? 2u : 1u) : 0u;
    o.ww_filter = general && a.stride == 2 && !o.shorts && (a.flags & F_WW) != 0;
    o.exact = a.xtab != nullptr;
    o.g4x_mode = a.g4x_mode;
    o.n_units = a.num_tiles;
    const bool staged = r.road >= 4;
    o.stage_cap = staged ? a.stage_cap : 0u;
    o.upt = staged ? a.upt : r.one_pass_upt;
    o.overflow_units = (staged && r.want) ? c.h_ctr->overflow_units : 0;
    o.emit = r.emit;
}
int ac_scan(const AcScan &c, krep_gpu_scan_out_t *out)
{
    memset(out, 0, sizeof *out);
    AcRun r;
    r.own_hi = std::min(c.own_hi, c.text_len);
    int rc = ac_early_out(c, r.own_hi, out);
    if (rc == kAcNext)
    {
        r.road = 1; // (the byte set's when it answers; the tiny one-pass road names its flavour)
        rc = ac_args(c, r) ? 2 : ac_byte_set(c, r, out);
    }
    if (rc == kAcNext) rc = ac_tiny_one_pass(c, r, out);
    if (rc != kAcNext)
    {
        if (!rc) ac_report(c, r);
        return rc;
    }
    if (ac_staged(c, r)) return 2;
    r.road = r.tiny ? 4u : 5u;
    ac_learn(c, r);
    if (r.want && c.h_ctr->overflow_units && ac_emit(c, r)) return 2;
    ac_report(c, r);
    return ac_result(c, r, true, out);
}

} // namespace kg
