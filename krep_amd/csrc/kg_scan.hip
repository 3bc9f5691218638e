// kg_scan.hip — krep_gpu_scan_device[_ex|_seq](): the device-resident scan with every reference return-value convention
// (verdict_for), the single-literal pass and its post-passes (lit_pass and its steps lit_args .. lit_reopen), one function per
// match-set family behind scan_literal (lit_nlwalk, lit_replay_piece / _whole, lit_neon_zero, lit_plain, lit_walk; the shared
// epilogue lit_finish; kg_greedy.hip / kg_tail.hip) and how a text may be split (kg::split_mode, the boundary record
// kg::fold_carry); the multi-pattern drivers are in kg_scan_ac.hip.  Host logic only; kernels live in kg_literal.hip /
// kg_single.hip / kg_ac.hip / kg_post.hip / kg_greedy.hip / kg_tail.hip / kg_format.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/krep_gpu.h"
#include "kg_common.h"
#include "kg_internal.h"
#include "kg_plan.h"
#include "kg_replay.h"
#include "kg_tickets.h"

using namespace kg;

// ------------------------------------------------------------------------------------ reference return-value conventions
// What the reference function returns / stores given the number of emitted matches (`total`, after
// greedy selection and -w) or distinct lines.  One place for all the max_count corner cases.
// (the rule itself is kg::verdict_rule, kg_internal.h: the batch's per-item cut is derived from the same function)
static Verdict verdict_for(int algo, const krep_gpu_plan *pl, uint64_t total, uint64_t lines, bool have_result)
{
    return verdict_rule(algo, pl->max_count, pl->lines, pl->track, total, lines, have_result);
}

int kg::stop_clock(krep_gpu_plan *pl, bool record_ev1, hipStream_t st, krep_gpu_scan_out_t *out)
{
    if (record_ev1) HIPCHK(hipEventRecord(pl->ev1, st));
    HIPCHK(hipStreamSynchronize(st));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, pl->ev0, pl->ev1));
    out->kernel_ms = ms;
    return 0;
}

// ------------------------------------------------------------------------------------ device scan: single literal
namespace {
// one pass of the literal kernel family + its ordering post-pass
struct LitPass
{
    bool ww = false, lines = false;
    bool first_byte = false;  // candidate pass of memchr_short -o: scan for pattern[0] only (starts clipped to n - m)
    size_t own_lo = 0, own_hi = 0;
    uint64_t excl_lo = 0, excl_hi = 0; // buffer-relative exclusion window (simd_avx512_search's unexamined block)
    uint64_t ww_exempt = ~0ull;        // buffer-relative start whose left-neighbour test is skipped
    enum Sink { COUNT, RECORDS, OCC } sink = COUNT;
    uint64_t *d_out = nullptr;         // RECORDS: final match_position_t buffer
    uint64_t out_cap = 0;
    PostScratch *post = nullptr;
    hipEvent_t ev_end = nullptr;       // recorded right behind the last kernel of the pass (before the counter read-back)
};
struct LitResult
{
    uint64_t total = 0, lines = 0;
    unsigned long long summary = 0;
    uint64_t n_units = 0, unit_bytes = 0, anchor = 0;
};
// a window as the literal kernels see it (lit_pass): their arguments and what the steps of one pass share
struct LitScan
{
    LitArgs a{};
    uint64_t hi_match = 0;  // starts in [a.own_lo, hi_match) are matched
    uint64_t n_units = 0;   // 32-KiB units of the launch
    int fsc = 0;            // krep_gpu_debug_force_stage_cap (0: the plan's own slot)
    bool dma_keep = false;  // KREP_GPU_LIT_DMA_KEEP (measurement aid): no look, no bar
    uint64_t span() const { return hi_match - a.anchor; }
    uint64_t unit_bytes() const { return (uint64_t)a.rounds * kSegBytes; }
    double density(uint64_t hits) const { return (double)hits / (double)span(); }
};
} // namespace

// hits per 32-KiB unit from which a 2..8-byte literal with records takes the one-pass kernel (KREP_GPU_FUSEDK_MIN: measurement aid)
static double fusedk_min_hits_per_unit()
{
    static const double v = [] {
        const char *e = getenv("KREP_GPU_FUSEDK_MIN");
        return e ? atof(e) : 24.0;
    }();
    return v;
}
// share of the 1-KiB cells beyond which a text bars the LDS-DMA kernel (KREP_GPU_LIT_DMA_MAX_PASS: measurement aid)
static double lit_dma_max_pass()
{
    static const double v = [] { const char *e = getenv("KREP_GPU_LIT_DMA_MAX_PASS"); return e ? atof(e) : 0.35; }();
    return v;
}

// the kernel arguments of a pass over the window: tiles, pattern words, flags, the LDS-DMA prefilter, the staging slot
static LitScan lit_args(const krep_gpu_plan *pl, const Window &w, const LitPass &ps, size_t own_hi, uint64_t hi_match)
{
    LitScan L;
    LitArgs &a = L.a;
    const uint32_t m_scan = ps.first_byte ? 1u : pl->m;
    L.hi_match = hi_match;
    a.text = w.d_text;
    a.text_len = w.text_len;
    a.own_lo = ps.own_lo;
    a.own_hi = own_hi;
    a.anchor = ps.own_lo & ~(uint64_t)15;
    {
        // big tiles (128 KiB) once there are enough of them to fill the chip several times over
        const uint64_t span = hi_match - a.anchor;
        a.rounds = span >= ((uint64_t)pl->num_cu * 16 * kRoundsBig * kSegBytes * kWavesPerBlk) ? kRoundsBig : 1;
        const int fr = g_force_rounds.load(std::memory_order_relaxed);
        if (fr == 1 || fr == kRoundsBig)
            a.rounds = (uint32_t)fr;
        const uint64_t tile_bytes = (uint64_t)a.rounds * kSegBytes * kWavesPerBlk;
        a.num_tiles = (span + tile_bytes - 1) / tile_bytes;
    }
    a.global_base = w.global_base;
    a.ww_exempt_left = ps.ww_exempt;
    a.excl_lo = ps.excl_lo;
    a.excl_hi = ps.excl_hi;
    a.m = m_scan;
    if (ps.first_byte)
    {
        const uint8_t b = pl->pat_folded[0];
        a.p0 = 0x01010101u * b;
        a.k0 = 0xffu;
        a.l0 = (!pl->cs && b >= 'a' && b <= 'z') ? 0x20202020u : 0u;
    }
    else
    {
        a.p0 = pl->p0; a.p1 = pl->p1; a.k0 = pl->k0; a.k1 = pl->k1;
        a.l0 = pl->l0; a.l1 = pl->l1;
        a.p2 = pl->p2; a.p3 = pl->p3; a.k2 = pl->k2; a.k3 = pl->k3; a.l2 = pl->l2; a.l3 = pl->l3;
    }
    a.pat = pl->d_pat;
    a.pat_chunks = pl->d_pat_chunks;
    a.n_chunks = ps.first_byte ? 0 : pl->n_chunks;
    a.ctr = pl->d_ctr;
    a.flags = (pl->cs ? 0 : F_CI) | (ps.ww ? F_WW : 0) | (ps.lines ? F_LINES : 0) | (ps.sink != LitPass::COUNT ? F_POS : 0);
    {
        // kg_literal_dma.hip's prefilter: only for a first byte that text rarely holds (the blank and the dozen most frequent letters
        // of running text, either case, would pass nearly every 16-byte lane: the test would be paid for nothing)
        // (case-sensitive: the lower-case ones only — a capital first letter is rare)
        const uint32_t b0 = (a.p0 & 0xffu) | (pl->cs ? 0u : 0x20u);
        static const char common[] = "etaoinshrdlu";
        bool rare = b0 != ' ' && b0 != '\n';
        for (const char *q = common; *q; ++q)
            rare = rare && b0 != (uint32_t)*q;
        a.prefilter = (rare && !ps.first_byte && !getenv("KREP_GPU_LIT_NO_PREFILTER")) ? 0x01010101u * b0 : 0u;
    }
    L.n_units = a.num_tiles * kWavesPerBlk;
    // Staging slot per unit.  Single byte: 512 offsets (1 KiB) per 32 KiB unit, ~1.5x BASELINE's 1 % density.  Sparse kinds:
    // 16 offsets = ONE 32-byte slot per 32 KiB unit (BASELINE's 1e-4/B puts 3.3 hits in a unit); units that hold more take the
    // emit-mode re-scan, and a scan in which more than 1 in 64 units did raises the plan's slot to 64 for its next scans.
    // Why so small: every unit's slot is a store into a different place, and the 4096 units in flight walk through the
    // staging array one slot each per step — with 128-byte slots through 128 pages of 4 KiB per step.  On boxes where the
    // driver backs the scratch with small page-table fragments the offsets-producing scan ran 0.3-0.5 ms slower in every
    // second process (store translation misses, coupled to the loads through the shared in-order vmcnt); 32-byte slots
    // cut that to < 0.1 ms (same process, 32 GiB: 5.75/5.48/5.82/5.52 ms with 64 entries, 5.47/5.43/5.52/5.41 with 16).
    a.stage_cap = 0;
    if (a.flags & F_POS)
        a.stage_cap = a.rounds == kRoundsBig ? (m_scan == 1 ? 512u : pl->sparse_cap) : (m_scan == 1 ? 256u : 32u);
    L.fsc = g_force_stage_cap.load(std::memory_order_relaxed);
    if (L.fsc && (a.flags & F_POS))
        a.stage_cap = (uint32_t)L.fsc;
    return L;
}

// The dealing of units to waves, and the LDS-DMA kernel's look at the text and the bar it sets.
static int lit_dma_look(krep_gpu_plan *pl, const Window &w, const LitPass &ps, LitScan &L, hipStream_t st)
{
    LitArgs &a = L.a;
    const uint32_t m_scan = a.m;
    // Dealing: from ~24 GiB on every wave draws tickets of 8 units (>= 24 tickets per resident wave, ~26 fetch-adds/us on the
    // ticket word); below that the static interleaved deal (upt = 0) is faster — measured at 8 GiB: 1.38 vs 1.41 ms with
    // offsets, 1.29 vs 1.37 ms counting; at 16 GiB 2.58 vs 2.63 ms; at 2 GiB 0.37 vs 0.48 ms (the ticket word becomes the limit
    // of a short scan); at 32 GiB tickets win: 5.20 vs 5.31 ms, and 7.1 vs 7.9 ms on the single-byte workload
    // (the LDS-DMA kernel, kg_literal_dma.hip, wants tickets — a ticket is what it streams through without a seam — and is ahead with them
    //  from ~8 GiB on: 8 GiB 1.339 against 1.362 ms for the register kernel's static deal, 16 GiB 2.610 against 2.639; round 6.  The 8 units
    //  set here are the SHORT ticket of its one-pass records mode, which sizes a long one for the bulk of the text by the density the plan
    //  knows: lit_dma_one_pass, kg_tickets.h TkMap; measured ticket sizes: profiles/r08_ticket_size.txt)
    const bool dma_shape = m_scan >= 2 && m_scan <= 8 && !ps.lines && !ps.first_byte && a.prefilter != 0u && !getenv("KREP_GPU_LIT_NO_DMA");
    auto tickets_for = [&](bool dma) { return (a.rounds == kRoundsBig && L.n_units / ((uint64_t)pl->num_cu * 16) >= (dma ? 64u : 192u)) ? 8u : 0u; };
    a.upt = tickets_for(dma_shape);
    // ... and wants a TEXT in which the prefilter's byte is rare: a 1-KiB cell that holds it pays the full compare, which two workgroups per CU
    // do not hide.  32 GiB, offsets produced, by the share of cells that hold the byte (profiles/r06_ldsdma_byte_rate.txt): 10 % 5.08 ms,
    // 27 % 5.08, 46 % 5.23, 68 % 5.75, 96 % 6.49 — against 5.19-5.20 ms of the register kernel throughout.  The static rule above only bars
    // the letters that running text is made of; what THIS text holds is sampled once (two 2-MiB windows, one wave per cell) before the plan's
    // first such launch, and counted by every launch of the kernel (Counters::candidates, lit_dma_rate).  A plan barred by one text looks
    // again at the next.
    const double max_pass = lit_dma_max_pass();
    L.dma_keep = getenv("KREP_GPU_LIT_DMA_KEEP") != nullptr; // measurement aid: no look, no bar
    if (dma_shape && (a.upt >= 4 || getenv("KREP_GPU_LIT_DMA_ALL")) && a.rounds == kRoundsBig && !L.dma_keep && L.span() >= (64ull << 20) &&
        (!pl->dma_look_done || (pl->dma_off && (pl->dma_off_text != (const void *)w.d_text || pl->dma_off_len != w.text_len))))
    {
        pl->dma_look_done = true;
        const uint64_t span = L.span(), win = 2ull << 20;
        HIPCHK(hipMemsetAsync(pl->d_ctr, 0, sizeof(Counters), st));
        for (int q = 0; q < 2; ++q)
            HIPCHK(launch_dma_byte_look(w.d_text, (a.anchor + span / 4 * (2 * q + 1)) & ~(uint64_t)15, (uint32_t)(win / kCellBytes), a.prefilter,
                                        !pl->cs, &pl->d_ctr->candidates, st));
        HIPCHK(hipMemcpyAsync(pl->h_ctr, pl->d_ctr, sizeof(Counters), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        pl->dma_pass_rate = (double)pl->h_ctr->candidates / (double)(2 * win / kCellBytes);
        pl->dma_off = pl->dma_pass_rate > max_pass;
        pl->dma_off_text = w.d_text;
        pl->dma_off_len = w.text_len;
        if (getenv("KREP_GPU_DEBUG"))
            fprintf(stderr, "krep-gpu: literal scan: the prefilter's byte 0x%02x occurs in %.1f %% of the sampled 1-KiB cells -> %s kernel\n", a.prefilter & 0xffu,
                    100.0 * pl->dma_pass_rate, pl->dma_off ? "register" : "LDS-DMA");
    }
    if (pl->dma_off && !L.dma_keep)
    {
        a.prefilter = 0u; // (kg_literal_dma.hip literal_dma_eligible: the register kernel)
        a.upt = tickets_for(false);
    }
    if (const char *e = getenv("KREP_GPU_LIT_UPT")) // measurement aid; only the values the kernel's parked-store bookkeeping
    {                                               // is built for (kPark = 240 must be a multiple)
        const int v = atoi(e);
        if (v == 0 || v == 1 || v == 2 || v == 4 || v == 8)
            a.upt = (uint32_t)v;
    }
    return 0;
}
// what the LDS-DMA kernel itself counted on this text (behind a scan): its later scans go by it
static void lit_dma_rate(krep_gpu_plan *pl, const Window &w, const LitScan &L)
{
    if (!literal_dma_eligible(L.a) || L.span() < (64ull << 20))
        return;
    pl->dma_pass_rate = (double)pl->h_ctr->candidates / ((double)L.span() / kCellBytes);
    if (pl->dma_pass_rate > lit_dma_max_pass() && !L.dma_keep)
    {
        pl->dma_off = true;
        pl->dma_off_text = w.d_text;
        pl->dma_off_len = w.text_len;
        if (getenv("KREP_GPU_DEBUG"))
            fprintf(stderr, "krep-gpu: literal scan: the prefilter passed %.1f %% of the 1-KiB cells -> the register kernel from the next scan on\n", 100.0 * pl->dma_pass_rate);
    }
}

// ---- the FIRST records scan of a plan on a large text: one cheap look before the full launch (round 6).  A plan
// used to learn the density of its text from whole scans — the two-pass road first, the one-pass writers and their ring shape
// from the third or fourth scan on (`-i Sh`: 4222 / 4886 / 5026 / 5097 GB/s in four consecutive scans), which a CLI process,
// making ONE scan, never reached.  Two 2-MiB windows are counted (~0.1 ms next to >= 0.16 ms of scan) and the road, the ring shape
// and the staging slot are chosen from that; every later scan re-evaluates them as before.
static int lit_first_look(krep_gpu_plan *pl, const LitPass &ps, LitScan &L, hipStream_t st)
{
    LitArgs &a = L.a;
    const uint32_t m_scan = a.m;
    if (!(ps.sink == LitPass::RECORDS && !pl->first_look_done && a.rounds == kRoundsBig && L.fsc == 0 && !ps.first_byte && !ps.lines &&
          ps.excl_lo == ps.excl_hi && L.span() >= (1ull << 30) && !getenv("KREP_GPU_NO_FIRST_LOOK")))
        return 0;
    pl->first_look_done = true;
    const uint64_t span = L.span(), win = 2ull << 20, tile_bytes = (uint64_t)kRoundsBig * kSegBytes * kWavesPerBlk;
    HIPCHK(hipMemsetAsync(pl->d_ctr, 0, sizeof(Counters), st));
    uint64_t looked = 0;
    for (int q = 0; q < 2; ++q)
    {
        LitArgs sm = a;
        sm.flags &= ~(uint32_t)(F_POS | F_LINES);
        sm.stage_cap = 0;
        sm.upt = 0;
        sm.emit_mode = 0;
        sm.own_lo = (a.anchor + span / 4 * (2 * q + 1)) & ~(uint64_t)15;
        sm.own_hi = std::min<uint64_t>(L.hi_match, sm.own_lo + win);
        sm.anchor = sm.own_lo;
        sm.num_tiles = (sm.own_hi - sm.anchor + tile_bytes - 1) / tile_bytes;
        looked += sm.own_hi - sm.own_lo;
        HIPCHK(launch_literal(sm, (uint32_t)pl->num_cu, st));
    }
    HIPCHK(hipMemcpyAsync(pl->h_ctr, pl->d_ctr, sizeof(Counters), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    const double density = looked ? (double)pl->h_ctr->total / (double)looked : 0.0, per_unit = density * 32768.0;
    pl->lit_density = density;
    if (m_scan == 1)
    {
        if (density > single_fused_max_density(kFusedShapeMax))
            pl->fused1_ok = false;
        else
            pl->fused1_shape = single_fused_shape_for(density, 1.05, 0);
    }
    else if (m_scan <= 8 && !pl->fusedk_never && per_unit >= fusedk_min_hits_per_unit() &&
             density <= single_fused_max_density(kFusedShapeMax))
    {
        pl->fusedk_on = true;
        pl->fusedk_shape = single_fused_shape_for(density, 1.05, 0);
    }
    else if (per_unit > 6.0) // the staging road with slots that hold what a unit holds (what a whole scan used to find out)
        pl->sparse_cap = std::max<uint32_t>(pl->sparse_cap, per_unit > 100.0 ? 256u : per_unit > 40.0 ? 128u : 64u);
    if (getenv("KREP_GPU_DEBUG"))
        fprintf(stderr, "krep-gpu: first look: %.2f hits per 32-KiB unit in %llu sampled bytes -> one-pass %d (shape %d / %d), staging slot %u\n", per_unit,
                (unsigned long long)looked, (int)(m_scan == 1 ? pl->fused1_ok : pl->fusedk_on), pl->fused1_shape, pl->fusedk_shape, pl->sparse_cap);
    if ((a.flags & F_POS) && !L.fsc)
        a.stage_cap = a.rounds == kRoundsBig ? (m_scan == 1 ? 512u : pl->sparse_cap) : a.stage_cap;
    return 0;
}

// ---- single byte with records (memchr_search, BASELINE config 3): ONE pass, the records written by the scanning waves
// at their final index (kg_single.hip) — no staging, no info words, no post-pass.  A scan too dense for the rings of its
// shape is counted but not recorded: the count picks the shape that holds it (up to ~20 % hits) and the scan runs again in
// that shape — the plan keeps it; beyond that the two-pass kernels take this scan and the plan's later ones.
// The same kernel takes a literal of 2..8 bytes (its MULTI instantiations) once a two-pass scan of the plan has counted a
// density at which the staging slots of the sparse kinds overflow (`-i sh`: 35 hits per unit; ` a`: 180): pl->fusedk_on.
// *done: the scan is complete (else the two-pass road takes it).
static int lit_one_pass(krep_gpu_plan *pl, const Window &w, const LitPass &ps, LitScan &L, hipStream_t st, LitResult *res, bool *done)
{
    LitArgs &a = L.a;
    const uint32_t m_scan = a.m;
    *done = false;
    const bool fusedk = m_scan >= 2 && m_scan <= 8 && pl->fusedk_on;
    // (-w: the 2..8-byte instantiations test it in registers since round 6; the single-byte ones do not build the window it needs)
    if (!((m_scan == 1 ? pl->fused1_ok : fusedk) && ps.sink == LitPass::RECORDS && !(ps.ww && m_scan == 1) && !ps.lines && !ps.first_byte &&
          a.rounds == kRoundsBig && L.fsc == 0 && ps.excl_lo == ps.excl_hi && w.text_len >= 2 * (size_t)kSegBytes &&
          !getenv("KREP_GPU_NO_FUSED1")))
        return 0;
    a.positions = ps.d_out;
    a.pos_cap = ps.out_cap;
    int &plan_shape = m_scan == 1 ? pl->fused1_shape : pl->fusedk_shape;
    const int rc = single_fused_run(a, L.n_units, L.span(), *ps.post, pl->d_ctr, pl->h_ctr, (uint32_t)pl->num_cu, &plan_shape, ps.ev_end, st,
                                    true);
    if (rc == 2)
        return 2;
    if (rc != kFusedGaveUp)
    {
        res->total = pl->h_ctr->total;
        res->summary = res->total ? (kLnHead | kLnTail) : 0;
        if (m_scan != 1 && L.density(res->total) * 32768.0 < 0.5 * fusedk_min_hits_per_unit())
            pl->fusedk_on = false; // (a sparser text: the staging road is faster there)
        *done = true;
        return 0;
    }
    if (m_scan == 1)
        pl->fused1_ok = false;
    else
        pl->fusedk_on = false, pl->fusedk_never = true;
    g_fused1_failovers.fetch_add(1);
    return 0;
}

// behind a two-pass scan into records or counts: the plan's staging slot and its one-pass road from the counted density
static void lit_learn_density(krep_gpu_plan *pl, const LitPass &ps, const LitScan &L)
{
    const LitArgs &a = L.a;
    const uint32_t m_scan = a.m;
    if (L.span() >= 8 * L.unit_bytes() && !ps.first_byte) // (a window shorter than a ticket says nothing about the text)
        pl->lit_density = L.density(pl->h_ctr->total);
    if ((a.flags & F_POS) && m_scan != 1 && a.rounds == kRoundsBig && pl->h_ctr->overflow_units * 64 > L.n_units && !L.fsc)
    {
        // a dense input: the next scans of this plan stage 64 hits per unit — and if more than 1 unit in 64 overflows that as
        // well (`-i sh`: 36 hits per unit on average, clustered), as many as the fullest unit held, up to 256: re-scanning
        // 5 % of the units cold cost m = 2 -i a fifth of its time
        uint32_t want = 64;
        if (pl->sparse_cap >= 64)
            for (want = 128; want < 256 && want < pl->h_ctr->max_unit_count; want *= 2) {}
        pl->sparse_cap = std::max(pl->sparse_cap, want);
    }
    if ((a.flags & F_POS) && m_scan >= 2 && m_scan <= 8 && a.rounds == kRoundsBig && !L.fsc && !pl->fusedk_never &&
        ps.sink == LitPass::RECORDS && !ps.lines && L.hi_match > a.anchor)
    {
        // dense enough for the one-pass record writer (kg_single.hip, MULTI)?  Its shape from the density just counted.
        const double density = L.density(pl->h_ctr->total);
        if (density * 32768.0 >= fusedk_min_hits_per_unit() && density <= single_fused_max_density(kFusedShapeMax))
        {
            pl->fusedk_on = true;
            pl->fusedk_shape = single_fused_shape_for(density, 1.0, 0);
        }
    }
    if (getenv("KREP_GPU_DEBUG") && (a.flags & F_POS))
        fprintf(stderr, "krep-gpu: literal scan: %llu of %llu units overflowed a %u-entry slot (fullest: %llu); one-pass next: %d (shape %d)\n",
                pl->h_ctr->overflow_units, (unsigned long long)L.n_units, a.stage_cap, pl->h_ctr->max_unit_count, (int)pl->fusedk_on,
                pl->fusedk_shape);
}
// behind every two-pass scan: a later, sparser text of the same plan takes the one-pass kernel again (the 2..8-byte
// instantiations as well: one overflowing text no longer bars them for good)
static void lit_reopen(krep_gpu_plan *pl, const LitScan &L)
{
    const uint32_t m_scan = L.a.m;
    if (!pl->fused1_ok && m_scan == 1 && single_fused_reopens(pl->h_ctr->total, L.span()))
        pl->fused1_ok = true;
    if (pl->fusedk_never && m_scan >= 2 && m_scan <= 8 && single_fused_reopens(pl->h_ctr->total, L.span()))
        pl->fusedk_never = false;
}

// ---- records of a SPARSE 2..8-byte literal on a ticketed text (BASELINE config 2: 3.3 hits per 32-KiB unit): the LDS-DMA kernel in its
// one-pass mode (kg_literal_dma.hip ONEP) — the scanning waves write the records at their final index through the ticket -> resolver ->
// deferred-store scheme of kg_tickets.h, so there are no info words, no staging slots and no ordering post-pass: on the stream, one
// memset (the counters and the ticket arrays lie in one block of post.d_tk), the launch, the end event, the read-back of the counters.
// A ticket with more hits than a wave's list holds (or the spin-limit safety net) raises overflow_units: the two-pass road takes this
// scan and the plan's later ones on this text (with long tickets in the map: shorter ones first).  *done: the scan is complete.
static int lit_dma_one_pass(krep_gpu_plan *pl, const Window &w, const LitPass &ps, LitScan &L, hipStream_t st, LitResult *res, bool *done)
{
    *done = false;
    // ($KREP_GPU_LIT_DMA_TWO_PASS is read per launch: the A/B tools flip it inside one process; the two switches below are the tests', flipped
    //  per test like literal_dma_eligible()'s, and are only looked at on a text below the ticketed range)
    if (!(ps.sink == LitPass::RECORDS && !ps.lines && !ps.first_byte && ps.excl_lo == ps.excl_hi && L.fsc == 0 && !getenv("KREP_GPU_LIT_DMA_TWO_PASS")))
        return 0;
    LitArgs a = L.a;
    if (!a.upt && getenv("KREP_GPU_LIT_DMA_ALL") && !getenv("KREP_GPU_LIT_UPT"))
        a.upt = 8; // (the tests' switch on a text below the ticketed range: this mode needs tickets from one counter)
    const char *upt_env = getenv("KREP_GPU_LIT_UPT");
    if (upt_env) // measurement aid, wider on this road than in lit_dma_look: the one-pass mode parks no units, so EVERY ticket takes 16 or 32
    {            // units as well (profiles/r08_ticket_size.txt); with the switch set, whatever its value, the map has one size
        const int v = atoi(upt_env);
        if (a.upt && (v == 16 || v == 32))
            a.upt = (uint32_t)v;
    }
    if (!a.upt || !literal_dma_eligible(a) || L.n_units >= (1ull << 32))
        return 0;
    if (pl->dma1p_off && pl->dma1p_off_text == (const void *)w.d_text && pl->dma1p_off_len == w.text_len)
        return 0;
    const uint64_t ticket_bytes = (uint64_t)a.upt * L.unit_bytes();
    // the gate, in hits per ticket: a quarter of the list, and never above the density from which the one-pass writers of kg_single.hip
    // take such a literal (fusedk_min_hits_per_unit) — this road does not run lit_learn_density(), so a text at or above the gate has to
    // reach the two-pass road, which switches them on (the defaults coincide: 768 / 4 = 24 x 8)
    const double gate = std::min(0.25 * (double)lit_dma_one_pass_list(), fusedk_min_hits_per_unit() * (double)a.upt);
    if (pl->lit_density >= 0.0 && pl->lit_density * (double)ticket_bytes >= gate)
        return 0;
    // Long tickets for the bulk of the text, today's for its end (kg_tickets.h TkMap): a wave crosses a seam — the ticket draw it has to wait
    // for, the tail piece, the count, the parked entry — a quarter as often, and the kernel's end stays graded by short tickets.  How long:
    // the largest of 32, 16 or 8 units at which the density the plan knows keeps a ticket at or under a quarter of the list (BASELINE's 105 hits
    // per MiB: 32); a plan that knows no density yet scans with 8.  The list's rule under them (kg_literal_dma.hip end_ticket): a flush leaves
    // at most the ticket that has just ended in the list, so the ticket being scanned has list_size - max(list_size / 2, hits of the one
    // before it) entries free — half the list unless a ticket held twice the gate, and a ticket denser than that is counted, not recorded.
    // How many: tk_map_long_tickets().  A long ticket that overflowed halves the plan's long ticket for this text (below).
    const bool long_text = pl->dma1p_long_text == (const void *)w.d_text && pl->dma1p_long_len == w.text_len;
    uint32_t upt_long = a.upt;
    if (!upt_env && a.upt == 8)
    {
        if (g_lit_dma1p_force_long) // (test hook)
            upt_long = (uint32_t)g_lit_dma1p_force_long;
        else if (pl->lit_density >= 0.0)
            for (uint32_t v = 32; v > a.upt && upt_long == a.upt; v >>= 1)
                if (pl->lit_density * (double)v * (double)L.unit_bytes() <= 0.25 * (double)lit_dma_one_pass_list())
                    upt_long = v;
        upt_long = std::min(upt_long, long_text ? std::max(pl->dma1p_long_max, a.upt) : 32u);
    }
    TkMap tk = {0u, a.upt, 0ull};
    if (upt_long > a.upt)
    {
        const uint64_t waves = (uint64_t)lit_dma_one_pass_grid(a, (uint32_t)pl->num_cu) * kWavesPerBlk;
        tk.n_long = g_lit_dma1p_force_long ? std::min<uint64_t>(g_lit_dma1p_force_n_long, L.n_units / upt_long)
                                           : tk_map_long_tickets(L.n_units, upt_long, a.upt, waves);
    }
    tk.upt_long = tk.n_long ? upt_long : 0u;
    if (getenv("KREP_GPU_DEBUG"))
        fprintf(stderr, "krep-gpu: literal scan, one pass: %llu units in %llu tickets of %u and the rest in tickets of %u\n", (unsigned long long)L.n_units,
                (unsigned long long)tk.n_long, tk.upt_long, tk.upt);
    // [Counters (16 words) | counts | prefixes]: one block, one memset
    constexpr uint64_t kCtrWords = 16;
    static_assert(sizeof(Counters) <= kCtrWords * sizeof(unsigned long long), "the counters in front of the ticket arrays");
    const uint64_t n_tk = tk_map_tickets(tk, L.n_units), cap_tk = n_tk + kCtrWords / 2;
    PostScratch &post = *ps.post;
    HIPCHK(grow_scratch(post.tk_cap, cap_tk, cap_tk, {dev_buf(post.d_tk, 2 * cap_tk * sizeof(unsigned long long))}));
    Counters *d_ctr = reinterpret_cast<Counters *>(post.d_tk);
    unsigned long long *d_agg = post.d_tk + kCtrWords, *d_pref = d_agg + n_tk;
    a.ctr = d_ctr;
    a.positions = ps.d_out;
    a.pos_cap = ps.out_cap;
    a.stage_cap = 0;
    HIPCHK(hipMemsetAsync(post.d_tk, 0, (kCtrWords + 2 * n_tk) * sizeof(unsigned long long), st));
    HIPCHK(launch_literal_dma_one_pass(a, tk, d_agg, d_pref, n_tk, (uint32_t)pl->num_cu, st));
    if (ps.ev_end) HIPCHK(hipEventRecord(ps.ev_end, st));
    HIPCHK(hipMemcpyAsync(pl->h_ctr, d_ctr, sizeof(Counters), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    LitScan La = L;
    La.a = a;
    lit_dma_rate(pl, w, La);
    if (pl->h_ctr->overflow_units)
    {
        if (tk.n_long)
        {
            // (the kernel does not say which ticket it was: with long tickets in the map the long ones are the first suspects — half as long
            //  on the plan's next scan of this text, the road itself barred only once an all-short map has overflowed too)
            pl->dma1p_long_max = tk.upt_long / 2;
            pl->dma1p_long_text = w.d_text;
            pl->dma1p_long_len = w.text_len;
        }
        else
        {
            pl->dma1p_off = true;
            pl->dma1p_off_text = w.d_text;
            pl->dma1p_off_len = w.text_len;
        }
        g_lit_dma1p_failovers.fetch_add(1);
        if (getenv("KREP_GPU_DEBUG"))
            fprintf(stderr, "krep-gpu: literal scan: a ticket overflowed the one-pass hit list -> the two-pass road for this %s\n",
                    tk.n_long ? "scan, shorter long tickets for this text" : "text");
        return 0;
    }
    if (L.span() >= ticket_bytes)
        pl->lit_density = L.density(pl->h_ctr->total);
    res->total = pl->h_ctr->total;
    res->summary = res->total ? (kLnHead | kLnTail) : 0;
    *done = true;
    return 0;
}

// ---- the two-pass road into records or counts: the scan (kg_literal.hip / kg_literal_dma.hip), the ordering post-pass
// (kg_post.hip) behind it, and an emit-mode re-scan of the units whose hits overflowed their staging slot
static int lit_two_pass(krep_gpu_plan *pl, const Window &w, const LitPass &ps, LitScan &L, bool chain, hipStream_t st)
{
    LitArgs &a = L.a;
    a.positions = ps.d_out;
    a.pos_cap = ps.sink == LitPass::RECORDS ? ps.out_cap : 0;
    HIPCHK(launch_literal(a, (uint32_t)pl->num_cu, st));
    if (chain && post_order(*ps.post, L.n_units, a.stage_cap, a.m, a.anchor + w.global_base, L.unit_bytes(), ps.lines, ps.d_out, a.pos_cap,
                            pl->d_ctr, pl->num_cu, st))
        return 2;
    if (ps.ev_end) HIPCHK(hipEventRecord(ps.ev_end, st));
    HIPCHK(hipMemcpyAsync(pl->h_ctr, pl->d_ctr, sizeof(Counters), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    lit_dma_rate(pl, w, L);
    lit_learn_density(pl, ps, L);
    if ((a.flags & F_POS) && pl->h_ctr->overflow_units)
    {
        // some units held more hits than their staging slot: re-scan exactly those, writing in place
        LitArgs e = a;
        e.emit_mode = 1;
        HIPCHK(hipMemsetAsync(&pl->d_ctr->ticket, 0, sizeof(unsigned long long), st));
        HIPCHK(launch_literal(e, (uint32_t)pl->num_cu, st));
        if (ps.ev_end) HIPCHK(hipEventRecord(ps.ev_end, st));
    }
    return 0;
}
// ---- the two-pass road into the occurrence list: all owned hits into post.d_occ (sized after the count is known), the input of
// the sequential-family walks
static int lit_two_pass_occ(krep_gpu_plan *pl, const Window &w, const LitPass &ps, const LitScan &L, hipStream_t st)
{
    const LitArgs &a = L.a;
    PostScratch &post = *ps.post;
    HIPCHK(launch_literal(a, (uint32_t)pl->num_cu, st));
    if (post_offsets_pass(post, L.n_units, false, pl->d_ctr, st))
        return 2;
    HIPCHK(hipMemcpyAsync(pl->h_ctr, pl->d_ctr, sizeof(Counters), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    const uint64_t n_occ = pl->h_ctr->total;
    HIPCHK(grow_scratch(post.occ_cap, n_occ, n_occ, {dev_buf(post.d_occ, n_occ * 2 * sizeof(uint64_t))}));
    if (n_occ)
    {
        if (post_gather_pass(post, L.n_units, a.stage_cap, a.m, a.anchor + w.global_base, L.unit_bytes(), post.d_occ, n_occ, pl->num_cu, st))
            return 2;
        if (pl->h_ctr->overflow_units)
        {
            LitArgs e = a;
            e.emit_mode = 1;
            e.positions = post.d_occ;
            e.pos_cap = n_occ;
            HIPCHK(hipMemsetAsync(&pl->d_ctr->ticket, 0, sizeof(unsigned long long), st));
            HIPCHK(launch_literal(e, (uint32_t)pl->num_cu, st));
        }
    }
    return 0;
}

// one pass of the literal kernel family over the window, with its ordering post-pass
static int lit_pass(krep_gpu_plan *pl, const Window &w, const LitPass &ps, hipStream_t st, LitResult *res)
{
    *res = LitResult{};
    const uint32_t m_scan = ps.first_byte ? 1u : pl->m;
    size_t own_hi = std::min(ps.own_hi, w.text_len);
    if (ps.first_byte)
        own_hi = std::min<size_t>(own_hi, w.text_len - pl->m + 1);
    const uint64_t hi_match = std::min<uint64_t>(own_hi, w.text_len - m_scan + 1);
    if (hi_match <= ps.own_lo)
        return 0;
    LitScan L = lit_args(pl, w, ps, own_hi, hi_match);
    if (lit_dma_look(pl, w, ps, L, st))
        return 2;
    res->n_units = L.n_units;
    res->unit_bytes = L.unit_bytes();
    res->anchor = L.a.anchor;
    bool done = false;
    if (lit_first_look(pl, ps, L, st) || lit_one_pass(pl, w, ps, L, st, res, &done))
        return 2;
    if (done)
        return 0;
    if (lit_dma_one_pass(pl, w, ps, L, st, res, &done))
        return 2;
    if (done)
        return 0;
    const bool chain = (L.a.flags & (F_POS | F_LINES)) != 0;
    if (chain)
    {
        PostScratch &post = *ps.post;
        if (post_reserve(post, L.n_units, (L.n_units * L.a.stage_cap + 3) / 4)) // 16-bit staging entries
            return 2;
        L.a.unitinfo = post.d_unitinfo;
        L.a.stage = (uint64_t *)post.d_stage;
        L.a.offsets = (const uint64_t *)post.d_offsets;
    }
    HIPCHK(hipMemsetAsync(pl->d_ctr, 0, sizeof(Counters), st));
    if (ps.sink != LitPass::OCC ? lit_two_pass(pl, w, ps, L, chain, st) : lit_two_pass_occ(pl, w, ps, L, st))
        return 2;
    res->total = pl->h_ctr->total;
    res->lines = pl->h_ctr->lines;
    lit_reopen(pl, L);
    res->summary = chain ? pl->h_ctr->summary : (res->total ? (kLnHead | kLnTail) : 0);
    return 0;
}

// ---- match-set family of the reference algorithm being reproduced -----------------------------------------------
namespace {
struct Family
{
    bool greedy = false;    // greedy leftmost non-overlapping occurrences (SSE4.2 / KMP; BMH under -o)
    bool mshort_o = false;  // memchr_short_search under -o: candidate walk
    bool need_walk = false; // a sequential pass over the ordered list is required (kg_greedy.hip)
    bool replay = false;    // -c through a block-structured function: end-of-text replay (kg_replay.h)
    bool neon_zero = false; // neon_search, count-only, max_count == 0 (tail-call convention)
    bool nlwalk = false;    // -c through simd_sse42_search / kmp_search with a '\n' inside the pattern (kg_greedy.hip (3))
    bool whole_text() const { return need_walk || replay || neon_zero || nlwalk; } // cannot be scanned in independent pieces
};
Family family_of(int algo, bool only_matching, bool lines, bool ww, bool track, size_t maxc, bool has_border, uint32_t m,
                 bool pat_has_newline = false)
{
    Family f;
    if (lines && pat_has_newline && (algo == KREP_RA_SSE42 || algo == KREP_RA_KMP))
    {
        f.nlwalk = true; // the line jump lands inside the match: a chain over every visited match, nothing else applies
        return f;
    }
    f.greedy = (algo == KREP_RA_SSE42 || algo == KREP_RA_KMP);
    if (only_matching)
    {
        if (algo == KREP_RA_SSE42)
            f.greedy = false; // -o: advance = index + 1 (krep.c:4842), in every mode
        else if (algo == KREP_RA_BMH && !lines)
            f.greedy = true; // -o without -c: i += pattern_len after a hit (krep.c:1371)
        else if (algo == KREP_RA_MEMCHR_SHORT)
            f.mshort_o = true; // -o: advance = candidate + pattern_len, also after a FAILED candidate (krep.c:4495)
    }
    f.need_walk = (f.greedy && has_border && m > 1) || f.mshort_o;
    // without -w a line holds a greedy hit iff it holds any occurrence (a line's first occurrence heads a cluster),
    // so plain -c needs no selection pass
    if (f.need_walk && !f.mshort_o && lines && !ww)
        f.need_walk = false;
    f.replay = lines && (algo == KREP_RA_AVX512 || algo == KREP_RA_NEON || (algo == KREP_RA_AVX2 && ww));
    f.neon_zero = algo == KREP_RA_NEON && maxc == 0 && !lines && !track;
    return f;
}
} // namespace
namespace kg {
// How may the text be cut?  kSplitPieces: independent pieces (start-offset ownership + halo) whose results merge.
// kSplitChain: pieces in text order, each taking the boundary record of the one before it (the greedy / -o walks: where the
// reference's scan stands; -c through simd_avx512_search / simd_avx2_search -w: the line-skip history the end-of-text replay
// needs, for neon_search with its grid origin; multi-pattern -c with a '\n' inside a pattern: newlines so far and the line of
// the last match — krep_gpu_seq_carry_t).  kSplitWhole: one window only — the newline-pattern -c walk of kg_greedy.hip (3),
// neon_search's max_count == 0 corner, a regex that can overlap itself without -c.
int split_mode(const search_params_t *p, const krep_gpu_config_t &c, size_t text_len)
{
    if (!p || (!p->use_regex && p->num_patterns == 0))
        return kSplitWhole;
    if (p->use_regex)
    { // a pattern that can overlap itself (an alternation: two occurrences that can share a byte) goes through the greedy pass over
      // the whole occurrence list; -c never does (kg_regex.hip, kg_regex_alt.hip)
        RegexCompiled rc;
        if (regex_compile_cached(p, &rc))
            return kSplitWhole;
        if (rc.line_walked()) // a match lies inside one line of at most 4096 bytes: pieces with that much context on both sides, once
                         // krep_gpu_set_regex_loops_windows() says so; else one window over the whole text (kg_regex_loops.hip)
            return g_regex_loops_windows.load(std::memory_order_relaxed) ? kSplitPieces : kSplitWhole;
        return rc.overlaps() && !p->count_lines_mode ? kSplitWhole : kSplitPieces;
    }
    if (p->num_patterns > 1)
    {
        if (!p->count_lines_mode)
            return kSplitPieces;
        for (size_t i = 0; i < p->num_patterns; ++i)
            if (p->pattern_lens[i] && memchr(p->patterns[i], '\n', p->pattern_lens[i]))
                return kSplitChain; // emission-order line changes: pieces owned by END, chained by (newlines, last line) — round 5
        return kSplitPieces;
    }
    const char *pat = p->patterns && p->pattern_lens ? p->patterns[0] : p->pattern;
    const size_t m = p->patterns && p->pattern_lens ? p->pattern_lens[0] : p->pattern_len;
    if (!pat || m == 0)
        return kSplitPieces;
    search_params_t q = *p;
    q.pattern = pat;
    q.pattern_len = m;
    const int algo = mirror_effective(mirror_top(&q, c), &q, text_len);
    std::vector<uint8_t> f((const uint8_t *)pat, (const uint8_t *)pat + m);
    if (!p->case_sensitive)
        for (auto &b : f)
            b = lo8(b);
    const Family fam = family_of(algo, c.only_matching != 0, p->count_lines_mode, p->whole_word, p->track_positions, p->max_count,
                                 pattern_has_border(f.data(), m), (uint32_t)m, memchr(pat, '\n', m) != nullptr);
    if (fam.neon_zero || (fam.mshort_o && p->count_lines_mode))
        return kSplitWhole; // (the second: a class krep's main() never produces, krep.c:3811-3814 — one window, no boundary record)
    return (fam.need_walk || fam.replay || fam.nlwalk) ? kSplitChain : kSplitPieces;
}
bool shardable(const search_params_t *p, const krep_gpu_config_t &c, size_t text_len) { return split_mode(p, c, text_len) != kSplitWhole; }
// The left fold of the boundary record (include/krep_gpu.h, krep_gpu_seq_carry_t): used by a piece that knows its predecessor's
// record, and by the host after shards were scanned out of order.
krep_gpu_seq_carry_t fold_carry(const krep_gpu_seq_carry_t &in, const krep_gpu_seq_carry_t &pc)
{
    krep_gpu_seq_carry_t o = pc; // keeps the piece's local_* fields
    o.resume = std::max<uint64_t>(in.resume, pc.resume);
    // multi-pattern -c with a newline inside a pattern: newlines so far, line of the last match's start (include/krep_gpu.h)
    o.nl_before = in.nl_before + pc.local_nl;
    o.last_line = pc.local_last ? in.nl_before + 1ull + (pc.local_last - (1ull << 62)) : in.last_line;
    if (!pc.local_q1)
    {
        o.q1 = in.q1;
        o.nl1 = in.nl1 ? in.nl1 : in.q1 ? pc.local_first_nl1 : 0;
        o.g0 = in.g0;
        return o;
    }
    o.q1 = pc.local_q1;
    o.nl1 = pc.local_nl1;
    switch (pc.local_g0_kind)
    {
    case 1: o.g0 = pc.local_g0; break;
    case 2: o.g0 = in.q1 ? (in.nl1 ? in.nl1 : pc.local_first_nl1) : 0; break; // nl1 is stored + 1: it IS the next line start
    case 3: o.g0 = in.q1 ? (in.nl1 ? in.nl1 : in.g0) : 0; break;
    default: o.g0 = 0;
    }
    return o;
}
} // namespace kg
extern "C" void krep_gpu_debug_fold_carry(const krep_gpu_seq_carry_t *in, const krep_gpu_seq_carry_t *piece, krep_gpu_seq_carry_t *out)
{
    if (in && piece && out)
        *out = kg::fold_carry(*in, *piece);
}
extern "C" int krep_gpu_split_mode(const search_params_t *p, size_t text_len)
{
    return kg::split_mode(p, kg::current_config(), text_len);
}

int kg::nl_reserve(krep_gpu_plan *pl, uint64_t need, uint64_t want, bool with_ln)
{
    HIPCHK(grow_scratch(pl->nl_cap, need, want,
                        {dev_buf(pl->d_nl_rec, want * sizeof(match_position_t)), dev_buf(pl->d_nl_ln, with_ln ? want * sizeof(uint64_t) : 0)}));
    if (with_ln && !pl->d_nl_ln)
        HIPCHK(hipMalloc(&pl->d_nl_ln, pl->nl_cap * sizeof(uint64_t)));
    return 0;
}

// Where the reference's block loop stands when it enters the last kReplayWindow bytes (kg_replay.h): `cur`, and for
// neon_search whether the (unterminated) line holding `cur` is already counted.  Uses the per-unit info words the
// canonical -c pass over [0, X) just left in pl->post.
// last accepted occurrence with (buffer-relative) start < limit among the starts the canonical -c pass `lr` covered: the last
// unit reporting hits in its info word, re-scanned with records (pl->aux)
static int last_accepted_before(krep_gpu_plan *pl, const Window &w, const LitResult &lr, uint64_t own_lo, uint64_t limit,
                                hipStream_t st, bool *found, uint64_t *q)
{
    unsigned long long *d_slot = &pl->d_ctr->pad[0], *h_slot = &pl->h_ctr->pad[0];
    *found = false;
    if (limit <= lr.anchor || lr.n_units == 0)
        return 0;
    uint64_t lim_units = std::min<uint64_t>(lr.n_units, (limit - lr.anchor + lr.unit_bytes - 1) / lr.unit_bytes);
    while (lim_units)
    {
        uint64_t up1 = 0;
        if (tail_last_hit(pl->post.d_unitinfo, lim_units, d_slot, h_slot, st, &up1))
            return 2;
        if (!up1)
            return 0;
        const uint64_t u = up1 - 1, ulo = lr.anchor + u * lr.unit_bytes;
        LitPass ps;
        ps.ww = pl->ww;
        ps.own_lo = std::max<uint64_t>(ulo, own_lo);
        ps.own_hi = std::min<uint64_t>(ulo + lr.unit_bytes, limit);
        ps.sink = LitPass::OCC;
        ps.post = &pl->aux;
        LitResult r2;
        if (lit_pass(pl, w, ps, st, &r2))
            return 2;
        if (r2.total)
        {
            uint64_t rec[2];
            HIPCHK(hipMemcpy(rec, pl->aux.d_occ + 2 * (r2.total - 1), sizeof rec, hipMemcpyDeviceToHost));
            *found = true;
            *q = rec[0] - w.global_base;
            return 0;
        }
        lim_units = u; // every hit of that unit starts at or after `limit`: look further left
    }
    return 0;
}

// The end-of-text replay of a PIECE: where the reference's block loop stands when it enters the last kReplayWindow bytes follows
// from the folded boundary record alone (global offsets, stored + 1); `text_g` is indexed with global offsets.
// (`text_g` is a DEVICE address rebased so that it can be indexed with global offsets; the first global offset really held is text_lo.
//  The rebasing is integer arithmetic on the address — no pointer outside an object is formed on the host)
static const uint8_t *rebased(const void *d_held, uint64_t held_from)
{
    return reinterpret_cast<const uint8_t *>(reinterpret_cast<uintptr_t>(d_held) - (uintptr_t)held_from);
}
static int replay_from_record(krep_gpu_plan *pl, int algo, const krep_gpu_seq_carry_t &co, const uint8_t *text_g, uint64_t text_lo, uint64_t G,
                              hipStream_t st, uint64_t *extra)
{
    *extra = 0;
    const uint64_t X = G > kReplayWindow ? G - kReplayWindow : 0, B = algo == KREP_RA_AVX512 ? 64 : algo == KREP_RA_AVX2 ? 32 : 16;
    uint64_t cur;
    int open = 0;
    if (!co.q1)
        cur = (X / B) * B; // the block grid never left offset 0
    else if (co.nl1)
        cur = co.nl1 <= X ? co.nl1 + ((X - co.nl1) / B) * B : co.nl1; // restarted at the line start behind q
    else if (algo == KREP_RA_NEON)
    {
        // no restart on an unterminated line: the previous counted line's grid (a grid origin behind X — a text shorter than the
        // replay window — is where the loop stands; ADVICE r05: the unsigned difference wrapped)
        cur = co.g0 <= X ? co.g0 + ((X - co.g0) / B) * B : co.g0;
        open = 1;
    }
    else
        cur = G; // unterminated line counted: the clamped advance ended the scan (krep.c:5006-5008, :5211-5213)
    ReplayIn r{};
    r.algo = algo; r.m = pl->m; r.ww = pl->ww; r.n = G; r.cur = cur; r.open = open;
    r.text = text_g;
    r.pat = pl->d_pat;
    if (cur < G && cur + 1 < text_lo + 1) // (the replay reads global offsets >= cur - 1: they have to lie in what the caller holds)
        return kg::fail("end-of-text replay: the loop stands at %llu, in front of the bytes held (from %llu)", (unsigned long long)cur, (unsigned long long)text_lo);
    if (cur < G && tail_run_replay(r, &pl->d_ctr->pad[0], &pl->h_ctr->pad[0], st, extra))
        return 2;
    return 0;
}

static int replay_entry(krep_gpu_plan *pl, int algo, const Window &w, const LitResult &lr, uint64_t X, hipStream_t st,
                        uint64_t *cur_out, int *open_out)
{
    const uint64_t n = w.text_len, B = algo == KREP_RA_AVX512 ? 64 : algo == KREP_RA_AVX2 ? 32 : 16;
    unsigned long long *d_slot = &pl->d_ctr->pad[0], *h_slot = &pl->h_ctr->pad[0];
    auto last_accepted_before = [&](uint64_t limit, bool *found, uint64_t *q) -> int {
        return ::last_accepted_before(pl, w, lr, 0, limit, st, found, q);
    };
    bool have_q = false;
    uint64_t q = 0;
    if (last_accepted_before(X, &have_q, &q))
        return 2;
    *open_out = 0;
    if (!have_q)
    {
        *cur_out = (X / B) * B; // the block grid never left offset 0
        return 0;
    }
    uint64_t nl = n;
    if (tail_find_next_newline(w.d_text, q, n, d_slot, h_slot, st, &nl))
        return 2;
    if (nl < n)
    {
        const uint64_t nls = nl + 1; // the loop restarted here after counting q's line
        *cur_out = nls <= X ? nls + ((X - nls) / B) * B : nls;
        return 0;
    }
    if (algo != KREP_RA_NEON)
    {
        *cur_out = n; // unterminated line counted: the clamped advance ends the scan (krep.c:5006-5008, :5211-5213)
        return 0;
    }
    // neon_search does not restart on an unterminated line: the grid is still the one set by the previous counted line
    uint64_t lsp1 = 0;
    if (tail_find_prev_newline(w.d_text, q, d_slot, h_slot, st, &lsp1))
        return 2;
    const uint64_t ls = lsp1; // start of q's line (0 when no '\n' precedes it)
    bool have_q2 = false;
    uint64_t q2 = 0, grid0 = 0;
    if (last_accepted_before(ls, &have_q2, &q2))
        return 2;
    if (have_q2)
    {
        uint64_t nl2 = n;
        if (tail_find_next_newline(w.d_text, q2, n, d_slot, h_slot, st, &nl2))
            return 2;
        grid0 = nl2 + 1; // <= ls
    }
    *cur_out = grid0 + ((X - grid0) / B) * B;
    *open_out = 1;
    return 0;
}

namespace {
// a single-literal scan as scan_literal hands it to the function of its family
struct LitJob
{
    krep_gpu_plan *pl;
    int algo;
    const Window &w;
    size_t own_hi;            // the ownership window's end, clipped to the buffer
    bool whole;               // the window is the whole text
    hipStream_t st;
    const krep_gpu_seq_carry_t *carry_in;
    krep_gpu_seq_carry_t *carry_out;
    match_position_t *d_pos;
    uint64_t cap, want;       // records room / records the caller can use
    uint64_t excl_lo = 0, excl_hi = 0, ww_exempt = ~0ull; // the block-structured functions' quirks (buffer-relative)
};
// what the plain, walk and replay families leave for the shared epilogue (lit_finish)
struct LitTotals
{
    uint64_t total = 0, lines = 0;
    unsigned long long summary = 0;
    bool ev1_recorded = false;
};
} // namespace

// -c through simd_sse42_search / kmp_search with a newline inside the pattern: all occurrences, the line number of every
// start, the -w verdicts — then ONE thread walks the list the way the reference's loop moves (kg_greedy.hip (3)).
// Pieces (round 5): a piece owns the occurrences that START in it; what couples it to the text in front of it is where
// the reference's scan stands (resume), the line it counted last and the newlines so far (krep_gpu_seq_carry_t).
static int lit_nlwalk(const LitJob &j, int time_it, krep_gpu_scan_out_t *out)
{
    krep_gpu_plan *pl = j.pl;
    const Window &w = j.w;
    const hipStream_t st = j.st;
    const uint32_t m = pl->m;
    const krep_gpu_seq_carry_t in = j.carry_in ? *j.carry_in : krep_gpu_seq_carry_t{};
    krep_gpu_seq_carry_t local{};
    if (!j.whole && !j.carry_in && w.global_base + w.own_lo != 0)
        return kg::fail("-c through %s with a newline inside the pattern is a chain over every counted match: scan the whole "
                        "text in one window, or its pieces in text order through krep_gpu_scan_device_seq()", krep_gpu_algorithm_name(j.algo));
    if (pl->max_count == 0)
        return 0; // krep.c:4713, :1634
    HIPCHK(hipSetDevice(pl->device));
    if (time_it) HIPCHK(hipEventRecord(pl->ev0, st));
    unsigned long long *d_slot = &pl->d_ctr->pad[0], *h_slot = &pl->h_ctr->pad[0];
    uint64_t nl_halo = 0, nl_own = 0;
    if (tail_count_newlines(w.d_text, 0, w.own_lo, d_slot, h_slot, st, &nl_halo) ||
        tail_count_newlines(w.d_text, w.own_lo, j.own_hi, d_slot, h_slot, st, &nl_own))
        return 2;
    local.local_nl = nl_own;
    LitPass ps;
    ps.own_lo = w.own_lo; ps.own_hi = j.own_hi; ps.sink = LitPass::OCC; ps.post = &pl->post;
    LitResult lr0;
    if (lit_pass(pl, w, ps, st, &lr0))
        return 2;
    uint64_t lines_counted = 0, cp_out = in.resume, seen_out = in.last_line ? in.last_line : ~0ull;
    if (lr0.total)
    {
        if (nl_reserve(pl, lr0.total, lr0.total + lr0.total / 4 + 1024, true))
            return 2;
        if (krep_gpu_line_numbers_ex(w.d_text, w.text_len, w.global_base, (const match_position_t *)pl->post.d_occ, lr0.total, pl->d_nl_ln, st))
            return 2;
        const uint32_t k0 = (uint32_t)((const uint8_t *)memchr(pl->pats[0].data(), '\n', m) - pl->pats[0].data());
        // buffer-relative line numbers (1 + newlines in [0, start)) -> global ones: + newlines in front of the buffer
        const uint64_t line_off = in.nl_before - nl_halo;
        if (post_nlwalk(pl->post, w.d_text, w.text_len, j.algo == KREP_RA_KMP ? kNlWalkKmp : kNlWalkSse42, m, k0, pl->ww,
                        pl->only_matching, pl->max_count == SIZE_MAX ? ~0ull : (uint64_t)pl->max_count, lr0.total, pl->d_nl_ln,
                        pl->d_ctr, pl->h_ctr, st, &lines_counted, w.global_base, w.global_len, line_off, in.resume,
                        in.last_line ? in.last_line : ~0ull, &cp_out, &seen_out))
            return 2;
    }
    if (time_it && stop_clock(pl, true, st, out))
        return 2;
    if (j.carry_out)
    {
        // (the line counted last, relative to own_lo and biased like the multi-pattern record's, so that fold_carry() re-bases it)
        if (seen_out != ~0ull && seen_out != (in.last_line ? in.last_line : ~0ull))
            local.local_last = (1ull << 62) + (seen_out - (in.nl_before + 1ull));
        krep_gpu_seq_carry_t o = kg::fold_carry(in, local);
        if (!local.local_last)
            o.last_line = in.last_line;
        o.resume = std::max<uint64_t>(in.resume, cp_out);
        *j.carry_out = o;
    }
    out->total_matches = lines_counted;
    out->line_count = lines_counted;
    out->has_newline = j.whole ? 0 : 1; // (pieces: krep_gpu_combine_line_counts adds the counts up, the record has settled the cuts)
    out->head_line_hit = out->tail_line_hit = j.whole ? lines_counted != 0 : 0;
    out->count = lines_counted; // the walk applies max_count the way the functions do (a break before the increment)
    return 0;
}

// -c through a block-structured function, a PIECE of the text (krep_gpu_scan_device_seq): canonical -c over the starts before the
// last kReplayWindow bytes, then the reference's own walk over the rest.  Only the piece that ends the text runs the replay; what it
// needs from the text in front of it is the line-skip history {last accepted occurrence q, first '\n' behind it}, which every piece
// extends (krep_gpu_seq_carry_t) — the piece's own contribution is reported next to the folded state, so that shards scanned out of
// order can be folded afterwards.
static int lit_replay_piece(const LitJob &j, LitTotals *t)
{
    krep_gpu_plan *pl = j.pl;
    const Window &w = j.w;
    const hipStream_t st = j.st;
    const int algo = j.algo;
    const uint64_t G = w.global_len, X = G > kReplayWindow ? G - kReplayWindow : 0;
    const uint64_t base = w.global_base, B = algo == KREP_RA_AVX512 ? 64 : algo == KREP_RA_AVX2 ? 32 : 16;
    const bool final_piece = base + j.own_hi >= G;
    if (base + w.own_lo != 0 && !j.carry_in)
        return kg::fail("-c through %s restarts its block grid at every counted line: scan the whole text in one window, "
                        "or its pieces in text order through krep_gpu_scan_device_seq()", krep_gpu_algorithm_name(algo));
    if (final_piece && (base + w.text_len != G || X < base + w.own_lo + B))
        return kg::fail("-c through %s: the piece that ends the text must hold its last %llu bytes", krep_gpu_algorithm_name(algo),
                        (unsigned long long)(kReplayWindow + B));
    const uint64_t lim = final_piece ? X - base : j.own_hi; // the canonical pass covers the starts in [own_lo, lim)
    const uint64_t nl_end = final_piece ? w.text_len : j.own_hi; // where this piece's newline searches stop
    unsigned long long *d_slot = &pl->d_ctr->pad[0], *h_slot = &pl->h_ctr->pad[0];
    LitResult lr;
    if (lim > w.own_lo)
    {
        LitPass ps;
        ps.ww = pl->ww; ps.lines = true; ps.own_lo = w.own_lo; ps.own_hi = lim; ps.post = &pl->post;
        if (lit_pass(pl, w, ps, st, &lr))
            return 2;
    }
    const krep_gpu_seq_carry_t in = j.carry_in ? *j.carry_in : krep_gpu_seq_carry_t{};
    krep_gpu_seq_carry_t pc{}; // this piece's own contribution
    bool have_q = false;
    uint64_t q = 0;
    if (lim > w.own_lo && last_accepted_before(pl, w, lr, w.own_lo, lim, st, &have_q, &q))
        return 2;
    {
        uint64_t nl = nl_end; // first newline of the piece (the record of a piece without an occurrence; neon_search's kind 2)
        if ((!have_q || algo == KREP_RA_NEON) && tail_find_next_newline(w.d_text, w.own_lo, nl_end, d_slot, h_slot, st, &nl))
            return 2;
        pc.local_first_nl1 = nl < nl_end ? base + nl + 1 : 0;
    }
    if (have_q)
    {
        uint64_t nl = nl_end;
        if (tail_find_next_newline(w.d_text, q, nl_end, d_slot, h_slot, st, &nl))
            return 2;
        pc.local_q1 = base + q + 1;
        pc.local_nl1 = nl < nl_end ? base + nl + 1 : 0;
        if (algo == KREP_RA_NEON)
        {
            // the grid origin in effect for q's line: (first newline behind the last accepted occurrence on an earlier
            // line) + 1 — from this piece if that occurrence lies in it, else from the record in front of it
            uint64_t lsp1 = 0;
            if (tail_find_prev_newline(w.d_text, q, d_slot, h_slot, st, &lsp1))
                return 2;
            if (lsp1 <= w.own_lo) // no newline in [own_lo, q): q's line started in front of this piece
                pc.local_g0_kind = 3;
            else
            {
                bool have_q2 = false;
                uint64_t q2 = 0;
                if (last_accepted_before(pl, w, lr, w.own_lo, lsp1, st, &have_q2, &q2))
                    return 2;
                if (!have_q2)
                    pc.local_g0_kind = 2;
                else
                {
                    uint64_t nl2 = nl_end;
                    if (tail_find_next_newline(w.d_text, q2, nl_end, d_slot, h_slot, st, &nl2))
                        return 2;
                    pc.local_g0_kind = 1;
                    pc.local_g0 = base + nl2 + 1; // nl2 < lsp1 <= q: it exists
                }
            }
        }
    }
    if (final_piece)
        pc.local_lines = lr.lines + 1; // (what krep_gpu_replay_tail() starts from when the record turns out different)
    const krep_gpu_seq_carry_t co = kg::fold_carry(in, pc);
    if (j.carry_out)
        *j.carry_out = co;
    t->total = lr.total; t->lines = lr.lines; t->summary = lr.summary;
    if (final_piece)
    {
        uint64_t extra = 0;
        if (replay_from_record(pl, algo, co, rebased(w.d_text, base), base ? base + 1 : 0, G, st, &extra)) // (global offsets >= cur - 1 >= base: inside the buffer)
            return 2;
        // the lines the replay counts are new ones (it starts behind the line of q), and the line open at the piece's
        // start can only be among them when nothing in front of the piece counted it: the canonical head bit stands
        t->lines = lr.lines + extra;
        t->total = t->lines;
    }
    return 0;
}

// -c through a block-structured function over the whole text: canonical -c over the starts before the last kReplayWindow bytes,
// then the reference's own walk over the rest
static int lit_replay_whole(const LitJob &j, LitTotals *t)
{
    krep_gpu_plan *pl = j.pl;
    const Window &w = j.w;
    const uint64_t G = w.global_len, X = G > kReplayWindow ? G - kReplayWindow : 0;
    LitResult lr;
    uint64_t cur = 0, extra = 0;
    int open = 0;
    if (X)
    {
        LitPass ps;
        ps.ww = pl->ww; ps.lines = true; ps.own_lo = 0; ps.own_hi = X; ps.post = &pl->post;
        if (lit_pass(pl, w, ps, j.st, &lr))
            return 2;
        if (replay_entry(pl, j.algo, w, lr, X, j.st, &cur, &open))
            return 2;
    }
    ReplayIn r{};
    r.algo = j.algo; r.m = pl->m; r.ww = pl->ww; r.n = G; r.cur = cur; r.open = open;
    r.text = w.d_text; r.pat = pl->d_pat;
    if (cur < G && tail_run_replay(r, &pl->d_ctr->pad[0], &pl->h_ctr->pad[0], j.st, &extra))
        return 2;
    t->lines = lr.lines + extra;
    t->total = t->lines; // occurrence totals are not defined by a -c scan
    t->summary = t->lines ? (kLnHead | kLnTail) : 0;
    return 0;
}

// neon_search, count-only with max_count == 0: the first body hit returns 0 (krep.c:4616); with no body hit the tail call's
// BMH returns 1 on its first hit (krep.c:1355-1367).  (ev1 is recorded, kernel_ms is not set.)
static int lit_neon_zero(const LitJob &j, int time_it, krep_gpu_scan_out_t *out)
{
    krep_gpu_plan *pl = j.pl;
    const Window &w = j.w;
    const uint64_t G = w.global_len, T = G - G % 16;
    if (!j.whole)
        return kg::fail("neon_search with max_count == 0 needs the whole text in one window");
    LitPass ps;
    ps.ww = pl->ww; ps.own_lo = 0; ps.own_hi = T; ps.ww_exempt = j.ww_exempt; ps.post = &pl->post;
    LitResult lr;
    if (lit_pass(pl, w, ps, j.st, &lr))
        return 2;
    uint64_t ret = 0;
    if (lr.total == 0 && G - T >= pl->m)
    {
        ps.own_lo = T; ps.own_hi = G;
        if (lit_pass(pl, w, ps, j.st, &lr))
            return 2;
        ret = lr.total ? 1 : 0;
    }
    if (time_it) HIPCHK(hipEventRecord(pl->ev1, j.st));
    HIPCHK(hipStreamSynchronize(j.st));
    out->count = ret;
    out->total_matches = lr.total;
    return 0;
}

// every occurrence the reference reports (memchr / BMH / the block-structured bodies, -c without a replay): one literal pass
static int lit_plain(const LitJob &j, int time_it, LitTotals *t)
{
    krep_gpu_plan *pl = j.pl;
    LitPass ps;
    ps.ww = pl->ww; ps.lines = pl->lines; ps.own_lo = j.w.own_lo; ps.own_hi = j.own_hi;
    ps.excl_lo = j.excl_lo; ps.excl_hi = j.excl_hi; ps.ww_exempt = j.ww_exempt;
    ps.sink = j.want ? LitPass::RECORDS : LitPass::COUNT;
    ps.d_out = (uint64_t *)j.d_pos; ps.out_cap = j.want; ps.post = &pl->post;
    ps.ev_end = time_it ? pl->ev1 : nullptr;
    LitResult lr;
    if (lit_pass(pl, j.w, ps, j.st, &lr))
        return 2;
    t->ev1_recorded = time_it != 0 && lr.n_units != 0;
    t->total = lr.total; t->lines = lr.lines; t->summary = lr.summary;
    return 0;
}

// sequential families on the ordered list (kg_greedy.hip): greedy non-overlapping selection (SSE4.2 / KMP, and BMH
// under -o) over all occurrences, or memchr_short's -o walk over the first-byte candidates.  A window inside the text
// starts where the reference's scan stands (carry_in->resume): starts in front of that point are consumed, the first
// one at or behind it is looked at afresh — exactly what the reference's loop does after `advance`.
static int lit_walk(const LitJob &j, const Family &fam, LitTotals *t)
{
    krep_gpu_plan *pl = j.pl;
    const Window &w = j.w;
    const hipStream_t st = j.st;
    const uint32_t m = pl->m;
    const size_t own_hi = j.own_hi;
    const bool mshort_o = fam.mshort_o;
    const bool ww_first = pl->ww && j.algo == KREP_RA_BMH; // BMH -o: a -w rejected hit does not consume (krep.c:1323-1329)
    const uint64_t resume_in = j.carry_in ? j.carry_in->resume : 0;
    size_t lo_eff = w.own_lo;
    if (resume_in > w.global_base + w.own_lo)
        lo_eff = (size_t)std::min<uint64_t>(own_hi, resume_in - w.global_base);
    uint64_t resume_out = 0;
    // ---- a pattern of ONE repeated byte (`  `, `--`, `aa`), counted: inside a run of R such bytes the kept matches start at every
    // m-th byte — no list of all occurrences (kg_runs.hip; round 6: `-c -o '  '` materialised 188 M occurrences at 0.65 TB/s)
    bool runs_done = false;
    if (!mshort_o && !pl->ww && !pl->lines && j.want == 0 && m >= 2 && !getenv("KREP_GPU_NO_RUNS"))
    {
        bool uniform = true;
        for (uint32_t i = 1; i < m; ++i)
            uniform = uniform && pl->pat_folded[i] == pl->pat_folded[0];
        if (uniform)
        {
            uint64_t end_p1 = 0;
            const int rc = runs_count_greedy(w.d_text, w.text_len, lo_eff, own_hi, m, pl->pat_folded[0], !pl->cs, pl->num_cu, &pl->d_ctr->pad[1],
                                             &pl->h_ctr->pad[1], st, &t->total, &end_p1);
            if (rc == 2)
                return 2;
            if (rc == 0)
            {
                runs_done = true;
                resume_out = end_p1 ? w.global_base + end_p1 : 0;
            }
        }
    }
    LitPass ps;
    ps.own_lo = lo_eff; ps.own_hi = own_hi; ps.sink = LitPass::OCC; ps.post = &pl->post;
    ps.first_byte = mshort_o;
    ps.ww = ww_first;
    LitResult lr;
    if (!runs_done && lit_pass(pl, w, ps, st, &lr))
        return 2;
    WalkSpec ws{};
    ws.mode = mshort_o ? (pl->lines ? kWalkShortOLines : kWalkShortO) : kWalkGreedy;
    if (ws.mode == kWalkShortOLines && !j.whole)
        return kg::fail("-c -o through memchr_short_search jumps to the next line start after every counted line: scan the whole "
                        "text in one window");
    ws.m = m;
    ws.ww = pl->ww && !ww_first;
    ws.lines = pl->lines;
    ws.ci = !pl->cs;
    ws.b1 = m > 1 ? pl->pat_folded[1] : 0;
    ws.b2 = m > 2 ? pl->pat_folded[2] : 0;
    if (lr.total)
    {
        HIPCHK(hipMemsetAsync(pl->d_ctr, 0, sizeof(Counters), st));
        int rc = post_walk(pl->post, w.d_text, w.text_len, w.global_base, ws, lr.total, (uint64_t *)j.d_pos, j.want, pl->d_ctr,
                           pl->h_ctr, st, &t->total, &t->lines, &resume_out);
        if (rc)
            return rc;
    }
    if (j.carry_out)
        j.carry_out->resume = std::max(resume_in, resume_out);
    t->summary = t->total ? (kLnHead | kLnTail) : 0;
    if (pl->lines && !j.whole)
    {
        // line bits of the owned window for the left-to-right fold over the pieces (krep_gpu_combine_line_counts): is there
        // a '\n' in [own_lo, own_hi), does a survivor start at or before the first / behind the last one
        unsigned long long *d_slot = &pl->d_ctr->pad[0], *h_slot = &pl->h_ctr->pad[0];
        uint64_t first_nl = own_hi, last_p1 = 0;
        if (tail_find_next_newline(w.d_text, w.own_lo, own_hi, d_slot, h_slot, st, &first_nl))
            return 2;
        t->summary = 0;
        if (first_nl < own_hi)
        {
            if (tail_find_prev_newline(w.d_text, own_hi, d_slot, h_slot, st, &last_p1))
                return 2;
            t->summary |= kLnNl;
        }
        if (t->total)
        {
            uint64_t s_first[2], s_last[2]; // the survivors were compacted into post.d_surv for the line count
            HIPCHK(hipMemcpy(s_first, pl->post.d_surv, sizeof s_first, hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(s_last, pl->post.d_surv + 2 * (t->total - 1), sizeof s_last, hipMemcpyDeviceToHost));
            const uint64_t f = s_first[0] - w.global_base, l = s_last[0] - w.global_base;
            if (!(t->summary & kLnNl))
                t->summary |= kLnHead | kLnTail;
            else
                t->summary |= (f <= first_nl ? kLnHead : 0) | (l >= last_p1 ? kLnTail : 0);
        }
    }
    return 0;
}

// the epilogue of the plain, walk and replay families: timing, the stream's end, the reference's return value and what is stored
static int lit_finish(const LitJob &j, int time_it, const LitTotals &t, krep_gpu_scan_out_t *out)
{
    krep_gpu_plan *pl = j.pl;
    if (time_it)
    {
        if (stop_clock(pl, !t.ev1_recorded, j.st, out))
            return 2;
    }
    else
        HIPCHK(hipStreamSynchronize(j.st));
    out->total_matches = t.total;
    out->line_count = t.lines;
    out->has_newline = (t.summary & kLnNl) != 0;
    out->head_line_hit = (t.summary & kLnHead) != 0;
    out->tail_line_hit = (t.summary & kLnTail) != 0;
    Verdict v = verdict_for(j.algo, pl, t.total, t.lines, j.d_pos != nullptr);
    out->count = v.ret;
    if (j.d_pos && j.cap && pl->track && !pl->lines)
    {
        // records the reference semantics need (memchr: one more than max_count, the host fixes the order)
        const uint64_t maxc = pl->max_count;
        const uint64_t needed = (j.algo == KREP_RA_MEMCHR && maxc != SIZE_MAX && maxc != 0) ? std::min<uint64_t>(t.total, maxc + 1)
                                                                                             : v.store;
        out->overflow = needed > j.cap;
        out->stored = std::min<uint64_t>(needed, std::min<uint64_t>(t.total, j.want));
    }
    return 0;
}

// krep_gpu_scan_device*: one single-literal scan, by the match-set family of the reference function reproduced (Family)
static int scan_literal(krep_gpu_plan *pl, int algo, const Window &w, match_position_t *d_pos, uint64_t cap, hipStream_t st,
                        int time_it, const krep_gpu_seq_carry_t *carry_in, krep_gpu_seq_carry_t *carry_out, krep_gpu_scan_out_t *out)
{
    const uint32_t m = pl->m;
    memset(out, 0, sizeof *out);
    if (carry_out)
        *carry_out = carry_in ? *carry_in : krep_gpu_seq_carry_t{};
    // the reference function sees the WHOLE text: its length decides the delegation and every early-out
    if (m == 0 || w.global_len < m || w.text_len < m || w.own_lo >= w.own_hi)
        return 0;
    const size_t own_hi = std::min(w.own_hi, w.text_len);
    const bool whole = w.global_base == 0 && w.own_lo == 0 && own_hi + m > w.text_len && w.global_len == w.text_len;

    const Family fam = family_of(algo, pl->only_matching, pl->lines, pl->ww, pl->track, pl->max_count, pl->has_border, m,
                                 pl->has_newline);
    LitJob j{pl, algo, w, own_hi, whole, st, carry_in, carry_out, d_pos, cap, 0};
    if (fam.nlwalk)
        return lit_nlwalk(j, time_it, out);
    // the walks couple neighbouring matches: a window that does not start the text needs the boundary record of the text
    // in front of it (where the reference's scan stands: krep_gpu_seq_carry_t::resume)
    if (fam.need_walk && !whole && !carry_in && w.global_base + w.own_lo != 0)
        return kg::fail("the greedy / only-matching families couple neighbouring matches: scan the whole text in one window, or "
                        "its pieces in text order through krep_gpu_scan_device_seq() (%s, pattern length %u)",
                        krep_gpu_algorithm_name(algo), m);

    // ---- where the block-structured functions put their quirks: positions in the WHOLE text, translated to the buffer
    {
        const uint64_t G = w.global_len, base = w.global_base;
        auto to_local = [&](uint64_t g) -> uint64_t { return g >= base && g - base < w.text_len ? g - base : ~0ull; };
        if (algo == KREP_RA_AVX512 && !pl->lines && G >= 64 && (G % 64) < (uint64_t)m - 1)
        { // krep.c:5171: the last full 64-byte block is stepped over unexamined when remaining < (m-1)+64
            const uint64_t ghi = G - G % 64, glo = ghi - 64;
            if (ghi > base && glo < base + w.text_len)
            {
                j.excl_lo = glo > base ? glo - base : 0;
                j.excl_hi = std::min<uint64_t>(ghi - base, w.text_len);
            }
        }
        if (pl->ww && !pl->lines)
        { // the scalar tail call of the block functions sees the tail as its own text: no left context at its first byte
            const uint64_t B = algo == KREP_RA_AVX2 ? 32 : algo == KREP_RA_AVX512 ? 64 : algo == KREP_RA_NEON ? 16 : 0;
            if (B && (G % B) >= m)
                j.ww_exempt = to_local(G - G % B);
        }
    }
    if (d_pos && cap && !pl->lines) // records the caller can use
    {
        const uint64_t maxc = pl->max_count;
        j.want = maxc;
        if ((algo == KREP_RA_KMP || algo == KREP_RA_MEMCHR) && maxc != SIZE_MAX)
            j.want = maxc + 1; // KMP stores one more (krep.c:1717); the memchr batch quirk needs the next record too
        j.want = std::min<uint64_t>(j.want, cap);
    }

    HIPCHK(hipSetDevice(pl->device));
    if (time_it) HIPCHK(hipEventRecord(pl->ev0, st));
    LitTotals t;
    int rc;
    if (fam.replay)
        rc = whole ? lit_replay_whole(j, &t) : lit_replay_piece(j, &t);
    else if (fam.need_walk)
        rc = lit_walk(j, fam, &t);
    else if (fam.neon_zero)
        return lit_neon_zero(j, time_it, out); // (fills `out` itself)
    else
        rc = lit_plain(j, time_it, &t);
    if (rc)
        return rc;
    return lit_finish(j, time_it, t, out);
}

static int scan_device_impl(krep_gpu_plan_t *pl, const void *d_text, size_t text_len, size_t own_lo, size_t own_hi,
                            size_t global_base, size_t global_len, match_position_t *d_positions, uint64_t position_capacity,
                            void *stream, int time_it, const krep_gpu_seq_carry_t *carry_in, krep_gpu_seq_carry_t *carry_out,
                            krep_gpu_scan_out_t *out)
{
    krep_gpu_scan_out_t tmp;
    if (!out)
        out = &tmp;
    memset(out, 0, sizeof *out);
    if (carry_out)
        *carry_out = carry_in ? *carry_in : krep_gpu_seq_carry_t{};
    if (!pl || (!d_text && text_len))
        return kg::fail("scan_device: bad arguments");
    if (global_len == 0)
        global_len = global_base + text_len;
    if (global_len < global_base + text_len)
        return kg::fail("scan_device: global_len %zu is shorter than global_base + text_len", global_len);
    {
        // hipGetLastError() is sticky per thread: an earlier, deliberately ignored failure (e.g. a hipFree in a
        // destructor) must not be mistaken for a failure of the launches below
        const hipError_t stale = hipGetLastError();
        if (stale != hipSuccess && getenv("KREP_GPU_DEBUG"))
            fprintf(stderr, "krep-gpu: (debug) cleared stale HIP error: %s\n", hipGetErrorString(stale));
    }
    hipStream_t st = (hipStream_t)stream;
    if (pl->unsupported)
        return kg::fail("%s", pl->unsupported);
    if (kg::inject(3))
        return kg::fail("injected failure: kernel launch");
    Window w{(const uint8_t *)d_text, text_len, own_lo, own_hi, global_base, global_len};
    if (pl->ref_algo == KREP_RA_AHO_CORASICK)
        return scan_ac(pl, w, d_positions, position_capacity, st, time_it, carry_in, carry_out, out);
    if (pl->ref_algo == KREP_RA_REGEX)
        return scan_regex(pl, w, d_positions, position_capacity, st, time_it, carry_in, carry_out, out);
    if (pl->sp.num_patterns != 1)
        return kg::fail("scan_device: no pattern");
    const int algo = mirror_effective(pl->ref_algo, &pl->sp, global_len);
    return scan_literal(pl, algo, w, d_positions, position_capacity, st, time_it, carry_in, carry_out, out);
}
extern "C" int krep_gpu_scan_device_ex(krep_gpu_plan_t *pl, const void *d_text, size_t text_len, size_t own_lo, size_t own_hi,
                                       size_t global_base, size_t global_len, match_position_t *d_positions,
                                       uint64_t position_capacity, void *stream, int time_it, krep_gpu_scan_out_t *out)
{
    return scan_device_impl(pl, d_text, text_len, own_lo, own_hi, global_base, global_len, d_positions, position_capacity, stream,
                            time_it, nullptr, nullptr, out);
}
// The pieces of one text, scanned in text order: each call takes the boundary record the previous one left (NULL for the
// piece that starts the text) and leaves its own.  For the families without a sequential dependency the record passes through.
extern "C" int krep_gpu_scan_device_seq(krep_gpu_plan_t *pl, const void *d_text, size_t text_len, size_t own_lo, size_t own_hi,
                                        size_t global_base, size_t global_len, match_position_t *d_positions,
                                        uint64_t position_capacity, void *stream, int time_it,
                                        const krep_gpu_seq_carry_t *carry_in, krep_gpu_seq_carry_t *carry_out,
                                        krep_gpu_scan_out_t *out)
{
    krep_gpu_seq_carry_t zero{};
    return scan_device_impl(pl, d_text, text_len, own_lo, own_hi, global_base, global_len, d_positions, position_capacity, stream,
                            time_it, carry_in ? carry_in : &zero, carry_out, out);
}
// The end-of-text replay alone (include/krep_gpu.h): the piece's canonical count and own contribution are in `piece`, the true
// record of the text in front of it in `carry_true`; only the last bytes of the text are read.
extern "C" int krep_gpu_replay_tail(krep_gpu_plan_t *pl, const void *d_tail, size_t tail_len, size_t global_len, void *stream,
                                    const krep_gpu_seq_carry_t *carry_true, const krep_gpu_seq_carry_t *piece,
                                    krep_gpu_seq_carry_t *carry_out, uint64_t *lines)
{
    if (!pl || !d_tail || !piece || !lines)
        return kg::fail("krep_gpu_replay_tail: NULL argument");
    if (pl->unsupported)
        return kg::fail("%s", pl->unsupported);
    if (pl->ref_algo == KREP_RA_AHO_CORASICK || pl->sp.num_patterns != 1)
        return kg::fail("krep_gpu_replay_tail: not a single-literal plan");
    const int algo = mirror_effective(pl->ref_algo, &pl->sp, global_len);
    const Family fam = family_of(algo, pl->only_matching, pl->lines, pl->ww, pl->track, pl->max_count, pl->has_border, pl->m, pl->has_newline);
    if (!fam.replay)
        return kg::fail("krep_gpu_replay_tail: %s under these parameters has no end-of-text replay", krep_gpu_algorithm_name(algo));
    if (!piece->local_lines)
        return kg::fail("krep_gpu_replay_tail: the record is not that of the piece that ends the text");
    const uint64_t G = global_len, need = std::min<uint64_t>(G, 512);
    if (tail_len > G || tail_len < need)
        return kg::fail("krep_gpu_replay_tail: the tail must hold the last %llu bytes of the text", (unsigned long long)need);
    const krep_gpu_seq_carry_t zero{};
    const krep_gpu_seq_carry_t co = kg::fold_carry(carry_true ? *carry_true : zero, *piece);
    uint64_t extra = 0;
    hipStream_t st = (hipStream_t)stream;
    // (the replay reads global offsets >= cur - 1 with cur >= the block in front of the last kReplayWindow bytes: > G - 512)
    if (replay_from_record(pl, algo, co, rebased(d_tail, G - tail_len), G - tail_len ? G - tail_len + 1 : 0, G, st, &extra))
        return 2;
    HIPCHK(hipStreamSynchronize(st));
    if (carry_out)
        *carry_out = co;
    *lines = (piece->local_lines - 1) + extra;
    return 0;
}
extern "C" int krep_gpu_scan_device(krep_gpu_plan_t *pl, const void *d_text, size_t text_len, size_t own_lo, size_t own_hi,
                                    size_t global_base, match_position_t *d_positions, uint64_t position_capacity,
                                    void *stream, int time_it, krep_gpu_scan_out_t *out)
{
    return krep_gpu_scan_device_ex(pl, d_text, text_len, own_lo, own_hi, global_base, 0, d_positions, position_capacity, stream,
                                   time_it, out);
}

extern "C" uint64_t krep_gpu_combine_line_counts(const krep_gpu_scan_out_t *s, int n)
{
    uint64_t total = 0;
    bool open = false; // the line entering the current shard already holds a match
    for (int i = 0; i < n; ++i)
    {
        total += s[i].line_count;
        if (open && s[i].head_line_hit)
            total -= 1;
        open = s[i].has_newline ? (s[i].tail_line_hit != 0) : (open || s[i].head_line_hit != 0);
    }
    return total;
}

