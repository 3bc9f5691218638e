// kg_scan_ac.hip — the multi-pattern (aho_corasick_search) drivers of krep_gpu_scan_device[_ex|_seq]: scan_ac picks the road —
// -c with a newline inside a pattern (scan_ac_newline_lines), -c on the record list (scan_ac_lines_on_list), the dictionary split
// into a long and a short part (scan_ac_split), else one ac_scan of the whole dictionary (kg_ac.hip).  Host logic only.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "kg_ac_tables.h"
#include "kg_internal.h"
#include "kg_plan.h"

using namespace kg;

// an ac_scan of `t` over the window, in the plan's workspace and with its -w: `cap` records at d_pos (none: counted only)
static AcScan ac_call(krep_gpu_plan *pl, AcTables *t, const Window &w, hipStream_t st, AcOwn own, match_position_t *d_pos, uint64_t cap,
                      bool track, size_t max_count, bool lines = false, int time_it = 0)
{
    return AcScan{t, pl->d_ctr, pl->h_ctr, &pl->post, pl->num_cu, pl->ev0, pl->ev1, st, w.d_text, w.text_len, w.own_lo, w.own_hi, w.global_base,
                  d_pos, cap, max_count, track, pl->ww, lines, own, time_it};
}
// a tiny dictionary: its in-kernel -c road keeps nothing in LDS (kg_ac_tiny.hip)
static bool ac_counts_lines_in_registers(const AcTables *t) { return t && t->tiny.ok && !t->tiny.five; }
// aho_corasick_search -c when a pattern contains '\n': matches are visited in emission order (end ascending, longest
// first) and the counter is bumped whenever the line of a match START differs from the line of the previously counted
// one (aho_corasick.c:383-396) — with a newline inside a pattern a later match may start on an EARLIER line, so a line
// can be counted more than once.  Reproduced literally: the ordered match list, the line number of every start
// (kg_format.hip), the number of changes along the list.
// Pieces (round 5): a piece owns the matches that END in [own_lo, own_hi) — the pieces' lists, concatenated in text order, ARE
// the emission order — and what couples it to the text in front of it is two numbers (krep_gpu_seq_carry_t): the newlines so
// far (its line numbers are global) and the line of the last match's start (its first match counts only on another line).
// The buffer must hold the longest pattern's length in front of own_lo (every piece of kg_exec.hip's run_pieces does).
static int scan_ac_newline_lines(krep_gpu_plan *pl, const Window &w, hipStream_t st, int time_it, const krep_gpu_seq_carry_t *carry_in,
                                 krep_gpu_seq_carry_t *carry_out, krep_gpu_scan_out_t *out)
{
    const krep_gpu_seq_carry_t in = carry_in ? *carry_in : krep_gpu_seq_carry_t{};
    krep_gpu_seq_carry_t local{};
    const size_t own_hi = std::min(w.own_hi, w.text_len);
    auto leave = [&]() { if (carry_out) *carry_out = fold_carry(in, local); };
    if (pl->max_count == 0 || w.own_lo >= own_hi) // aho_corasick.c:316
    {
        leave();
        return 0;
    }
    if (time_it) HIPCHK(hipEventRecord(pl->ev0, st));
    unsigned long long *d_slot = &pl->d_ctr->pad[0], *h_slot = &pl->h_ctr->pad[0];
    krep_gpu_scan_out_t o1;
    int rc = ac_scan(ac_call(pl, pl->ac, w, st, AcOwn::End, nullptr, 0, false, SIZE_MAX), &o1);
    if (rc)
        return rc;
    const uint64_t total = o1.total_matches;
    uint64_t changes = 0, nl_halo = 0, nl_own = 0;
    if (tail_count_newlines(w.d_text, 0, w.own_lo, d_slot, h_slot, st, &nl_halo) || tail_count_newlines(w.d_text, w.own_lo, own_hi, d_slot, h_slot, st, &nl_own))
        return 2;
    local.local_nl = nl_own;
    if (total)
    {
        if (nl_reserve(pl, total, total + total / 4 + 1024, true))
            return 2;
        rc = ac_scan(ac_call(pl, pl->ac, w, st, AcOwn::End, pl->d_nl_rec, total, true, SIZE_MAX), &o1);
        if (!rc)
            rc = krep_gpu_line_numbers_ex(w.d_text, w.text_len, w.global_base, pl->d_nl_rec, total, pl->d_nl_ln, st); // 1 + newlines in [buffer start, start)
        if (!rc)
            rc = tail_count_changes(pl->d_nl_ln, total, d_slot, h_slot, st, &changes);
        if (rc)
            return rc;
        uint64_t ends[2] = {0, 0};
        HIPCHK(hipMemcpyAsync(&ends[0], pl->d_nl_ln, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(&ends[1], pl->d_nl_ln + (total - 1), sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        // line of a start relative to own_lo (negative for a start in the halo): (ln - 1) - newlines of the halo
        const uint64_t bias = 1ull << 62;
        const uint64_t first_rel = bias + (ends[0] - 1ull) - nl_halo, last_rel = bias + (ends[1] - 1ull) - nl_halo;
        if (in.last_line && in.nl_before + 1ull + (first_rel - bias) == in.last_line)
            changes -= 1; // the first match of this piece starts on the line of the text's last match so far: not counted again
        local.local_last = last_rel;
    }
    if (time_it && stop_clock(pl, true, st, out))
        return 2;
    leave();
    out->total_matches = total;
    out->line_count = changes;
    out->has_newline = 1; // (krep_gpu_combine_line_counts then adds the pieces' counts up: nothing merges across a cut that the record has not settled)
    out->head_line_hit = out->tail_line_hit = 0;
    out->count = std::min<uint64_t>(changes, pl->max_count);
    return 0;
}
// ---- a dictionary with SHORT patterns beside many longer ones on a word-like text (round 6) ----------------------------------
// The anchored scan (kg_ac_anchor.hip) is what makes a word dictionary fast on word text — 20x — and it is refused when the dictionary
// holds a 1..3-byte pattern: the pair filter's wildcard entries for such a pattern pass a 2-gram's worth of positions, and the exact
// anchor buckets are keyed on four bytes.  One `the` or `of` in a list of a thousand words sent the whole scan back to 0.027 of the
// roofline.  Here the two parts are dictionaries of their own: the patterns of >= 4 bytes (anchored), the 1..3-byte ones (the tiny
// register-compare kernel when they qualify, the general kernel otherwise); their counts add, and their record lists — each in
// aho_corasick_search's order, END ascending and longest first (aho_corasick.c:383-437), patterns of different lengths never produce the
// same record — are merged by two stable radix sorts, by start and then by END.  Decided once per plan, on its first text of >= 1 MiB,
// by sampling that text with the long part (ac_anchor_prepare): split only where the long part anchors.  Returns 1: not applicable.
// (a merged list beyond this — a dense short part — is not worth two sorts with 32 bytes of scratch per record; $KREP_GPU_AC_SPLIT_MAX: the tests' way to the fallback)
static const uint64_t kAcSplitMaxRecords = [] { const char *e = getenv("KREP_GPU_AC_SPLIT_MAX"); return e && atoll(e) > 0 ? (uint64_t)atoll(e) : (1ull << 28); }();
// the decision (once per plan, on its first text of >= 1 MiB): 2 = split, 1 = one dictionary; 0 = not decided yet (the text is too small to sample)
static int ac_split_decide(krep_gpu_plan *pl, const Window &w, hipStream_t st)
{
    AcTables *t = pl->ac;
    if (pl->ac_split)
        return pl->ac_split;
    if (!t || t->has_empty || !(t->has1 || t->has2 || t->has3) || pl->max_count == 0 || getenv("KREP_GPU_AC_NO_SPLIT"))
        return pl->ac_split = 1;
    const size_t hi = std::min(w.own_hi, w.text_len);
    if (w.text_len < (1u << 20) || hi <= w.own_lo || hi - w.own_lo < (1u << 19))
        return 0; // (too small to sample: decided by a later text)
    size_t n_long = 0;
    for (size_t i = 0; i < pl->sp.num_patterns; ++i)
        n_long += pl->sp.pattern_lens[i] >= 4;
    const size_t n_short = pl->sp.num_patterns - n_long;
    pl->ac_split = 1;
    if (n_long < 8 || n_short == 0)
        return 1;
    // a part as a dictionary of its own (null: its build failed, the error cleared)
    auto build_part = [&](bool is_long) {
        std::vector<const char *> pats;
        std::vector<size_t> lens;
        for (size_t i = 0; i < pl->sp.num_patterns; ++i)
            if ((pl->sp.pattern_lens[i] >= 4) == is_long)
                pats.push_back(pl->sp.patterns[i]), lens.push_back(pl->sp.pattern_lens[i]);
        search_params_t sub = pl->sp;
        sub.patterns = pats.data();
        sub.pattern_lens = lens.data();
        sub.num_patterns = pats.size();
        sub.pattern = nullptr;
        sub.pattern_len = 0;
        AcTables *part = ac_build(sub, pl->device);
        if (!part)
            krep_gpu_clear_error();
        return part;
    };
    if (!(pl->ac_long = build_part(true)))
        return 1;
    if (hipSetDevice(pl->device) != hipSuccess || ac_anchor_prepare(pl->ac_long, w.d_text, w.text_len, w.own_lo, hi, st) == 2)
        (void)hipGetLastError();
    // (the long part gains nothing from anchors on this text: one scan of the whole dictionary, as always)
    if (pl->ac_long->anch_state != 2 || !(pl->ac_short = build_part(false)))
    {
        ac_free(pl->ac_long);
        pl->ac_long = nullptr;
        return 1;
    }
    if (getenv("KREP_GPU_DEBUG"))
        fprintf(stderr, "krep-gpu: multi-pattern scan split: %zu patterns of >= 4 bytes (anchored) + %zu of 1..3 bytes, lists merged by (end, start)\n", n_long,
                n_short);
    return pl->ac_split = 2;
}
// The split dictionary's two scans into dst[0, room): the long part's records first, the short part's behind them, each part at most
// part_cap.  *d2: where the short part's went (null: no room was left behind the first list, the short part was counted only).
static int ac_split_scan(krep_gpu_plan *pl, AcScan c, match_position_t *dst, uint64_t room, uint64_t part_cap, krep_gpu_scan_out_t *oa,
                         krep_gpu_scan_out_t *ob, match_position_t **d2)
{
    c.t = pl->ac_long;
    c.d_pos = dst;
    c.cap = std::min(room, part_cap);
    if (const int rc = ac_scan(c, oa))
        return rc;
    *d2 = (dst && room > oa->stored) ? dst + oa->stored : nullptr;
    c.t = pl->ac_short;
    c.d_pos = *d2;
    c.cap = *d2 ? std::min(room - oa->stored, part_cap) : 0;
    return ac_scan(c, ob);
}
// The two parts' n records at dst merged into the one list's order (when `sort`: start, then END — records with one END come out
// longest first, the smaller start), the first copy_n of them copied to copy_to (if any).  1: the sort's scratch — 32 bytes per
// record — did not fit, or the list exceeds the device sort's 2^31-1 items (a dictionary whose short part is dense): one scan of
// the whole dictionary, from now on.
static int ac_split_merge(krep_gpu_plan *pl, const Window &w, match_position_t *dst, uint64_t n, bool sort, match_position_t *copy_to,
                          uint64_t copy_n, hipStream_t st)
{
    if (sort && (n > kAcSplitMaxRecords || order_records(dst, n, w.global_base + w.text_len + 1, st, false) ||
                 order_records(dst, n, w.global_base + w.text_len + 1, st, true)))
    {
        krep_gpu_clear_error();
        pl->ac_split = 1;
        return 1;
    }
    if (copy_to && copy_n)
    {
        HIPCHK(hipMemcpyAsync(copy_to, dst, copy_n * sizeof(match_position_t), hipMemcpyDeviceToDevice, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    // (a later text on which the long part no longer anchors — its decision follows the text, kg_ac.hip — ends the split)
    if (pl->ac_long->anch_state == 1)
        pl->ac_split = 1;
    return 0;
}
static int scan_ac_split(krep_gpu_plan *pl, const Window &w, match_position_t *d_pos, uint64_t cap, hipStream_t st, int time_it,
                         krep_gpu_scan_out_t *out)
{
    if (ac_split_decide(pl, w, st) != 2)
        return 1;
    // Under a max_count that the caller's list can hold (max_count == cap included: the long part alone could fill that list) the
    // result is the first max_count records of the MERGED list: either part may contribute all of them, so both parts' first max_count
    // records go to a scratch list of the plan, are merged there, and the first max_count are copied out.  Without such a limit the
    // caller's list holds everything (or overflows, as always).
    const bool want = d_pos && pl->track, limited = want && pl->max_count != SIZE_MAX && (uint64_t)pl->max_count <= cap;
    match_position_t *dst = d_pos;
    uint64_t room = cap;
    if (limited)
    {
        const uint64_t need = 2 * (uint64_t)pl->max_count;
        if (grow_scratch(pl->split_cap, need, need, {dev_buf(pl->d_split_rec, need * sizeof(match_position_t))}) != hipSuccess)
        {
            (void)hipGetLastError();
            return 1; // (no room for the scratch list: one scan of the whole dictionary)
        }
        dst = pl->d_split_rec;
        room = need;
    }
    krep_gpu_scan_out_t o1, o2;
    match_position_t *d2 = nullptr;
    if (const int rc = ac_split_scan(pl, ac_call(pl, nullptr, w, st, AcOwn::Start, nullptr, 0, pl->track, pl->max_count, false, time_it),
                                     want ? dst : nullptr, want ? room : 0, limited ? (uint64_t)pl->max_count : room, &o1, &o2, &d2))
        return rc;
    memset(out, 0, sizeof *out);
    const uint64_t total = o1.total_matches + o2.total_matches;
    out->total_matches = total;
    out->count = std::min<uint64_t>(total, (uint64_t)pl->max_count);
    out->head_line_hit = out->tail_line_hit = total != 0;
    out->kernel_ms = o1.kernel_ms + o2.kernel_ms;
    const uint64_t s1 = want ? o1.stored : 0, s2 = d2 ? o2.stored : 0, n = s1 + s2;
    out->overflow = want && out->count > cap;
    out->stored = (want && !out->overflow) ? std::min<uint64_t>(n, out->count) : 0;
    return ac_split_merge(pl, w, dst, n, want && !out->overflow && s1 && s2, limited ? d_pos : nullptr, out->stored, st);
}
// aho_corasick_search with count_lines_mode, no newline inside any pattern, on a large sparse text: the matches are scanned as
// RECORDS by the fast kernel (staging + post-pass into the plan's grow-only list) and the lines are counted ON THE LIST — two
// neighbours of the end-ordered list lie on different lines iff the gap between them holds a '\n' (kg_tail.hip,
// tail_line_gaps).  The in-kernel line bookkeeping of kg_ac.hip (exact newline mask of every 1-KiB cell, hit and newline
// bitmaps per unit, a line pass over all 16 cells of every unit) runs at 0.43 of the HBM roofline on BASELINE config 4; this
// road costs the records scan (0.61) plus ~2 cache lines per match.  The line summary of the window (has_newline / head / tail,
// krep_gpu_combine_line_counts) comes from two early-exit newline sweeps and the first and last record.  Matches are owned by
// their END (last byte in [own_lo, own_hi)) on both roads, so neighbouring pieces may take different roads (kg_ac.hip ac_args).
// Returns 1 when the text turns out to be too dense for the list (the caller takes the in-kernel road), 2 on error.
constexpr size_t kAcLinesOnListMin = (size_t)32 << 20;
static int scan_ac_lines_on_list(krep_gpu_plan *pl, const Window &w, hipStream_t st, int time_it, krep_gpu_scan_out_t *out)
{
    memset(out, 0, sizeof *out);
    if (pl->max_count == 0) // aho_corasick.c:316
        return 0;
    const size_t own_hi = std::min(w.own_hi, w.text_len);
    if (w.own_lo >= own_hi)
        return 0;
    if (time_it) HIPCHK(hipEventRecord(pl->ev0, st));
    // More matches than this and the list is no shortcut: a record costs its 16 bytes plus ~2 random cache lines of gap test
    // (~48 ps), the in-kernel line pass 0.1-0.13 ps per byte of text — break-even at one match per ~400 bytes (measured at
    // 32 GiB, profiles/r04_dictionaries.txt: `xq zj`, one per 500 bytes, 3.1 TB/s on the list against 2.2 in the kernel;
    // `er th an`, one per 300, 1.8 against 2.0; `a Sherlock`, one per 28, 0.65 against 2.4).  The plan remembers.
    // (a tiny dictionary counts its lines in registers since round 5 — 3.4-4.4 TB/s whatever the density: the list is ahead only
    //  below one match per ~1000 bytes; profiles/r05_dictionaries.txt: `he she hers`, one per 811, 3.34 on the list against 3.44)
    const uint64_t dense = w.text_len / (ac_counts_lines_in_registers(pl->ac) ? 1000 : 400) + 4096;
    if (pl->lines_list_off)
        return 1;
    if (nl_reserve(pl, 1, std::max<uint64_t>(w.text_len / 1024, 1u << 16), false))
        return 2;
    krep_gpu_scan_out_t o1;
    for (int attempt = 0;; ++attempt)
    {
        int rc = 0;
        bool merged = false; // (the list below is the two parts', merged)
        if (ac_split_decide(pl, w, st) == 2)
        {
            // (a dictionary with short patterns on word-like text, scan_ac_split: the two parts' END-owned lists, merged into the order the
            //  one list would have — END ascending, longest first —, the line gaps counted on the merged list below)
            krep_gpu_scan_out_t oa, ob;
            match_position_t *d2 = nullptr;
            rc = ac_split_scan(pl, ac_call(pl, nullptr, w, st, AcOwn::End, nullptr, 0, true, SIZE_MAX), pl->d_nl_rec, pl->nl_cap, pl->nl_cap, &oa, &ob, &d2);
            if (rc)
                return rc;
            memset(&o1, 0, sizeof o1);
            o1.total_matches = oa.total_matches + ob.total_matches;
            o1.overflow = oa.overflow || ob.overflow || !d2 || o1.total_matches > pl->nl_cap;
            o1.line_count = ~0ull; // (counted on the merged list below)
            merged = !ac_split_merge(pl, w, pl->d_nl_rec, o1.total_matches, !o1.overflow && oa.stored && ob.stored, nullptr, 0, st);
        }
        if (!merged)
            rc = ac_scan(ac_call(pl, pl->ac, w, st, AcOwn::LinesOnList, pl->d_nl_rec, pl->nl_cap, true, SIZE_MAX), &o1);
        if (rc)
            return rc;
        if (o1.total_matches > dense)
        {
            pl->lines_list_off = true;
            return 1;
        }
        if (!o1.overflow || attempt == 1)
            break;
        // (whatever nl_cap says: the list overflowed)
        if (nl_reserve(pl, pl->nl_cap + 1, o1.total_matches + o1.total_matches / 8 + 1024, false))
            return 2;
    }
    const uint64_t total = o1.total_matches;
    uint64_t lines = o1.line_count; // counted behind the post-pass on the stream, unless some unit overflowed its staging slot
    if (total && lines == ~0ull && tail_count_line_gaps(w.d_text, w.text_len, w.global_base, (const uint64_t *)pl->d_nl_rec, total, &pl->d_ctr->pad[0], &pl->h_ctr->pad[0],
                                      st, &lines))
        return 2;
    if (time_it) HIPCHK(hipEventRecord(pl->ev1, st));
    // the window's line summary: first and last '\n' of the owned bytes, first and last record
    uint64_t first_nl = own_hi, last_nl1 = 0;
    if (tail_find_next_newline(w.d_text, w.own_lo, own_hi, &pl->d_ctr->pad[0], &pl->h_ctr->pad[0], st, &first_nl))
        return 2;
    const bool has_nl = first_nl < own_hi;
    if (has_nl && tail_find_prev_newline(w.d_text, own_hi, &pl->d_ctr->pad[0], &pl->h_ctr->pad[0], st, &last_nl1))
        return 2;
    bool head = total != 0, tail = total != 0;
    if (total && has_nl)
    {
        match_position_t ends[2];
        HIPCHK(hipMemcpyAsync(&ends[0], pl->d_nl_rec, sizeof(match_position_t), hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(&ends[1], pl->d_nl_rec + (total - 1), sizeof(match_position_t), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        // a match before the first / behind the last newline exists iff the first / last record of the end-ordered list is one
        // (no match holds a newline, so none can reach across it)
        head = ends[0].start_offset - w.global_base < first_nl;
        tail = ends[1].start_offset - w.global_base >= last_nl1;
    }
    if (time_it && stop_clock(pl, false, st, out)) // (ev1: behind the line count above)
        return 2;
    out->total_matches = total;
    out->line_count = lines;
    out->has_newline = has_nl;
    out->head_line_hit = head;
    out->tail_line_hit = tail;
    out->count = std::min<uint64_t>(lines, pl->max_count);
    return 0;
}
// the roads in order: each of the first three may hand the window on (1) to the next
int kg::scan_ac(krep_gpu_plan *pl, const Window &w, match_position_t *d_pos, uint64_t cap, hipStream_t st, int time_it,
                const krep_gpu_seq_carry_t *carry_in, krep_gpu_seq_carry_t *carry_out, krep_gpu_scan_out_t *out)
{
    if (pl->lines && pl->ac_has_newline)
        return scan_ac_newline_lines(pl, w, st, time_it, carry_in, carry_out, out);
    if (pl->lines && w.text_len >= kAcLinesOnListMin && !getenv("KREP_GPU_AC_LINES_INKERNEL"))
    {
        // (small texts keep the in-kernel road: the list road ends with a few host round trips, ~0.1 ms)
        const int rc = scan_ac_lines_on_list(pl, w, st, time_it, out);
        if (rc != 1)
            return rc;
    }
    if (!pl->lines)
    {
        const int rc = scan_ac_split(pl, w, d_pos, cap, st, time_it, out);
        if (rc != 1)
            return rc;
    }
    const int rc = ac_scan(ac_call(pl, pl->ac, w, st, AcOwn::Start, d_pos, cap, pl->track, pl->max_count, pl->lines, time_it), out);
    // the in-kernel road knows the match count too: a text at half the list's break-even density re-opens the list road for
    // the plan's next pieces (the decision was one-way until round 5)
    if (!rc && pl->lines && pl->lines_list_off && out->total_matches < w.text_len / (ac_counts_lines_in_registers(pl->ac) ? 2000 : 800))
        pl->lines_list_off = false;
    return rc;
}
