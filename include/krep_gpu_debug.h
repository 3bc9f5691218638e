/* krep_gpu_debug.h — TEST HOOKS of libkrep_gpu.so.  Not part of the drop-in boundary (include/krep_gpu.h): nothing a host
 * program needs is declared here.  The symbols are exported by the same library so that the test-suite (tests/, through
 * krep_amd/engine.py) can force rare paths — tile shapes, starved grids, injected failures — and read counters that say which
 * kernel answered.  Round 6: moved out of krep_gpu.h. */
#ifndef KREP_GPU_DEBUG_H
#define KREP_GPU_DEBUG_H
#include "krep_gpu.h"
#ifdef __cplusplus
extern "C" {
#endif

/* test hook (host only, no GPU needed): the end-of-text replay of the block-structured -c paths
 * (krep_amd/csrc/kg_replay.h) run on host memory, so that the CPU test-suite can pin it against the oracle */
uint64_t krep_gpu_debug_replay_host(int krep_ref_algo, const void *text, size_t n, const void *pattern, uint32_t m,
                                    int whole_word, size_t cur, int open_line);
/* test hook: force the kernel tile shape (0 = auto, 1 = 32 KiB tiles, 4 = 128 KiB tiles) */
void krep_gpu_debug_force_rounds(int rounds);
/* test hook: staging records per scan unit (0 = auto); small values exercise the emit-mode re-scan */
void krep_gpu_debug_force_stage_cap(int records);
/* test hooks of the one-pass single-byte kernel (kg_single.hip): at most `blocks` workgroups (0 = auto) — a starved grid, as
 * on a shared or partitioned device; and how many of its scans handed over to the two-pass kernels (ring overflow on a
 * dense text, or the spin-limit safety net) since the process started */
void krep_gpu_debug_force_single_grid(int blocks);
uint64_t krep_gpu_debug_single_failovers(void);
/* ... and how many launches of that kernel there were (its 2..8-byte instantiations included: a plan takes them for records of a
 * dense short literal once a two-pass scan has counted the density) */
uint64_t krep_gpu_debug_single_launches(void);
/* test hook: launches of the tiny-dictionary kernel (kg_ac_tiny.hip: every pattern <= 4 bytes, compared in registers) since the
 * process started; $KREP_GPU_AC_NO_TINY=1 (read when a plan is built) keeps such dictionaries on the general kernel */
uint64_t krep_gpu_debug_tiny_launches(void);
/* ... and those of its one-pass record writer in the DENSE flavour (16-bit ring entries, tickets sized by the counted density) */
uint64_t krep_gpu_debug_tiny_dense_launches(void);
/* test hook: make the next operator calls fail at a chosen point — 0 off, 1 device allocation, 2 host->device copy,
 * 3 kernel launch, 4 device->host copy of the records.  Also read from $KREP_GPU_INJECT_FAILURE. */
void krep_gpu_debug_inject_failure(int kind);
/* test hook: pieces the multi-shard operators scanned AGAIN because their boundary record turned out different (rescans) and
 * end pieces that only re-ran the end-of-text replay (replays), since the process started */
void krep_gpu_debug_chain_fixups(uint64_t *rescans, uint64_t *replays);
/* test hook (host only, no GPU needed): the left fold of the boundary record exactly as the library applies it — a piece's
 * own contribution (its local_* fields) onto the record of the text in front of it — so that the CPU test-suite can pin the
 * chained-pieces algebra against the oracle (tests/test_replay_cpu.py) */
void krep_gpu_debug_fold_carry(const krep_gpu_seq_carry_t *in, const krep_gpu_seq_carry_t *piece, krep_gpu_seq_carry_t *out);
/* test hook: launches of the multi-pattern kernel's ANCHORED instantiation (kg_ac_anchor.hip: anchor grams chosen by rarity in a
 * sample of the text) since the process started; $KREP_GPU_AC_ANCHOR=1 anchors every eligible dictionary whatever the estimated
 * gain, $KREP_GPU_AC_NO_ANCHOR=1 none (both read when a dictionary meets its first text of >= 1 MiB) */
uint64_t krep_gpu_debug_anchored_launches(void);
/* test hook: launches of the LDS-DMA literal kernel (kg_literal_dma.hip: 2..8-byte patterns on 32-KiB units without -c) since the
 * process started; $KREP_GPU_LIT_NO_DMA=1 keeps such scans on the register-load kernel (kg_literal.hip) */
uint64_t krep_gpu_debug_literal_dma_launches(void);
/* ... in its one-pass records mode (the scanning waves write the records at their final index, no ordering post-pass: records of a sparse
 * literal on a ticketed text), how many of those scans handed over to the two-pass road (a ticket denser than a wave's hit list, or the
 * spin-limit safety net), and a starved grid for that mode: at most `blocks` workgroups (0 = auto).  $KREP_GPU_LIT_DMA_TWO_PASS=1 keeps
 * such scans on the two-pass road (A/B inside one library) */
uint64_t krep_gpu_debug_literal_dma_one_pass_launches(void);
uint64_t krep_gpu_debug_literal_dma_one_pass_failovers(void);
void krep_gpu_debug_force_literal_dma_grid(int blocks);
/* ... and its ticket map forced: the first `n_long` tickets (as many of them as the text holds) take `long_units` units (8, 16 or 32), the
 * rest 8, whatever the density the plan knows; long_units = 0: the library's choice again.  A text of 2 MiB reaches every kind of seam so.
 * A plan whose long ticket overflowed a wave's list on a text halves it for that text all the same. */
void krep_gpu_debug_force_literal_dma_tickets(int long_units, uint64_t n_long);
/* ... and the map the last launch of that mode ran with: the units of its long tickets and how many there were (n_long = 0: one size) */
void krep_gpu_debug_literal_dma_last_tickets(uint32_t *long_units, uint64_t *n_long);
/* test hooks (host only, no GPU needed) of that map (krep_amd/csrc/kg_tickets.h): ticket `ticket`'s first unit and units under the map
 * {upt_long, upt, n_long} on a text of n_units, and the map's number of tickets; returns 0, or 2 for a map the launcher refuses.  And the
 * number of long tickets the library gives a text of n_units scanned by `waves` waves (0: none, every ticket short) */
int krep_gpu_debug_ticket_map(uint32_t upt_long, uint32_t upt, uint64_t n_long, uint64_t n_units, uint64_t ticket, uint64_t *first,
                              uint32_t *units, uint64_t *n_tickets);
uint64_t krep_gpu_debug_ticket_map_long_tickets(uint64_t n_units, uint32_t upt_long, uint32_t upt, uint64_t waves);
/* what chose between that kernel and the register kernel for `plan`: has the text been sampled, is the kernel barred for it (the prefilter's
 * byte occurs in more than 35 % of its 1-KiB cells; $KREP_GPU_LIT_DMA_MAX_PASS), the share last measured (sample or launch).
 * $KREP_GPU_LIT_DMA_KEEP=1: no sample, no bar (measurement aid) */
int krep_gpu_debug_literal_dma_state(const krep_gpu_plan_t *plan, int *looked, int *barred, double *pass_rate);
/* test hook: launches of the run-length kernel (kg_runs.hip: the greedy families on a pattern of one repeated byte, count-only);
 * $KREP_GPU_NO_RUNS=1 keeps such scans on the list road */
uint64_t krep_gpu_debug_runs_launches(void);
/* test hook of the regex scan (kg_regex.hip): at most `blocks` workgroups (0 = auto) — a starved grid, so that a wave takes a
 * second and third 32-KiB unit on a text of a few hundred KiB (its own grid does that only beyond 5 units per compute unit) */
void krep_gpu_debug_force_regex_grid(int blocks);
/* test hooks of the loops scan (kg_regex_loops.hip; its line walk's grid is capped by the hook above too): which road finds the
 * candidate lines — 0 the scan's choice (the filter's occurrences per text byte), 1 the sparse road (the filter's records), 2 the dense
 * road (every line, from the newline records); and how many scans took each road since the process started */
void krep_gpu_debug_force_regex_loops_road(int road);
/* test hook of the line walk's general step (kg_regex_loops.hip): with both krep_gpu_set_regex_loops() and krep_gpu_set_regex_groups()
 * on, a plan made while this is on walks an expression the LOOPS compiler took by the step of the groups compiler's automaton (its
 * places read as positions: a place hands over along CHAIN, a repeating place is in SELF, no jump pairs) — for the measurement of what
 * the general step costs and the test that the two steps agree.  Off, or with either switch off, nothing changes. */
void krep_gpu_debug_force_regex_general(int on);
/* launches of the line walk's general step since the process started (counting and emitting launches alike): what tells a scan by
 * the general step from one by the old step */
uint64_t krep_gpu_debug_regex_general_walks(void);
void krep_gpu_debug_regex_loops_roads(uint64_t *sparse, uint64_t *dense);
/* test hooks of the long-line walk (kg_regex_loops.hip, krep_gpu_set_regex_long_lines): the bytes of scratch words one round of long
 * lines may hold (0: the default, 256 MiB), so that a text of a few hundred KiB takes several rounds and a line of a few KiB meets the
 * cap min(1 MiB, bytes / 4); and the launches of that walk since the process started (counting, -c and emitting rounds alike) */
void krep_gpu_debug_set_regex_long_budget(uint64_t bytes);
uint64_t krep_gpu_debug_regex_long_walks(void);
/* a multi-pattern plan whose dictionary holds 1..3-byte patterns beside >= 8 longer ones: 0 not decided yet, 1 scanned as one dictionary, 2 split
 * (the long part anchored, the short part on its own, the record lists merged: kg_scan_ac.hip scan_ac_split); $KREP_GPU_AC_NO_SPLIT=1: never */
int krep_gpu_debug_split_state(const krep_gpu_plan_t *plan);
/* what that decision was for `plan`: state 0 not taken yet / 1 end grams kept / 2 anchored; patterns moved off their end; the
 * estimated candidates per tested position with the end grams and with the anchors.  Returns 0, or 2 for a single-literal plan. */
int krep_gpu_debug_anchor_info(const krep_gpu_plan_t *plan, int *state, uint32_t *moved, double *rate_end_grams, double *rate_anchors);
/* what the last general-kernel scan of `plan` MEASURED (candidates per tested position, counted in the kernel), and how many times a
 * measurement that contradicted the estimate re-opened the decision (at most 3; $KREP_GPU_AC_NO_RESAMPLE=1: never) */
int krep_gpu_debug_anchor_measured(const krep_gpu_plan_t *plan, double *measured, int *resamples);
/* which kernel answered the last multi-pattern scan of one dictionary of `plan`, and with what (kg_ac.hip ac_scan; host values only) */
typedef struct krep_gpu_debug_ac_scan
{
    uint32_t road;      /* 0 early-out (nothing launched), 1 byte-set one-pass (kg_single.hip), 2 tiny one-pass (items), 3 tiny one-pass (dense),
                           4 tiny staged (kg_ac_tiny.hip), 5 the general kernel ac_scan_kernel<CI, LINES, SHORT, STRIDE, ANCH, WW> */
    uint32_t ci, lines; /* -i, in-kernel -c */
    uint32_t shorts;    /* the dictionary holds a 1..3-byte pattern (SHORT) */
    uint32_t stride;    /* 1 or 2 (0: the scan left before its arguments were made) */
    uint32_t anch;      /* 0 end grams, 1 anchored on four classes, 2 on five */
    uint32_t ww_filter; /* the WW instantiation was launched (-w, stride 2, no short pattern) */
    uint32_t exact;     /* the exact dictionary (xtab) was passed */
    uint32_t g4x_mode;
    uint32_t stage_cap; /* staged matches per unit as launched (0: no records wanted, or a one-pass road) */
    uint32_t upt;       /* units per ticket */
    uint64_t n_units;
    uint64_t overflow_units; /* units with more matches than stage_cap */
    uint32_t emit;      /* the emit pass: 0 none, 1 over the redo list, 2 a walk over every unit */
    uint32_t next_stage_cap; /* what the scan left for the dictionary's following scan */
    uint32_t short_lens;     /* bit k - 1: the dictionary holds a pattern of k bytes, k = 1..3 */
    uint64_t scans;     /* scans this dictionary has reported so far: a report is the last call's iff this moved by one */
} krep_gpu_debug_ac_scan_t;
/* part 0: the plan's dictionary, or the long part of a split plan (krep_gpu_debug_split_state() == 2); part 1: the short part of a split
 * plan.  Returns 0, or 2 for a single-literal plan and for a part that does not exist.  A dictionary that has not scanned yet reports
 * scans == 0 and zeroes. */
int krep_gpu_debug_ac_last_scan(const krep_gpu_plan_t *plan, int part, krep_gpu_debug_ac_scan_t *out);
/* test hook of krep_gpu_search_batch(): the packed size at which a batch is cut into a further pack (0 = the default, two pieces of
 * the configuration's stream_chunk_bytes), so that a batch of a few hundred KiB takes several scans */
void krep_gpu_debug_batch_pack_limit(size_t bytes);
/* where the calling thread's last krep_gpu_search_batch() spent its time, in milliseconds of wall clock: gathering the items into
 * the pinned staging ring and copying them to the device, the scan, the segmentation kernels, the read-back (tools/batch_bench.py) */
void krep_gpu_debug_batch_times(double *pack_ms, double *scan_ms, double *segment_ms, double *readback_ms);
/* test hook (host only, no GPU needed): bytes [lo, lo + cnt) of the pack krep_gpu_search_batch() makes of `items` — the items with one
 * '\n' between neighbours — written to dst by the function its staging ring fills every chunk with (kg::batch_fill), over the offset
 * table the batch call builds.  Returns 0, or 2 when [lo, lo + cnt) leaves the pack (tests/test_batch_fill_cpu.py) */
int krep_gpu_debug_batch_fill_host(const krep_gpu_batch_item_t *items, size_t n, size_t lo, size_t cnt, void *dst);
/* test hook: launches of the batch's record rebase with the items' offset table in LDS (it fits: items + 1 <= 4096 entries) and with the
 * table in global memory, since the process started: which of the two a batch at the edge took shows in no result */
void krep_gpu_debug_batch_rebase_launches(uint64_t *lds_table, uint64_t *global_table);
/* test hook: launches of the batch's per-item max_count cut (batch_cut, krep_gpu_set_batch_max_count) with the summed kept-record table
 * in LDS (items + 1 <= 4096 entries) and with the table in global memory, since the process started.  A batch without max_count, one that
 * returns no records (-c, count-only) and one with max_count == 0 launch none. */
void krep_gpu_debug_batch_cut_launches(uint64_t *lds_table, uint64_t *global_table);
/* the sibling of krep_gpu_debug_batch_times() for krep_gpu_grep_batch(): where the calling thread's last call spent its time, in
 * milliseconds of wall clock — pack, scan and segmentation as above; format: the ordering of a multi-pattern list, the upload of the
 * prefixes and the formatter over the pack; readback: the copies of the bytes, the item offsets and the counts (tools/batch_grep_bench.py) */
void krep_gpu_debug_grep_batch_times(double *pack_ms, double *scan_ms, double *segment_ms, double *format_ms, double *readback_ms);
/* test hook: calls of the pack formatters (krep_gpu_format_lines_items / krep_gpu_format_matches_items) that looked a record's item up
 * with the offset table in LDS (items + 1 <= 4096 entries) and with the table in global memory, since the process started */
void krep_gpu_debug_batch_format_launches(uint64_t *lds_table, uint64_t *global_table);
/* test hook: the prefix scan every formatter, the batch segmentation and the line analysis share (kg_format.hip scan_exclusive), alone:
 * d_out[i] = d_in[0] + .. + d_in[i - 1] mod 2^64, or with take_max the largest of them (0 in front of the first), for n 64-bit words on the
 * device; synchronises `stream` before it returns.  d_out must be a buffer of its own: the scan's kernels take both pointers as
 * __restrict__ and no caller in the library scans in place, so d_out == d_in is not supported and is refused.  Nothing behind
 * d_out[n - 1] is written.  Returns 0, or 2 (tests/test_gpu_scan_exclusive.py) */
int krep_gpu_debug_scan_exclusive(const uint64_t *d_in, uint64_t n, uint64_t *d_out, int take_max, void *stream);

#ifdef __cplusplus
}
#endif
#endif
