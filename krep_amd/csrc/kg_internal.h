// kg_internal.h — internal (C++) interfaces between the translation units of libkrep_gpu.so.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstring>
#include <functional>
#include <initializer_list>
#include <mutex>
#include <vector>

#include "../../include/krep_gpu.h"
#include "../../include/krep_gpu_debug.h" // (test hooks, exported by the same library)
#include "kg_batch_pack.h"
#include "kg_common.h"
#include "kg_regex_compile.h"

namespace kg {

int fail(const char *fmt, ...); // records krep_gpu_last_error(), prints "krep-gpu: ..." and returns 2
const char *device_unusable(int device); // NULL: a gfx950 device this code object runs on; else why not
bool inject(int kind);                   // test hook: is failure `kind` being injected (krep_gpu_debug_inject_failure)
// a HIP call that fails makes the calling function return fail(...)
#define HIPCHK(x)                                                                                 \
    do                                                                                            \
    {                                                                                             \
        hipError_t e_ = (x);                                                                      \
        if (e_ != hipSuccess)                                                                     \
            return kg::fail("%s failed: %s (%s:%d)", #x, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

// Grow-only device scratch.  When `need` is beyond `cap`, every buffer of the group is freed first, then each is allocated again
// with its own byte count (the caller's slack included; 0: left null for a later user) and `cap` becomes `new_cap`.  A failed
// allocation returns its error with `cap` at 0; what it means (an error, or another road) is the caller's decision.
struct DevBuf
{
    void **p;
    size_t bytes;
};
template <class T> DevBuf dev_buf(T *&p, size_t bytes) { return {reinterpret_cast<void **>(&p), bytes}; }
inline hipError_t grow_scratch(uint64_t &cap, uint64_t need, uint64_t new_cap, std::initializer_list<DevBuf> bufs)
{
    if (need <= cap)
        return hipSuccess;
    for (const DevBuf &b : bufs)
    {
        if (*b.p) (void)hipFree(*b.p);
        *b.p = nullptr;
    }
    cap = 0;
    for (const DevBuf &b : bufs)
        if (b.bytes)
            if (const hipError_t e = hipMalloc(b.p, b.bytes); e != hipSuccess)
                return e;
    cap = new_cap;
    return hipSuccess;
}

// More than 64 KiB of dynamic LDS is requested once per kernel and device (the call sits on the latency path of small host buffers);
// atomic flags: several host threads may launch one kernel; devices beyond the table set it every time.
template <auto Kernel> hipError_t grant_dynamic_lds(int bytes)
{
    static std::atomic<bool> granted[64];
    int dev = 0;
    (void)hipGetDevice(&dev);
    const bool known = dev >= 0 && dev < 64;
    if (known && granted[dev].load(std::memory_order_acquire))
        return hipSuccess;
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e == hipSuccess && known)
        granted[dev].store(true, std::memory_order_release);
    return e;
}

// kg_literal.hip
hipError_t launch_literal(const LitArgs &a, uint32_t num_cu, hipStream_t st); // grid = resident blocks of the variant x CUs
// kg_runs.hip: the greedy families on a pattern of one repeated byte, counted without a list (1: a run too long for its look-back)
int runs_count_greedy(const uint8_t *d_text, uint64_t text_len, uint64_t lo, uint64_t hi, uint32_t m, uint8_t byte, bool ci, int num_cu,
                      unsigned long long *d_slots, unsigned long long *h_slots, hipStream_t st, uint64_t *total, uint64_t *end_p1);
bool literal_dma_eligible(const LitArgs &a);                                       // kg_literal_dma.hip: 2..8-byte patterns, 32-KiB units, no -c
hipError_t launch_literal_dma(const LitArgs &a, uint32_t num_cu, hipStream_t st);
hipError_t launch_dma_byte_look(const uint8_t *text, uint64_t lo, uint32_t n_cells, uint32_t prefilter, bool ci, unsigned long long *out, hipStream_t st); // 1-KiB cells of a sample that hold the prefilter's byte
extern std::atomic<uint64_t> g_runs_launches;                                      // launches of run_count_kernel (kg_runs.hip, test hook)
extern std::atomic<uint64_t> g_lit_dma_launches;                                   // launches of lit_scan_dma (test hook)
// ... its one-pass records mode: the scanning waves write the records at their final index (kg_tickets.h); d_agg / d_pref: n_tickets =
// tk_map_tickets(tk, units) words each (kg_tickets.h: tk = the ticket map, long tickets in front, tk.upt = a.upt), zeroed on the stream in
// front of the launch like a.ctr (whose pad[0] the resolver is claimed through)
struct TkMap;
hipError_t launch_literal_dma_one_pass(const LitArgs &a, const TkMap &tk, unsigned long long *d_agg, unsigned long long *d_pref, uint64_t n_tickets,
                                       uint32_t num_cu, hipStream_t st);
uint32_t lit_dma_one_pass_list();                                                  // entries of a wave's hit list: what a ticket may hold at most
extern std::atomic<uint64_t> g_lit_dma1p_launches;                                 // launches in that mode (test hook)
extern std::atomic<uint64_t> g_lit_dma1p_failovers;                                // ... that handed their scan over to the two-pass road
extern int g_lit_dma1p_force_grid;                                                 // test hook: at most this many workgroups (0 = auto)
uint32_t lit_dma_one_pass_grid(const LitArgs &a, uint32_t num_cu);                 // workgroups that mode launches (x 4 waves: who draws its tickets)
extern std::atomic<uint32_t> g_lit_dma1p_last_long;                                // test hook: the last launch's long ticket (units; the short one if none) ...
extern std::atomic<uint64_t> g_lit_dma1p_last_n_long;                              // ... and how many of its tickets were long
extern int g_lit_dma1p_force_long;                                                // test hook: units of a long ticket (0 = the host's choice) ...
extern uint64_t g_lit_dma1p_force_n_long;                                          // ... and how many tickets are long (as far as the text holds them)

// kg_single.hip — single byte with records in one pass (counts resolved by one wave, records written a ticket later)
struct PostScratch;
constexpr int kFusedShapeMax = 5;
double single_fused_max_density(int shape); // hits per byte a shape's rings are sure to hold (shapes 0..5: ~1.2 / 3.7 / 5 / 7.5 / 10 / 20 %)
// the smallest shape from `start` on whose rings hold `margin` x `density` hits per byte (kFusedShapeMax when none does)
int single_fused_shape_for(double density, double margin, int start);
// a text sparse enough (`total` hits in `span` bytes) to re-open the one-pass road to a plan that overflowed its largest rings
bool single_fused_reopens(uint64_t total, uint64_t span);
// One one-pass scan at *shape over the `n_units` units of `a` (`span` bytes from a.anchor), its ticket scratch in post.d_tk.  A ticket
// that overflowed its ring: the counted density picks a larger shape (*shape follows) and the scan runs again.  Done (0): the
// counters are in *h_ctr, and a text half as sparse as the next smaller shape holds has stepped *shape down for the next scan.
// kFusedGaveUp: too dense for the largest rings (or the total is not to be trusted).  2: an error.  ev_end (if any) is recorded
// behind each launch; count_launch: each launch counts towards krep_gpu_debug_single_launches.
constexpr int kFusedGaveUp = 1;
int single_fused_run(const LitArgs &a, uint64_t n_units, uint64_t span, PostScratch &post, Counters *d_ctr, Counters *h_ctr,
                     uint32_t num_cu, int *shape, hipEvent_t ev_end, hipStream_t st, bool count_launch);

// kg_post.hip — ordering post-pass shared by the literal and Aho-Corasick scans
struct PostScratch
{
    unsigned long long *d_unitinfo = nullptr; // [units] info words written by the scan kernel
    unsigned long long *d_offsets = nullptr;  // [units] exclusive global index of each unit's first hit
    unsigned long long *d_blk = nullptr;      // [2 * units/1024] block sums / line carries
    uint64_t units_cap = 0;
    unsigned long long *d_stage = nullptr;    // [units * stage_cap] staged, unit-ordered hit words
    uint64_t stage_cap_words = 0;
    uint64_t *d_occ = nullptr;                // all-occurrence records for the greedy (family N) filter
    uint64_t occ_cap = 0;                     // in records
    uint8_t *d_keep = nullptr;                // greedy survivor flags
    unsigned long long *d_gblk = nullptr;     // compaction block counts
    unsigned long long *d_surv = nullptr;     // compacted survivors (line counting)
    uint64_t keep_cap = 0;
    unsigned long long *d_tk = nullptr;       // kg_single.hip: per-ticket hit counts | their exclusive prefixes
    uint64_t tk_cap = 0;                      // in tickets
};
void post_free(PostScratch &s);
int post_reserve(PostScratch &s, uint64_t n_units, uint64_t stage_words);
// K1..K4 on `st`: offsets, distinct-line total (ctr->lines), line summary (ctr->summary), gather into d_pos
// fixed_len > 0: 16-bit unit-relative staging, record start = origin + unit * unit_bytes + offset
int post_order(PostScratch &s, uint64_t n_units, uint32_t stage_cap, uint32_t fixed_len, uint64_t origin, uint64_t unit_bytes,
               bool want_lines, uint64_t *d_pos, uint64_t pos_cap, Counters *d_ctr, int num_cu, hipStream_t st);
int post_offsets_pass(PostScratch &s, uint64_t n_units, bool want_lines, Counters *d_ctr, hipStream_t st);
int post_gather_pass(PostScratch &s, uint64_t n_units, uint32_t stage_cap, uint32_t fixed_len, uint64_t origin,
                     uint64_t unit_bytes, uint64_t *d_pos, uint64_t pos_cap, int num_cu, hipStream_t st);
// kg_greedy.hip — the sequential match-set families, walked cluster by cluster on the ordered list in s.d_occ
constexpr uint32_t kWalkGreedy = 0; // simd_sse42_search / kmp_search (and BMH under -o): greedy non-overlapping occurrences
constexpr uint32_t kWalkShortO = 1; // memchr_short_search under -o: first-byte candidates, m skipped after a failed one too
constexpr uint32_t kWalkShortOLines = 2; // ... with -c as well (krep.c:4449-4470): an accepted match counts its line and sends the
                                         // walk to the next line start — every visited accepted candidate is one counted line
constexpr uint32_t kWalkAlt = 3;    // krep -E alternation (kg_regex_alt.hip): records ordered by start, equal starts in ascending length; the
                                    // longest record of a visited start is kept and consumes its own length; m = Lmax splits the clusters
struct WalkSpec
{
    uint32_t mode, m;
    bool ww, lines, ci;
    uint8_t b1, b2; // kWalkShortO: (folded) pattern bytes 1 and 2
};
int post_walk(PostScratch &s, const uint8_t *d_text, uint64_t text_len, uint64_t global_base, const WalkSpec &ws,
              uint64_t n_occ, uint64_t *d_pos, uint64_t want, Counters *d_ctr, Counters *h_ctr, hipStream_t st,
              uint64_t *total, uint64_t *nlines, uint64_t *resume);

constexpr uint32_t kNlWalkSse42 = 0, kNlWalkKmp = 1; // post_nlwalk modes
int post_nlwalk(PostScratch &s, const uint8_t *d_text, uint64_t text_len, uint32_t mode, uint32_t m, uint32_t k0, bool ww, bool om,
                uint64_t maxc, uint64_t n_occ, const uint64_t *d_lineno, Counters *d_ctr, Counters *h_ctr, hipStream_t st,
                uint64_t *count, uint64_t global_base, uint64_t global_len, uint64_t line_off, uint64_t cp_in, uint64_t seen_in,
                uint64_t *cp_out, uint64_t *seen_out);

// kg_tail.hip — end-of-text replay of the block-structured -c paths (kg_replay.h)
struct ReplayIn;
int tail_last_hit(const unsigned long long *d_unitinfo, uint64_t limit_units, unsigned long long *d_slot,
                  unsigned long long *h_slot, hipStream_t st, uint64_t *unit_plus1);
int tail_find_next_newline(const uint8_t *d_text, uint64_t from, uint64_t n, unsigned long long *d_slot,
                           unsigned long long *h_slot, hipStream_t st, uint64_t *pos);
int tail_find_prev_newline(const uint8_t *d_text, uint64_t before, unsigned long long *d_slot, unsigned long long *h_slot,
                           hipStream_t st, uint64_t *pos_plus1);
int tail_count_changes(const uint64_t *d_v, uint64_t n, unsigned long long *d_slot, unsigned long long *h_slot, hipStream_t st,
                       uint64_t *changes);
int tail_count_line_gaps(const uint8_t *d_text, uint64_t text_len, uint64_t global_base, const uint64_t *d_rec, uint64_t n, unsigned long long *d_slot,
                         unsigned long long *h_slot, hipStream_t st, uint64_t *lines);
int tail_launch_line_gaps(const uint8_t *d_text, uint64_t text_len, uint64_t global_base, const uint64_t *d_rec, const unsigned long long *d_n,
                          const unsigned long long *d_skip_if, uint64_t cap, unsigned long long *d_out, hipStream_t st);
// '\n' bytes of d_text[lo, hi) -> *count (kg_tail.hip; results through the plan's pinned counter block)
int tail_count_newlines(const uint8_t *d_text, uint64_t lo, uint64_t hi, unsigned long long *d_slot, unsigned long long *h_slot,
                        hipStream_t st, uint64_t *count);
int tail_run_replay(const ReplayIn &r, unsigned long long *d_slot, unsigned long long *h_slot, hipStream_t st, uint64_t *lines);

// kg_ac.hip — multi-pattern scan
int order_records(match_position_t *d_positions, uint64_t n, size_t max_offset, hipStream_t st, bool by_end); // kg_format.hip: stable radix sort of a record list by start / by end
struct AcTables;
AcTables *ac_build(const search_params_t &sp, int device);
void ac_free(AcTables *t);
// One multi-pattern scan: what ac_scan reads and where it writes (the scan side fills the workspace from its plan: kg_scan_ac.hip)
// AcOwn: Start — a match belongs to the window of its START; LinesOnList — END-owned records, their line gaps counted behind the
// post-pass (-c on the record list); End — END-owned records only (the emission-order list of -c with a newline inside a pattern)
enum class AcOwn { Start, LinesOnList, End };
struct AcScan
{
    AcTables *t = nullptr;
    Counters *d_ctr = nullptr, *h_ctr = nullptr; // workspace
    PostScratch *post = nullptr;
    int num_cu = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipStream_t st = nullptr;
    const uint8_t *d_text = nullptr; // window
    size_t text_len = 0, own_lo = 0, own_hi = 0, global_base = 0;
    match_position_t *d_pos = nullptr; // record sink
    uint64_t cap = 0, max_count = SIZE_MAX;
    bool track = false, ww = false, lines = false;
    AcOwn own = AcOwn::Start;
    int time_it = 0;
};
int ac_scan(const AcScan &c, krep_gpu_scan_out_t *out);

// kg_config.hip — test hooks shared with the scan drivers
extern std::atomic<int> g_force_rounds, g_force_stage_cap;   // krep_gpu_debug_force_rounds / _stage_cap
extern std::atomic<int> g_rx_force_grid;                     // krep_gpu_debug_force_regex_grid: at most this many workgroups (0 = auto)
extern std::atomic<int> g_regex_loops;                       // krep_gpu_set_regex_loops: a search asks the loops compiler too
extern std::atomic<int> g_regex_groups;                      // krep_gpu_set_regex_groups: a search asks the groups compiler too, fifth
extern std::atomic<uint64_t> g_rl_general;                   // krep_gpu_debug_regex_general_walks: launches of the line walk's general step
extern std::atomic<int> g_rl_force_general;                  // krep_gpu_debug_force_regex_general: loops programs through the general step
extern std::atomic<int> g_regex_loops_windows;               // krep_gpu_set_regex_loops_windows: a loops search is scanned in windows
extern std::atomic<int> g_regex_long_lines;                  // krep_gpu_set_regex_long_lines: lines over 4096 bytes of a loops search are walked
extern std::atomic<uint64_t> g_rl_long_budget;               // krep_gpu_debug_set_regex_long_budget: bytes of C words a round holds (0: default)
extern std::atomic<uint64_t> g_rl_long;                      // krep_gpu_debug_regex_long_walks: launches of the long-line walk
extern std::atomic<int> g_batch_max_count;                   // krep_gpu_set_batch_max_count: the batch takes a finite max_count
extern std::atomic<int> g_rl_force_road;                     // krep_gpu_debug_force_regex_loops_road: 0 auto, 1 sparse, 2 dense
extern std::atomic<uint64_t> g_rl_sparse, g_rl_dense;        // scans of kg_regex_loops.hip that took each road
extern std::atomic<uint64_t> g_tiny_launches;                // launches of ac_tiny_kernel (kg_ac_tiny.hip)
extern std::atomic<uint64_t> g_tiny_dense_launches;          // ... of its DENSE one-pass flavour
extern std::atomic<uint64_t> g_ac_anchored_launches;         // launches of ac_scan_kernel<.., ANCH> (kg_ac.hip, kg_ac_anchor.hip)
extern std::atomic<uint64_t> g_fused1_launches;              // launches of single_fused (kg_single.hip)
extern std::atomic<uint64_t> g_fused1_failovers;             // one-pass single-byte scans that handed over to the two-pass kernels
inline uint8_t lo8(uint8_t c) { return (c >= 'A' && c <= 'Z') ? (uint8_t)(c + 32) : c; } // lower_table, krep.c:125-134
inline bool pattern_has_border(const uint8_t *p, size_t m)   // a proper prefix is also a suffix: all occurrences != greedy
{
    for (size_t k = 1; k < m; ++k)
        if (memcmp(p, p + k, m - k) == 0)
            return true;
    return false;
}

// kg_config.hip / kg_mirror.hip — configuration (explicit; see krep_gpu_config_t), selector mirror, result container
krep_gpu_config_t current_config(); // the calling thread's override, else the process-wide defaults
int mirror_top(const search_params_t *p, const krep_gpu_config_t &c);
int mirror_effective(int top, const search_params_t *p, size_t text_len);
const char *unsupported_reason(const search_params_t *p, const krep_gpu_config_t &c); // NULL = accelerated
// regex_compile_search (kg_regex_compile.h: the -E compilers in the order every search asks them, RegexCompiled their verdict) behind a
// one-entry cache per thread: an operator call asks the selector, the executor, the split rule and (on a cache miss) the plan about
// the same pattern, and one compile is up to 16 regcomp calls and 4096 regexec probes.  The key is everything the compilers read
// (the bytes and the length of every pattern, case, -w, whether the locale is multibyte).
const char *regex_compile_cached(const search_params_t *p, RegexCompiled *out); // NULL: taken; else the refusal
constexpr int kSplitWhole = 0, kSplitPieces = 1, kSplitChain = 2; // enum krep_gpu_split (include/krep_gpu.h)
int split_mode(const search_params_t *p, const krep_gpu_config_t &c, size_t text_len);
bool shardable(const search_params_t *p, const krep_gpu_config_t &c, size_t text_len); // split_mode != whole
// a piece's own contribution (the local_* fields of `piece`) folded onto the record of the text in front of it
krep_gpu_seq_carry_t fold_carry(const krep_gpu_seq_carry_t &in, const krep_gpu_seq_carry_t &piece);
bool result_reserve(match_result_t *r, uint64_t extra);
inline bool by_start_end(const match_position_t &a, const match_position_t &b) // the formatter's order (krep.c:420-434)
{
    return a.start_offset != b.start_offset ? a.start_offset < b.start_offset : a.end_offset < b.end_offset;
}
bool have_error();

// What the reference function returns / stores given the number of emitted matches (`total`, after greedy selection and -w) or
// distinct lines.  One place for all the max_count corner cases: the scans ask it with their plan (kg_scan.hip verdict_for), the
// batch derives its per-item cut from it (kg_batch.hip batch_cut_rule).
struct Verdict { uint64_t ret, store; };
inline Verdict verdict_rule(int algo, size_t maxc, bool lines, bool track, uint64_t total, uint64_t nlines, bool have_result)
{
    const bool store = track && have_result;
    Verdict v{0, 0};
    switch (algo)
    {
    case KREP_RA_MEMCHR: // krep.c:3897, :3955, :3976
    case KREP_RA_KMP:    // krep.c:1634, :1696, :1717
    case KREP_RA_AHO_CORASICK: // aho_corasick.c:316
    case KREP_RA_SSE42: // :4713 then the pre-increment checks :4778/:4804
        if (maxc == 0)
            return v;
        break;
    case KREP_RA_NEON: // :4516 then the pre-increment checks :4582/:4616; count-only with max_count == 0 is resolved by
                       // the caller (the tail call's BMH convention, lit_neon_zero)
        if (maxc == 0)
            return v;
        break;
    default: // BMH :1266, memchr_short :4376, AVX2 :4887, AVX-512 :5119
        if (maxc == 0)
        {
            if (lines || track)
                return v;
            v.ret = total > 0 ? 1 : 0; // count-only: the first hit makes 1 >= 0 true (krep.c:1355-1367)
            return v;
        }
    }
    if (lines)
    {
        v.ret = nlines < maxc ? nlines : maxc;
        return v;
    }
    v.ret = total < maxc ? total : maxc;
    if (store)
    {
        v.store = v.ret;
        if (algo == KREP_RA_KMP && maxc != SIZE_MAX && total > maxc)
            v.store = v.ret + 1; // krep.c:1717-1724 stores the (max_count+1)-th match before breaking
    }
    return v;
}
// memchr_search's final flush (krep.c:3976-3991 + :4026-4038) displaces a record of a list of `have` under max_count `maxc`
// (kg_exec.hip memchr_batch_quirk moves it; the batch's cut reads through the same map)
inline bool memchr_flush_displaces(uint64_t have, size_t maxc)
{
    return !(maxc == SIZE_MAX || maxc == 0 || have <= maxc || (maxc % 4096) != 0);
}

// kg_format.hip — what the formatter-side entry points share: the scratch, the scan and the newline table below; the host steps of
// the grep-output drivers (entry checks, format strings, the cursor over the scratch, the output tail) are declared in kg_format_host.h
void format_release(); // frees the formatter scratch of every device
extern std::mutex g_fmt_mu;                 // held for a whole formatter call: its scratch is one buffer per device
int fmt_reserve(size_t bytes, void **out);  // that buffer, grown to at least `bytes` (g_fmt_mu held); 2: failed
uint64_t scan_sums_words(uint64_t n);       // words of scratch (`sums`) a scan of n words needs
// exclusive prefix scan of in[0, n) into out (a buffer of its own) on `st`: the sum, or with take_max the running maximum (0 in front)
void scan_exclusive(const unsigned long long *in, uint64_t n, unsigned long long *out, unsigned long long *sums, bool take_max,
                    hipStream_t st);
constexpr uint32_t kLineBlock = 4096;       // newline counts are kept per 4 KiB of text
// entries of the table below: one per block of the text and one more, so that its last entry is the text's total
inline uint64_t line_blocks(uint64_t text_len) { return (text_len + kLineBlock - 1) / kLineBlock + 1; }
// one streaming pass over the text on `st`: before[b] = the newlines in front of block b; `counts` (line_blocks words) and `sums`
// (scan_sums_words(line_blocks)) are scratch.  (krep_gpu_line_numbers, kg_matches.hip)
int newlines_before_blocks(const uint8_t *d_text, uint64_t text_len, unsigned long long *counts, unsigned long long *before,
                           unsigned long long *sums, hipStream_t st);

// kg_comm.hip — the RCCL all-reduce of the per-shard counters (one process driving several devices)
int allreduce_across_devices(const std::vector<int> &devs, std::vector<std::vector<unsigned long long>> &vecs);
int comm_warmup(const std::vector<int> &devs);       // creates the communicator of a device list ahead of the first search
int comm_clique_ranks(const std::vector<int> &devs); // ranks of the cached communicator over `devs` (0: none)

// kg_cost.hip — krep_gpu_worthwhile()'s cost model: what this process has measured about its own GPU side
void cost_note_device_init(double ms);                  // the first device call of the process (availability probe)
void cost_note_host_path(size_t bytes, double seconds); // a host-buffer operator call that went through the staging ring

// kg_exec.hip — a host buffer through HBM, whole or in pieces over num_gpus devices, records appended to `result`; 2: failed
int host_scan(const search_params_t *params, const krep_gpu_config_t &cfg, const char *text, size_t text_len, int num_gpus,
              match_result_t *result, uint64_t *ret);

// ---- what the host-buffer entry points share (kg_ops.hip, kg_batch.hip)
// One view of the caller's params: legacy callers fill only pattern / pattern_len (the reference's own
// tests, test/test_krep.c:233-235), the CLI fills the arrays as well.  After this, num_patterns >= 1, patterns / pattern_lens
// are valid and pattern / pattern_len name the first one (run_pieces read pattern_lens[] of the raw struct).
struct NormParams
{
    search_params_t sp{};
    const char *one_pat = nullptr;
    size_t one_len = 0;
    bool valid = false;
    explicit NormParams(const search_params_t *p)
    {
        sp = *p;
        if (p->num_patterns > 1)
        {
            valid = p->patterns && p->pattern_lens;
            return;
        }
        if (p->num_patterns == 1 && p->patterns && p->pattern_lens && p->patterns[0])
        {
            one_pat = p->patterns[0];
            one_len = p->pattern_lens[0];
        }
        else if (p->pattern)
        {
            one_pat = p->pattern;
            one_len = p->pattern_len;
        }
        else
            return;
        sp.pattern = one_pat;
        sp.pattern_len = one_len;
        sp.patterns = &one_pat;
        sp.pattern_lens = &one_len;
        sp.num_patterns = 1;
        valid = true;
    }
    NormParams(const NormParams &) = delete;
    NormParams &operator=(const NormParams &) = delete;
};
// restores the calling thread's current HIP device: the operators are called on the HOST's threads (krep.c:1950), and a
// library must not leave their device changed
struct DeviceGuard
{
    int prev = -1;
    DeviceGuard() { (void)hipGetDevice(&prev); (void)hipGetLastError(); }
    ~DeviceGuard()
    {
        if (prev >= 0)
            (void)hipSetDevice(prev);
    }
};
void note_error(const char *why); // kg_config.hip: sets krep_gpu_last_error() without printing (a refusal that is an answer, not a failure)

// kg_batch.hip — a batch of texts in one scan (krep_gpu_search_batch): when packing is exact, and the segmentation of a pack's records
const char *batch_unsupported_reason(const search_params_t *p, const krep_gpu_config_t &c); // NULL: newline-separable, taken
struct BatchScratch // grow-only, one per device context
{
    unsigned long long *d_off = nullptr; // [items + 1] base offset of every item in the pack; the last entry is packed size + 1
    unsigned long long *d_res = nullptr; // [items] krep_gpu_batch_result_t
    uint64_t items_cap = 0;
    uint64_t *d_lines = nullptr;          // -c: [records] line number of every record's start
    unsigned long long *d_flags = nullptr; // ... 1 where a record opens a line nobody before it counted
    unsigned long long *d_prefix = nullptr; // ... their exclusive sum
    unsigned long long *d_sums = nullptr;   // ... scratch of that sum
    uint64_t rec_cap = 0;
    // krep_gpu_grep_batch: the items' prefixes and their offsets [items + 1], where every item's output begins [items + 1]; the output
    unsigned char *d_pfx = nullptr;
    uint64_t pfx_cap = 0;
    unsigned long long *d_pfx_off = nullptr, *d_item_out = nullptr;
    uint64_t grep_items_cap = 0;
    unsigned char *d_out = nullptr;
    uint64_t out_cap = 0;
    // a batch under max_count (BatchCut): per item [items + 2] the records kept, their exclusive sum (entry `items`: the kept total)
    // and the item's first record in the uncut list (entry `items`: n_rec); the scratch of that sum; the kept records
    unsigned long long *d_keep = nullptr, *d_new_first = nullptr, *d_lo = nullptr, *d_cut_sums = nullptr;
    uint64_t cut_items_cap = 0;
    match_position_t *d_cut = nullptr;
    uint64_t cut_cap = 0;
};
void batch_scratch_free(BatchScratch &s);
// The per-item cut of a pack's record list under max_count (krep_gpu_set_batch_max_count), as the kernels take it.
// For item i: T its records in the uncut list, Ln its distinct lines.  count = min(Ln, m) under -c, else min(T, m), and with m == 0:
// zero_one && T > 0.  Kept: min(T, m) records, `extra` more when T > m (kmp_search), none when m == 0; `displace`: memchr_search's
// flush map applies when T > m.  batch_cut_rule derives every field from verdict_rule / memchr_flush_displaces.
struct BatchCut
{
    unsigned long long m;
    uint32_t zero_one, extra, displace;
};
enum class BatchCutOut { None, Rebased, PackSorted }; // no records; the search's list per item; the grep list (start order within an item's single-pattern list)
BatchCut batch_cut_rule(const search_params_t *p, const krep_gpu_config_t &c, bool search_file_cap);
// The record list of one pack and how to cut it into the n_items results of BatchScratch::d_res: n_rec records in d_pos, pack-relative,
// in the reference's emission order (by_end: a multi-pattern list, ascending in end).  first_record = rec_base + the item's first
// index when `report`, else rec_base with n_records = 0; lines: count = the distinct lines of the item's record starts, the list is
// ordered by start on the way and not rebased; else count = the item's records and, with `report`, every record is rebased to its
// item's first byte.  h_off: the table of BatchScratch::d_off on the host.  cut (NULL: none, and no buffer of the cut is touched): the
// rule above applied per item; `form` says whether the kept records are written to BatchScratch::d_cut (Rebased: as `report` rebases
// them; PackSorted: pack-relative, the displaced memchr record at its place by start); first_record / n_records then describe the
// kept list, and batch_kept_total reads its length once the stream has been waited for.
struct BatchSegment
{
    const uint8_t *d_text;
    uint64_t packed;
    const uint64_t *h_off;
    uint64_t n_items;
    match_position_t *d_pos;
    uint64_t n_rec, rec_base;
    bool by_end, lines, report;
    const BatchCut *cut;
    BatchCutOut form;
};
int batch_segment(BatchScratch &s, const BatchSegment &g, hipStream_t st); // (queued on `st`, not synchronised)
int batch_kept_total(const BatchScratch &s, uint64_t n_items, uint64_t n_rec, uint64_t *n_kept); // (a cut with records, n_rec > 0)
// (the next pack of a batch on the host — its offset table, the bytes of any slice of it: kg_batch_pack.h, batch_pack_offsets / batch_fill)
// kg_exec.hip — one pack through the device context of cfg->device (host_batch_pack): gathered through the staging ring into the arena,
// scanned in one window with the records plan `scan`, segmented, read back.
struct BatchPackOnDevice // the pack as it lies on the device behind the segmentation
{
    BatchScratch &scratch;
    const uint8_t *d_text;
    uint64_t packed;
    const unsigned long long *d_off; // [n_items + 1], as BatchScratch::d_off
    uint64_t n_items;
    match_position_t *d_pos; // pack-relative, in emission order (by_end: a multi-pattern list, ascending in end); under a cut: the kept list
    uint64_t n_rec;
    bool by_end;
};
using BatchStep = std::function<int(const BatchPackOnDevice &)>;
struct BatchTimes // wall clock of a call's stages, ms (krep_gpu_debug_batch_times, krep_gpu_debug_grep_batch_times)
{
    double pack = 0, scan = 0, segment = 0, format = 0, read_back = 0;
    void operator+=(const BatchTimes &t) { pack += t.pack, scan += t.scan, segment += t.segment, format += t.format, read_back += t.read_back; }
};
struct BatchPackJob
{
    const search_params_t *scan; // the records plan's params
    const krep_gpu_config_t *cfg;
    const krep_gpu_batch_item_t *items; // [n], and off[n + 1]: batch_pack_offsets
    size_t n;
    const uint64_t *off;
    bool lines, report; // as BatchSegment
    // with `report` the rebased records go to records->positions behind records->count + appended (the block grows, count is left
    // alone: a later failure appends nothing)
    match_result_t *records;
    uint64_t appended;
    // (NULL: none, krep_gpu_search_batch) called between the segmentation and the read-back with the pack as it lies on the device
    // (krep_gpu_grep_batch formats it there); a step that returns non-zero fails the pack, and its time is its own
    const BatchStep *step;
    const BatchCut *cut; // as BatchSegment
    BatchCutOut form;
};
struct BatchPackDone
{
    uint64_t n_rec = 0, n_kept = 0; // the records of the scan; under a cut with records: those kept
    float kernel_ms = 0;
    BatchTimes ms; // pack, scan, segment, read_back of this pack (of one that failed: as far as it got)
};
int host_batch_pack(const BatchPackJob &job, krep_gpu_batch_result_t *res_out /* [job.n] */, BatchPackDone *done); // 2: failed

// kg_batch_format.hip — the formatters over a pack behind krep_gpu_format_lines_items / krep_gpu_format_matches_items.  grow (NULL:
// none): asked for the output buffer once the size is known (-> a device buffer of at least that many bytes, NULL: it failed and said
// why), so that krep_gpu_grep_batch analyses a pack once instead of asking for the size first
using FormatOutGrow = std::function<void *(size_t)>;
int format_lines_items(const void *d_pack, size_t packed_len, const krep_gpu_pack_view_t *v, const match_position_t *d_positions, uint64_t n,
                       const krep_gpu_line_format_t *fmt, void *d_out, size_t out_capacity, const FormatOutGrow *grow,
                       uint64_t *d_item_out_off, krep_gpu_lines_out_t *out, hipStream_t st);
int format_matches_items(const void *d_pack, size_t packed_len, const krep_gpu_pack_view_t *v, const match_position_t *d_positions,
                         uint64_t n, const krep_gpu_match_format_t *fmt, void *d_out, size_t out_capacity, const FormatOutGrow *grow,
                         uint64_t *d_item_out_off, krep_gpu_matches_out_t *out, hipStream_t st);

} // namespace kg
