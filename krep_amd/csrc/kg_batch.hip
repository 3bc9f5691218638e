// kg_batch.hip — a batch of texts in one scan (krep_gpu_search_batch, include/krep_gpu.h "a batch of texts in one scan"): the reference's
// -r mode meets many small texts, and one operator call per text costs more than scanning it.  The items of a batch are packed into one
// device buffer with one '\n' between neighbours (kg_exec.hip host_batch_pack), the pack is scanned once with records, and the record
// list is cut back into per-item results HERE:
//   batch_bounds     one thread per item: lower bounds of the item's base offsets over the record starts -> first_record, n_records, count
//   batch_rebase     one thread per record: its item by binary search over the offset table (in LDS when it fits), start and end made
//                    relative to the item's first byte
//   batch_line_flags -c: 1 where a record's line differs from its predecessor's; an exclusive sum over the flags makes an item's
//                    distinct-line count the difference at its two bounds (no loop per item: one item may hold every record)
// under a max_count (krep_gpu_set_batch_max_count; the rule: batch_cut_rule) the same bounds, then the cut, then the order:
//   batch_bounds_cut one thread per item: count and the records KEPT from the rule; an exclusive sum over the kept numbers
//   batch_first      one thread per item: first_record from that sum
//   batch_cut        one thread per KEPT record: its item by binary search over the summed kept numbers (in LDS when they fit), its
//                    source through the inverse of memchr_search's flush map, 16 B in and 16 B out into a second list — rebased
//                    (krep_gpu_search_batch) or pack-relative (krep_gpu_grep_batch)
// launched by batch_segment in steps (segment_reserve, segment_line_prefix, then segment_cut or segment_plain to its end), and the rule
// that says when all this is exact (kg::batch_unsupported_reason: newline-separable searches only).
// Both calls are one walk (BatchWalk): enter — the refusals both share, in one order — the call's own checks, the
// device, then per pack next() and pack() (kg_exec.hip host_batch_pack), then the call's commit of its results at the very end.
// krep_gpu_grep_batch gives every pack one step more: the pack is formatted where it lies (grep_format_pack over
// kg_batch_format.hip) and the printed bytes are read back instead of the records; under -c grep_print_counts prints on the host.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstring>
#include <optional>
#include <vector>

#include "../../include/krep_gpu.h"
#include "kg_device.h"
#include "kg_format_dev.h"
#include "kg_internal.h"

using namespace kg;

namespace kg {
namespace {
constexpr u32 kBatchLdsItems = 4096; // offset-table entries (items + 1) batch_rebase keeps in LDS: 32 KiB
constexpr u32 kRebasePerBlock = 2048; // records one workgroup of batch_rebase walks: the table load is paid once per 2048 records

// (a) res[i] = {count, first_record, n_records}.  prefix != NULL (-c): count = the flags summed over the item's records.
__global__ void __launch_bounds__(256) batch_bounds(const u64 *__restrict__ rec, u64 n_rec, const u64 *__restrict__ off, u64 n_items,
                                                    u64 rec_base, int report, const u64 *__restrict__ prefix,
                                                    const u64 *__restrict__ flags, u64 *__restrict__ res)
{
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_items)
        return;
    const u64 lo = first_record_at(rec, n_rec, off[i]), hi = first_record_at(rec, n_rec, off[i + 1]);
    u64 count = hi - lo;
    if (prefix && n_rec)
    {
        const u64 total = prefix[n_rec - 1] + flags[n_rec - 1];
        count = (hi < n_rec ? prefix[hi] : total) - (lo < n_rec ? prefix[lo] : total);
    }
    res[3 * i] = count;
    res[3 * i + 1] = report ? rec_base + lo : rec_base;
    res[3 * i + 2] = report ? hi - lo : 0;
}

// (b) every record relative to its item's first byte.  LDS: off[0 .. n_items] fits kBatchLdsItems entries.
template <bool LDS>
__global__ void __launch_bounds__(256) batch_rebase(u64 *__restrict__ rec, u64 n_rec, const u64 *__restrict__ off, u64 n_items)
{
    __shared__ u64 s_off[LDS ? kBatchLdsItems : 1];
    if (LDS)
    {
        for (u32 t = threadIdx.x; t <= (u32)n_items; t += blockDim.x)
            s_off[t] = off[t];
        __syncthreads();
    }
    const u64 *tab = LDS ? s_off : off;
    const u64 k0 = (u64)blockIdx.x * kRebasePerBlock, k1 = k0 + kRebasePerBlock < n_rec ? k0 + kRebasePerBlock : n_rec;
    for (u64 k = k0 + threadIdx.x; k < k1; k += blockDim.x)
    {
        uint4 r = *reinterpret_cast<const uint4 *>(rec + 2 * k);
        const u64 start = ((u64)r.y << 32) | r.x, end = ((u64)r.w << 32) | r.z;
        u64 lo = 0, hi = n_items; // the last item whose base is at or in front of the start: tab[lo] <= start < tab[hi]
        while (hi - lo > 1)
        {
            const u64 mid = lo + (hi - lo) / 2;
            if (tab[mid] <= start)
                lo = mid;
            else
                hi = mid;
        }
        const u64 base = tab[lo], s = start - base, e = end - base;
        r.x = (u32)s; r.y = (u32)(s >> 32); r.z = (u32)e; r.w = (u32)(e >> 32);
        *reinterpret_cast<uint4 *>(rec + 2 * k) = r;
    }
}

// (c) -c: record k opens a line when its line differs from record k-1's.  The first record of an item always does: the separator
// in front of the item is a '\n', so its line number is larger than that of every record of the items before it.
__global__ void __launch_bounds__(256) batch_line_flags(const u64 *__restrict__ lines, u64 n_rec, u64 *__restrict__ flags)
{
    const u64 k = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n_rec)
        flags[k] = (k == 0 || lines[k] != lines[k - 1]) ? 1 : 0;
}

// ---- under a max_count: the rule per item, then the kept records into a second list
// (a') batch_bounds with the cut: res[i] = {count, (first_record: batch_first), kept}; keep[i] = kept, lo[i] = the item's first record in
// the uncut list.  Thread n_items writes the closing entries (keep 0, lo n_rec), so that sum[n_items] is the kept total.
__global__ void __launch_bounds__(256) batch_bounds_cut(const u64 *__restrict__ rec, u64 n_rec, const u64 *__restrict__ off, u64 n_items,
                                                        int records, const u64 *__restrict__ prefix, const u64 *__restrict__ flags,
                                                        const BatchCut cut, u64 *__restrict__ res, u64 *__restrict__ keep,
                                                        u64 *__restrict__ lo_out)
{
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n_items)
        return;
    if (i == n_items)
    {
        keep[i] = 0;
        lo_out[i] = n_rec;
        return;
    }
    const u64 lo = first_record_at(rec, n_rec, off[i]), hi = first_record_at(rec, n_rec, off[i + 1]);
    const u64 T = hi - lo;
    u64 have = T;
    if (prefix && n_rec)
    {
        const u64 total = prefix[n_rec - 1] + flags[n_rec - 1];
        have = (hi < n_rec ? prefix[hi] : total) - (lo < n_rec ? prefix[lo] : total);
    }
    u64 count = min(have, cut.m), kept = 0;
    if (cut.m == 0)
        count = (cut.zero_one && T > 0) ? 1 : 0;
    else if (records)
        kept = min(T, cut.m) + (T > cut.m ? (u64)cut.extra : 0ull);
    res[3 * i] = count;
    res[3 * i + 2] = kept;
    keep[i] = kept;
    lo_out[i] = lo;
}

// (a'') first_record = rec_base + the kept records of the items in front
__global__ void __launch_bounds__(256) batch_first(const u64 *__restrict__ new_first, u64 n_items, u64 rec_base, int report,
                                                   u64 *__restrict__ res)
{
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_items)
        res[3 * i + 1] = report ? rec_base + new_first[i] : rec_base;
}

// (b') kept record d of the pack: its item is the last i with new_first[i] <= d (an item that keeps nothing shares its entry with
// its successor and is never the last), its place in the item j = d - new_first[i], its source lo[i] + the inverse of the flush map.
// LDS: new_first[0 .. n_items] fits kBatchLdsItems entries.  REBASE: relative to the item's first byte (what batch_rebase does), in
// the search's order; else pack-relative with the displaced record where its start puts it (the item's last place).
template <bool LDS, bool REBASE>
__global__ void __launch_bounds__(256) batch_cut(const u64 *__restrict__ rec, u64 n_rec, u64 *__restrict__ dst, u64 room,
                                                 const u64 *__restrict__ new_first, const u64 *__restrict__ lo_tab,
                                                 const u64 *__restrict__ off, u64 n_items, const BatchCut cut)
{
    __shared__ u64 s_first[LDS ? kBatchLdsItems : 1];
    // the grid covers `room` (the host's bound, what dst holds); a workgroup behind the kept total leaves before it stages anything
    const u64 n_kept = min(new_first[n_items], room);
    if ((u64)blockIdx.x * kRebasePerBlock >= n_kept)
        return;
    if (LDS)
    {
        for (u32 t = threadIdx.x; t <= (u32)n_items; t += blockDim.x)
            s_first[t] = new_first[t];
        __syncthreads();
    }
    const u64 *tab = LDS ? s_first : new_first;
    const u64 k0 = (u64)blockIdx.x * kRebasePerBlock, k1 = k0 + kRebasePerBlock < n_kept ? k0 + kRebasePerBlock : n_kept;
    for (u64 d = k0 + threadIdx.x; d < k1; d += blockDim.x)
    {
        u64 lo = 0, hi = n_items; // tab[lo] <= d < tab[hi] (tab[0] = 0, tab[n_items] = n_kept > d)
        while (hi - lo > 1)
        {
            const u64 mid = lo + (hi - lo) / 2;
            if (tab[mid] <= d)
                lo = mid;
            else
                hi = mid;
        }
        const u64 j = d - tab[lo], first = lo_tab[lo], T = lo_tab[lo + 1] - first;
        u64 src = j;
        if (cut.displace && T > cut.m)
        {
            if (REBASE)
            { // R[0 .. m-4096), R[m], R[m-4096 .. m-1)
                const u64 f = cut.m - 4096;
                src = j < f ? j : j == f ? cut.m : j - 1;
            }
            else // R[0 .. m-1), R[m]
                src = j + 1 == cut.m ? cut.m : j;
        }
        src += first;
        if (src >= n_rec) // (cannot happen: src - first < T by the rule)
            continue;
        uint4 r = *reinterpret_cast<const uint4 *>(rec + 2 * src);
        if (REBASE)
        {
            const u64 base = off[lo], st = (((u64)r.y << 32) | r.x) - base, e = (((u64)r.w << 32) | r.z) - base;
            r.x = (u32)st; r.y = (u32)(st >> 32); r.z = (u32)e; r.w = (u32)(e >> 32);
        }
        *reinterpret_cast<uint4 *>(dst + 2 * d) = r;
    }
}

std::atomic<size_t> g_pack_limit{0};                       // krep_gpu_debug_batch_pack_limit
thread_local BatchTimes tl_search_times, tl_grep_times;    // krep_gpu_debug_batch_times, krep_gpu_debug_grep_batch_times
std::atomic<uint64_t> g_rebase_lds{0}, g_rebase_global{0}; // krep_gpu_debug_batch_rebase_launches
std::atomic<uint64_t> g_cut_lds{0}, g_cut_global{0};       // krep_gpu_debug_batch_cut_launches

// ---- the segmentation of one pack in steps (batch_segment below)
// the scratch's growth rule: half again what is needed, `floor` at the least
uint64_t grown(uint64_t need, uint64_t floor = 0) { return std::max<uint64_t>(need + need / 2, floor); }
bool counts_lines(const BatchSegment &g) { return g.lines && g.n_rec; } // -c with records: the line prefix step runs
bool cut_keeps_records(const BatchSegment &g) { return g.form != BatchCutOut::None && !g.lines; }
// under a cut the kept records are at most this many (0: none is kept, batch_cut does not run): d_cut and the grid of batch_cut are
// sized by that bound, the kernel reads the kept total itself (no wait between the sum and the cut; the host reads the total behind
// the segmentation, batch_kept_total)
u64 cut_room(const BatchSegment &g)
{
    const u64 per_item = g.cut->m + g.cut->extra;
    if (!cut_keeps_records(g) || !g.n_rec)
        return 0;
    return (per_item && g.n_items > g.n_rec / per_item) ? g.n_rec : g.n_items * per_item;
}

int segment_reserve(BatchScratch &s, const BatchSegment &g)
{
    const uint64_t items = grown(g.n_items, 1024);
    HIPCHK(grow_scratch(s.items_cap, g.n_items, items,
                        {dev_buf(s.d_off, (items + 1) * sizeof(u64)), dev_buf(s.d_res, items * sizeof(krep_gpu_batch_result_t))}));
    if (counts_lines(g))
    {
        const uint64_t recs = grown(g.n_rec, 1u << 16);
        HIPCHK(grow_scratch(s.rec_cap, g.n_rec, recs,
                            {dev_buf(s.d_lines, recs * sizeof(uint64_t)), dev_buf(s.d_flags, recs * sizeof(u64)),
                             dev_buf(s.d_prefix, recs * sizeof(u64)), dev_buf(s.d_sums, (scan_sums_words(recs) + 1) * sizeof(u64))}));
    }
    if (!g.cut)
        return 0;
    HIPCHK(grow_scratch(s.cut_items_cap, g.n_items, items,
                        {dev_buf(s.d_keep, (items + 2) * sizeof(u64)), dev_buf(s.d_new_first, (items + 2) * sizeof(u64)),
                         dev_buf(s.d_lo, (items + 2) * sizeof(u64)), dev_buf(s.d_cut_sums, (scan_sums_words(items + 2) + 1) * sizeof(u64))}));
    if (const u64 room = cut_room(g))
        HIPCHK(grow_scratch(s.cut_cap, room, grown(room, 1u << 12), {dev_buf(s.d_cut, grown(room, 1u << 12) * sizeof(match_position_t))}));
    return 0;
}

// -c: s.d_prefix[k] = the lines opened by the records in front of record k, s.d_flags[k] = whether record k opens one
int segment_line_prefix(BatchScratch &s, const BatchSegment &g, hipStream_t st)
{
    // the line of every record's start, in start order (a multi-pattern list comes in end order: two records of one line may
    // have a record of the next line between them there)
    if (g.by_end && krep_gpu_order_by_start(g.d_pos, g.n_rec, g.packed, st))
        return 2;
    if (krep_gpu_line_numbers(g.d_text, g.packed, g.d_pos, g.n_rec, s.d_lines, st))
        return 2;
    hipLaunchKernelGGL(batch_line_flags, dim3((u32)((g.n_rec + 255) / 256)), dim3(256), 0, st, (const u64 *)s.d_lines, (u64)g.n_rec, s.d_flags);
    scan_exclusive(s.d_flags, g.n_rec, s.d_prefix, s.d_sums, false, st);
    return 0;
}

// the road under a max_count: bounds in emission order, then the cut, then (the caller's) order
int segment_cut(BatchScratch &s, const BatchSegment &g, hipStream_t st)
{
    const u64 *prefix = counts_lines(g) ? s.d_prefix : nullptr, *flags = counts_lines(g) ? s.d_flags : nullptr;
    const u32 grid_i = (u32)((g.n_items + 1 + 255) / 256);
    hipLaunchKernelGGL(batch_bounds_cut, dim3(grid_i), dim3(256), 0, st, (const u64 *)g.d_pos, (u64)g.n_rec, (const u64 *)s.d_off,
                       (u64)g.n_items, cut_keeps_records(g) ? 1 : 0, prefix, flags, *g.cut, s.d_res, s.d_keep, s.d_lo);
    scan_exclusive(s.d_keep, g.n_items + 1, s.d_new_first, s.d_cut_sums, false, st);
    hipLaunchKernelGGL(batch_first, dim3(grid_i), dim3(256), 0, st, (const u64 *)s.d_new_first, (u64)g.n_items, (u64)g.rec_base,
                       g.report ? 1 : 0, s.d_res);
    HIPCHK(hipGetLastError());
    if (const u64 room = cut_room(g))
    {
        const bool lds = g.n_items + 1 <= kBatchLdsItems, rebase = g.form == BatchCutOut::Rebased;
        (lds ? g_cut_lds : g_cut_global).fetch_add(1, std::memory_order_relaxed);
        const auto kernel = lds ? (rebase ? batch_cut<true, true> : batch_cut<true, false>)
                                : (rebase ? batch_cut<false, true> : batch_cut<false, false>);
        hipLaunchKernelGGL(kernel, dim3((u32)((room + kRebasePerBlock - 1) / kRebasePerBlock)), dim3(256), 0, st, (const u64 *)g.d_pos,
                           (u64)g.n_rec, (u64 *)s.d_cut, (u64)room, (const u64 *)s.d_new_first, (const u64 *)s.d_lo, (const u64 *)s.d_off,
                           (u64)g.n_items, *g.cut);
        HIPCHK(hipGetLastError());
    }
    return 0;
}
// the plain road: the bounds, then every record relative to its item
int segment_plain(BatchScratch &s, const BatchSegment &g, hipStream_t st)
{
    const u64 *prefix = counts_lines(g) ? s.d_prefix : nullptr, *flags = counts_lines(g) ? s.d_flags : nullptr;
    hipLaunchKernelGGL(batch_bounds, dim3((u32)((g.n_items + 255) / 256)), dim3(256), 0, st, (const u64 *)g.d_pos, (u64)g.n_rec,
                       (const u64 *)s.d_off, (u64)g.n_items, (u64)g.rec_base, g.report ? 1 : 0, prefix, flags, s.d_res);
    if (g.report && !g.lines && g.n_rec)
    {
        const u32 grid = (u32)((g.n_rec + kRebasePerBlock - 1) / kRebasePerBlock);
        const bool lds = g.n_items + 1 <= kBatchLdsItems; // off[0 .. n_items] is n_items + 1 entries
        (lds ? g_rebase_lds : g_rebase_global).fetch_add(1, std::memory_order_relaxed);
        hipLaunchKernelGGL(lds ? batch_rebase<true> : batch_rebase<false>, dim3(grid), dim3(256), 0, st, (u64 *)g.d_pos, (u64)g.n_rec,
                           (const u64 *)s.d_off, (u64)g.n_items);
    }
    HIPCHK(hipGetLastError());
    return 0;
}

} // namespace

void batch_scratch_free(BatchScratch &s)
{
    for (void *p : {(void *)s.d_off, (void *)s.d_res, (void *)s.d_lines, (void *)s.d_flags, (void *)s.d_prefix, (void *)s.d_sums,
                    (void *)s.d_pfx, (void *)s.d_pfx_off, (void *)s.d_item_out, (void *)s.d_out, (void *)s.d_keep, (void *)s.d_new_first,
                    (void *)s.d_lo, (void *)s.d_cut_sums, (void *)s.d_cut})
        if (p)
            (void)hipFree(p);
    s = BatchScratch{};
}

int batch_kept_total(const BatchScratch &s, uint64_t n_items, uint64_t n_rec, uint64_t *n_kept)
{
    u64 kept = 0;
    HIPCHK(hipMemcpy(&kept, s.d_new_first + n_items, sizeof kept, hipMemcpyDeviceToHost));
    if (kept > n_rec)
        return fail("batch: the cut keeps %llu of %llu records", (unsigned long long)kept, (unsigned long long)n_rec);
    *n_kept = kept;
    return 0;
}

int batch_segment(BatchScratch &s, const BatchSegment &g, hipStream_t st)
{
    if (!g.n_items)
        return 0;
    if (segment_reserve(s, g))
        return 2;
    HIPCHK(hipMemcpyAsync(s.d_off, g.h_off, (g.n_items + 1) * sizeof(u64), hipMemcpyHostToDevice, st));
    if (counts_lines(g) && segment_line_prefix(s, g, st))
        return 2;
    return g.cut ? segment_cut(s, g, st) : segment_plain(s, g, st);
}

// ------------------------------------------------------------------------------------------------ when packing is exact
// NULL: result(A + '\n' + B) = result(A), then result(B) shifted by |A| + 1, for all texts A and B (DESIGN.md §9 carries the code line
// that makes each refused class depend on where a line stands in the text).
const char *batch_unsupported_reason(const search_params_t *p, const krep_gpu_config_t &c)
{
    if (const char *why = unsupported_reason(p, c))
        return why;
    const bool cutting = p->max_count != SIZE_MAX;
    if (cutting && !g_batch_max_count.load(std::memory_order_relaxed))
        return "batch: max_count is a property of each item's own record list; cutting per item is follow-up work";
    if (p->use_regex)
    {
        RegexCompiled rc;
        if (const char *why = regex_compile_cached(p, &rc))
            return why;
        // (a line walk's classes never hold '\n', and its one-window rule is no reason against a pack: a pack is one window)
        if (rc.holds_newline())
            return "batch: a byte class of the expression holds '\\n': a match could take in the separator between two items";
        if (rc.has_eol() && !p->case_sensitive)
            return "batch: $ in a case-insensitive search: the end of the text ends no line there (REG_NOTEOL, krep.c:1420), which holds "
                   "at the end of every item alone and in a pack only at the end of the last";
        return nullptr;
    }
    NormParams np(p);
    if (!np.valid)
        return "no pattern";
    const search_params_t *q = &np.sp;
    for (size_t i = 0; i < q->num_patterns; ++i)
        if (q->pattern_lens[i] && memchr(q->patterns[i], '\n', q->pattern_lens[i]))
            return "batch: a pattern holds '\\n': a match could take in the separator between two items";
    if (q->num_patterns > 1)
        return nullptr;
    const size_t m = q->pattern_len;
    if (m == 0)
        return nullptr;
    // the function that does the work on a text that is not shorter than the pattern (a shorter item holds no match under any of them)
    const int algo = mirror_effective(mirror_top(q, c), q, m);
    const bool lines = q->count_lines_mode, ww = q->whole_word, om = c.only_matching != 0;
    if (lines && (algo == KREP_RA_AVX512 || algo == KREP_RA_NEON || (algo == KREP_RA_AVX2 && ww)))
        return "batch: -c through the block loop of simd_avx512_search / simd_avx2_search -w / neon_search replays the end of the TEXT "
               "(krep.c:5203-5218, :5000-5013, :4590-4611): an item's count depends on where the item ends";
    if (algo == KREP_RA_AVX512)
        return "batch: simd_avx512_search leaves the last full 64-byte block of the TEXT unexamined (krep.c:5171): which block that is "
               "depends on the length of everything in front of it";
    if (ww && (algo == KREP_RA_AVX2 || algo == KREP_RA_NEON))
        return "batch: -w through the scalar tail of simd_avx2_search / neon_search: the first byte of the TEXT's tail has no left "
               "neighbour (krep.c:5059-5097), and where that tail begins depends on the whole text's length";
    if (om && !lines && (algo == KREP_RA_AVX2 || algo == KREP_RA_NEON) && pattern_has_border((const uint8_t *)q->pattern, m))
        return "batch: -o through simd_avx2_search / neon_search with a pattern that can overlap itself: the block body reports every "
               "occurrence, the scalar tail is boyer_moore_search, which skips a match's length under -o (krep.c:1371), and where that "
               "tail begins depends on the whole text's length";
    if (algo == KREP_RA_MEMCHR_SHORT && om && lines)
        return "batch: -c with -o through memchr_short_search jumps to the next line start after every counted line (krep.c:4449-4470): "
               "one window over one text only";
    if (algo == KREP_RA_MEMCHR_SHORT && om && m >= 3)
        return "batch: memchr_short_search under -o skips pattern_len bytes behind a failed candidate too (krep.c:4495): with a 3-byte "
               "pattern a candidate on the last byte of an item steps over the first byte of the next one";
    if (cutting && q->max_count == 0 && algo == KREP_RA_NEON)
        return "batch: max_count == 0 through neon_search: a count-only search hands the TEXT's last length % 16 bytes to "
               "boyer_moore_search, whose first hit answers 1 (krep.c:4516, :1355-1367): an item's answer depends on where the item ends";
    if (cutting && q->max_count == 0 && algo == KREP_RA_AVX2 && !lines && !q->track_positions)
        return "batch: max_count == 0, count-only, through simd_avx2_search: a hit in the block body answers 1, a hit in the scalar tail "
               "is capped back to 0 (krep.c:5036, :5066-5093), and where that tail begins depends on the whole text's length";
    return nullptr;
}

// The cut of one item's list as a function of (params, cfg): the reference function is taken as batch_unsupported_reason takes it, and
// every field is read off the scans' own verdict (verdict_rule) and memchr_batch_quirk's predicate — probes, not a second table.
// search_file_cap: krep_gpu_grep_batch repeats search_file() behind the function (krep.c:2954-2981, :3018-3026): the list and the
// count are capped at max_count there, so kmp_search's extra record and the count-only 1 at max_count == 0 go.
BatchCut batch_cut_rule(const search_params_t *p, const krep_gpu_config_t &c, bool search_file_cap)
{
    const int algo = mirror_effective(mirror_top(p, c), p, p->pattern_len);
    const size_t m = p->max_count;
    BatchCut k{};
    k.m = m;
    if (!search_file_cap)
    {
        k.zero_one = (uint32_t)verdict_rule(algo, 0, p->count_lines_mode, p->track_positions, 1, 1, true).ret;
        const Verdict over = verdict_rule(algo, 1, false, true, 2, 2, true); // one record beyond max_count
        k.extra = (uint32_t)(over.store - over.ret);
    }
    k.displace = algo == KREP_RA_MEMCHR && memchr_flush_displaces((uint64_t)m + 1, m) ? 1 : 0;
    return k;
}

namespace {
// ------------------------------------------------------------------------------------------------ what both calls share
// A call is: BatchWalk::enter (nothing on the device yet), its own checks, device_ready, an empty batch answered, start, then per pack
// next() and pack() with the call's own fields of the job, then the call's commit of its results — at the very end only, so that a
// failure leaves the caller's memory as it was.
using clk = std::chrono::steady_clock;
double ms_since(clk::time_point t) { return std::chrono::duration<double, std::milli>(clk::now() - t).count(); }

struct BatchWalk
{
    BatchTimes &times; // the calling thread's instance for this call
    krep_gpu_config_t cfg{};
    std::optional<NormParams> np;
    const search_params_t *params = nullptr; // the caller's, normalised
    search_params_t scan{}; // the pack is scanned with RECORDS whatever the caller wants back: the list is what gets cut per item, under -c too
    BatchCut cut{};         // a finite max_count (the switch is on: the batch rule): the unlimited list is cut per item behind the scan
    bool no_trie = false;   // aho_corasick.c:306: no trie, no matches — every count stays 0, nothing is scanned
    size_t limit = 0;       // the packed size at which a further pack begins
    std::optional<DeviceGuard> guard; // taken with the first pack
    size_t n_items = 0, i0 = 0, i1 = 0; // the pack in hand: items [i0, i1)
    std::vector<uint64_t> off;          // ... its offset table
    BatchPackJob job{}; // ... and its job: items and cut from here; the call sets lines / report / records / appended / step / form
    krep_gpu_batch_info_t bi{};
    explicit BatchWalk(BatchTimes &t) : times(t) {}

    // What both calls do first, in this order: the error cleared, *info and the times zeroed, `null_pointer` (the call's own test)
    // with its message, the configuration, the batch rule, "no pattern".  -> 2 and the message
    int enter(const char *null_msg, bool null_pointer, const search_params_t *raw, const krep_gpu_config_t *cfg_in, krep_gpu_batch_info_t *info)
    {
        krep_gpu_clear_error();
        if (info)
            *info = krep_gpu_batch_info_t{};
        times = BatchTimes{};
        if (null_pointer)
            return fail("%s", null_msg);
        cfg = cfg_in ? *cfg_in : current_config();
        if (const char *why = batch_unsupported_reason(raw, cfg))
            return fail("%s", why);
        np.emplace(raw);
        params = &np->sp;
        return np->valid ? 0 : fail("no pattern");
    }
    int device_ready() const // the last refusal, behind the call's own: every refusal comes before any device work
    {
        const char *why = device_unusable(cfg.device);
        return why ? fail("%s", why) : 0;
    }
    void start(const krep_gpu_batch_item_t *items, size_t n, bool search_file_cap /* see batch_cut_rule */)
    {
        n_items = n;
        scan = *params;
        scan.count_lines_mode = false;
        scan.track_positions = true;
        scan.max_count = SIZE_MAX;
        if (params->max_count != SIZE_MAX)
            cut = batch_cut_rule(params, cfg, search_file_cap);
        job = BatchPackJob{}; // (the call's own fields: none, no records, no step)
        job.scan = &scan, job.cfg = &cfg, job.items = items;
        job.cut = params->max_count != SIZE_MAX ? &cut : nullptr;
        job.form = BatchCutOut::None;
        no_trie = params->num_patterns > 1 && !params->ac_trie && !params->use_regex; // (several -E patterns are one alternation)
        const size_t chunk = cfg.stream_chunk_bytes ? cfg.stream_chunk_bytes : ((size_t)128 << 20);
        limit = g_pack_limit.load() ? g_pack_limit.load() : 2 * chunk;
    }
    // the next pack, cut between items and never inside one (an item beyond the limit is a pack of its own); false: none is left
    bool next()
    {
        job.items += i1 - i0;
        i0 = i1;
        if (no_trie || i0 >= n_items)
            return false;
        if (!guard)
            guard.emplace(); // (behind the no-trie answer: that one needs no device)
        job.n = batch_pack_offsets(job.items, n_items - i0, limit, off);
        job.off = off.data();
        i1 = i0 + job.n;
        return true;
    }
    int pack(krep_gpu_batch_result_t *res /* [n_items] */, BatchPackDone *done)
    {
        const int rc = host_batch_pack(job, res + i0, done);
        times += done->ms;
        if (rc)
            return 2;
        bi.packed_bytes += off.back() - 1;
        bi.scans += 1;
        bi.total_records += done->n_rec;
        bi.kernel_ms += done->kernel_ms;
        return 0;
    }
};

// ------------------------------------------------------------------------------------------------ the grep output of a batch
// krep_gpu_grep_batch's own refusals, between the entry and the device: search_file()'s own branch (krep.c:3014-3027), the format,
// per item its text and then its prefix, the output block
int grep_batch_refuse(const search_params_t *raw, const krep_gpu_batch_item_t *items, size_t n_items, const krep_gpu_grep_format_t *fmt,
                      const krep_gpu_grep_output_t *out)
{
    if (!(raw->count_lines_mode || raw->count_matches_mode) && !raw->track_positions)
        return fail("grep_batch: track_positions == false outside -c: the reference prints its empty-match line then (krep.c:3029-3038), "
                    "which no batchable search produces");
    if (fmt->line.prefix_len || fmt->match.prefix_len)
        return fail("grep_batch: the prefix of fmt->line / fmt->match must be empty: the prefixes are per item");
    const char *str[6] = {fmt->line.before_match, fmt->line.after_match, fmt->line.line_close,
                          fmt->match.before_number, fmt->match.after_number, fmt->match.after_match};
    const size_t len[6] = {fmt->line.before_match_len, fmt->line.after_match_len, fmt->line.line_close_len,
                           fmt->match.before_number_len, fmt->match.after_number_len, fmt->match.after_match_len};
    for (int k = 0; k < 6; ++k)
        if ((len[k] && !str[k]) || (len[k] >> 20))
            return fail("grep_batch: a string of the format is NULL with a length, or longer than 2^20 bytes");
    for (size_t i = 0; i < n_items; ++i)
    {
        if (!items[i].text && items[i].len)
            return fail("grep_batch: item %zu has a NULL text and a length of %zu", i, items[i].len);
        if ((fmt->prefix_lens[i] && !fmt->prefixes[i]) || (fmt->prefix_lens[i] >> 20))
            return fail("grep_batch: the prefix of item %zu is NULL with a length, or longer than 2^20 bytes", i);
    }
    if (out->len > out->capacity || (!out->bytes && out->capacity))
        return fail("grep_batch: out holds %zu bytes in a block of %zu", out->len, out->capacity);
    return 0;
}

// The caller's block while a call appends to it: the bytes go behind len0 + appended, out->len moves at the very end only
struct GrepOut
{
    krep_gpu_grep_output_t *out;
    size_t len0;
    uint64_t appended = 0;
    char *end() const { return out->bytes + len0 + appended; }
    bool host_room(uint64_t more) // out->bytes holds len0 + appended + more bytes
    {
        const size_t need = len0 + appended + more;
        if (need <= out->capacity)
            return true;
        const size_t cap = std::max<size_t>({need, 2 * out->capacity, (size_t)4096});
        char *p = (char *)realloc(out->bytes, cap);
        if (!p)
            return false;
        out->bytes = p;
        out->capacity = cap;
        return true;
    }
};
struct GrepCall // what the steps below need of one krep_gpu_grep_batch call
{
    const krep_gpu_grep_format_t *fmt;
    bool om;
    GrepOut out;
    std::vector<krep_gpu_grep_item_t> pi; // per_item until the commit
    const BatchWalk &walk; // (i0: the first item of the pack in hand; times: the call's stage clocks)
    std::vector<uint64_t> poff, item_out;
    std::vector<uint8_t> blob;
};

// The BatchStep of a pack, between its segmentation and its read-back: the items' prefixes onto the device, the pack formatted where it
// lies, its bytes copied behind what the block holds, the items' places noted
int grep_format_pack(GrepCall &g, const BatchPackOnDevice &p)
{
    auto t0 = clk::now();
    BatchScratch &s = p.scratch;
    const size_t n = (size_t)p.n_items;
    g.item_out.assign(n + 1, 0);
    uint64_t bytes = 0;
    if (p.n_rec)
    {
        if (p.by_end && krep_gpu_order_by_start(p.d_pos, p.n_rec, p.packed, nullptr))
            return 2;
        (void)batch_prefix_blob(g.fmt->prefixes + g.walk.i0, g.fmt->prefix_lens + g.walk.i0, n, (size_t)1 << 20, g.blob, g.poff); // (checked at entry)
        if (inject(1))
            return fail("grep_batch: device allocation failed (injected)");
        HIPCHK(grow_scratch(s.pfx_cap, g.blob.size(), grown(g.blob.size()) + 4096, {dev_buf(s.d_pfx, grown(g.blob.size()) + 4096)}));
        const uint64_t want = std::max<uint64_t>(n + 1 + n / 2, 1024);
        HIPCHK(grow_scratch(s.grep_items_cap, n + 1, want, {dev_buf(s.d_pfx_off, want * sizeof(u64)), dev_buf(s.d_item_out, want * sizeof(u64))}));
        if (inject(2))
            return fail("grep_batch: H2D copy of the prefixes failed (injected)");
        if (!g.blob.empty())
            HIPCHK(hipMemcpyAsync(s.d_pfx, g.blob.data(), g.blob.size(), hipMemcpyHostToDevice, nullptr));
        HIPCHK(hipMemcpyAsync(s.d_pfx_off, g.poff.data(), (n + 1) * sizeof(u64), hipMemcpyHostToDevice, nullptr));
        const krep_gpu_pack_view_t view{(const uint64_t *)p.d_off, (uint64_t)n, s.d_pfx, (const uint64_t *)s.d_pfx_off};
        const FormatOutGrow grow = [&s](size_t want) -> void * { // the rule of the other scratch: grown by half again
            if (grow_scratch(s.out_cap, want, grown(want), {dev_buf(s.d_out, grown(want))}) == hipSuccess)
                return s.d_out;
            (void)hipGetLastError();
            (void)fail("grep_batch: allocation of %zu bytes for the formatted output failed", (size_t)grown(want));
            return nullptr;
        };
        if (inject(3))
            return fail("grep_batch: launch of the pack formatter failed (injected)");
        krep_gpu_matches_out_t mo{};
        krep_gpu_lines_out_t lo{};
        if (g.om ? format_matches_items(p.d_text, p.packed, &view, p.d_pos, p.n_rec, &g.fmt->match, nullptr, 0, &grow, (uint64_t *)s.d_item_out, &mo, nullptr)
                 : format_lines_items(p.d_text, p.packed, &view, p.d_pos, p.n_rec, &g.fmt->line, nullptr, 0, &grow, (uint64_t *)s.d_item_out, &lo, nullptr))
            return 2;
        bytes = g.om ? mo.out_bytes : lo.out_bytes;
        g.walk.times.format += ms_since(t0);
        t0 = clk::now();
        if (inject(4))
            return fail("D2H copy of the formatted output failed (injected)");
        if (!g.out.host_room(bytes))
            return fail("grep_batch: out of memory growing the output to %zu bytes", (size_t)(g.out.len0 + g.out.appended + bytes));
        if ((bytes && hipMemcpy(g.out.end(), s.d_out, bytes, hipMemcpyDeviceToHost) != hipSuccess) ||
            hipMemcpy(g.item_out.data(), s.d_item_out, (n + 1) * sizeof(u64), hipMemcpyDeviceToHost) != hipSuccess)
            return fail("D2H copy of the formatted output failed");
        g.walk.times.read_back += ms_since(t0);
    }
    for (size_t k = 0; k < n; ++k)
        g.pi[g.walk.i0 + k] = krep_gpu_grep_item_t{0, g.out.appended + g.item_out[k], g.item_out[k + 1] - g.item_out[k]};
    g.out.appended += bytes;
    return 0;
}

// -c: the counts are printed on the host, prefix COUNT '\n' for every item
int grep_print_counts(GrepCall &g, const krep_gpu_batch_result_t *res, size_t n_items)
{
    const auto t0 = clk::now();
    const krep_gpu_grep_format_t *fmt = g.fmt;
    uint64_t total = 0;
    for (size_t i = 0; i < n_items; ++i)
        total += fmt->prefix_lens[i] + 21;
    if (!g.out.host_room(total))
        return fail("grep_batch: out of memory growing the output by %zu bytes", (size_t)total);
    for (size_t i = 0; i < n_items; ++i)
    {
        char *dst = g.out.end();
        if (fmt->prefix_lens[i])
            memcpy(dst, fmt->prefixes[i], fmt->prefix_lens[i]);
        char num[24];
        const int d = snprintf(num, sizeof num, "%llu\n", (unsigned long long)res[i].count);
        memcpy(dst + fmt->prefix_lens[i], num, (size_t)d);
        g.pi[i] = krep_gpu_grep_item_t{0, g.out.appended, fmt->prefix_lens[i] + (uint64_t)d};
        g.out.appended += g.pi[i].out_bytes;
    }
    g.walk.times.read_back += ms_since(t0);
    return 0;
}
} // namespace
} // namespace kg

extern "C" void krep_gpu_debug_batch_pack_limit(size_t bytes) { g_pack_limit.store(bytes); }
extern "C" void krep_gpu_debug_batch_times(double *pack_ms, double *scan_ms, double *segment_ms, double *readback_ms)
{
    const BatchTimes &t = tl_search_times;
    if (pack_ms) *pack_ms = t.pack;
    if (scan_ms) *scan_ms = t.scan;
    if (segment_ms) *segment_ms = t.segment;
    if (readback_ms) *readback_ms = t.read_back;
}
extern "C" void krep_gpu_debug_grep_batch_times(double *pack_ms, double *scan_ms, double *segment_ms, double *format_ms, double *readback_ms)
{
    const BatchTimes &t = tl_grep_times;
    if (pack_ms) *pack_ms = t.pack;
    if (scan_ms) *scan_ms = t.scan;
    if (segment_ms) *segment_ms = t.segment;
    if (format_ms) *format_ms = t.format;
    if (readback_ms) *readback_ms = t.read_back;
}

extern "C" void krep_gpu_debug_batch_rebase_launches(uint64_t *lds_table, uint64_t *global_table)
{
    if (lds_table) *lds_table = g_rebase_lds.load();
    if (global_table) *global_table = g_rebase_global.load();
}

extern "C" void krep_gpu_debug_batch_cut_launches(uint64_t *lds_table, uint64_t *global_table)
{
    if (lds_table) *lds_table = g_cut_lds.load();
    if (global_table) *global_table = g_cut_global.load();
}

extern "C" int krep_gpu_debug_batch_fill_host(const krep_gpu_batch_item_t *items, size_t n, size_t lo, size_t cnt, void *dst)
{
    std::vector<uint64_t> off;
    if (!n || !items || kg::batch_pack_offsets(items, n, UINT64_MAX, off) != n)
        return 2;
    const uint64_t packed = off.back() - 1;
    if (lo > packed || cnt > packed - lo)
        return 2; // [lo, lo + cnt) leaves the pack
    if (cnt)
        kg::batch_fill(items, off.data(), n, (uint8_t *)dst, lo, cnt);
    return 0;
}

extern "C" int krep_gpu_batch_can_accelerate(const search_params_t *params)
{
    krep_gpu_clear_error();
    const krep_gpu_config_t c = kg::current_config();
    const char *why = kg::batch_unsupported_reason(params, c);
    if (!why)
        why = kg::device_unusable(c.device);
    if (why)
        kg::note_error(why);
    return why ? 0 : 1;
}

extern "C" int krep_gpu_search_batch(const search_params_t *raw, const krep_gpu_config_t *cfg_in, const krep_gpu_batch_item_t *items,
                                     size_t n_items, krep_gpu_batch_result_t *results, match_result_t *records,
                                     krep_gpu_batch_info_t *info)
{
    BatchWalk w(tl_search_times);
    if (w.enter("search_batch: NULL params / items / results", !raw || (n_items && (!items || !results)), raw, cfg_in, info))
        return 2;
    for (size_t i = 0; i < n_items; ++i)
        if (!items[i].text && items[i].len)
            return kg::fail("search_batch: item %zu has a NULL text and a length of %zu", i, items[i].len);
    if (w.device_ready())
        return 2;
    if (!n_items)
        return 0;
    const bool lines = w.params->count_lines_mode;
    const bool report = w.params->track_positions && records != nullptr && !lines;
    const uint64_t count0 = records ? records->count : 0;
    std::vector<krep_gpu_batch_result_t> res(n_items, krep_gpu_batch_result_t{0, count0, 0}); // (what no trie answers)
    w.start(items, n_items, false);
    w.job.lines = lines, w.job.report = report, w.job.records = records;
    w.job.form = report ? BatchCutOut::Rebased : BatchCutOut::None;
    for (BatchPackDone done; w.next();)
    {
        if (w.pack(res.data(), &done))
            return 2; // (records->count was never moved: nothing is appended)
        if (report)
            w.job.appended += w.job.cut ? done.n_kept : done.n_rec;
    }
    memcpy(results, res.data(), n_items * sizeof *results);
    if (report)
        records->count = count0 + w.job.appended;
    if (info)
        *info = w.bi;
    return 0;
}

extern "C" int krep_gpu_grep_batch(const search_params_t *raw, const krep_gpu_config_t *cfg_in, const krep_gpu_batch_item_t *items,
                                   size_t n_items, const krep_gpu_grep_format_t *fmt, krep_gpu_grep_item_t *per_item,
                                   krep_gpu_grep_output_t *out, krep_gpu_batch_info_t *info)
{
    BatchWalk w(tl_grep_times);
    if (w.enter("grep_batch: NULL params / items / fmt / per_item / out",
                !raw || !fmt || !out || (n_items && (!items || !per_item || !fmt->prefixes || !fmt->prefix_lens)), raw, cfg_in, info))
        return 2;
    if (grep_batch_refuse(raw, items, n_items, fmt, out) || w.device_ready())
        return 2;
    if (!n_items)
        return 0;
    const bool count_mode = raw->count_lines_mode || raw->count_matches_mode;
    GrepCall g{fmt, !count_mode && w.cfg.only_matching, GrepOut{out, out->len}, std::vector<krep_gpu_grep_item_t>(n_items), w};
    std::vector<krep_gpu_batch_result_t> res(n_items, krep_gpu_batch_result_t{0, 0, 0});
    const BatchStep format = [&g](const BatchPackOnDevice &p) { return grep_format_pack(g, p); };
    w.start(items, n_items, true); // (a finite max_count: search_file()'s cut per item; the formatter sees the kept list only)
    w.job.lines = count_mode && raw->count_lines_mode;
    w.job.step = count_mode ? nullptr : &format;
    w.job.form = count_mode ? BatchCutOut::None : BatchCutOut::PackSorted;
    for (BatchPackDone done; w.next();)
        if (w.pack(res.data(), &done))
            return 2; // (out->len was never moved: nothing is appended)
    if (count_mode && grep_print_counts(g, res.data(), n_items))
        return 2;
    for (size_t i = 0; i < n_items; ++i)
        g.pi[i].count = res[i].count;
    memcpy(per_item, g.pi.data(), n_items * sizeof *per_item);
    out->len = g.out.len0 + g.out.appended;
    if (info)
        *info = w.bi;
    return 0;
}
