// kg_matches.hip — the reference's -o output on a text that is resident in HBM: one `FILE:LINE:match` per record, as
// print_matching_items() writes it in only-matching mode (krep.c:517-793), with or without its colour strings.
//
// Contract (restated from krep.c:597-780; the record list is in (start, end) order and already cut to max_count records, as
// search_file() leaves it, n = result->count):
//   * record i < min(n, max_items) prints  prefix before_number LINE ':' after_number MATCH after_match '\n'; the four strings are
//     the caller's (the escape codes of krep.h:34-39 under --color=always, nothing but "FILE:" without);
//   * MATCH = text[start, min(end, text_len)) with every '\n' replaced by a blank (:736-747);
//   * LINE = 1 + the newlines in [0, start) — except that with more than 10 records the reference looks the line up in an index of
//     the text's N newlines (:531-556, :619-653), and a record that starts behind the last newline finds nothing there and prints
//     what the search before it left: LINE of the nearest earlier record that starts at or before the last newline, else 1.  On an
//     ascending list those records are a suffix, and they are the records whose true number is N + 1.
//
// Steps: (1) the newline-count pass of kg_format.hip over the text and its sum: N and the newlines in front of every 4 KiB block;
// (2) per record its true line number, counted from the NEARER end of its own block in 16-byte steps; the same kernel refuses a
// list that is not ascending or points outside the text, and leaves the largest number <= N in a counter word: the stale value;
// (3) per record the number it prints and its byte count (the stale value's digits are known only now), summed; (4) the gather,
// dealt by OUTPUT bytes: a lane owns 16 aligned bytes of the output, a wave 1 KiB, the first record of a tile comes from a binary
// search in the summed offsets.  A call reads the text once in (1), then only around the records and what it copies.
//
// krep_gpu_format_matches_window is the same output for a WINDOW of a text (a buffer that holds text[global_base, + text_len), records
// with offsets in the whole text, any consecutive run of its list).  Two numbers couple a window to the rest of the text, and the caller
// chains them: the newlines in front of the buffer, and the stale value the records in front of the list leave.  "Behind the last newline"
// is decided by offset against last_newline1, which the caller states (the window does not know N).  Its kernels (mw_*) mirror the steps:
// (1) unchanged on the buffer, (2w) mw_lines, (3w) mw_sizes, (4w) om_gather<true> = the gather with the source moved by global_base,
// (5w) mw_count_to: the newlines in front of count_to, the next window's carry.  The whole-text call keeps its kernels.
//
// Host side of both calls (the shared pieces are kg_format_host.h's): out, fmt_enter — the window call with its own pointer test and
// `win` in front of it — the strings of om_strings (FormatStrings::refuse), the call's own checks; under g_fmt_mu the scratch from
// om_layout (one layout for both), the strings' upload, the kernels above, the read-back of the counter words and the total (each
// call's own: the window reads four words and takes *out back on a refusal), fmt_gather with om_gather<WIN> as its launch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>

#include "../../include/krep_gpu.h"
#include "kg_device.h"
#include "kg_format_dev.h"
#include "kg_format_host.h"
#include "kg_internal.h"

namespace kg {

// (kOmStaleAfter, kOmMaxText, nl_count, om_digits, om_find, OmFixed, OmItem / om_item / om_byte and om_blank live in kg_format_dev.h:
// kg_batch_format.hip formats a pack of items with the same helpers)

// (2) line[i] = 1 + the newlines in front of record i's start; before[] = newlines in front of every 4 KiB block, one entry more
// than the text has blocks (its last entry is N).  A record that may not be read raises ctr[0] and touches no text.  ctr[1]: the
// largest line number <= N (0: none), i.e. that of the last record with a newline at or behind its start
__global__ __launch_bounds__(256) void om_lines(const uint8_t *__restrict__ text, u64 text_len, const u64 *__restrict__ rec, u64 n,
                                                const u64 *__restrict__ before, u64 nblocks, u64 *__restrict__ line,
                                                u64 *__restrict__ ctr)
{
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    u64 ln = 0;
    if (i < n)
    {
        const uint4 r = *reinterpret_cast<const uint4 *>(rec + 2 * i);
        const u64 s = ((u64)r.y << 32) | r.x, e = ((u64)r.w << 32) | r.z;
        if (s >= text_len || e < s || (i > 0 && rec[2 * (i - 1)] > s))
            ctr[0] = 1; // (every writer stores the same value)
        else
        {
            const u64 b = s / kLineBlock, base = b * kLineBlock, lim = min(base + kLineBlock, text_len);
            ln = s - base <= lim - s ? 1 + before[b] + nl_count(text, base, s) : 1 + before[b + 1] - nl_count(text, s, lim);
        }
        line[i] = ln;
    }
    u64 m = ln <= before[nblocks - 1] ? ln : 0ull;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1)
        m = max(m, (u64)__shfl_xor(m, o));
    if ((threadIdx.x & 63u) == 0 && m)
        (void)__hip_atomic_fetch_max(ctr + 1, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// (3) the number record i prints (line[i], in place) and what it adds to the output; entry n: 0, so that the summed entry n is the
// total.  (On a refused list the numbers mean nothing; nothing is read through them, and the host reports the refusal)
__global__ __launch_bounds__(256) void om_sizes(const u64 *__restrict__ rec, u64 n, u64 text_len, const u64 *__restrict__ total_newlines,
                                                u64 max_items, u64 fixed, const u64 *__restrict__ ctr, u64 *__restrict__ line,
                                                u64 *__restrict__ bytes)
{
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n)
        return;
    if (i == n || i >= max_items)
    {
        bytes[i] = 0;
        return;
    }
    const u64 newlines = *total_newlines;
    u64 ln = line[i];
    if (n > kOmStaleAfter && newlines && ln == newlines + 1)
    {
        ln = max(ctr[1], 1ull);
        line[i] = ln;
    }
    const u64 s = rec[2 * i], e = min(rec[2 * i + 1], text_len);
    bytes[i] = fixed + om_digits(ln) + 1 + (e - s) + 1;
}

// (4) chunk c is the 16 aligned bytes at (out - misalign) + 16 c, i.e. output offsets [16 c - misalign, + 16); `emit` records add bytes
// text_len: the length of the WHOLE text, the clamp of a record's end in both instantiations.  WIN: the window call's gather — text[0] is
// byte `win_base` of the whole text (the whole-text call passes win_base = 0 and does not read it)
template <bool WIN>
__global__ __launch_bounds__(256) void om_gather(const uint8_t *__restrict__ text, u64 text_len, const u64 *__restrict__ rec,
                                                 const u64 *__restrict__ line, const u64 *__restrict__ off, u64 emit,
                                                 const uint8_t *__restrict__ fix, const OmFixed f, uint8_t *__restrict__ out, u64 total,
                                                 u32 misalign, u64 nchunks, u64 win_base)
{
    const u64 base = WIN ? win_base : 0ull;
    const u32 lane = threadIdx.x & 63u;
    const u64 wid = (u64)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), nw = (u64)gridDim.x * (blockDim.x >> 6);
    for (u64 c0 = wid * 64; c0 < nchunks; c0 += nw * 64)
    {
        // the records of the wave's 1 KiB tile
        const u64 tile_lo = c0 ? c0 * 16 - misalign : 0ull, tile_hi = min((c0 + 64) * 16 - misalign, total) - 1;
        const u64 r_lo = om_find(off, 0, emit - 1, tile_lo), r_hi = om_find(off, r_lo, emit - 1, tile_hi);
        const u64 c = c0 + lane;
        if (c >= nchunks)
            continue;
        const u64 o0 = c ? c * 16 - misalign : 0ull, o1 = min((c + 1) * 16 - misalign, total);
        const bool whole = o1 - o0 == 16;
        u64 r = om_find(off, r_lo, r_hi, o0);
        OmItem it = om_item(rec, line, text_len, f, r, base);
        u64 k = o0 - off[r];
        if (whole && k >= it.b4 && k + 16 <= it.b5) // wholly inside one match
        {
            const uint4 v = load_unaligned<uint4>(text + it.src + (k - it.b4));
            *reinterpret_cast<uint4 *>(out + o0) = make_uint4(om_blank(v.x), om_blank(v.y), om_blank(v.z), om_blank(v.w));
            continue;
        }
        u32 w[4] = {0, 0, 0, 0};
        const u32 shift = (u32)(o0 + misalign - c * 16); // bytes of the chunk in front of the output (chunk 0 only)
        const u32 cnt = (u32)(o1 - o0);
#pragma unroll
        for (u32 q = 0; q < 16; ++q)
        {
            if (q >= shift && q - shift < cnt)
            {
                if (k > it.b6) // the record is used up (every emitted record adds bytes)
                {
                    it = om_item(rec, line, text_len, f, ++r, base);
                    k = 0;
                }
                w[q >> 2] |= om_byte(text, fix, f, it, k) << (8 * (q & 3u));
                ++k;
            }
        }
        if (whole)
            *reinterpret_cast<uint4 *>(out + o0) = make_uint4(w[0], w[1], w[2], w[3]);
        else
        {
#pragma unroll
            for (u32 q = 0; q < 16; ++q)
                if (q >= shift && q - shift < cnt)
                    out[o0 + (q - shift)] = (uint8_t)(w[q >> 2] >> (8 * (q & 3u)));
        }
    }
}

// ---- the same output for a WINDOW of a text (krep_gpu_format_matches_window) ----
// The buffer `text` holds the whole text's bytes [base, base + buf_len); the records carry offsets in the whole text; the 4 KiB blocks
// of before[] are the BUFFER's.  What the window cannot count itself comes in: nl_before, the newlines in front of `base`.
struct MwWindow
{
    u64 base, buf_len, global_len; // base + buf_len <= global_len
    u64 nl_before;                 // '\n' bytes in front of base
    u64 last_nl1;                  // offset of the whole text's last '\n', + 1 (0: none)
    u64 stale_in;                  // the stale value the lists in front of this one leave (0: none)
    u32 stale_rule;                // the whole list holds more than 10 records
};

// (2w) om_lines with the window's bounds: line[i] = 1 + nl_before + the newlines of the buffer in front of record i's start.
// ctr[0]: refused; ctr[1]: the largest line number among the records that start at or before the last newline (0: none)
__global__ __launch_bounds__(256) void mw_lines(const uint8_t *__restrict__ text, const MwWindow w, const u64 *__restrict__ rec, u64 n,
                                                const u64 *__restrict__ before, u64 *__restrict__ line, u64 *__restrict__ ctr)
{
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    u64 m = 0;
    if (i < n)
    {
        const uint4 r = *reinterpret_cast<const uint4 *>(rec + 2 * i);
        const u64 s = ((u64)r.y << 32) | r.x, e = ((u64)r.w << 32) | r.z;
        u64 ln = 0;
        if (s < w.base || s - w.base >= w.buf_len || e < s || min(e, w.global_len) - w.base > w.buf_len ||
            (i > 0 && rec[2 * (i - 1)] > s))
            ctr[0] = 1; // (every writer stores the same value)
        else
        {
            const u64 o = s - w.base, b = o / kLineBlock, lo = b * kLineBlock, lim = min(lo + kLineBlock, w.buf_len);
            ln = w.nl_before + (o - lo <= lim - o ? 1 + before[b] + nl_count(text, lo, o) : 1 + before[b + 1] - nl_count(text, o, lim));
            m = s < w.last_nl1 ? ln : 0ull;
        }
        line[i] = ln;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1)
        m = max(m, (u64)__shfl_xor(m, o));
    if ((threadIdx.x & 63u) == 0 && m)
        (void)__hip_atomic_fetch_max(ctr + 1, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// (3w) om_sizes with the stale decision by OFFSET: a record that starts behind the whole text's last newline prints the stale value
__global__ __launch_bounds__(256) void mw_sizes(const u64 *__restrict__ rec, u64 n, const MwWindow w, u64 max_items, u64 fixed,
                                                const u64 *__restrict__ ctr, u64 *__restrict__ line, u64 *__restrict__ bytes)
{
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n)
        return;
    if (i == n || i >= max_items)
    {
        bytes[i] = 0;
        return;
    }
    const u64 s = rec[2 * i], e = min(rec[2 * i + 1], w.global_len);
    u64 ln = line[i];
    if (w.stale_rule && w.last_nl1 && s >= w.last_nl1)
    {
        const u64 mine = ctr[1];
        ln = mine ? mine : max(w.stale_in, 1ull);
        line[i] = ln;
    }
    bytes[i] = fixed + om_digits(ln) + 1 + (e - s) + 1;
}

// (5w) one wave: ctr[2] = nl_before + the newlines of the buffer in front of buffer offset `upto` (<= buf_len): a table entry and a
// partial block; ctr[3] = the newlines of the whole buffer
__global__ __launch_bounds__(64) void mw_count_to(const uint8_t *__restrict__ text, const MwWindow w, u64 upto, const u64 *__restrict__ before,
                                                  u64 nblocks, u64 *__restrict__ ctr)
{
    const u64 b = upto / kLineBlock, lo = b * kLineBlock + (u64)threadIdx.x * (kLineBlock / 64);
    u64 c = lo < upto ? (u64)nl_count(text, lo, min(lo + kLineBlock / 64, upto)) : 0ull;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1)
        c += (u64)__shfl_xor(c, o);
    if (threadIdx.x == 0)
    {
        ctr[2] = w.nl_before + before[b] + c;
        ctr[3] = before[nblocks - 1];
    }
}

// step (2) for a caller in another file (kg_batch_format.hip: the line numbers of a pack, before they are made relative per item)
void om_lines_on(const uint8_t *d_text, u64 text_len, const u64 *d_rec, u64 n, const u64 *before, u64 nblocks, u64 *line, u64 *ctr,
                 hipStream_t st)
{
    hipLaunchKernelGGL(om_lines, dim3((u32)((n + 255) / 256)), dim3(256), 0, st, d_text, text_len, d_rec, n, before, nblocks, line, ctr);
}

} // namespace kg

using namespace kg;

// the four strings of a format (NULL: all empty)
static FormatStrings om_strings(const krep_gpu_match_format_t *fmt)
{
    const krep_gpu_match_format_t none{};
    const krep_gpu_match_format_t &m = fmt ? *fmt : none;
    return {{m.prefix, m.prefix_len}, {m.before_number, m.before_number_len}, {m.after_number, m.after_number_len},
            {m.after_match, m.after_match_len}};
}

// the scratch of both calls (g_fmt_mu held)
struct OmWork
{
    u64 *ctr, *counts, *before, *line, *bytes, *off, *sum_words; // ctr: {refused, stale value, (window) the two newline counts}
    uint8_t *d_fix;
    u64 nblocks;
};
static int om_layout(u64 text_len, u64 n, size_t fixed, OmWork &w)
{
    const u64 nblocks = line_blocks(text_len), n1 = n + 1;
    const u64 sums = scan_sums_words(std::max(nblocks, n1));
    FmtCursor c;
    if (c.reserve(8 + 2 * nblocks + 3 * n1 + sums, fixed))
        return 2;
    w.nblocks = nblocks;
    w.ctr = c.take(8), w.counts = c.take(nblocks), w.before = c.take(nblocks);
    w.line = c.take(n1), w.bytes = c.take(n1), w.off = c.take(n1), w.sum_words = c.take(sums);
    w.d_fix = c.tail();
    return 0;
}

extern "C" int krep_gpu_format_matches(const void *d_text, size_t text_len, const match_position_t *d_positions, uint64_t n,
                                       uint64_t max_items, const krep_gpu_match_format_t *fmt, void *d_out, size_t out_capacity,
                                       krep_gpu_matches_out_t *out, void *stream)
{
    const char *who = "krep_gpu_format_matches";
    if (!out)
        return fail("%s: out is NULL", who);
    *out = krep_gpu_matches_out_t{};
    const FormatStrings fs = om_strings(fmt);
    if (fmt_enter(who, nullptr, n && (!d_text || !d_positions), "d_text / d_positions", n) || fs.refuse(who))
        return 2;
    if (!n)
        return 0;
    if (!text_len)
        return fail("%s: records on an empty text", who);
    if (text_len >= kOmMaxText)
        return fail("%s: text too long", who);
    hipStream_t st = (hipStream_t)stream;
    std::lock_guard<std::mutex> lk(g_fmt_mu);
    const OmFixed f{(u32)(fs.len(0) + fs.len(1)), (u32)fs.len(2), (u32)fs.len(3)};
    const u64 fixed = fs.bytes(), n1 = n + 1;
    OmWork w;
    if (om_layout(text_len, n, fixed, w))
        return 2;
    HIPCHK(hipMemsetAsync(w.ctr, 0, 8 * sizeof(u64), st));
    if (fs.upload(w.d_fix, st))
        return 2;
    if (newlines_before_blocks((const uint8_t *)d_text, text_len, w.counts, w.before, w.sum_words, st))
        return 2;
    hipLaunchKernelGGL(om_lines, dim3((u32)((n + 255) / 256)), dim3(256), 0, st, (const uint8_t *)d_text, (u64)text_len,
                       (const u64 *)d_positions, (u64)n, (const u64 *)w.before, w.nblocks, w.line, w.ctr);
    hipLaunchKernelGGL(om_sizes, dim3((u32)((n1 + 255) / 256)), dim3(256), 0, st, (const u64 *)d_positions, (u64)n, (u64)text_len,
                       (const u64 *)(w.before + w.nblocks - 1), (u64)max_items, fixed, (const u64 *)w.ctr, w.line, w.bytes);
    scan_exclusive(w.bytes, n1, w.off, w.sum_words, false, st);
    HIPCHK(hipGetLastError());
    u64 refused = 0, total = 0;
    HIPCHK(hipMemcpyAsync(&refused, w.ctr, sizeof(u64), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&total, w.off + n, sizeof(u64), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (refused)
        return fail("%s: the record list is not ascending in start, or a record lies outside the text", who);
    const u64 emit = std::min<u64>(n, max_items);
    out->items = emit;
    out->out_bytes = total;
    return fmt_gather(total, d_out, out_capacity, nullptr, &out->overflow, st, [&](uint8_t *o, u32 misalign, u64 nchunks, u32 grid) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(om_gather<false>), dim3(grid), dim3(256), 0, st, (const uint8_t *)d_text, (u64)text_len,
                           (const u64 *)d_positions, (const u64 *)w.line, (const u64 *)w.off, emit, (const uint8_t *)w.d_fix, f, o, total,
                           misalign, nchunks, (u64)0);
    });
}

extern "C" int krep_gpu_format_matches_window(const void *d_text, size_t text_len, const krep_gpu_matches_window_t *win,
                                              const match_position_t *d_positions, uint64_t n, uint64_t max_items,
                                              const krep_gpu_match_format_t *fmt, void *d_out, size_t out_capacity,
                                              krep_gpu_matches_window_out_t *out, void *stream)
{
    const char *who = "krep_gpu_format_matches_window";
    if (!out)
        return fail("%s: out is NULL", who);
    *out = krep_gpu_matches_window_out_t{};
    const FormatStrings fs = om_strings(fmt);
    // (this call also runs without records, on the text alone: its pointer test is its own, and `win` is looked at in front of it)
    if (fmt_enter(who, win ? nullptr : "win is NULL", (text_len && !d_text) || (n && !d_positions), "d_text / d_positions", n) ||
        fs.refuse(who))
        return 2;
    const u64 gb = win->global_base, glen = win->global_len;
    if (glen >= kOmMaxText)
        return fail("%s: text too long", who);
    if (gb > glen || text_len > glen - gb)
        return fail("%s: the buffer [%llu, + %zu) is not inside the text of %llu bytes", who, (unsigned long long)gb, text_len,
                    (unsigned long long)glen);
    if (win->count_to < gb || win->count_to - gb > text_len)
        return fail("%s: count_to = %llu lies outside the buffer", who, (unsigned long long)win->count_to);
    if (win->last_newline1 > glen)
        return fail("%s: last_newline1 = %llu lies behind the text", who, (unsigned long long)win->last_newline1);
    if (win->newlines_before >= kOmMaxText || win->stale_line >= kOmMaxText)
        return fail("%s: a line number of more than 16 digits", who);
    if (n && !text_len)
        return fail("%s: records on an empty buffer", who);
    out->stale_line = win->stale_line;
    out->newlines_before_count_to = win->newlines_before;
    if (!text_len)
        return 0;
    hipStream_t st = (hipStream_t)stream;
    std::lock_guard<std::mutex> lk(g_fmt_mu);
    const OmFixed f{(u32)(fs.len(0) + fs.len(1)), (u32)fs.len(2), (u32)fs.len(3)};
    const MwWindow mw{gb, (u64)text_len, glen, win->newlines_before, win->last_newline1, win->stale_line, win->stale_rule ? 1u : 0u};
    const u64 fixed = fs.bytes(), n1 = n + 1;
    OmWork w; // ctr: {refused, stale value, newlines in front of count_to, newlines of the buffer}
    if (om_layout(text_len, n, fixed, w))
        return 2;
    HIPCHK(hipMemsetAsync(w.ctr, 0, 8 * sizeof(u64), st));
    if (n && fs.upload(w.d_fix, st))
        return 2;
    if (newlines_before_blocks((const uint8_t *)d_text, text_len, w.counts, w.before, w.sum_words, st))
        return 2;
    hipLaunchKernelGGL(mw_count_to, dim3(1), dim3(64), 0, st, (const uint8_t *)d_text, mw, (u64)(win->count_to - gb), (const u64 *)w.before,
                       w.nblocks, w.ctr);
    if (n)
    {
        hipLaunchKernelGGL(mw_lines, dim3((u32)((n + 255) / 256)), dim3(256), 0, st, (const uint8_t *)d_text, mw, (const u64 *)d_positions,
                           (u64)n, (const u64 *)w.before, w.line, w.ctr);
        hipLaunchKernelGGL(mw_sizes, dim3((u32)((n1 + 255) / 256)), dim3(256), 0, st, (const u64 *)d_positions, (u64)n, mw, (u64)max_items,
                           fixed, (const u64 *)w.ctr, w.line, w.bytes);
        scan_exclusive(w.bytes, n1, w.off, w.sum_words, false, st);
    }
    HIPCHK(hipGetLastError());
    u64 h_ctr[4] = {0, 0, 0, 0}, total = 0;
    HIPCHK(hipMemcpyAsync(h_ctr, w.ctr, sizeof(h_ctr), hipMemcpyDeviceToHost, st));
    if (n)
        HIPCHK(hipMemcpyAsync(&total, w.off + n, sizeof(u64), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (h_ctr[0] || win->newlines_before + h_ctr[3] + 1 >= kOmMaxText)
        *out = krep_gpu_matches_window_out_t{};
    if (h_ctr[0])
        return fail("%s: the record list is not ascending in start, or a record lies outside the buffer or outruns it", who);
    if (win->newlines_before + h_ctr[3] + 1 >= kOmMaxText)
        return fail("%s: a line number of more than 16 digits", who);
    if (h_ctr[1])
        out->stale_line = h_ctr[1];
    out->newlines_before_count_to = h_ctr[2];
    const u64 emit = std::min<u64>(n, max_items);
    out->matches.items = emit;
    out->matches.out_bytes = total;
    return fmt_gather(total, d_out, out_capacity, nullptr, &out->matches.overflow, st, [&](uint8_t *o, u32 misalign, u64 nchunks, u32 grid) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(om_gather<true>), dim3(grid), dim3(256), 0, st, (const uint8_t *)d_text, glen,
                           (const u64 *)d_positions, (const u64 *)w.line, (const u64 *)w.off, emit, (const uint8_t *)w.d_fix, f, o, total,
                           misalign, nchunks, gb);
    });
}
