// kg_batch_format.hip — the two grep outputs over a PACK of items while it lies in HBM (krep_gpu_format_lines_items,
// krep_gpu_format_matches_items; include/krep_gpu.h "the grep output of a batch").
//
// A pack is the items of a batch with one '\n' between neighbours.  The searches a batch takes are newline-separable, so
//   * every line of the pack lies inside one item, and the separator is a real newline that ends an item's last line: the line
//     analysis of kg_lines.hip on the WHOLE pack (block newline table, per-record bounds, heads and sums: ln_analyse) finds exactly
//     the lines, cursors, clamps and 2048-caps the items have alone;
//   * a record's LINE inside its item is its line in the pack minus the newlines in front of the item's first byte.
// What is per item is looked up: the prefix (at line heads in the lines form, at every record under -o), the line-number base and
// the reference's stale number, which it applies once per FILE (print_matching_items() runs per file).  Steps:
//   (0) the refusal: bf_check_tables (one thread per table entry) and bf_check_records (one thread per record: its item by binary
//       search over the offset table, in LDS when it fits; under -o the item index is kept) read the tables and the list only;
//       the host waits for their verdict before any kernel reads the pack through the list;
//   lines  (1)-(3) ln_analyse on the pack; (4) bf_lc_sizes = lc_sizes with the prefix length of the head's item; sums;
//          (5) bf_gather<BfLines>: the LcItem piece layout, piece 0 read through the item's prefix offset;
//   -o     (1) newlines_before_blocks, (2) om_lines on the pack; (2i) bf_om_items, one thread per item: the newlines in front of the
//          item and inside it (two table entries and two partial blocks: bounded work whatever the item's size), its record range
//          (two lower bounds) and its stale value (one more binary search inside that range: line numbers ascend with start);
//          (3) bf_om_sizes: LINE made relative, the stale rule per item, the byte count; sums; (4) bf_gather<BfMatches>: the OmItem
//          piece layout behind the item's prefix.
//   item output offsets: the summed per-record sizes read at each item's first record (bf_item_offsets).
// "Behind the item's last newline" is decided as kg_matches.hip decides it for a text: the record's true LINE is the item's newline
// count + 1.  No kernel loops per item over its records or per record over a line.
//
// Host side of both calls (the shared pieces are kg_format_host.h's): out, bf_enter = fmt_enter with the pack view in front of the
// pointers, the pack's own rule about fmt->prefix, FormatStrings::refuse on the three other strings, n == 0; under g_fmt_mu
// bf_refuse = (0), the scratch (ln_analyse's for the lines form, with the item words and the strings behind it; a FmtCursor for
// -o), the strings' upload, the kernels, the read-back (ln_read_back for the lines form) and fmt_gather with bf_gather<P> as its
// launch, which also asks `grow` for the buffer.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <mutex>

#include "../../include/krep_gpu.h"
#include "kg_device.h"
#include "kg_format_dev.h"
#include "kg_format_host.h"
#include "kg_internal.h"

namespace kg {
namespace {
constexpr u32 kBfLdsItems = 4096;  // offset-table entries (items + 1) kept in LDS: 32 KiB
constexpr u32 kBfPerBlock = 2048;  // records one workgroup walks: the table load is paid once per 2048 records
constexpr u64 kBfMaxString = 1ull << 20;

std::atomic<uint64_t> g_bf_lds{0}, g_bf_global{0}; // krep_gpu_debug_batch_format_launches

// the item a pack offset lies in: the last i in [0, n_items) with tab[i] <= pos (tab[0] = 0)
__device__ __forceinline__ u64 bf_item_of(const u64 *tab, u64 n_items, u64 pos)
{
    u64 lo = 0, hi = n_items;
    while (hi - lo > 1)
    {
        const u64 mid = lo + (hi - lo) / 2;
        if (tab[mid] <= pos)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

// the offset table for a workgroup: staged in LDS when it fits (all threads of the workgroup call this)
template <bool LDS> __device__ __forceinline__ const u64 *bf_table(u64 *s_off, const u64 *__restrict__ off, u64 n_items)
{
    if (LDS)
    {
        for (u32 t = threadIdx.x; t <= (u32)n_items; t += blockDim.x)
            s_off[t] = off[t];
        __syncthreads();
        return s_off;
    }
    return off;
}

// (0) entry i of both tables, i in [0, n_items]; ctr[0] is raised by a table that may not be used
__global__ __launch_bounds__(256) void bf_check_tables(const u64 *__restrict__ off, u64 n_items, u64 packed_len, const u64 *__restrict__ poff,
                                                       u64 *__restrict__ ctr)
{
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n_items)
        return;
    bool bad = false;
    if (i == 0)
        bad = off[0] != 0;
    if (i == n_items)
        bad = bad || off[i] != packed_len + 1;
    else
    {
        const u64 p0 = poff[i], p1 = poff[i + 1];
        bad = bad || off[i + 1] <= off[i] || p1 < p0 || p1 - p0 > kBfMaxString;
    }
    if (bad)
        ctr[0] = 1; // (every writer stores the same value)
}

// (0) record k: ascending in start, end >= start, the start inside an item, the end not behind that item's end.  item != NULL: the
// index of its item is kept.  Reads the list and the table only
template <bool LDS>
__global__ __launch_bounds__(256) void bf_check_records(const u64 *__restrict__ rec, u64 n, const u64 *__restrict__ off, u64 n_items,
                                                        u64 packed_len, u64 *__restrict__ item, u64 *__restrict__ ctr)
{
    __shared__ u64 s_off[LDS ? kBfLdsItems : 1];
    const u64 *tab = bf_table<LDS>(s_off, off, n_items);
    const u64 k0 = (u64)blockIdx.x * kBfPerBlock, k1 = min(k0 + kBfPerBlock, n);
    for (u64 k = k0 + threadIdx.x; k < k1; k += blockDim.x)
    {
        const uint4 r = *reinterpret_cast<const uint4 *>(rec + 2 * k);
        const u64 s = ((u64)r.y << 32) | r.x, e = ((u64)r.w << 32) | r.z;
        u64 it = 0;
        bool bad = s >= packed_len || e < s || (k > 0 && rec[2 * (k - 1)] > s);
        if (!bad)
        {
            it = bf_item_of(tab, n_items, s);
            const u64 item_end = tab[it + 1] - 1; // the separator behind the item, or packed_len
            bad = s >= item_end || e > item_end;
        }
        if (bad)
            ctr[1] = 1; // (every writer stores the same value)
        if (item)
            item[k] = it;
    }
}

// ---- the lines form ------------------------------------------------------------------------------------------------------------
// (4) lc_sizes with a per-item prefix: the record that opens a line looks its item up, keeps the index and adds that item's prefix
// length.  f.prefix is 0: the strings in `fix` are before_match | after_match | line_close
template <bool LDS>
__global__ __launch_bounds__(256) void bf_lc_sizes(const u64 *__restrict__ rec, const u64 *__restrict__ ls, const u64 *__restrict__ le,
                                                   const u64 *__restrict__ heads_before, const u64 *__restrict__ mark_before, u64 n,
                                                   const LcFixed f, const u64 *__restrict__ off, u64 n_items, const u64 *__restrict__ poff,
                                                   u64 *__restrict__ bytes, u64 *__restrict__ range, u64 *__restrict__ item,
                                                   u64 *__restrict__ ctr)
{
    __shared__ u64 s_off[LDS ? kBfLdsItems : 1];
    const u64 *tab = bf_table<LDS>(s_off, off, n_items);
    const u64 k0 = (u64)blockIdx.x * kBfPerBlock, k1 = min(k0 + kBfPerBlock, n + 1);
    for (u64 i = k0 + threadIdx.x; i < k1; i += blockDim.x)
    {
        if (i == n)
        {
            bytes[n] = 0; // (so that the summed entry n is the total)
            continue;
        }
        const LnExtent x = ln_extent(rec, ls, le, heads_before, mark_before, n, ~0ull, i, ctr);
        if (!x.counted)
        {
            bytes[i] = 0;
            range[i] = 0;
            continue;
        }
        u64 plen = 0;
        if (x.first)
        {
            const u64 it = bf_item_of(tab, n_items, rec[2 * i]);
            item[i] = it;
            plen = poff[it + 1] - poff[it];
        }
        bytes[i] = plen + (x.end - x.src) + (x.solid ? (u64)f.before + f.after : 0ull) + (x.last ? (u64)f.close + 1ull : 0ull);
        range[i] = x.src | (x.first ? kLnFirst : 0ull) | (x.last ? kLnLast : 0ull) | (x.solid ? kLcSolid : 0ull);
    }
}

// what the gather needs to know about a record of the lines form: the LcItem layout, piece 0 with a source and a length of its own
struct BfLines
{
    const uint8_t *text;
    const u64 *rec, *le, *off, *range, *item;
    const uint8_t *fix; // before_match | after_match | line_close
    LcFixed f;          // (prefix = 0)
    const uint8_t *pfx;
    const u64 *poff;
    struct Rec
    {
        LcItem it;
        const uint8_t *pre;
    };
    __device__ __forceinline__ Rec load(u64 r) const
    {
        Rec x;
        x.it = lc_item(rec, le, off, range, f, r);
        x.pre = pfx;
        if (range[r] & kLnFirst)
        {
            const u64 i = item[r], p0 = poff[i];
            const u32 plen = (u32)(poff[i + 1] - p0);
            x.pre = pfx + p0;
            x.it.e0 = plen; // (e5, e6 and total come from the summed sizes, which hold the prefix already)
            x.it.e1 += plen;
            x.it.e2 += plen;
            x.it.e3 += plen;
            x.it.e4 += plen;
        }
        return x;
    }
    __device__ __forceinline__ u64 total(const Rec &x) const { return x.it.total; }
    __device__ __forceinline__ u32 byte(const Rec &x, u64 k) const { return k < x.it.e0 ? (u32)x.pre[k] : lc_byte(text, fix, f, x.it, k); }
    // 16 output bytes from k on that lie wholly inside one of the three text pieces
    __device__ __forceinline__ bool run16(const Rec &x, u64 k, uint4 &v) const
    {
        const LcItem &it = x.it;
        u64 skip = kLnNone; // the string bytes in front of the piece
        if (k >= it.e0 && k + 16 <= it.e1)
            skip = it.e0;
        else if (k >= it.e2 && k + 16 <= it.e3)
            skip = it.e2 - (it.e1 - it.e0);
        else if (k >= it.e4 && k + 16 <= it.e5)
            skip = it.e4 - (it.e1 - it.e0) - (it.e3 - it.e2);
        if (skip == kLnNone)
            return false;
        v = load_unaligned<uint4>(text + it.src + (k - skip));
        return true;
    }
};

// ---- the -o form ---------------------------------------------------------------------------------------------------------------
// the newlines in text[0, x) (x <= text_len): a table entry and a partial block
__device__ __forceinline__ u64 bf_newlines_before(const uint8_t *__restrict__ text, const u64 *__restrict__ before, u64 x)
{
    const u64 b = x / kLineBlock;
    return before[b] + nl_count(text, b * kLineBlock, x);
}

// (2i) item i: base[i] = the newlines of the pack in front of its first byte, inside[i] = those inside it, stale[i] = what a record
// behind its last newline prints (0: the item prints true numbers — at most 10 records, or no newline)
__global__ __launch_bounds__(256) void bf_om_items(const uint8_t *__restrict__ text, const u64 *__restrict__ before, const u64 *__restrict__ rec,
                                                   u64 n, const u64 *__restrict__ line, const u64 *__restrict__ off, u64 n_items,
                                                   u64 *__restrict__ base, u64 *__restrict__ inside, u64 *__restrict__ stale)
{
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_items)
        return;
    const u64 lo_off = off[i], hi_off = off[i + 1] - 1;
    const u64 nb = bf_newlines_before(text, before, lo_off), ni = bf_newlines_before(text, before, hi_off) - nb;
    u64 st = 0;
    const u64 lo = first_record_at(rec, n, lo_off), hi = first_record_at(rec, n, off[i + 1]);
    if (hi - lo > kOmStaleAfter && ni)
    {
        // the last record of the item whose LINE is at most ni, i.e. that starts at or before the item's last newline
        u64 a = lo, z = hi;
        while (a < z)
        {
            const u64 mid = a + (z - a) / 2;
            if (line[mid] - nb <= ni)
                a = mid + 1;
            else
                z = mid;
        }
        st = a > lo ? line[a - 1] - nb : 1ull;
    }
    base[i] = nb;
    inside[i] = ni;
    stale[i] = st;
}

// (3) the number record k prints (line[k], in place: relative to its item, the stale rule applied) and what it adds to the output
__global__ __launch_bounds__(256) void bf_om_sizes(const u64 *__restrict__ rec, u64 n, u64 text_len, const u64 *__restrict__ item,
                                                   const u64 *__restrict__ poff, const u64 *__restrict__ base, const u64 *__restrict__ inside,
                                                   const u64 *__restrict__ stale, u64 fixed, u64 *__restrict__ line, u64 *__restrict__ bytes)
{
    const u64 k = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (k > n)
        return;
    if (k == n)
    {
        bytes[n] = 0;
        return;
    }
    const u64 i = item[k];
    u64 ln = line[k] - base[i];
    const u64 st = stale[i];
    if (st && ln == inside[i] + 1)
        ln = st;
    line[k] = ln;
    const u64 s = rec[2 * k], e = min(rec[2 * k + 1], text_len);
    bytes[k] = (poff[i + 1] - poff[i]) + fixed + om_digits(ln) + 1 + (e - s) + 1;
}

// a record of the -o form: the item's prefix, then the OmItem layout with head = before_number
struct BfMatches
{
    const uint8_t *text;
    u64 text_len;
    const u64 *rec, *line, *item;
    const uint8_t *fix; // before_number | after_number | after_match
    OmFixed f;          // (head = before_number alone)
    const uint8_t *pfx;
    const u64 *poff;
    struct Rec
    {
        OmItem it;
        const uint8_t *pre;
        u32 plen;
    };
    __device__ __forceinline__ Rec load(u64 r) const
    {
        Rec x;
        x.it = om_item(rec, line, text_len, f, r);
        const u64 i = item[r], p0 = poff[i];
        x.pre = pfx + p0;
        x.plen = (u32)(poff[i + 1] - p0);
        return x;
    }
    __device__ __forceinline__ u64 total(const Rec &x) const { return (u64)x.plen + x.it.b6 + 1; }
    __device__ __forceinline__ u32 byte(const Rec &x, u64 k) const
    {
        return k < x.plen ? (u32)x.pre[k] : om_byte(text, fix, f, x.it, k - x.plen);
    }
    // 16 output bytes from k on that lie wholly inside the match
    __device__ __forceinline__ bool run16(const Rec &x, u64 k, uint4 &v) const
    {
        if (k < (u64)x.plen + x.it.b4 || k + 16 > (u64)x.plen + x.it.b5)
            return false;
        const uint4 t = load_unaligned<uint4>(text + x.it.src + (k - x.plen - x.it.b4));
        v = make_uint4(om_blank(t.x), om_blank(t.y), om_blank(t.z), om_blank(t.w));
        return true;
    }
};

// ---- the gather of both forms, dealt by OUTPUT bytes as ln_gather / om_gather deal it: chunk c is the 16 aligned bytes at
// (out - misalign) + 16 c, i.e. output offsets [16 c - misalign, + 16); a lane owns a chunk, a wave 1 KiB; the first record of a tile
// comes from a binary search in the summed sizes `off`
template <class P>
__global__ __launch_bounds__(256) void bf_gather(const P p, const u64 *__restrict__ off, u64 n, uint8_t *__restrict__ out, u64 total,
                                                 u32 misalign, u64 nchunks)
{
    const u32 lane = threadIdx.x & 63u;
    const u64 wid = (u64)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), nw = (u64)gridDim.x * (blockDim.x >> 6);
    for (u64 c0 = wid * 64; c0 < nchunks; c0 += nw * 64)
    {
        const u64 tile_lo = c0 ? c0 * 16 - misalign : 0ull, tile_hi = min((c0 + 64) * 16 - misalign, total) - 1;
        const u64 r_lo = ln_find(off, 0, n - 1, tile_lo), r_hi = ln_find(off, r_lo, n - 1, tile_hi);
        const u64 c = c0 + lane;
        if (c >= nchunks)
            continue;
        const u64 o0 = c ? c * 16 - misalign : 0ull, o1 = min((c + 1) * 16 - misalign, total);
        const bool whole = o1 - o0 == 16;
        u64 r = ln_find(off, r_lo, r_hi, o0);
        typename P::Rec x = p.load(r);
        u64 k = o0 - off[r];
        if (whole)
        {
            uint4 v;
            if (p.run16(x, k, v))
            {
                *reinterpret_cast<uint4 *>(out + o0) = v;
                continue;
            }
        }
        u32 w[4] = {0, 0, 0, 0};
        const u32 shift = (u32)(o0 + misalign - c * 16); // bytes of the chunk in front of the output (chunk 0 only)
        const u32 cnt = (u32)(o1 - o0);
#pragma unroll
        for (u32 q = 0; q < 16; ++q)
        {
            if (q >= shift && q - shift < cnt)
            {
                if (k >= p.total(x)) // the record is used up: the next one that adds bytes
                {
                    ++r;
                    if (off[r + 1] == off[r])
                        r = ln_find(off, r, n - 1, o0 + (q - shift));
                    x = p.load(r);
                    k = 0;
                }
                w[q >> 2] |= p.byte(x, k) << (8 * (q & 3u));
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

// item i's bytes begin where its first record's do (an item without records: where the next record's do); entry n_items: the total
__global__ __launch_bounds__(256) void bf_item_offsets(const u64 *__restrict__ rec, u64 n, const u64 *__restrict__ off, u64 n_items,
                                                       const u64 *__restrict__ out_off, u64 *__restrict__ item_out)
{
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n_items)
        return;
    item_out[i] = out_off[i == n_items ? n : first_record_at(rec, n, off[i])];
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
// what both calls check before they touch the device; *done: nothing is left to do (n == 0: the sizes stay 0, the item offsets are 0)
int bf_enter(const char *who, const void *d_pack, const krep_gpu_pack_view_t *v, const match_position_t *d_positions, uint64_t n,
             const size_t prefix_len, const FormatStrings &fs, uint64_t *d_item_out_off, hipStream_t st, bool *done)
{
    *done = false;
    const char *view = !v                                                            ? "the pack view is NULL"
                       : (v->n_items && (!v->d_item_off || !v->d_prefix_off)) ? "d_item_off / d_prefix_off is NULL"
                                                                              : nullptr; // (looked at in front of the pointers)
    if (fmt_enter(who, view, n && (!d_pack || !d_positions), "d_pack / d_positions", n))
        return 2;
    if (prefix_len)
        return fail("%s: fmt->prefix must be empty: the prefixes of a pack are per item (krep_gpu_pack_view_t)", who);
    if (fs.refuse(who))
        return 2;
    if (n && !v->n_items)
        return fail("%s: records on a pack without items", who);
    if (!n)
    {
        if (d_item_out_off)
        {
            HIPCHK(hipMemsetAsync(d_item_out_off, 0, (v->n_items + 1) * sizeof(uint64_t), st));
            HIPCHK(hipStreamSynchronize(st));
        }
        *done = true;
    }
    return 0;
}

// step (0) on `st`, waited for: 2 when a table or the list is refused.  ctr: 2 device words; item: n device words, or NULL
int bf_refuse(const char *who, const krep_gpu_pack_view_t &v, u64 packed_len, const u64 *rec, u64 n, u64 *ctr, u64 *item, hipStream_t st)
{
    const bool lds = v.n_items + 1 <= kBfLdsItems;
    HIPCHK(hipMemsetAsync(ctr, 0, 2 * sizeof(u64), st));
    hipLaunchKernelGGL(bf_check_tables, dim3((u32)((v.n_items + 1 + 255) / 256)), dim3(256), 0, st, (const u64 *)v.d_item_off, (u64)v.n_items,
                       packed_len, (const u64 *)v.d_prefix_off, ctr);
    const u32 grid = (u32)((n + kBfPerBlock - 1) / kBfPerBlock);
    if (lds)
        hipLaunchKernelGGL(bf_check_records<true>, dim3(grid), dim3(256), 0, st, rec, n, (const u64 *)v.d_item_off, (u64)v.n_items, packed_len,
                           item, ctr);
    else
        hipLaunchKernelGGL(bf_check_records<false>, dim3(grid), dim3(256), 0, st, rec, n, (const u64 *)v.d_item_off, (u64)v.n_items, packed_len,
                           item, ctr);
    HIPCHK(hipGetLastError());
    u64 h[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(h, ctr, sizeof h, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (h[0])
        return fail("%s: the offset table is not ascending from 0 to packed_len + 1, or the prefix table is not ascending or holds a "
                    "prefix of more than 2^20 bytes", who);
    if (h[1])
        return fail("%s: the record list is not ascending in start, or a record does not lie inside one item", who);
    (lds ? g_bf_lds : g_bf_global).fetch_add(1, std::memory_order_relaxed);
    return 0;
}

} // namespace

int format_lines_items(const void *d_pack, size_t packed_len, const krep_gpu_pack_view_t *v, const match_position_t *d_positions, uint64_t n,
                       const krep_gpu_line_format_t *fmt, void *d_out, size_t out_capacity, const FormatOutGrow *grow,
                       uint64_t *d_item_out_off, krep_gpu_lines_out_t *out, hipStream_t st)
{
    const char *who = "krep_gpu_format_lines_items";
    if (!out)
        return fail("%s: out is NULL", who);
    *out = krep_gpu_lines_out_t{};
    const krep_gpu_line_format_t none{};
    const krep_gpu_line_format_t &m = fmt ? *fmt : none;
    const FormatStrings fs{{m.before_match, m.before_match_len}, {m.after_match, m.after_match_len}, {m.line_close, m.line_close_len}};
    bool done = false;
    if (bf_enter(who, d_pack, v, d_positions, n, m.prefix_len, fs, d_item_out_off, st, &done))
        return 2;
    if (done)
        return 0;
    std::lock_guard<std::mutex> lk(g_fmt_mu);
    const LcFixed f{0u, (u32)fs.len(0), (u32)fs.len(1), (u32)fs.len(2)};
    const u64 *rec = (const u64 *)d_positions;
    {
        void *base = nullptr;
        if (fmt_reserve(8 * sizeof(u64), &base) || bf_refuse(who, *v, packed_len, rec, n, (u64 *)base, nullptr, st))
            return 2;
    }
    // (1)-(3) on the whole pack; behind its words: item[n + 1], then the strings
    const u64 n1 = n + 1;
    LnWork w;
    if (ln_analyse((const uint8_t *)d_pack, packed_len, rec, n, n1 * sizeof(u64) + fs.bytes(), w, st))
        return 2;
    u64 *item = (u64 *)w.prefix;
    uint8_t *d_fix = (uint8_t *)(item + n1);
    if (fs.upload(d_fix, st))
        return 2;
    u64 *off = w.ls; // the line starts are not read again behind the size pass: their buffer takes the summed byte counts
    const u32 grid_s = (u32)((n1 + kBfPerBlock - 1) / kBfPerBlock);
    if (v->n_items + 1 <= kBfLdsItems)
        hipLaunchKernelGGL(bf_lc_sizes<true>, dim3(grid_s), dim3(256), 0, st, rec, (const u64 *)w.ls, (const u64 *)w.le,
                           (const u64 *)w.heads_before, (const u64 *)w.mark_before, (u64)n, f, (const u64 *)v->d_item_off, (u64)v->n_items,
                           (const u64 *)v->d_prefix_off, w.a, w.range, item, w.ctr);
    else
        hipLaunchKernelGGL(bf_lc_sizes<false>, dim3(grid_s), dim3(256), 0, st, rec, (const u64 *)w.ls, (const u64 *)w.le,
                           (const u64 *)w.heads_before, (const u64 *)w.mark_before, (u64)n, f, (const u64 *)v->d_item_off, (u64)v->n_items,
                           (const u64 *)v->d_prefix_off, w.a, w.range, item, w.ctr);
    scan_exclusive(w.a, n1, off, w.sums, false, st);
    if (d_item_out_off)
        hipLaunchKernelGGL(bf_item_offsets, dim3((u32)((v->n_items + 1 + 255) / 256)), dim3(256), 0, st, rec, (u64)n,
                           (const u64 *)v->d_item_off, (u64)v->n_items, (const u64 *)off, (u64 *)d_item_out_off);
    HIPCHK(hipGetLastError());
    u64 h[2] = {0, 0};
    if (ln_read_back(who, "pack", w, off, n, ~0ull, h, 2, out, st)) // (no limit: every line of the pack is emitted)
        return 2;
    const u64 bytes = out->out_bytes;
    const BfLines p{(const uint8_t *)d_pack, rec, w.le, off, w.range, item, d_fix, f, (const uint8_t *)v->d_prefix_bytes,
                    (const u64 *)v->d_prefix_off};
    return fmt_gather(bytes, d_out, out_capacity, grow, &out->overflow, st, [&](uint8_t *o, u32 misalign, u64 nchunks, u32 grid) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(bf_gather<BfLines>), dim3(grid), dim3(256), 0, st, p, (const u64 *)off, (u64)n, o, bytes, misalign,
                           nchunks);
    });
}

int format_matches_items(const void *d_pack, size_t packed_len, const krep_gpu_pack_view_t *v, const match_position_t *d_positions,
                         uint64_t n, const krep_gpu_match_format_t *fmt, void *d_out, size_t out_capacity, const FormatOutGrow *grow,
                         uint64_t *d_item_out_off, krep_gpu_matches_out_t *out, hipStream_t st)
{
    const char *who = "krep_gpu_format_matches_items";
    if (!out)
        return fail("%s: out is NULL", who);
    *out = krep_gpu_matches_out_t{};
    const krep_gpu_match_format_t none{};
    const krep_gpu_match_format_t &m = fmt ? *fmt : none;
    const FormatStrings fs{{m.before_number, m.before_number_len}, {m.after_number, m.after_number_len}, {m.after_match, m.after_match_len}};
    bool done = false;
    if (bf_enter(who, d_pack, v, d_positions, n, m.prefix_len, fs, d_item_out_off, st, &done))
        return 2;
    if (done)
        return 0;
    if (packed_len >= kOmMaxText)
        return fail("%s: pack too long", who);
    std::lock_guard<std::mutex> lk(g_fmt_mu);
    const OmFixed f{(u32)fs.len(0), (u32)fs.len(1), (u32)fs.len(2)};
    const u64 *rec = (const u64 *)d_positions;
    const u64 fixed = fs.bytes(), nblocks = line_blocks(packed_len), n1 = n + 1, ni = v->n_items;
    const u64 sums = scan_sums_words(std::max(nblocks, n1));
    FmtCursor c;
    if (c.reserve(8 + 2 * nblocks + 4 * n1 + 3 * ni + sums, fixed))
        return 2;
    u64 *ctr = c.take(8), *counts = c.take(nblocks), *before = c.take(nblocks); // ctr: {refused, (om_lines' stale word, not used here)}
    u64 *line = c.take(n1), *bytes = c.take(n1), *off = c.take(n1), *item = c.take(n1);
    u64 *nl_base = c.take(ni), *nl_inside = c.take(ni), *stale = c.take(ni), *sum_words = c.take(sums);
    uint8_t *d_fix = c.tail();
    if (bf_refuse(who, *v, packed_len, rec, n, ctr, item, st))
        return 2;
    HIPCHK(hipMemsetAsync(ctr, 0, 8 * sizeof(u64), st));
    if (fs.upload(d_fix, st))
        return 2;
    if (newlines_before_blocks((const uint8_t *)d_pack, packed_len, counts, before, sum_words, st))
        return 2;
    om_lines_on((const uint8_t *)d_pack, packed_len, rec, n, before, nblocks, line, ctr, st);
    hipLaunchKernelGGL(bf_om_items, dim3((u32)((ni + 255) / 256)), dim3(256), 0, st, (const uint8_t *)d_pack, (const u64 *)before, rec, (u64)n,
                       (const u64 *)line, (const u64 *)v->d_item_off, ni, nl_base, nl_inside, stale);
    hipLaunchKernelGGL(bf_om_sizes, dim3((u32)((n1 + 255) / 256)), dim3(256), 0, st, rec, (u64)n, (u64)packed_len, (const u64 *)item,
                       (const u64 *)v->d_prefix_off, (const u64 *)nl_base, (const u64 *)nl_inside, (const u64 *)stale, fixed, line, bytes);
    scan_exclusive(bytes, n1, off, sum_words, false, st);
    if (d_item_out_off)
        hipLaunchKernelGGL(bf_item_offsets, dim3((u32)((ni + 1 + 255) / 256)), dim3(256), 0, st, rec, (u64)n, (const u64 *)v->d_item_off, ni,
                           (const u64 *)off, (u64 *)d_item_out_off);
    HIPCHK(hipGetLastError());
    u64 refused = 0, total = 0;
    HIPCHK(hipMemcpyAsync(&refused, ctr, sizeof(u64), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&total, off + n, sizeof(u64), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (refused)
        return fail("%s: the record list is not ascending in start, or a record lies outside the pack", who);
    out->items = n;
    out->out_bytes = total;
    const BfMatches p{(const uint8_t *)d_pack, (u64)packed_len, rec, line, item, d_fix, f, (const uint8_t *)v->d_prefix_bytes,
                      (const u64 *)v->d_prefix_off};
    return fmt_gather(total, d_out, out_capacity, grow, &out->overflow, st, [&](uint8_t *o, u32 misalign, u64 nchunks, u32 grid) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(bf_gather<BfMatches>), dim3(grid), dim3(256), 0, st, p, (const u64 *)off, (u64)n, o, total, misalign,
                           nchunks);
    });
}

} // namespace kg

extern "C" int krep_gpu_format_lines_items(const void *d_pack, size_t packed_len, const krep_gpu_pack_view_t *v,
                                           const match_position_t *d_positions, uint64_t n, const krep_gpu_line_format_t *fmt, void *d_out,
                                           size_t out_capacity, uint64_t *d_item_out_off, krep_gpu_lines_out_t *out, void *stream)
{
    return kg::format_lines_items(d_pack, packed_len, v, d_positions, n, fmt, d_out, out_capacity, nullptr, d_item_out_off, out,
                                  (hipStream_t)stream);
}

extern "C" int krep_gpu_format_matches_items(const void *d_pack, size_t packed_len, const krep_gpu_pack_view_t *v,
                                             const match_position_t *d_positions, uint64_t n, const krep_gpu_match_format_t *fmt,
                                             void *d_out, size_t out_capacity, uint64_t *d_item_out_off, krep_gpu_matches_out_t *out,
                                             void *stream)
{
    return kg::format_matches_items(d_pack, packed_len, v, d_positions, n, fmt, d_out, out_capacity, nullptr, d_item_out_off, out,
                                    (hipStream_t)stream);
}

extern "C" void krep_gpu_debug_batch_format_launches(uint64_t *lds_table, uint64_t *global_table)
{
    if (lds_table) *lds_table = kg::g_bf_lds.load();
    if (global_table) *global_table = kg::g_bf_global.load();
}
