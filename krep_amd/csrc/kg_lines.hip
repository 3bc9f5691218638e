// kg_lines.hip — the reference's DEFAULT output on a text that is resident in HBM: every line that holds the start of a match,
// once, as print_matching_items() writes it in full-line mode without colour (krep.c:797-1071).
//
// Contract (restated from krep.c:838-1061; the record list is in (start, end) order, as search_file() leaves it):
//   * a record belongs to the line of its START: line_start = one past the last '\n' in [0, start) (find_line_start,
//     krep.c:363-398), line_end = the first '\n' at or after it, else text_len (find_line_end, :401-415);
//   * every distinct line once, ascending, at most max_lines of them; only the first 2048 records of a line take part
//     (MAX_MATCHES_PER_LINE, :496, :893-913);
//   * a line's bytes follow a cursor that starts at line_start: per record the text between the cursor and the record's start (if
//     the start lies behind the cursor), then the match clamped to line_end, and the cursor moves to the clamped end — also
//     BACKWARDS, so overlapping records repeat bytes; a record whose clamped match is empty is passed over (:973-974); behind the
//     last record the text from the cursor to line_end, then '\n' (:963-1018).
// In front of a record's match lies either nothing new (its start is behind the cursor) or the text from the cursor on, and
// behind the last record's match the rest of the line: what a record adds is ONE range of the text, [min(start, cursor),
// clamped end or line_end), plus the prefix in front of the line's first record and the '\n' behind its last.  So the sizes are a
// prefix sum and the copy is a segmented gather.  (A record that starts ON a '\n' has an empty clamped match: it belongs to the line
// that newline ends and adds nothing of its own.  The reference CLI does not terminate on such a list without -m 1.)
//
// Steps: (1) one streaming pass over the text leaves per 4 KiB block its first and last newline; a running maximum / minimum over
// the blocks turns them into "last newline in front of this block" / "first newline behind it"; (2) per record both line bounds,
// searched in 16-byte steps inside the record's own block only, else taken from the table — no thread walks more than one block per
// direction, whatever the text; the same kernel refuses a list that is not ascending or points outside the text; (3) line heads,
// line index and first record of the line (one sum, one running maximum); (4) per record its range and byte count, summed;
// (5) the gather, dealt by OUTPUT bytes: a lane owns 16 aligned bytes of the output, a wave 1 KiB, the first record of a tile comes
// from a binary search in the summed offsets.  A call reads the text once in (1), then only around the records and what it copies.
// krep_gpu_format_lines_ex (--color=always: the caller's strings around the line and around every match) shares (1)-(3) and has a
// size pass and a gather of its own, (4') and (5') below.  krep_gpu_format_lines_window (the same lines for a WINDOW of a text: the
// buffer may begin and end inside a line, the call owns the lines that START in [own_lo, own_hi)) shares (1), the sums and (5') and
// has (2"), (3") and (4") of its own, further below.
//
// Host side, the same for the three formatting calls (the shared pieces are kg_format_host.h's): ln_check (out, fmt_enter), the
// format's strings (FormatStrings::refuse), the call's own checks; under g_fmt_mu the scratch from ln_layout, the strings' upload,
// ln_table = (1), ln_records = (2)-(3) with ln_bounds / ln_heads or the window's lw_bounds / lw_heads — ln_analyse is the layout
// and these steps for a whole text; then the call's size pass and sum, ln_read_back (one wait: the totals and the counter words,
// the refusal of a bad list, *out) and fmt_gather with the call's gather as its launch.  krep_gpu_matching_lines has no gather and
// reads other words back: it shares ln_check and ln_analyse only.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>

#include "../../include/krep_gpu.h"
#include "kg_device.h"
#include "kg_format_dev.h"
#include "kg_format_host.h"
#include "kg_internal.h"

namespace kg {

// (the constants, LnRecord / ln_record, LnExtent / ln_extent, ln_find, LcFixed, LcItem / lc_item / lc_byte and LnWork live in
// kg_format_dev.h: kg_batch_format.hip formats a pack of items with the same helpers)

// bit q set: byte q of the 16 is a '\n'
__device__ __forceinline__ u32 nl_mask16(const uint4 v)
{
    return movemask4(eq_bytes(v.x, 0x0a0a0a0au)) | (movemask4(eq_bytes(v.y, 0x0a0a0a0au)) << 4) |
           (movemask4(eq_bytes(v.z, 0x0a0a0a0au)) << 8) | (movemask4(eq_bytes(v.w, 0x0a0a0a0au)) << 12);
}

// (1) one wave per block.  last1[b]: one past the block's last newline (0: none); first_rev[nb - 1 - b]: the complement of its
// first newline's offset (0: none) — reversed and complemented, the running MAXIMUM in front of an entry is the first newline
// BEHIND the block
__global__ __launch_bounds__(256) void ln_block_table(const uint8_t *__restrict__ text, u64 text_len, u64 nb, u64 *__restrict__ last1,
                                                      u64 *__restrict__ first_rev)
{
    const u32 lane = threadIdx.x & 63u;
    const u64 wid = (u64)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), nw = (u64)gridDim.x * (blockDim.x >> 6);
    for (u64 b = wid; b < nb; b += nw)
    {
        const u64 base = b * kLnBlock;
        u32 lo = ~0u, hi = 0; // offset of the first newline in the block / one past the last
        for (u32 it = 0; it < kLnBlock / 1024; ++it)
        {
            const u32 rel = it * 1024 + lane * 16;
            const u64 off = base + rel;
            u32 m = 0;
            if (off + 16 <= text_len)
                m = nl_mask16(load_unaligned<uint4>(text + off));
            else
                for (u32 q = 0; q < 16; ++q)
                    if (off + q < text_len && text[off + q] == '\n')
                        m |= 1u << q;
            if (m)
            {
                lo = min(lo, rel + (u32)__ffs(m) - 1u);
                hi = rel + 32u - (u32)__clz(m);
            }
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1)
        {
            lo = min(lo, (u32)__shfl_xor(lo, o));
            hi = max(hi, (u32)__shfl_xor(hi, o));
        }
        if (lane == 0)
        {
            last1[b] = hi ? base + hi : 0ull;
            first_rev[nb - 1 - b] = lo != ~0u ? ~(base + lo) : 0ull;
        }
    }
}

// (2) line bounds of every record; a record that may not be read (outside the text, end before start, start before its
// predecessor's) raises the flag and touches no text
__global__ __launch_bounds__(256) void ln_bounds(const uint8_t *__restrict__ text, u64 text_len, const u64 *__restrict__ rec, u64 n,
                                                 const u64 *__restrict__ prev1, const u64 *__restrict__ next_rev, u64 nb,
                                                 u64 *__restrict__ ls, u64 *__restrict__ le, u64 *__restrict__ ctr)
{
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    const uint4 r = *reinterpret_cast<const uint4 *>(rec + 2 * i);
    const u64 s = ((u64)r.y << 32) | r.x, e = ((u64)r.w << 32) | r.z;
    if (s >= text_len || e < s || (i > 0 && rec[2 * (i - 1)] > s))
    {
        ctr[0] = 1; // (every writer stores the same value)
        ls[i] = 0;
        le[i] = 0;
        return;
    }
    const u64 b = s / kLnBlock, base = b * kLnBlock, lim = min(base + kLnBlock, text_len);
    u64 p = s, a = kLnNone;
    while (p >= base + 16)
    {
        const u32 m = nl_mask16(load_unaligned<uint4>(text + p - 16));
        if (m)
        {
            a = p - 16 + (32u - (u32)__clz(m));
            break;
        }
        p -= 16;
    }
    if (a == kLnNone)
    {
        for (; p > base; --p)
            if (text[p - 1] == '\n')
                break;
        a = p > base ? p : prev1[b]; // (a newline in the block's last byte before `base` is the table's)
    }
    u64 q = s, z = kLnNone;
    while (q + 16 <= lim)
    {
        const u32 m = nl_mask16(load_unaligned<uint4>(text + q));
        if (m)
        {
            z = q + (u32)__ffs(m) - 1u;
            break;
        }
        q += 16;
    }
    if (z == kLnNone)
    {
        for (; q < lim; ++q)
            if (text[q] == '\n')
                break;
        if (q < lim)
            z = q;
        else
        {
            const u64 nx = next_rev[nb - 1 - b];
            z = nx ? ~nx : text_len;
        }
    }
    ls[i] = a;
    le[i] = z;
}

// (3) head[i]: the record opens a line; mark[i]: its index + 1 there, else 0 (their running maximum is the line's first record)
__global__ __launch_bounds__(256) void ln_heads(const u64 *__restrict__ ls, u64 n, u64 *__restrict__ head, u64 *__restrict__ mark)
{
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n)
        return;
    const bool h = i < n && (i == 0 || ls[i] != ls[i - 1]);
    head[i] = h ? 1ull : 0ull; // (entry n: 0, so that the scanned entry n is the total)
    mark[i] = h ? i + 1 : 0ull;
}

// krep_gpu_matching_lines: the spans and first records of the first `emit` lines (write != 0), and the emitted lines that hold more
// than 2048 records
__global__ __launch_bounds__(256) void ln_spans(const u64 *__restrict__ ls, const u64 *__restrict__ le, const u64 *__restrict__ heads_before,
                                                const u64 *__restrict__ mark_before, u64 n, u64 emit, int write, u64 *__restrict__ lines,
                                                u64 *__restrict__ first_record, u64 *__restrict__ ctr)
{
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    const LnRecord r = ln_record(ls, heads_before, mark_before, i);
    if (r.line < emit && i - r.first == kLnCap)
        (void)__hip_atomic_fetch_add(ctr + 1, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (!write)
        return;
    if (r.head && r.line <= emit)
    {
        first_record[r.line] = i;
        if (r.line < emit)
        {
            lines[2 * r.line] = ls[i];
            lines[2 * r.line + 1] = le[i];
        }
    }
    if (i == n - 1 && heads_before[n] == emit)
        first_record[emit] = n;
}

// (4) what record i adds to the output: bytes[i], and range[i] = flags | offset of its range in the text
__global__ __launch_bounds__(256) void ln_sizes(const u64 *__restrict__ rec, const u64 *__restrict__ ls, const u64 *__restrict__ le,
                                                const u64 *__restrict__ heads_before, const u64 *__restrict__ mark_before, u64 n,
                                                u64 max_lines, u64 prefix_len, u64 *__restrict__ bytes, u64 *__restrict__ range,
                                                u64 *__restrict__ ctr)
{
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n)
        return;
    if (i == n)
    {
        bytes[n] = 0;
        return;
    }
    const LnExtent x = ln_extent(rec, ls, le, heads_before, mark_before, n, max_lines, i, ctr);
    if (!x.counted)
    {
        bytes[i] = 0;
        range[i] = 0;
        return;
    }
    bytes[i] = (x.first ? prefix_len : 0ull) + (x.end - x.src) + (x.last ? 1ull : 0ull);
    range[i] = x.src | (x.first ? kLnFirst : 0ull) | (x.last ? kLnLast : 0ull);
}

// where a lane stands in the output: inside record r, with `pre` bytes of the prefix, `txt` bytes of the text and `nl` newline to go
struct LnCursor
{
    u64 r, src, txt;
    u32 pre, ppos, nl;
};
__device__ __forceinline__ LnCursor ln_enter(const u64 *__restrict__ off, const u64 *__restrict__ range, u32 prefix_len, u64 r, u64 skip)
{
    LnCursor c;
    const u64 w = range[r], total = off[r + 1] - off[r];
    const u32 pl = (w & kLnFirst) ? prefix_len : 0u, nl = (w & kLnLast) ? 1u : 0u;
    const u64 tl = total - pl - nl;
    c.r = r;
    c.src = w & kLnSrc;
    c.ppos = 0;
    c.pre = pl;
    c.txt = tl;
    c.nl = nl;
    if (skip)
    {
        const u32 sp = (u32)min((u64)pl, skip);
        c.ppos = sp;
        c.pre = pl - sp;
        skip -= sp;
        const u64 st = min(tl, skip);
        c.src += st;
        c.txt = tl - st;
        skip -= st;
        if (skip)
            c.nl = 0;
    }
    return c;
}

// (5) chunk c is the 16 aligned bytes at (out - misalign) + 16 c, i.e. output offsets [16 c - misalign, + 16)
__global__ __launch_bounds__(256) void ln_gather(const uint8_t *__restrict__ text, const u64 *__restrict__ off, const u64 *__restrict__ range,
                                                 u64 n, const uint8_t *__restrict__ prefix, u32 prefix_len, uint8_t *__restrict__ out,
                                                 u64 total, u32 misalign, u64 nchunks)
{
    const u32 lane = threadIdx.x & 63u;
    const u64 wid = (u64)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), nw = (u64)gridDim.x * (blockDim.x >> 6);
    for (u64 c0 = wid * 64; c0 < nchunks; c0 += nw * 64)
    {
        // the records of the wave's 1 KiB tile
        const u64 tile_lo = c0 ? c0 * 16 - misalign : 0ull, tile_hi = min((c0 + 64) * 16 - misalign, total) - 1;
        const u64 r_lo = ln_find(off, 0, n - 1, tile_lo), r_hi = ln_find(off, r_lo, n - 1, tile_hi);
        const u64 c = c0 + lane;
        if (c >= nchunks)
            continue;
        const u64 o0 = c ? c * 16 - misalign : 0ull, o1 = min((c + 1) * 16 - misalign, total);
        const bool whole = o1 - o0 == 16;
        u64 r = ln_find(off, r_lo, r_hi, o0);
        LnCursor k = ln_enter(off, range, prefix_len, r, o0 - off[r]);
        if (whole && k.pre == 0 && k.txt >= 16)
        {
            *reinterpret_cast<uint4 *>(out + o0) = load_unaligned<uint4>(text + k.src);
            continue;
        }
        u32 w[4] = {0, 0, 0, 0};
        const u32 shift = (u32)(o0 + misalign - c * 16); // bytes of the chunk in front of the output (chunk 0 only)
        u64 pos = o0;
#pragma unroll
        for (u32 q = 0; q < 16; ++q)
        {
            if (q >= shift && pos < o1)
            {
                while (k.pre == 0 && k.txt == 0 && k.nl == 0) // the record is used up: the next one that adds bytes
                {
                    r = k.r + 1;
                    if (off[r + 1] == off[r])
                        r = ln_find(off, r, n - 1, pos);
                    k = ln_enter(off, range, prefix_len, r, 0);
                }
                u32 byte;
                if (k.pre)
                {
                    byte = prefix[k.ppos++];
                    --k.pre;
                }
                else if (k.txt)
                {
                    byte = text[k.src++];
                    --k.txt;
                }
                else
                {
                    byte = '\n';
                    k.nl = 0;
                }
                w[q >> 2] |= byte << (8 * (q & 3u));
                ++pos;
            }
        }
        if (whole)
            *reinterpret_cast<uint4 *>(out + o0) = make_uint4(w[0], w[1], w[2], w[3]);
        else
        {
#pragma unroll
            for (u32 q = 0; q < 16; ++q)
                if (q >= shift && o0 + (q - shift) < o1)
                    out[o0 + (q - shift)] = (uint8_t)(w[q >> 2] >> (8 * (q & 3u)));
        }
    }
}

// ---- the same lines with the caller's strings in them (krep_gpu_format_lines_ex) ---------------------------------------------
// A record's range of the text stays ONE range [src, end); before_match goes in at start - src and after_match at cend - src, the
// prefix in front of a line's first record, line_close and '\n' behind its last.  So a record is at most seven pieces besides the
// newline, and four of them are the strings, which lie behind one another in one small device buffer `fix`.

// (4') bytes[i] and range[i] = flags | offset of the record's range in the text
__global__ __launch_bounds__(256) void lc_sizes(const u64 *__restrict__ rec, const u64 *__restrict__ ls, const u64 *__restrict__ le,
                                                const u64 *__restrict__ heads_before, const u64 *__restrict__ mark_before, u64 n,
                                                u64 max_lines, const LcFixed f, u64 *__restrict__ bytes, u64 *__restrict__ range,
                                                u64 *__restrict__ ctr)
{
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n)
        return;
    if (i == n)
    {
        bytes[n] = 0;
        return;
    }
    const LnExtent x = ln_extent(rec, ls, le, heads_before, mark_before, n, max_lines, i, ctr);
    if (!x.counted)
    {
        bytes[i] = 0;
        range[i] = 0;
        return;
    }
    bytes[i] = (x.first ? (u64)f.prefix : 0ull) + (x.end - x.src) + (x.solid ? (u64)f.before + f.after : 0ull) +
               (x.last ? (u64)f.close + 1ull : 0ull);
    range[i] = x.src | (x.first ? kLnFirst : 0ull) | (x.last ? kLnLast : 0ull) | (x.solid ? kLcSolid : 0ull);
}

// (5') as ln_gather: chunk c is the 16 aligned bytes at (out - misalign) + 16 c, i.e. output offsets [16 c - misalign, + 16)
__global__ __launch_bounds__(256) void lc_gather(const uint8_t *__restrict__ text, const u64 *__restrict__ rec, const u64 *__restrict__ le,
                                                 const u64 *__restrict__ off, const u64 *__restrict__ range, u64 n,
                                                 const uint8_t *__restrict__ fix, const LcFixed f, uint8_t *__restrict__ out, u64 total,
                                                 u32 misalign, u64 nchunks)
{
    const u32 lane = threadIdx.x & 63u;
    const u64 wid = (u64)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), nw = (u64)gridDim.x * (blockDim.x >> 6);
    for (u64 c0 = wid * 64; c0 < nchunks; c0 += nw * 64)
    {
        // the records of the wave's 1 KiB tile
        const u64 tile_lo = c0 ? c0 * 16 - misalign : 0ull, tile_hi = min((c0 + 64) * 16 - misalign, total) - 1;
        const u64 r_lo = ln_find(off, 0, n - 1, tile_lo), r_hi = ln_find(off, r_lo, n - 1, tile_hi);
        const u64 c = c0 + lane;
        if (c >= nchunks)
            continue;
        const u64 o0 = c ? c * 16 - misalign : 0ull, o1 = min((c + 1) * 16 - misalign, total);
        const bool whole = o1 - o0 == 16;
        u64 r = ln_find(off, r_lo, r_hi, o0);
        LcItem it = lc_item(rec, le, off, range, f, r);
        u64 k = o0 - off[r];
        if (whole)
        {
            // wholly inside one of the three text pieces: `skip` string bytes lie in front of it
            u64 skip = kLnNone;
            if (k >= it.e0 && k + 16 <= it.e1)
                skip = it.e0;
            else if (k >= it.e2 && k + 16 <= it.e3)
                skip = it.e2 - (it.e1 - it.e0);
            else if (k >= it.e4 && k + 16 <= it.e5)
                skip = it.e4 - (it.e1 - it.e0) - (it.e3 - it.e2);
            if (skip != kLnNone)
            {
                *reinterpret_cast<uint4 *>(out + o0) = load_unaligned<uint4>(text + it.src + (k - skip));
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
                if (k >= it.total) // the record is used up: the next one that adds bytes
                {
                    ++r;
                    if (off[r + 1] == off[r])
                        r = ln_find(off, r, n - 1, o0 + (q - shift));
                    it = lc_item(rec, le, off, range, f, r);
                    k = 0;
                }
                w[q >> 2] |= lc_byte(text, fix, f, it, k) << (8 * (q & 3u));
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

// ---- the same lines for a window of a text (krep_gpu_format_lines_window) ------------------------------------------------------
// The buffer holds text[global_base, global_base + text_len) and may begin and end inside a line; the records carry GLOBAL offsets.
// A record is KEPT when its line is owned (line_start in [own_lo, own_hi), known from a newline inside the buffer or from
// global_base == 0) and complete (its newline lies in front of records_hi, or the buffer ends the text and the list with it).
// Everything behind (2") works on buffer-relative offsets: (2") leaves a relative copy of the list and ls = kLnNone for a record
// that is passed over, (3") opens lines at kept records only, (4") gives a passed-over record zero bytes — so the sums and
// lc_gather run as they are, on a list whose passed-over records add nothing, without compaction.
constexpr u32 kLwFirst = 2, kLwStart1 = 3; // counter block: [2] least index of a record on the owned line that is incomplete (kLnNone:
                                           // none), [3] that line's global line_start + 1

struct LwWindow
{
    u64 base, own_lo, own_hi, records_hi; // global_base; the other three RELATIVE to it
    u32 ends_text;                        // the buffer ends the text and the list is complete up to there
};

// (2") line bounds of every record inside the buffer, ownership and completeness; refuses as ln_bounds does
__global__ __launch_bounds__(256) void lw_bounds(const uint8_t *__restrict__ text, u64 text_len, const u64 *__restrict__ rec, u64 n,
                                                 const LwWindow w, const u64 *__restrict__ prev1, const u64 *__restrict__ next_rev, u64 nb,
                                                 u64 *__restrict__ loc, u64 *__restrict__ ls, u64 *__restrict__ le, u64 *__restrict__ ctr)
{
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    u64 open = kLnNone, open_start1 = 0; // i, if record i lies on the owned line that is incomplete
    if (i < n)
    {
        const uint4 r = *reinterpret_cast<const uint4 *>(rec + 2 * i);
        const u64 sg = ((u64)r.y << 32) | r.x, eg = ((u64)r.w << 32) | r.z;
        u64 a = kLnNone, z = 0, s = 0, e = 0;
        if (sg < w.base || sg - w.base >= text_len || eg < sg || (i > 0 && rec[2 * (i - 1)] > sg))
            ctr[0] = 1; // (every writer stores the same value)
        else
        {
            s = sg - w.base;
            e = eg - w.base;
            const u64 b = s / kLnBlock, base = b * kLnBlock, lim = min(base + kLnBlock, text_len);
            u64 p = s;
            while (p >= base + 16)
            {
                const u32 m = nl_mask16(load_unaligned<uint4>(text + p - 16));
                if (m)
                {
                    a = p - 16 + (32u - (u32)__clz(m));
                    break;
                }
                p -= 16;
            }
            if (a == kLnNone)
            {
                for (; p > base; --p)
                    if (text[p - 1] == '\n')
                        break;
                a = p > base ? p : prev1[b];
                if (a == 0 && w.base != 0)
                    a = kLnNone; // no newline in front of it inside the buffer: the line starts in front of the buffer
            }
            u64 q = s;
            z = kLnNone;
            while (q + 16 <= lim)
            {
                const u32 m = nl_mask16(load_unaligned<uint4>(text + q));
                if (m)
                {
                    z = q + (u32)__ffs(m) - 1u;
                    break;
                }
                q += 16;
            }
            if (z == kLnNone)
            {
                for (; q < lim; ++q)
                    if (text[q] == '\n')
                        break;
                if (q < lim)
                    z = q;
                else
                {
                    const u64 nx = next_rev[nb - 1 - b];
                    z = nx ? ~nx : text_len; // text_len: no newline up to the buffer's end
                }
            }
            if (a == kLnNone || a < w.own_lo || a >= w.own_hi)
                a = kLnNone; // a neighbour's line
            else if (z < text_len ? z >= w.records_hi : !w.ends_text)
            {
                open = i;
                open_start1 = w.base + a + 1;
                a = kLnNone;
            }
        }
        ls[i] = a;
        le[i] = z;
        *reinterpret_cast<uint4 *>(loc + 2 * i) = make_uint4((u32)s, (u32)(s >> 32), (u32)e, (u32)(e >> 32));
    }
    u64 m = open;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1)
        m = min(m, (u64)__shfl_xor((unsigned long long)m, o));
    if (m != kLnNone && open == m)
    {
        (void)__hip_atomic_fetch_min(ctr + kLwFirst, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        ctr[kLwStart1] = open_start1; // (at most one line is incomplete: every writer stores the same value)
    }
}

// (3") as ln_heads, but only a kept record opens a line
__global__ __launch_bounds__(256) void lw_heads(const u64 *__restrict__ ls, u64 n, u64 *__restrict__ head, u64 *__restrict__ mark)
{
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n)
        return;
    const bool h = i < n && ls[i] != kLnNone && (i == 0 || ls[i] != ls[i - 1]);
    head[i] = h ? 1ull : 0ull;
    mark[i] = h ? i + 1 : 0ull;
}

// (4") as lc_sizes on the relative list; a record that is passed over adds nothing
__global__ __launch_bounds__(256) void lw_sizes(const u64 *__restrict__ loc, const u64 *__restrict__ ls, const u64 *__restrict__ le,
                                                const u64 *__restrict__ heads_before, const u64 *__restrict__ mark_before, u64 n,
                                                u64 max_lines, const LcFixed f, u64 *__restrict__ bytes, u64 *__restrict__ range,
                                                u64 *__restrict__ ctr)
{
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n)
        return;
    if (i == n)
    {
        bytes[n] = 0;
        return;
    }
    LnExtent x{};
    if (ls[i] != kLnNone)
        x = ln_extent(loc, ls, le, heads_before, mark_before, n, max_lines, i, ctr);
    if (!x.counted)
    {
        bytes[i] = 0;
        range[i] = 0;
        return;
    }
    bytes[i] = (x.first ? (u64)f.prefix : 0ull) + (x.end - x.src) + (x.solid ? (u64)f.before + f.after : 0ull) +
               (x.last ? (u64)f.close + 1ull : 0ull);
    range[i] = x.src | (x.first ? kLnFirst : 0ull) | (x.last ? kLnLast : 0ull) | (x.solid ? kLcSolid : 0ull);
}

// ---- host side ------------------------------------------------------------------------------------------------------------

int ln_check(const char *who, const void *d_text, const void *d_positions, uint64_t n, krep_gpu_lines_out_t *out)
{
    if (!out)
        return fail("%s: out is NULL", who);
    *out = krep_gpu_lines_out_t{};
    return fmt_enter(who, nullptr, n && (!d_text || !d_positions), "d_text / d_positions", n);
}

// The scratch of a line analysis (g_fmt_mu held): the 8 counter words, `own_words` words of the caller's (16-byte aligned: they follow
// the counters), the block table and its scans, six words per record and one more, the sums, then `own_bytes` bytes at w.prefix
static int ln_layout(u64 text_len, u64 n, u64 own_words, size_t own_bytes, LnWork &w, u64 *&own)
{
    const u64 nb = (text_len + kLnBlock - 1) / kLnBlock, n1 = n + 1;
    const u64 sums = scan_sums_words(std::max(nb, n1));
    FmtCursor c;
    if (c.reserve(8 + own_words + 4 * nb + 6 * n1 + sums, own_bytes))
        return 2;
    w.nb = nb;
    w.ctr = c.take(8);
    own = c.take(own_words);
    w.last1 = c.take(nb), w.prev1 = c.take(nb), w.first_rev = c.take(nb), w.next_rev = c.take(nb);
    w.ls = c.take(n1), w.le = c.take(n1), w.a = c.take(n1), w.heads_before = c.take(n1), w.mark_before = c.take(n1), w.range = c.take(n1);
    w.sums = c.take(sums);
    w.prefix = c.tail();
    return 0;
}

// step (1) on `st`: the block table and its two running maxima
static void ln_table(const uint8_t *d_text, u64 text_len, const LnWork &w, hipStream_t st)
{
    const u32 grid_t = (u32)std::min<u64>((w.nb + 3) / 4, 256u * 32u);
    hipLaunchKernelGGL(ln_block_table, dim3(grid_t), dim3(256), 0, st, d_text, text_len, w.nb, w.last1, w.first_rev);
    scan_exclusive(w.last1, w.nb, w.prev1, w.sums, true, st);
    scan_exclusive(w.first_rev, w.nb, w.next_rev, w.sums, true, st);
}

// steps (2)-(3) on `st`; win != NULL: the window's (2") and (3"), which leave the relative copy of the list in `loc`
static void ln_records(const uint8_t *d_text, u64 text_len, const u64 *d_rec, u64 n, const LnWork &w, hipStream_t st,
                       const LwWindow *win = nullptr, u64 *loc = nullptr)
{
    const u64 n1 = n + 1;
    const u32 grid_n = (u32)((n1 + 255) / 256);
    if (win)
    {
        hipLaunchKernelGGL(lw_bounds, dim3(grid_n), dim3(256), 0, st, d_text, text_len, d_rec, n, *win, (const u64 *)w.prev1,
                           (const u64 *)w.next_rev, w.nb, loc, w.ls, w.le, w.ctr);
        hipLaunchKernelGGL(lw_heads, dim3(grid_n), dim3(256), 0, st, (const u64 *)w.ls, n, w.a, w.range);
    }
    else
    {
        hipLaunchKernelGGL(ln_bounds, dim3(grid_n), dim3(256), 0, st, d_text, text_len, d_rec, n, (const u64 *)w.prev1,
                           (const u64 *)w.next_rev, w.nb, w.ls, w.le, w.ctr);
        hipLaunchKernelGGL(ln_heads, dim3(grid_n), dim3(256), 0, st, (const u64 *)w.ls, n, w.a, w.range);
    }
    scan_exclusive(w.a, n1, w.heads_before, w.sums, false, st);
    scan_exclusive(w.range, n1, w.mark_before, w.sums, true, st);
}

// the layout and steps (1)-(3) on `st` (g_fmt_mu held by the caller)
int ln_analyse(const uint8_t *d_text, u64 text_len, const u64 *d_rec, u64 n, size_t prefix_len, LnWork &w, hipStream_t st)
{
    if (!text_len)
        return fail("krep_gpu_matching_lines / krep_gpu_format_lines: records on an empty text");
    u64 *none = nullptr;
    if (ln_layout(text_len, n, 0, prefix_len, w, none))
        return 2;
    HIPCHK(hipMemsetAsync(w.ctr, 0, 8 * sizeof(u64), st));
    ln_table(d_text, text_len, w, st);
    ln_records(d_text, text_len, d_rec, n, w, st);
    HIPCHK(hipGetLastError());
    return 0;
}

int ln_read_back(const char *who, const char *what, const LnWork &w, const u64 *off, u64 n, u64 max_lines, u64 *h, int k,
                 krep_gpu_lines_out_t *out, hipStream_t st)
{
    u64 total = 0, bytes = 0;
    HIPCHK(hipMemcpyAsync(&total, w.heads_before + n, sizeof(u64), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&bytes, off + n, sizeof(u64), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(h, w.ctr, k * sizeof(u64), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (h[0])
        return fail("%s: the record list is not ascending in start, or a record lies outside the %s", who, what);
    out->lines = std::min<u64>(total, max_lines);
    out->lines_total = total;
    out->out_bytes = bytes;
    out->capped_lines = h[1];
    return 0;
}

} // namespace kg

using namespace kg;

extern "C" int krep_gpu_matching_lines(const void *d_text, size_t text_len, const match_position_t *d_positions, uint64_t n,
                                       uint64_t max_lines, match_position_t *d_lines, uint64_t *d_first_record, uint64_t line_capacity,
                                       krep_gpu_lines_out_t *out, void *stream)
{
    if (ln_check("krep_gpu_matching_lines", d_text, d_positions, n, out))
        return 2;
    if (!n)
        return 0;
    hipStream_t st = (hipStream_t)stream;
    std::lock_guard<std::mutex> lk(g_fmt_mu);
    LnWork w;
    if (ln_analyse((const uint8_t *)d_text, text_len, (const u64 *)d_positions, n, 0, w, st))
        return 2;
    u64 h[2] = {0, 0}, total = 0;
    HIPCHK(hipMemcpyAsync(&total, w.heads_before + n, sizeof(u64), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(h, w.ctr, sizeof(u64), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (h[0])
        return fail("krep_gpu_matching_lines: the record list is not ascending in start, or a record lies outside the text");
    const u64 emit = std::min<u64>(total, max_lines);
    const bool query = !d_lines || !d_first_record || !line_capacity;
    const bool fits = !query && emit <= line_capacity;
    hipLaunchKernelGGL(ln_spans, dim3((u32)((n + 255) / 256)), dim3(256), 0, st, (const u64 *)w.ls, (const u64 *)w.le,
                       (const u64 *)w.heads_before, (const u64 *)w.mark_before, (u64)n, emit, fits ? 1 : 0, (u64 *)d_lines,
                       (u64 *)d_first_record, w.ctr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(h, w.ctr, 2 * sizeof(u64), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    out->lines = emit;
    out->lines_total = total;
    out->capped_lines = h[1];
    out->overflow = !query && !fits;
    return 0;
}

extern "C" int krep_gpu_format_lines(const void *d_text, size_t text_len, const match_position_t *d_positions, uint64_t n,
                                     uint64_t max_lines, const char *prefix, size_t prefix_len, void *d_out, size_t out_capacity,
                                     krep_gpu_lines_out_t *out, void *stream)
{
    if (ln_check("krep_gpu_format_lines", d_text, d_positions, n, out))
        return 2;
    if (prefix_len && !prefix)
        return fail("krep_gpu_format_lines: prefix is NULL");
    if (prefix_len >> 20)
        return fail("krep_gpu_format_lines: a prefix of %zu bytes", prefix_len);
    if (!n)
        return 0;
    hipStream_t st = (hipStream_t)stream;
    std::lock_guard<std::mutex> lk(g_fmt_mu);
    LnWork w;
    if (ln_analyse((const uint8_t *)d_text, text_len, (const u64 *)d_positions, n, prefix_len, w, st))
        return 2;
    if (prefix_len)
        HIPCHK(hipMemcpyAsync(w.prefix, prefix, prefix_len, hipMemcpyHostToDevice, st));
    u64 *off = w.ls; // the line starts are not read again behind ln_sizes: their buffer takes the summed byte counts
    hipLaunchKernelGGL(ln_sizes, dim3((u32)((n + 1 + 255) / 256)), dim3(256), 0, st, (const u64 *)d_positions, (const u64 *)w.ls,
                       (const u64 *)w.le, (const u64 *)w.heads_before, (const u64 *)w.mark_before, (u64)n, (u64)max_lines, (u64)prefix_len,
                       w.a, w.range, w.ctr);
    scan_exclusive(w.a, n + 1, off, w.sums, false, st);
    HIPCHK(hipGetLastError());
    u64 h[2] = {0, 0};
    if (ln_read_back("krep_gpu_format_lines", "text", w, off, n, max_lines, h, 2, out, st))
        return 2;
    return fmt_gather(out->out_bytes, d_out, out_capacity, nullptr, &out->overflow, st, [&](uint8_t *o, u32 misalign, u64 nchunks, u32 grid) {
        hipLaunchKernelGGL(ln_gather, dim3(grid), dim3(256), 0, st, (const uint8_t *)d_text, (const u64 *)off, (const u64 *)w.range, (u64)n,
                           (const uint8_t *)w.prefix, (u32)prefix_len, o, (u64)out->out_bytes, misalign, nchunks);
    });
}

extern "C" int krep_gpu_format_lines_ex(const void *d_text, size_t text_len, const match_position_t *d_positions, uint64_t n,
                                        uint64_t max_lines, const krep_gpu_line_format_t *fmt, void *d_out, size_t out_capacity,
                                        krep_gpu_lines_out_t *out, void *stream)
{
    const char *who = "krep_gpu_format_lines_ex";
    if (ln_check(who, d_text, d_positions, n, out))
        return 2;
    const krep_gpu_line_format_t none{};
    const krep_gpu_line_format_t &m = fmt ? *fmt : none;
    const FormatStrings fs{{m.prefix, m.prefix_len}, {m.before_match, m.before_match_len}, {m.after_match, m.after_match_len},
                           {m.line_close, m.line_close_len}};
    if (fs.refuse(who))
        return 2;
    if (!n)
        return 0;
    hipStream_t st = (hipStream_t)stream;
    std::lock_guard<std::mutex> lk(g_fmt_mu);
    const LcFixed f{(u32)fs.len(0), (u32)fs.len(1), (u32)fs.len(2), (u32)fs.len(3)};
    LnWork w;
    if (ln_analyse((const uint8_t *)d_text, text_len, (const u64 *)d_positions, n, fs.bytes(), w, st) || fs.upload(w.prefix, st))
        return 2;
    u64 *off = w.ls; // the line starts are not read again behind lc_sizes: their buffer takes the summed byte counts
    hipLaunchKernelGGL(lc_sizes, dim3((u32)((n + 1 + 255) / 256)), dim3(256), 0, st, (const u64 *)d_positions, (const u64 *)w.ls,
                       (const u64 *)w.le, (const u64 *)w.heads_before, (const u64 *)w.mark_before, (u64)n, (u64)max_lines, f, w.a,
                       w.range, w.ctr);
    scan_exclusive(w.a, n + 1, off, w.sums, false, st);
    HIPCHK(hipGetLastError());
    u64 h[2] = {0, 0};
    if (ln_read_back(who, "text", w, off, n, max_lines, h, 2, out, st))
        return 2;
    return fmt_gather(out->out_bytes, d_out, out_capacity, nullptr, &out->overflow, st, [&](uint8_t *o, u32 misalign, u64 nchunks, u32 grid) {
        hipLaunchKernelGGL(lc_gather, dim3(grid), dim3(256), 0, st, (const uint8_t *)d_text, (const u64 *)d_positions, (const u64 *)w.le,
                           (const u64 *)off, (const u64 *)w.range, (u64)n, (const uint8_t *)w.prefix, f, o, (u64)out->out_bytes, misalign,
                           nchunks);
    });
}

extern "C" int krep_gpu_format_lines_window(const void *d_text, size_t text_len, const krep_gpu_lines_window_t *win,
                                            const match_position_t *d_positions, uint64_t n, uint64_t max_lines,
                                            const krep_gpu_line_format_t *fmt, void *d_out, size_t out_capacity,
                                            krep_gpu_lines_window_out_t *out, void *stream)
{
    const char *who = "krep_gpu_format_lines_window";
    if (!out)
        return fail("%s: out is NULL", who);
    *out = krep_gpu_lines_window_out_t{};
    if (ln_check(who, d_text, d_positions, n, &out->lines))
        return 2;
    const krep_gpu_line_format_t none{};
    const krep_gpu_line_format_t &m = fmt ? *fmt : none;
    const FormatStrings fs{{m.prefix, m.prefix_len}, {m.before_match, m.before_match_len}, {m.after_match, m.after_match_len},
                           {m.line_close, m.line_close_len}};
    if (fs.refuse(who))
        return 2;
    if (!win)
        return fail("%s: win is NULL", who);
    const u64 gb = win->global_base, glen = win->global_len;
    if (gb > glen || text_len > glen - gb)
        return fail("%s: the buffer [%zu, +%zu) does not lie inside a text of %zu bytes", who, win->global_base, text_len, win->global_len);
    if (!(gb <= win->own_lo && win->own_lo <= win->own_hi && win->own_hi <= win->records_hi && win->records_hi <= gb + text_len))
        return fail("%s: the window wants global_base <= own_lo <= own_hi <= records_hi <= global_base + text_len", who);
    if (win->own_lo == gb && gb != 0)
        return fail("%s: own_lo == global_base > 0: the byte in front of own_lo must be in the buffer", who);
    out->incomplete_first_record = n;
    if (!n)
        return 0;
    if (!text_len)
        return fail("%s: records on an empty buffer", who);
    hipStream_t st = (hipStream_t)stream;
    std::lock_guard<std::mutex> lk(g_fmt_mu);
    const LcFixed f{(u32)fs.len(0), (u32)fs.len(1), (u32)fs.len(2), (u32)fs.len(3)};
    const LwWindow lw{gb, win->own_lo - gb, win->own_hi - gb, win->records_hi - gb,
                      (gb + text_len == glen && win->records_hi == glen) ? 1u : 0u};
    // ln_analyse's steps with the window's kernels in (2)-(3); the relative copy of the list lies behind the counter words
    LnWork w;
    u64 *loc = nullptr;
    if (ln_layout(text_len, n, 2 * (n + 1), fs.bytes(), w, loc))
        return 2;
    HIPCHK(hipMemsetAsync(w.ctr, 0, 8 * sizeof(u64), st));
    HIPCHK(hipMemsetAsync(w.ctr + kLwFirst, 0xff, sizeof(u64), st));
    if (fs.upload(w.prefix, st))
        return 2;
    ln_table((const uint8_t *)d_text, text_len, w, st);
    ln_records((const uint8_t *)d_text, text_len, (const u64 *)d_positions, n, w, st, &lw, loc);
    u64 *off = w.ls; // the line starts are not read again behind lw_sizes: their buffer takes the summed byte counts
    hipLaunchKernelGGL(lw_sizes, dim3((u32)((n + 1 + 255) / 256)), dim3(256), 0, st, (const u64 *)loc, (const u64 *)w.ls, (const u64 *)w.le,
                       (const u64 *)w.heads_before, (const u64 *)w.mark_before, (u64)n, (u64)max_lines, f, w.a, w.range, w.ctr);
    scan_exclusive(w.a, n + 1, off, w.sums, false, st);
    HIPCHK(hipGetLastError());
    u64 h[4] = {0, 0, 0, 0};
    if (ln_read_back(who, "buffer", w, off, n, max_lines, h, 4, &out->lines, st))
    {
        if (h[0])
            out->incomplete_first_record = 0;
        return 2;
    }
    // the incomplete line is the last owned one: lines_total lines stand in front of it
    if (h[kLwFirst] != kLnNone && out->lines.lines_total < max_lines)
    {
        out->incomplete_line_start1 = h[kLwStart1];
        out->incomplete_first_record = h[kLwFirst];
    }
    return fmt_gather(out->lines.out_bytes, d_out, out_capacity, nullptr, &out->lines.overflow, st,
                      [&](uint8_t *o, u32 misalign, u64 nchunks, u32 grid) {
                          hipLaunchKernelGGL(lc_gather, dim3(grid), dim3(256), 0, st, (const uint8_t *)d_text, (const u64 *)loc,
                                             (const u64 *)w.le, (const u64 *)off, (const u64 *)w.range, (u64)n, (const uint8_t *)w.prefix, f, o,
                                             (u64)out->lines.out_bytes, misalign, nchunks);
                      });
}
