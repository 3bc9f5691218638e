// kg_format_dev.h — the device helpers and small structs the output formatters share: kg_lines.hip (the matching lines), kg_matches.hip
// (the -o output) and kg_batch_format.hip (both over a pack of items).  What a record adds to the output is described ONCE here (LnExtent,
// LcItem, OmItem); the kernels around these helpers stay with their files.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/krep_gpu.h"
#include "kg_device.h"

namespace kg {

// ---- the matching lines (kg_lines.hip) ---------------------------------------------------------------------------------------
constexpr u32 kLnBlock = 4096;           // the table keeps the first and the last newline per 4 KiB of text
constexpr u64 kLnCap = 2048;             // MAX_MATCHES_PER_LINE (krep.c:496)
constexpr u64 kLnNone = ~0ull;
constexpr u64 kLnFirst = 1ull << 63, kLnLast = 1ull << 62, kLnSrc = kLnLast - 1; // a record's range word: flags | source offset


struct LnRecord
{
    bool head;
    u64 line, first; // index of its line, index of that line's first record
};
__device__ __forceinline__ LnRecord ln_record(const u64 *ls, const u64 *heads_before, const u64 *mark_before, u64 i)
{
    LnRecord r;
    r.head = i == 0 || ls[i] != ls[i - 1];
    r.line = heads_before[i] + (r.head ? 1u : 0u) - 1u;
    r.first = r.head ? i : mark_before[i] - 1;
    return r;
}

// what record i adds to its line: ONE range [src, end) of the text; counted: it is among the first 2048 records of an emitted line
struct LnExtent
{
    bool counted, first, last, solid; // first / last counted record of its line; solid: its clamped match [start, cend) is not empty
    u64 src, end;
};
__device__ __forceinline__ LnExtent ln_extent(const u64 *__restrict__ rec, const u64 *__restrict__ ls, const u64 *__restrict__ le,
                                              const u64 *__restrict__ heads_before, const u64 *__restrict__ mark_before, u64 n,
                                              u64 max_lines, u64 i, u64 *__restrict__ ctr)
{
    LnExtent x{};
    const LnRecord r = ln_record(ls, heads_before, mark_before, i);
    const u64 emit = min(heads_before[n], max_lines), rank = i - r.first;
    if (r.line < emit && rank == kLnCap)
        (void)__hip_atomic_fetch_add(ctr + 1, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (r.line >= emit || rank >= kLnCap)
        return x;
    const u64 a = ls[i], z = le[i], s = rec[2 * i], cend = min(rec[2 * i + 1], z);
    const bool solid = s < cend; // its clamped match is not empty
    // the cursor in front of it: the clamped end of the nearest record before it on the line whose match is not empty (the record
    // just before it, unless that one starts on the newline or is empty: at most 2047 steps, on such lists only)
    u64 cur = a;
    for (u64 j = i; j > r.first; --j)
    {
        const u64 sj = rec[2 * (j - 1)], ej = min(rec[2 * (j - 1) + 1], z);
        if (sj < ej)
        {
            cur = ej;
            break;
        }
    }
    x.counted = true;
    x.first = rank == 0;
    x.last = rank == kLnCap - 1 || i + 1 == n || ls[i + 1] != a;
    x.solid = solid;
    x.src = solid ? min(s, cur) : cur;
    x.end = x.last ? z : (solid ? cend : cur);
    return x;
}

// the largest r in [lo, hi] with off[r] <= pos (off[lo] <= pos)
__device__ __forceinline__ u64 ln_find(const u64 *__restrict__ off, u64 lo, u64 hi, u64 pos)
{
    while (lo < hi)
    {
        const u64 mid = lo + (hi - lo + 1) / 2;
        if (off[mid] <= pos)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}

// the lines with the caller's strings in them: one more flag in the range word, and the strings' lengths
constexpr u64 kLcSolid = 1ull << 61, kLcSrc = kLcSolid - 1; // one more flag in the range word

struct LcFixed
{
    u32 prefix, before, after, close; // the lengths; in `fix`: prefix | before_match | after_match | line_close
};

// one record's output, counted from its first byte: prefix [0, e0), text [e0, e1), before_match [e1, e2), the match [e2, e3),
// after_match [e3, e4), text [e4, e5), line_close [e5, e6), '\n' at e6 if the record closes its line.  Lines of 1 GiB and more are
// legal: the ends are 64-bit.  The three text pieces are one range: byte k of them is text[src + k - (string bytes in front of k)]
struct LcItem
{
    u64 src, e1, e2, e3, e4, e5, e6, total;
    u32 e0;
};
__device__ __forceinline__ LcItem lc_item(const u64 *__restrict__ rec, const u64 *__restrict__ le, const u64 *__restrict__ off,
                                          const u64 *__restrict__ range, const LcFixed f, u64 r)
{
    LcItem it;
    const u64 w = range[r];
    const bool first = w & kLnFirst, last = w & kLnLast, solid = w & kLcSolid;
    it.total = off[r + 1] - off[r];
    it.src = w & kLcSrc;
    u64 t1 = 0, t2 = 0;
    if (solid)
    {
        const uint4 p = *reinterpret_cast<const uint4 *>(rec + 2 * r);
        const u64 s = ((u64)p.y << 32) | p.x, e = min(((u64)p.w << 32) | p.z, le[r]);
        t1 = s - it.src;
        t2 = e - s;
    }
    it.e0 = first ? f.prefix : 0u;
    it.e1 = it.e0 + t1;
    it.e2 = it.e1 + (solid ? f.before : 0u);
    it.e3 = it.e2 + t2;
    it.e4 = it.e3 + (solid ? f.after : 0u);
    it.e6 = it.total - (last ? 1u : 0u);
    it.e5 = it.e6 - (last ? f.close : 0u);
    return it;
}
// its byte k (k < total)
__device__ __forceinline__ u32 lc_byte(const uint8_t *__restrict__ text, const uint8_t *__restrict__ fix, const LcFixed f, const LcItem &it,
                                       u64 k)
{
    if (k < it.e2)
    {
        if (k < it.e0)
            return fix[k];
        return k < it.e1 ? (u32)text[it.src + (k - it.e0)] : (u32)fix[f.prefix + (k - it.e1)];
    }
    if (k < it.e4)
        return k < it.e3 ? (u32)text[it.src + (k - it.e2) + (it.e1 - it.e0)] : (u32)fix[f.prefix + f.before + (k - it.e3)];
    if (k < it.e5)
        return text[it.src + (k - it.e4) + (it.e1 - it.e0) + (it.e3 - it.e2)];
    return k < it.e6 ? (u32)fix[f.prefix + f.before + f.after + (k - it.e5)] : (u32)'\n';
}

// the scratch of one line analysis (host side: ln_analyse lays it out)
struct LnWork
{
    u64 *ctr, *last1, *prev1, *first_rev, *next_rev; // counters {refused, capped lines}; the block table and its scans
    u64 *ls, *le, *a, *heads_before, *mark_before, *range, *sums;
    uint8_t *prefix;
    u64 nb;
};
// kg_lines.hip: the checks every line call makes first, and steps (1)-(3) on `st` (g_fmt_mu held by the caller); `prefix_len` bytes
// are left for the caller behind the words, at w.prefix (8-byte aligned)
int ln_check(const char *who, const void *d_text, const void *d_positions, uint64_t n, krep_gpu_lines_out_t *out);
int ln_analyse(const uint8_t *d_text, u64 text_len, const u64 *d_rec, u64 n, size_t prefix_len, LnWork &w, hipStream_t st);

// ---- the -o output (kg_matches.hip) ------------------------------------------------------------------------------------------
constexpr u64 kOmStaleAfter = 10;          // result->count > 10 builds the newline index (krep.c:531)
constexpr u64 kOmMaxText = 10000000000000000ull; // a line number has at most 16 digits here (two registers of 8)

// newlines among the 16 bytes
__device__ __forceinline__ u32 nl_count16(const uint4 v)
{
    return (u32)(__popc(eq_bytes(v.x, 0x0a0a0a0au)) + __popc(eq_bytes(v.y, 0x0a0a0a0au)) + __popc(eq_bytes(v.z, 0x0a0a0a0au)) +
                 __popc(eq_bytes(v.w, 0x0a0a0a0au)));
}
// newlines in text[lo, hi) (hi <= text_len), any alignment
__device__ __forceinline__ u32 nl_count(const uint8_t *__restrict__ text, u64 lo, u64 hi)
{
    u32 c = 0;
    u64 p = lo;
#pragma unroll 4
    for (; p + 16 <= hi; p += 16)
        c += nl_count16(load_unaligned<uint4>(text + p));
    for (; p < hi; ++p)
        c += text[p] == '\n';
    return c;
}
__device__ __forceinline__ u32 om_digits(u64 v)
{
    u32 d = 1;
    for (; v >= 10; v /= 10)
        ++d;
    return d;
}

// the largest r in [lo, hi] with off[r] <= pos (off[lo] <= pos)
__device__ __forceinline__ u64 om_find(const u64 *__restrict__ off, u64 lo, u64 hi, u64 pos)
{
    while (lo < hi)
    {
        const u64 mid = lo + (hi - lo + 1) / 2;
        if (off[mid] <= pos)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}

// the lengths of the three fixed strings, which lie behind one another in `fix`: prefix + before_number | after_number | after_match
struct OmFixed
{
    u32 head, mid, tail;
};
// one record's output: where its parts end, counted from its first byte (b6 + 1 = its length)
struct OmItem
{
    u64 src, b4, b5; // the match is text[src, src + b5 - b4)
    u64 dlo, dhi;    // the digits of LINE as characters, the first one in the lowest byte of dlo
    u32 b1, b2;      // head [0, b1), digits [b1, b2), ':' at b2, after_number [b2 + 1, b4), after_match [b5, b6), '\n' at b6
    u64 b6;
};
// (`base`: the text offset of text[0] — 0 for the whole-text call, global_base for a window, whose text_len is the whole text's length)
__device__ __forceinline__ OmItem om_item(const u64 *__restrict__ rec, const u64 *__restrict__ line, u64 text_len, const OmFixed f, u64 r,
                                          u64 base = 0)
{
    OmItem it;
    const uint4 w = *reinterpret_cast<const uint4 *>(rec + 2 * r);
    const u64 s = ((u64)w.y << 32) | w.x, e = min(((u64)w.w << 32) | w.z, text_len);
    u64 v = line[r], lo = 0, hi = 0;
    u32 d = 0;
    do // the least significant digit first: each one pushes the others up by a byte
    {
        hi = (hi << 8) | (lo >> 56);
        lo = (lo << 8) | (u64)('0' + (u32)(v % 10));
        v /= 10;
        ++d;
    } while (v);
    it.src = s - base;
    it.dlo = lo;
    it.dhi = hi;
    it.b1 = f.head;
    it.b2 = f.head + d;
    it.b4 = (u64)it.b2 + 1 + f.mid;
    it.b5 = it.b4 + (e - s);
    it.b6 = it.b5 + f.tail;
    return it;
}
// its byte k (k <= b6)
__device__ __forceinline__ u32 om_byte(const uint8_t *__restrict__ text, const uint8_t *__restrict__ fix, const OmFixed f, const OmItem &it, u64 k)
{
    if (k >= it.b4)
    {
        if (k < it.b5)
        {
            const u32 c = text[it.src + (k - it.b4)];
            return c == '\n' ? (u32)' ' : c;
        }
        return k < it.b6 ? (u32)fix[f.head + f.mid + (k - it.b5)] : (u32)'\n';
    }
    if (k < it.b1)
        return fix[k];
    if (k < it.b2)
    {
        const u32 j = (u32)k - it.b1;
        return (u32)((j < 8 ? it.dlo >> (8 * j) : it.dhi >> (8 * (j - 8))) & 0xffu);
    }
    return k == it.b2 ? (u32)':' : (u32)fix[f.head + (k - it.b2 - 1)];
}
// '\n' -> ' ' in the four bytes of w: the bytes differ in 0x2a
__device__ __forceinline__ u32 om_blank(u32 w) { return w ^ ((eq_bytes(w, 0x0a0a0a0au) >> 7) * 0x2au); }
// kg_matches.hip: step (2) of the -o output on `st`: line[i] = 1 + the newlines in front of record i's start, ctr[0] raised by a
// record that may not be read (om_lines)
void om_lines_on(const uint8_t *d_text, u64 text_len, const u64 *d_rec, u64 n, const u64 *before, u64 nblocks, u64 *line, u64 *ctr,
                 hipStream_t st);

// ---- a record list cut by offsets (kg_batch.hip, kg_batch_format.hip) --------------------------------------------------------
// first index k in [0, n) whose record starts at or behind `key` (n when none): the list is item-contiguous in item order, so
// "starts in front of an item's base" is a prefix of it whether it ascends in start (single literal, regex) or in end (multi-pattern)
__device__ __forceinline__ u64 first_record_at(const u64 *__restrict__ rec, u64 n, u64 key)
{
    u64 lo = 0, hi = n;
    while (lo < hi)
    {
        const u64 mid = lo + (hi - lo) / 2;
        if (rec[2 * mid] < key)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

} // namespace kg
