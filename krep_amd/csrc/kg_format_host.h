// kg_format_host.h — the host steps the grep-output drivers share between their extern "C" line and their launches (kg_lines.hip,
// kg_matches.hip, kg_batch_format.hip).  A driver is: fmt_enter and FormatStrings::refuse (nothing on the device yet), its own
// checks, g_fmt_mu, FmtCursor over the scratch, FormatStrings::upload, its kernels, a read-back (ln_read_back for the line
// drivers), fmt_gather.  The non-template parts are defined in kg_format.hip; ln_read_back in kg_lines.hip.
#pragma once
#include <algorithm>

#include "kg_device.h"
#include "kg_internal.h"

namespace kg {

// What every driver checks first, in this order: a HIP device, one this code object runs on, `refuse_first` (a driver's own refusal
// that stands in front of the pointers, e.g. "win is NULL"; NULL: none), `null_pointer` (the driver's own test: they differ) with
// the pointers' names, n < 2^40.  -> 2 and the message "<who>: ..."
int fmt_enter(const char *who, const char *refuse_first, bool null_pointer, const char *pointers, uint64_t n);

// The 3 or 4 host strings of a format, in the order they lie behind one another on the device
struct FormatStrings
{
    struct Str
    {
        const char *ptr;
        size_t len;
    };
    Str s[4] = {};
    int k = 0;
    FormatStrings(std::initializer_list<Str> l)
    {
        for (const Str &x : l)
            s[k++] = x;
    }
    int refuse(const char *who) const; // 2 and the message: the first string that is NULL with a length, or of 2^20 bytes or more
    size_t len(int i) const { return s[i].len; }
    size_t bytes() const { return s[0].len + s[1].len + s[2].len + s[3].len; }
    // (g_fmt_mu held) joins the strings in the one host staging vector, which lives until the copy has run, and queues the copy to d
    int upload(uint8_t *d, hipStream_t st) const;
};

// The scratch of a call (g_fmt_mu held): `words` 64-bit words handed out from the front in the order they are taken, then
// `tail_bytes` bytes (8-byte aligned)
struct FmtCursor
{
    u64 *p = nullptr;
    int reserve(u64 words, size_t tail_bytes)
    {
        void *base = nullptr;
        if (fmt_reserve(words * sizeof(u64) + tail_bytes + 16, &base))
            return 2;
        p = (u64 *)base;
        return 0;
    }
    u64 *take(u64 words)
    {
        u64 *q = p;
        p += words;
        return q;
    }
    uint8_t *tail() const { return (uint8_t *)p; }
};

// The line drivers' read-back (kg_lines.hip): heads_before[n], off[n] and ctr[0, k) -> h in one wait; h[0]: 2 and "<who>: the record
// list is not ascending in start, or a record lies outside the <what>"; else lines, lines_total, out_bytes and capped_lines of *out
struct LnWork;
int ln_read_back(const char *who, const char *what, const LnWork &w, const u64 *off, u64 n, u64 max_lines, u64 *h, int k,
                 krep_gpu_lines_out_t *out, hipStream_t st);

// The end of every gathering driver: the buffer from `grow` (if any), nothing to do on a size query or without bytes, *overflow on a
// capacity that is too small; else launch(out, misalign, nchunks, grid) — chunk c is the 16 aligned bytes at (out - misalign) + 16 c —
// and the wait for it
template <class Launch>
int fmt_gather(u64 bytes, void *d_out, size_t out_capacity, const FormatOutGrow *grow, int *overflow, hipStream_t st, Launch &&launch)
{
    if (grow && bytes)
    {
        d_out = (*grow)(bytes);
        out_capacity = bytes;
        if (!d_out)
            return 2;
    }
    if (!d_out || !out_capacity || !bytes)
        return 0;
    if (bytes > out_capacity)
    {
        *overflow = 1;
        return 0;
    }
    const u32 misalign = (u32)(reinterpret_cast<size_t>(d_out) & 15u);
    const u64 nchunks = (bytes + misalign + 15) / 16;
    const u32 grid = (u32)std::min<u64>((nchunks + 255) / 256, 256u * 64u);
    launch((uint8_t *)d_out, misalign, nchunks, grid);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
    return 0;
}

} // namespace kg
