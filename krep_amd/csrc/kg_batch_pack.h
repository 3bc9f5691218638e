// kg_batch_pack.h — a batch of texts as one pack, on the host (krep_gpu_search_batch, kg_batch.hip): the offset table
// of the next pack and the bytes of any slice of it.  Host code without any HIP in it, so that a stand-alone program can run it under
// the sanitizers (tools/batch_fill_san.cpp) and the CPU suite can ask it through krep_gpu_debug_batch_fill_host
// (tests/test_batch_fill_cpu.py).  The pack is never built on the host: the staging ring (kg_exec.hip Stager::gather) asks for one chunk
// at a time, and for a large chunk a quarter of it per thread.
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/krep_gpu.h"

namespace kg {

// off = the offset table of the leading items of items[0, n) that make ONE pack, and their number: item k lies at [off[k], off[k] + len),
// its separator on the byte behind it, off[last + 1] = packed size + 1.  The pack is cut between items and never inside one, in front of
// the first item that would end beyond `limit`; an item beyond the limit is a pack of its own.
inline size_t batch_pack_offsets(const krep_gpu_batch_item_t *items, size_t n, uint64_t limit, std::vector<uint64_t> &off)
{
    off.assign(1, 0);
    size_t i1 = 0;
    for (; i1 < n; ++i1)
    {
        const uint64_t end = off.back() + items[i1].len; // (the separator in front of it is in off.back() already)
        if (i1 > 0 && end > limit)
            break;
        off.push_back(end + 1);
    }
    return i1;
}

// bytes [lo, lo + cnt) of the pack of items[0, n) into dst, for any slice inside the pack (lo + cnt <= off[n] - 1): it may begin in the
// middle of an item, on a separator, or in a run of empty items
inline void batch_fill(const krep_gpu_batch_item_t *items, const uint64_t *off, size_t n, uint8_t *dst, size_t lo, size_t cnt)
{
    size_t k = (size_t)(std::upper_bound(off, off + n, (uint64_t)lo) - off) - 1;
    for (size_t pos = lo, end = lo + cnt; pos < end; ++k)
    {
        const size_t ib = (size_t)off[k], ie = ib + items[k].len;
        if (pos < ie)
        {
            const size_t c = std::min(ie, end) - pos;
            memcpy(dst + (pos - lo), items[k].text + (pos - ib), c);
            pos += c;
        }
        if (pos < end && pos == ie)
            dst[pos++ - lo] = '\n';
    }
}

// krep_gpu_grep_batch: the prefixes of n items behind one another in `blob`, poff[k] = where prefix k begins, poff[n] = the blob's size:
// what the device formatters read a prefix through.  -1, or the index of the first prefix that is NULL with a length or longer than
// max_len bytes (the vectors then hold the prefixes in front of it)
inline long batch_prefix_blob(const char *const *prefixes, const size_t *lens, size_t n, size_t max_len, std::vector<uint8_t> &blob,
                              std::vector<uint64_t> &poff)
{
    blob.clear();
    poff.assign(1, 0);
    size_t total = 0;
    for (size_t k = 0; k < n; ++k)
        total += lens[k] <= max_len ? lens[k] : 0;
    blob.reserve(total);
    for (size_t k = 0; k < n; ++k)
    {
        if (lens[k] > max_len || (lens[k] && !prefixes[k]))
            return (long)k;
        if (lens[k])
            blob.insert(blob.end(), (const uint8_t *)prefixes[k], (const uint8_t *)prefixes[k] + lens[k]);
        poff.push_back(blob.size());
    }
    return -1;
}

} // namespace kg
