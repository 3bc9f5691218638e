// tools/batch_fill_san.cpp — the host side of a batch's pack (krep_amd/csrc/kg_batch_pack.h: host code, no HIP) as a stand-alone
// program for AddressSanitizer / UBSan:  python tools/sanitize.py batchfill   (or by hand:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer tools/batch_fill_san.cpp -o batch_fill_san).
// Random lists of small items (a third of them empty), every item and every destination in a heap block of exactly its length so that a
// read or a write one byte out is a report; EVERY slice (lo, cnt) of each pack is asked of kg::batch_fill and compared with the same
// slice of a naive pack.  Then the cut rule of kg::batch_pack_offsets against its definition.  Prints the number of slices; exits 1 on a
// difference.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../krep_amd/csrc/kg_batch_pack.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n)
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return (uint32_t)((rng_state >> 33) % n);
}

int main()
{
    uint64_t slices = 0;
    for (int list = 0; list < 3000; ++list)
    {
        const size_t n = 1 + rnd(12);
        std::vector<std::unique_ptr<char[]>> blocks; // exact-size heap blocks: no slack behind an item
        std::vector<krep_gpu_batch_item_t> items(n);
        std::string naive;
        for (size_t i = 0; i < n; ++i)
        {
            const size_t len = rnd(3) == 0 ? 0 : rnd(9);
            blocks.emplace_back(len ? new char[len] : nullptr);
            for (size_t j = 0; j < len; ++j)
                blocks.back()[j] = (char)('a' + rnd(26));
            items[i].text = blocks.back().get();
            items[i].len = len;
            if (i)
                naive.push_back('\n');
            naive.append(blocks.back().get() ? blocks.back().get() : "", len);
        }
        std::vector<uint64_t> off;
        if (kg::batch_pack_offsets(items.data(), n, UINT64_MAX, off) != n || off.size() != n + 1 || off.back() != naive.size() + 1)
        {
            fprintf(stderr, "list %d: the offset table does not describe the pack\n", list);
            return 1;
        }
        for (size_t lo = 0; lo <= naive.size(); ++lo)
            for (size_t cnt = 0; lo + cnt <= naive.size(); ++cnt)
            {
                std::unique_ptr<uint8_t[]> dst(new uint8_t[cnt ? cnt : 1]);
                if (cnt)
                    kg::batch_fill(items.data(), off.data(), n, dst.get(), lo, cnt);
                if (cnt && memcmp(dst.get(), naive.data() + lo, cnt) != 0)
                {
                    fprintf(stderr, "list %d: slice (%zu, %zu) differs from the naive pack\n", list, lo, cnt);
                    return 1;
                }
                ++slices;
            }
        // the cut rule: between items, never inside one; an item beyond the limit is a pack of its own
        const uint64_t limit = rnd(20);
        for (size_t i0 = 0; i0 < n;)
        {
            const size_t took = kg::batch_pack_offsets(items.data() + i0, n - i0, limit, off);
            uint64_t used = 0;
            size_t want = 0;
            while (i0 + want < n && (want == 0 || used + items[i0 + want].len <= limit))
                used += items[i0 + want++].len + 1;
            if (took != want || took == 0 || off.size() != took + 1 || off.back() != used)
            {
                fprintf(stderr, "list %d: pack at item %zu under limit %llu: %zu items, expected %zu\n", list, i0, (unsigned long long)limit, took, want);
                return 1;
            }
            i0 += took;
        }
    }
    printf("batch_fill: %llu slices equal the naive pack\n", (unsigned long long)slices);
    return 0;
}
