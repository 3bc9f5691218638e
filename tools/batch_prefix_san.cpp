// tools/batch_prefix_san.cpp — the prefix blob of krep_gpu_grep_batch (krep_amd/csrc/kg_batch_pack.h kg::batch_prefix_blob: host code, no
// HIP) as a stand-alone program for AddressSanitizer / UBSan:  python tools/sanitize.py batchprefix   (or by hand:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer tools/batch_prefix_san.cpp -o batch_prefix_san).
// Random lists of prefixes (a third of them empty, some NULL with length 0), every prefix in a heap block of exactly its length so that
// a read one byte out is a report; the blob and the offsets are compared with a naive concatenation.  Then the two refusals: a prefix
// longer than the limit and a NULL prefix with a length, each reported by its index with the prefixes in front of it laid out.
// Prints the number of lists; exits 1 on a difference.
#include <cstdio>
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
    const size_t kMax = 40;
    int lists = 0;
    for (; lists < 20000; ++lists)
    {
        const size_t n = rnd(12);
        std::vector<std::unique_ptr<char[]>> blocks; // exact-size heap blocks: no slack behind a prefix
        std::vector<const char *> ptr(n);
        std::vector<size_t> len(n);
        std::string naive;
        std::vector<uint64_t> want(1, 0);
        long bad = -1;
        for (size_t i = 0; i < n; ++i)
        {
            size_t l = rnd(3) == 0 ? 0 : rnd((uint32_t)kMax + 1);
            const uint32_t kind = rnd(40);
            if (kind == 0)
                l = kMax + 1 + rnd(5); // too long
            blocks.emplace_back(l ? new char[l] : nullptr);
            for (size_t j = 0; j < l; ++j)
                blocks.back()[j] = (char)('a' + rnd(26));
            ptr[i] = blocks.back().get();
            len[i] = l;
            if (kind == 1 && l)
                ptr[i] = nullptr; // NULL with a length
            if (bad < 0 && (l > kMax || (l && !ptr[i])))
                bad = (long)i;
            if (bad < 0)
            {
                naive.append(ptr[i] ? ptr[i] : "", l);
                want.push_back(naive.size());
            }
        }
        std::vector<uint8_t> blob;
        std::vector<uint64_t> poff;
        const long got = kg::batch_prefix_blob(ptr.data(), len.data(), n, kMax, blob, poff);
        if (got != bad || poff != want || blob.size() != naive.size() || (blob.size() && memcmp(blob.data(), naive.data(), blob.size()) != 0))
        {
            fprintf(stderr, "list %d: %zu prefixes, first bad %ld (expected %ld), %zu bytes (expected %zu)\n", lists, n, got, bad, blob.size(),
                    naive.size());
            return 1;
        }
    }
    printf("batch_prefix_blob: %d lists equal the naive concatenation\n", lists);
    return 0;
}
