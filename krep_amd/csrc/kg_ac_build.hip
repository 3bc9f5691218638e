// kg_ac_build.hip — host side of the multi-pattern scan: ac_build() turns a dictionary into the tables of kg_ac_tables.h
// (what ac_trie_build and its helpers are to aho_corasick_search, /root/reference/aho_corasick.c:74-297 — here a reversed trie,
// an exact-class 4-gram filter for LDS in two layouts, chain-compressed 4-gram buckets, exact bitmaps of the short patterns and
// the register-compare description of a tiny dictionary), ac_free() releases them.  Each table is built on the host by a step of
// its own and uploaded at the end; the two-way bucket fitter and the class-gram expansion serve kg_ac_anchor.hip as well.  No
// kernel in this file (round 5: split out of kg_ac.hip, which keeps the scan kernel and its drivers).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <unordered_map>
#include <vector>

#include "../../include/krep_gpu.h"
#include "kg_ac_common.h"
#include "kg_ac_tables.h"
#include "kg_internal.h"

namespace kg {

static inline uint8_t ac_lo8(uint8_t c) { return (c >= 'A' && c <= 'Z') ? (uint8_t)(c + 32) : c; }

TwoWayFit fit_two_way(size_t n, u32 nb_max, const u32 (&muls)[6], const std::function<u32(size_t, u32)> &hash)
{
    TwoWayFit f;
    f.slot.resize(n);
    std::vector<uint8_t> fill;
    for (u32 nb = 1024; nb <= nb_max; nb <<= 1)
    {
        if ((u64)nb * 2 < n)
            continue;
        for (u32 mul : muls)
        {
            fill.assign(nb, 0);
            size_t i = 0;
            for (; i < n; ++i)
            {
                const u32 b = hash(i, mul) & (nb - 1);
                if (fill[b] == 2)
                    break;
                f.slot[i] = 2 * b + fill[b]++;
            }
            if (i == n)
            {
                f.nb = nb;
                f.mul = mul;
                return f;
            }
        }
    }
    f.slot.clear();
    return f;
}

void set_class_grams(std::vector<u32> &tab, ClsLayout layout, const std::vector<uint8_t> &p, size_t end)
{
    const size_t ncls = layout == ClsLayout::Five ? 5 : 4, known = std::min(ncls, end);
    u32 fixed = 0; // the `known` classes in front of `end` (text order, the last one highest), the rest free
    for (size_t q = 0; q < known; ++q)
        fixed |= ((u32)p[end - known + q] & 31u) << (5 * (ncls - known + q));
    for (u32 f = 0, nfree = 1u << (5 * (ncls - known)); f < nfree; ++f)
    {
        const u32 x = fixed | f;
        u32 dw = x >> 5, bit = x & 31u;
        if (layout == ClsLayout::Pair || layout == ClsLayout::Pair19)
            ac_pair_slot(x, dw, bit);
        else if (layout == ClsLayout::Five)
            ac_pair_slot5(x >> 5, x & 31u, dw, bit); // (x & 31: the class of the byte in front of the gram)
        if (layout == ClsLayout::Plain19 || layout == ClsLayout::Pair19)
            dw &= (1u << (kXBitsLines - 5)) - 1u; // the kernel masks the byte address with 0xfffc
        tab[dw] |= 1u << bit;
    }
}

namespace {

// the host images of what ac_build uploads
struct AcHost
{
    std::vector<std::vector<uint8_t>> pats; // folded under -i, the empty ones left out
    std::vector<u32> S1, S2, S3;            // exact bitmaps of the 1-/2-/3-byte patterns (empty: no such pattern)
    std::unordered_map<u32, u32> edge;      // reversed trie: node << 8 | byte -> child
    std::vector<u32> copies;                // per node: patterns that end there
    std::vector<uint2> tab, g4;             // the edge table; exact 4-gram -> depth-4 node
    std::vector<uint4> g4x;                 // chain-compressed entries (same slots as g4, or the two-way buckets)
    std::vector<u32> X20, X19, S20, S19;    // filter tables (S20 / S19: the stride-2 filter, uploaded when stride2)
    bool stride2 = false;
};

// fold and validate the patterns; false after fail(...)
bool fold_patterns(const search_params_t &sp, AcTables *t, AcHost &h)
{
    if (sp.num_patterns > 4095)
    {
        fail("too many patterns (%zu > 4095; the reference CLI accepts 1024)", (size_t)sp.num_patterns);
        return false;
    }
    for (size_t i = 0; i < sp.num_patterns; ++i)
    {
        std::vector<uint8_t> p((const uint8_t *)sp.patterns[i], (const uint8_t *)sp.patterns[i] + sp.pattern_lens[i]);
        if (t->ci)
            for (auto &c : p)
                c = ac_lo8(c); // the trie is built on folded bytes (aho_corasick.c:161)
        if (p.empty())
        {
            t->has_empty = true; // only ever matches the empty text (aho_corasick.c:441-463)
            continue;
        }
        if (p.size() > 1024)
        {
            fail("pattern %zu longer than 1024 bytes", i);
            return false;
        }
        if (memchr(p.data(), '\n', p.size()))
            t->has_nl = true;
        t->lmax = std::max<u32>(t->lmax, (u32)p.size());
        t->lmin = t->lmin ? std::min<u32>(t->lmin, (u32)p.size()) : (u32)p.size();
        h.pats.push_back(std::move(p));
    }
    t->pats_h = h.pats; // (the anchor decision of kg_ac_anchor.hip, taken when the first large text arrives)
    return true;
}

// exact bitmaps of the short patterns (verifier)
void short_bitmaps(AcTables *t, AcHost &h)
{
    auto setbit = [&](std::vector<u32> &v, u32 words, u32 key) {
        if (v.empty())
            v.assign(words, 0);
        if ((v[key >> 5] >> (key & 31)) & 1u)
            t->short_dup = true;
        v[key >> 5] |= 1u << (key & 31);
    };
    for (auto &p : h.pats)
    {
        const size_t n = p.size();
        if (n == 1) { t->has1 = 1; setbit(h.S1, kS1Words, p[0]); }
        else if (n == 2) { t->has2 = 1; setbit(h.S2, kS2Words, (u32)p[0] | ((u32)p[1] << 8)); }
        else if (n == 3) { t->has3 = 1; setbit(h.S3, kS3Words, (u32)p[0] | ((u32)p[1] << 8) | ((u32)p[2] << 16)); }
        else t->has4 = 1;
    }
}

// bytes p[end - 1], p[end - 2], ... (n of them) into bytes 0, 1, ... of pk; lf marks the letters among them under -i
void tiny_pack(const std::vector<uint8_t> &p, size_t end, size_t n, bool ci, u32 &pk, u32 &lf)
{
    for (size_t s = 0; s < n; ++s)
    {
        const uint8_t c = p[end - 1 - s];
        pk |= (u32)c << (8 * s);
        lf |= (ci && c >= 'a' && c <= 'z') ? 1u << s : 0u;
    }
}

// tiny dictionary?  (kg_ac_tiny.hip: compared in registers, no tables)
void tiny_description(AcTables *t, const std::vector<std::vector<uint8_t>> &pats)
{
    AcTiny &td = t->tiny;
    // ... and worth it: with a 1- or 2-byte pattern the general kernel reads two or three LDS tables per position (3.3 TB/s
    // on `he she hers`, 1.4 on `e t`); a dictionary of 3- and 4-byte patterns only runs there at 5.2-5.9 TB/s, faster than
    // the register compare (profiles/r04_dictionaries.txt)
    // Lengths: 1..4, or 1..3 beside ONE length of 5..8 (`-e a -e Sherlock`), which then takes the place of length 4
    bool ok = !pats.empty() && !t->has_empty && t->lmax <= 8 && t->lmin <= 2 && !getenv("KREP_GPU_AC_NO_TINY");
    const u32 llong = t->lmax > 4 ? t->lmax : 0u;
    bool five = false; // 4-byte patterns beside the long length: the long ones become a fifth class (AcTiny::five)
    for (auto &q : pats)
        five = five || (llong && q.size() == 4);
    for (size_t i = 0; ok && i < pats.size(); ++i)
    {
        for (size_t k = 0; k < i; ++k)
            if (pats[k] == pats[i])
                ok = false; // a duplicate reports twice (aho_corasick.c:383-437): the masks cannot count copies
        const size_t L = pats[i].size();
        if (llong && L > 4 && L != llong)
            ok = false; // a second length beyond 4 bytes
        const bool in5 = five && L > 4;
        const size_t cls = L > 4 ? 4 : L; // the class a pattern is compared and reported in
        u32 &count = in5 ? td.n5 : td.n[cls - 1];
        if (!ok || count >= kTinyPer)
        {
            ok = false;
            break;
        }
        const u32 p = count++;
        // a long pattern: its LAST four bytes, and its first L - 4, byte s = s places before the end of that part
        tiny_pack(pats[i], L, cls, t->ci, in5 ? td.pk5[p] : td.pk[cls - 1][p], in5 ? td.lf5[p] : td.lf[cls - 1][p]);
        if (L > 4)
            tiny_pack(pats[i], L - 4, L - 4, t->ci, td.pk2[p], td.lf2[p]);
    }
    td.llong = ok ? llong : 0u;
    td.five = (ok && five) ? 1u : 0u;
    td.lmax = t->lmax;
    for (int L = 0; L < 4; ++L)
        td.ncls += td.n[L] ? 1u : 0u;
    td.ok = ok ? 1u : 0u;
    if (ok && t->lmax == 1 && pats.size() >= 2 && pats.size() <= 4)
    {
        t->set_n = (u32)pats.size();
        for (size_t i = 0; i < pats.size(); ++i)
            t->set_b[i] = pats[i][0];
    }
}

// the reversed trie and its edge table (linear probing); false after fail(...)
bool reversed_trie(AcTables *t, AcHost &h)
{
    h.copies.assign(1, 0);
    for (auto &p : h.pats)
    {
        u32 node = 0;
        for (size_t k = p.size(); k-- > 0;)
        {
            const u32 key = (node << 8) | p[k];
            auto it = h.edge.find(key);
            if (it == h.edge.end())
            {
                const u32 nn = (u32)h.copies.size();
                h.copies.push_back(0);
                h.edge.emplace(key, nn);
                node = nn;
            }
            else
                node = it->second;
        }
        h.copies[node]++;
    }
    t->nnodes = (u32)h.copies.size();
    if (t->nnodes >= (1u << 23))
    {
        fail("pattern set too large (%u trie nodes)", t->nnodes);
        return false;
    }
    u32 cap = 1024;
    while (cap < h.edge.size() * 2 + 16)
        cap <<= 1;
    t->emask = cap - 1;
    h.tab.assign(cap, make_uint2(0xffffffffu, 0u));
    for (auto &kv : h.edge)
    {
        u32 s = (kv.first * kHashMul) >> 7;
        while (h.tab[s & t->emask].x != 0xffffffffu)
            ++s;
        h.tab[s & t->emask] = make_uint2(kv.first, kv.second | (h.copies[kv.second] ? 0x80000000u : 0u));
    }
    return true;
}

// exact 4-gram -> depth-4 node (used when every pattern has >= 4 bytes), with the unary chain below that node (ac_walk_fast),
// in a sparse linear-probing table
void gram4_entries(AcTables *t, AcHost &h)
{
    struct Item { u32 node, depth, gram; };
    std::vector<std::vector<std::pair<u32, u32>>> kids(t->nnodes); // node -> (byte, child)
    for (auto &kv : h.edge)
        kids[kv.first >> 8].push_back({kv.first & 255u, kv.second});
    std::vector<Item> st{{0u, 0u, 0u}}, d4;
    while (!st.empty())
    {
        Item it = st.back();
        st.pop_back();
        if (it.depth == 4)
        {
            d4.push_back(it);
            continue;
        }
        for (auto &bc : kids[it.node])
            // depth-1 byte is text[i] (top byte of E), depth-4 byte is text[i-3] (low byte)
            st.push_back({bc.second, it.depth + 1, it.gram | (bc.first << (8 * (3 - it.depth)))});
    }
    // sparse on purpose (load <= 1/16 while the table stays <= 8 MiB): a probe sequence is a chain of DEPENDENT L2
    // round trips that the whole 64-candidate batch waits for; at load 1/2 the longest of ~80 probes took 4-5
    // steps and the verify stage 3x as long (2.30 -> 3.34 TB/s on config 4 with the stride-2 filter)
    u32 gcap = 1024;
    while (gcap < d4.size() * 16 + 16 && (size_t)gcap * 2 * 32 <= (8u << 20))
        gcap <<= 1;
    while (gcap < d4.size() * 2 + 16)
        gcap <<= 1;
    t->g4mask = gcap - 1;
    h.g4.assign(gcap, make_uint2(0u, 0u));
    h.g4x.assign(2 * (size_t)gcap, make_uint4(0u, 0u, 0u, 0u));
    for (auto &it : d4)
    {
        u32 s = (it.gram * kHashMul) >> 9;
        while (h.g4[s & t->g4mask].y != 0u)
            ++s;
        const u32 child = it.node | (h.copies[it.node] ? 0x80000000u : 0u);
        h.g4[s & t->g4mask] = make_uint2(it.gram, child);
        // the unary chain below the depth-4 node: <= 12 bytes, depths 5..16
        u32 node = it.node, clen = 0, endmask = 0;
        bool simple = h.copies[node] <= 1;
        uint8_t cb[12] = {0};
        while (clen < 12 && kids[node].size() == 1)
        {
            const u32 byte = kids[node][0].first;
            node = kids[node][0].second;
            cb[11 - clen] = (uint8_t)byte; // depth 5 + clen <-> window byte 16 - depth
            if (h.copies[node])
            {
                endmask |= 1u << clen;
                if (h.copies[node] != 1)
                    simple = false;
            }
            ++clen;
        }
        const u32 info = clen | (simple ? kG4Simple : 0u) | (!kids[node].empty() ? kG4Cont : 0u);
        auto word = [&](int w) { return (u32)cb[4 * w] | ((u32)cb[4 * w + 1] << 8) | ((u32)cb[4 * w + 2] << 16) | ((u32)cb[4 * w + 3] << 24); };
        h.g4x[2 * (size_t)(s & t->g4mask)] = make_uint4(it.gram, child, info, endmask);
        h.g4x[2 * (size_t)(s & t->g4mask) + 1] = make_uint4(word(0), word(1), word(2), 0u);
    }
}

// Preferred layout of the chain entries: buckets of two entries (one 64-byte line) with NO overfull bucket, so that a probe is
// one round trip without a loop; searched over a few multipliers and sizes up to 8 MiB.  Linear probing (above) stays as the
// fallback for dictionaries too large for that (the chance that three of n keys share one of nb buckets is ~ n^3 / (6 nb^2)).
// The entries are placed in the slot order of the linear-probing table.
void gram4_buckets(AcTables *t, AcHost &h)
{
    std::vector<u32> used; // occupied slots of the linear-probing table
    for (u32 s = 0; s <= t->g4mask; ++s)
        if (h.g4x[2 * (size_t)s].y != 0u)
            used.push_back(s);
    // (KREP_GPU_AC_LINEAR=1: test hook, keeps the linear-probing layout)
    if (used.empty() || getenv("KREP_GPU_AC_LINEAR"))
        return;
    const TwoWayFit f = fit_two_way(used.size(), (8u << 20) / 64, kBucketMuls, [&](size_t i, u32 mul) { return (h.g4x[2 * (size_t)used[i]].x * mul) >> 9; });
    if (!f.nb)
        return;
    std::vector<uint4> bk(4 * (size_t)f.nb, make_uint4(0u, 0u, 0u, 0u));
    for (size_t i = 0; i < used.size(); ++i)
    {
        bk[2 * (size_t)f.slot[i]] = h.g4x[2 * (size_t)used[i]];
        bk[2 * (size_t)f.slot[i] + 1] = h.g4x[2 * (size_t)used[i] + 1];
    }
    h.g4x.swap(bk);
    t->g4x_mode = 1;
    t->g4x_mask = f.nb - 1;
    t->g4x_mul = f.mul;
}

// filter: exact-class table over the last 4 bytes; a pattern shorter than 4 sets every class of the bytes in front of it
// (32 / 1024 / 32768 entries)
void filter_tables(AcTables *t, AcHost &h)
{
    h.X20.assign((1u << kXBitsBig) / 32, 0);
    h.X19.assign((1u << kXBitsLines) / 32, 0);
    for (auto &p : h.pats)
    {
        set_class_grams(h.X20, ClsLayout::Plain, p, p.size());
        set_class_grams(h.X19, ClsLayout::Plain19, p, p.size());
    }
    // stride-2 table (the slot layout of the stride-2 kernel without -c, ac_pair_slot): final gram (match ends at the tested
    // position) + the gram one byte earlier (the match ends one later: its last byte is not part of the tested gram, one class
    // fewer is known)
    if (t->has1)
        return;
    h.S20.assign(h.X20.size(), 0);
    h.S19.assign(h.X19.size(), 0);
    for (auto &p : h.pats)
        for (size_t end : {p.size(), p.size() - 1})
        {
            set_class_grams(h.S20, ClsLayout::Pair, p, end);
            set_class_grams(h.S19, ClsLayout::Pair19, p, end);
        }
    u64 e1 = 0, e2 = 0;
    for (size_t w = 0; w < h.X20.size(); ++w)
    {
        e1 += (u64)__builtin_popcount(h.X20[w]);
        e2 += (u64)__builtin_popcount(h.S20[w]);
    }
    // worth it while the denser table keeps the candidate volume in the same range (per byte e2 / 2^21 against
    // e1 / 2^20, two ends to verify per candidate) or small in absolute terms (<= 0.4 % of the even positions,
    // the rate of BASELINE config 4).  KREP_GPU_AC_STRIDE1=1 forces the one-position filter.
    const bool force2 = getenv("KREP_GPU_AC_STRIDE2") != nullptr; // (measurement hook: the stride-2 filter whatever its density)
    h.stride2 = (((e2 <= 6 * e1 + 64 || e2 <= 4096) && e2 < (1u << kXBitsBig) / 64) || force2) && !getenv("KREP_GPU_AC_STRIDE1");
}

// a failed HIP call: fail(...) and 2
template <class T> int upload(T *&d, const std::vector<T> &v)
{
    HIPCHK(hipMalloc(&d, v.size() * sizeof(T)));
    HIPCHK(hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return 0;
}

int upload_tables(AcTables *t, const AcHost &h)
{
    return upload(t->d_gram4, h.g4) || upload(t->d_g4x, h.g4x) || upload(t->d_filterx20, h.X20) || upload(t->d_filterx19, h.X19) ||
           (h.stride2 && (upload(t->d_filters20, h.S20) || upload(t->d_filters19, h.S19))) || (!h.S1.empty() && upload(t->d_s1, h.S1)) ||
           (!h.S2.empty() && upload(t->d_s2, h.S2)) || (!h.S3.empty() && upload(t->d_s3, h.S3)) || upload(t->d_edges, h.tab) ||
           upload(t->d_copies, h.copies);
}

} // namespace

AcTables *ac_build(const search_params_t &sp, int device)
{
    auto *t = new AcTables();
    t->device = device;
    t->ci = !sp.case_sensitive;
    t->npat = (u32)sp.num_patterns;
    AcHost h;
    if (!fold_patterns(sp, t, h))
    {
        delete t;
        return nullptr;
    }
    short_bitmaps(t, h);
    tiny_description(t, h.pats);
    if (!reversed_trie(t, h))
    {
        delete t;
        return nullptr;
    }
    gram4_entries(t, h);
    gram4_buckets(t, h);
    filter_tables(t, h);
    if (upload_tables(t, h))
    {
        ac_free(t);
        return nullptr;
    }
    return t;
}

void ac_free(AcTables *t)
{
    if (!t)
        return;
    (void)hipSetDevice(t->device);
    if (t->d_redo) (void)hipFree(t->d_redo);
    if (t->d_s1) (void)hipFree(t->d_s1);
    if (t->d_s2) (void)hipFree(t->d_s2);
    if (t->d_s3) (void)hipFree(t->d_s3);
    if (t->d_filterx20) (void)hipFree(t->d_filterx20);
    if (t->d_filterx19) (void)hipFree(t->d_filterx19);
    if (t->d_filters20) (void)hipFree(t->d_filters20);
    if (t->d_filters19) (void)hipFree(t->d_filters19);
    if (t->d_edges) (void)hipFree(t->d_edges);
    if (t->d_copies) (void)hipFree(t->d_copies);
    if (t->d_gram4) (void)hipFree(t->d_gram4);
    if (t->d_g4x) (void)hipFree(t->d_g4x);
    ac_anchor_free(t);
    delete t;
}

} // namespace kg
