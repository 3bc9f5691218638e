// kg_ac_anchor.hip — anchor grams chosen by rarity for the multi-pattern scan (round 6).
//
// Why.  aho_corasick_search (/root/reference/aho_corasick.c:328-437) walks an automaton and costs the same on every text.  Its
// replacement (kg_ac.hip) is a 4-gram class filter + exact verify whose cost follows the CANDIDATE rate, and until round 5 the
// filter always keyed on a pattern's LAST five bytes.  On i.i.d. letters every gram is equally rare (0.5 % of the tested positions
// for BASELINE config 4).  On word-like text with a word dictionary the last grams are the language's suffixes (`tion`, `ness`,
// `ings` ...): 14 % of the tested positions were candidates and the 1000-pattern scan ran at 0.04 of the HBM roofline where the
// i.i.d. text ran at 0.69 (profiles/r06_wordtext.txt, VERDICT r05 missing #2).
//
// What.  On the first text of >= 1 MiB that a dictionary scans, a 4-gram CLASS histogram of a 4-MiB sample of that text is taken
// on the device (2^20 bins, the filter's own index space).  Per pattern the 5-byte window P[L-5-k .. L-k) whose two class grams are
// rarest in the sample becomes its ANCHOR (k <= 12 bytes before its end; a pattern moves off its end only for a 4x rarer window,
// so a dictionary on i.i.d. text keeps k = 0 everywhere and the round-5 kernel, bit for bit).  When the estimated candidate rate
// drops enough, EVERY pattern takes its rarest window and the dictionary gets a second filter table (pair layout, 2^20 bits) and a
// table {exact anchor gram -> mask of offsets k}; the scan kernel's ANCH instantiation marks the END pairs its candidates name and
// verifies the marked pairs with the end-anchored verifier it always had.  The anchors only decide WHICH ends are looked at: a
// superset filter, results unchanged.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <unordered_map>
#include <vector>

#include "../../include/krep_gpu.h"
#include "kg_ac_common.h"
#include "kg_ac_tables.h"
#include "kg_device.h"
#include "kg_internal.h"

namespace kg {

constexpr u32 kHistBins = 1u << kXBitsBig;
constexpr u32 kHistChunk = 64u * 1024u, kHistChunks = 64u; // the sample: 64 chunks of 64 KiB spread evenly over the owned window

// one workgroup per chunk; bin = the class gram of the four bytes AT p .. p + 3 (ac_cls4: first byte lowest)
__global__ __launch_bounds__(256) void ac_gram_hist_kernel(const uint8_t *text, u64 lo, u64 span, u32 nchunks, u32 chunk_bytes, u32 *hist)
{
    const u64 c = blockIdx.x;
    u64 base = lo + (nchunks > 1 ? (span - chunk_bytes) / (nchunks - 1) * c : 0ull);
    for (u32 p = threadIdx.x; p + 4u <= chunk_bytes; p += blockDim.x)
        atomicAdd(&hist[ac_cls4(load_unaligned<u32>(text + base + p))], 1u);
}

// how often do the given five-class grams (sorted keys, c(b0) | c(b1) << 5 | ... | c(b4) << 20) occur in the same sample?
__global__ __launch_bounds__(256) void ac_gram5_count_kernel(const uint8_t *text, u64 lo, u64 span, u32 nchunks, u32 chunk_bytes, const u32 *keys,
                                                             u32 nkeys, u32 *counts)
{
    const u64 c = blockIdx.x;
    const u64 base = lo + (nchunks > 1 ? (span - chunk_bytes) / (nchunks - 1) * c : 0ull);
    for (u32 p = threadIdx.x; p + 5u <= chunk_bytes; p += blockDim.x)
    {
        const u32 key = ac_cls4(load_unaligned<u32>(text + base + p)) | (((u32)text[base + p + 4] & 31u) << 20);
        u32 a = 0, b = nkeys; // lower bound
        while (a < b)
        {
            const u32 m = (a + b) >> 1;
            if (keys[m] < key)
                a = m + 1;
            else
                b = m;
        }
        if (a < nkeys && keys[a] == key)
            atomicAdd(&counts[a], 1u);
    }
}

void ac_anchor_free(AcTables *t)
{
    if (t->d_filtera20) (void)hipFree(t->d_filtera20);
    if (t->d_anch) (void)hipFree(t->d_anch);
    if (t->d_xlen) (void)hipFree(t->d_xlen);
    if (t->d_xtab) (void)hipFree(t->d_xtab);
    t->d_filtera20 = nullptr;
    t->d_anch = nullptr;
    t->d_xlen = nullptr;
    t->d_xtab = nullptr;
}

namespace {

using Pats = std::vector<std::vector<uint8_t>>;

inline u32 load4(const uint8_t *g) { return (u32)g[0] | ((u32)g[1] << 8) | ((u32)g[2] << 16) | ((u32)g[3] << 24); } // first byte lowest

// two host tables to the device: malloc, malloc, copy, copy, sync; false: a HIP call failed (the caller frees what was allocated)
template <class A, class B> bool upload_pair(A *&da, const std::vector<A> &a, B *&db, const std::vector<B> &b, hipStream_t st)
{
    return hipMalloc(&da, a.size() * sizeof(A)) == hipSuccess && hipMalloc(&db, b.size() * sizeof(B)) == hipSuccess &&
           hipMemcpyAsync(da, a.data(), a.size() * sizeof(A), hipMemcpyHostToDevice, st) == hipSuccess &&
           hipMemcpyAsync(db, b.data(), b.size() * sizeof(B), hipMemcpyHostToDevice, st) == hipSuccess && hipStreamSynchronize(st) == hipSuccess;
}

// The length-keyed exact dictionary (kg_ac_common.h ac_exact_end) of a dictionary whose patterns all have 4..16 bytes: what answers an end
// where the chain-compressed entries cannot (the reversed trie branches behind the final gram) — stage 3 of the anchored scan, and the
// slow path of every other instantiation.  Built for texts on which the end grams are frequent (a word-like text and dictionary).
struct ExactDict
{
    std::vector<unsigned short> xlen = std::vector<unsigned short>(2 * 65536, 0); // [0]: lengths 4..7 by the last four bytes, [1]: 8..16 by the last eight
    std::vector<uint4> xt;                                                         // two-way buckets of {the 16 bytes, {length, copies}}
    u32 nb = 0, mul = 0;                                                           // nb == 0: no layout fits
};
ExactDict exact_table(const Pats &pats)
{
    // A pattern of MORE than 16 bytes (a phrase in a word list) is entered by its last 16 bytes as a 16-byte entry with copies = 2: an
    // end that matches it comes back `multi`, and the caller's level walk — which knows every length — answers that end; such ends are
    // as rare as the phrase.  (Until this was done ONE long pattern switched the exact dictionary off for the whole dictionary: 1000
    // words + one 20-byte phrase on word text ran at 15.4 ms per 32 GiB against 7.8.)
    struct X { u32 w[4]; u32 len, copies; };
    std::vector<X> xs;
    ExactDict d;
    for (auto &p : pats)
    {
        X x{};
        uint8_t b[16] = {0};
        const size_t keep = std::min<size_t>(p.size(), 16);
        memcpy(b + (16 - keep), p.data() + (p.size() - keep), keep);
        for (int w = 0; w < 4; ++w)
            x.w[w] = load4(b + 4 * w);
        x.len = (u32)keep;
        x.copies = p.size() > 16 ? 2u : 1u;
        auto same = std::find_if(xs.begin(), xs.end(), [&](const X &y) { return y.len == x.len && !memcmp(y.w, x.w, sizeof x.w); });
        if (same != xs.end())
            ++same->copies;
        else
            xs.push_back(x);
        if (x.len < 8)
            d.xlen[ac_xlen_slot(x.w[3])] |= (unsigned short)(1u << (x.len - 4));
        else
            d.xlen[65536u + ac_xlen_slot8(x.w[2], x.w[3])] |= (unsigned short)(1u << (x.len - 4));
    }
    const TwoWayFit f = fit_two_way(xs.size(), 1u << 18, kExactMuls, [&](size_t i, u32 mul) {
        const X &x = xs[i];
        return ac_xhash(x.w[0], x.w[1], x.w[2], x.w[3], x.len, mul);
    });
    if (!f.nb)
        return d;
    d.xt.assign(4 * (size_t)f.nb, make_uint4(0u, 0u, 0u, 0u));
    for (size_t i = 0; i < xs.size(); ++i)
    {
        d.xt[2 * (size_t)f.slot[i]] = make_uint4(xs[i].w[0], xs[i].w[1], xs[i].w[2], xs[i].w[3]);
        d.xt[2 * (size_t)f.slot[i] + 1] = make_uint4(xs[i].len, xs[i].copies, 0u, 0u);
    }
    d.nb = f.nb;
    d.mul = f.mul;
    return d;
}

void build_exact_dictionary(AcTables *t, hipStream_t st)
{
    if (t->d_xtab || getenv("KREP_GPU_AC_NO_EXACT") || t->lmin < 4)
        return;
    const ExactDict d = exact_table(t->pats_h);
    if (d.nb && upload_pair(t->d_xlen, d.xlen, t->d_xtab, d.xt, st))
    {
        t->xmask = d.nb - 1;
        t->xmul = d.mul;
        return;
    }
    (void)hipGetLastError();
    if (t->d_xlen) (void)hipFree(t->d_xlen);
    if (t->d_xtab) (void)hipFree(t->d_xtab);
    t->d_xlen = nullptr;
    t->d_xtab = nullptr; // (stage 3 then walks the trie as before)
}

// the sample: 64 chunks of 64 KiB spread evenly over the owned window
struct Sample
{
    const uint8_t *text;
    u64 lo, span;
    u32 chunk, nchunks;
    hipStream_t st;
    double positions() const { return (double)nchunks * (double)(chunk - 3u); }
};

// One sampling launch: the histogram of the sample's class grams (keys == nullptr) or the counts of the sorted five-class keys, into
// `out`; false: a HIP call failed (its error is left for the caller)
bool sample_counts(const Sample &s, const std::vector<u32> *keys, std::vector<u32> &out)
{
    u32 *d_k = nullptr, *d_out = nullptr;
    const size_t kbytes = keys ? keys->size() * sizeof(u32) : 0, obytes = out.size() * sizeof(u32);
    bool ok = (!keys || hipMalloc(&d_k, kbytes) == hipSuccess) && hipMalloc(&d_out, obytes) == hipSuccess &&
              (!keys || hipMemcpyAsync(d_k, keys->data(), kbytes, hipMemcpyHostToDevice, s.st) == hipSuccess) &&
              hipMemsetAsync(d_out, 0, obytes, s.st) == hipSuccess;
    if (ok)
    {
        if (keys)
            hipLaunchKernelGGL(ac_gram5_count_kernel, dim3(s.nchunks), dim3(256), 0, s.st, s.text, s.lo, s.span, s.nchunks, s.chunk, d_k, (u32)keys->size(), d_out);
        else
            hipLaunchKernelGGL(ac_gram_hist_kernel, dim3(s.nchunks), dim3(256), 0, s.st, s.text, s.lo, s.span, s.nchunks, s.chunk, d_out);
        ok = hipGetLastError() == hipSuccess && hipMemcpyAsync(out.data(), d_out, obytes, hipMemcpyDeviceToHost, s.st) == hipSuccess &&
             hipStreamSynchronize(s.st) == hipSuccess;
    }
    if (d_k) (void)hipFree(d_k);
    if (d_out) (void)hipFree(d_out);
    return ok;
}

// occurrences in the sample of the class gram of the four pattern bytes in front of `end`; end == 3: one byte sticks out in front of
// the pattern, every class there
u64 gram_count(const std::vector<u32> &hist, const std::vector<uint8_t> &p, size_t end)
{
    if (end >= 4)
        return hist[ac_cls4(load4(p.data() + end - 4))];
    u64 s = 0;
    const u32 known = (((u32)p[0] & 31u) << 5) | (((u32)p[1] & 31u) << 10) | (((u32)p[2] & 31u) << 15);
    for (u32 c0 = 0; c0 < 32; ++c0)
        s += hist[known | c0];
    return s;
}

// ---- per pattern: the rarest 5-byte window ----
// cost of offset k = occurrences in the sample of the window's two class grams — A = P[L-4-k .. L-k), the one the exact table is
// keyed by, and B = P[L-5-k .. L-1-k), the same one byte earlier (tested positions are odd: one of the two lies on one) — plus a
// prior, so that sampling noise between grams the sample hardly holds moves nothing (8 expected on i.i.d. letters)
struct Offsets
{
    std::vector<u32> ks, kfree; // the moves no sampling noise explains (what the DECISION rests on); the plain minimum
    u32 moved = 0;              // patterns with ks != 0
};
Offsets anchor_offsets(const Pats &pats, const std::vector<u32> &hist, bool force)
{
    Offsets o{std::vector<u32>(pats.size(), 0), std::vector<u32>(pats.size(), 0)};
    for (size_t i = 0; i < pats.size(); ++i)
    {
        const auto &p = pats[i];
        const size_t L = p.size(), kmax = std::min<size_t>(L - 4, kAnchMaxK);
        u64 best = ~0ull, c0 = 0;
        u32 bk = 0;
        for (size_t k = 0; k <= kmax; ++k)
        {
            const u64 c = gram_count(hist, p, L - k) + gram_count(hist, p, L - k - 1) + 16;
            if (k == 0)
                c0 = c;
            if (c < best)
            {
                best = c;
                bk = (u32)k;
            }
        }
        o.kfree[i] = bk;
        if (bk && (force || best * 4 < c0))
        {
            o.ks[i] = bk;
            ++o.moved;
        }
    }
    return o;
}

u32 count_moved(const std::vector<u32> &kk) { return (u32)std::count_if(kk.begin(), kk.end(), [](u32 k) { return k != 0; }); }

// ---- the two tables: the pair-layout class table of the anchor windows and {exact anchor gram -> offset mask + the bytes in front}.
// Rebuilt into the same object on purpose: clear() keeps the map's bucket count, which with the insert order decides the order the
// anchor buckets are filled in.
struct Anchor { u32 kmask = 0, ctx = 0, cmask = 0xffffffu; bool first = true; };
struct AnchorTables
{
    std::vector<u32> T20 = std::vector<u32>(kHistBins / 32, 0);
    std::unordered_map<u32, Anchor> keys; // exact anchor gram (text order, first byte lowest) -> offset mask + the bytes in front
};
void anchor_tables(AnchorTables &a, const Pats &pats, const std::vector<u32> &kk, bool five)
{
    std::fill(a.T20.begin(), a.T20.end(), 0u);
    a.keys.clear();
    for (size_t i = 0; i < pats.size(); ++i)
    {
        const auto &p = pats[i];
        const size_t L = p.size(), k = kk[i];
        // the window's two grams; five classes (ANCH == 2): each with the class of the byte in front of it, free where the
        // pattern does not reach (32 or 1024 slots)
        set_class_grams(a.T20, five ? ClsLayout::Five : ClsLayout::Pair, p, L - k);
        set_class_grams(a.T20, five ? ClsLayout::Five : ClsLayout::Pair, p, L - k - 1);
        Anchor &an = a.keys[load4(p.data() + (L - 4 - k))];
        an.kmask |= 1u << k;
        // the three bytes in front of the 5-byte window (text order: a - 6 lowest), as far as the pattern reaches; several
        // patterns on one gram keep the bytes they agree on
        u32 cx = 0, cm = 0;
        for (int j = 0; j < 3; ++j) // byte a - 4 - j... stored at byte 2 - j
        {
            const long q = (long)L - 5 - (long)k - j;
            if (q >= 0)
            {
                cx |= (u32)p[(size_t)q] << (8 * (2 - j));
                cm |= 0xffu << (8 * (2 - j));
            }
        }
        if (an.first)
        {
            an.ctx = cx;
            an.cmask = cm;
            an.first = false;
        }
        else
        {
            u32 keep = an.cmask & cm;
            for (int b = 0; b < 3; ++b)
                if (((an.ctx ^ cx) >> (8 * b)) & 0xffu)
                    keep &= ~(0xffu << (8 * b));
            an.cmask = keep;
            an.ctx &= keep;
        }
    }
}

// estimated candidates per tested position of a table: the sample's grams that it holds
double rate_of(const std::vector<u32> &hist, const std::vector<u32> &tab, bool pair, double nsamp)
{
    u64 hits = 0;
    for (u32 x = 0; x < kHistBins; ++x)
    {
        if (!hist[x])
            continue;
        u32 dw = x >> 5, bit = x & 31;
        if (pair)
            ac_pair_slot(x, dw, bit);
        if ((tab[dw] >> bit) & 1u)
            hits += hist[x];
    }
    return (double)hits / nsamp;
}

// ---- the four-class decision: the rates of the end grams and of the anchors; true: anchored
bool four_class_decision(AcTables *t, const std::vector<u32> &hist, double nsamp, const Offsets &o, bool force, AnchorTables &a)
{
    std::vector<u32> E20(kHistBins / 32, 0);
    for (auto &p : t->pats_h)
    {
        set_class_grams(E20, ClsLayout::Plain, p, p.size());
        set_class_grams(E20, ClsLayout::Plain, p, p.size() - 1);
    }
    anchor_tables(a, t->pats_h, o.ks, false);
    t->anch_rate0 = rate_of(hist, E20, false, nsamp);
    t->anch_rate = rate_of(hist, a.T20, true, nsamp);
    // worth a second stage: at least a third fewer candidates with the noise-proof moves alone, and a rate that matters to begin with
    const bool go = force || (o.moved && t->anch_rate0 > 0.008 && t->anch_rate < 0.66 * t->anch_rate0);
    if (go && !force)
    {
        // ... then every pattern takes its rarest window (a choice among windows the sample hardly holds costs nothing if it is noise)
        anchor_tables(a, t->pats_h, o.kfree, false);
        t->anch_rate = rate_of(hist, a.T20, true, nsamp);
        t->anch_moved = count_moved(o.kfree);
    }
    if (getenv("KREP_GPU_DEBUG"))
        fprintf(stderr, "krep-gpu: anchors: %u of %zu patterns off their end (%u beyond sampling noise); candidates per tested position %.4f %% (end grams) -> %.4f %% (anchors), %zu anchor grams: %s\n",
                t->anch_moved, t->pats_h.size(), o.moved, 100.0 * t->anch_rate0, 100.0 * t->anch_rate, a.keys.size(), go ? "anchored" : "end grams kept");
    return go;
}

// ---- five classes per lookup?  A 6-byte window of a word is several times rarer than its rarest 5-byte one (word text, 1000 rare
// words: 0.37 % against 2.6 % of the tested positions), at two more VALU per tested position.  Windows that reach in front of a
// pattern leave classes free (a 4-byte pattern: 32 + 1024 slots), so this is for dictionaries (almost) without 4- and 5-byte patterns.
// The five-class grams of every window are counted in the sample on the device; per pattern the window whose two grams are rarest,
// and the sum of their counts.  -> the windows counted; 0: nothing to count, or a HIP call failed (its error cleared).
size_t five_class_offsets(const Pats &pats, const Sample &s, const std::vector<u32> &hist, std::vector<u32> &k5, u64 &sum5)
{
    auto key5 = [](const uint8_t *g) { return ac_cls4(load4(g)) | (((u32)g[4] & 31u) << 20); };
    std::vector<u32> K;
    for (auto &p : pats)
        for (size_t k = 0, L = p.size(), kmax = std::min<size_t>(L - 4, kAnchMaxK); k <= kmax; ++k)
            for (size_t end : {L - k, L - k - 1})
                if (end >= 5)
                    K.push_back(key5(p.data() + (end - 5)));
    std::sort(K.begin(), K.end());
    K.erase(std::unique(K.begin(), K.end()), K.end());
    std::vector<u32> cnt5(K.size(), 0);
    if (K.empty() || !sample_counts(s, &K, cnt5))
    {
        (void)hipGetLastError();
        return 0;
    }
    auto count5 = [&](const std::vector<uint8_t> &p, size_t end) -> u64 { // the gram in front of end with the byte in front of it
        if (end >= 5)
            return cnt5[(size_t)(std::lower_bound(K.begin(), K.end(), key5(p.data() + (end - 5))) - K.begin())];
        return gram_count(hist, p, end); // the byte(s) in front lie outside the pattern: any class — the 4- (3-) gram's own count
    };
    k5.assign(pats.size(), 0);
    sum5 = 0;
    for (size_t i = 0; i < pats.size(); ++i)
    {
        const size_t L = pats[i].size(), kmax = std::min<size_t>(L - 4, kAnchMaxK);
        u64 best = ~0ull;
        for (size_t k = 0; k <= kmax; ++k)
        {
            const u64 c = count5(pats[i], L - k) + count5(pats[i], L - k - 1);
            if (c < best)
            {
                best = c;
                k5[i] = (u32)k;
            }
        }
        sum5 += best;
    }
    return K.size();
}

// ... and the decision: taken when it cuts the rate by 40 % with few table slots (the tables stay five-class), else the four-class
// tables are rebuilt; -> the new `go`
bool five_class_decision(AcTables *t, const Sample &s, const std::vector<u32> &hist, const Offsets &o, bool force, bool go, AnchorTables &a)
{
    std::vector<u32> k5;
    u64 sum5 = 0;
    const size_t windows = getenv("KREP_GPU_AC_NO_ANCHOR5") ? 0 : five_class_offsets(t->pats_h, s, hist, k5, sum5);
    if (!windows)
        return go;
    const double rate4 = go ? t->anch_rate : t->anch_rate0; // (what the scan would run with otherwise)
    anchor_tables(a, t->pats_h, k5, true);
    u64 slots = 0;
    for (u32 w : a.T20)
        slots += (u64)__builtin_popcount(w);
    // what the sample holds of the chosen windows + what a random 5-gram finds set by chance
    const double rate5 = (double)sum5 / s.positions() + (double)slots / (double)kHistBins;
    const bool five = slots <= 16384 && rate5 < 0.6 * rate4;
    if (getenv("KREP_GPU_DEBUG"))
        fprintf(stderr, "krep-gpu: anchors, five classes: %zu windows counted, %llu table slots, candidates per tested position %.4f %% (four classes: %.4f %%): %s\n",
                windows, (unsigned long long)slots, 100.0 * rate5, 100.0 * rate4, five ? "taken" : "not taken");
    if (!five && !getenv("KREP_GPU_AC_ANCHOR5"))
    {
        anchor_tables(a, t->pats_h, force ? o.ks : o.kfree, false); // (back to the four-class tables)
        return go;
    }
    t->anch_five = 1;
    t->anch_rate = rate5;
    t->anch_moved = count_moved(k5);
    return true;
}

// ---- buckets of two 16-byte entries {key, 1 << 31 | offset mask, bytes in front, their mask}: no bucket overfull, one 32-byte probe;
// empty when no layout fits
std::vector<uint4> anchor_buckets(const AnchorTables &a, u32 &nb, u32 &mul)
{
    std::vector<const std::pair<const u32, Anchor> *> items; // in the map's order
    for (auto &kv : a.keys)
        items.push_back(&kv);
    const TwoWayFit f = fit_two_way(items.size(), 1u << 20, kBucketMuls, [&](size_t i, u32 m) { return (items[i]->first * m) >> 9; });
    std::vector<uint4> bk(2 * (size_t)f.nb, make_uint4(0u, 0u, 0u, 0u));
    for (size_t i = 0; i < f.slot.size(); ++i)
    {
        const Anchor &an = items[i]->second;
        bk[f.slot[i]] = make_uint4(items[i]->first, an.kmask | 0x80000000u, an.ctx & an.cmask, an.cmask);
    }
    nb = f.nb;
    mul = f.mul;
    return bk;
}

} // namespace

// -> 0 (anch_state settled to 1 or 2), 2 on a HIP error (anch_state 1: the scan goes on with the end grams)
int ac_anchor_prepare(AcTables *t, const uint8_t *d_text, size_t text_len, size_t own_lo, size_t own_hi, hipStream_t st)
{
    t->anch_state = 1;
    // (a repeated decision — kg_ac.hip ac_scan, when a later text's measured candidates contradict this one's estimate — drops the
    //  anchor tables of the text before; the exact dictionary is the patterns' alone and stays)
    if (t->d_filtera20) (void)hipFree(t->d_filtera20);
    if (t->d_anch) (void)hipFree(t->d_anch);
    t->d_filtera20 = nullptr;
    t->d_anch = nullptr;
    t->anch_five = 0;
    const bool force = getenv("KREP_GPU_AC_ANCHOR") != nullptr; // test hook: anchors by plain minimum, whatever the gain
    if (getenv("KREP_GPU_AC_NO_ANCHOR") || !t->d_filters20 || t->has1 || t->has2 || t->has3 || t->tiny.ok || t->pats_h.empty())
        return 0;
    own_hi = std::min(own_hi, text_len);
    if (own_hi <= own_lo || own_hi - own_lo < 4096)
        return 0;
    const u64 span = own_hi - own_lo;
    const u32 chunk = (u32)std::min<u64>(kHistChunk, span), nchunks = (u32)std::min<u64>(kHistChunks, std::max<u64>(1, span / chunk));
    const Sample s{d_text, (u64)own_lo, span, chunk, nchunks, st};
    std::vector<u32> hist(kHistBins);
    if (!sample_counts(s, nullptr, hist))
        return 2;
    const Offsets o = anchor_offsets(t->pats_h, hist, force); // (every pattern has >= 4 bytes: has1..3 excluded above)
    t->anch_moved = o.moved;
    AnchorTables a;
    bool go = four_class_decision(t, hist, s.positions(), o, force, a);
    const bool wordy = t->anch_rate0 > 0.008; // the end grams are frequent in this text: structure, not chance
    if (!go && !wordy)
        return 0;
    go = five_class_decision(t, s, hist, o, force, go, a);
    if (!go)
    {
        build_exact_dictionary(t, st); // (the end grams stay, but their slow path need not walk the trie)
        return 0;
    }
    u32 nb = 0, mul = 0;
    const std::vector<uint4> bk = anchor_buckets(a, nb, mul);
    if (!nb)
        return 0;
    if (!upload_pair(t->d_filtera20, a.T20, t->d_anch, bk, st))
    {
        ac_anchor_free(t);
        return 2;
    }
    t->anch_mask = nb - 1;
    t->anch_mul = mul;
    t->anch_state = 2;
    // (an anchored scan parks nothing — the END bitmap has the park area — so the 64-entry staging slot costs it nothing, and a word
    //  dictionary's matches cluster: with 16 entries the FIRST scan of `uniform` re-scanned its overflowed units, 34.7 ms against 11.7)
    t->stage_cap = std::max<u32>(t->stage_cap, 64u);
    build_exact_dictionary(t, st);
    return 0;
}

} // namespace kg
