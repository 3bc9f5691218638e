// kg_exec.hip — the executor that brings a host buffer through HBM (kg::host_scan, behind the operators of kg_ops.hip):
//   * ONE PIECE (the whole text staged, then scanned) for small inputs and for the three input classes that need the whole
//     text in one window (kg::split_mode() == whole);
//   * PIECES otherwise — contiguous chunks with start-offset ownership and Lmax+1 bytes of halo, spread over the requested
//     devices (search_buffer(num_gpus > 1), the operators with cfg.num_gpus > 1: the reference's chunk loop,
//     krep.c:2816-2905, without its double counting; the shards' counters meet in ONE RCCL all-reduce, kg_comm.hip) and, per
//     device, STREAMED: piece k+1 is copied through the pinned staging ring (mmap'd / pageable source -> pinned -> DMA) while
//     piece k is scanned, two device buffers per device, so a haystack larger than HBM works and the scan time hides under
//     the PCIe time (the reference's counterpart is mmap + MAP_POPULATE, krep.c:2630-2726).  The sequential
//     match-set families run as CHAINED pieces: each takes the boundary record of the one before it (krep_gpu_seq_carry_t).
// Every device has ONE context (buffers, staging ring, a small plan cache) behind a mutex: the operators are re-entrant
// from any number of threads (SURVEY §8b "Threading", krep.c:1950), calls on one device serialise.
#include <hip/hip_runtime.h>
#include <pthread.h>
#include <sched.h>
#include <cctype>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/krep_gpu.h"
#include "kg_common.h"
#include "kg_internal.h"
#include "kg_plan.h"

using namespace kg;

namespace {
thread_local krep_gpu_shard_info_t tl_shards{1, 1, {0}, 0, 0}; // krep_gpu_last_shard_info()
// ---------------------------------------------------------------------------------------------- device buffers
struct OwnedBuf
{
    uint8_t *p = nullptr;
    size_t cap = 0;
    int dev = -1;
    int ensure(size_t n, int device)
    {
        if (dev == device && cap >= n && p)
            return 0;
        release();
        HIPCHK(hipSetDevice(device));
        const size_t want = std::max<size_t>(n, 1 << 20);
        if (kg::inject(1))
            return kg::fail("injected failure: device allocation of %zu bytes", want);
        if (hipMalloc(&p, want) != hipSuccess)
        {
            p = nullptr;
            (void)hipGetLastError();
            return kg::fail("hipMalloc of %zu bytes failed on device %d", want, device);
        }
        cap = want;
        dev = device;
        return 0;
    }
    void release()
    {
        if (p)
        {
            (void)hipSetDevice(dev);
            (void)hipFree(p);
        }
        p = nullptr;
        cap = 0;
        dev = -1;
    }
};

// ONE allocation per device for the host path: the text buffer(s) and, right behind them, the record buffer.  Where the driver
// places a buffer physically moves the offsets-producing scans by several per cent, and freeing / re-allocating buffers between
// calls is what churns that placement (profiles/r03_box_to_box.txt: the record buffer re-allocated inside one
// process draws 6.58 ... 7.42 ms for the single-byte workload).  Round 3 kept that discipline in bench.py only; here the CLI
// and every host-buffer caller get it: the arena grows (rarely: 1.5x steps), it is never freed and re-made per call, and the
// record area always sits behind the text.  A list that outgrows its area (a second, exact-size pass) takes a buffer of its
// own for that call: the staged text must not move.
struct Arena
{
    uint8_t *base = nullptr;
    size_t cap = 0, text_each = 0, pos_bytes = 0;
    int ntext = 0, dev = -1;
    OwnedBuf pos_extra; // only while a record list does not fit pos_bytes
    static size_t pos_for(size_t text_bytes) { return std::max<size_t>((size_t)1 << 20, text_bytes / 4 + 4096); } // 16 B per 64 B of text
    // `count` text buffers of `each` bytes (64-byte multiples) + the record area: keeps what is there when it is large enough
    int ensure(size_t each, int count, int device)
    {
        each = (each + 255) & ~(size_t)255;
        if (base && dev == device && ntext >= count && text_each >= each)
            return 0;
        const int n = std::max(count, ntext);
        size_t want_each = std::max(each, text_each);
        if (base && dev == device)
            want_each = std::max(want_each, text_each + text_each / 2); // grow in steps: a run of growing files re-allocates log times
        const size_t want_pos = pos_for(want_each), total = (size_t)n * want_each + want_pos;
        release();
        HIPCHK(hipSetDevice(device));
        if (kg::inject(1))
            return kg::fail("injected failure: device allocation of %zu bytes", total);
        // $KREP_GPU_PLACE_TRIES=k (2..8): an arena of >= 4 GiB is drawn for (kg_place.hip krep_gpu_alloc_placed: up to k candidates, the
        // single-byte workload timed on each, the fastest kept).  Off by default: the host path stages its text over PCIe at <= 55 GB/s, next
        // to which the 2-10 % of a scan that placement moves are not visible, and every draw costs an allocation + ~50 ms of probe scans.
        static const int place_tries = [] { const char *e = getenv("KREP_GPU_PLACE_TRIES"); return e ? atoi(e) : 1; }();
        if (place_tries > 1 && total >= ((size_t)4 << 30))
        {
            void *t = nullptr, *r = nullptr;
            // (the arena's layout: n text buffers in a row, the record area behind them — the probe treats the row as one text)
            if (krep_gpu_alloc_placed(device, (size_t)n * want_each - 64, want_pos, place_tries, &t, &r, nullptr) == 0)
            {
                base = (uint8_t *)t;
                cap = total;
                ntext = n;
                text_each = want_each;
                pos_bytes = want_pos;
                dev = device;
                return 0;
            }
            krep_gpu_clear_error(); // (the plain allocation below is tried before anything is reported)
        }
        if (hipMalloc(&base, total) != hipSuccess)
        {
            base = nullptr;
            (void)hipGetLastError();
            // not enough room for the growth step: exactly what was asked for
            want_each = each;
            const size_t exact = (size_t)count * each + pos_for(each);
            if (hipMalloc(&base, exact) != hipSuccess)
            {
                base = nullptr;
                (void)hipGetLastError();
                return kg::fail("hipMalloc of %zu bytes failed on device %d", exact, device);
            }
            cap = exact;
            ntext = count;
            text_each = each;
            pos_bytes = pos_for(each);
            dev = device;
            return 0;
        }
        cap = total;
        ntext = n;
        text_each = want_each;
        pos_bytes = want_pos;
        dev = device;
        return 0;
    }
    uint8_t *text(int i) const { return base + (size_t)i * text_each; }
    // the record area for `bytes` of records: behind the text when it fits, a buffer of its own otherwise
    uint8_t *pos(size_t bytes, int device)
    {
        if (base && bytes <= pos_bytes)
            return base + (size_t)ntext * text_each;
        return pos_extra.ensure(bytes, device) ? nullptr : pos_extra.p;
    }
    void release()
    {
        if (base)
        {
            (void)hipSetDevice(dev);
            (void)hipFree(base);
        }
        base = nullptr;
        cap = text_each = pos_bytes = 0;
        ntext = 0;
        dev = -1;
        pos_extra.release();
    }
};

// Host buffer -> HBM through two pinned staging buffers: the CPU copy of chunk k+1 overlaps the DMA of chunk k
// (a pageable hipMemcpy stages serially).  PCIe-bound by construction (<= ~55 GB/s); this rate is reported separately and
// is never the roofline number.
struct Stager
{
    static constexpr size_t kChunk = 32u << 20;
    static constexpr size_t kSlack = 1u << 20; // a tail of up to this much rides with the last full chunk: a piece's few halo bytes
                                               // as a chunk of their own would leave the CPU nothing to do while a DMA still owns
                                               // the other staging buffer (measured: one DMA time, 0.4 ms, lost per piece)
    uint8_t *pin[2] = {nullptr, nullptr};
    hipStream_t st = nullptr;
    hipEvent_t done[2] = {nullptr, nullptr};
    int dev = -1;
    bool ready = false; // every resource below exists (set last by init(); a half-built stager is torn down)
    void release()
    {
        ready = false;
        if (dev < 0)
            return;
        (void)hipSetDevice(dev);
        for (int i = 0; i < 2; ++i)
        {
            if (pin[i]) (void)hipHostFree(pin[i]);
            if (done[i]) (void)hipEventDestroy(done[i]);
            pin[i] = nullptr;
            done[i] = nullptr;
        }
        if (st) (void)hipStreamDestroy(st);
        st = nullptr;
        dev = -1;
        seq = 0;
    }
    int init(int device)
    {
        if (dev == device && ready)
            return 0;
        release();
        HIPCHK(hipSetDevice(device));
        dev = device;
        bool ok = true;
        for (int i = 0; i < 2 && ok; ++i)
            ok = hipHostMalloc(&pin[i], kChunk + kSlack) == hipSuccess &&
                 hipEventCreateWithFlags(&done[i], hipEventDisableTiming) == hipSuccess;
        ok = ok && hipStreamCreateWithFlags(&st, hipStreamNonBlocking) == hipSuccess;
        if (!ok)
        {
            (void)hipGetLastError();
            release(); // a recoverable out-of-memory must not leave NULL buffers behind for the next call
            return kg::fail("cannot create the pinned staging ring on device %d", device);
        }
        ready = true;
        return 0;
    }
    uint64_t seq = 0; // staging chunks issued so far: the ring runs on across calls (no drain between the pieces of a stream)
    // queues the whole copy on the staging stream and returns when the last CPU-side chunk copy has been handed to the DMA
    // engine; `after` (may be NULL) is recorded behind the last DMA.  The two pinned buffers alternate across calls, so
    // piece k+1's first chunk is staged while piece k's last DMA is still running.
    int copy_async(uint8_t *d_dst, const char *src, size_t len, hipEvent_t after)
    {
        if (!ready)
            return kg::fail("staging ring not initialised");
        if (kg::inject(2))
            return kg::fail("injected failure: host->device copy");
        HIPCHK(hipSetDevice(dev));
        for (size_t off = 0, n = 0; off < len; off += n, ++seq)
        {
            const int b = (int)(seq & 1);
            n = len - off <= kChunk + kSlack ? len - off : kChunk;
            if (seq >= 2)
                HIPCHK(hipEventSynchronize(done[b])); // the DMA that last used this staging buffer
            {
                // The staging copy feeds a DMA engine that takes 57.6 GB/s from pinned memory on this part
                // (tools/ubench/host_register.hip, profiles/r04_ingest.txt); one host thread copies 12-30 GB/s depending on the
                // host, so the copy is split over just enough helper threads to stay ahead of the DMA — measured once per
                // process on the first full chunk (round 3 always used 4).  Zero-copy ingest (hipHostRegister of the caller's
                // mapping, krep.c:2630-2726) was measured and is NOT used: pinning 2 GiB costs 90-106 ms, the ring moves them
                // in 39 ms.  $KREP_GPU_COPY_THREADS overrides.
                static std::atomic<int> threads{0};
                int kT = threads.load(std::memory_order_relaxed);
                if (kT == 0)
                {
                    const char *e = getenv("KREP_GPU_COPY_THREADS");
                    kT = e && *e ? std::min(8, std::max(1, atoi(e))) : 0;
                    if (kT == 0 && n >= ((size_t)8 << 20))
                    {
                        const size_t probe = (size_t)4 << 20; // (this part of the chunk is copied again below: a one-off 4 MiB)
                        const auto t0 = std::chrono::steady_clock::now();
                        memcpy(pin[b], src + off, probe);
                        const double gbps = probe / std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() / 1e9;
                        kT = std::min(4, std::max(2, (int)std::ceil(64.0 / std::max(1.0, gbps))));
                    }
                    if (kT)
                        threads.store(kT, std::memory_order_relaxed);
                    else
                        kT = 2; // a small first chunk: decide later
                }
                std::thread th[8];
                const size_t part = (n + (size_t)kT - 1) / (size_t)kT;
                for (int q = 1; q < kT; ++q)
                {
                    const size_t o = (size_t)q * part;
                    if (o < n)
                        th[q - 1] = std::thread([=] { memcpy(pin[b] + o, src + off + o, std::min(part, n - o)); });
                }
                memcpy(pin[b], src + off, std::min(part, n));
                for (auto &t : th)
                    if (t.joinable())
                        t.join();
            }
            HIPCHK(hipMemcpyAsync(d_dst + off, pin[b], n, hipMemcpyHostToDevice, st));
            HIPCHK(hipEventRecord(done[b], st));
        }
        if (after)
            HIPCHK(hipEventRecord(after, st));
        return 0;
    }
    // The same ring for bytes that are not contiguous on the host (a batch of texts packed into one, kg_batch.hip): fill(dst, off, n)
    // writes bytes [off, off + n) of the packed text into the pinned chunk; the CPU fills chunk k+1 while the DMA of chunk k runs.
    // Returns once the last DMA is done.
    template <class Fill> int gather(uint8_t *d_dst, size_t len, Fill fill)
    {
        if (!ready)
            return kg::fail("staging ring not initialised");
        if (kg::inject(2))
            return kg::fail("injected failure: host->device copy");
        HIPCHK(hipSetDevice(dev));
        for (size_t off = 0, n = 0; off < len; off += n, ++seq)
        {
            const int b = (int)(seq & 1);
            n = len - off <= kChunk + kSlack ? len - off : kChunk;
            if (seq >= 2)
                HIPCHK(hipEventSynchronize(done[b])); // the DMA that last used this staging buffer
            const size_t kT = n >= ((size_t)8 << 20) ? 4 : 1, part = (n + kT - 1) / kT; // (a large chunk: four host threads, as copy_async)
            std::thread th[3];
            for (size_t q = 1; q < kT; ++q)
                if (q * part < n)
                    th[q - 1] = std::thread([=] { fill(pin[b] + q * part, off + q * part, std::min(part, n - q * part)); });
            fill(pin[b], off, std::min(part, n));
            for (auto &t : th)
                if (t.joinable())
                    t.join();
            HIPCHK(hipMemcpyAsync(d_dst + off, pin[b], n, hipMemcpyHostToDevice, st));
            HIPCHK(hipEventRecord(done[b], st));
        }
        HIPCHK(hipStreamSynchronize(st));
        return 0;
    }
    int copy(uint8_t *d_dst, const char *src, size_t len)
    {
        if (!ready)
            return kg::fail("staging ring not initialised");
        if (kg::inject(2))
            return kg::fail("injected failure: host->device copy");
        HIPCHK(hipSetDevice(dev));
        if (len < (4u << 20)) // small buffers: one synchronous copy is cheaper than the pipeline
        {
            HIPCHK(hipMemcpy(d_dst, src, len, hipMemcpyHostToDevice));
            return 0;
        }
        if (copy_async(d_dst, src, len, nullptr))
            return 2;
        HIPCHK(hipStreamSynchronize(st));
        return 0;
    }
};

// ---------------------------------------------------------------------------------------------- plan cache
// The CLI calls the operator once per file (krep.c:1950) with the same params, and building a plan costs device
// allocations + (multi-pattern) table construction.  Keyed by every field the scan depends on, configuration included.
struct PlanKey
{
    std::vector<std::vector<uint8_t>> pats;
    bool cs = true, lines = false, track = false, ww = false, regex = false;
    size_t max_count = SIZE_MAX;
    int simd = 0, only_matching = 0, no_simd = 0, algo = 0, device = 0;
    bool operator==(const PlanKey &o) const
    {
        return pats == o.pats && cs == o.cs && lines == o.lines && track == o.track && ww == o.ww && regex == o.regex &&
               max_count == o.max_count && simd == o.simd && only_matching == o.only_matching && no_simd == o.no_simd &&
               algo == o.algo && device == o.device;
    }
};
PlanKey key_of(const search_params_t *p, const krep_gpu_config_t &c, int device)
{
    PlanKey k;
    if (p->num_patterns >= 1 && p->patterns && p->pattern_lens)
        for (size_t i = 0; i < p->num_patterns; ++i)
            k.pats.emplace_back((const uint8_t *)p->patterns[i], (const uint8_t *)p->patterns[i] + p->pattern_lens[i]);
    else if (p->pattern)
        k.pats.emplace_back((const uint8_t *)p->pattern, (const uint8_t *)p->pattern + p->pattern_len);
    k.cs = p->case_sensitive; k.lines = p->count_lines_mode; k.track = p->track_positions; k.ww = p->whole_word;
    k.regex = p->use_regex;
    k.max_count = p->max_count;
    k.simd = c.reference_simd; k.only_matching = c.only_matching; k.no_simd = c.force_no_simd; k.algo = c.algo_override;
    k.device = device;
    return k;
}

// ---------------------------------------------------------------------------------------------- per-device context
struct DeviceCtx
{
    std::mutex mu; // one host-buffer operation at a time per device
    int device = 0;
    struct Entry
    {
        PlanKey key;
        krep_gpu_plan_t *plan = nullptr;
        uint64_t tick = 0;
    };
    std::vector<Entry> plans; // small LRU
    uint64_t tick = 0;
    Arena mem; // text buffer(s) + record area, one allocation
    Stager stager;
    BatchScratch batch; // krep_gpu_search_batch: offset table, per-item results, the -c line flags (kg_batch.hip)

    krep_gpu_plan_t *plan_for(const search_params_t *p, const krep_gpu_config_t &c)
    {
        PlanKey k = key_of(p, c, device);
        for (auto &e : plans)
            if (e.key == k)
            {
                e.tick = ++tick;
                return e.plan;
            }
        krep_gpu_config_t cc = c;
        cc.device = device;
        krep_gpu_plan_t *pl = krep_gpu_plan_create_ex(p, &cc);
        if (!pl)
            return nullptr;
        constexpr size_t kMaxPlans = 4;
        if (plans.size() >= kMaxPlans)
        {
            size_t victim = 0;
            for (size_t i = 1; i < plans.size(); ++i)
                if (plans[i].tick < plans[victim].tick)
                    victim = i;
            krep_gpu_plan_destroy(plans[victim].plan);
            plans.erase(plans.begin() + (long)victim);
        }
        plans.push_back(Entry{std::move(k), pl, ++tick});
        return pl;
    }
    void release()
    {
        for (auto &e : plans)
            krep_gpu_plan_destroy(e.plan);
        plans.clear();
        mem.release();
        stager.release();
        (void)hipSetDevice(device);
        batch_scratch_free(batch);
    }
};
std::mutex g_ctx_mu;
std::vector<std::unique_ptr<DeviceCtx>> *g_ctx = nullptr; // leaked at process exit on purpose: the HIP runtime may be gone by then
DeviceCtx *ctx_for(int device)
{
    std::lock_guard<std::mutex> lk(g_ctx_mu);
    if (!g_ctx)
        g_ctx = new std::vector<std::unique_ptr<DeviceCtx>>();
    if ((size_t)device >= g_ctx->size())
        g_ctx->resize((size_t)device + 1);
    if (!(*g_ctx)[device])
    {
        (*g_ctx)[device].reset(new DeviceCtx());
        (*g_ctx)[device]->device = device;
    }
    return (*g_ctx)[device].get();
}

// memchr_search's final flush (krep.c:3976-3991 + :4026-4038): when max_count is a multiple of the 4096-entry batch and more
// matches exist, the (max_count+1)-th record is stored FIRST (in front of the last batch) and the max_count-th is dropped.
void memchr_batch_quirk(match_position_t *recs, uint64_t have, size_t maxc)
{
    if (!memchr_flush_displaces(have, maxc))
        return;
    const uint64_t f = maxc - 4096;
    match_position_t extra = recs[maxc];
    memmove(recs + f + 1, recs + f, 4095 * sizeof(match_position_t));
    recs[f] = extra;
}

// scan(d_pos, cap) with a list of `cap` records in the arena (0: no list), then once more at the exact size when `so` (what the
// scan reports) says the list overflowed; *d_pos: where the records are
template <class Scan> int sized_scan(DeviceCtx &cx, uint64_t cap, const krep_gpu_scan_out_t &so, match_position_t **d_pos, Scan scan)
{
    for (int attempt = 0;; ++attempt)
    {
        *d_pos = cap ? (match_position_t *)cx.mem.pos(cap * sizeof(match_position_t), cx.device) : nullptr;
        if ((cap && !*d_pos) || scan(*d_pos, cap))
            return 2;
        if (!so.overflow || attempt == 1)
            return 0;
        cap = so.total_matches + 1; // exact size, second and last pass
    }
}

int records_to_host(match_position_t *dst, const match_position_t *d_pos, uint64_t n)
{
    if (kg::inject(4) || hipMemcpy(dst, d_pos, n * sizeof(match_position_t), hipMemcpyDeviceToHost) != hipSuccess)
        return kg::fail("D2H copy of the records failed");
    return 0;
}

// the plan of a piece and of its chain fix-ups
krep_gpu_plan_t *piece_plan(DeviceCtx &cx, const search_params_t *params, const krep_gpu_config_t &cfg)
{
    search_params_t local = *params;
    local.max_count = SIZE_MAX; // prefix-ordered truncation happens after the pieces are merged
    return cx.plan_for(&local, cfg);
}

// ------------------------------------------------------------------------------------------------ one piece
// The whole text in one device buffer: every reference convention (max_count corners, batch quirk, sequential families,
// end-of-text replay) is applied by krep_gpu_scan_device_ex() itself.
int run_whole(DeviceCtx &cx, const search_params_t *params, const krep_gpu_config_t &cfg, const char *text, size_t text_len,
              match_result_t *result, uint64_t *ret_out)
{
    *ret_out = 0;
    krep_gpu_plan_t *pl = cx.plan_for(params, cfg);
    if (!pl)
        return 2;
    if (pl->ref_algo == KREP_RA_AHO_CORASICK && !params->ac_trie)
        return 0; // aho_corasick.c:306: no trie, no matches
    if (cx.mem.ensure(text_len + 64, 1, cx.device))
        return 2;
    uint8_t *const d_text = cx.mem.text(0);
    if (text_len && (cx.stager.init(cx.device) || cx.stager.copy(d_text, text, text_len)))
    {
        if (!kg::have_error())
            kg::fail("H2D copy failed");
        return 2;
    }
    const bool want_pos = params->track_positions && result != nullptr && !params->count_lines_mode;
    uint64_t cap = 0;
    if (want_pos)
    {
        cap = std::max<uint64_t>(1u << 16, text_len / 64);
        if (params->max_count != SIZE_MAX)
            cap = std::min<uint64_t>(cap, (uint64_t)params->max_count + 1);
        cap = std::max<uint64_t>(cap, 1);
    }
    krep_gpu_scan_out_t so;
    match_position_t *d_pos = nullptr;
    if (sized_scan(cx, cap, so, &d_pos, [&](match_position_t *d, uint64_t c) {
            return krep_gpu_scan_device_ex(pl, d_text, text_len, 0, text_len, 0, text_len, d, c, nullptr, 0, &so);
        }))
        return 2;
    *ret_out = so.count;
    if (want_pos && so.stored)
    {
        if (cfg.result_order && pl->ref_algo == KREP_RA_AHO_CORASICK &&
            krep_gpu_order_by_start(d_pos, so.stored, text_len, nullptr))
            return 2;
        std::vector<match_position_t> tmp(so.stored);
        if (records_to_host(tmp.data(), d_pos, so.stored))
            return 2;
        uint64_t n = so.stored;
        const int algo = pl->ref_algo == KREP_RA_AHO_CORASICK ? KREP_RA_AHO_CORASICK : mirror_effective(pl->ref_algo, &pl->sp, text_len);
        if (algo == KREP_RA_MEMCHR && params->max_count != SIZE_MAX)
        {
            memchr_batch_quirk(tmp.data(), n, params->max_count);
            n = std::min<uint64_t>(n, params->max_count);
            if (cfg.result_order) // the caller skips its qsort: hand the (one displaced) record back in file order
                std::sort(tmp.begin(), tmp.begin() + (long)n, by_start_end);
        }
        if (!result_reserve(result, n))
            return kg::fail("out of memory growing match_result_t");
        memcpy(result->positions + result->count, tmp.data(), n * sizeof(match_position_t));
        result->count += n;
    }
    return 0;
}

// ------------------------------------------------------------------------------------------------ pieces
std::atomic<uint64_t> g_chain_rescans{0}, g_chain_replays{0}; // chain fix-ups since the process started (test hook)
struct Piece
{
    size_t lo = 0, hi = 0; // owned window in the text
    size_t b0 = 0, b1 = 0; // bytes staged: [b0, b1) superset of [lo, hi)
    int device = 0;
    int shard = 0; // logical shard (one per requested GPU) this piece belongs to
    krep_gpu_scan_out_t out{};
    std::vector<match_position_t> recs;
    // kSplitChain: the boundary record this piece was scanned with and the one it leaves
    krep_gpu_seq_carry_t carry_used{}, carry_out{};
};
inline bool rec_less(const match_position_t &a, const match_position_t &b) // emission order of aho_corasick_search
{
    return a.end_offset != b.end_offset ? a.end_offset < b.end_offset : a.start_offset < b.start_offset;
}

// one run over pieces: what every step reads
struct PieceJob
{
    const search_params_t *params;
    krep_gpu_config_t cfg;
    const char *buf; // the text, len bytes
    size_t len;
    bool want_pos, chain; // chain: kSplitChain, pieces in text order, each with its predecessor's boundary record
    int algo, G;          // the reference function the verdict and the -m conventions follow; logical shards
};

// all pieces of one device, in text order; piece k+1 is staged by a helper thread while piece k is scanned
struct DeviceRun
{
    const PieceJob *job = nullptr;
    DeviceCtx *cx = nullptr;
    std::vector<Piece *> pieces;
    int rc = 0;
    std::string err;
};

// one piece, resident in d_text: scan (second pass with an exact buffer when the position buffer was too small), records to
// the host.  carry_in == NULL: nothing in front of the piece is consumed.
int scan_one_piece(DeviceCtx &cx, krep_gpu_plan_t *pl, const uint8_t *d_text, Piece *p, size_t global_len, bool want_pos,
                   const krep_gpu_seq_carry_t *carry_in)
{
    const size_t nb = p->b1 - p->b0;
    p->carry_used = carry_in ? *carry_in : krep_gpu_seq_carry_t{};
    p->recs.clear();
    match_position_t *d_pos = nullptr;
    if (sized_scan(cx, want_pos ? std::max<uint64_t>(1u << 16, nb / 64) : 0, p->out, &d_pos, [&](match_position_t *d, uint64_t cap) {
            return krep_gpu_scan_device_seq(pl, d_text, nb, p->lo - p->b0, p->hi - p->b0, p->b0, global_len, d, cap, nullptr, 0, carry_in,
                                            &p->carry_out, &p->out);
        }))
        return 2;
    if (!want_pos || !p->out.stored)
        return 0;
    p->recs.resize(p->out.stored);
    return records_to_host(p->recs.data(), d_pos, p->out.stored);
}

void bind_thread_near_device(int device)
{
    char bdf[32] = {0};
    if (hipDeviceGetPCIBusId(bdf, sizeof bdf, device) != hipSuccess)
    {
        (void)hipGetLastError();
        return;
    }
    for (char *c = bdf; *c; ++c)
        *c = (char)tolower(*c);
    char path[160];
    snprintf(path, sizeof path, "/sys/bus/pci/devices/%s/numa_node", bdf);
    FILE *f = fopen(path, "r");
    if (!f)
        return;
    int node = -1;
    const int got = fscanf(f, "%d", &node);
    fclose(f);
    if (got != 1 || node < 0)
        return;
    snprintf(path, sizeof path, "/sys/devices/system/node/node%d/cpulist", node);
    f = fopen(path, "r");
    if (!f)
        return;
    char list[4096] = {0};
    const bool ok = fgets(list, sizeof list, f) != nullptr;
    fclose(f);
    if (!ok)
        return;
    cpu_set_t set;
    CPU_ZERO(&set);
    int n = 0;
    for (char *tok = strtok(list, ",\n"); tok; tok = strtok(nullptr, ",\n"))
    {
        int a = 0, b = 0;
        const int k = sscanf(tok, "%d-%d", &a, &b);
        if (k == 1)
            b = a;
        if (k >= 1)
            for (int c = a; c <= b && c < CPU_SETSIZE; ++c, ++n)
                CPU_SET(c, &set);
    }
    if (n)
        (void)pthread_setaffinity_np(pthread_self(), sizeof set, &set);
}

void run_device(DeviceRun *dr)
{
    const PieceJob &job = *dr->job;
    DeviceCtx &cx = *dr->cx;
    std::lock_guard<std::mutex> lk(cx.mu);
    dr->rc = 2;
    const size_t np = dr->pieces.size();
    size_t maxb = 0;
    for (Piece *p : dr->pieces)
        maxb = std::max(maxb, p->b1 - p->b0);
    krep_gpu_plan_t *pl = piece_plan(cx, job.params, job.cfg);
    if (!pl || hipSetDevice(cx.device) != hipSuccess || cx.stager.init(cx.device) || cx.mem.ensure(maxb + 64, np > 1 ? 2 : 1, cx.device))
    {
        dr->err = krep_gpu_last_error();
        return;
    }
    // producer: queues the staging of piece k into buffer k & 1 once piece k-2 has been consumed; ready[k & 1] fires when
    // its last DMA is done.  The staging ring never drains between pieces.
    hipEvent_t ready[2] = {nullptr, nullptr};
    for (int i = 0; i < 2; ++i)
        if (hipEventCreateWithFlags(&ready[i], hipEventDisableTiming) != hipSuccess)
        {
            dr->err = "event creation failed";
            return;
        }
    std::mutex m;
    std::condition_variable cv;
    size_t staged = 0, consumed = 0;
    bool stage_failed = false, stop = false;
    std::string stage_err;
    std::thread producer([&] {
        for (size_t k = 0; k < np; ++k)
        {
            {
                std::unique_lock<std::mutex> l(m);
                cv.wait(l, [&] { return stop || k < consumed + 2; });
                if (stop)
                    return;
            }
            Piece *p = dr->pieces[k];
            const int rc = cx.stager.copy_async(cx.mem.text((int)(k & 1)), job.buf + p->b0, p->b1 - p->b0, ready[k & 1]);
            std::lock_guard<std::mutex> l(m);
            if (rc)
            {
                stage_failed = true;
                stage_err = krep_gpu_last_error(); // thread-local of the producer: hand it over
                cv.notify_all();
                return;
            }
            staged = k + 1;
            cv.notify_all();
        }
    });
    auto finish = [&](const char *err) { // err == NULL: every piece is done
        {
            std::lock_guard<std::mutex> l(m);
            stop = true;
        }
        cv.notify_all();
        producer.join();
        (void)hipStreamSynchronize(cx.stager.st);
        for (int i = 0; i < 2; ++i)
            (void)hipEventDestroy(ready[i]);
        if (err)
            dr->err = err;
        else
            dr->rc = 0;
    };
    for (size_t k = 0; k < np; ++k)
    {
        {
            std::unique_lock<std::mutex> l(m);
            cv.wait(l, [&] { return stage_failed || staged > k; });
            if (stage_failed)
            {
                const std::string e = "staging failed: " + stage_err;
                l.unlock();
                return finish(e.c_str());
            }
        }
        if (hipEventSynchronize(ready[k & 1]) != hipSuccess) // the piece's last DMA
            return finish("staging DMA failed");
        Piece *p = dr->pieces[k];
        // chain: inside a shard every piece takes its predecessor's boundary record; the FIRST piece of a shard is scanned
        // optimistically — its left neighbour is another device's work, still running — and checked by chain_fixup afterwards
        // (one rule for every layout: shards that share a device on a small box take the same road as eight devices)
        const krep_gpu_seq_carry_t *cin = nullptr;
        if (job.chain && k > 0 && dr->pieces[k - 1]->shard == p->shard)
            cin = &dr->pieces[k - 1]->carry_out;
        if (scan_one_piece(cx, pl, cx.mem.text((int)(k & 1)), p, job.len, job.want_pos, cin))
            return finish(krep_gpu_last_error());
        {
            std::lock_guard<std::mutex> l(m);
            consumed = k + 1;
        }
        cv.notify_all();
    }
    finish(nullptr);
}

constexpr size_t kChainTailPiece = 256u << 10; // the piece that holds the end of the text, chained multi-shard runs

// The pieces in text order: shard g owns the g-th share of the text, cut into `chunk`-byte pieces when streamed (0: one piece), each
// staged with ctx bytes of halo on both sides, on device (cfg.device + g) % ndev.  Arithmetic only.
std::vector<Piece> piece_layout(const PieceJob &job, size_t chunk, int ndev)
{
    const size_t len = job.len;
    size_t lmax = 1;
    for (size_t i = 0; i < job.params->num_patterns; ++i)
        lmax = std::max(lmax, job.params->pattern_lens[i]);
    if (job.params->use_regex)
    {
        lmax = std::max<size_t>(lmax, 16); // a{16} is five pattern bytes and sixteen text bytes: the halo follows L <= 16
        RegexCompiled rc;
        if (!regex_compile_cached(job.params, &rc) && rc.line_walked())
            lmax = 4096; // *, + and {n,}: a piece holds every line that meets its owned range, whole (kg_regex_loops.hip)
    }
    const size_t ctx = lmax + 1; // pattern_len-1 to complete straddling matches, +1 for -w, +1 slack
    const size_t share = (len + (size_t)job.G - 1) / (size_t)job.G;
    std::vector<Piece> pcs;
    for (int g = 0; g < job.G; ++g)
    {
        const size_t glo = std::min(len, (size_t)g * share), ghi = std::min(len, glo + share);
        if (ghi <= glo && !(len == 0 && g == 0))
            continue;
        const size_t step = chunk ? std::max<size_t>(chunk, 4096) : std::max<size_t>(ghi - glo, 1);
        size_t lo = glo;
        do
        {
            Piece p;
            p.lo = lo;
            p.hi = std::min(ghi, lo + step);
            p.b0 = p.lo > ctx ? p.lo - ctx : 0;
            p.b1 = std::min(len, p.hi + ctx);
            p.device = (job.cfg.device + g) % ndev;
            p.shard = g;
            pcs.push_back(std::move(p));
            lo += step;
        } while (lo < ghi);
    }
    if (pcs.size() >= 2 && pcs.back().hi - pcs.back().lo < 4096)
    { // a sliver at the end joins its neighbour (the piece that ends the text must hold the end-of-text replay window)
        Piece &prev = pcs[pcs.size() - 2];
        prev.hi = pcs.back().hi;
        prev.b1 = pcs.back().b1;
        pcs.pop_back();
    }
    if (job.chain && job.G > 1 && !pcs.empty() && pcs.back().hi == len && pcs.back().hi - pcs.back().lo > 2 * kChainTailPiece)
    {
        // Sequential families over several shards: the piece that ENDS the text is the only one whose result depends on the
        // line-skip history of everything in front of it (the end-of-text replay, kg_replay.h) — and every shard starts from a
        // zero record, so whenever an earlier shard held an accepted occurrence that piece is staged and scanned again (chain_fixup).
        // Its last 256 KiB become a piece of their own (same device, scanned behind its neighbour with that neighbour's record):
        // the repeat then costs 256 KiB, not a shard.
        Piece t = pcs.back();
        Piece &big = pcs.back();
        big.hi = len - kChainTailPiece;
        big.b1 = std::min(len, big.hi + ctx);
        t.lo = big.hi;
        t.b0 = t.lo > ctx ? t.lo - ctx : 0;
        pcs.push_back(std::move(t));
    }
    return pcs;
}

// one worker per PHYSICAL device (several logical shards may share one on a small box)
int run_workers(const PieceJob &job, std::vector<Piece> &pcs, std::vector<DeviceRun> &runs)
{
    for (Piece &p : pcs)
    {
        auto r = std::find_if(runs.begin(), runs.end(), [&](const DeviceRun &d) { return d.cx->device == p.device; });
        if (r == runs.end())
            r = runs.insert(runs.end(), DeviceRun{&job, ctx_for(p.device)});
        r->pieces.push_back(&p);
    }
    if (runs.size() == 1)
        run_device(&runs[0]);
    else
    {
        std::vector<std::thread> th;
        for (auto &r : runs)
            th.emplace_back([](DeviceRun *d) {
                if (!getenv("KREP_GPU_NO_NUMA_BIND"))
                    bind_thread_near_device(d->cx->device);
                run_device(d);
            }, &r);
        for (auto &t : th)
            t.join();
    }
    for (auto &r : runs)
        if (r.rc)
            return kg::fail("device %d failed: %s", r.cx->device, r.err.c_str());
    return 0;
}

// a chain fix-up on the piece's device, under its lock: `n` bytes of the text from `from` staged in text buffer 0, then run(cx, plan, d_text)
template <class Run> int rerun_on(const PieceJob &job, int device, size_t from, size_t n, Run run)
{
    DeviceCtx &cx = *ctx_for(device);
    std::lock_guard<std::mutex> lk(cx.mu);
    krep_gpu_plan_t *pl = piece_plan(cx, job.params, job.cfg);
    if (!pl || cx.mem.ensure(n + 64, 1, cx.device) || cx.stager.init(cx.device) || cx.stager.copy(cx.mem.text(0), job.buf + from, n))
        return 2;
    return run(cx, pl, cx.mem.text(0));
}

// The one exchange step of the sequential families: walk the pieces in text order and compare what each
// was scanned with against what its left neighbour really left.  They differ only where a cluster of overlapping
// occurrences straddles a cut between two devices (the last consumed occurrence reaches < m bytes into the next
// shard); that piece is staged and scanned again with the true record — and, should its own record change, the one
// behind it.
int chain_fixup(const PieceJob &job, std::vector<Piece> &pcs)
{
    const search_params_t *params = job.params;
    const size_t len = job.len;
    krep_gpu_seq_carry_t tc{}; // what the text in front of the current piece REALLY leaves
    // -c with a newline inside a pattern (the emission-order line changes of aho_corasick_search, the window-grid walk of
    // simd_sse42_search / kmp_search): the piece's count depends on the EXACT record in front of it
    bool nl_chain = false;
    if (params->count_lines_mode)
        for (size_t i = 0; i < params->num_patterns; ++i)
            nl_chain = nl_chain || (params->pattern_lens[i] && memchr(params->patterns[i], '\n', params->pattern_lens[i]));
    for (Piece &p : pcs)
    {
        // walks: the piece's own list depends on where the scan stands at its start; block-loop -c: only the piece that
        // ends the text depends on the line-skip history
        // (multi-pattern -c with a newline inside a pattern: every piece's count depends on the newlines and the last match's
        //  line in front of it — for every other family these two fields stay 0)
        const bool stale = std::max<uint64_t>(p.carry_used.resume, p.lo) != std::max<uint64_t>(tc.resume, p.lo) ||
                           (p.hi == len && (p.carry_used.q1 != tc.q1 || p.carry_used.nl1 != tc.nl1 || p.carry_used.g0 != tc.g0)) ||
                           p.carry_used.nl_before != tc.nl_before || p.carry_used.last_line != tc.last_line ||
                           (nl_chain && p.carry_used.resume != tc.resume);
        // ... and when the line-skip history is ALL that differs for the piece that ends the text (the rule: every shard
        // starts from a zero record, so this is every multi-shard -c search through the block loops with an occurrence in an
        // earlier shard), only the end-of-text replay runs again — on the last 512 bytes of the text, with the piece's own
        // canonical count and contribution as they stand in its record (krep_gpu_replay_tail)
        const bool replay_only = stale && p.hi == len && p.carry_out.local_lines != 0 && !nl_chain &&
                                 std::max<uint64_t>(p.carry_used.resume, p.lo) == std::max<uint64_t>(tc.resume, p.lo) &&
                                 p.carry_used.nl_before == tc.nl_before && p.carry_used.last_line == tc.last_line &&
                                 !getenv("KREP_GPU_NO_REPLAY_FIXUP");
        if (replay_only)
        {
            const size_t tail = std::min<size_t>(len, 512);
            uint64_t lines = 0;
            krep_gpu_seq_carry_t co{};
            if (rerun_on(job, p.device, len - tail, tail, [&](DeviceCtx &, krep_gpu_plan_t *pl, uint8_t *d_tail) {
                    return krep_gpu_replay_tail(pl, d_tail, tail, len, nullptr, &tc, &p.carry_out, &co, &lines);
                }))
                return 2;
            p.carry_used = tc;
            p.carry_out = co;
            p.out.line_count = p.out.count = p.out.total_matches = lines; // (a -c scan: the count IS the line count; max_count is applied to the fold)
            g_chain_replays.fetch_add(1, std::memory_order_relaxed);
        }
        else if (stale)
        {
            if (rerun_on(job, p.device, p.b0, p.b1 - p.b0, [&](DeviceCtx &cx, krep_gpu_plan_t *pl, uint8_t *d_text) {
                    return scan_one_piece(cx, pl, d_text, &p, len, job.want_pos, &tc);
                }))
                return 2;
            g_chain_rescans.fetch_add(1, std::memory_order_relaxed);
        }
        // fold this piece's own contribution onto the true record (for a piece scanned with the true record this
        // reproduces its carry_out)
        tc = kg::fold_carry(tc, p.carry_out);
    }
    return 0;
}

// The shards' counters meet: per logical shard one slot {matches, lines, head, tail, has_nl}, each
// device fills the slots of its own shards, ONE RCCL all-reduce (uint64 sum over xGMI) makes every device hold all of them
// — the sum doubles as the all-gather the left-to-right line fold needs.  The reference's counterpart is the host loop
// over thread_args[] (krep.c:2930-3016).  A single shard has nothing to reduce.
void reduce_shards(const PieceJob &job, const std::vector<DeviceRun> &runs, uint64_t *total, uint64_t *lines)
{
    const int G = job.G;
    constexpr size_t kSlot = 5;
    std::vector<std::vector<unsigned long long>> vecs(runs.size(), std::vector<unsigned long long>(kSlot * (size_t)G, 0ull));
    for (size_t r = 0; r < runs.size(); ++r)
        for (int g = 0; g < G; ++g)
        {
            std::vector<krep_gpu_scan_out_t> outs;
            for (Piece *p : runs[r].pieces)
                if (p->shard == g)
                    outs.push_back(p->out);
            if (outs.empty())
                continue;
            unsigned long long *slot = &vecs[r][kSlot * (size_t)g];
            for (auto &o : outs)
            {
                slot[0] += o.total_matches;
                slot[4] |= o.has_newline;
            }
            slot[1] = krep_gpu_combine_line_counts(outs.data(), (int)outs.size());
            for (size_t i = 0; i < outs.size(); ++i) // a match before the shard's first newline
            {
                slot[2] |= outs[i].head_line_hit;
                if (outs[i].has_newline)
                    break;
            }
            for (size_t i = outs.size(); i-- > 0;) // ... after its last
            {
                slot[3] |= outs[i].tail_line_hit;
                if (outs[i].has_newline)
                    break;
            }
        }
    tl_shards = krep_gpu_shard_info_t{G, (int)runs.size(), {0}, 0, 0};
    for (size_t r = 0; r < runs.size() && r < 16; ++r)
        tl_shards.device_ids[r] = runs[r].cx->device;
    if (G > 1)
    {
        std::vector<int> devs;
        for (auto &r : runs)
            devs.push_back(r.cx->device);
        if (kg::allreduce_across_devices(devs, vecs) == 0)
        {
            tl_shards.reduced_by = 1;
            tl_shards.comm_ranks = kg::comm_clique_ranks(devs);
        }
        else
        {
            // This process already holds every shard's slots; the collective is how they are MEANT to meet, not a
            // reason to throw a finished search away: when librccl cannot be loaded or a communicator cannot be created the
            // host adds the slot vectors itself.  The reason stays in krep_gpu_last_error(), reported once.
            static std::atomic<bool> told{false};
            if (!told.exchange(true))
                fprintf(stderr, "krep-gpu: RCCL unavailable for the %d-shard count reduction; summing on the host\n", G);
            for (size_t r = 1; r < vecs.size(); ++r)
                for (size_t i = 0; i < vecs[0].size(); ++i)
                    vecs[0][i] += vecs[r][i];
            tl_shards.reduced_by = 2;
        }
    }
    *total = 0;
    std::vector<krep_gpu_scan_out_t> shard_outs((size_t)G);
    for (int g = 0; g < G; ++g)
    {
        const unsigned long long *slot = &vecs[0][kSlot * (size_t)g];
        *total += slot[0];
        shard_outs[g].line_count = slot[1];
        shard_outs[g].head_line_hit = slot[2] != 0;
        shard_outs[g].tail_line_hit = slot[3] != 0;
        shard_outs[g].has_newline = slot[4] != 0;
    }
    *lines = krep_gpu_combine_line_counts(shard_outs.data(), G);
}

// the operator's return value
uint64_t piece_verdict(const PieceJob &job, uint64_t total, uint64_t lines)
{
    const search_params_t *params = job.params;
    if (params->max_count == 0)
        return (job.algo == KREP_RA_BMH || job.algo == KREP_RA_MEMCHR_SHORT || job.algo == KREP_RA_AVX2 || job.algo == KREP_RA_AVX512 ||
                job.algo == KREP_RA_REGEX) &&
                       !params->count_lines_mode && !params->track_positions
                   ? (total > 0 ? 1 : 0) // count-only: the first hit makes 1 >= 0 true (krep.c:1355-1367)
                   : 0;
    return std::min<uint64_t>(params->count_lines_mode ? lines : total, params->max_count);
}

// The piece lists, one after the other into dst (room for all of them), each freed once copied: in parallel when they are large
// (at BASELINE config 3 density that is 5.5 GB; one thread copying it twice — into a scratch vector, then into the result — cost
// seconds).  multi: every piece list is in the reference's (end, start) order and owns its matches by START, so only a
// suffix of what precedes a cut and a prefix of what follows it can interleave — that zone is merged at every cut.
void gather_pieces(std::vector<Piece> &pcs, match_position_t *dst, bool multi)
{
    std::vector<size_t> off(pcs.size() + 1, 0);
    for (size_t i = 0; i < pcs.size(); ++i)
        off[i + 1] = off[i] + pcs[i].recs.size();
    std::atomic<size_t> next{0};
    auto work = [&] {
        for (size_t i; (i = next.fetch_add(1)) < pcs.size();)
        {
            if (!pcs[i].recs.empty())
                memcpy(dst + off[i], pcs[i].recs.data(), pcs[i].recs.size() * sizeof(match_position_t));
            std::vector<match_position_t>().swap(pcs[i].recs);
        }
    };
    const size_t nt = off.back() * sizeof(match_position_t) < (64u << 20) ? 1 : std::min<size_t>(8, pcs.size());
    std::vector<std::thread> th;
    for (size_t t = 1; t < nt; ++t)
        th.emplace_back(work);
    work();
    for (auto &t : th)
        t.join();
    if (multi)
        for (size_t i = 1; i < pcs.size(); ++i)
        {
            match_position_t *first_new = dst + off[i], *end = dst + off[i + 1];
            if (first_new == dst || first_new == end)
                continue;
            match_position_t *zone_lo = std::upper_bound(dst, first_new, *first_new, rec_less);
            match_position_t *zone_hi = std::upper_bound(first_new, end, *(first_new - 1), rec_less);
            std::inplace_merge(zone_lo, first_new, zone_hi, rec_less);
        }
}

// the records of `ret` > 0 matches: the merged piece lists, cut with the reference's -m conventions
int emit_records(const PieceJob &job, std::vector<Piece> &pcs, uint64_t ret, match_result_t *out)
{
    const bool multi = job.params->num_patterns > 1 && !job.params->use_regex; // (several -E patterns: one alternation, records by start)
    const size_t maxc = job.params->max_count;
    size_t tot = 0;
    for (const Piece &p : pcs)
        tot += p.recs.size();
    if (maxc == SIZE_MAX) // no truncation: the piece lists go STRAIGHT into the caller's block
    {
        if (!result_reserve(out, tot))
            return kg::fail("out of memory growing match_result_t");
        match_position_t *dst = out->positions + out->count;
        gather_pieces(pcs, dst, multi);
        if (multi && job.cfg.result_order) // the formatter's order (krep.c:420-434)
            std::sort(dst, dst + tot, by_start_end);
        out->count += tot;
        return 0;
    }
    std::vector<match_position_t> all(tot);
    gather_pieces(pcs, all.data(), multi);
    uint64_t n = std::min<uint64_t>(tot, ret);
    if (job.algo == KREP_RA_KMP && tot > maxc)
        n = maxc + 1; // krep.c:1717-1724
    if (job.algo == KREP_RA_MEMCHR)
        memchr_batch_quirk(all.data(), tot, maxc);
    if ((multi || job.algo == KREP_RA_MEMCHR) && job.cfg.result_order) // the formatter's order (krep.c:420-434)
        std::sort(all.begin(), all.begin() + (long)n, by_start_end);
    if (!result_reserve(out, n))
        return kg::fail("out of memory growing match_result_t");
    memcpy(out->positions + out->count, all.data(), n * sizeof(match_position_t));
    out->count += n;
    return 0;
}

// The text in pieces over G logical shards: lay them out, scan them (one worker per device), fix up the chain, reduce the shards'
// counters, then the verdict and the records
int run_pieces(const search_params_t *params, const krep_gpu_config_t &cfg, const char *buf, size_t len, int num_gpus, size_t chunk,
               match_result_t *out, uint64_t *ret_out)
{
    *ret_out = 0;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return kg::fail("no HIP device available");
    const PieceJob job{params, cfg, buf, len, params->track_positions && out != nullptr && !params->count_lines_mode,
                       kg::split_mode(params, cfg, len) == kSplitChain,
                       params->num_patterns > 1 && !params->use_regex ? KREP_RA_AHO_CORASICK : mirror_effective(mirror_top(params, cfg), params, len),
                       (int)std::min<size_t>((size_t)std::max(1, num_gpus), len / 4096 + 1)};
    std::vector<Piece> pcs = piece_layout(job, chunk, ndev);
    std::vector<DeviceRun> runs;
    if (run_workers(job, pcs, runs) || (job.chain && chain_fixup(job, pcs)))
        return 2;
    uint64_t total = 0, lines = 0;
    reduce_shards(job, runs, &total, &lines);
    *ret_out = piece_verdict(job, total, lines);
    return job.want_pos && *ret_out ? emit_records(job, pcs, *ret_out, out) : 0;
}
} // namespace

namespace kg {
int host_scan(const search_params_t *params, const krep_gpu_config_t &cfg, const char *text, size_t text_len, int num_gpus,
              match_result_t *result, uint64_t *ret)
{
    // streaming threshold: pieces of `chunk` bytes once the text is larger than two of them
    const size_t chunk = cfg.stream_chunk_bytes ? cfg.stream_chunk_bytes : ((size_t)128 << 20);
    const bool split = kg::shardable(params, cfg, text_len) && (num_gpus > 1 || text_len > 2 * chunk);
    tl_shards = krep_gpu_shard_info_t{1, 1, {cfg.device}, 0, 0};
    if (split)
        return run_pieces(params, cfg, text, text_len, num_gpus, text_len > 2 * chunk ? chunk : 0, result, ret);
    DeviceCtx *cx = ctx_for(cfg.device);
    std::lock_guard<std::mutex> lk(cx->mu);
    return run_whole(*cx, params, cfg, text, text_len, result, ret);
}

} // namespace kg

// ------------------------------------------------------------------------------------------------ a batch of texts as one text
// One pack of krep_gpu_search_batch / krep_gpu_grep_batch (kg_batch.hip): the items gathered through the staging ring into the arena's
// text buffer with a '\n' between neighbours, ONE scan over the whole pack in one window with records (again at the exact size when
// the list overflowed, as the operators do), the list cut per item on the device, the caller's step on the pack where it lies,
// results and rebased records read back in one copy each.  The steps in that order, cx.mu held:
namespace {
struct PackRun
{
    DeviceCtx &cx;
    const BatchPackJob &job;
    krep_gpu_plan_t *pl;
    size_t packed;
    uint8_t *d_text = nullptr;
    match_position_t *d_pos = nullptr; // the scan's list
    uint64_t n_rec = 0;
    match_position_t *d_list = nullptr; // the list every step behind the segmentation works on: under a cut cx.batch.d_cut
    uint64_t n_list = 0;
    bool by_end() const { return pl->ref_algo == KREP_RA_AHO_CORASICK; }

    int gather()
    {
        const auto fill = [items = job.items, off = job.off, n = job.n](uint8_t *dst, size_t lo, size_t cnt) {
            batch_fill(items, off, n, dst, lo, cnt);
        };
        return packed && (cx.stager.init(cx.device) || cx.stager.gather(d_text, packed, fill)) ? 2 : 0;
    }
    int scan(BatchPackDone *done)
    {
        krep_gpu_scan_out_t so{};
        if (packed && sized_scan(cx, std::max<uint64_t>(1u << 16, packed / 64), so, &d_pos, [&](match_position_t *d, uint64_t c) {
                return krep_gpu_scan_device_ex(pl, d_text, packed, 0, packed, 0, packed, d, c, nullptr, 1, &so);
            }))
            return 2;
        if (so.overflow)
            return kg::fail("search_batch: the record list outgrew its second, exact-size buffer");
        n_rec = done->n_rec = so.stored;
        done->kernel_ms = so.kernel_ms;
        return 0;
    }
    int segment(BatchPackDone *done) // the segmentation, the wait for it, and under a cut that keeps records their number
    {
        const uint64_t rec_base = (job.records ? job.records->count : 0) + (job.report ? job.appended : 0);
        if (batch_segment(cx.batch, BatchSegment{d_text, packed, job.off, job.n, d_pos, n_rec, rec_base, by_end(), job.lines, job.report,
                                                 job.cut, job.form}, nullptr))
            return 2;
        HIPCHK(hipStreamSynchronize(nullptr));
        if (job.cut && job.form != BatchCutOut::None && !job.lines && n_rec && job.cut->m && batch_kept_total(cx.batch, job.n, n_rec, &done->n_kept))
            return 2;
        d_list = job.cut ? cx.batch.d_cut : d_pos;
        n_list = job.cut ? done->n_kept : n_rec;
        return 0;
    }
    int read_back(krep_gpu_batch_result_t *res_out)
    {
        if (kg::inject(4) || hipMemcpy(res_out, cx.batch.d_res, job.n * sizeof *res_out, hipMemcpyDeviceToHost) != hipSuccess)
            return kg::fail("D2H copy of the batch results failed");
        if (!job.report || !n_list)
            return 0;
        if (!result_reserve(job.records, job.appended + n_list))
            return kg::fail("out of memory growing match_result_t");
        return records_to_host(job.records->positions + job.records->count + job.appended, d_list, n_list);
    }
};
} // namespace

int kg::host_batch_pack(const BatchPackJob &job, krep_gpu_batch_result_t *res_out, BatchPackDone *done)
{
    using clk = std::chrono::steady_clock;
    *done = BatchPackDone{};
    DeviceCtx &cx = *ctx_for(job.cfg->device);
    std::lock_guard<std::mutex> lk(cx.mu);
    krep_gpu_plan_t *pl = cx.plan_for(job.scan, *job.cfg);
    if (!pl)
        return 2;
    PackRun r{cx, job, pl, (size_t)job.off[job.n] - 1};
    HIPCHK(hipSetDevice(cx.device));
    if (cx.mem.ensure(r.packed + 64, 1, cx.device))
        return 2;
    r.d_text = cx.mem.text(0);
    auto t0 = clk::now();
    const auto timed = [&t0](double &stage, int rc) { // the wall clock since the stage before ended
        stage = std::chrono::duration<double, std::milli>(clk::now() - t0).count();
        t0 = clk::now();
        return rc;
    };
    if (timed(done->ms.pack, r.gather()) || timed(done->ms.scan, r.scan(done)) || timed(done->ms.segment, r.segment(done)))
        return 2;
    if (job.step && (*job.step)(BatchPackOnDevice{cx.batch, r.d_text, r.packed, cx.batch.d_off, job.n, r.d_list, r.n_list, r.by_end()}))
        return 2; // (its time is its own)
    t0 = clk::now();
    return timed(done->ms.read_back, r.read_back(res_out));
}

extern "C" void krep_gpu_last_shard_info(krep_gpu_shard_info_t *out) { if (out) *out = tl_shards; }

extern "C" void krep_gpu_release_device_resources(void)
{
    std::vector<DeviceCtx *> all;
    {
        std::lock_guard<std::mutex> lk(g_ctx_mu);
        if (g_ctx)
            for (auto &c : *g_ctx)
                if (c)
                    all.push_back(c.get());
    }
    for (DeviceCtx *c : all)
    {
        std::lock_guard<std::mutex> lk(c->mu);
        c->release();
    }
    kg::format_release();
}

extern "C" void krep_gpu_debug_chain_fixups(uint64_t *rescans, uint64_t *replays)
{
    if (rescans) *rescans = g_chain_rescans.load();
    if (replays) *replays = g_chain_replays.load();
}
