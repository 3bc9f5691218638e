// kg_ops.hip — the host-buffer side of the C-ABI: the search_func_t operators, search_buffer[_ex](), the drop-in for
// select_search_algorithm(); their executor is kg_exec.hip (kg::host_scan).  FAILURE: an attempt that fails appends nothing;
// the host's registered CPU function answers (run_with_fallback).  The configuration travels explicitly (krep_gpu_config_t);
// nothing here writes a global.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <vector>

#include "../../include/krep_gpu.h"
#include "kg_internal.h"

using namespace kg;

// ------------------------------------------------------------------------------------------------ dispatcher
namespace {
thread_local int tl_status = KREP_GPU_OK;
std::atomic<krep_gpu_cpu_select_t> g_cpu_select{nullptr};
} // namespace

extern "C" int krep_gpu_last_status(void) { return tl_status; }
extern "C" void krep_gpu_set_cpu_fallback(krep_gpu_cpu_select_t f) { g_cpu_select.store(f); }

// the GPU attempt: 0 = *ret and `result` are good; 2 = failed, nothing appended
static int run_host_operator(const search_params_t *raw, const char *text, size_t text_len, match_result_t *result,
                             const krep_gpu_config_t &cfg, int num_gpus, uint64_t *ret)
{
    *ret = 0;
    if (!raw || (!text && text_len))
        return kg::fail("NULL params/text");
    NormParams np(raw);
    if (!np.valid)
        return kg::fail("no pattern");
    const search_params_t *params = &np.sp;
    if (const char *why = kg::unsupported_reason(params, cfg))
        return kg::fail("%s", why);
    if (const char *why = kg::device_unusable(cfg.device))
        return kg::fail("%s", why);
    if (params->num_patterns > 1 && !params->ac_trie && !params->use_regex)
        return 0; // aho_corasick.c:306: no trie, no matches (several -E patterns are one alternation: no trie is involved)
    DeviceGuard guard;
    int ndev = 1;
    (void)hipGetDeviceCount(&ndev);
    if (num_gpus <= 0)
        num_gpus = ndev; // "all visible devices"
    const uint64_t count0 = result ? result->count : 0;
    if (kg::host_scan(params, cfg, text, text_len, num_gpus, result, ret) == 0)
        return 0;
    if (result)
        result->count = count0; // a failed attempt leaves the caller's list as it found it
    return 2;
}

// GPU attempt, then — on ANY failure (no device, refused input class, allocation, copy, launch) — the host's own CPU
// function, if it registered its selector.  A 0 that means "could not look" is never returned with status OK
// (SURVEY §8b "Errors"; the reference's fallback idiom krep.c:1944-1948, its error channel krep.c:2940-2947).
static uint64_t run_with_fallback(const search_params_t *params, const char *text, size_t text_len, match_result_t *result,
                                  const krep_gpu_config_t &cfg, int num_gpus, int *status_out, bool allow_fallback = true)
{
    krep_gpu_clear_error();
    const auto t0 = std::chrono::steady_clock::now();
    uint64_t n = 0;
    if (run_host_operator(params, text, text_len, result, cfg, num_gpus, &n) == 0)
    {
        kg::cost_note_host_path(text_len, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
        tl_status = KREP_GPU_OK;
        if (status_out) *status_out = 0;
        return n;
    }
    const krep_gpu_cpu_select_t sel = g_cpu_select.load();
    search_func_t cpu = (sel && params && allow_fallback) ? sel(params) : nullptr;
    if (cpu == krep_gpu_literal_search || cpu == krep_gpu_aho_corasick_search || cpu == krep_gpu_regex_search)
        cpu = nullptr; // a selector that hands our own operators back would recurse
    if (!cpu)
    {
        tl_status = KREP_GPU_FAILED;
        if (status_out) *status_out = 2;
        return 0;
    }
    static std::atomic<bool> warned{false};
    if (!warned.exchange(true))
        fprintf(stderr, "krep-gpu: falling back to the CPU function for this search (reported once)\n");
    const uint64_t count0 = result ? result->count : 0;
    const uint64_t r = cpu(params, text, text_len, result);
    if (result && cfg.result_order && result->count > count0 + 1)
        // krep_gpu_set_result_order(1) promises the formatter's (start, end) order (krep.c:420-434) whoever produced the records
        std::stable_sort(result->positions + count0, result->positions + result->count, by_start_end);
    tl_status = KREP_GPU_FELL_BACK;
    if (status_out) *status_out = 0;
    return r;
}

extern "C" uint64_t krep_gpu_literal_search(const search_params_t *params, const char *text, size_t len, match_result_t *result)
{
    const krep_gpu_config_t cfg = kg::current_config();
    return run_with_fallback(params, text, len, result, cfg, cfg.num_gpus, nullptr);
}
extern "C" uint64_t krep_gpu_aho_corasick_search(const search_params_t *params, const char *text, size_t len,
                                                 match_result_t *result)
{
    const krep_gpu_config_t cfg = kg::current_config();
    return run_with_fallback(params, text, len, result, cfg, cfg.num_gpus, nullptr);
}
extern "C" uint64_t krep_gpu_regex_search(const search_params_t *params, const char *text, size_t len, match_result_t *result)
{
    const krep_gpu_config_t cfg = kg::current_config();
    return run_with_fallback(params, text, len, result, cfg, cfg.num_gpus, nullptr);
}
extern "C" search_func_t krep_gpu_select_search_algorithm(const search_params_t *params)
{
    if (!params)
        return nullptr;
    const krep_gpu_config_t cfg = kg::current_config();
    // NULL: the caller keeps the CPU function pointer select_search_algorithm() gives it — for an input class that is not
    // reproduced, and when there is no device this library can run on (asked HERE, before any operator is handed out)
    if (kg::unsupported_reason(params, cfg) || kg::device_unusable(cfg.device))
        return nullptr;
    if (cfg.num_gpus != 1)
    {
        // a sharding host: create the devices' communicator NOW — the selector runs before the host has written a byte of
        // output, so RCCL's first-communicator banner (muted by redirecting fd 1 for that moment, kg_comm.hip) cannot swallow
        // output of another host thread later.  A failure here is not an error: a sharded search reports and sums on the host.
        DeviceGuard guard;
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) == hipSuccess && ndev > 1)
        {
            const int g = cfg.num_gpus <= 0 ? ndev : std::min(cfg.num_gpus, ndev);
            std::vector<int> devs;
            for (int i = 0; i < g; ++i)
                devs.push_back((cfg.device + i) % ndev);
            if (devs.size() > 1 && kg::comm_warmup(devs))
                krep_gpu_clear_error();
        }
    }
    if (params->use_regex)
        return krep_gpu_regex_search;
    return params->num_patterns > 1 ? krep_gpu_aho_corasick_search : krep_gpu_literal_search;
}

// search_string()'s validation and verdict (krep.c:2013-2049, :2166-2199), minus strlen and printing
extern "C" int search_buffer_ex(const search_params_t *params, const char *buf, size_t len, const krep_gpu_config_t *cfg_in,
                                int num_gpus, match_result_t *out, uint64_t *count_out)
{
    if (count_out)
        *count_out = 0;
    tl_status = KREP_GPU_FAILED; // until the search below says otherwise
    if (!params || params->num_patterns == 0 || !params->patterns || !params->pattern_lens)
        return kg::fail("Error: No pattern specified.");
    if (!buf && len)
        return kg::fail("Error: NULL text in search_buffer.");
    for (size_t i = 0; i < params->num_patterns; ++i)
    {
        if (params->pattern_lens[i] == 0)
        {
            if (params->num_patterns > 1)
                return kg::fail("Error: Empty pattern provided for literal search with multiple patterns.");
        }
        else if (params->pattern_lens[i] > 1024) // MAX_PATTERN_LENGTH, krep.c:77
            return kg::fail("Error: Pattern too long (max 1024).");
    }
    const krep_gpu_config_t cfg = cfg_in ? *cfg_in : kg::current_config();
    int st = 2;
    search_params_t local = *params;
    static int dummy_trie;
    const bool no_trie = local.num_patterns > 1 && !local.ac_trie && !local.use_regex;
    if (no_trie)
        local.ac_trie = (ac_trie_t *)&dummy_trie; // search_string builds the trie itself (krep.c:2067-2078)
    // (a CPU function could not use that placeholder: the fallback needs the caller's real trie)
    uint64_t n = run_with_fallback(&local, buf, len, out, cfg, num_gpus, &st, !no_trie);
    if (st)
        return 2;
    const size_t maxc = params->max_count;
    if (maxc != SIZE_MAX && n > maxc)
        n = maxc;
    if (out && maxc != SIZE_MAX && out->count > maxc)
        out->count = maxc;
    bool found;
    if (params->count_lines_mode || params->count_matches_mode)
        found = n > 0;
    else
    {
        found = out && out->count > 0;
        if (found)
            n = out->count;
        else if (!out)
            found = n > 0;
    }
    if (count_out)
        *count_out = n;
    return found ? 0 : 1;
}
extern "C" int search_buffer(const search_params_t *params, const char *buf, size_t len, int only_matching, int num_gpus,
                             match_result_t *out, uint64_t *count_out)
{
    krep_gpu_config_t cfg = kg::current_config();
    cfg.only_matching = only_matching != 0;
    return search_buffer_ex(params, buf, len, &cfg, num_gpus, out, count_out);
}
