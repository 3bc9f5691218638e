// kg_config.hip — the part of the C-ABI (include/krep_gpu.h) that holds no search logic: the error channel, the explicit
// configuration object behind the reference's compile-time SIMD macros and file-static option globals (krep.c:47-74,
// :117-120), device availability (asked by the selector BEFORE an operator is handed out), failure injection and the other
// test hooks.  Host logic only.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/krep_gpu.h"
#include "kg_common.h"
#include "kg_internal.h"
#include "kg_plan.h"
#include "kg_replay.h"
#include "kg_tickets.h"

using namespace kg;

// ------------------------------------------------------------------------------------ errors
static thread_local std::string g_err;
namespace kg {
int fail(const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    fprintf(stderr, "krep-gpu: %s\n", buf);
    return 2;
}
bool have_error() { return !g_err.empty(); }
void note_error(const char *why) { g_err = why ? why : ""; }
} // namespace kg
extern "C" const char *krep_gpu_last_error(void) { return g_err.c_str(); }
extern "C" void krep_gpu_clear_error(void) { g_err.clear(); }
extern "C" const char *krep_gpu_version(void) { return "krep-gpu 0.3 (gfx950)"; }
extern "C" int krep_gpu_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess)
        return 0;
    return n;
}

// ------------------------------------------------------------------------------------ configuration
// The reference decides its algorithm — hence the match-set family — from compile-time SIMD macros and three
// file-static globals (krep.c:47-74, :117-120).  Here they are one explicit krep_gpu_config_t.  The setters below write
// PROCESS-WIDE defaults (relaxed atomics: the reference's globals are process-wide too, set once by main() before the
// pool threads start); krep_gpu_set_thread_config() overrides them for the calling thread; plans and search_buffer_ex()
// carry their configuration explicitly.  Nothing on a scan path writes any of this.
static std::atomic<int> g_simd{KREP_REF_AVX2}, g_only_matching{0}, g_no_simd{0}, g_algo_override{KREP_ALGO_AUTO},
    g_result_order{0}, g_device{-1};
static std::atomic<size_t> g_stream_chunk{0};
static std::atomic<int> g_num_gpus{INT32_MIN};            // INT32_MIN: not set -> $KREP_GPU_NUM, else 1
static std::atomic<size_t> g_min_bytes{SIZE_MAX};         // SIZE_MAX: not set -> $KREP_GPU_MIN_BYTES, else 1 MiB
static thread_local bool tl_cfg_set = false;
static thread_local krep_gpu_config_t tl_cfg;

static int env_device()
{
    const char *e = getenv("KREP_GPU_DEVICE");
    return e && *e ? atoi(e) : 0;
}
static int env_num_gpus()
{
    const char *e = getenv("KREP_GPU_NUM");
    return e && *e ? atoi(e) : 1;
}
static size_t env_min_bytes()
{
    const char *e = getenv("KREP_GPU_MIN_BYTES");
    return e && *e ? (size_t)strtoull(e, nullptr, 0) : ((size_t)1 << 20);
}
extern "C" void krep_gpu_config_default(krep_gpu_config_t *c)
{
    if (!c)
        return;
    c->reference_simd = g_simd.load(std::memory_order_relaxed);
    c->only_matching = g_only_matching.load(std::memory_order_relaxed);
    c->force_no_simd = g_no_simd.load(std::memory_order_relaxed);
    c->algo_override = g_algo_override.load(std::memory_order_relaxed);
    c->result_order = g_result_order.load(std::memory_order_relaxed);
    const int d = g_device.load(std::memory_order_relaxed);
    c->device = d >= 0 ? d : env_device();
    c->stream_chunk_bytes = g_stream_chunk.load(std::memory_order_relaxed);
    const int ng = g_num_gpus.load(std::memory_order_relaxed);
    c->num_gpus = ng != INT32_MIN ? ng : env_num_gpus();
    const size_t mb = g_min_bytes.load(std::memory_order_relaxed);
    c->min_text_bytes = mb != SIZE_MAX ? mb : env_min_bytes();
}
extern "C" void krep_gpu_set_thread_config(const krep_gpu_config_t *c)
{
    tl_cfg_set = c != nullptr;
    if (c)
        tl_cfg = *c;
}
namespace kg {
krep_gpu_config_t current_config()
{
    if (tl_cfg_set)
        return tl_cfg;
    krep_gpu_config_t c;
    krep_gpu_config_default(&c);
    return c;
}
} // namespace kg
extern "C" void krep_gpu_set_reference_simd(int l) { g_simd.store(l, std::memory_order_relaxed); }
extern "C" int krep_gpu_get_reference_simd(void) { return kg::current_config().reference_simd; }
extern "C" void krep_gpu_set_only_matching(int on) { g_only_matching.store(on != 0, std::memory_order_relaxed); }
extern "C" void krep_gpu_set_result_order(int by_start) { g_result_order.store(by_start != 0, std::memory_order_relaxed); }
extern "C" void krep_gpu_set_force_no_simd(int on) { g_no_simd.store(on != 0, std::memory_order_relaxed); }
extern "C" void krep_gpu_set_algo_override(int a) { g_algo_override.store(a, std::memory_order_relaxed); }
extern "C" void krep_gpu_set_device(int d) { g_device.store(d, std::memory_order_relaxed); }
extern "C" void krep_gpu_set_stream_chunk(size_t bytes) { g_stream_chunk.store(bytes, std::memory_order_relaxed); }
extern "C" void krep_gpu_set_num_gpus(int n) { g_num_gpus.store(n, std::memory_order_relaxed); }
extern "C" void krep_gpu_set_min_text_bytes(size_t b) { g_min_bytes.store(b, std::memory_order_relaxed); }

// ------------------------------------------------------------------------------------ availability
// "Is there a device this library can run on" is asked by the SELECTOR, before any operator is handed out (SURVEY §8b:
// a backend must be able to fail BEFORE producing output): device count, range of the configured device, gfx950, and one
// probe kernel of this code object launched and read back.  Once per device and process.
__global__ void kg_probe_kernel(unsigned *out) { *out = 0x950u; }
namespace {
struct Avail
{
    std::mutex mu;
    std::vector<int> state;           // per device: 0 unknown, 1 usable, 2 not usable
    std::vector<std::string> reason;  // why not
};
Avail &avail()
{
    static Avail *a = new Avail(); // leaked: may be consulted from atexit paths
    return *a;
}
thread_local std::string tl_unavail;
bool probe_device(int device, std::string &why)
{
    int prev = -1;
    (void)hipGetDevice(&prev);
    auto done = [&](bool ok) {
        if (prev >= 0)
            (void)hipSetDevice(prev);
        (void)hipGetLastError();
        return ok;
    };
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess)
    {
        why = "hipGetDeviceProperties failed";
        return done(false);
    }
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    {
        why = std::string("device is ") + prop.gcnArchName + ", this library holds gfx950 code only";
        return done(false);
    }
    unsigned *d = nullptr, h = 0;
    if (hipSetDevice(device) != hipSuccess || hipMalloc(&d, sizeof(unsigned)) != hipSuccess)
    {
        why = "cannot allocate on the device";
        return done(false);
    }
    hipLaunchKernelGGL(kg_probe_kernel, dim3(1), dim3(1), 0, nullptr, d);
    const bool ok = hipGetLastError() == hipSuccess && hipMemcpy(&h, d, sizeof h, hipMemcpyDeviceToHost) == hipSuccess && h == 0x950u;
    (void)hipFree(d);
    if (!ok)
        why = "the gfx950 code object of this library does not run on the device";
    return done(ok);
}
} // namespace
namespace kg {
// NULL = usable; otherwise the reason (valid until the calling thread asks again)
const char *device_unusable(int device)
{
    if (const char *e = getenv("KREP_GPU_DISABLE"))
        if (*e && *e != '0')
            return "disabled by KREP_GPU_DISABLE";
    if (const char *e = getenv("KREP_GPU_ASSUME_AVAILABLE")) // test hook: skip the probe, so that a box WITHOUT a device
        if (*e && *e != '0')                                  // reaches the operators and exercises their run-time failure paths
            return nullptr;
    int ndev = 0;
    const auto t_first = std::chrono::steady_clock::now(); // (the process's first HIP call starts the runtime: kg_cost.hip wants to know)
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    {
        (void)hipGetLastError();
        return "no HIP device available";
    }
    if (device < 0 || device >= ndev)
    {
        tl_unavail = "device " + std::to_string(device) + " out of range (have " + std::to_string(ndev) + ")";
        return tl_unavail.c_str();
    }
    Avail &a = avail();
    std::lock_guard<std::mutex> lk(a.mu);
    if ((size_t)ndev > a.state.size())
    {
        a.state.resize((size_t)ndev, 0);
        a.reason.resize((size_t)ndev);
    }
    if (a.state[device] == 0)
    {
        a.state[device] = probe_device(device, a.reason[device]) ? 1 : 2;
        if (a.state[device] == 1)
            cost_note_device_init(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_first).count());
    }
    if (a.state[device] == 1)
        return nullptr;
    tl_unavail = a.reason[device];
    return tl_unavail.c_str();
}
// ---- failure injection (test hook): the failure paths of the operators must be reachable on a healthy box
static std::atomic<int> g_inject{-1};
bool inject(int kind)
{
    int v = g_inject.load(std::memory_order_relaxed);
    if (v < 0)
    {
        const char *e = getenv("KREP_GPU_INJECT_FAILURE");
        v = e && *e ? atoi(e) : 0;
        g_inject.store(v, std::memory_order_relaxed);
    }
    return v == kind;
}
} // namespace kg
extern "C" void krep_gpu_debug_inject_failure(int kind) { kg::g_inject.store(kind < 0 ? 0 : kind, std::memory_order_relaxed); }
extern "C" int krep_gpu_available(void) { return kg::device_unusable(kg::current_config().device) == nullptr ? 1 : 0; }
extern "C" const char *krep_gpu_unavailable_reason(void)
{
    const char *r = kg::device_unusable(kg::current_config().device);
    return r ? r : "";
}

namespace kg {
std::atomic<int> g_force_rounds{0};    // test hook: 0 = auto, 1 / 4 = force the tile shape
std::atomic<int> g_force_stage_cap{0}; // test hook: staging records per unit (0 = auto)
std::atomic<int> g_rx_force_grid{0};   // test hook: workgroups of the regex scan (0 = auto)
}
extern "C" void krep_gpu_debug_force_stage_cap(int c) { g_force_stage_cap.store(c); }
extern "C" void krep_gpu_debug_force_rounds(int r) { g_force_rounds.store(r); }
extern "C" void krep_gpu_debug_force_regex_grid(int blocks) { g_rx_force_grid.store(blocks < 0 ? 0 : blocks); }
// The loops compiler behind a switch (include/krep_gpu.h, krep_gpu_regex_compile_loops): process-wide like the setters above, but not a
// field of krep_gpu_config_t — it is off by default and on for a whole process or not at all.
static int env_regex_loops()
{
    const char *e = getenv("KREP_GPU_REGEX_LOOPS");
    return e && *e && atoi(e) != 0 ? 1 : 0;
}
// ... and whether such a search may be cut into windows (include/krep_gpu.h, "Windows"): a switch of its own, off by default
static int env_regex_loops_windows()
{
    const char *e = getenv("KREP_GPU_REGEX_LOOPS_WINDOWS");
    return e && *e && atoi(e) != 0 ? 1 : 0;
}
// ... and the groups compiler behind a switch of its own (include/krep_gpu.h, krep_gpu_regex_compile_groups), independent of the two above
static int env_regex_groups()
{
    const char *e = getenv("KREP_GPU_REGEX_GROUPS");
    return e && *e && atoi(e) != 0 ? 1 : 0;
}
// ... and the linear walk of lines over 4096 bytes in a loops or groups search (include/krep_gpu.h, "Long lines"), likewise
static int env_regex_long_lines()
{
    const char *e = getenv("KREP_GPU_REGEX_LONG_LINES");
    return e && *e && atoi(e) != 0 ? 1 : 0;
}
namespace kg {
std::atomic<int> g_regex_groups{env_regex_groups()};
std::atomic<int> g_rl_force_general{0}; // test hook: a loops program is walked by the general step (kg_regex.hip, regex_prog_create)
std::atomic<uint64_t> g_rl_general{0};  // launches of the line walk's general step (kg_regex_loops.hip)
std::atomic<int> g_regex_loops{env_regex_loops()}; // (read when the library is loaded)
std::atomic<int> g_regex_loops_windows{env_regex_loops_windows()};
std::atomic<int> g_regex_long_lines{env_regex_long_lines()};
std::atomic<uint64_t> g_rl_long_budget{0};         // test hook: bytes of C words a round of long lines may hold (0: the default)
std::atomic<uint64_t> g_rl_long{0};                // launches of the long-line walk (kg_regex_loops.hip)
std::atomic<int> g_rl_force_road{0};               // test hook: 0 auto, 1 the sparse road, 2 the dense road (kg_regex_loops.hip)
std::atomic<uint64_t> g_rl_sparse{0}, g_rl_dense{0}; // scans that took each road
}
extern "C" void krep_gpu_set_regex_loops(int on) { kg::g_regex_loops.store(on != 0, std::memory_order_relaxed); }
extern "C" int krep_gpu_get_regex_loops(void) { return kg::g_regex_loops.load(std::memory_order_relaxed); }
extern "C" void krep_gpu_set_regex_loops_windows(int on) { kg::g_regex_loops_windows.store(on != 0, std::memory_order_relaxed); }
extern "C" int krep_gpu_get_regex_loops_windows(void) { return kg::g_regex_loops_windows.load(std::memory_order_relaxed); }
extern "C" void krep_gpu_set_regex_groups(int on) { kg::g_regex_groups.store(on != 0, std::memory_order_relaxed); }
extern "C" int krep_gpu_get_regex_groups(void) { return kg::g_regex_groups.load(std::memory_order_relaxed); }
extern "C" void krep_gpu_set_regex_long_lines(int on) { kg::g_regex_long_lines.store(on != 0, std::memory_order_relaxed); }
extern "C" int krep_gpu_get_regex_long_lines(void) { return kg::g_regex_long_lines.load(std::memory_order_relaxed); }
extern "C" void krep_gpu_debug_set_regex_long_budget(uint64_t bytes) { kg::g_rl_long_budget.store(bytes, std::memory_order_relaxed); }
extern "C" uint64_t krep_gpu_debug_regex_long_walks(void) { return kg::g_rl_long.load(); }
extern "C" void krep_gpu_debug_force_regex_general(int on) { kg::g_rl_force_general.store(on != 0); }
extern "C" uint64_t krep_gpu_debug_regex_general_walks(void) { return kg::g_rl_general.load(); }
extern "C" void krep_gpu_debug_force_regex_loops_road(int road) { kg::g_rl_force_road.store(road == 1 || road == 2 ? road : 0); }
extern "C" void krep_gpu_debug_regex_loops_roads(uint64_t *sparse, uint64_t *dense)
{
    if (sparse) *sparse = kg::g_rl_sparse.load();
    if (dense) *dense = kg::g_rl_dense.load();
}
// The batch's per-item max_count cut behind a switch of the same kind (include/krep_gpu.h, krep_gpu_set_batch_max_count)
static int env_batch_max_count()
{
    const char *e = getenv("KREP_GPU_BATCH_MAX_COUNT");
    return e && *e && atoi(e) != 0 ? 1 : 0;
}
namespace kg {
std::atomic<int> g_batch_max_count{env_batch_max_count()}; // (read when the library is loaded)
}
extern "C" void krep_gpu_set_batch_max_count(int on) { kg::g_batch_max_count.store(on != 0, std::memory_order_relaxed); }
extern "C" int krep_gpu_get_batch_max_count(void) { return kg::g_batch_max_count.load(std::memory_order_relaxed); }
namespace kg {
extern int g_s1_force_grid;
std::atomic<uint64_t> g_fused1_failovers{0}; // one-pass single-byte scans that handed over to the two-pass kernels
}
extern "C" void krep_gpu_debug_force_single_grid(int blocks) { kg::g_s1_force_grid = blocks < 0 ? 0 : blocks; }
extern "C" uint64_t krep_gpu_debug_single_failovers(void) { return g_fused1_failovers.load(); }
namespace kg {
std::atomic<uint64_t> g_fused1_launches{0};
}
extern "C" uint64_t krep_gpu_debug_single_launches(void) { return kg::g_fused1_launches.load(); }
namespace kg {
std::atomic<uint64_t> g_tiny_launches{0}; // launches of ac_tiny_kernel
}
extern "C" uint64_t krep_gpu_debug_tiny_launches(void) { return kg::g_tiny_launches.load(); }
namespace kg {
std::atomic<uint64_t> g_tiny_dense_launches{0}; // ... of its DENSE one-pass flavour
}
extern "C" uint64_t krep_gpu_debug_tiny_dense_launches(void) { return kg::g_tiny_dense_launches.load(); }
namespace kg {
std::atomic<uint64_t> g_ac_anchored_launches{0}; // launches of the multi-pattern kernel's anchored instantiation
}
extern "C" uint64_t krep_gpu_debug_anchored_launches(void) { return kg::g_ac_anchored_launches.load(); }
extern "C" uint64_t krep_gpu_debug_literal_dma_launches(void) { return kg::g_lit_dma_launches.load(); }
extern "C" uint64_t krep_gpu_debug_literal_dma_one_pass_launches(void) { return kg::g_lit_dma1p_launches.load(); }
extern "C" uint64_t krep_gpu_debug_literal_dma_one_pass_failovers(void) { return kg::g_lit_dma1p_failovers.load(); }
extern "C" void krep_gpu_debug_force_literal_dma_grid(int blocks) { kg::g_lit_dma1p_force_grid = blocks < 0 ? 0 : blocks; }
extern "C" void krep_gpu_debug_force_literal_dma_tickets(int long_units, uint64_t n_long)
{
    const bool ok = long_units == 8 || long_units == 16 || long_units == 32;
    kg::g_lit_dma1p_force_long = ok ? long_units : 0;
    kg::g_lit_dma1p_force_n_long = ok ? n_long : 0;
}
extern "C" void krep_gpu_debug_literal_dma_last_tickets(uint32_t *long_units, uint64_t *n_long)
{
    *long_units = kg::g_lit_dma1p_last_long.load();
    *n_long = kg::g_lit_dma1p_last_n_long.load();
}
extern "C" int krep_gpu_debug_ticket_map(uint32_t upt_long, uint32_t upt, uint64_t n_long, uint64_t n_units, uint64_t ticket, uint64_t *first,
                                         uint32_t *units, uint64_t *n_tickets)
{
    if (!upt || (n_long && (!upt_long || n_long > n_units / upt_long)))
        return 2;
    const kg::TkMap m = {upt_long, upt, n_long};
    const kg::TkSpan s = kg::tk_map(m, n_units, ticket);
    *first = s.first;
    *units = s.units;
    *n_tickets = kg::tk_map_tickets(m, n_units);
    return 0;
}
extern "C" uint64_t krep_gpu_debug_ticket_map_long_tickets(uint64_t n_units, uint32_t upt_long, uint32_t upt, uint64_t waves)
{
    return kg::tk_map_long_tickets(n_units, upt_long, upt, waves);
}
extern "C" uint64_t krep_gpu_debug_runs_launches(void) { return kg::g_runs_launches.load(); }

