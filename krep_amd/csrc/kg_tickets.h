// kg_tickets.h — the ticket -> resolver -> deferred-store scheme of the one-pass record writers (kg_single.hip: a single byte or a
// byte set; kg_ac_tiny.hip FUSED: the register-compare dictionary kernel; kg_literal_dma.hip ONEP: the sparse 2..8-byte literal, which
// parks several tickets and picks their prefixes up together), device side.
//
// A scanning wave draws tickets from ONE counter (so the drawn tickets are always a prefix of the ticket space), ranks the matches
// of a ticket into an LDS ring, publishes the ticket's count (`agg[t] = count | kTkReady`) and goes on; ONE resolver wave — the first
// wave 0 of any block to claim the role, a wave that RUNS whatever part of the grid is resident — turns the counts into exclusive
// prefixes (`pref[t] = first record index | kTkReady`), ticket by ticket as far as the run of published counts extends; a scanning
// wave picks its previous ticket's prefix up one ticket later and writes that ticket's records at their final index.  Progress
// without residency assumptions: with m the smallest unpublished ticket, every prefix up to m is published; m's holder is
// scanning it or waits for the prefix of an EARLIER ticket (published), so it goes on; no wait is circular (kg_single.hip header).
#pragma once
#include <hip/hip_runtime.h>
#include "kg_common.h"
#include "kg_device.h"

namespace kg {

// ---- the ticket map of kg_literal_dma.hip ONEP: which units a ticket number stands for.  Two sizes: the first n_long tickets hold
// upt_long units each (the bulk of the text: fewer seams per wave), the rest upt units (the end of the text: the kernel's tail stays as
// short as a short ticket), the last one what is left.  n_long * upt_long <= n_units.  n_long = 0 is the one-size map, t * upt.
// The kernel and the host use these three functions and nothing else to get from tickets to units.
struct TkMap
{
    uint32_t upt_long; // units of a long ticket
    uint32_t upt;      // units of a short one (>= 1)
    uint64_t n_long;   // tickets [0, n_long) are long
};
struct TkSpan
{
    uint64_t first; // the ticket's first unit
    uint32_t units; // ... and how many it holds (0, first = n_units: the ticket lies behind the text)
};
__host__ __device__ inline TkSpan tk_map(const TkMap m, const uint64_t n_units, const uint64_t t)
{
    const uint64_t u = t < m.n_long ? t * m.upt_long : m.n_long * m.upt_long + (t - m.n_long) * m.upt;
    const uint32_t c = t < m.n_long ? m.upt_long : m.upt;
    if (u >= n_units)
        return TkSpan{n_units, 0u};
    return TkSpan{u, n_units - u < (uint64_t)c ? (uint32_t)(n_units - u) : c};
}
__host__ __device__ inline uint64_t tk_map_tickets(const TkMap m, const uint64_t n_units)
{
    return m.n_long + (n_units - m.n_long * m.upt_long + m.upt - 1) / m.upt;
}
// How many long tickets a text of n_units gets when `waves` waves scan it.  The text ends with a region of short tickets; when the last
// long ticket is drawn every other wave is somewhere inside a long ticket of its own, and that region is what keeps them busy until the
// last one ends.  With equal speeds the worst case is a wave that draws the last long ticket just as all the others finish theirs: they
// need one long-ticket time each, 1.0 x waves x upt_long units (uniformly spread phases would need half of that).  Waves do not run at
// equal speeds (the scan moves by 2-3 % with placement alone, a wave that flushes records loses a round), so the region is 1.5 x that:
// a last long ticket up to half a ticket time late still ends inside the short tickets.  A text that has no room for one long ticket per
// wave in front of the region gets none: the one-size map.
__host__ __device__ inline uint64_t tk_map_long_tickets(const uint64_t n_units, const uint32_t upt_long, const uint32_t upt, const uint64_t waves)
{
    if (upt_long <= upt || !waves)
        return 0;
    const uint64_t region = (3 * waves * upt_long + 1) / 2;
    if (n_units < region)
        return 0;
    const uint64_t n_long = (n_units - region) / upt_long;
    return n_long >= waves ? n_long : 0;
}

constexpr unsigned long long kTkReady = 1ull << 63;
constexpr uint32_t kTkSpinLimit = 1u << 24;  // ~0.25 us per spin: seconds — only a logic error gets there (see the safety nets)
constexpr uint32_t kTkResolveChunk = 8;      // tickets per resolver lane and pass (512 per pass)

// The resolver wave's whole life: returns when every ticket has its prefix (ctr->total = the grand total), or — safety net, never
// expected — after flagging the scan as failed-over (ctr->overflow_units) and releasing every waiter with a made-up prefix.
__device__ __forceinline__ void tk_resolve(unsigned long long *__restrict__ agg, unsigned long long *__restrict__ pref,
                                           const unsigned long long n_tickets, Counters *ctr, const uint32_t lane)
{
    // Window of 64 x kTkResolveChunk tickets from `base`; every pass publishes the prefixes of the leading run of ready
    // tickets and moves the window behind it.  In the steady state the scanners are far ahead and a pass takes the whole
    // window; what matters is that the prefix of ticket p never waits for a ticket BEHIND p.
    u64 running = 0, base = 0;
    u32 spins = 0;
    while (base < n_tickets)
    {
        const u64 mine = base + (u64)lane * kTkResolveChunk;
        u64 v[kTkResolveChunk];
        u32 lead = 0, nvalid = 0;
        bool run = true;
#pragma unroll
        for (u32 k = 0; k < kTkResolveChunk; ++k)
        {
            const bool valid = mine + k < n_tickets;
            v[k] = valid ? __hip_atomic_load(&agg[mine + k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0ull;
            nvalid += valid ? 1u : 0u;
            run = run && valid && (v[k] & kTkReady);
            lead += run ? 1u : 0u;
        }
        const u64 open = __ballot(lead != nvalid);                 // lanes whose chunk holds a count that has not arrived
        const u32 f = open ? (u32)__builtin_ctzll(open) : 64u;     // the first of them: the ready run ends inside its chunk
        const u32 take = lane < f ? nvalid : (lane == f ? lead : 0u);
        u64 s = 0;
#pragma unroll
        for (u32 k = 0; k < kTkResolveChunk; ++k)
            s += k < take ? (v[k] & ~kTkReady) : 0ull;
        u64 incl = s;
        u32 tincl = take;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1)
        {
            const u64 up = __shfl_up(incl, o);
            const u32 tup = __shfl_up(tincl, o);
            if (lane >= (u32)o)
            {
                incl += up;
                tincl += tup;
            }
        }
        u64 e = running + incl - s;
#pragma unroll
        for (u32 k = 0; k < kTkResolveChunk; ++k)
        {
            if (k < take)
                __hip_atomic_store(&pref[mine + k], e | kTkReady, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            e += k < take ? (v[k] & ~kTkReady) : 0ull;
        }
        const u32 published = __shfl(tincl, 63);
        running += __shfl(incl, 63);
        base += published;
        if (published)
            spins = 0;
        else
        {
            if (++spins > kTkSpinLimit)
            {
                // safety net (never expected): a count that does not arrive within seconds must not hang the device.  Flag the
                // scan as failed-over (the host re-runs the two-pass kernels) and release every waiter with a made-up prefix.
                if (lane == 0)
                    atomicAdd(&ctr->overflow_units, 1ull);
                for (u64 t = base + lane; t < n_tickets; t += 64)
                    __hip_atomic_store(&pref[t], kTkReady, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                return;
            }
            __builtin_amdgcn_s_sleep(8);
        }
    }
    if (lane == 0)
        ctr->total = running;
}

// the first record index of ticket t, once the resolver has published it (lane 0 spins, the value is broadcast)
__device__ __forceinline__ unsigned long long tk_wait_prefix(const unsigned long long *__restrict__ pref, const unsigned long long t,
                                                              Counters *ctr, const uint32_t lane)
{
    u64 p = 0;
    if (lane == 0)
    {
        for (uint32_t spins = 0;; ++spins)
        {
            p = __hip_atomic_load(&pref[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (p & kTkReady)
                break;
            if (spins > 2u * kTkSpinLimit) // safety net, as in the resolver: flag the scan, go on with a made-up prefix
            {
                atomicAdd(&ctr->overflow_units, 1ull);
                p = kTkReady;
                break;
            }
            __builtin_amdgcn_s_sleep(4);
        }
    }
    return rfl64(p) & ~kTkReady;
}

// ... of the CALLING LANE's own ticket: every lane that calls spins for itself, so a wave that parked several tickets — all their counts
// published — picks their prefixes up in one memory latency (kg_literal_dma.hip ONEP: one lane per parked ticket)
__device__ __forceinline__ unsigned long long tk_wait_prefix_lane(const unsigned long long *__restrict__ pref, const unsigned long long t,
                                                                   Counters *ctr)
{
    u64 p = 0;
    for (uint32_t spins = 0;; ++spins)
    {
        p = __hip_atomic_load(&pref[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (p & kTkReady)
            break;
        if (spins > 2u * kTkSpinLimit) // safety net, as above
        {
            atomicAdd(&ctr->overflow_units, 1ull);
            p = kTkReady;
            break;
        }
        __builtin_amdgcn_s_sleep(4);
    }
    return p & ~kTkReady;
}

} // namespace kg
