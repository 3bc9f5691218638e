// kg_device.h — the device primitives the scan kernels share (gfx950, wave64): lane arithmetic, 64-bit readfirstlane, SWAR byte
// tests, the -w word-character rule, unaligned and bounds-checked text loads, the line-state bits of an info word and the
// wave-uniform counter draw.  One definition each; the kernel files include this header instead of keeping copies.
#pragma once
#include <hip/hip_runtime.h>
#include "kg_common.h"

namespace kg {

using u32 = uint32_t;
using u64 = unsigned long long;

// this lane's index in the wave (0..63)
__device__ __forceinline__ u32 lane_id() { return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }
// popcount(mask & lanes_below_me)
__device__ __forceinline__ u32 mbcnt64(u64 m) { return __builtin_amdgcn_mbcnt_hi((u32)(m >> 32), __builtin_amdgcn_mbcnt_lo((u32)m, 0u)); }
// the first active lane's 64-bit value in every lane.  readfirstlane returns an int: the low word goes through a u32, so it is
// zero-extended (OR-ing the int straight into a u64 would sign-extend it and set the high word of any value with bit 31 set)
__device__ __forceinline__ u64 rfl64(u64 v)
{
    const u32 lo = __builtin_amdgcn_readfirstlane((u32)v), hi = __builtin_amdgcn_readfirstlane((u32)(v >> 32));
    return ((u64)hi << 32) | lo;
}
// lane 0 adds v to the counter; every lane of the wave gets the value it held before (one atomic per wave)
__device__ __forceinline__ u64 wave_fetch_add(unsigned long long *ctr, u64 v, u32 lane)
{
    u64 old = 0;
    if (lane == 0)
        old = __hip_atomic_fetch_add(ctr, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return rfl64(old);
}

// 0x80 in every byte of x that equals the byte replicated in c4 (exact, no false positives)
__device__ __forceinline__ u32 eq_bytes(u32 x, u32 c4)
{
    const u32 y = x ^ c4;
    const u32 t = (y & 0x7f7f7f7fu) + 0x7f7f7f7fu;
    return ~(t | y | 0x7f7f7f7fu);
}
// gather the four 0x80 flags of a dword into a 4-bit mask
__device__ __forceinline__ u32 movemask4(u32 t) { return (((t >> 7) * 0x00204081u) >> 21) & 0xfu; }

// -w: a word character (is_whole_word_match, krep.h:312-319: C-locale isalnum or '_')
__device__ __forceinline__ bool is_wordc(u32 c) { return (c - '0' < 10u) || ((c | 0x20u) - 'a' < 26u) || c == '_'; }

// a T read from any byte address (one unaligned load)
template <typename T>
__device__ __forceinline__ T load_unaligned(const uint8_t *p)
{
    struct __attribute__((packed)) P { T v; };
    return reinterpret_cast<const P *>(p)->v;
}

// guarded 24-byte window for the (at most two) tiles that touch the end of the buffer: bytes past text_len read as 0
struct W6 { u32 v[6]; };
inline __device__ __noinline__ W6 load_window_guarded(const uint8_t *text, u64 text_len, u64 off)
{
    W6 r;
#pragma unroll
    for (int w = 0; w < 6; ++w)
    {
        u32 v = 0;
        for (int b = 0; b < 4; ++b)
        {
            const u64 o = off + (u64)(w * 4 + b);
            if (o < text_len)
                v |= (u32)text[o] << (8 * b);
        }
        r.v[w] = v;
    }
    return r;
}

// line bookkeeping of a window: distinct lines holding a match, has a '\n', a match before the first / after the last '\n'
struct LineState { u32 cnt; bool nl, head, tail; };
// its line bits in an info word (kLnNl | kLnHead | kLnTail)
__device__ __forceinline__ u64 line_bits(const LineState &s) { return (s.nl ? kLnNl : 0) | (s.head ? kLnHead : 0) | (s.tail ? kLnTail : 0); }

} // namespace kg
