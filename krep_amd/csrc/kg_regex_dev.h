// kg_regex_dev.h — what the two -E scans share (kg_regex.hip: one class sequence; kg_regex_alt.hip: an alternation of them): the
// program a plan holds, the unit size, and the device helpers that load a lane's bytes and make its range and newline masks.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/krep_gpu.h"
#include "kg_common.h"
#include "kg_device.h"
#include "kg_internal.h"
#include "kg_plan.h"

namespace kg {

struct RegexProg
{
    krep_gpu_regex_anchored_t info{};
    u32 *d_table = nullptr; // T[256] over the extended sequence: bit 0 is ^'s newline when bol, bit bol + j class j, bit bol + L $'s newline
    // an alternation (krep_gpu_regex_compile_alt took the search, the anchored compiler did not): branch i in bits [o_i, o_i + L_i) of
    // the state, T[b] bit o_i + j set iff b is in C[i][j]; init = every o_i, fin = every o_i + L_i - 1
    // alt_bol / alt_eol (krep_gpu_regex_compile_ext): every branch has the place { '\n' } in front of / behind its classes, so branch i
    // takes L_i + alt_bol + alt_eol bits
    bool is_alt = false;
    krep_gpu_regex_alt_t alt{};
    u32 alt_bol = 0, alt_eol = 0;
    u32 init = 0, fin = 0;
};

constexpr u32 kRxUnitBytes = kRoundsBig * kSegBytes; // 32 KiB of coordinates per wave unit

// 16 bytes from `off`, bytes at or past text_len read as 0
static __device__ __noinline__ uint4 rx_load_guarded(const uint8_t *text, u64 text_len, u64 off)
{
    u32 v[4];
#pragma unroll
    for (int w = 0; w < 4; ++w)
    {
        u32 x = 0;
        for (int b = 0; b < 4; ++b)
        {
            const u64 o = off + (u64)(w * 4 + b);
            if (o < text_len)
                x |= (u32)text[o] << (8 * b);
        }
        v[w] = x;
    }
    return make_uint4(v[0], v[1], v[2], v[3]);
}
// bit k set iff lo <= q + k < hi, k = 0..15
static __device__ __forceinline__ u32 rx_range(u64 q, u64 lo, u64 hi)
{
    const u32 lk = lo > q ? (u32)min(lo - q, (u64)16) : 0u, hk = hi > q ? (u32)min(hi - q, (u64)16) : 0u;
    return ((1u << hk) - 1u) & ~((1u << lk) - 1u);
}
static __device__ __forceinline__ u32 rx_newlines(const uint4 &d)
{
    return movemask4(eq_bytes(d.x, 0x0a0a0a0au)) | (movemask4(eq_bytes(d.y, 0x0a0a0a0au)) << 4) |
           (movemask4(eq_bytes(d.z, 0x0a0a0a0au)) << 8) | (movemask4(eq_bytes(d.w, 0x0a0a0a0au)) << 12);
}


// kg_regex_alt.hip: the scan of a window for an alternation (scan_regex hands over when the program is one)
int scan_regex_alt(krep_gpu_plan *pl, const Window &w, match_position_t *d_pos, uint64_t cap, hipStream_t st, int time_it,
                   krep_gpu_scan_out_t *out);
} // namespace kg
