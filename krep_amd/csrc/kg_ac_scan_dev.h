// kg_ac_scan_dev.h — the stages of ac_scan_kernel (kg_ac.hip, whose header holds the stage map), one function per stage.  Each names the
// template parameters it uses and gets what it reads and writes through its arguments: the launch's AcArgs, the wave's AcWave, plain values.
#pragma once
#include "kg_ac_common.h"
#include "kg_internal.h"

namespace kg {

#ifndef KG_AC_LINES_ROLL_CELLS
#define KG_AC_LINES_ROLL_CELLS 4 // cells (1 KiB each) of the next round a -c scan prefetches (A/B: krep_amd/build.py --variant x -DKG_AC_LINES_ROLL_CELLS=8)
#endif

// What the stages of one wave share: its areas of the block's LDS (set once) and the unit an emission refers to (set per unit; the
// deferred stage 3 of the anchored scan re-aims it at the unit a pending pair belongs to).
struct AcWave
{
    u32 *cbits;            // candidate bitmap of the unit: one bit per end position, entry (r * 8 + j) * 64 + lane, index order = position order
    u32 *ebits;            // ANCH: the unit's END-pair bitmap (1 KiB, the park area: an anchored scan parks nothing)
    u32 *bitmap;           // -c: the unit's hit bitmap, one bit per END
    unsigned short *nlmap; // -c: newline masks, 16 bits per lane and cell
    u32 *park_slots;       // [kAcUnitsPerTicketMax][16] staged words
    u64 *park_info;        // [kAcUnitsPerTicketMax]
    u64 e_useg, e_fbase;   // first byte of the unit emitted into | its first record (emit pass)
    u32 *e_slot;           // its staging slot
    u32 wcnt;              // matches of the unit so far == rank of the next one (uniform)
    bool do_stage, do_final;
};

constexpr u32 ac_xbits(bool lines) { return lines ? kXBitsLines : kXBitsBig; } // index bits of the exact-class table
constexpr u32 ac_tab_mask(bool lines) { return ac_xbits(lines) == 20 ? 0x1fffcu : 0xfffcu; } // byte address of a pair-layout slot
// -c prefetches only the first kRoll cells of the next round with the stride-1 filter and none with the pair filter (every
// -c instantiation then fits the 128 VGPRs of a 1024-thread block without scratch; with the full prefetch they spilled 8-44
// bytes per lane.  Measured at 32 GiB on the 1000-pattern dictionary, in-kernel -c road: 9.90 ms without the prefetch,
// 9.61 ms with it and 20 bytes of scratch, profiles/r05_line_counting.txt; texts of 32 MiB and more count their lines on the
// record list, kg_scan.hip, at 6.8 ms); the rest of a prefetched round is requested at its start
// (the anchored instantiations roll six of the eight cells: the last two are requested at the round's start and consumed last —
//  their eight registers are free while the two verify stages run, which otherwise spilled 12-20 bytes per lane)
constexpr int ac_roll_cells(bool lines, int stride, int anch) { return lines ? (stride == 2 ? 0 : KG_AC_LINES_ROLL_CELLS) : (anch != 0 ? kCells - 2 : kCells); }
// the deferred verify (ac_pend_unit) applies to: the anchored scan; with -DKG_AC_DEFER_GENERIC also the pipelined end-gram kernel
constexpr bool ac_pends(bool lines, bool shorts, int stride, int anch)
{
#ifdef KG_AC_DEFER_GENERIC
    return anch != 0 || (stride == 2 && !lines && !shorts);
#else
    return anch != 0;
#endif
}
// -c owns a match by its END and records it in the unit's hit bitmap, so the end j + 2 of the unit's last candidate bit
// (= the first byte of the next unit) cannot be reported from here: every unit instead verifies one EXTRA candidate, the
// tested position in front of its first byte, for its second end only
constexpr bool ac_xcand(bool lines, int stride) { return stride == 2 && lines; }
constexpr u32 ac_wpl(bool lines, int stride) { return stride == 2 && !lines ? 4u : 8u; } // bitmap dwords per enumerating lane (256 positions)

typedef __attribute__((address_space(3))) const u32 ac_lds_u32;
// the pair-layout table's dword for the pair register u (kg_ac_common.h ac_pair_slot): byte address = ((u >> 3) ^ (u >> 13)) & mask.
// The table sits at LDS address 0 (checked at kernel entry): an absolute LDS pointer saves the v_add of the (link-time) base of
// s_mem on every lookup.  (-c: a 2^19-bit table, address bit 16 = bit 3 of the class c2 dropped)
template <bool LINES>
__device__ __forceinline__ u32 ac_pair_dword(const u32 u) { return *(ac_lds_u32 *)(size_t)(((u >> 3) ^ (u >> 13)) & ac_tab_mask(LINES)); }
// ... and its answer: the bit is the earliest class (the shifter reads the low 5 bits itself)
template <bool LINES>
__device__ __forceinline__ bool ac_pair_test(const u32 u) { return ((ac_pair_dword<LINES>(u) >> (u & 31u)) & 1u) != 0u; }
// The eight pair registers x of a cell's tested (odd) positions from the pair classes t[0..4] of the lane's 20 bytes, and the table
// dwords v they select: the gram of k = 3 (mod 4) is a class register as it is, the gram of k = 1 (mod 4) one v_alignbit over two.
template <bool LINES, int ANCH>
__device__ __forceinline__ void ac_cell_pairs(const u32 (&t)[5], u32 (&x)[8], u32 (&v)[8])
{
#pragma unroll
    for (int q = 0; q < 8; ++q)
    {
        const int w = q / 2 + 1;
        x[q] = (q & 1) ? t[w] : __builtin_amdgcn_alignbit(t[w], t[w - 1], 16u);
        if constexpr (ANCH == 2) // the class of the byte in front of the gram (byte 2q - 3 of the lane), mixed into the class fields
            x[q] = ac_mix5(x[q], __builtin_amdgcn_ubfe(t[(2 * q + 1) / 4], ((2 * q + 1) % 4 == 1) ? 5u : 21u, 5u));
        v[q] = ac_pair_dword<LINES>(x[q]);
    }
}

// ---------------------------------------------------------------------------------------------- the filter of a round
// The 4 bytes in front of a round: carried from the round before or loaded.
// `before` is settled BEFORE the round's loads are issued and kept SCALAR: as a vector register filled on a cold path it made the
// compiler wait vmcnt(0) where the paths join — at the start of EVERY round, draining the rolling prefetch the filter never needed
// to wait for
__device__ __forceinline__ u32 ac_round_before(const AcArgs &a, const u64 seg, const bool have, const u32 carry)
{
    if (have)
        return carry;
    u32 bb = 0;
    if (seg >= 4 && seg <= a.text_len)
        bb = *reinterpret_cast<const u32 *>(a.text + seg - 4);
    else
        for (u32 b = 0; b < 4; ++b)
            if (seg + b >= 4 && seg + b - 4 < a.text_len)
                bb |= (u32)a.text[seg + b - 4] << (8 * b);
    return __builtin_amdgcn_readfirstlane(bb);
}

// the 16 positions of a lane-cell at offset lrel of the round `seg` that lie in [lo, hi): window bounds relative to the round
// (uniform, clamped to [0, 8 KiB]) against the lane's 32-bit offset
__device__ __forceinline__ u32 ac_window_mask(const u64 lo, const u64 hi, const u64 seg, const u32 lrel)
{
    const u32 rlo = lo > seg ? (u32)((lo - seg) < kSegBytes ? (lo - seg) : kSegBytes) : 0u;
    const u32 rhi = hi > seg ? (u32)((hi - seg) < kSegBytes ? (hi - seg) : kSegBytes) : 0u;
    const u32 klo = rlo > lrel ? ((rlo - lrel) < 16u ? (rlo - lrel) : 16u) : 0u;
    const u32 khi = rhi > lrel ? ((rhi - lrel) < 16u ? (rhi - lrel) : 16u) : 0u;
    return khi > klo ? (((1u << khi) - 1u) & ~((1u << klo) - 1u)) : 0u;
}

// The filter of cell j of round r: the lane's candidates into the unit's bitmap (cbits), -c also the newline mask (nlmap).
// W[0] = the 4 bytes before the lane, W[1..4] = the lane's 16 bytes of cell j
// have_c: the caller already holds the classes of W[0] and W[4] (fast path: it shuffles the 20-bit class word
// of the neighbour lane instead of its raw bytes, which saves one compress per cell)
template <bool LINES, int STRIDE, int ANCH>
__device__ __forceinline__ void ac_filter_cell(const AcArgs &a, const AcWave &wv, const u32 lane, const int r, const int j, const u64 seg,
                                               const bool interior, const u32 (&W)[5], const bool have_c, const u32 pc0, const u32 pc4)
{
    constexpr bool PAIR = STRIDE == 2;    // pair-layout table, odd positions tested
    constexpr bool PIPE = PAIR && !LINES; // (the bitmap's layout with the pipelined filter, ac_pair_round)
    u32 NL = 0;
    if (LINES)
    {
        // (exact 16-bit mask in every cell, ~40 VALU: storing only a has-newline flag and fetching the hit lanes' bytes
        //  in the line pass was measured — one more memory round trip per unit cost more than it saved: 10.15 -> 11.3 ms)
#pragma unroll
        for (int w = 0; w < 4; ++w)
            NL |= movemask4(eq_bytes(W[w + 1], 0x0a0a0a0au)) << (4 * w);
    }
    u32 cand = 0;
    if constexpr (PAIR)
    {
        // ---- filter, pair layout (stride 2 without -c): the ODD positions are tested, so the gram of position k is two
        //      16-bit-aligned byte pairs.  A dword becomes two 10-bit pair classes in its halves (3 VALU); the gram of
        //      k = 3 (mod 4) is that register as it is, the gram of k = 1 (mod 4) one v_alignbit over two of them.  The
        //      table slot is chosen for this register (ac_pair_slot): bit = the earliest class (the shifter reads the low
        //      5 bits itself), byte address = ((u >> 3) ^ (u >> 13)) & 0x1fffc — two shifts and one v_bitop3, and the
        //      LDS bank is the XOR of two classes (one class alone sends the 16 % blanks of a text to ONE bank: 10.6
        //      instead of 7.2 cycles per 64-lane read).  Per tested position: 0.5 + 3 + 2 VALU and 1.5 for the
        //      classes — 58 per 1-KiB cell where the 100-bit class stream took ~95 ----
        u32 t[5];
#pragma unroll
        for (int w = 1; w < 4; ++w)
            t[w] = ac_pair(W[w]);
        t[0] = have_c ? pc0 : ac_pair(W[0]);
        t[4] = have_c ? pc4 : ac_pair(W[4]);
        u32 xs[8], dws[8];
        ac_cell_pairs<LINES, ANCH>(t, xs, dws);
        __builtin_amdgcn_sched_barrier(0);
        u32 acc = 0;
#pragma unroll
        for (int q = 0; q < 8; ++q)
            acc = __builtin_amdgcn_alignbit(dws[q] >> (xs[q] & 31u), acc, 2u);
        cand = (acc >> 16) & 0x5555u; // bit 2q <-> tested position 2q + 1 (the verify stage adds the 1)
    }
    else
    {
        // ---- filter, exact-class table: the lane's 20 bytes as a 100-bit stream of 5-bit classes; the
        //      index of end position k is the 20-bit window at bit 5(k+1): one v_alignbit, no hash ----
        u32 c[5];
#pragma unroll
        for (int w = 1; w < 4; ++w)
            c[w] = ac_cls4(W[w]);
        c[0] = have_c ? pc0 : ac_cls4(W[0]);
        c[4] = have_c ? pc4 : ac_cls4(W[4]);
        u32 R[5];
        R[0] = c[0] | (c[1] << 20);
        R[1] = (c[1] >> 12) | (c[2] << 8) | (c[3] << 28);
        R[2] = (c[3] >> 4) | (c[4] << 16);
        R[3] = c[4] >> 16;
        R[4] = 0;
        // per position 5 VALU: window, dword address, ds_read_b32, shift by the low 5 index bits (the shifter
        // masks them itself), and a funnel shift that pushes the hit bit into the accumulator from the top
        // all table reads of the cell are issued before the first one is consumed (the scheduler otherwise
        // serialises read -> wait -> shift through the accumulator chain: 8-16 LDS latencies per cell)
        constexpr int NK = 16 / STRIDE;
        // (stride 1 with the rolling prefetch: in two batches of 8 — 32 index / data registers at once spilled 12-20 bytes
        //  per lane under the 128-VGPR cap)
#ifndef KG_AC_S1_ONE_BATCH // (A/B switch)
        constexpr int NB = (NK == 16 && !LINES) ? 8 : NK;
#else
        constexpr int NB = NK;
#endif
        u32 acc = 0;
#pragma unroll
        for (int q0 = 0; q0 < NK; q0 += NB)
        {
            u32 xs[NB], dws[NB];
#pragma unroll
            for (int q = 0; q < NB; ++q)
            {
                const int o = 5 * ((q0 + q) * STRIDE + 1);
                xs[q] = (o & 31) ? __builtin_amdgcn_alignbit(R[(o >> 5) + 1], R[o >> 5], (u32)(o & 31)) : R[o >> 5];
                // the table sits at LDS address 0 (checked at kernel entry): an absolute LDS pointer saves the
                // v_add of the (link-time) base of s_mem on every lookup
                dws[q] = *(ac_lds_u32 *)(size_t)((xs[q] >> 3) & ((1u << (ac_xbits(LINES) - 3)) - 4u));
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int q = 0; q < NB; ++q)
                acc = __builtin_amdgcn_alignbit(dws[q] >> (xs[q] & 31u), acc, (u32)STRIDE);
            if (q0 + NB < NK)
                __builtin_amdgcn_sched_barrier(0);
        }
        cand = STRIDE == 2 ? (acc >> 16) & 0x5555u : acc >> 16;
    }
    u32 nlm = NL;
    if (!interior)
    {
        const u32 lrel = (u32)j * kCellBytes + lane * 16u;
        const u32 endm = ac_window_mask(a.end_lo, a.end_hi, seg, lrel);
        if (!PAIR) // (pair layout: a bit stands for the ends k + 1 and k + 2, the second possibly in the next lane; the
                   //  verify stage applies the exact window)
            cand &= STRIDE == 2 ? (endm | (endm >> 1)) : endm; // stride 2: t or t + 1 is an end of this launch
        if (LINES)
            nlm &= ac_window_mask(a.own_lo, a.own_hi, seg, lrel);
    }
    const u32 at = (u32)r * (kSegBytes / 16) + (u32)j * kWave + lane;
    if (LINES) // kept in LDS, not in 16 registers, across the verify stage
        wv.nlmap[at] = (unsigned short)nlm;

    // ---- the lane's candidates go into the unit's bitmap; they are enumerated once per unit (ac_verify_count) instead
    //      of ranked per cell (ballots + a divergent store loop: ~15 VALU per cell), and nothing overflows ----
    if (PIPE)
    {
        u32 x = cand & 0x5555u; // even bits -> 8 contiguous bits
        x = (x | (x >> 1)) & 0x3333u;
        x = (x | (x >> 2)) & 0x0f0fu;
        x = (x | (x >> 4)) & 0x00ffu;
        reinterpret_cast<uint8_t *>(wv.cbits)[at] = (uint8_t)x;
    }
    else
        reinterpret_cast<unsigned short *>(wv.cbits)[at] = (unsigned short)cand;
}

// pipelined pair filter, first half of cell j: its classes out of d[j] (which then receives cell j of the next round), the pair
// registers x and the table reads v
template <int ANCH>
__device__ __forceinline__ void ac_pair_issue(const int j, uint4 (&d)[kCells], const uint4 *nsrc, u32 &before, u32 (&x)[8], u32 (&v)[8])
{
    u32 t[5];
    t[1] = ac_pair(d[j].x); t[2] = ac_pair(d[j].y); t[3] = ac_pair(d[j].z); t[4] = ac_pair(d[j].w);
    const u32 last = d[j].w;
    if (j < ac_roll_cells(false, 2, ANCH))
        d[j] = nsrc[j * kWave];
    t[0] = (u32)__builtin_amdgcn_update_dpp((int)ac_pair(before), (int)t[4], 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
    before = __builtin_amdgcn_readlane(last, 63);
    ac_cell_pairs<false, ANCH>(t, x, v);
}
// ... second half: the eight answers into the unit's candidate bitmap
__device__ __forceinline__ void ac_pair_finish(u32 *cbits, const u32 lane, const int r, const int j, const u32 (&x)[8], const u32 (&v)[8])
{
    u32 acc = 0;
#pragma unroll
    for (int q = 0; q < 8; ++q)
        acc = __builtin_amdgcn_alignbit(v[q] >> (x[q] & 31u), acc, 1u);
    reinterpret_cast<uint8_t *>(cbits)[(u32)r * (kSegBytes / 16) + (u32)j * kWave + lane] = (uint8_t)(acc >> 24); // bit q <-> tested position 2q + 1
}
// A full round of the pair filter without -c: pair layout, software-pipelined over the cells of the round: the table reads of cell j + 1 are issued before the
// results of cell j are consumed, so a wave waits for LDS once per round instead of once per cell (the LDS pipe
// is ~50 % busy with 4 waves per SIMD: the exposed read latency, not its throughput, was the limit).
template <int ANCH>
__device__ __forceinline__ void ac_pair_round(u32 *cbits, const u32 lane, const int r, uint4 (&d)[kCells], const uint4 *nsrc, u32 &before)
{
    u32 xs[2][8], dw[2][8];
    ac_pair_issue<ANCH>(0, d, nsrc, before, xs[0], dw[0]);
#pragma unroll
    for (int j = 0; j < kCells; ++j)
    {
        if (j + 1 < kCells)
            ac_pair_issue<ANCH>(j + 1, d, nsrc, before, xs[(j + 1) & 1], dw[(j + 1) & 1]);
        __builtin_amdgcn_sched_barrier(0);
        ac_pair_finish(cbits, lane, r, j, xs[j & 1], dw[j & 1]);
        __builtin_amdgcn_sched_barrier(0);
    }
}
// A full round of the other filters (stride 1, -c), cell by cell; never anchored: ANCH implies the pair filter without -c (ac_pair_round).
// straight-line: no branch between a prefetch and the next cell's read of d[]
template <bool LINES, int STRIDE>
__device__ __forceinline__ void ac_cell_round(const AcArgs &a, const AcWave &wv, const u32 lane, const int r, const u64 seg, const bool interior,
                                              uint4 (&d)[kCells], const uint4 *nsrc, u32 &before)
{
    constexpr bool PAIR = STRIDE == 2;
#pragma unroll
    for (int j = 0; j < kCells; ++j)
    {
        u32 W[5];
        W[1] = d[j].x; W[2] = d[j].y; W[3] = d[j].z; W[4] = d[j].w;
        if (j < ac_roll_cells(LINES, STRIDE, 0))
            d[j] = nsrc[j * kWave];
        // the class word of the 4 bytes in front of the lane = the left neighbour's last one: a DPP wave shift
        // (lane 0 keeps `old` = the classes of `before`, uniform: scalar ALU) — no LDS permute, no branch
        const u32 c4 = PAIR ? ac_pair(W[4]) : ac_cls4(W[4]);
        const u32 cb = PAIR ? ac_pair(before) : ac_cls4(before);
        const u32 c0 = (u32)__builtin_amdgcn_update_dpp((int)cb, (int)c4, 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
        W[0] = 0;
        before = __builtin_amdgcn_readlane(W[4], 63); // the next cell's (and round's) left neighbour
        ac_filter_cell<LINES, STRIDE, 0>(a, wv, lane, r, j, seg, interior, W, true, c0, c4);
    }
}
// the ragged end of the text: bytewise, bounds-checked
template <bool LINES, int STRIDE, int ANCH>
__device__ __forceinline__ void ac_ragged_round(const AcArgs &a, const AcWave &wv, const u32 lane, const int r, const u64 seg, const bool interior)
{
#pragma unroll
    for (int j = 0; j < kCells; ++j)
    {
        const u64 lbase = seg + (u64)j * kCellBytes + (u64)lane * 16u;
        u32 W[5];
#pragma unroll
        for (int w = 0; w < 5; ++w)
        {
            u32 v = 0;
            for (int b = 0; b < 4; ++b)
            {
                const u64 o = lbase + (u64)(w * 4 + b);
                if (o >= 4 && o - 4 < a.text_len)
                    v |= (u32)a.text[o - 4] << (8 * b);
            }
            W[w] = v;
        }
        ac_filter_cell<LINES, STRIDE, ANCH>(a, wv, lane, r, j, seg, interior, W, false, 0u, 0u);
    }
}

// ---------------------------------------------------------------------------------------------- anchored, stage 2: candidates -> END-pair bitmap
// the unit verifies the ends useg + 1 .. useg + 16384 (bit b <-> the pair 2b + 1, 2b + 2), as the end-gram kernel does
__device__ __forceinline__ void ac_anchor_mark(u32 *ebits, const u64 useg, const u64 e)
{
    if (e > useg && e <= useg + kAcUnitBytes)
    {
        const u32 b = (u32)(e - useg - 1u) >> 1;
        atomicOr(&ebits[b >> 5], 1u << (b & 31u));
    }
}
// the candidates of a batch: lane -> tested position (binary search over the owners' prefix sums, then the t-th set bit)
__device__ __forceinline__ void ac_anchor_locate(const AcArgs &a, const u32 *cbits, const u32 lane, const u64 useg, const u32 incl, const u32 mycnt,
                                                 const u32 n, const u32 n_tot, const u32 b0, u64 &t, bool &live, bool &valid)
{
    const u32 qi = b0 + lane;
    live = qi < n;
    const bool isx = qi >= n && qi < n_tot;
    const u32 rel = 2u * ac_nth_set_bit<4u>(cbits, incl, mycnt, qi, live);   // (bit b <-> tested position 2b + 1)
    t = isx ? useg - 11u + 2u * (u64)(qi - n) : useg + rel + 1u; // the tested position (odd)
    valid = (live || isx) && t < a.text_len;
}
// its eight bytes t - 6 .. t + 1 (without the last one where the text ends: one byte lower, shifted back)
__device__ __forceinline__ u64 ac_anchor_fetch(const AcArgs &a, const u64 t, const bool valid)
{
    if (!valid || t < 16u)
        return 0ull;
    const bool hasB = t + 1 < a.text_len;
    const u64 q8 = load_unaligned<u64>(a.text + (t - (hasB ? 6u : 7u)));
    return hasB ? q8 : (q8 >> 8);
}
// the table's answer for the gram whose LAST byte is byte `last` of the window Q (ANCH == 2: with the class of the
// byte in front of the gram, byte last - 4)
template <int ANCH>
__device__ __forceinline__ bool ac_anchor_gram(const u64 Q, const int last)
{
    u32 u = ac_pair((u32)(Q >> (8 * (last - 3))));
    if constexpr (ANCH == 2)
        u = ac_mix5(u, (u32)(Q >> (8 * (last - 4))) & 31u);
    return ac_pair_test<false>(u);
}
// the offset mask of the bucket entry (of two) that holds the exact anchor gram `key` in front of the bytes cx
__device__ __forceinline__ u32 ac_anchor_pick(const uint4 &e0, const uint4 &e1, const u32 key, const u32 cx)
{
    const uint4 &e = (e0.x == key && (e0.y >> 31)) ? e0 : e1;
    return (e.x == key && (e.y >> 31) && ((cx ^ e.z) & e.w) == 0u) ? (e.y & 0x7fffffffu) : 0u;
}
// The stage: the unit's candidates (cbits), 64 at a time, mark the ENDs their anchor grams name in ebits.
template <bool CI, int ANCH>
__device__ __forceinline__ void ac_anchor_stage2(const AcArgs &a, AcWave &wv, const u32 lane, const u64 useg, u32 &acc_cand)
{
    const u32 mycnt = ac_block_popc<4u>(wv.cbits, lane);
    const u32 incl = ac_wave_scan_incl(mycnt); // (on the DPP network: the shuffle version's six address registers spilled in the -i -w instantiations)
    const bool off = (a.flags & (1u << 31)) != 0u; // (ablation hook KREP_GPU_AC_NOVERIFY: filter cost only)
    const u32 n = off ? 0u : __shfl(incl, 63);
    acc_cand += (u32)__builtin_amdgcn_readfirstlane((int)n);
    // an END lies up to 13 bytes behind the tested position that names it: the six tested positions in front of the unit
    // whose ends can fall into it are looked at again here (their own unit drops the ends beyond its last pair)
    const u32 n_x = (!off && useg >= 16u) ? 6u : 0u;
    const u32 n_tot = n + n_x;
    // Two dependent round trips per batch (window, then bucket) and, on a text where most candidates reach their bucket, three
    // or four batches per unit: the NEXT batch's windows are requested before this batch's buckets, so a batch waits once
    u64 tN = 0, QN = 0;
    bool liveN = false, validN = false;
    if (n_tot)
    {
        ac_anchor_locate(a, wv.cbits, lane, useg, incl, mycnt, n, n_tot, 0u, tN, liveN, validN);
        QN = ac_anchor_fetch(a, tN, validN);
    }
    for (u32 b0 = 0; b0 < n_tot; b0 += 64)
    {
        const u64 t = tN, Q = QN;
        const bool live = liveN, valid = validN;
        if (b0 + 64u < n_tot)
        {
            ac_anchor_locate(a, wv.cbits, lane, useg, incl, mycnt, n, n_tot, b0 + 64u, tN, liveN, validN);
            QN = ac_anchor_fetch(a, tN, validN);
        }
        if (a.flags & (1u << 30))
        { // (ablation hook KREP_GPU_AC_NOPROBE: the count that comes back is the number of filter candidates)
            wv.wcnt += (u32)__popcll(__ballot(live));
            continue;
        }
        if (!valid)
            continue;
        if (t < 16u)
        { // (the first bytes of the text: no window in front — every end the position could name)
            for (u32 k = 0; k <= kAnchMaxK + 1u; ++k)
                ac_anchor_mark(wv.ebits, useg, t + k);
            continue;
        }
        const bool hasB = t + 1 < a.text_len;
        // the position's own gram again for the six in front of the unit; then, as in the end-gram kernel: an anchor
        // gram ENDS at t where the window's other gram sits at t - 1, at t + 1 where this one is that other gram
        // (window bytes 0..7 = text bytes t - 6 .. t + 1)
        const bool own_ok = live || ac_anchor_gram<ANCH>(Q, 6);
        const bool liveA = own_ok && ac_anchor_gram<ANCH>(Q, 5);
        const bool liveB = own_ok && hasB && ac_anchor_gram<ANCH>(Q, 7);
        u32 kA = (u32)(Q >> 24), kB = (u32)(Q >> 32); // the exact anchor gram: bytes t - 3 .. t | t - 2 .. t + 1
        if (CI)
        {
            kA = ac_fold4(kA);
            kB = ac_fold4(kB);
        }
        // buckets of two 16-byte entries {exact anchor gram, 1 << 31 | offset mask, the three bytes in front of the
        // 5-byte window, their byte mask}: seven exact bytes decide, all of them in the window already fetched
        u32 cxA = (u32)Q & 0xffffffu, cxB = (u32)(Q >> 8) & 0xffffffu; // bytes a - 6 .. a - 4 of either parity
        if (CI)
        {
            cxA = ac_fold4(cxA);
            cxB = ac_fold4(cxB);
        }
        uint4 a0 = make_uint4(0, 0, 0, 0), a1 = a0, b0_ = a0, b1_ = a0;
        if (liveA)
        {
            const uint4 *bk = a.anch + 2u * (size_t)(((kA * a.anch_mul) >> 9) & a.anch_mask);
            a0 = bk[0];
            a1 = bk[1];
        }
        if (liveB)
        {
            const uint4 *bk = a.anch + 2u * (size_t)(((kB * a.anch_mul) >> 9) & a.anch_mask);
            b0_ = bk[0];
            b1_ = bk[1];
        }
        u32 mA = liveA ? ac_anchor_pick(a0, a1, kA, cxA) : 0u;
        u32 mB = liveB ? ac_anchor_pick(b0_, b1_, kB, cxB) : 0u;
        while (mA)
        {
            ac_anchor_mark(wv.ebits, useg, t + (u32)__builtin_ctz(mA));
            mA &= mA - 1u;
        }
        while (mB)
        {
            ac_anchor_mark(wv.ebits, useg, t + 1u + (u32)__builtin_ctz(mB));
            mB &= mB - 1u;
        }
    }
}

// ---------------------------------------------------------------------------------------------- verify, rank, emit
// the verification of ONE END pair per lane (ends pos and pos + 1): the number of matches at either end, their depth masks (or the
// level walk's verdict) — everything of a verify batch except its ranking and emission
template <bool CI, bool LINES, bool SHORT, int STRIDE, int ANCH, bool WW>
__device__ __forceinline__ void ac_verify_ends(const AcArgs &a, const u64 pos, const bool live, const bool isx, const u64 vuseg, u32 &cA, u32 &cB,
                                               u64 &dmA, u64 &dmB, bool &simA, bool &simB)
{
    constexpr bool PAIR = STRIDE == 2;
    constexpr bool XCAND = ac_xcand(LINES, STRIDE); // (the extra candidate in front of a -c unit, ac_verify_count)
    bool liveA = live, liveB = false;
    if (STRIDE == 2)
        liveA = live && pos >= a.end_lo && pos < a.end_hi;
    if (STRIDE == 2) // a candidate stands for the ends t and t + 1
        liveB = (live || isx) && pos + 1 >= a.end_lo && pos + 1 < a.end_hi &&
                (!XCAND || pos + 1 < vuseg + kAcUnitBytes); // (-c: that end belongs to the next unit's extra candidate)
    cA = cB = 0;
    dmA = dmB = 0;
    simA = simB = false;
    if (STRIDE == 2)
    {
        bool slA = false, slB = false;
        u32 mA = 0, mB = 0;
#ifndef KG_AC_NO_BTEST // (A/B switches of krep_amd/build.py --variant)
        constexpr bool kGram = PAIR && ac_xbits(LINES) == 20 && !ANCH; // the probe asks the class table about both ends (kg_ac_common.h; ANCH: the table holds anchor grams, not end grams)
#else
        constexpr bool kGram = false;
#endif
#ifndef KG_AC_NO_STAGE
        constexpr bool kStaged = kGram;
#else
        constexpr bool kStaged = false;
#endif
        bool exact_done = false;
        if constexpr (ANCH != 0)
#ifndef KG_AC_EXACT_SERIAL
            if (a.xtab && pos >= 15u && (WW || !(a.flags & F_WW))) // (-w: tested inside ac_exact_end2<.., WW>, on the window's own bytes)
#else
            if (a.xtab && !(a.flags & F_WW) && pos >= 15u)
#endif
            {
                // stage 3 through the length-keyed exact dictionary (kg_ac_common.h ac_exact_end): no trie, no chain
                bool muA = false, muB = false;
#ifndef KG_AC_EXACT_SERIAL // (A/B switch of krep_amd/build.py --variant: the two ends one behind the other, as first built)
                if (liveA || liveB)
                    ac_exact_end2<CI, WW>(a, pos, liveA, liveB, mA, mB, muA, muB);
#else
                if (liveA)
                    mA = ac_exact_end<CI>(a, pos, muA);
                if (liveB)
                    mB = ac_exact_end<CI>(a, pos + 1u, muB);
#endif
                mA = ac_own_clip(mA, pos, a.own_lo, a.own_hi);
                mB = ac_own_clip(mB, pos + 1u, a.own_lo, a.own_hi);
                // a `multi` entry (a pattern the dictionary holds twice, or the 16-byte stand-in of a LONGER pattern, kg_ac_anchor.hip
                // exact_table): counted and emitted by the level walk, which owns by the TRUE start.  Decided on the unclipped answer —
                // the clip above takes a stand-in for a 16-byte pattern and would drop a longer one that starts in front of own_hi
                // and ends 16 bytes or more behind it (muA implies a hit, i.e. a mask that was not empty before the clip).
                slA = muA;
                slB = muB;
                exact_done = true;
            }
        if (exact_done)
        {
        }
        else if (!(a.flags & (1u << 30))) // (ablation hook KREP_GPU_AC_NOPROBE: candidate enumeration without the probes)
            ac_walk_probe2<CI, SHORT, kStaged, WW>(a, pos, liveA, liveB, LINES, mA, slA, mB, slB, [&](u32 E) -> bool {
                if constexpr (kGram) // the filter's own lookup for a gram that lies in one dword (ac_cell_pairs, k = 3 mod 4)
                    return ac_pair_test<LINES>(ac_pair(E));
                else
                    return true;
            });
        else
            mA = liveA ? 1u : 0u; // ... and the count that comes back is the number of candidates
        dmA = mA; dmB = mB;
        cA = (u32)__popc(mA); cB = (u32)__popc(mB);
        simA = simB = true;
#ifndef KG_AC_NO_EXACT_SLOW // (A/B switch of krep_amd/build.py --variant)
        if constexpr (!SHORT && ANCH == 0 && !CI) // (-i: eight bytes of scratch per lane in the BASELINE-shaped kernel for a path the anchored instantiations cover)
            if (a.xtab && !(a.flags & F_WW) && pos >= 15u && (slA || slB))
            {
                // an end the chain-compressed entry cannot answer (the trie branches behind its final gram): the exact dictionary
                // instead of the level walk, where there is one (a word-like text, patterns of 4..16 bytes)
                bool mu = false;
                if (slA)
                {
                    const u32 x = ac_exact_end<CI>(a, pos, mu), m = LINES ? x : ac_own_clip(x, pos, a.own_lo, a.own_hi); // (-c owns by END)
                    if (!mu) { mA = m; slA = false; } // (mu: the level walk decides, by the true start — a stand-in's bit 16 is not its length)
                }
                if (slB)
                {
                    const u32 x = ac_exact_end<CI>(a, pos + 1u, mu), m = LINES ? x : ac_own_clip(x, pos + 1u, a.own_lo, a.own_hi);
                    if (!mu) { mB = m; slB = false; }
                }
                dmA = mA; dmB = mB;
                cA = (u32)__popc(mA); cB = (u32)__popc(mB);
            }
#endif
#pragma unroll 1
        for (int e = 0; e < 2; ++e) // the one call site of the level walk
            if (e ? slB : slA)
            {
                u64 dm;
                bool sim;
                const u32 c = ac_walk_slow<CI, SHORT>(a, pos + (u64)e, LINES, dm, sim);
                if (e) { cB = c; dmB = dm; simB = sim; }
                else { cA = c; dmA = dm; simA = sim; }
            }
    }
    else if (liveA)
        cA = ac_walk_fast<CI, SHORT>(a, pos, LINES, dmA, simA);
}

// one record of the unit wv emits into, at rank `at`: a staged word, or (emit pass) the final record
__device__ __forceinline__ void ac_emit_write(const AcArgs &a, const AcWave &wv, const u32 at, const u64 s0, const u32 len)
{
    if (wv.do_stage)
    {
        if (at < a.stage_cap)
            wv.e_slot[at] = ((u32)(s0 + 1024u - wv.e_useg) << 11) | len; // start relative to the unit (>= -1023), length <= 1024
    }
    else
    {
        const u64 g = wv.e_fbase + at;
        if (g < a.pos_cap)
        {
            const u64 st = s0 + a.global_base, en = st + len;
            *reinterpret_cast<uint4 *>(a.positions + 2 * g) = make_uint4((u32)st, (u32)(st >> 32), (u32)en, (u32)(en >> 32));
        }
    }
}
// the matches of one batch (one END pair per lane: cA at pos, cB at pos + 1, depth masks or the level walk's verdict):
// unit-local ranks by a wave prefix, then staging slots / final records / the -c hit bitmap, longest first at one end
// (what an emission refers to: wv.e_* — this unit, or, for the deferred stage 3 of the anchored scan, the unit a pending pair belongs to)
template <bool CI, bool LINES, bool SHORT, int STRIDE>
__device__ __forceinline__ void ac_rank_and_emit(const AcArgs &a, AcWave &wv, const u32 lane, const u64 pos, const u32 cA, const u32 cB, const u64 dmA,
                                                 const u64 dmB, const bool simA, const bool simB)
{
    const u32 c = cA + cB;
    const u32 incl = ac_shfl_scan_incl(c, lane);
    const u32 rank0 = wv.wcnt + incl - c;
    wv.wcnt += __shfl(incl, 63);
#pragma unroll 1
    for (int e = 0; e < (STRIDE == 2 ? 2 : 1); ++e)
    {
        const u32 ce = e ? cB : cA;
        if (!ce)
            continue;
        const u64 pe = pos + (u64)e, dme = e ? dmB : dmA;
        const u32 re = rank0 + (e ? cA : 0u), rele = (u32)(pe - wv.e_useg); // the END's bit in the unit's hit bitmap
        const bool sime = e ? simB : simA;
        if (LINES)
            atomicOr(&wv.bitmap[rele >> 5], 1u << (rele & 31u));
        if (wv.do_stage || wv.do_final)
        {
            if (sime)
            {
                u32 at = re;
                for (u64 rest = dme; rest;) // longest first
                {
                    const u32 d = 63u - (u32)__builtin_clzll(rest);
                    rest &= ~(1ull << d);
                    ac_emit_write(a, wv, at++, pe + 1 - (u64)d, d);
                }
            }
            else
                ac_walk<CI, true, !SHORT>(a, pe, ce, [&](u32 r, u64 s2, u32 len) { ac_emit_write(a, wv, re + r, s2, len); });
        }
    }
}

// ---------------------------------------------------------------------------------------------- the verify loop of a unit, plain and pending
// (bit b of a unit's END bitmap <-> the pair 2b + 1, 2b + 2; a pending pair: unit of the ticket << 14 | b)
__device__ __forceinline__ u64 ac_pend_pos(const AcArgs &a, const u64 u_begin, const u32 pend)
{
    return a.anchor + (u_begin + (u64)(pend >> 14)) * (u64)kAcUnitBytes + ((pend & 0x3fffu) << 1) + 1u;
}
// the verify batch of the first `cnt` lanes' pending pairs, ranked and emitted unit by unit
template <bool CI, bool LINES, bool SHORT, int STRIDE, int ANCH, bool WW>
__device__ __forceinline__ void ac_pend_flush(const AcArgs &a, AcWave &wv, const u32 lane, const u32 cnt, const u32 pend, u32 &ucnt, const u64 u_begin,
                                              const bool defer, const bool parked)
{
    const bool live = lane < cnt;
    u32 cA, cB;
    u64 dmA, dmB;
    bool simA, simB;
    ac_verify_ends<CI, LINES, SHORT, STRIDE, ANCH, WW>(a, ac_pend_pos(a, u_begin, pend), live, false, 0ull, cA, cB, dmA, dmB, simA, simB);
    const u32 cc = cA | (cB << 8);
    const u32 v0 = (u32)__builtin_amdgcn_readfirstlane((int)(pend >> 14)), v1 = (u32)__builtin_amdgcn_readlane((int)(pend >> 14), (int)(cnt - 1u));
    for (u32 v = v0; v <= v1; ++v) // (uniform: the units the batch spans, ascending; not deferred: this unit)
    {
        const bool in = live && (pend >> 14) == v;
        if (!__ballot(in))
            continue;
        if (defer)
        {
            wv.e_useg = a.anchor + (u_begin + (u64)v) * (u64)kAcUnitBytes;
            wv.e_slot = parked ? wv.park_slots + v * 16u : reinterpret_cast<u32 *>(a.stage) + (u_begin + (u64)v) * (u64)a.stage_cap;
            wv.wcnt = (u32)__builtin_amdgcn_readlane((int)ucnt, (int)v);
        }
        ac_rank_and_emit<CI, LINES, SHORT, STRIDE>(a, wv, lane, ac_pend_pos(a, u_begin, pend), in ? (cc & 0xffu) : 0u, in ? (cc >> 8) : 0u, dmA, dmB, simA, simB);
        if (defer && lane == v)
            ucnt = wv.wcnt;
    }
    if (defer)
        wv.wcnt = 0;
}
// the marked pairs per lane (four dwords of the bitmap each), their inclusive prefix and their number
__device__ __forceinline__ void ac_pend_recount(const AcArgs &a, const u32 *vbits, const u32 lane, u32 &mycnt, u32 &incl, u32 &n)
{
    mycnt = ac_block_popc<4u>(vbits, lane);
    incl = ac_wave_scan_incl(mycnt);
    n = (a.flags & (1u << 31)) ? 0u : (u32)__builtin_amdgcn_readlane((int)incl, 63); // (ablation hook KREP_GPU_AC_NOVERIFY: filter cost only)
}
// ANCH, stage 3 DEFERRED over the ticket (round 6): a unit of word text marks ~6 END pairs — a verify batch of 6 lanes that waits
// for three dependent round trips (window, length masks, bucket) like a full one.  The marked pairs of the ticket's units are
// collected instead — one per lane in `pend` (unit of the ticket << 14 | pair), verified when 64 are there or the ticket ends —
// and the units' match counts wait in lanes 0..7 of `ucnt` until the ticket's info words are written.  Ranking and emission
// stay per unit, in END order: the pairs arrive unit by unit, ascending.
// (The end-gram kernel with the pipelined pair filter can do the same with its CANDIDATES — -DKG_AC_DEFER_GENERIC — and is slower with
//  it: BASELINE config 4 holds ~40 candidates per unit, its batches are two thirds full already, and a batch that spans two units
//  ranks and emits twice: 6.45-6.54 ms against 6.32-6.40 in alternating runs on one box.  Off.)
template <bool CI, bool LINES, bool SHORT, int STRIDE, int ANCH, bool WW>
__device__ __forceinline__ void ac_pend_unit(const AcArgs &a, AcWave &wv, const u32 lane, const u32 *vbits, const u64 unit, const u64 u_begin,
                                             const u64 u_end, const bool defer, const bool parked, u32 &pend, u32 &npend, u32 &ucnt, u32 &acc_cand)
{
    if (ANCH != 0 && (a.flags & (1u << 28))) // (ablation hook KREP_GPU_AC_NOSTAGE3: the anchor stage alone; the count is the number of marked END pairs)
    {
        wv.wcnt += (u32)__builtin_amdgcn_readlane((int)ac_wave_scan_incl(ac_block_popc<4u>(wv.ebits, lane)), 63);
        *reinterpret_cast<uint4 *>(wv.ebits + lane * 4u) = make_uint4(0u, 0u, 0u, 0u);
    }
    else if (ANCH == 0 || !(a.flags & (1u << 30)))
    {
        // ---- the unit's marked pairs (end-gram kernel: its candidates) join the pending ones; 64 pending pairs are a verify batch.  Deferred: what is left waits for the
        //      ticket's next unit; otherwise (emit mode, -w, no exact dictionary) it is verified here, at the unit's end ----
        // (registers: nothing of the collection below lives across a batch, and a pair's position is re-derived from its `pend` word —
        //  kept live they cost the anchored instantiations 20-28 B/lane of scratch, whose reloads drain the text prefetch)
        const u32 uv = (u32)(unit - u_begin);
        u32 n = 0, mycnt = 0, incl = 0;
        ac_pend_recount(a, vbits, lane, mycnt, incl, n);
        if (ANCH == 0)
            acc_cand += n;
        u32 taken = 0;
        do // (ONE call site of the verify batch: it is inlined, and two copies cost the anchored instantiations 12-20 B/lane of scratch)
        {
            const u32 room = 64u - npend, take = room < n - taken ? room : n - taken;
            const bool mine = lane >= npend && lane < npend + take;
            const u32 b = ac_nth_set_bit<4u>(vbits, incl, mycnt, mine ? taken + (lane - npend) : 0u, mine);
            if (mine)
                pend = (uv << 14) | b;
            npend += take;
            taken += take;
            if (npend == 64u || (taken >= n && npend && (!defer || unit + 1 == u_end)))
            {
                ac_pend_flush<CI, LINES, SHORT, STRIDE, ANCH, WW>(a, wv, lane, npend, pend, ucnt, u_begin, defer, parked);
                npend = 0;
                if (taken < n)
                    ac_pend_recount(a, vbits, lane, mycnt, incl, n); // (see ac_pend_flush)
            }
        } while (taken < n);
        if (ANCH != 0 && n) // (wave-uniform) the END-pair bitmap is the next unit's again
        {
            // (the zeros are made HERE: as a loop-invariant uint4 they were kept in four registers from the kernel's start, spilled,
            //  and reloaded in front of this store — a scratch load whose wait drained the text prefetch once per unit)
            u32 z;
            asm volatile("v_mov_b32 %0, 0" : "=v"(z));
            *reinterpret_cast<uint4 *>(wv.ebits + lane * 4u) = make_uint4(z, z, z, z);
        }
    }
}
// ---- verify (and stage/emit) the candidates, 64 at a time, one per lane.  Lane L owns the 256 positions
//      [256 L, 256 L + 256) of the bitmap (8 dwords; pipelined pair filter: 4); a wave scan of the popcounts gives every lane its rank
//      range, and the lane verifying rank q finds its candidate by a binary search over those sums and a
//      select of the t-th set bit in the owner's block (ac_nth_set_bit) ----
// (The loop over a unit's batches is the kernel's: inside a function here it cost the two -c -w instantiations two VGPRs, 103 -> 105.)
// the unit's candidates: per lane (mycnt), their inclusive prefix over the lanes, their number n; n_tot counts the extra candidate
template <bool LINES, int STRIDE>
__device__ __forceinline__ void ac_verify_count(const AcArgs &a, const u32 *vbits, const u32 lane, const u64 useg, u32 &mycnt, u32 &incl, u32 &n, u32 &n_tot)
{
    mycnt = ac_block_popc<ac_wpl(LINES, STRIDE)>(vbits, lane);
    incl = ac_shfl_scan_incl(mycnt, lane); // inclusive prefix of the candidate counts over lanes
    n = (a.flags & (1u << 31)) ? 0u : __shfl(incl, 63); // (ablation hook KREP_GPU_AC_NOVERIFY: filter cost only)
    n_tot = n + ((ac_xcand(LINES, STRIDE) && !(a.flags & (1u << 31)) && useg >= 1u) ? 1u : 0u); // rank n: the extra candidate
}
// the batch of the candidates b0 .. b0 + 63: located, verified, ranked and emitted (never anchored: those instantiations pend)
template <bool CI, bool LINES, bool SHORT, int STRIDE, bool WW>
__device__ __forceinline__ void ac_verify_batch(const AcArgs &a, AcWave &wv, const u32 lane, const u32 *vbits, const u64 useg, const u32 mycnt,
                                                const u32 incl, const u32 n, const u32 n_tot, const u32 b0)
{
    constexpr bool PAIR = STRIDE == 2, PIPE = PAIR && !LINES;
    const u32 qi = b0 + lane;
    const bool live = qi < n;
    const bool isx = ac_xcand(LINES, STRIDE) && qi == n && qi < n_tot;
    const u32 b = ac_nth_set_bit<ac_wpl(LINES, STRIDE)>(vbits, incl, mycnt, qi, live);
    const u32 rel = PIPE ? 2u * b : b; // (pipelined pair filter: bit b <-> tested position 2b + 1)
    // pair layout: bit j of the bitmap is tested position j + 1
    const u64 pos = isx ? useg - 1u : useg + rel + (PAIR ? 1u : 0u);
    u32 cA, cB;
    u64 dmA, dmB;
    bool simA, simB;
    ac_verify_ends<CI, LINES, SHORT, STRIDE, 0, WW>(a, pos, live, isx, useg, cA, cB, dmA, dmB, simA, simB);
    ac_rank_and_emit<CI, LINES, SHORT, STRIDE>(a, wv, lane, pos, cA, cB, dmA, dmB, simA, simB);
}

// ---------------------------------------------------------------------------------------------- the unit's and the ticket's results
// -c: the distinct lines of the unit that hold a match END, from its hit and newline bitmaps; the hit bitmap is the next unit's again
__device__ __forceinline__ LineState ac_unit_lines(const AcWave &wv, const u32 lane)
{
    const LineState ls = ac_line_pass(kAcRounds * kCells, [&](int rj, u32 &H, u32 &N) {
        const u32 bitoff = (u32)rj * kCellBytes + lane * 16u;
        H = (wv.bitmap[bitoff >> 5] >> (bitoff & 31u)) & 0xffffu;
        N = wv.nlmap[bitoff >> 4];
    });
    for (u32 w = lane; w < kAcBitmapWords; w += 64)
        wv.bitmap[w] = 0u;
    return ls;
}
// info word of a records / counts unit with `cnt` matches
__device__ __forceinline__ u64 ac_count_info(const u32 cnt) { return (u64)cnt | (cnt ? (kLnHead | kLnTail) : 0ull); }
// a unit whose `cnt` matches do not fit its staging slot: the emit pass scans it again
__device__ __forceinline__ void ac_report_overflow(const AcArgs &a, const u32 cnt)
{
    if (cnt > a.stage_cap)
    {
        atomicAdd(&a.ctr->overflow_units, 1ull);
        atomicMax(&a.ctr->max_unit_count, (u64)cnt);
    }
}
// the unit's info word (one lane): to its place, or parked until the ticket's end
template <bool LINES>
__device__ __forceinline__ void ac_unit_info(const AcArgs &a, const AcWave &wv, const u64 unit, const u64 u_begin, const bool parked, const bool want_pos,
                                             const LineState &wls)
{
    const u64 info = LINES ? ((u64)wv.wcnt | line_bits(wls) | ((u64)(wls.cnt & kUiLineMask) << kUiLineShift)) : ac_count_info(wv.wcnt);
    if (parked)
        wv.park_info[(u32)(unit - u_begin)] = info;
    else
        a.unitinfo[unit] = info;
    if (want_pos)
        ac_report_overflow(a, wv.wcnt);
}
// deferred stage 3: the ticket's `nun` units, their counts from lanes 0..7 of `ucnt` (returns their sum), their info words in one store
template <bool PARKS>
__device__ __forceinline__ u32 ac_ticket_info(const AcArgs &a, const AcWave &wv, const u32 lane, const u64 u_begin, const u32 nun, const u32 ucnt,
                                              const bool chain, const bool want_pos)
{
    const u32 c = lane < nun ? ucnt : 0u;
    const u32 sum = (u32)__builtin_amdgcn_readlane((int)ac_wave_scan_incl(c), 63); // (lanes 0..7 hold the counts; on the DPP network: no address registers)
    if (chain && lane < nun)
    {
        u32 l2 = lane;
        asm volatile("" : "+v"(l2)); // (the address is formed here, not kept — and spilled — from the kernel's start)
        if (PARKS && a.stage_cap == 16u) // (parked: written with the ticket's slots, ac_ticket_unpark)
            wv.park_info[l2] = ac_count_info(c);
        else
            a.unitinfo[u_begin + l2] = ac_count_info(c);
        if (want_pos)
            ac_report_overflow(a, c);
    }
    return sum;
}
// the ticket's parked info words and slots (consecutive units: one contiguous 64-byte-per-unit region), two stores
__device__ __forceinline__ void ac_ticket_unpark(const AcArgs &a, const AcWave &wv, const u32 lane, const u64 u_begin, const u32 nun, const bool want_pos)
{
    u32 l3 = lane;
    asm volatile("" : "+v"(l3)); // (the two addresses are formed here, not kept — and spilled — from the kernel's start)
    if (l3 < nun)
        a.unitinfo[u_begin + l3] = wv.park_info[l3];
    if (want_pos && l3 < nun * 4u)
        reinterpret_cast<uint4 *>(reinterpret_cast<u32 *>(a.stage) + u_begin * 16u)[l3] = reinterpret_cast<const uint4 *>(wv.park_slots)[l3];
}

} // namespace kg
