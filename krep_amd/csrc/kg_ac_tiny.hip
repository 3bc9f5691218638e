// kg_ac_tiny.hip — the multi-pattern scan (aho_corasick_search, /root/reference/aho_corasick.c:303-463) for TINY dictionaries:
// every pattern 1..4 bytes long, at most kTinyPer patterns of each length, no duplicates (`-e he -e she -e hers`, `-e e -e t`).
//
// The general kernel (kg_ac.hip) looks every text position up in LDS tables and verifies candidates through hash probes: with
// 1-3-byte patterns that is 2-3 table reads per position at stride 1 (the LDS pipe saturates near 3 TB/s) and, for a dense
// dictionary, a memory round trip per hit.  Here the dictionary lives in SCALAR registers and the text is compared in vector
// registers, four positions per dword:
//   X_j = the lane's 16 bytes shifted by j bytes (byte e of X_j is text[e - j]; 3 x 4 v_alignbyte per 1-KiB cell),
//   a pattern c_0 .. c_{L-1} ends at byte e  <=>  byte e of  V = (X_{L-1} ^ c_0c_0c_0c_0) | ... | (X_0 ^ c_{L-1}...)  is zero,
//   one exact zero-byte test per pattern and dword (eq_bytes), OR-ed into one flag word per LENGTH and dword.
// What a cell leaves depends on what the scan is for (template parameters):
//   * a count (`KEEP = false`): the popcounts of the flag words — no LDS at all, 12 waves per CU;
//   * records (`KEEP`): per lane-cell the four lengths' 16-bit masks in a scrambled order that costs 4 shifts instead of 4
//     multiplies (bit 8 b + w <-> position 4 w + b), 8 KiB of LDS per wave.  Once per 16-KiB unit a wave prefix of the per-lane
//     popcounts ranks the matches, and every lane walks the lane-cells it owns — END ascending, longest first, as the automaton's
//     output chain reports them (aho_corasick.c:383-437) — into the unit's staging slot, parked in LDS until the ticket ends;
//   * `-c` (`LINES`, never with `KEEP` since round 5): the END mask and the newline mask of the cell in position order, consumed
//     where they are — the carry chain of ac_line_pass (kg_ac_common.h) in the cell; nothing goes to LDS;
//   * the emit-mode launch (`EMIT`): final records for the units whose matches did not fit their slot — or for every unit of a
//     plan that turned out dense (ac_scan: count pass, offsets from the post-pass, this launch) — 2048 at a time through LDS so
//     that consecutive lanes store consecutive records.
// No candidates, no probes, no text gathers.  Units, staging slots, info words, emit mode and the post-pass are those of the
// general kernel (ac_scan drives both); workgroups of 4 waves (256 threads), as many per CU as registers and LDS allow.
#include <algorithm>
#include <atomic>
#include <type_traits>
#include <utility>

#include "kg_ac_common.h"
#include "kg_internal.h"
#include "kg_tickets.h"

namespace kg {

bool ac_tiny_keeps(const AcArgs &a);
extern int g_s1_force_grid; // (kg_single.hip)
#ifndef KG_TINY_KEEP_WAVES
#define KG_TINY_KEEP_WAVES 2
#endif
#ifndef KG_TINY_FUSED_WAVES
#define KG_TINY_FUSED_WAVES 3
#endif
#ifndef KG_TINY_FIVE_WAVES
#define KG_TINY_FIVE_WAVES 2 // (a fifth class: under the 168 registers of 3 waves per SIMD those instantiations spill 144-176 bytes per lane)
#endif
#ifndef KG_TINY_ROLL_CELLS
#define KG_TINY_ROLL_CELLS 6
#endif
#ifndef KG_TINY_LINES_WAVES
#define KG_TINY_LINES_WAVES 3
#endif
#ifndef KG_TINY_COUNT_WAVES
#define KG_TINY_COUNT_WAVES 3
#endif
#define KG_TINY_KEEP_WAVES_ARG ((KEEP && !EMIT) ? KG_TINY_KEEP_WAVES : (FIVE ? KG_TINY_FIVE_WAVES : (FUSED ? KG_TINY_FUSED_WAVES : (LINES ? KG_TINY_LINES_WAVES : KG_TINY_COUNT_WAVES))))
// FUSED (round 5): records in ONE pass and nothing else — no masks kept per unit, no staging slot, no info word, no post-pass.
// A lane-cell that holds a match leaves ONE item in the wave's LDS ring — its two length words and its index in the ticket,
// 12 bytes, ranked by a single ballot; the matches themselves are only counted (a per-lane sum, reduced once per ticket).  The
// ticket's count is published, a resolver wave turns the counts into prefixes (kg_tickets.h, kg_single.hip's scheme), and a ticket
// later the wave expands the parked items DENSELY — 64 items at a time, one per lane, a wave prefix of their match counts — into
// records at their final index, END ascending and longest first.  (Decoding a cell's matches where they are found, as the first
// version did, runs the walk with 1-2 of 64 lanes active in 70 % of the cells: 3.5 TB/s, no faster than the staging road.)
// The streaming KEEP instantiation keeps a unit's length words in 8 KiB of LDS per wave, walks them once per unit and needs 200
// VGPRs (2 waves per SIMD).  A ticket with more match-holding lane-cells than the ring has room for is counted, not recorded
// (ctr->overflow_units): the host falls back to the staging road (ac_scan).
constexpr int kTinyBlock = kTinyWaves * 64;
constexpr u32 kTinyEntries = kAcUnitBytes / 16; // lane-cells of a unit (1024)

template <int... J, typename F>
__device__ __forceinline__ void tiny_static_for(std::integer_sequence<int, J...>, F &&f)
{
    (f(std::integral_constant<int, J>{}), ...);
}
__device__ __forceinline__ u32 tiny_scramble16(u32 m) // position-ordered 16 bits -> bit 8 b + w for position 4 w + b
{
    u32 f = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w)
        f |= ((((m >> (4 * w)) & 0xfu) * 0x00204081u) & 0x01010101u) << w;
    return f;
}

// KEEP: the masks of a unit go to LDS (records are wanted, or -c counts lines); without it only their popcounts matter
// EMIT: the emit-mode launch (final records of the units whose matches did not fit their staging slot; its own instantiation
// because its record walk holds a unit's 32 length words in registers — in the streaming launch those registers spilled, and a
// scratch reload waits in the same in-order vmcnt queue as the prefetched text: the pipeline drained once per unit)
// LONG: the dictionary holds a long length (AcTiny::llong) — its own instantiations, so that the others carry none of its code
// FIVE: 4-byte patterns AND a long length (AcTiny::five): the long patterns are a fifth class.  Shipped for case-sensitive
// COUNTING only (168 VGPRs, 3 waves per SIMD: `if else while` 3.4 -> 4.2 TB/s).  Its one-pass and -i instantiations were built and
// measured slower than the general kernel at the 2 waves per SIMD they need (one pass: 211-217 VGPRs, `if else while` 2.8 against
// 3.3 TB/s with offsets; -i: 173 VGPRs, 3.0 against 3.4 TB/s — DESIGN.md 4.2b): they are not dispatched, and the kernel holds no code
// for them (static_assert below)
// DENSE (with FUSED): the one-pass writer for texts on which most lane-cells hold a match (`-e a -e Sherlock`: 3.5 % of the bytes,
// 577 matches per 16-KiB unit — 440 twelve-byte items, three units and the ring is full).  The matches are decoded WHERE THEY ARE
// FOUND — at that density a third of the lanes walk, not one in sixty — into 16-bit ring entries, the END's offset in the unit and a
// two-bit length code, ranked by ballot bit-planes: kg_single.hip's ring with this kernel's compare in front.  Tickets of 1..4
// units, chosen by the host from the density a scan counted (ac_scan).
template <bool CI, bool LINES, bool KEEP, bool EMIT, bool LONG, bool FUSED = false, bool FIVE = false, bool DENSE = false>
__global__ __launch_bounds__(kTinyBlock, KG_TINY_KEEP_WAVES_ARG) void ac_tiny_kernel(const AcArgs a, const AcTiny td)
{
    static_assert(!DENSE || (FUSED && !FIVE), "DENSE is a flavour of the one-pass writer");
    extern __shared__ __attribute__((aligned(16))) u32 s_tiny[];
    const u32 lane = lane_id(), wave = threadIdx.x >> 6;
    static_assert(!FUSED || (!LINES && !KEEP && !EMIT), "the one-pass record writer is its own mode");
    static_assert(!FIVE || (!CI && !LINES && !KEEP && !EMIT && !LONG && !FUSED), "a fifth class: the case-sensitive count only");
    if constexpr (FUSED)
    {
        // the resolver: whichever wave 0 of a block gets here first (a wave that runs, whatever part of the grid is resident)
        bool resolver = false;
        if (__builtin_amdgcn_readfirstlane(wave) == 0u)
            resolver = wave_fetch_add(&a.ctr->pad[0], 1ull, lane) == 0ull;
        if (resolver)
        {
            tk_resolve(a.tk_agg, a.tk_pref, a.n_tk, a.ctr, lane);
            return;
        }
    }
    // per wave, records: the length words per lane-cell (8 KiB)
    //           + the staging slots (<= 64 words) and info words of a ticket's <= 8 units, parked until the ticket ends: a wave
    //           stores nothing while it streams (on gfx9 a store waits in the same in-order vmcnt queue as the prefetched loads)
    constexpr u32 kPark = kAcUnitsPerTicketMax * 64 + kAcUnitsPerTicketMax * 2;
    constexpr u32 kPerWave = FUSED ? kTinyRing * 3u : kTinyEntries * 2 + kPark;
    u32 *base = s_tiny + wave * kPerWave;
    u32 *park_slots = base + kTinyEntries * 2;                                                     // [unit of the ticket][64]
    u64 *park_info = reinterpret_cast<u64 *>(base + kTinyEntries * 2 + kAcUnitsPerTicketMax * 64); // [unit of the ticket]
    uint2 *cw = reinterpret_cast<uint2 *>(base);

    const bool want_pos = (a.flags & F_POS) != 0;
    const bool chain = !FUSED && (want_pos || LINES); // (the one-pass writer publishes per ticket, not per unit)
    constexpr bool emit_final = EMIT; // (== a.emit_mode != 0: ac_tiny_launch)
    // ---- FUSED: the wave's ring (length words | lane-cell index) and the ticket whose items still wait in it (uniform)
    uint2 *ring_m = reinterpret_cast<uint2 *>(base);
    u32 *ring_id = base + 2u * kTinyRing;
    bool pend = false, overflowed = false;
    u64 pend_t = 0;
    u32 pend_at = 0, pend_items = 0, wp = 0; // ring position / items of the waiting ticket; write position (modulo kTinyRing at use)
    u32 f_at = 0, f_room = 0, f_items = 0;   // the ticket being scanned: where its items start, how many fit, how many it holds so far
    u32 lane_cnt = 0;                        // ... and this LANE's matches in it (summed over the wave when the ticket ends)
    // DENSE: 16-bit entries (END offset in the unit << 2 | length code) in the same 12 KiB; f_items / pend_items count MATCHES, and
    // the matches of the ticket's first three units tell a record's unit (as in kg_single.hip)
    constexpr u32 kDenseRing = kTinyRing * 6u; // entries
    unsigned short *ring16 = reinterpret_cast<unsigned short *>(base);
    u32 u_c0 = 0, u_c1 = 0, u_c2 = 0, u_before = 0, pend_c0 = 0, pend_c1 = 0, pend_c2 = 0;
    auto dwrap = [](const u32 x) -> u32 { return x >= kDenseRing ? x - kDenseRing : x; };
    auto flush_dense = [&](const u32 l4) __attribute__((always_inline)) {
        const u64 first = tk_wait_prefix(a.tk_pref, pend_t, a.ctr, lane);
        const u64 tbase = a.anchor + pend_t * (u64)a.upt * kAcUnitBytes + a.global_base + 1u; // (+1: one past the END)
        const u32 b1 = pend_c0, b2 = pend_c0 + pend_c1, b3 = pend_c0 + pend_c1 + pend_c2;
        const u32 pad = (u32)(first & 7ull); // lanes <-> record indices rounded down to a 128-byte line (kg_single.hip)
        for (u32 g = lane; g < pend_items + pad; g += 64u)
        {
            if (g < pad)
                continue;
            const u32 i = g - pad;
            const u32 ent = ring16[dwrap(pend_at + i)];
            const u32 unit = (i >= b1 ? 1u : 0u) + (i >= b2 ? 1u : 0u) + (i >= b3 ? 1u : 0u);
            const u64 idx = first + i;
            if (idx < a.pos_cap)
            {
                const u32 code = ent & 3u, len = code == 3u ? l4 : code + 1u;
                const u64 en = tbase + (u64)unit * kAcUnitBytes + (ent >> 2), st = en - len;
                typedef u32 u32x4 __attribute__((ext_vector_type(4)));
                const u32x4 rec = {(u32)st, (u32)(st >> 32), (u32)en, (u32)(en >> 32)};
                __builtin_nontemporal_store(rec, reinterpret_cast<u32x4 *>(a.positions + 2 * idx));
            }
        }
        pend = false;
    };
    // the matches of one lane-cell from its two length words, in the reference's order — END ascending, longest first
    // (aho_corasick.c:383-437): put(position e of the END inside the lane's 16 bytes, length)
    auto walk_lane_cell = [&](const u32 cx, const u32 cy, const u32 l4, auto put) __attribute__((always_inline)) {
        // ENDs of the lane-cell in position order: bit 8 b + w of the any-length word is position 4 w + b
        const u32 hs = (cx | (cx >> 4) | cy | (cy >> 4)) & 0x0f0f0f0fu;
        u32 h = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b)
        { // bit w of the byte's nibble -> bit 4 w + b (shifts and ORs: a multiply would carry where two bits meet)
            const u32 x = (hs >> (8 * b)) & 0xfu;
            h |= ((x | (x << 3) | (x << 6) | (x << 9)) & 0x1111u) << b;
        }
        while (h)
        {
            const u32 e = (u32)__builtin_ctz(h);
            h &= h - 1u;
            const u32 bit = 8u * (e & 3u) + (e >> 2);
            if ((cy >> (bit + 4u)) & 1u) put(e, l4);
            if ((cy >> bit) & 1u) put(e, 3u);
            if ((cx >> (bit + 4u)) & 1u) put(e, 2u);
            if ((cx >> bit) & 1u) put(e, 1u);
        }
    };
    auto flush = [&](const u32 l4) __attribute__((always_inline)) {
        const u64 first = tk_wait_prefix(a.tk_pref, pend_t, a.ctr, lane);
        const u64 tbase = a.anchor + pend_t * (u64)a.upt * kAcUnitBytes + a.global_base;
        u64 run = first; // record index of the batch's first match (uniform)
        for (u32 b0 = 0; b0 < pend_items; b0 += 64u)
        {
            const bool live = b0 + lane < pend_items;
            const u32 slot = (pend_at + b0 + lane) & (kTinyRing - 1u);
            const uint2 m = live ? ring_m[slot] : make_uint2(0u, 0u);
            const u32 id = live ? ring_id[slot] : 0u;
            const u32 c = (u32)(__popc(m.x) + __popc(m.y));
            // exclusive lane prefix of the match counts from ballot bit-planes (an item holds 1-3 matches: two planes as a rule)
            u32 excl = 0, tot = 0;
            auto plane = [&](const int b) __attribute__((always_inline)) {
                const u64 bm = __ballot((c >> b) & 1u);
                excl += mbcnt64(bm) << b;
                tot += (u32)__popcll(bm) << b;
            };
            plane(0);
            plane(1);
            if (__ballot(c > 3u))
            {
                plane(2);
                plane(3);
                if (__ballot(c > 15u))
                {
                    plane(4);
                    plane(5);
                    plane(6);
                }
            }
            u64 idx = run + excl;
            run += tot;
            if (c)
            {
                const u64 end0 = tbase + (u64)id * 16u + 1u; // one past the END at position 0 of the lane-cell
                walk_lane_cell(m.x, m.y, l4, [&](const u32 e, const u32 len) {
                    if (idx < a.pos_cap)
                    {
                        const u64 en = end0 + e, st = en - len;
                        typedef u32 u32x4 __attribute__((ext_vector_type(4)));
                        const u32x4 rec = {(u32)st, (u32)(st >> 32), (u32)en, (u32)(en >> 32)};
                        __builtin_nontemporal_store(rec, reinterpret_cast<u32x4 *>(a.positions + 2 * idx));
                    }
                    ++idx;
                });
            }
        }
        pend = false;
    };
    u64 acc_total = 0; // chain: wave total (uniform); else this LANE's hits (reduced once, at the end)
    u64 ovf_units = 0; // units of this wave whose matches exceeded the staging slot, and the largest such count (lane 0's copy counts)
    u32 ovf_max = 0;
    // LINES without KEEP (round 5): the lines are counted IN the cell — the carry chain of ac_line_pass on the END and newline masks
    // while they are in registers; nothing goes to LDS, no second pass over the unit, 3 waves per SIMD instead of 2
    constexpr bool LINL = LINES && !KEEP;
    static_assert(!EMIT || (KEEP && !LINES), "emit mode writes records");
    static_assert(!(KEEP && LINES), "-c keeps nothing: its lines are counted in the cell");
    u32 k7f;
    asm volatile("v_mov_b32 %0, 0x7f7f7f7f" : "=v"(k7f)); // (a vector register on purpose: see the splats in the cell)
    const u32 lmax = __builtin_amdgcn_readfirstlane(td.lmax), llong = (LONG || FIVE) ? __builtin_amdgcn_readfirstlane(td.llong) : 0u;
    const u32 len4 = (LONG && llong) ? llong : 4u; // the length behind class 4 (a LONG class of 5..8 bytes takes its place: AcTiny)
    const u32 n5 = FIVE ? __builtin_amdgcn_readfirstlane(td.n5) : 0u;
    const u32 n1 = __builtin_amdgcn_readfirstlane(td.n[0]), n2 = __builtin_amdgcn_readfirstlane(td.n[1]),
              n3 = __builtin_amdgcn_readfirstlane(td.n[2]), n4 = __builtin_amdgcn_readfirstlane(td.n[3]);

    for (;;)
    {
        const u64 tk = wave_fetch_add(&a.ctr->ticket, 1ull, lane);
        // (emit mode draws groups of 64 units and looks at all their info words at once: one load per lane and a ballot instead
        //  of a dependent load per unit)
        const u64 upt = EMIT ? 64ull : (u64)a.upt;
        const u64 u_begin = tk * upt;
        if (u_begin >= a.num_tiles)
            break;
        const u64 u_end = (u_begin + upt < a.num_tiles) ? u_begin + upt : a.num_tiles;
        u64 em_mask = 0;
        if (EMIT)
            em_mask = __ballot(u_begin + lane < u_end && (u32)(a.unitinfo[u_begin + lane] & kUiCountMask) > a.stage_cap);
        uint4 d[kCells]; // the round about to be filtered (or on its way)
        // cells of the NEXT round requested while this one is compared (see the round loop)
        constexpr int kRoll = ((FUSED && !DENSE && !FIVE) || (LINES && (CI || LONG)) || (CI && LONG && !KEEP && !FUSED && !LINES)) ? KG_TINY_ROLL_CELLS : kCells;
        bool have = false;
        u32 carry = 0, carry2 = 0;
        if (FUSED)
        {
            f_at = wp;
            f_room = (DENSE ? kDenseRing : kTinyRing) - pend_items; // what this ticket may use while the previous one is still parked
            f_items = 0;
            lane_cnt = 0;
            u_c0 = u_c1 = u_c2 = u_before = 0;
        }
        for (u64 unit = u_begin; unit < u_end; ++unit)
        {
            const u64 useg = a.anchor + unit * (u64)kAcUnitBytes;
            if (emit_final && !((em_mask >> (u32)(unit - u_begin)) & 1ull))
                continue;
            const bool do_final = emit_final && want_pos, do_stage = !emit_final && want_pos;
            u32 *slot = reinterpret_cast<u32 *>(a.stage) + unit * (u64)a.stage_cap;
            // parked: staged matches and info words wait in LDS for the ticket's end (slots beyond 64 entries — a test hook — and
            // tickets beyond 8 units do not fit: they store as they go)
            const bool parked = KEEP && !LINES && do_stage && a.stage_cap <= 64u && a.upt <= kAcUnitsPerTicketMax;
            const u64 fbase = do_final ? a.offsets[unit] : 0ull;
            u32 mycnt = 0; // hits in the lane-cells this lane FILTERED (count-only modes)
            // LINL: the unit's line state (kg_ac_common.h ac_line_pass; l_cnt per lane, the rest uniform)
            u32 l_cnt = 0, s_new = 0;
            bool s_open = false, s_seen = false, s_head = false;
            auto line_cell = [&](const u32 H, const u32 N) __attribute__((always_inline)) {
                const u64 B_any = __ballot(H != 0u), B_nl = __ballot(N != 0u);
                if (!B_any)
                {
                    if (B_nl)
                    {
                        if (!s_seen)
                        {
                            s_head = s_open;
                            s_seen = true;
                        }
                        s_open = false;
                    }
                    return;
                }
                const u32 Hs = H | N;
                l_cnt += (u32)__popc(H & ~(Hs - ((N << 1) & 0xffffu)));    // first match behind each newline of the lane
                const u64 B_head = __ballot((H & (Hs ^ (Hs - 1u))) != 0u); // the lane's lowest flag is a match
                const u64 G = __ballot(H > N), P = ~(B_nl | B_any);        // the highest flag is a match | nothing in the lane
                const unsigned __int128 sum = (unsigned __int128)(G | P) + G + (s_open ? 1u : 0u);
                const u64 O = (u64)sum ^ P; // bit l: the line entering lane l already holds a match
                s_new += (u32)__popcll(B_head & ~O);
                if (!s_seen && B_nl)
                {
                    s_head = (((O | B_head) >> __builtin_ctzll(B_nl)) & 1ull) != 0ull;
                    s_seen = true;
                }
                s_open = (u64)(sum >> 64) != 0ull;
            };

#pragma unroll 1
            for (int r = 0; r < kAcRounds; ++r)
            {
                const u64 seg = useg + (u64)r * kSegBytes;
                const bool fast_now = seg + kSegBytes <= a.text_len;
                // interior: every END of the round lies in the launch's window, and so does the START of a 4-byte match at its
                // first byte (starts own a match outside -c) — nothing to clip
                const bool interior = seg >= a.own_lo + (lmax - 1u) && seg >= a.end_lo && seg + kSegBytes <= a.own_hi && seg + kSegBytes <= a.end_hi;
                const uint4 *src = reinterpret_cast<const uint4 *>(a.text + seg) + lane;
                auto cell = [&](auto interC, const int j, const u32 (&D)[4], const u32 P, const u32 P2) __attribute__((always_inline)) {
                    constexpr bool inter = decltype(interC)::value, kp = KEEP;
                    // The dictionary's shape, re-read through an empty asm in every cell: as loop-invariant booleans the ~20
                    // conditions below were hoisted into 40 scalar registers, spilled to vector lanes and read back with
                    // v_readlane before every branch; as fresh scalars each is one s_cmp in front of its branch.
                    u32 c1 = n1, c2 = n2, c3 = n3, c4 = n4, lmx = lmax, ll = llong;
                    asm volatile("" : "+s"(c1), "+s"(c2), "+s"(c3), "+s"(c4), "+s"(lmx));
                    u32 c5 = n5;
                    if (LONG || FIVE)
                        asm volatile("" : "+s"(ll));
                    if (FIVE)
                        asm volatile("" : "+s"(c5));
                    u32 NL = 0;
                    if (LINES)
                    {
#pragma unroll
                        for (int w = 0; w < 4; ++w)
                            NL |= movemask4(eq_bytes(D[w], 0x0a0a0a0au)) << (4 * w);
                    }
                    // ---- the shifted copies of the lane's bytes: byte e of X[s][w] is text[lane base + 4 w + e - s], as far back
                    //      as the longest pattern reaches (a class that uses X[s] exists only when lmax > s: never read undefined)
                    u32 X[4][4];
#pragma unroll
                    for (int w = 0; w < 4; ++w)
                        X[0][w] = D[w];
                    if (lmx > 1u)
                    {
#pragma unroll
                        for (int w = 0; w < 4; ++w)
                            X[1][w] = __builtin_amdgcn_alignbyte(D[w], w ? D[w - 1] : P, 3u);
                        if (lmx > 2u)
                        {
#pragma unroll
                            for (int w = 0; w < 4; ++w)
                                X[2][w] = __builtin_amdgcn_alignbyte(D[w], w ? D[w - 1] : P, 2u);
                            if (lmx > 3u)
                            {
#pragma unroll
                                for (int w = 0; w < 4; ++w)
                                    X[3][w] = __builtin_amdgcn_alignbyte(D[w], w ? D[w - 1] : P, 1u);
                            }
                        }
                    }
                    // a LONG pattern (5..8 bytes) = its last four bytes ending here AND its first ll - 4 bytes ending one dword
                    // earlier: the same shifted copies one dword to the left, whose first dword comes from the 8 bytes in front
                    u32 XP[4] = {P, 0u, 0u, 0u};
                    if ((LONG || FIVE) && ll)
                    {
                        XP[1] = __builtin_amdgcn_alignbyte(P, P2, 3u);
                        XP[2] = __builtin_amdgcn_alignbyte(P, P2, 2u);
                        XP[3] = __builtin_amdgcn_alignbyte(P, P2, 1u);
                    }
                    // window of the launch (boundary rounds only), per length: the END in [end_lo, end_hi), never before byte L - 1
                    // of the text, and (outside -c, where a match is owned by its start) the START in [own_lo, own_hi)
                    const u32 lrel = (u32)j * kCellBytes + lane * 16u;
                    auto clip = [&](u64 lo, u64 hi) -> u32 {
                        const u32 rlo = lo > seg ? (u32)((lo - seg) < kSegBytes ? (lo - seg) : kSegBytes) : 0u;
                        const u32 rhi = hi > seg ? (u32)((hi - seg) < kSegBytes ? (hi - seg) : kSegBytes) : 0u;
                        const u32 klo = rlo > lrel ? ((rlo - lrel) < 16u ? (rlo - lrel) : 16u) : 0u;
                        const u32 khi = rhi > lrel ? ((rhi - lrel) < 16u ? (rhi - lrel) : 16u) : 0u;
                        return khi > klo ? (((1u << khi) - 1u) & ~((1u << klo) - 1u)) : 0u;
                    };
                    // ---- per length: 0x80 in every byte at which a pattern of that length ENDS.  One pattern = one scalar
                    //      register (its bytes, last one lowest) + under -i one of letter flags; splats on the scalar unit.
                    u32 HA[4] = {0u, 0u, 0u, 0u}, F[4] = {0u, 0u, 0u, 0u}; // any length, per dword | scrambled mask per length
                    // DENSE: the lane-cell's matches as ONE 64-bit word in emission order — bit 4 e + (4 - class) for a match of that
                    // class ending at position e: END ascending, longest class first.  Interior rounds build it per dword (Y[w]: a
                    // nibble per position at bit 8 b, compressed below), boundary rounds from the clipped 16-bit masks.
                    u32 Y[4] = {0u, 0u, 0u, 0u};
                    u64 Bx = 0;
                    u32 m16 = 0;                                           // END mask in position order
                    auto one = [&](auto Lc, u32 (&Z)[4], const bool first, const u32 pk, const u32 lf, const u32 pk2, const u32 lf2,
                                   auto longc) __attribute__((always_inline)) {
                        constexpr int L = decltype(Lc)::value;
                        constexpr bool kLongCls = decltype(longc)::value; // the fifth class: a long pattern's last four bytes
                        // the splats are made on the scalar unit and MOVED to vector registers: v_bitop3_b32 / v_and / v_xor with
                        // vector operands only issue every ~2.2 cycles, with a scalar operand every ~3.7 (profiles/r04_valu_issue_rates.txt)
                        u32 c[L], m[L];
#pragma unroll
                        for (int s = 0; s < L; ++s)
                        {
                            const u32 cs = ((pk >> (8 * s)) & 0xffu) * 0x01010101u;
                            const u32 ms = ((lf >> s) & 1u) * 0x20202020u; // -i: a letter matches both of its cases, (x | 0x20) == c
                            asm volatile("v_mov_b32 %0, %1" : "=v"(c[s]) : "s"(cs));
                            if (CI)
                                asm volatile("v_mov_b32 %0, %1" : "=v"(m[s]) : "s"(ms));
                        }
#pragma unroll
                        for (int w = 0; w < 4; ++w)
                        {
                            u32 V = 0;
#pragma unroll
                            for (int s = 0; s < L; ++s) // s bytes before the end: pattern byte L - 1 - s
                                V |= (CI ? (X[s][w] | m[s]) : X[s][w]) ^ c[s];
                            if (((LONG && L == 4) || kLongCls) && ll) // (uniform) the long pattern's first ll - 4 bytes, one dword earlier
                            {
                                auto xa = [&](const int sa) -> u32 { return w ? X[sa][w ? w - 1 : 0] : XP[sa]; };
                                auto term = [&](const int sa) -> u32 {
                                    const u32 ca = ((pk2 >> (8 * sa)) & 0xffu) * 0x01010101u, ma = ((lf2 >> sa) & 1u) * 0x20202020u;
                                    return (CI ? (xa(sa) | ma) : xa(sa)) ^ ca;
                                };
                                V |= term(0);
                                if (ll > 5u)
                                {
                                    V |= term(1);
                                    if (ll > 6u)
                                    {
                                        V |= term(2);
                                        if (ll > 7u)
                                            V |= term(3);
                                    }
                                }
                            }
                            const u32 z = ~(((V & k7f) + k7f) | V | k7f); // 0x80 in every zero byte, exact (eq_bytes)
                            Z[w] = first ? z : (Z[w] | z);
                        }
                    };
                    auto cls = [&](auto Lc, const u32 n) __attribute__((always_inline)) {
                        constexpr int L = decltype(Lc)::value;
                        if (n) // (uniform, like the three below)
                        {
                            u32 Z[4];
                            one(Lc, Z, true, td.pk[L - 1][0], td.lf[L - 1][0], td.pk2[0], td.lf2[0], std::false_type{});
                            if (n > 1)
                            {
                                one(Lc, Z, false, td.pk[L - 1][1], td.lf[L - 1][1], td.pk2[1], td.lf2[1], std::false_type{});
                                if (n > 2)
                                {
                                    one(Lc, Z, false, td.pk[L - 1][2], td.lf[L - 1][2], td.pk2[2], td.lf2[2], std::false_type{});
                                    if (n > 3)
                                        one(Lc, Z, false, td.pk[L - 1][3], td.lf[L - 1][3], td.pk2[3], td.lf2[3], std::false_type{});
                                }
                            }
                            if (inter)
                            {
                                if constexpr (FUSED && DENSE)
                                {
#pragma unroll
                                    for (int w = 0; w < 4; ++w)
                                        Y[w] |= Z[w] >> (3 + L); // the byte's 0x80 flag -> bit (4 - L) of its nibble
                                }
                                else if (!kp && !FUSED)
                                { // a count: the flags are all that is needed
#pragma unroll
                                    for (int w = 0; w < 4; ++w) // (v_bcnt_u32_b32 adds its second operand: one instruction per dword)
                                        asm("v_bcnt_u32_b32 %0, %1, %0" : "+v"(mycnt) : "v"(Z[w]));
                                    if (LINL) // (the line cell wants the ENDs of every length)
                                    {
#pragma unroll
                                        for (int w = 0; w < 4; ++w)
                                            HA[w] |= Z[w];
                                    }
                                }
                                else
                                { // the length's mask in the scrambled order: 4 shifts instead of 4 multiplies
                                    F[L - 1] = (Z[0] >> 7) | (Z[1] >> 6) | (Z[2] >> 5) | (Z[3] >> 4);
                                }
                            }
                            else
                            {
                                u32 pm = 0;
#pragma unroll
                                for (int w = 0; w < 4; ++w)
                                    pm |= movemask4(Z[w]) << (4 * w);
                                const u64 lm1 = (L == 4 ? (u64)len4 : (u64)L) - 1ull; // (class 4 may stand for a long length)
                                pm &= clip(a.end_lo, a.end_hi) & clip(lm1, ~0ull);
                                if (!LINES)
                                    pm &= clip(a.own_lo + lm1, a.own_hi + lm1);
                                m16 |= pm;
                                if constexpr (FUSED && DENSE)
                                { // bit e -> bit 4 e + (4 - L)
                                    u64 x = pm;
                                    x = (x | (x << 24)) & 0x000000ff000000ffull;
                                    x = (x | (x << 12)) & 0x000f000f000f000full;
                                    x = (x | (x << 6)) & 0x0303030303030303ull;
                                    x = (x | (x << 3)) & 0x1111111111111111ull;
                                    Bx |= x << (4 - L);
                                }
                                else
                                    F[L - 1] = tiny_scramble16(pm);
                                mycnt += (kp || FUSED) ? 0u : (u32)__popc(pm);
                            }
                        }
                    };
                    cls(std::integral_constant<int, 1>{}, c1);
                    cls(std::integral_constant<int, 2>{}, c2);
                    cls(std::integral_constant<int, 3>{}, c3);
                    cls(std::integral_constant<int, 4>{}, c4);
                    if constexpr (FIVE)
                    {
                        if (c5 && ll) // (uniform) the long patterns: last four bytes ending here, the first ll - 4 one dword earlier
                        {
                            u32 Z[4];
                            const std::integral_constant<int, 4> L4{};
                            one(L4, Z, true, td.pk5[0], td.lf5[0], td.pk2[0], td.lf2[0], std::true_type{});
                            if (c5 > 1)
                            {
                                one(L4, Z, false, td.pk5[1], td.lf5[1], td.pk2[1], td.lf2[1], std::true_type{});
                                if (c5 > 2)
                                {
                                    one(L4, Z, false, td.pk5[2], td.lf5[2], td.pk2[2], td.lf2[2], std::true_type{});
                                    if (c5 > 3)
                                        one(L4, Z, false, td.pk5[3], td.lf5[3], td.pk2[3], td.lf2[3], std::true_type{});
                                }
                            }
                            if (inter)
                            {
#pragma unroll
                                for (int w = 0; w < 4; ++w)
                                    asm("v_bcnt_u32_b32 %0, %1, %0" : "+v"(mycnt) : "v"(Z[w]));
                            }
                            else
                            {
                                u32 pm = 0;
#pragma unroll
                                for (int w = 0; w < 4; ++w)
                                    pm |= movemask4(Z[w]) << (4 * w);
                                const u64 lm1 = (u64)ll - 1ull;
                                pm &= clip(a.end_lo, a.end_hi) & clip(lm1, ~0ull) & clip(a.own_lo + lm1, a.own_hi + lm1);
                                mycnt += (u32)__popc(pm);
                            }
                        }
                    }
                    if constexpr (FUSED && DENSE)
                    {
                        u32 Blo, Bhi;
                        if constexpr (inter)
                        {
                            u32 g[4];
#pragma unroll
                            for (int w = 0; w < 4; ++w)
                            { // nibbles at bits 0, 8, 16, 24 -> 16 contiguous bits
                                const u32 t = (Y[w] | (Y[w] >> 4)) & 0x00ff00ffu;
                                g[w] = (t | (t >> 8)) & 0xffffu;
                            }
                            Blo = g[0] | (g[1] << 16);
                            Bhi = g[2] | (g[3] << 16);
                        }
                        else
                        {
                            Blo = (u32)Bx;
                            Bhi = (u32)(Bx >> 32);
                        }
                        const u32 c = (u32)(__popc(Blo) + __popc(Bhi)); // this lane's matches in the cell (<= 64)
                        if (__ballot(c != 0u))
                        {
                            // rank inside the ticket: matches so far (uniform) + exclusive lane prefix, from ballot bit-planes
                            u32 idx = f_items, tot = 0;
                            auto plane = [&](const int b) __attribute__((always_inline)) {
                                const u64 bm = __ballot((c >> b) & 1u);
                                idx += mbcnt64(bm) << b;
                                tot += (u32)__popcll(bm) << b;
                            };
                            plane(0);
                            plane(1);
                            if (__ballot(c > 3u))
                            {
                                plane(2);
                                plane(3);
                                if (__ballot(c > 15u))
                                {
                                    plane(4);
                                    plane(5);
                                    plane(6);
                                }
                            }
                            f_items += tot;
                            // (a ticket that outgrows its room is lost as a whole — counted, not recorded: no per-entry test)
                            if (f_items <= f_room)
                            {
                                // entry = (END offset in the unit << 2) | length code = (lane-cell's first byte << 2) + (bit ^ 3)
                                const u32 e0 = (((u32)r * (kSegBytes / 16) + (u32)j * kWave + lane) * 16u) << 2;
                                u32 slot = dwrap(f_at + idx);
                                auto half = [&](u32 x, const u32 eb) __attribute__((always_inline)) {
                                    while (x)
                                    {
                                        const u32 b = (u32)__builtin_ctz(x);
                                        x &= x - 1u;
                                        ring16[slot] = (unsigned short)(eb + (b ^ 3u));
                                        slot = slot + 1u == kDenseRing ? 0u : slot + 1u;
                                    }
                                };
                                half(Blo, e0);
                                half(Bhi, e0 + 32u);
                            }
                        }
                    }
                    else if constexpr (FUSED)
                    {
                        const u32 cx = F[0] | (F[1] << 4), cy = F[2] | (F[3] << 4);
                        const u32 c = (u32)(__popc(cx) + __popc(cy)); // this lane's matches in the cell
                        lane_cnt += c;
                        const u64 bm = __ballot(c != 0u);
                        if (bm)
                        {
                            const u32 idx = f_items + mbcnt64(bm);
                            if (c && idx < f_room)
                            {
                                const u32 slot = (f_at + idx) & (kTinyRing - 1u);
                                ring_m[slot] = make_uint2(cx, cy);
                                ring_id[slot] = (u32)(unit - u_begin) * kTinyEntries + (u32)r * (kSegBytes / 16) + (u32)j * kWave + lane;
                            }
                            f_items += (u32)__popcll(bm);
                        }
                    }
                    if constexpr (LINL)
                    {
                        if (inter)
                        {
#pragma unroll
                            for (int w = 0; w < 4; ++w)
                                m16 |= movemask4(HA[w]) << (4 * w);
                        }
                        u32 nlm = NL;
                        if (!inter)
                            nlm &= clip(a.own_lo, a.own_hi);
                        line_cell(m16, nlm);
                    }
                    if (kp)
                    { // records: the lane-cell's two length words wait in LDS for the unit's record pass
                        const u32 idx = (u32)r * (kSegBytes / 16) + (u32)j * kWave + lane;
                        const u32 cwx = F[0] | (F[1] << 4), cwy = F[2] | (F[3] << 4);
                        mycnt += (u32)(__popc(cwx) + __popc(cwy));
                        cw[idx] = make_uint2(cwx, cwy);
                    }
                };
                if (fast_now)
                {
                    // Rolling prefetch as in ac_scan_kernel: cell j of the NEXT round replaces cell j as soon as it has been copied
                    // out, so a wave always has 8 KiB in flight.  The per-pattern code of a cell sits behind uniform branches,
                    // but no path through it issues a load: the s_waitcnt counts stay static (the ragged round is a separate loop).
                    typedef u32 u32x4 __attribute__((ext_vector_type(4)));
                    auto ntload = [](const uint4 *p) -> uint4 { // nothing re-reads the text here: stream it past the caches
                        const u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(p));
                        return make_uint4(v.x, v.y, v.z, v.w);
                    };
                    u32 before = 0, before2 = 0; // the 4 bytes in front of the round, and the 4 in front of those (uniform)
                    if (have)
                    {
                        before = carry;
                        before2 = carry2;
                    }
                    else
                    {
                        if (seg >= 4)
                            before = __builtin_amdgcn_readfirstlane(*reinterpret_cast<const u32 *>(a.text + seg - 4));
                        if ((LONG || FIVE) && llong && seg >= 8)
                            before2 = __builtin_amdgcn_readfirstlane(*reinterpret_cast<const u32 *>(a.text + seg - 8));
                    }
                    // Six instantiations — the item flavour of the one-pass writer, in-kernel -c beside -i or a long length, the -i count with a
                    // long length — needed 2-12 registers more than the 168 of three waves per SIMD and spilled 12-52 B/lane (VERDICT r05
                    // weak #7).  They roll kRoll of the round's eight cells: the rest is requested here, at the round's start, and consumed
                    // last — its registers are free while the cells in front of it are compared.
#pragma unroll
                    for (int j = 0; j < kCells; ++j)
                        if (!have || j >= kRoll)
                            d[j] = ntload(src + j * kWave);
                    const bool pf_next = !emit_final && seg + 2 * (u64)kSegBytes <= a.text_len && (r + 1 < kAcRounds || unit + 1 < u_end);
                    const uint4 *nsrc = pf_next ? src + kSegBytes / 16 : reinterpret_cast<const uint4 *>(a.text + seg); // (none: one cached line)
                    auto cells = [&](auto interC) __attribute__((always_inline)) {
                        auto one_cell = [&](const int j) __attribute__((always_inline)) {
                            const u32 D[4] = {d[j].x, d[j].y, d[j].z, d[j].w};
                            if (j < kRoll)
                                d[j] = ntload(nsrc + j * kWave);
                            const u32 P = (u32)__builtin_amdgcn_update_dpp((int)before, (int)D[3], 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
                            before = __builtin_amdgcn_readlane(D[3], 63);
                            u32 P2 = 0;
                            if ((LONG || FIVE) && llong) // (uniform: only a long pattern looks eight bytes back)
                            {
                                P2 = (u32)__builtin_amdgcn_update_dpp((int)before2, (int)D[2], 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
                                before2 = __builtin_amdgcn_readlane(D[2], 63);
                            }
                            cell(interC, j, D, P, P2);
                        };
                        if constexpr (FIVE || DENSE)
                        {
                            // unrolled by construction (the DENSE -i instantiation with a long length has the same problem): with a fifth class the body outgrows the unroller's budget, `#pragma unroll`
                            // is dropped, d[j] is indexed at run time and the round's 128 bytes live in scratch (144 B/lane, 2.3 TB/s)
                            tiny_static_for(std::make_integer_sequence<int, kCells>{}, [&](auto jc) __attribute__((always_inline)) { one_cell(decltype(jc)::value); });
                        }
                        else
                        {
#pragma unroll
                            for (int j = 0; j < kCells; ++j)
                                one_cell(j);
                        }
                    };
                    if (interior) // two copies of the round: the window clipping of a boundary round costs the interior ones nothing
                        cells(std::true_type{});
                    else
                        cells(std::false_type{});
                    have = pf_next;
                    carry = before;
                    carry2 = before2;
                }
                else
                {
                    have = false;
#pragma unroll 1
                    for (int j = 0; j < kCells; ++j)
                    { // the ragged end of the text: bytewise, bounds-checked (bytes outside read as 0 and are clipped in the cell)
                        const u64 lbase = seg + (u64)j * kCellBytes + (u64)lane * 16u;
                        u32 W[6]; // the 8 bytes in front of the lane's 16, and those
#pragma unroll
                        for (int w = 0; w < 6; ++w)
                        {
                            u32 v = 0;
                            for (int b = 0; b < 4; ++b)
                            {
                                const u64 o = lbase + (u64)(w * 4 + b);
                                if (o >= 8 && o - 8 < a.text_len)
                                    v |= (u32)a.text[o - 8] << (8 * b);
                            }
                            W[w] = v;
                        }
                        const u32 D[4] = {W[2], W[3], W[4], W[5]};
                        cell(std::false_type{}, j, D, W[1], W[0]); // (a ragged round is a boundary round)
                    }
                }
            } // rounds

            if constexpr (FUSED && DENSE)
            { // the unit's matches (selects, not an indexed array: that would live in scratch)
                const u32 cu = f_items - u_before, uu = (u32)(unit - u_begin);
                u_before = f_items;
                u_c0 = uu == 0u ? cu : u_c0;
                u_c1 = uu == 1u ? cu : u_c1;
                u_c2 = uu == 2u ? cu : u_c2;
            }
            u32 wcnt = 0; // matches of the unit (uniform)
            if (KEEP && !LINES && want_pos) // (-c never asks for records: ac_scan)
            {
                // ---- records: lane L owns the lane-cells [16 L, 16 L + 16) = the unit's positions [256 L, 256 L + 256); their
                //      length words come into registers, a wave prefix of the per-lane counts ranks them
                uint4 q[EMIT ? 8 : 1];
                u32 oc = 0, nz = 0; // nz: bit i = the lane's i-th lane-cell holds a match
                {
                    const uint4 *mine = reinterpret_cast<const uint4 *>(cw + 16u * lane);
#pragma unroll(EMIT ? 8 : 2) // (streaming launch: two reads in flight, not eight — 24 registers less beside the text prefetch)
                    for (int k = 0; k < 8; ++k)
                    {
                        const uint4 v = mine[k];
                        if (EMIT)
                            q[k] = v;
                        oc += (u32)(__popc(v.x) + __popc(v.y) + __popc(v.z) + __popc(v.w));
                        nz |= ((v.x | v.y) ? 1u << (2 * k) : 0u) | ((v.z | v.w) ? 2u << (2 * k) : 0u);
                    }
                }
                u32 incl = oc;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1)
                {
                    const u32 t = __shfl_up(incl, o);
                    if (lane >= (u32)o)
                        incl += t;
                }
                wcnt = __shfl(incl, 63);
                const u32 at0 = incl - oc; // rank of this lane's first match in the unit
                // the matches of one lane-cell in the reference's order — END ascending, longest first (aho_corasick.c:383-437):
                // put(rank, start relative to the unit (>= -3), length)
                auto cellwalk = [&](const u32 i, const u32 cx, const u32 cy, u32 &at, auto put) __attribute__((always_inline)) {
                    // ENDs of the lane-cell in position order: bit 8 b + w of the any-length word is position 4 w + b
                    const u32 hs = (cx | (cx >> 4) | cy | (cy >> 4)) & 0x0f0f0f0fu;
                    u32 h = 0;
#pragma unroll
                    for (int b = 0; b < 4; ++b)
                    { // bit w of the byte's nibble -> bit 4 w + b (shifts and ORs: a multiply would carry where two bits meet)
                        const u32 x = (hs >> (8 * b)) & 0xfu;
                        h |= ((x | (x << 3) | (x << 6) | (x << 9)) & 0x1111u) << b;
                    }
                    const int r0 = (int)((16u * lane + i) * 16u) + 1; // (one past the END of position 0 of the cell)
                    while (h)
                    {
                        const u32 e = (u32)__builtin_ctz(h);
                        h &= h - 1u;
                        const u32 bit = 8u * (e & 3u) + (e >> 2);
                        const int end1 = r0 + (int)e;
                        if ((cy >> (bit + 4u)) & 1u) put(at++, end1 - (int)len4, len4);
                        if ((cy >> bit) & 1u) put(at++, end1 - 3, 3u);
                        if ((cx >> (bit + 4u)) & 1u) put(at++, end1 - 2, 2u);
                        if ((cx >> bit) & 1u) put(at++, end1 - 1, 1u);
                    }
                };
                if constexpr (!EMIT)
                {
                    // staging (a sparse dictionary: a few matches per unit): only the lane-cells that hold one, re-read from LDS
                    // (through 64 words of LDS and out with ONE store of consecutive lanes: twenty scattered 4-byte stores per unit
                    //  were a third of this kernel's time; slots beyond 64 entries — a test hook — take them directly)
                    const bool via_lds = parked;
                    u32 *sitems = park_slots + (u32)(unit - u_begin) * 64u;
                    if (oc && at0 < a.stage_cap)
                    {
                        u32 at = at0;
                        while (nz)
                        {
                            const u32 i = (u32)__builtin_ctz(nz);
                            nz &= nz - 1u;
                            const uint2 c2 = cw[16u * lane + i];
                            cellwalk(i, c2.x, c2.y, at, [&](const u32 rk, const int srel, const u32 len) {
                                if (rk < a.stage_cap)
                                {
                                    const u32 word = ((u32)(srel + 1024) << 11) | len; // as ac_scan_kernel stages them
                                    if (via_lds)
                                        sitems[rk] = word;
                                    else
                                        slot[rk] = word;
                                }
                            });
                        }
                    }
                    // (parked: the slot leaves with the ticket, below)
                }
                if constexpr (EMIT)
                {
                    // final records (an overflowed unit, or every unit of a dense dictionary): 2048 at a time through LDS — the
                    // length words are in registers now, their 8 KiB take the compact items — and out with consecutive lanes on
                    // consecutive records (a lane storing its own run of records touches 64 different lines per instruction)
                    u32 *items = reinterpret_cast<u32 *>(cw);
                    for (u32 cb = 0; cb < wcnt; cb += 2048u)
                    {
                        if (oc && at0 < cb + 2048u && at0 + oc > cb)
                        {
                            u32 at = at0;
#pragma unroll
                            for (int i = 0; i < 16; ++i)
                            {
                                const u32 cx = (i & 1) ? q[i >> 1].z : q[i >> 1].x, cy = (i & 1) ? q[i >> 1].w : q[i >> 1].y;
                                if (cx | cy)
                                    cellwalk((u32)i, cx, cy, at, [&](const u32 rk, const int srel, const u32 len) {
                                        if (rk - cb < 2048u)
                                            items[rk - cb] = ((u32)(srel + 8) << 3) | (len - 1u);
                                    });
                            }
                        }
                        const u32 nitem = wcnt - cb < 2048u ? wcnt - cb : 2048u;
                        for (u32 k = lane; k < nitem; k += 64u)
                        {
                            const u32 it = items[k];
                            const u64 g = fbase + cb + k;
                            if (g < a.pos_cap)
                            {
                                const u64 st = useg + (u64)(it >> 3) - 8u + a.global_base, en = st + (it & 7u) + 1u;
                                *reinterpret_cast<uint4 *>(a.positions + 2 * g) = make_uint4((u32)st, (u32)(st >> 32), (u32)en, (u32)(en >> 32));
                            }
                        }
                    }
                }
            }
            else
            {
                if (chain) // -c: the unit's match count goes into its info word
                {
                    u32 c = mycnt;
#pragma unroll
                    for (int o = 32; o >= 1; o >>= 1)
                        c += __shfl_xor(c, o);
                    wcnt = c;
                }
                else
                    acc_total += mycnt;
            }

            LineState wls{0, false, false, false};
            if constexpr (LINL)
            {
#pragma unroll
                for (int o = 32; o >= 1; o >>= 1)
                    l_cnt += __shfl_xor(l_cnt, o);
                wls = LineState{l_cnt + s_new, s_seen, s_seen ? s_head : s_open, s_open};
            }

            if (chain)
                acc_total += wcnt;
            if (chain && !emit_final && lane == 0)
            {
                u64 info = (u64)wcnt;
                if (LINES) // (written out: through line_bits() the four LINES instantiations compile differently)
                    info |= (wls.nl ? kLnNl : 0) | (wls.head ? kLnHead : 0) | (wls.tail ? kLnTail : 0) |
                            ((u64)(wls.cnt & kUiLineMask) << kUiLineShift);
                else if (wcnt)
                    info |= kLnHead | kLnTail;
                if (parked)
                    park_info[(u32)(unit - u_begin)] = info;
                else
                    a.unitinfo[unit] = info;
                if (want_pos && wcnt > a.stage_cap)
                { // (kept per wave: with a dense dictionary EVERY unit overflows, and two atomics per unit on one address serialise)
                    ++ovf_units;
                    ovf_max = wcnt > ovf_max ? wcnt : ovf_max;
                }
            }
        }
        if constexpr (FUSED && DENSE)
        {
            if (f_items > f_room)
                overflowed = true; // too dense for the ring: counted, not recorded — the host picks smaller tickets or the staging road
            if (lane == 0)
                __hip_atomic_store(&a.tk_agg[tk], (u64)f_items | kTkReady, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (pend)
                flush_dense(len4);
            if (f_items && f_items <= f_room)
            {
                pend = true;
                pend_t = tk;
                pend_at = f_at;
                pend_items = f_items;
                pend_c0 = u_c0;
                pend_c1 = u_c1;
                pend_c2 = u_c2;
                wp = dwrap(f_at + f_items);
            }
            else
                pend_items = 0;
        }
        else if constexpr (FUSED)
        {
            u32 tcnt = lane_cnt; // the ticket's matches
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1)
                tcnt += __shfl_xor(tcnt, o);
            if (f_items > f_room)
                overflowed = true; // too dense for the ring: counted, not recorded — the host takes the staging road
            // publish the count BEFORE waiting for anything; the ticket drawn next is behind every ticket this wave has parked
            if (lane == 0)
                __hip_atomic_store(&a.tk_agg[tk], (u64)tcnt | kTkReady, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (pend)
                flush(len4);
            if (f_items && f_items <= f_room)
            {
                pend = true;
                pend_t = tk;
                pend_at = f_at;
                pend_items = f_items;
                wp = (f_at + f_items) & (kTinyRing - 1u);
            }
            else
                pend_items = 0;
        }
        if (KEEP && !LINES && want_pos && !emit_final && a.stage_cap <= 64u && a.upt <= kAcUnitsPerTicketMax)
        { // the ticket's parked info words and staging slots, in a few stores of consecutive lanes
            const u32 nun = (u32)(u_end - u_begin);
            if (lane < nun)
                a.unitinfo[u_begin + lane] = park_info[lane];
            u32 *dst = reinterpret_cast<u32 *>(a.stage) + u_begin * (u64)a.stage_cap;
            for (u32 k = lane; k < nun * a.stage_cap; k += 64u)
                dst[k] = park_slots[(k / a.stage_cap) * 64u + k % a.stage_cap];
        }
    }
    if constexpr (FUSED)
    {
        if (pend)
        {
            if constexpr (DENSE)
                flush_dense(len4);
            else
                flush(len4);
        }
        if (overflowed && lane == 0)
            atomicAdd(&a.ctr->overflow_units, 1ull);
        return; // (the resolver's running sum is the total)
    }
    if (!chain)
    { // count only: the lanes' own totals, reduced once
        u64 c = acc_total;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1)
            c += (u64)__shfl_xor((unsigned long long)c, o);
        acc_total = c;
    }
    if (lane == 0 && acc_total && !a.emit_mode)
        atomicAdd(&a.ctr->total, acc_total);
    if (lane == 0 && ovf_units)
    {
        atomicAdd(&a.ctr->overflow_units, (unsigned long long)ovf_units);
        atomicMax(&a.ctr->max_unit_count, (unsigned long long)ovf_max);
    }
}

u32 ac_tiny_lds_bytes(bool lines, bool records)
{
    if (lines || !records)
        return 0; // a count, or -c (lines counted in the cell): nothing is kept
    return kTinyWaves * (kTinyEntries * 2 + kAcUnitsPerTicketMax * 66) * (u32)sizeof(u32);
}
// resident workgroups per CU: 12 waves by registers for the counting and the emit-mode instantiations, 8 for the ones that keep
// a unit's masks AND stream (their record / line pass runs with the next round's prefetch in registers: under the 168-register
// cap of 3 waves per SIMD it spilled, and a scratch access drains the in-order vmcnt queue of the prefetch — 2 waves per SIMD,
// no scratch)
u32 ac_tiny_blocks_per_cu(const AcArgs &a)
{
    const bool keep = ac_tiny_keeps(a), lines = (a.flags & F_LINES) != 0;
    const u32 lds = keep ? ac_tiny_lds_bytes(lines, !lines) : 0u, by_regs = (keep && !a.emit_mode) ? (u32)KG_TINY_KEEP_WAVES : 3u;
    return lds ? std::min<u32>(by_regs, 160u * 1024u / lds) : by_regs;
}

template <bool CI, bool LN, bool KEEP, bool EMIT, bool LONG>
static hipError_t tiny_launch4(const AcArgs &a, const AcTiny &td, u32 grid, hipStream_t st)
{
    if (const hipError_t e = grant_dynamic_lds<&ac_tiny_kernel<CI, LN, KEEP, EMIT, LONG>>(160 * 1024); e != hipSuccess) // (the most: see ac_launch3)
        return e;
    hipLaunchKernelGGL((ac_tiny_kernel<CI, LN, KEEP, EMIT, LONG>), dim3(grid), dim3(kTinyBlock), KEEP ? ac_tiny_lds_bytes(LN, !LN) : 0u, st, a, td);
    return hipGetLastError();
}

template <bool CI, bool LN, bool KEEP, bool EMIT>
static hipError_t tiny_launch3(const AcArgs &a, const AcTiny &td, u32 grid, hipStream_t st)
{
    return td.llong ? tiny_launch4<CI, LN, KEEP, EMIT, true>(a, td, grid, st) : tiny_launch4<CI, LN, KEEP, EMIT, false>(a, td, grid, st);
}

// records == false: a count — or the COUNT PASS of a dense dictionary (F_POS with stage_cap 0: every unit "overflows" an empty
// staging slot and gets its records from the emit-mode launch; see ac_scan)
bool ac_tiny_keeps(const AcArgs &a)
{
    return !(a.flags & F_LINES) && (a.flags & F_POS) && (a.emit_mode || a.stage_cap); // (-c counts its lines in the cell: nothing kept)
}

// the one-pass record writer: 48 KiB of rings per workgroup, 3 workgroups per CU (registers and LDS alike); one block more than the
// tickets need is never useful, and at least one scanning wave stands next to the resolver
template <bool CI>
static hipError_t tiny_launch_fused2(const AcArgs &a, const AcTiny &td, u32 grid, hipStream_t st)
{
    constexpr u32 lds = kTinyWaves * kTinyRing * 3u * (u32)sizeof(u32);
    // (a fifth class — 4-byte patterns beside a long length — needs 211-217 VGPRs here: at 2 waves per SIMD it measured SLOWER than the
    //  general kernel, `if else while` 2.8 against 3.3 TB/s with offsets; ac_scan does not send such dictionaries this way)
    if (td.five || td.llong) // (a long length in the place of class 4: that instantiation spills — such dictionaries keep the staging road, ac_scan)
        return hipErrorInvalidValue;
    else
        hipLaunchKernelGGL((ac_tiny_kernel<CI, false, false, false, false, true>), dim3(grid), dim3(kTinyBlock), lds, st, a, td);
    return hipGetLastError();
}
// the DENSE flavour: any tiny dictionary without a fifth class, a long length included (tickets of at most 4 units: ac_scan)
template <bool CI, bool LONG>
static hipError_t tiny_launch_dense2(const AcArgs &a, const AcTiny &td, u32 grid, hipStream_t st)
{
    constexpr u32 lds = kTinyWaves * kTinyRing * 3u * (u32)sizeof(u32);
    hipLaunchKernelGGL((ac_tiny_kernel<CI, false, false, false, LONG, true, false, true>), dim3(grid), dim3(kTinyBlock), lds, st, a, td);
    return hipGetLastError();
}
u32 ac_tiny_dense_ring() { return kTinyRing * 6u; } // 16-bit entries per wave
hipError_t ac_tiny_launch_fused(const AcArgs &a, const AcTiny &td, u64 n_tickets, u32 num_cu, hipStream_t st, bool dense)
{
    if (dense)
    {
        if (td.five || a.upt < 1u || a.upt > 4u)
            return hipErrorInvalidValue;
        u32 grid = (u32)std::max<u64>(1, std::min<u64>((n_tickets + kTinyWaves - 1) / kTinyWaves + 1, (u64)num_cu * (u32)KG_TINY_FUSED_WAVES));
        if (g_s1_force_grid > 0)
            grid = std::min<u32>(grid, (u32)g_s1_force_grid);
        g_tiny_launches.fetch_add(1, std::memory_order_relaxed);
        g_tiny_dense_launches.fetch_add(1, std::memory_order_relaxed);
        const bool ci = (a.flags & F_CI) != 0;
        if (td.llong)
            return ci ? tiny_launch_dense2<true, true>(a, td, grid, st) : tiny_launch_dense2<false, true>(a, td, grid, st);
        return ci ? tiny_launch_dense2<true, false>(a, td, grid, st) : tiny_launch_dense2<false, false>(a, td, grid, st);
    }
    u32 grid = (u32)std::max<u64>(1, std::min<u64>((n_tickets + kTinyWaves - 1) / kTinyWaves + 1, (u64)num_cu * (u32)KG_TINY_FUSED_WAVES));
    if (g_s1_force_grid > 0) // test hook: a starved grid (krep_gpu_debug_force_single_grid) — the progress argument of kg_tickets.h
        grid = std::min<u32>(grid, (u32)g_s1_force_grid);
    g_tiny_launches.fetch_add(1, std::memory_order_relaxed);
    return (a.flags & F_CI) ? tiny_launch_fused2<true>(a, td, grid, st) : tiny_launch_fused2<false>(a, td, grid, st);
}

hipError_t ac_tiny_launch(const AcArgs &a, const AcTiny &td, u64 n_tickets, u32 num_cu, hipStream_t st)
{
    const u32 grid = (u32)std::min<u64>((n_tickets + kTinyWaves - 1) / kTinyWaves, (u64)num_cu * ac_tiny_blocks_per_cu(a));
    const bool ci = a.flags & F_CI, ln = a.flags & F_LINES, keep = ac_tiny_keeps(a);
    g_tiny_launches.fetch_add(1, std::memory_order_relaxed);
    const bool emit = a.emit_mode != 0;
    if (td.five) // a fifth class: only the counting instantiation knows it (ac_scan sends every other mode of such a dictionary elsewhere)
    {
        if (ln || emit || keep || ci) // (-i: 173 VGPRs = 2 waves per SIMD, 3.0 TB/s against the general kernel's 3.4 — not sent here)
            return hipErrorInvalidValue;
        hipLaunchKernelGGL((ac_tiny_kernel<false, false, false, false, false, false, true>), dim3(grid), dim3(kTinyBlock), 0, st, a, td);
        return hipGetLastError();
    }
    if (ln) return ci ? tiny_launch3<true, true, false, false>(a, td, grid, st) : tiny_launch3<false, true, false, false>(a, td, grid, st);
    if (emit) return ci ? tiny_launch3<true, false, true, true>(a, td, grid, st) : tiny_launch3<false, false, true, true>(a, td, grid, st);
    if (keep) return ci ? tiny_launch3<true, false, true, false>(a, td, grid, st) : tiny_launch3<false, false, true, false>(a, td, grid, st);
    return ci ? tiny_launch3<true, false, false, false>(a, td, grid, st) : tiny_launch3<false, false, false, false>(a, td, grid, st);
}

} // namespace kg
