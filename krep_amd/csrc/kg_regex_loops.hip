// kg_regex_loops.hip — krep -E with *, + and {n,} behind an atom (include/krep_gpu.h, krep_gpu_regex_compile_loops): ERROR.*timeout,
// [0-9]+\.[0-9]+, colou*r, ^#+ .  The line walk kernel kg::rx_line_walk and the scan kg::scan_regex_loops, a sequence of the steps
// in front of it (rl_window, rl_args, rl_cut_line_look, rl_sparse_road, rl_dense_road, rl_walk_passes, rl_newline_summary).  The
// program is a RegexWalk (kg_regex_compile.h: table, init, fin, self — PLUS and SELF below —, chain and jump pairs, bol, eol, filter);
// kg_regex.hip puts it on the device and hands over when the plan's program is of this kind.
//
// Two properties carry the scan.  No class of such a program holds '\n', so under the reference's REG_NEWLINE a match lies inside one
// line: the lines are independent, and the leftmost-longest walk of one line is a small sequential job.  And every match holds a
// fixed-length factor of its branch as consecutive bytes (the program's FILTER), which the fixed-length kernels find at their rate.
// Stage 1, the candidate lines, by one of two roads:
//   sparse: the filter alternation is scanned over the text with records by scan_regex_alt / rx_drive (an inner plan); the line
//     analysis of krep_gpu_matching_lines() turns the records into the distinct line spans that hold one.  The filter's classes hold no
//     '\n' either, so every line with an occurrence holds the start of a record, whatever the greedy selection kept.
//   dense: a filter like [a-z] would write 16 bytes of record per text byte.  When the filter's counting launch reports more than one
//     occurrence per 64 text bytes its emitting launch is skipped (krep_gpu_plan::rx_emit_limit) and EVERY line is a candidate: the
//     record list of an inner single-byte plan for '\n' (kg_single.hip) says where they are.
// Stage 2, kg::rx_line_walk<LINES, EMIT, WIN>: one lane per candidate line, grid-stride.  Branch i lives in bits [o_i, o_i + L_i) of a 32-bit
// state, T[byte] has bit o_i + j set when byte is in place j of branch i (in LDS once per bank, rx_fill_table), INIT holds every o_i,
// FIN every o_i + L_i - 1, PLUS the places that repeat.  An attempt from s starts with S = INIT & T[text[s]] and steps
// S = (((S << 1) & ~INIT) | (S & PLUS)) & T[b]: a place hands over to the next one, a repeating place also stays.  The last position
// behind which S & FIN was non-zero is the longest match at s (with $ only the line's end counts; the end of the text ends a line in a
// case-sensitive search only).  The attempt ends when S is 0 or at the line's end; a start whose byte is in no first place costs one
// lookup.  The first start with a match is emitted and the walk resumes at its end (with ^ only the line's first byte is tried).
// Passes: a counting launch writes every candidate line's match count (under -c one per line that holds a match, summed in the
// kernel with the line bits), the offsets pass of kg_post.hip turns the counts into record indices, the emitting launch walks
// again and writes each record at its final index, the first max_count only.
// Bounded work: a lane's worst case is quadratic in its line's length (a.*b on a line of a's).  The counting launch does not walk a
// candidate line of more than 4096 bytes and raises Counters::overflow_units; the host reads that first and refuses the scan (2)
// with nothing written.  With krep_gpu_set_regex_long_lines on, the scan of the whole text lists those lines instead (rx_long_list) and
// walks them in linear time by a backward and a forward pass (rx_long_walk, "long lines" below); the refusal stays for any other
// window and for a line beyond min(1 MiB, budget / 4).
// Windows (krep_gpu_set_regex_loops_windows; off: any window but the whole text is refused).  The kernel owns STARTS, not lines: a
// line is looked at when it meets [own_lo, own_hi) (ls < own_hi && le > own_lo), its walk starts at the line's first byte — the
// matches in front of own_lo say where the first owned attempt stands —, a match is counted or emitted when own_lo <= s < own_hi, and
// the walk ends with the owned starts (under -c with the first OWNED match).  -c reports what every other scan reports for its owned
// window: kLnHead for a counted line with ls <= own_lo, kLnTail for one with le >= own_hi, kLnNl for a '\n' inside the owned range
// (the host looks for one itself when no line that meets the range says so).  A line that meets the owned range and touches an end
// of the buffer that is not an end of the text is CUT: the buffer does not show where it starts, or ends.  Longer than 4096 bytes
// as far as it shows, it raises overflow_units bit 0 like any long line; else bit 1, and the host refuses the scan (2) with a reason
// of its own.  Since no line of more than 4096 bytes is walked, 4096 bytes of context on each side of the owned range hold every line
// the window needs.  Stage 1 runs over the BUFFER, the inner plans see it as a whole text with base 0; the road is chosen per buffer.
// On the sparse road the line the buffer's end cuts is looked at by the host as well: its filter occurrence may lie behind that end.
// The whole-text scan is the case own_lo = 0, own_hi = text_len in a buffer that begins and ends the text; it runs the instantiations
// without WIN, in which these are constants and the ownership tests fold away (rl_launch picks them).
// The GENERAL step (rx_line_walk<..., GEN>; krep_gpu_regex_compile_groups took the search, or the test hook
// krep_gpu_debug_force_regex_general sends a loops program through it): the state is a set of POSITIONS of the expression's Glushkov
// automaton, one bit per atom occurrence, T[byte] has bit i set when byte is in position i's class, INIT is the first set, FIN the
// last set, and a step is S = follow(S) & T[b] with follow(S) = ((S & CHAIN) << 1) | (S & SELF) | the targets of every jump pair whose
// sources meet S (rl_follow; RlJumps rides in the kernel arguments: the 32 KiB of T leave no LDS at five workgroups per CU).
// Everything else — the roads, the line loop, ownership, the passes, the 4096-byte rule — is the one copy described above.
// Reads: no byte outside [0, text_len), one byte at a time at any alignment: the walk of a lane per line is not coalesced, which is
// the price of the dense road.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/krep_gpu.h"
#include "kg_common.h"
#include "kg_device.h"
#include "kg_internal.h"
#include "kg_plan.h"
#include "kg_regex_dev.h"

namespace kg {

constexpr u32 kRlMaxLine = 4096; // bytes of the longest candidate line a lane walks

// follow(S) of the general step beside SELF: the positions that hand over to their right neighbour, and n pairs (sources, targets) for
// every other edge; the unused pairs are 0
struct RlJumps
{
    u32 chain, n;
    u32 src[kRegexGroupsMaxJumps], dst[kRegexGroupsMaxJumps];
};
struct RlArgs
{
    const uint8_t *text;
    u64 text_len;
    // the candidate lines.  from_nl == 0: line l is [spans[2l], spans[2l + 1]).  from_nl == 1: spans holds the n_lines - 1 newline
    // records of the text in order, line l starts behind newline l - 1 (line 0 at 0) and ends on newline l (the last at text_len)
    const u64 *spans;
    u64 n_lines;
    u64 global_base;
    u64 own_lo, own_hi; // the starts this scan owns (offsets in the buffer, own_hi <= text_len): a match is counted or emitted when
                        // own_lo <= s < own_hi, a line is looked at when it meets that range
    u32 from_nl;
    u32 init, fin, plus;
    // bit 0 ^, bit 1 $, bit 2: the end of the text ends a line ($ in a case-sensitive search, in the buffer that ends the text),
    // bit 3: the buffer begins the text, bit 4: it ends the text
    u32 flags;
    const u32 *table;
    RxOut o;   // unitinfo: the count of every candidate line; offsets: the index of its first record (kg_regex_dev.h)
    // the general step (GEN, a position automaton: init = first, fin = last, plus = SELF): the rest of the follow relation.  Wave-uniform
    // kernel arguments, not a table in LDS: the 32 KiB of T leave no LDS for a sixth array at five workgroups per CU.  Behind
    // everything the old step reads, so that its instantiations load their arguments from the offsets they always had
    RlJumps j;
};

// the positions that can stand behind one of S: chain never holds bit 31, so the shift loses nothing.  The pairs in groups of four,
// each group behind a wave-uniform branch: an automaton of few jumps pays for four
__device__ __forceinline__ u32 rl_follow(u32 S, u32 self, const RlJumps &j)
{
    u32 N = ((S & j.chain) << 1) | (S & self);
#pragma unroll
    for (int k = 0; k < 4; ++k)
        N |= (S & j.src[k]) ? j.dst[k] : 0u;
    if (j.n > 4u)
    {
#pragma unroll
        for (int k = 4; k < 8; ++k)
            N |= (S & j.src[k]) ? j.dst[k] : 0u;
    }
    if (j.n > 8u)
    {
#pragma unroll
        for (int k = 8; k < (int)kRegexGroupsMaxJumps; ++k)
            N |= (S & j.src[k]) ? j.dst[k] : 0u;
    }
    return N;
}
// the longest match that starts at s in a line that ends at le: its end, 0 when there is none (a match is never empty).  GEN: the
// state is a set of positions of an automaton (init = first, fin = last, plus = SELF) and a step is rl_follow; else of places of
// flat sequences, and a step is the shift
template <bool GEN>
__device__ __forceinline__ u64 rl_attempt(const uint8_t *text, const u32 *T, u32 init, u32 fin, u32 plus, const RlJumps &j, u64 s, u64 le, bool eol)
{
    u32 S = T[(u32)text[s] << 5] & init;
    u64 best = 0;
    if (S)
    {
        u64 p = s + 1; // S: the state behind byte p - 1
        for (;;)
        {
            if ((S & fin) != 0u && (!eol || p == le))
                best = p;
            if (p >= le)
                break;
            S = (GEN ? rl_follow(S, plus, j) : (((S << 1) & ~init) | (S & plus))) & T[(u32)text[p] << 5];
            if (!S)
                break;
            ++p;
        }
    }
    return best;
}

// LINES: -c, a line is done with its first match and nothing is written per line; EMIT: the records at offsets[line]; WIN: the owned
// range and the two ends of the buffer are what RlArgs says — without it they are the constants of a scan of the whole text
// ([0, text_len) in a buffer that begins and ends the text) and the compiler folds the ownership tests away: measured, the same tests
// on run-time values moved rows of profiles/regex_loops_scan.txt by 3-7 % in both directions (profiles/regex_loops_windows.txt)
// GEN: the attempt steps a position automaton (rl_follow); the line loop is this one copy either way
template <bool LINES, bool EMIT, bool WIN, bool GEN>
__global__ __launch_bounds__(kBlock) void rx_line_walk(const RlArgs a)
{
    static_assert(!(LINES && EMIT), "-c writes no records");
    __shared__ u32 s_T[256 * 32];
    rx_fill_table(s_T, a.table);
    const u32 *T = s_T + (lane_id() & 31u);
    const u64 text_len = a.text_len; // (a value of its own: min() takes references, and the address of a kernel argument is a stack slot)
    const bool bol = (a.flags & 1u) != 0u, eol = (a.flags & 2u) != 0u, eot_ends = (a.flags & 4u) != 0u;
    const bool begins = !WIN || (a.flags & 8u) != 0u, ends = !WIN || (a.flags & 16u) != 0u;
    const u64 own_lo = WIN ? a.own_lo : 0, own_hi = WIN ? a.own_hi : text_len;
    const u64 n_threads = (u64)gridDim.x * kBlock;
    u64 mine = 0;                 // owned matches (LINES: lines that hold one) of this lane's lines
    unsigned long long bits = 0;  // LINES: kLnNl | kLnHead | kLnTail as far as this lane's lines say them
    bool too_long = false, cut_line = false;

    for (u64 line = (u64)blockIdx.x * kBlock + threadIdx.x; line < a.n_lines; line += n_threads)
    {
        u64 ls, le;
        if (a.from_nl)
        {
            ls = line ? a.spans[2 * (line - 1)] + 1u : 0u;
            le = line + 1 < a.n_lines ? a.spans[2 * line] : text_len;
        }
        else
        {
            ls = a.spans[2 * line];
            le = a.spans[2 * line + 1];
        }
        le = min(le, text_len); // (whatever a span says, no byte outside the text is read)
        ls = min(ls, le);
        u32 cnt = 0;
        // a line that does not meet the owned range holds no owned start: not walked, not measured, count 0 and no bit
        const bool relevant = ls < own_hi && le > own_lo;
        if (!relevant)
            ;
        else if (le - ls > kRlMaxLine)
            too_long = true;
        else if ((ls == 0 && !begins) || (le == text_len && !ends))
            cut_line = true; // the buffer does not show where the line really starts, or ends
        else if (!eol || le < text_len || eot_ends)
        {
            u64 idx = EMIT ? a.o.offsets[line] : 0;
            const u64 stop = min(le, own_hi); // the walk ends with the owned starts
            u64 s = ls;
            // The walk starts at the line's first byte, as the greedy rule wants it: the matches in front of own_lo say where the
            // first owned attempt stands, and are not counted.  (With ^ the line's first byte is its only start.)  Only a line that
            // straddles own_lo comes through here; the loop behind it is the walk of a whole line.
            if (bol && ls < own_lo)
                s = stop;
            while (s < own_lo)
            {
                const u64 best = rl_attempt<GEN>(a.text, T, a.init, a.fin, a.plus, a.j, s, le, eol);
                s = best ? best : s + 1;
            }
            while (s < stop)
            {
                const u64 best = rl_attempt<GEN>(a.text, T, a.init, a.fin, a.plus, a.j, s, le, eol);
                if (best)
                {
                    if (EMIT)
                    {
                        if (idx < a.o.pos_cap)
                            rx_store_record(a.o.positions, idx, s + a.global_base, best + a.global_base);
                        ++idx;
                    }
                    ++cnt;
                    if (LINES || bol)
                        break; // (-c: the line's first OWNED match settles it)
                    s = best;
                }
                else
                {
                    if (bol)
                        break;
                    ++s;
                }
            }
        }
        if (EMIT)
            continue;
        mine += cnt;
        if (LINES)
        {
            // the bits every other scan reports for its owned window (krep_gpu_combine_line_counts): a '\n' inside it — the one that
            // ends this line or the one in front of it —, a counted line that began at or before own_lo, one that ends behind own_hi
            if (relevant && ((le < text_len && le < own_hi) || (ls > 0 && ls - 1 >= own_lo)))
                bits |= kLnNl;
            if (cnt)
                bits |= (ls <= own_lo ? kLnHead : 0ull) | (le >= own_hi ? kLnTail : 0ull);
        }
        else
            a.o.unitinfo[line] = cnt;
    }
    if (EMIT)
        return;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1)
        mine += __shfl_xor(mine, o);
    if (lane_id() == 0 && mine)
    {
        atomicAdd(&a.o.ctr->total, (unsigned long long)mine);
        if (LINES)
            atomicAdd(&a.o.ctr->lines, (unsigned long long)mine);
    }
    if (LINES && bits)
        atomicOr(&a.o.ctr->summary, bits);
    if (too_long || cut_line)
        atomicOr(&a.o.ctr->overflow_units, (too_long ? 1ull : 0ull) | (cut_line ? 2ull : 0ull));
}

template <bool GEN> static hipError_t rl_launch(const RlArgs &a, int mode, int num_cu, hipStream_t st)
{
    // one lane per line; 32 KiB of LDS each: five workgroups fit a CU
    const u64 blocks = (a.n_lines + kBlock - 1) / kBlock;
    u32 grid = (u32)std::max<u64>(1, std::min<u64>(blocks, (u64)num_cu * 5u));
    if (const int force = g_rx_force_grid.load(); force > 0) // test hook: a starved grid (krep_gpu_debug_force_regex_grid)
        grid = std::min<u32>(grid, (u32)force);
    if (GEN)
        g_rl_general.fetch_add(1, std::memory_order_relaxed); // (krep_gpu_debug_regex_general_walks)
    // (the scan of a whole text: the instantiations without WIN)
    const bool win = !(a.own_lo == 0 && a.own_hi == a.text_len && (a.flags & 24u) == 24u);
    if (mode == kRxLines)
    {
        if (win) hipLaunchKernelGGL((rx_line_walk<true, false, true, GEN>), dim3(grid), dim3(kBlock), 0, st, a);
        else hipLaunchKernelGGL((rx_line_walk<true, false, false, GEN>), dim3(grid), dim3(kBlock), 0, st, a);
    }
    else if (mode == kRxEmit)
    {
        if (win) hipLaunchKernelGGL((rx_line_walk<false, true, true, GEN>), dim3(grid), dim3(kBlock), 0, st, a);
        else hipLaunchKernelGGL((rx_line_walk<false, true, false, GEN>), dim3(grid), dim3(kBlock), 0, st, a);
    }
    else
    {
        if (win) hipLaunchKernelGGL((rx_line_walk<false, false, true, GEN>), dim3(grid), dim3(kBlock), 0, st, a);
        else hipLaunchKernelGGL((rx_line_walk<false, false, false, GEN>), dim3(grid), dim3(kBlock), 0, st, a);
    }
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ long lines (krep_gpu_set_regex_long_lines)
// What rx_line_walk leaves out, a candidate line of more than kRlMaxLine bytes in a scan of the whole text, walked in linear time
// by two passes over the line [ls, le):
//   backward: C[p] = T[text[p]] & (F(p) | pred(C[p + 1])), C[le] = 0, F(p) = fin where a match may end behind byte p (without $
//     everywhere, with $ behind the line's last byte only), pred the reverse of the step.  By induction from the line's end C[p] holds
//     exactly the places that take byte p and from there still reach an allowed end: C is EXACT, not an over-estimate.
//   forward: an attempt at s starts with S = init & C[s] and steps S = follow(S) & C[p] (C[p] lies inside T[text[p]], so the text is
//     not read again).  Every place of S reaches an end, so S is 0 directly behind the longest match's end and not before: an
//     attempt costs its match's length plus one step, a start without a match one load.  n backward and at most about 2n forward
//     steps, whatever the expression.
// C is one u32 per line byte in global scratch (RxLoopsWork::d_C), a line's words at the offset the lister drew for it.  -c keeps
// only the running word: a line holds a match iff some C[s] meets init (with ^: C[ls]).
struct RlLong
{
    u64 *list;           // pairs (candidate line, its first C word counted over all listed lines), appended by rx_long_list
    u64 list_cap, n;     // entries the list holds | entries it has
    u32 *C;
    u64 budget, round;   // a launch walks the entries whose first word lies in [round * budget, (round + 1) * budget)
    u32 kept;            // EMIT: the counting launch's C words still stand (the one round of the scan), no backward pass
};
// line `line` of the candidate lines as rx_line_walk reads it
struct RlSpan { u64 ls, le; };
__device__ __forceinline__ RlSpan rl_line_span(const u64 *spans, u32 from_nl, u64 n_lines, u64 text_len, u64 line)
{
    u64 ls, le;
    if (from_nl)
    {
        ls = line ? spans[2 * (line - 1)] + 1u : 0u;
        le = line + 1 < n_lines ? spans[2 * line] : text_len;
    }
    else
    {
        ls = spans[2 * line];
        le = spans[2 * line + 1];
    }
    le = le < text_len ? le : text_len; // (whatever a span says, no byte outside the text is read)
    return RlSpan{ls < le ? ls : le, le};
}
// the lister: every candidate line rx_line_walk refused, and where its C words go (Counters::pad[1]: lines, pad[2]: the byte cursor,
// max_unit_count: the longest of them).  Launched behind the counting launch, in front of the copy of the counters.  (A template
// like the kernels around it, so that it stands behind rx_line_walk's instantiations in the code object.)
template <class = void> __global__ __launch_bounds__(kBlock) void rx_long_list(const RlArgs a, const RlLong g)
{
    const u64 n_threads = (u64)gridDim.x * kBlock;
    for (u64 line = (u64)blockIdx.x * kBlock + threadIdx.x; line < a.n_lines; line += n_threads)
    {
        const RlSpan sp = rl_line_span(a.spans, a.from_nl, a.n_lines, a.text_len, line);
        const u64 len = sp.le - sp.ls;
        if (len <= kRlMaxLine)
            continue;
        const u64 k = atomicAdd(&a.o.ctr->pad[1], 1ull), off = atomicAdd(&a.o.ctr->pad[2], (unsigned long long)len);
        atomicMax(&a.o.ctr->max_unit_count, (unsigned long long)len);
        if (k < g.list_cap)
        {
            g.list[2 * k] = line;
            g.list[2 * k + 1] = off;
        }
    }
}
// the places that can stand in front of one of S: the reverse of the shift, or of rl_follow (the pairs in its groups of four)
template <bool GEN> __device__ __forceinline__ u32 rl_pred(u32 S, u32 init, u32 self, const RlJumps &j)
{
    if (!GEN)
        return ((S & ~init) >> 1) | (S & self);
    u32 N = ((S >> 1) & j.chain) | (S & self);
#pragma unroll
    for (int k = 0; k < 4; ++k)
        N |= (S & j.dst[k]) ? j.src[k] : 0u;
    if (j.n > 4u)
    {
#pragma unroll
        for (int k = 4; k < 8; ++k)
            N |= (S & j.dst[k]) ? j.src[k] : 0u;
    }
    if (j.n > 8u)
    {
#pragma unroll
        for (int k = 8; k < (int)kRegexGroupsMaxJumps; ++k)
            N |= (S & j.dst[k]) ? j.src[k] : 0u;
    }
    return N;
}
// the backward pass over [ls, le): C[p - ls] written when C is not null; returns C[ls], and in *any whether some C[s] meets init
template <bool GEN>
__device__ __forceinline__ u32 rl_back(const RlArgs &a, const u32 *T, u32 *C, u64 ls, u64 le, bool eol, bool *any)
{
    u32 c = 0, seen = 0;
    for (u64 p = le; p-- > ls;)
    {
        const u32 F = (!eol || p + 1 == le) ? a.fin : 0u;
        c = T[(u32)a.text[p] << 5] & (F | rl_pred<GEN>(c, a.init, a.plus, a.j));
        seen |= c;
        if (C)
            C[p - ls] = c;
    }
    *any = (seen & a.init) != 0u;
    return c;
}
// One lane per listed line of this round, grid-stride over the list.  LINES, EMIT, GEN as in rx_line_walk; the window is the whole
// text.  Counting: the line's count replaces the 0 rx_line_walk left in unitinfo[line] and joins ctr->total.
template <bool LINES, bool EMIT, bool GEN>
__global__ __launch_bounds__(kBlock) void rx_long_walk(const RlArgs a, const RlLong g)
{
    static_assert(!(LINES && EMIT), "-c writes no records");
    __shared__ u32 s_T[256 * 32];
    rx_fill_table(s_T, a.table);
    const u32 *T = s_T + (lane_id() & 31u);
    const u64 text_len = a.text_len;
    const bool bol = (a.flags & 1u) != 0u, eol = (a.flags & 2u) != 0u, eot_ends = (a.flags & 4u) != 0u;
    const u64 n_threads = (u64)gridDim.x * kBlock;
    u64 mine = 0;
    unsigned long long bits = 0;

    for (u64 k = (u64)blockIdx.x * kBlock + threadIdx.x; k < g.n; k += n_threads)
    {
        const u64 line = g.list[2 * k], off = g.list[2 * k + 1];
        if (off / g.budget != g.round)
            continue;
        const RlSpan sp = rl_line_span(a.spans, a.from_nl, a.n_lines, a.text_len, line);
        const u64 ls = sp.ls, le = sp.le;
        u32 *C = LINES ? nullptr : g.C + (off - g.round * g.budget); // (-c: no scratch, one round)
        u32 cnt = 0;
        if (!eol || le < text_len || eot_ends)
        {
            bool any = false;
            if (LINES)
            {
                const u32 c0 = rl_back<GEN>(a, T, nullptr, ls, le, eol, &any);
                cnt = (bol ? (c0 & a.init) != 0u : any) ? 1u : 0u;
            }
            else
            {
                if (!EMIT || !g.kept)
                    (void)rl_back<GEN>(a, T, C, ls, le, eol, &any);
                u64 idx = EMIT ? a.o.offsets[line] : 0;
                u64 s = ls;
                while (s < le)
                {
                    u32 S = C[s - ls] & a.init;
                    u64 best = 0;
                    if (S)
                    {
                        u64 p = s + 1; // S: the state behind byte p - 1
                        for (;;)
                        {
                            if ((S & a.fin) != 0u && (!eol || p == le))
                                best = p;
                            if (p >= le)
                                break;
                            S = (GEN ? rl_follow(S, a.plus, a.j) : (((S << 1) & ~a.init) | (S & a.plus))) & C[p - ls];
                            if (!S)
                                break;
                            ++p;
                        }
                    }
                    if (best)
                    {
                        if (EMIT)
                        {
                            if (idx < a.o.pos_cap)
                                rx_store_record(a.o.positions, idx, s + a.global_base, best + a.global_base);
                            ++idx;
                        }
                        ++cnt;
                    }
                    if (bol)
                        break;
                    s = best ? best : s + 1;
                }
            }
        }
        if (EMIT)
            continue;
        mine += cnt;
        if (LINES)
        {
            if (le < text_len || ls > 0)
                bits |= kLnNl;
            if (cnt)
                bits |= (ls == 0 ? kLnHead : 0ull) | (le >= text_len ? kLnTail : 0ull);
        }
        else
            a.o.unitinfo[line] = cnt;
    }
    if (EMIT)
        return;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1)
        mine += __shfl_xor(mine, o);
    if (lane_id() == 0 && mine)
    {
        atomicAdd(&a.o.ctr->total, (unsigned long long)mine);
        if (LINES)
            atomicAdd(&a.o.ctr->lines, (unsigned long long)mine);
    }
    if (LINES && bits)
        atomicOr(&a.o.ctr->summary, bits);
}
static u32 rl_long_grid(u64 n, int num_cu, u32 wg_per_cu)
{
    u32 grid = (u32)std::max<u64>(1, std::min<u64>((n + kBlock - 1) / kBlock, (u64)num_cu * wg_per_cu));
    if (const int force = g_rx_force_grid.load(); force > 0)
        grid = std::min<u32>(grid, (u32)force);
    return grid;
}
static hipError_t rl_long_list_launch(const RlArgs &a, const RlLong &g, int num_cu, hipStream_t st); // (at the end of the file)
// one round of the listed lines; 32 KiB of LDS a workgroup, like rx_line_walk
template <bool GEN> static hipError_t rl_long_launch(const RlArgs &a, const RlLong &g, int mode, int num_cu, hipStream_t st)
{
    const dim3 grid(rl_long_grid(g.n, num_cu, 5)), block(kBlock);
    g_rl_long.fetch_add(1, std::memory_order_relaxed); // (krep_gpu_debug_regex_long_walks)
    if (mode == kRxLines) hipLaunchKernelGGL((rx_long_walk<true, false, GEN>), grid, block, 0, st, a, g);
    else if (mode == kRxEmit) hipLaunchKernelGGL((rx_long_walk<false, true, GEN>), grid, block, 0, st, a, g);
    else hipLaunchKernelGGL((rx_long_walk<false, false, GEN>), grid, block, 0, st, a, g);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ what a plan keeps between scans
struct RxLoopsWork
{
    krep_gpu_plan *filter = nullptr;   // a plan whose program is the filter alternation (records, no -c, no max_count)
    krep_gpu_plan *newlines = nullptr; // the single-byte plan for '\n' with records
    match_position_t *d_rec = nullptr; // the filter's records, or the newline records
    uint64_t rec_cap = 0;
    match_position_t *d_spans = nullptr; // sparse road: the candidate lines and (krep_gpu_matching_lines wants it) their first records
    uint64_t *d_first = nullptr;
    uint64_t span_cap = 0;
    uint64_t *d_long = nullptr; // long lines: the lister's pairs
    uint64_t long_cap = 0;      // in entries
    uint32_t *d_C = nullptr;    // ... and the C words of a round
    uint64_t c_cap = 0;         // in words
};
void rx_loops_work_free(RxLoopsWork *w)
{
    if (!w)
        return;
    if (w->filter) krep_gpu_plan_destroy(w->filter);
    if (w->newlines) krep_gpu_plan_destroy(w->newlines);
    if (w->d_rec) (void)hipFree(w->d_rec);
    if (w->d_spans) (void)hipFree(w->d_spans);
    if (w->d_first) (void)hipFree(w->d_first);
    if (w->d_long) (void)hipFree(w->d_long);
    if (w->d_C) (void)hipFree(w->d_C);
    delete w;
}
// the inner plans, on the outer plan's device and with its configuration
static int rl_work_create(krep_gpu_plan *pl)
{
    auto *wk = new RxLoopsWork();
    pl->rx->work = wk; // (freed with the program, whatever fails below)
    auto *f = new krep_gpu_plan();
    wk->filter = f;
    f->cfg = pl->cfg;
    f->device = pl->device;
    f->cs = pl->cs;
    f->track = true;
    f->sp = search_params_t{};
    f->sp.case_sensitive = pl->sp.case_sensitive;
    f->sp.use_regex = true;
    f->sp.track_positions = true;
    f->sp.max_count = SIZE_MAX;
    f->ref_algo = KREP_RA_REGEX;
    f->num_cu = pl->num_cu;
    HIPCHK(hipMalloc(&f->d_ctr, sizeof(Counters)));
    HIPCHK(hipHostMalloc(&f->h_ctr, sizeof(Counters)));
    HIPCHK(hipEventCreate(&f->ev0));
    HIPCHK(hipEventCreate(&f->ev1));
    f->rx = regex_prog_create_alt(pl->rx->walk.filter);
    if (!f->rx)
        return 2;
    search_params_t nl{};
    nl.pattern = "\n";
    nl.pattern_len = 1;
    nl.case_sensitive = true;
    nl.track_positions = true;
    nl.max_count = SIZE_MAX;
    nl.num_patterns = 1;
    wk->newlines = krep_gpu_plan_create_ex(&nl, &pl->cfg);
    return wk->newlines ? 0 : 2;
}
static int rl_reserve_records(RxLoopsWork &wk, u64 need)
{
    HIPCHK(grow_scratch(wk.rec_cap, need, need, {dev_buf(wk.d_rec, need * sizeof(match_position_t))}));
    return 0;
}

// the two refusals of a scan (Counters::overflow_units bit 0 and bit 1): nothing was written
static int rl_refuse_long(u32 max_line = kRlMaxLine)
{
    return fail("regex with *, + or {n,}: a line of more than %u bytes: kept on krep's regex_search (a lane walks one line, and its "
                "worst case is quadratic in the line's length)", max_line);
}
static int rl_refuse_cut()
{
    return fail("regex with *, + or {n,}: the window does not hold the whole of a line that meets its owned range (the buffer begins or "
                "ends inside it): stage %u bytes of the text on both sides of the owned range", kRlMaxLine);
}

// ------------------------------------------------------------------------------------------------ the scan of a window, in steps
// what the steps of one scan share
struct RlScan
{
    krep_gpu_plan *pl;
    const Window &w;
    hipStream_t st;
    u64 own_hi; // min(w.own_hi, text_len)
    bool ends;  // the buffer ends the text
    RlArgs a;   // the walk's arguments; stage 1 fills in the candidate lines (spans, n_lines, from_nl)
    bool has_newline = false, know_newline = false; // -c: what stage 1 learnt about a '\n' in the owned range
};
struct RlTotals { uint64_t total = 0, nlines = 0; unsigned long long summary = 0; };

// The window rule.  *go: there is something to walk — without it the zeroed *out is the answer (no match is empty).  2: a window
// that is not the whole text while krep_gpu_set_regex_loops_windows is off.
static int rl_window(const Window &w, u64 *own_hi, bool *go)
{
    *go = false;
    if (w.text_len == 0 || w.global_len == 0 || w.own_lo >= w.own_hi)
        return 0;
    const bool whole = w.global_base == 0 && w.own_lo == 0 && w.own_hi >= w.text_len && w.global_len == w.text_len;
    if (!whole && !g_regex_loops_windows.load(std::memory_order_relaxed))
        return fail("a regex with *, + or {n,} is walked line by line from each line's first byte: scan the whole text in one window "
                    "(krep_gpu_split_mode() == KREP_GPU_SPLIT_WHOLE)");
    *own_hi = std::min<u64>(w.own_hi, w.text_len);
    *go = w.own_lo < *own_hi;
    return 0;
}
// the walk's arguments from the window and the plan's program (of a program that steps by the shift, chain and the jump pairs are 0)
static RlArgs rl_args(const krep_gpu_plan *pl, const Window &w, u64 own_hi)
{
    const RegexWalk &p = pl->rx->walk;
    RlArgs a{};
    a.text = w.d_text; a.text_len = w.text_len;
    a.global_base = w.global_base;
    a.own_lo = w.own_lo; a.own_hi = own_hi;
    a.init = p.init; a.fin = p.fin; a.plus = p.self;
    const bool begins = w.global_base == 0, ends = w.global_base + w.text_len == w.global_len;
    a.flags = (p.bol ? 1u : 0u) | (p.eol ? 2u : 0u) | (pl->sp.case_sensitive && ends ? 4u : 0u) | (begins ? 8u : 0u) | (ends ? 16u : 0u);
    a.table = pl->rx->d_table;
    a.j.chain = p.chain; a.j.n = p.n_jumps;
    memcpy(a.j.src, p.jump_src, sizeof a.j.src);
    memcpy(a.j.dst, p.jump_dst, sizeof a.j.dst);
    a.o.ctr = pl->d_ctr;
    return a;
}
// The sparse road in a buffer that does not end the text: the road looks at the lines that hold a filter occurrence IN THE BUFFER.
// The line the buffer's end cuts may hold its occurrence behind that end and a match that starts in the owned range all the same, so
// that one line is looked at here: it meets the owned range when no newline stands between the last owned byte and the buffer's end.
// (A line the buffer's START cuts needs no such look: an owned match lies in the part the buffer holds, with its occurrence.)
static int rl_cut_line_look(const RlScan &s)
{
    uint64_t pos = s.w.text_len;
    if (tail_find_next_newline(s.w.d_text, s.own_hi - 1, s.w.text_len, &s.pl->d_ctr->pad[0], &s.pl->h_ctr->pad[0], s.st, &pos))
        return 2;
    if (pos >= s.w.text_len)
        return s.w.text_len - (s.own_hi - 1) > kRlMaxLine ? rl_refuse_long() : rl_refuse_cut();
    return 0;
}
// The sparse road: the filter's records (its emitting launch skipped, and the scan repeated with more room, when there are more than
// the buffer holds), then the lines that hold one.  *dense: more than one occurrence per 64 text bytes (a first value, the
// bench tool runs both roads; force == 1: never) — nothing is set, the dense road names the lines.
static int rl_sparse_road(RlScan &s, int force, bool *dense)
{
    RxLoopsWork &wk = *s.pl->rx->work;
    const Window &w = s.w;
    // Stage 1 looks at the BUFFER, not at the owned range: a match that starts in front of own_hi may hold its filter factor behind it,
    // and the inner plans refuse windows of their own (a filter alternation that can overlap itself).  To them the buffer is a whole
    // text with base 0, so their records are buffer-relative, as krep_gpu_matching_lines() wants them.
    const Window wb{w.d_text, w.text_len, 0, w.text_len, 0, w.text_len};
    const u64 limit = force == 1 ? UINT64_MAX : w.text_len / 64;
    for (;;)
    {
        if (rl_reserve_records(wk, std::max<u64>(wk.rec_cap, std::min<u64>(limit, w.text_len / 64) + 1)))
            return 2;
        krep_gpu_scan_out_t fo;
        memset(&fo, 0, sizeof fo);
        wk.filter->rx_emit_limit = std::min<u64>(limit, wk.rec_cap);
        if (const int rc = scan_regex_alt(wk.filter, wb, wk.d_rec, wk.rec_cap, s.st, 0, &fo))
            return rc;
        if (fo.total_matches <= wk.filter->rx_emit_limit)
        {
            s.a.n_lines = fo.stored;
            break;
        }
        if (fo.total_matches > limit)
        {
            *dense = true;
            return 0;
        }
        if (rl_reserve_records(wk, fo.total_matches)) // (the forced sparse road on a text denser than the buffer was sized for)
            return 2;
    }
    g_rl_sparse.fetch_add(1, std::memory_order_relaxed);
    if (!s.a.n_lines)
        return 0;
    const u64 n_rec = s.a.n_lines;
    HIPCHK(grow_scratch(wk.span_cap, n_rec, n_rec,
                        {dev_buf(wk.d_spans, n_rec * sizeof(match_position_t)), dev_buf(wk.d_first, (n_rec + 1) * sizeof(uint64_t))}));
    krep_gpu_lines_out_t lo;
    if (krep_gpu_matching_lines(w.d_text, w.text_len, wk.d_rec, n_rec, UINT64_MAX, wk.d_spans, wk.d_first, n_rec, &lo, s.st))
        return 2;
    s.a.n_lines = lo.lines;
    s.a.spans = (const u64 *)wk.d_spans;
    return 0;
}
// The dense road: every line of the buffer is a candidate, the newline records of the inner single-byte plan say where they are (the
// scan repeated with more room when there are more than the buffer holds)
static int rl_dense_road(RlScan &s)
{
    RxLoopsWork &wk = *s.pl->rx->work;
    const Window &w = s.w;
    g_rl_dense.fetch_add(1, std::memory_order_relaxed);
    krep_gpu_scan_out_t no;
    for (;;)
    {
        if (krep_gpu_scan_device_ex(wk.newlines, w.d_text, w.text_len, 0, w.text_len, 0, w.text_len, wk.d_rec, wk.rec_cap, s.st, 0, &no))
            return 2;
        if (no.total_matches <= wk.rec_cap)
            break;
        if (rl_reserve_records(wk, no.total_matches))
            return 2;
    }
    s.a.from_nl = 1;
    s.a.spans = (const u64 *)wk.d_rec;
    s.a.n_lines = no.total_matches + 1;
    if (w.own_lo == 0 && s.own_hi == w.text_len)
    { // (the owned range is the buffer: its newline count says it)
        s.has_newline = no.total_matches != 0;
        s.know_newline = true;
    }
    return 0;
}
// ---- long lines (krep_gpu_set_regex_long_lines): the steps rl_walk_passes adds with the switch on
constexpr u64 kRlLongBudget = 256ull << 20; // bytes of C words a round may hold (krep_gpu_debug_set_regex_long_budget: another value)
constexpr u64 kRlLongMaxLine = 1ull << 20;  // bytes of the longest line admitted: 4 MiB of C words in one lane's hands
// Only the scan of the whole text takes long lines (the instantiations without WIN of rl_launch): the 4096 bytes of context a
// window stages rest on the 4096-byte line rule
static bool rl_long_on(const RlScan &s)
{
    return g_regex_long_lines.load(std::memory_order_relaxed) && s.a.own_lo == 0 && s.a.own_hi == s.a.text_len && (s.a.flags & 24u) == 24u;
}
static int rl_read_counters(RlScan &s)
{
    HIPCHK(hipMemcpyAsync(s.pl->h_ctr, s.pl->d_ctr, sizeof(Counters), hipMemcpyDeviceToHost, s.st));
    HIPCHK(hipStreamSynchronize(s.st));
    return 0;
}
// room for the lister's pairs: a text holds at most text_len / (kRlMaxLine + 1) + 1 long lines
static int rl_long_reserve_list(RlScan &s, RlLong *g)
{
    RxLoopsWork &wk = *s.pl->rx->work;
    const u64 need = std::min<u64>(s.a.n_lines, s.a.text_len / (kRlMaxLine + 1) + 1);
    HIPCHK(grow_scratch(wk.long_cap, need, need, {dev_buf(wk.d_long, need * 2 * sizeof(uint64_t))}));
    g->list = (u64 *)wk.d_long;
    g->list_cap = wk.long_cap;
    return 0;
}
// What the lister counted (in the counters just read).  The refusal that stays: a line of more than min(1 MiB, budget / 4) bytes —
// its C words alone would overrun a round.  Else the C scratch, never beyond the budget and the longest line, so that no line
// straddles its end: a line's round is its first word / budget.
static int rl_long_admit(RlScan &s, RlLong *g, u64 *rounds)
{
    RxLoopsWork &wk = *s.pl->rx->work;
    const Counters &h = *s.pl->h_ctr;
    const u64 set = g_rl_long_budget.load(std::memory_order_relaxed);
    g->budget = std::max<u64>(1, (set ? set : kRlLongBudget) / sizeof(u32));
    const u64 max_line = std::min<u64>(kRlLongMaxLine, g->budget);
    if (h.max_unit_count > max_line)
        return rl_refuse_long((u32)max_line);
    g->n = std::min<u64>(h.pad[1], g->list_cap);
    *rounds = (h.pad[2] - 1) / g->budget + 1;
    const u64 need = std::min<u64>(h.pad[2], g->budget + h.max_unit_count);
    HIPCHK(grow_scratch(wk.c_cap, need, need, {dev_buf(wk.d_C, need * sizeof(u32))}));
    g->C = wk.d_C;
    return 0;
}
// the listed lines round by round in one mode (-c keeps no C words: one launch takes them all)
using RlLongLaunch = hipError_t (*)(const RlArgs &, const RlLong &, int, int, hipStream_t);
static int rl_long_rounds(RlScan &s, RlLongLaunch launch, RlLong g, u64 rounds, int mode)
{
    if (mode == kRxLines)
    {
        g.budget = UINT64_MAX;
        rounds = 1;
    }
    g.kept = mode == kRxEmit && rounds == 1;
    for (g.round = 0; g.round < rounds; ++g.round)
        HIPCHK(launch(s.a, g, mode, s.pl->num_cu, s.st));
    return 0;
}
// Stage 2, the walk of the candidate lines: the counting launch (under -c the only one), the two refusals it can raise, and for a
// caller that takes records the offsets pass and the emitting launch.  With long lines taken (rl_long_on) the lister runs behind
// the counting launch, overflow_units bit 0 is a refusal only for a line beyond the cap, and the listed lines' rounds follow the
// counting and the emitting launch on the same stream.
static int rl_walk_passes(RlScan &s, bool lines, u64 want, match_position_t *d_pos, RlTotals *t)
{
    krep_gpu_plan *pl = s.pl;
    RlArgs &a = s.a;
    const auto launch = !pl->rx->walk.general ? rl_launch<false> : rl_launch<true>; // (the old step first: its kernels keep their place in the code object)
    const RlLongLaunch launch_long = !pl->rx->walk.general ? rl_long_launch<false> : rl_long_launch<true>; // (... and behind them these)
    const bool take_long = rl_long_on(s);
    RlLong g{};
    u64 rounds = 0;
    if (!lines)
    {
        if (post_reserve(pl->post, a.n_lines, 0))
            return 2;
        a.o.unitinfo = pl->post.d_unitinfo;
        a.o.offsets = (const u64 *)pl->post.d_offsets;
    }
    if (take_long && rl_long_reserve_list(s, &g))
        return 2;
    HIPCHK(hipMemsetAsync(pl->d_ctr, 0, sizeof(Counters), s.st));
    HIPCHK(launch(a, lines ? kRxLines : kRxCount, pl->num_cu, s.st));
    if (take_long)
        HIPCHK(rl_long_list_launch(a, g, pl->num_cu, s.st));
    if (rl_read_counters(s))
        return 2;
    if ((pl->h_ctr->overflow_units & 1ull) && !take_long)
        return rl_refuse_long();
    if (pl->h_ctr->overflow_units & ~1ull)
        return rl_refuse_cut();
    if (pl->h_ctr->overflow_units)
    {
        if (const int rc = rl_long_admit(s, &g, &rounds))
            return rc;
        if (rl_long_rounds(s, launch_long, g, rounds, lines ? kRxLines : kRxCount) || rl_read_counters(s))
            return 2;
    }
    t->total = pl->h_ctr->total;
    t->nlines = pl->h_ctr->lines;
    t->summary = pl->h_ctr->summary;
    if (want && t->total)
    {
        if (post_offsets_pass(pl->post, a.n_lines, false, pl->d_ctr, s.st))
            return 2;
        a.o.positions = (u64 *)d_pos;
        a.o.pos_cap = want;
        HIPCHK(launch(a, kRxEmit, pl->num_cu, s.st));
        if (rounds && rl_long_rounds(s, launch_long, g, rounds, kRxEmit))
            return 2;
        HIPCHK(hipStreamSynchronize(s.st));
    }
    return 0;
}
// -c: has_newline as a scan of the owned window reports it.  The candidate lines may not say (none that meets the range, or one that
// covers it): then the host looks for a '\n' in the range itself
static int rl_newline_summary(RlScan &s, unsigned long long *summary)
{
    if (!s.know_newline && !(*summary & kLnNl))
    {
        uint64_t pos = s.own_hi;
        if (tail_find_next_newline(s.w.d_text, s.w.own_lo, s.own_hi, &s.pl->d_ctr->pad[0], &s.pl->h_ctr->pad[0], s.st, &pos))
            return 2;
        s.has_newline = pos < s.own_hi;
    }
    *summary = (*summary & ~kLnNl) | ((s.has_newline || (*summary & kLnNl)) ? kLnNl : 0ull);
    return 0;
}

int scan_regex_loops(krep_gpu_plan *pl, const Window &w, match_position_t *d_pos, uint64_t cap, hipStream_t st, int time_it,
                     krep_gpu_scan_out_t *out)
{
    u64 own_hi = 0;
    bool go = false;
    if (const int rc = rl_window(w, &own_hi, &go); rc || !go)
        return rc;
    if (!pl->rx->work && rl_work_create(pl))
        return 2;
    const bool lines = pl->lines;
    const u64 want = (d_pos && cap && !lines && pl->track) ? std::min<u64>(pl->max_count, cap) : 0;
    HIPCHK(hipSetDevice(pl->device));
    if (time_it) HIPCHK(hipEventRecord(pl->ev0, st));
    RlScan s{pl, w, st, own_hi, w.global_base + w.text_len == w.global_len, rl_args(pl, w, own_hi)};

    // ---- stage 1: the candidate lines, by the sparse road unless the filter is dense (or a test forces a road)
    const int force = g_rl_force_road.load();
    bool dense = force == 2;
    if (!dense && !s.ends)
        if (const int rc = rl_cut_line_look(s))
            return rc;
    if (!dense)
        if (const int rc = rl_sparse_road(s, force, &dense))
            return rc;
    if (dense && rl_dense_road(s))
        return 2;

    // ---- stage 2: the walk of the candidate lines
    RlTotals t;
    if (s.a.n_lines)
        if (const int rc = rl_walk_passes(s, lines, want, d_pos, &t))
            return rc;
    if (!lines)
        t.summary = t.total ? (kLnHead | kLnTail) : 0;
    else if (rl_newline_summary(s, &t.summary))
        return 2;
    if (time_it && stop_clock(pl, true, st, out))
        return 2;
    rx_fill_out(pl, lines, t.total, t.nlines, t.summary, d_pos, cap, want, out);
    return 0;
}
// (here, so that the lister is the last kernel the file asks for: the older kernels keep their place in the code object)
static hipError_t rl_long_list_launch(const RlArgs &a, const RlLong &g, int num_cu, hipStream_t st)
{
    hipLaunchKernelGGL(rx_long_list<>, dim3(rl_long_grid(a.n_lines, num_cu, 8)), dim3(kBlock), 0, st, a, g);
    return hipGetLastError();
}
} // namespace kg
