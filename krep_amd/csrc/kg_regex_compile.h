// kg_regex_compile.h — the pattern compilers of the -E path (include/krep_gpu.h) and the order a search asks them in.  Host code
// without any HIP in it, so that a stand-alone program can run it under the sanitizers and pin its answers
// (tools/regex_compile_san.cpp).  It never sees a text: what it produces is a table, the search is the kernels' (kg_regex.hip,
// kg_regex_alt.hip).  In the order of the file:
//   the rules every compiler shares, one copy of each: what a search and a pattern must be (regex_check_search, regex_check_pattern),
//     where an atom ends (regex_atom), a repetition count (regex_count), the quantifier behind an operand (regex_quant), an atom's
//     class from libc's own regcomp / regexec (regex_probe_atom), the walk over a search's patterns and the frame of an entry point
//     that zeroes a refused struct (regex_each_pattern, regex_compile_zeroing), when two sequences overlap
//     (regex_branches_overlap_anchored), identical class tables merging (regex_branch_add), and the fields behind the classes
//     (regex_seq_finish, regex_alt_finish);
//   krep_gpu_regex_compile / _anchored: a TOKENISER that cuts an expression into a fixed number of one-byte atoms;
//   krep_gpu_regex_compile_alt: cuts an alternation at its top-level '|', takes one pair of parentheses off a branch and hands
//     every branch to that tokeniser;
//   krep_gpu_regex_compile_ext: EXPANDS ?, {n,m} and inner groups into such an alternation and takes a ^ in front of and a $ behind
//     every top-level branch, the same pair on all of them;
//   krep_gpu_regex_compile_loops: the expanding compiler's walk with *, + and {n,} behind an atom taken too: a place of a sequence may
//     REPEAT (C+).  It also picks the filter, the fixed-length factors the older kernels find the candidate lines with;
//   krep_gpu_regex_compile_groups: a recursive parser of its own for repeated and nested groups; it does not expand but builds the
//     position (Glushkov) automaton of the expression, cuts its follow relation into what the line walk steps (regex_groups_jumps)
//     and derives a filter from the positions every match passes;
//   the tables the kernels look a byte up in (rx_seq_table, rx_alt_table) and RegexWalk, the one program of the line walk
//     (kg_regex_loops.hip), built from a loops program, from a position automaton, or from the first rewritten as the second
//     (regex_walk_of_loops, regex_walk_of_groups, regex_walk_as_general);
//   regex_compile_search: those that take a search, in the order every search asks them, the reason it reports, and its verdict
//     RegexCompiled: which kind of program (kSeq, kAlt, kWalk), that kind's payload, and what the code around the scans asks of it.
// Each compiler reports the first fault IT meets, and they meet faults in different orders (the tokeniser probes atoms only after
// the whole pattern is cut, the expanding compiler as it goes, the alternation compiler walks a branch's parentheses before it
// tokenises the branch, the groups compiler has no "without a bound" stage): the refusal strings are public, so the shared rules sit
// under their control flows.
#pragma once
#include <regex.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/krep_gpu.h"

namespace kg {

constexpr uint32_t kRegexMaxL = 16, kRegexMaxBranches = 8, kRegexMaxTotalL = 32;

// ---- the shared rules -----------------------------------------------------------------------------------------------------------
// What every compiler asks of the search.  several_ok: the compiler takes several patterns (the alternation and the expanding one).
inline const char *regex_check_search(const search_params_t *p, bool several_ok)
{
    if (!p->use_regex)
        return "not a regex search (use_regex is not set)";
    if (!several_ok && p->num_patterns > 1)
        return "several regex patterns are an alternation (the CLI joins them with '|'): kept on krep's regex_search";
    if (p->whole_word)
        return "regex with -w: the CLI compiles \\bPATTERN\\b, a library caller PATTERN, and the operator sees neither compiled "
               "expression: kept on krep's regex_search";
    // In a multibyte locale libc's regexec matches CHARACTERS: '.', a negated or named class and, under REG_ICASE, even a letter
    // take a whole multibyte sequence as one atom, so no pattern is a fixed number of BYTE classes there and one-byte probes cannot
    // say what an atom matches.  The krep CLI never calls setlocale(): it runs in the C locale, where a character is a byte.
    if (MB_CUR_MAX > 1)
        return "regex in a multibyte locale (the process called setlocale): libc matches characters there, not bytes: kept on "
               "krep's regex_search (krep itself runs in the C locale)";
    if (several_ok && p->num_patterns > 1 && !(p->patterns && p->pattern_lens))
        return "several patterns announced but patterns / pattern_lens are NULL";
    return nullptr;
}
// ... and of every pattern
inline const char *regex_check_pattern(const uint8_t *pat, size_t n)
{
    if (!pat)
        return "no pattern";
    if (n == 0)
        return "an empty regex matches the empty string: kept on krep's regex_search";
    if (n > 1024)
        return "regex pattern longer than 1024 bytes";
    for (size_t i = 0; i < n; ++i)
        if (pat[i] < 0x01 || pat[i] > 0x7f)
            return "regex pattern holds a byte outside 0x01-0x7F";
    return nullptr;
}

inline bool regex_is_punct(uint8_t c) { return (c >= 0x21 && c <= 0x2f) || (c >= 0x3a && c <= 0x40) || (c >= 0x5b && c <= 0x60) || (c >= 0x7b && c <= 0x7e); }

// the closing ']' of the bracket expression that opens at pat[i] (POSIX 9.3.5): an optional '^', a ']' directly behind that is
// literal, [:name:] [.x.] [=x=] are stepped over.  Returns its index, or n when the expression is not closed.
inline size_t regex_bracket_end(const uint8_t *pat, size_t n, size_t i)
{
    size_t k = i + 1;
    if (k < n && pat[k] == '^')
        ++k;
    if (k < n && pat[k] == ']')
        ++k;
    while (k < n && pat[k] != ']')
    {
        if (pat[k] == '[' && k + 1 < n && (pat[k + 1] == ':' || pat[k + 1] == '.' || pat[k + 1] == '='))
        {
            const uint8_t close = pat[k + 1];
            size_t e = k + 2;
            while (e + 1 < n && !(pat[e] == close && pat[e + 1] == ']'))
                ++e;
            if (e + 1 >= n)
                return n;
            k = e + 2;
        }
        else
            ++k;
    }
    return k;
}
// The atom at pat[i], i < n: an ordinary byte, a backslash with the punctuation byte behind it, a bracket expression up to its ']'.
// NULL and its length in *len, or why it is none.  A refused escape still spans *len = 2 bytes (who only looks for the operators
// between the atoms steps over it and leaves the reason to the compiler of the branch); *len = 0: the pattern ends inside the atom.
inline const char *regex_atom(const uint8_t *pat, size_t n, size_t i, size_t *len)
{
    *len = 1;
    if (pat[i] == '\\')
    {
        *len = 0;
        if (i + 1 >= n)
            return "regex: trailing backslash";
        *len = 2;
        const uint8_t e = pat[i + 1];
        if ((e >= '0' && e <= '9') || ((e | 0x20) >= 'a' && (e | 0x20) <= 'z'))
            return "regex: a backslash in front of a letter or digit (\\b, \\w, \\1, ...) is an operator: kept on krep's regex_search";
        if (!regex_is_punct(e))
            return "regex: a backslash in front of a byte that is not punctuation";
    }
    else if (pat[i] == '[')
    {
        const size_t e = regex_bracket_end(pat, n, i);
        *len = e < n ? e + 1 - i : 0;
        if (e >= n)
            return "regex: bracket expression without its ']'";
    }
    return nullptr;
}
// The count of a repetition, digits from pat[*k] on: its value (read up to the first digit that takes it past 1000) in *v, *k behind
// it.  false: no digit, or the pattern ends behind the digits — malformed, like whatever the caller does not find behind the count.
constexpr const char *kRegexMalformed = "regex: malformed repetition";
inline bool regex_count(const uint8_t *pat, size_t n, size_t *k, uint32_t *v)
{
    bool digits = false;
    *v = 0;
    while (*k < n && pat[*k] >= '0' && pat[*k] <= '9' && *v <= 1000)
    {
        *v = *v * 10 + (uint32_t)(pat[*k] - '0');
        digits = true;
        ++*k;
    }
    return digits && *k < n;
}

// The class of one atom: the bytes b for which libc's regexec, with the atom compiled alone under the reference's flags
// (krep.c:2148), matches the one-byte text b.  false: regcomp refused the atom.
inline bool regex_probe_atom(const uint8_t *atom, size_t len, bool case_sensitive, uint8_t cls[32])
{
    char buf[1032];
    if (len >= sizeof buf)
        return false;
    memcpy(buf, atom, len);
    buf[len] = 0;
    regex_t re;
    if (regcomp(&re, buf, REG_EXTENDED | REG_NEWLINE | (case_sensitive ? 0 : REG_ICASE)) != 0)
        return false;
    memset(cls, 0, 32);
    for (int b = 0; b < 256; ++b)
    {
        const char t[2] = {(char)b, 0};
        regmatch_t m;
        m.rm_so = 0;
        m.rm_eo = 1;
        if (regexec(&re, t, 1, &m, REG_STARTEND) == 0 && m.rm_so == 0 && m.rm_eo == 1)
            cls[b >> 3] |= (uint8_t)(1u << (b & 7));
    }
    regfree(&re);
    return true;
}
constexpr const char *kRegexAtomRefused = "regex: regcomp refuses an atom of the pattern";

// The quantifier behind an operand, pat[*i] one of ? * + {: ? is {0,1}, * is {0,}, + is {1,}, {n} {n,} {n,m} with counts up to 1000.
// kNone: *q says it (hi == lo when unbounded) and *i stands behind it.  Else the first fault in the order every caller reports them:
// without unbounded_ok a * or + (kStarPlus) and a {n,} (kOpenCount) where it is met, before the range is judged; a malformed or
// reversed range or a count past 1000; a range that ends at 0; a second quantifier behind this one.  The strings are the callers'.
struct RegexQuant { uint32_t lo, hi; bool unbounded; };
enum class RegexQuantFault { kNone, kStarPlus, kOpenCount, kMalformed, kZero, kBehindQuant };
inline bool regex_is_quant(uint8_t c) { return c == '?' || c == '*' || c == '+' || c == '{'; }
inline RegexQuantFault regex_quant(const uint8_t *pat, size_t n, size_t *i, bool unbounded_ok, RegexQuant *q)
{
    *q = RegexQuant{0, 1, false};
    if (pat[*i] == '*' || pat[*i] == '+')
    {
        if (!unbounded_ok)
            return RegexQuantFault::kStarPlus;
        *q = RegexQuant{pat[*i] == '+' ? 1u : 0u, pat[*i] == '+' ? 1u : 0u, true};
        ++*i;
    }
    else if (pat[*i] == '?')
        ++*i;
    else
    {
        size_t k = *i + 1;
        if (!regex_count(pat, n, &k, &q->lo))
            return RegexQuantFault::kMalformed;
        q->hi = q->lo;
        if (pat[k] == ',')
        {
            ++k;
            if (k < n && pat[k] == '}')
            {
                if (!unbounded_ok)
                    return RegexQuantFault::kOpenCount;
                q->unbounded = true;
            }
            else if (!regex_count(pat, n, &k, &q->hi))
                return RegexQuantFault::kMalformed;
        }
        if (pat[k] != '}' || q->lo > q->hi || q->hi > 1000)
            return RegexQuantFault::kMalformed;
        if (!q->unbounded && q->hi == 0)
            return RegexQuantFault::kZero;
        *i = k + 1;
    }
    return *i < n && regex_is_quant(pat[*i]) ? RegexQuantFault::kBehindQuant : RegexQuantFault::kNone;
}

// What the entry points that take several patterns share.  The frame: NULL params, *out zeroed, the compiler, *out zeroed again when
// it refuses.  The walk: what the search must be, then every pattern fetched, checked and handed to each(pat, n).
// the patterns a search names: patterns[0..num_patterns) when the arrays are there, else pattern alone
inline size_t regex_pattern_count(const search_params_t *p) { return (p->num_patterns >= 1 && p->patterns && p->pattern_lens) ? p->num_patterns : 1; }
inline void regex_pattern_at(const search_params_t *p, size_t k, const uint8_t **pat, size_t *n)
{
    const bool arrays = p->num_patterns >= 1 && p->patterns && p->pattern_lens;
    *pat = (const uint8_t *)(arrays ? p->patterns[k] : p->pattern);
    *n = arrays ? p->pattern_lens[k] : p->pattern_len;
}
template <class Out, class Compile> inline const char *regex_compile_zeroing(const search_params_t *p, Out *out, Compile compile)
{
    if (!p || !out)
        return "NULL params";
    memset(out, 0, sizeof *out);
    const char *why = compile(p, out);
    if (why)
        memset(out, 0, sizeof *out);
    return why;
}
template <class Each> inline const char *regex_each_pattern(const search_params_t *p, Each each)
{
    if (const char *why = regex_check_search(p, true))
        return why;
    const size_t n_pat = regex_pattern_count(p);
    for (size_t k = 0; k < n_pat; ++k)
    {
        const uint8_t *pat;
        size_t n;
        regex_pattern_at(p, k, &pat, &n);
        if (const char *why = regex_check_pattern(pat, n))
            return why;
        if (const char *why = each(pat, n))
            return why;
    }
    return nullptr;
}

inline bool regex_classes_meet(const uint8_t a[32], const uint8_t b[32])
{
    for (int w = 0; w < 32; ++w)
        if (a[w] & b[w])
            return true;
    return false;
}
inline bool regex_class_holds_nl(const uint8_t cls[32]) { return ((cls['\n' >> 3] >> ('\n' & 7)) & 1u) != 0; }
// Can an occurrence of sequence j start d bytes into an occurrence of sequence i (every class pair that lies on one byte meets) when
// both stand between the same anchors.  d == 0 (the same start) is never ruled out by an anchor.  d >= 1 under ^: the byte in front
// of j lies inside i.  Under $: the byte behind the occurrence that ends first lies inside the other one.
inline bool regex_branches_overlap_anchored(const krep_gpu_regex_info_t &bi, const krep_gpu_regex_info_t &bj, uint32_t d, bool bol, bool eol)
{
    for (uint32_t t = 0; d + t < bi.L && t < bj.L; ++t)
        if (!regex_classes_meet(bi.classes[d + t], bj.classes[t]))
            return false;
    if (d == 0)
        return true;
    if (bol && !regex_class_holds_nl(bi.classes[d - 1]))
        return false;
    if (eol && bi.L - d < bj.L && !regex_class_holds_nl(bj.classes[bi.L - d]))
        return false;
    if (eol && d + bj.L < bi.L && !regex_class_holds_nl(bi.classes[d + bj.L]))
        return false;
    return true;
}
// While a compiler expands an expression, a sequence keeps the 16-bit mask of its places that REPEAT (C+, the loops compiler) in its
// `anchor` field, which means nothing until regex_seq_finish() sets it: 0 in every sequence of the older compilers.
inline uint32_t &regex_seq_plus(krep_gpu_regex_info_t &q) { return q.anchor; }
inline uint32_t regex_seq_plus(const krep_gpu_regex_info_t &q) { return q.anchor; }
// q among the *n distinct sequences of `set` (room for 8; L, the classes and the repeat mask are compared): identical ones merge.
// false: it would be the ninth.
inline bool regex_branch_add(krep_gpu_regex_info_t *set, uint32_t *n, const krep_gpu_regex_info_t &q)
{
    for (uint32_t i = 0; i < *n; ++i)
        if (set[i].L == q.L && regex_seq_plus(set[i]) == regex_seq_plus(q) && memcmp(set[i].classes, q.classes, (size_t)q.L * 32) == 0)
            return true;
    if (*n >= kRegexMaxBranches)
        return false;
    set[(*n)++] = q;
    return true;
}
// The fields behind the classes of a sequence whose L and classes are set: the anchor class with its bytes, and self_overlap (a
// shift d >= 1 at which the sequence, between its anchors, overlaps itself)
inline void regex_seq_finish(krep_gpu_regex_info_t *out, bool bol, bool eol)
{
    const uint32_t L = out->L;
    auto size_of = [&](uint32_t k) {
        uint32_t s = 0;
        for (int b = 0; b < 256; ++b)
            s += (out->classes[k][b >> 3] >> (b & 7)) & 1u;
        return s;
    };
    uint32_t best = 0, best_n = size_of(0);
    for (uint32_t k = 1; k < L; ++k)
        if (const uint32_t s = size_of(k); s < best_n)
        {
            best = k;
            best_n = s;
        }
    out->anchor = best;
    if (best_n >= 1 && best_n <= 4)
        for (int b = 0; b < 256; ++b)
            if ((out->classes[best][b >> 3] >> (b & 7)) & 1u)
                out->anchor_bytes[out->n_anchor++] = (uint8_t)b;
    for (uint32_t d = 1; d < L && !out->self_overlap; ++d)
        out->self_overlap = regex_branches_overlap_anchored(*out, *out, d, bol, eol) ? 1 : 0;
}
// The fields behind the branches of an alternation whose n_branches and branch[] are set: Lmin, Lmax, total_L and cross_overlap
// (two occurrences, of one branch at a shift d >= 1 or of two at any shift, can share a byte between the anchors)
inline void regex_alt_finish(krep_gpu_regex_alt_t *alt, bool bol, bool eol)
{
    alt->Lmin = kRegexMaxL;
    for (uint32_t b = 0; b < alt->n_branches; ++b)
    {
        const uint32_t L = alt->branch[b].L;
        alt->Lmin = L < alt->Lmin ? L : alt->Lmin;
        alt->Lmax = L > alt->Lmax ? L : alt->Lmax;
        alt->total_L += L;
    }
    for (uint32_t i = 0; i < alt->n_branches && !alt->cross_overlap; ++i)
        for (uint32_t j = 0; j < alt->n_branches && !alt->cross_overlap; ++j)
            for (uint32_t d = i == j ? 1u : 0u; d < alt->branch[i].L && !alt->cross_overlap; ++d)
                alt->cross_overlap = regex_branches_overlap_anchored(alt->branch[i], alt->branch[j], d, bol, eol) ? 1 : 0;
}

// ---- krep_gpu_regex_compile, krep_gpu_regex_compile_anchored: one sequence of byte classes ----------------------------------------
// one atom of the pattern: bytes [at, at + len) of it, `rep` times in a row
struct RegexAtom { size_t at, len; uint32_t rep; };

constexpr const char *kRegexSeqTooManyClasses = "regex: more than 16 byte classes in a row";
constexpr const char *kRegexSeqTooManyPlaces = "regex: more than 16 places in a row (^ and $ take one each beside the byte classes)";

// Both entry points.  anchors: a '^' as the first and a '$' as the last pattern byte are line anchors (krep_gpu_regex_compile_anchored);
// without it they are refused like everywhere else in the pattern (krep_gpu_regex_compile, whose struct cannot say them).
// NULL: `out`, *bol and *eol are filled.  Else why the pattern is not taken (a string literal).
inline const char *regex_compile_seq(const search_params_t *p, bool anchors, krep_gpu_regex_info_t *out, int *bol_out, int *eol_out)
{
    memset(out, 0, sizeof *out);
    *bol_out = *eol_out = 0;
    if (const char *why = regex_check_search(p, false))
        return why;
    const uint8_t *pat = (const uint8_t *)p->pattern;
    size_t n = p->pattern_len;
    if (p->num_patterns == 1 && p->patterns && p->pattern_lens && p->patterns[0])
    {
        pat = (const uint8_t *)p->patterns[0];
        n = p->pattern_lens[0];
    }
    if (const char *why = regex_check_pattern(pat, n))
        return why;
    RegexAtom atoms[kRegexMaxL];
    uint32_t n_atoms = 0, L = 0;
    bool repeatable = false; // the token in front is an atom that has no repetition yet
    bool bol = false, eol = false;
    for (size_t i = 0; i < n;)
    {
        const uint8_t c = pat[i];
        // (the loop steps over escapes and bracket expressions whole: a '^' or '$' it stands on is an unescaped one outside brackets)
        if ((c == '^' && i == 0) || (c == '$' && i + 1 == n))
        {
            if (!anchors)
                return "regex: a line anchor (^ in front, $ at the end) is not a byte class and krep_gpu_regex_info_t cannot say it: "
                       "krep_gpu_regex_compile_anchored() takes it";
            (c == '^' ? bol : eol) = true;
            repeatable = false;
            ++i;
            continue;
        }
        if (c == '^' || c == '$')
            return "regex: ^ that is not the first or $ that is not the last byte of the pattern (a^b, a$b, ^^a, a$$) anchors inside "
                   "the sequence: kept on krep's regex_search";
        if (c == '{')
        {
            if (bol && i == 1)
                return "regex: a repetition directly behind ^ repeats the anchor: kept on krep's regex_search";
            if (!repeatable)
                return "regex: '{' not behind an atom";
            size_t k = i + 1;
            uint32_t v;
            if (!regex_count(pat, n, &k, &v))
                return kRegexMalformed;
            if (pat[k] == ',')
                return "regex: {n,} and {n,m} repeat a varying number of times: kept on krep's regex_search";
            if (pat[k] != '}')
                return kRegexMalformed;
            if (v < 1)
                return "regex: {0} makes an atom optional: kept on krep's regex_search";
            if (L - 1 + v > kRegexMaxL)
                return kRegexSeqTooManyClasses;
            L += v - 1;
            atoms[n_atoms - 1].rep = v;
            repeatable = false;
            i = k + 1;
            continue;
        }
        if (c == '(' || c == ')' || c == '*' || c == '+' || c == '?' || c == '|')
            return "regex: ( ) * + ? | make a general automaton: kept on krep's regex_search";
        size_t len;
        if (const char *why = regex_atom(pat, n, i, &len))
            return why;
        if (L + 1 > kRegexMaxL)
            return kRegexSeqTooManyClasses;
        atoms[n_atoms++] = RegexAtom{i, len, 1};
        ++L;
        repeatable = true;
        i += len;
    }
    if (L < 1)
        return (bol || eol) ? "regex: ^, $ and ^$ on their own match the empty string: kept on krep's regex_search" : "regex: no atom";
    if (L + bol + eol > kRegexMaxL)
        return kRegexSeqTooManyPlaces;
    uint32_t j = 0;
    for (uint32_t a = 0; a < n_atoms; ++a)
    {
        uint8_t cls[32];
        if (!regex_probe_atom(pat + atoms[a].at, atoms[a].len, p->case_sensitive, cls))
            return kRegexAtomRefused;
        for (uint32_t r = 0; r < atoms[a].rep; ++r)
            memcpy(out->classes[j++], cls, 32);
    }
    out->L = L;
    regex_seq_finish(out, bol, eol);
    *bol_out = bol;
    *eol_out = eol;
    return nullptr;
}
// krep_gpu_regex_compile: exactly the unanchored grammar
inline const char *regex_compile(const search_params_t *p, krep_gpu_regex_info_t *out)
{
    if (!p || !out)
        return "NULL params";
    int bol, eol;
    return regex_compile_seq(p, false, out, &bol, &eol);
}
// krep_gpu_regex_compile_anchored: the same with an optional ^ in front and an optional $ at the end
inline const char *regex_compile_anchored(const search_params_t *p, krep_gpu_regex_anchored_t *out)
{
    if (!p || !out)
        return "NULL params";
    out->bol = out->eol = 0;
    return regex_compile_seq(p, true, &out->seq, &out->bol, &out->eol);
}

// ---- krep_gpu_regex_compile_alt: an alternation of class sequences ------------------------------------------------------------
// does the search say an alternation: several patterns, or a '|' or '(' outside brackets and not behind a backslash
inline bool regex_has_alt_syntax(const search_params_t *p)
{
    if (!p || !p->use_regex)
        return false;
    if (p->num_patterns > 1)
        return true;
    const uint8_t *pat;
    size_t n;
    regex_pattern_at(p, 0, &pat, &n);
    if (!pat)
        return false;
    for (size_t i = 0, len; i < n; i += len)
    {
        if (pat[i] == '|' || pat[i] == '(')
            return true;
        if (regex_atom(pat, n, i, &len) && !len)
            break;
    }
    return false;
}
constexpr const char *kRegexAltEmptyBranch = "regex alternation: an empty branch (a|, |a, (), a||b) matches the empty string: kept on krep's regex_search";
constexpr const char *kRegexAltUnbalanced = "regex alternation: unbalanced parentheses: kept on krep's regex_search";
constexpr const char *kRegexAltNested = "regex alternation: nested parentheses: kept on krep's regex_search";
constexpr const char *kRegexAltGroupNotBranch = "regex alternation: a group that is not a whole branch ((ab)c, (ab){2}, x(a|b)y) is a general automaton: kept on "
                                                "krep's regex_search";
constexpr const char *kRegexAltGroupHoldsAlt = "regex alternation: a group that holds an alternation ((a|b)) is not one class sequence: kept on krep's regex_search";
constexpr const char *kRegexAltMixedAnchors = "regex alternation: ^ or $ in a branch (anchors inside an alternation): kept on krep's regex_search";
constexpr const char *kRegexAltBranchTooLong = "regex alternation: a branch of more than 16 byte classes: kept on krep's regex_search";
constexpr const char *kRegexAltTooManyBranches = "regex alternation: more than 8 branches: kept on krep's regex_search";
constexpr const char *kRegexAltTooWide = "regex alternation: more than 32 byte classes in all branches together: kept on krep's regex_search";

// The top-level branch of pat that begins at bs: *end its '|' or n, [*lo, *hi) its sequence with the one pair of parentheses around it
// taken off.  The walk reports what it meets first, a misplaced parenthesis or anchor or an atom the pattern ends in; every other
// fault of an atom is the tokeniser's, which gets the sequence.
inline const char *regex_alt_branch(const uint8_t *pat, size_t n, size_t bs, size_t *lo, size_t *hi, size_t *end)
{
    size_t i = bs, inner = bs;         // inner: where the sequence begins, behind a '('
    bool open = false, closed = false; // inside the branch's group | its ')' is behind the cursor
    while (i < n && pat[i] != '|')
    {
        const uint8_t c = pat[i];
        if ((closed && c != ')') || (c == '(' && !open && i != bs))
            return kRegexAltGroupNotBranch;
        size_t len = 1;
        if (c == '(')
        {
            if (open)
                return kRegexAltNested;
            open = true;
            inner = i + 1;
        }
        else if (c == ')')
        {
            if (!open)
                return kRegexAltUnbalanced;
            open = false;
            closed = true;
            if (i == inner)
                return kRegexAltEmptyBranch;
        }
        else if (c == '^' || c == '$')
            return kRegexAltMixedAnchors;
        else if (const char *why = regex_atom(pat, n, i, &len); why && !len)
            return why;
        i += len;
    }
    if (open)
        return i < n ? kRegexAltGroupHoldsAlt : kRegexAltUnbalanced;
    *lo = closed ? inner : bs;
    *hi = closed ? i - 1 : i;
    *end = i;
    return *hi <= *lo ? kRegexAltEmptyBranch : nullptr;
}
inline const char *regex_compile_alt_branches(const search_params_t *p, krep_gpu_regex_alt_t *out)
{
    const char *why = regex_each_pattern(p, [&](const uint8_t *pat, size_t n) -> const char * {
        for (size_t bs = 0, end; bs <= n; bs = end + 1) // (a '|' at the very end has an empty branch behind it)
        {
            size_t lo, hi;
            if (const char *why = regex_alt_branch(pat, n, bs, &lo, &hi, &end))
                return why;
            search_params_t q = *p;
            q.pattern = (const char *)pat + lo;
            q.pattern_len = hi - lo;
            q.patterns = nullptr;
            q.pattern_lens = nullptr;
            q.num_patterns = 0;
            krep_gpu_regex_info_t info;
            int bol, eol;
            if (const char *why = regex_compile_seq(&q, false, &info, &bol, &eol))
                return why == kRegexSeqTooManyClasses ? kRegexAltBranchTooLong : why;
            if (!regex_branch_add(out->branch, &out->n_branches, info))
                return kRegexAltTooManyBranches;
        }
        return nullptr;
    });
    if (why)
        return why;
    regex_alt_finish(out, false, false);
    return out->total_L > kRegexMaxTotalL ? kRegexAltTooWide : nullptr;
}
// krep_gpu_regex_compile_alt: NULL and *out filled, or the refusal and *out zeroed
inline const char *regex_compile_alt(const search_params_t *p, krep_gpu_regex_alt_t *out) { return regex_compile_zeroing(p, out, regex_compile_alt_branches); }

// ---- krep_gpu_regex_compile_ext: ?, {n,m}, inner groups and anchored alternations, expanded into class sequences --------------
// A partial expansion: at most 8 distinct sequences (only L and classes of each are in use; L == 0 is the empty sequence).  The
// number of distinct sequences never shrinks when something is put behind all of them, and no sequence gets shorter, so a set
// that passes 8 sequences or a sequence that passes 16 classes ends the expansion at once.
struct RegexSeqSet
{
    uint32_t n;
    krep_gpu_regex_info_t s[kRegexMaxBranches];
};
constexpr const char *kRegexExtTooMany = "regex expansion: ?, {n,m} and groups multiply out to more than 8 distinct class sequences: kept on krep's regex_search";
constexpr const char *kRegexExtTooLong = "regex expansion: a sequence of more than 16 places (^ and $ take one each beside the byte classes): kept on krep's "
                                         "regex_search";
constexpr const char *kRegexExtTooWide = "regex expansion: more than 32 places in all sequences together (^ and $ take one each in every sequence): kept on "
                                         "krep's regex_search";
constexpr const char *kRegexExtEmpty = "regex expansion: one of the sequences holds no byte class (a?, (a|b)?, a{0,1}): it matches the empty string: kept on "
                                       "krep's regex_search";
inline bool regex_ext_own_limit(const char *why) { return why == kRegexExtTooMany || why == kRegexExtTooLong || why == kRegexExtTooWide || why == kRegexExtEmpty; }

inline const char *regex_set_union(RegexSeqSet &S, const RegexSeqSet &A)
{
    for (uint32_t i = 0; i < A.n; ++i)
        if (!regex_branch_add(S.s, &S.n, A.s[i]))
            return kRegexExtTooMany;
    return nullptr;
}
// C = every sequence of A with every sequence of B behind it
inline const char *regex_set_cat(const RegexSeqSet &A, const RegexSeqSet &B, RegexSeqSet &C)
{
    C.n = 0;
    for (uint32_t i = 0; i < A.n; ++i)
        for (uint32_t j = 0; j < B.n; ++j)
        {
            if (A.s[i].L + B.s[j].L > kRegexMaxL)
                return kRegexExtTooLong;
            krep_gpu_regex_info_t q = A.s[i];
            regex_seq_plus(q) |= regex_seq_plus(B.s[j]) << A.s[i].L;
            for (uint32_t t = 0; t < B.s[j].L; ++t)
                memcpy(q.classes[q.L++], B.s[j].classes[t], 32);
            if (!regex_branch_add(C.s, &C.n, q))
                return kRegexExtTooMany;
        }
    return nullptr;
}
inline void regex_set_empty_seq(RegexSeqSet &S)
{
    memset(&S, 0, sizeof S);
    S.n = 1;
}
// A{lo,hi}: lo..hi sequences of A in a row (hi >= 1)
inline const char *regex_set_repeat(RegexSeqSet &A, uint32_t lo, uint32_t hi)
{
    RegexSeqSet P, R, T;
    regex_set_empty_seq(P);
    memset(&R, 0, sizeof R);
    for (uint32_t k = 0;; ++k)
    {
        if (k >= lo)
            if (const char *why = regex_set_union(R, P))
                return why;
        if (k == hi)
            break;
        if (const char *why = regex_set_cat(P, A, T))
            return why;
        P = T;
    }
    A = R;
    return nullptr;
}

// the cursor over one pattern
struct RegexExtCursor
{
    const uint8_t *pat;
    size_t n, i;
    bool case_sensitive;
    bool loops = false;     // the loops compiler: *, + and {n,} behind an atom are taken
    bool unbounded = false; // ... and one of them has been met
};
constexpr const char *kRegexStarPlus = "regex: * and + repeat without a bound, which needs an unbounded state: kept on krep's regex_search";
constexpr const char *kRegexOpenCount = "regex: {n,} repeats without a bound, which needs an unbounded state: kept on krep's regex_search";
constexpr const char *kRegexLoopsGroup = "regex loops: *, + or {n,} behind a group ((ab)+, (a|b)*) loops over a sub-sequence, not over one byte class: kept on "
                                         "krep's regex_search";
// an optional quantifier at the cursor, applied to A (atom: A is one atom's single place, else a group's alternatives)
inline const char *regex_ext_quant(RegexExtCursor &c, RegexSeqSet &A, bool atom)
{
    if (c.i >= c.n || !regex_is_quant(c.pat[c.i]))
        return nullptr;
    RegexQuant q;
    switch (regex_quant(c.pat, c.n, &c.i, c.loops, &q))
    {
    case RegexQuantFault::kNone: break;
    case RegexQuantFault::kStarPlus: return kRegexStarPlus;
    case RegexQuantFault::kOpenCount: return kRegexOpenCount;
    case RegexQuantFault::kMalformed: return kRegexMalformed;
    case RegexQuantFault::kZero: return "regex: {0} repeats an atom zero times, a{0} matches the empty string: kept on krep's regex_search";
    case RegexQuantFault::kBehindQuant: return "regex: a quantifier behind a quantifier (a?{2}, a{2}{3}, a?+): kept on krep's regex_search";
    }
    if (!q.unbounded)
        return regex_set_repeat(A, q.lo, q.hi);
    // C+ is the place C that repeats; C{n,} is C n - 1 times and then C+; C* and C{0,} are nothing, or C+
    if (!atom)
        return kRegexLoopsGroup;
    c.unbounded = true;
    RegexSeqSet plus = A, T;
    regex_seq_plus(plus.s[0]) = 1u;
    if (q.lo == 0)
    {
        regex_set_empty_seq(A);
        return regex_set_union(A, plus);
    }
    if (const char *why = regex_set_repeat(A, q.lo - 1, q.lo - 1))
        return why;
    if (const char *why = regex_set_cat(A, plus, T))
        return why;
    A = T;
    return nullptr;
}
// one atom at the cursor with its optional quantifier: its alternatives into A
inline const char *regex_ext_atom(RegexExtCursor &c, RegexSeqSet &A)
{
    size_t len;
    if (const char *why = regex_atom(c.pat, c.n, c.i, &len))
        return why;
    regex_set_empty_seq(A);
    if (!regex_probe_atom(c.pat + c.i, len, c.case_sensitive, A.s[0].classes[0]))
        return kRegexAtomRefused;
    A.s[0].L = 1;
    c.i += len;
    return regex_ext_quant(c, A, true);
}
// a group, the cursor behind its '(': '(' seq ('|' seq)* ')' quant?, seq = (atom quant?)+
inline const char *regex_ext_group(RegexExtCursor &c, RegexSeqSet &G)
{
    RegexSeqSet cur, A, T;
    memset(&G, 0, sizeof G);
    regex_set_empty_seq(cur);
    bool any = false; // the alternative under the cursor holds an atom
    for (;;)
    {
        if (c.i >= c.n)
            return kRegexAltUnbalanced;
        const uint8_t ch = c.pat[c.i];
        if (ch == '(')
            return kRegexAltNested;
        if (ch == '^' || ch == '$')
            return "regex: ^ or $ inside a group anchors in the middle of the expression: kept on krep's regex_search";
        if (ch == '|' || ch == ')')
        {
            if (!any)
                return "regex alternation: an empty alternative in a group ((), (a|), (|a)) matches the empty string: kept on krep's "
                       "regex_search";
            if (const char *why = regex_set_union(G, cur))
                return why;
            regex_set_empty_seq(cur);
            any = false;
            ++c.i;
            if (ch == ')')
                return regex_ext_quant(c, G, false);
            continue;
        }
        if (regex_is_quant(ch))
            return "regex: a quantifier that is not behind an atom or a group";
        if (const char *why = regex_ext_atom(c, A))
            return why;
        if (const char *why = regex_set_cat(cur, A, T))
            return why;
        cur = T;
        any = true;
    }
}
// one top-level branch, up to its '|' or the end of the pattern: ['^'] item+ ['$']
inline const char *regex_ext_branch(RegexExtCursor &c, RegexSeqSet &S, int *bol, int *eol)
{
    RegexSeqSet A, T;
    regex_set_empty_seq(S);
    *bol = *eol = 0;
    bool any = false;
    if (c.i < c.n && c.pat[c.i] == '^')
    {
        *bol = 1;
        ++c.i;
    }
    while (c.i < c.n && c.pat[c.i] != '|')
    {
        const uint8_t ch = c.pat[c.i];
        if (ch == '$' && (c.i + 1 == c.n || c.pat[c.i + 1] == '|'))
        {
            *eol = 1;
            ++c.i;
            break;
        }
        if (ch == '^' || ch == '$')
            return "regex: ^ that is not the first or $ that is not the last byte of a branch (a^b, a$b, ^^a, a$$) anchors in the middle of "
                   "the expression: kept on krep's regex_search";
        if (ch == ')')
            return kRegexAltUnbalanced;
        if (regex_is_quant(ch))
            return (*bol && !any) ? "regex: a repetition directly behind ^ repeats the anchor: kept on krep's regex_search"
                                  : "regex: a quantifier that is not behind an atom or a group";
        if (ch == '(')
        {
            ++c.i;
            if (const char *why = regex_ext_group(c, A))
                return why;
        }
        else if (const char *why = regex_ext_atom(c, A))
            return why;
        if (const char *why = regex_set_cat(S, A, T))
            return why;
        S = T;
        any = true;
    }
    if (!any)
        return (*bol || *eol) ? "regex: ^, $ and ^$ on their own match the empty string: kept on krep's regex_search" : kRegexAltEmptyBranch;
    for (uint32_t k = 0; k < S.n; ++k)
        if (S.s[k].L == 0)
            return kRegexExtEmpty;
    return nullptr;
}
// loops: *, + and {n,} behind an atom are taken too (the loops compiler); plus[b]: the repeat mask of branch b, *unbounded: one was met
inline const char *regex_compile_ext_branches(const search_params_t *p, krep_gpu_regex_ext_t *out, bool loops = false, uint32_t *plus = nullptr,
                                              bool *unbounded = nullptr)
{
    krep_gpu_regex_alt_t &alt = out->alt;
    bool first = true;
    const char *why = regex_each_pattern(p, [&](const uint8_t *pat, size_t n) -> const char * {
        RegexExtCursor c{pat, n, 0, p->case_sensitive, loops};
        for (;;)
        {
            RegexSeqSet S;
            int bol, eol;
            if (const char *why = regex_ext_branch(c, S, &bol, &eol))
                return why;
            if (first)
            {
                out->bol = bol;
                out->eol = eol;
                first = false;
            }
            else if (bol != out->bol || eol != out->eol)
                return kRegexAltMixedAnchors;
            for (uint32_t b = 0; b < S.n; ++b)
                if (!regex_branch_add(alt.branch, &alt.n_branches, S.s[b]))
                    return kRegexExtTooMany;
            if (c.i >= c.n)
                break;
            ++c.i; // the '|'
            if (c.i >= c.n)
                return kRegexAltEmptyBranch;
        }
        if (unbounded)
            *unbounded = *unbounded || c.unbounded;
        return nullptr;
    });
    if (why)
        return why;
    const uint32_t extra = (uint32_t)(out->bol + out->eol);
    for (uint32_t b = 0; b < alt.n_branches; ++b)
    {
        if (alt.branch[b].L + extra > kRegexMaxL)
            return kRegexExtTooLong;
        if (plus)
            plus[b] = regex_seq_plus(alt.branch[b]);
        regex_seq_plus(alt.branch[b]) = 0;
        regex_seq_finish(&alt.branch[b], false, false); // (each branch what krep_gpu_regex_compile() makes of it alone)
    }
    regex_alt_finish(&alt, out->bol != 0, out->eol != 0);
    if (alt.total_L + alt.n_branches * extra > kRegexMaxTotalL)
        return kRegexExtTooWide;
    return nullptr;
}
// krep_gpu_regex_compile_ext: NULL and *out filled, or the refusal and *out zeroed
inline const char *regex_compile_ext(const search_params_t *p, krep_gpu_regex_ext_t *out)
{
    return regex_compile_zeroing(p, out, [](const search_params_t *q, krep_gpu_regex_ext_t *o) { return regex_compile_ext_branches(q, o); });
}

// ---- krep_gpu_regex_compile_loops: *, + and {n,} behind an atom, expanded into sequences of places that may repeat ------------------
constexpr const char *kRegexLoopsEmpty = "regex loops: one of the expanded sequences holds no place (a*, a*b*, (a|b*)): it matches the empty string: kept on "
                                         "krep's regex_search";
constexpr const char *kRegexLoopsNewline = "regex loops: a byte class of the expression holds '\\n', so a match can cross a line end and the lines of the text "
                                           "are no longer independent: kept on krep's regex_search";
constexpr const char *kRegexLoopsNone = "regex loops: the expression holds no *, + or {n,}: it is the older compilers' (krep_gpu_regex_compile_anchored, _alt, "
                                        "_ext)";
// the bytes of a class
inline uint32_t regex_class_size(const uint8_t cls[32])
{
    uint32_t s = 0;
    for (int w = 0; w < 32; ++w)
        s += (uint32_t)__builtin_popcount(cls[w]);
    return s;
}
// The filter of a compiled program: per branch the factor (a run of places none of which, strictly inside it, repeats) whose classes
// have the smallest product of |class| / 256; on a tie the longer, then the leftmost; identical factors merge.
inline void regex_loops_filter(krep_gpu_regex_loops_t *out)
{
    for (uint32_t i = 0; i < out->alt.n_branches; ++i)
    {
        const krep_gpu_regex_info_t &br = out->alt.branch[i];
        const uint32_t plus = out->repeat[i];
        uint32_t best_a = 0, best_len = 0;
        unsigned __int128 best = 0;
        for (uint32_t a = 0; a < br.L; ++a)
        {
            unsigned __int128 prod = 1;
            for (uint32_t b = a; b < br.L; ++b)
            {
                // (no class holds '\n': every |class| <= 255, so the product of len of them stays below 256^len <= 2^128)
                prod *= regex_class_size(br.classes[b]);
                const uint32_t len = b - a + 1;
                const unsigned __int128 v = prod << (8u * (kRegexMaxL - len)); // the product over 256^len, times 256^16
                if (!best_len || v < best || (v == best && len > best_len))
                {
                    best = v;
                    best_a = a;
                    best_len = len;
                }
                if (b > a && ((plus >> b) & 1u))
                    break; // a repeating place ends the run: it may stand at an end of a factor, never inside
            }
        }
        krep_gpu_regex_info_t q{};
        q.L = best_len;
        memcpy(q.classes, br.classes[best_a], (size_t)best_len * 32);
        (void)regex_branch_add(out->filter.branch, &out->filter.n_branches, q); // (at most one per branch: never a ninth)
    }
    for (uint32_t b = 0; b < out->filter.n_branches; ++b)
        regex_seq_finish(&out->filter.branch[b], false, false);
    regex_alt_finish(&out->filter, false, false);
}
inline const char *regex_compile_loops_expand(const search_params_t *p, krep_gpu_regex_loops_t *out)
{
    krep_gpu_regex_ext_t ext{};
    uint32_t plus[kRegexMaxBranches] = {0};
    bool unbounded = false;
    if (const char *why = regex_compile_ext_branches(p, &ext, true, plus, &unbounded))
        return why == kRegexExtEmpty ? kRegexLoopsEmpty : why;
    if (!unbounded)
        return kRegexLoopsNone;
    for (uint32_t b = 0; b < ext.alt.n_branches; ++b)
        for (uint32_t j = 0; j < ext.alt.branch[b].L; ++j)
            if (regex_class_holds_nl(ext.alt.branch[b].classes[j]))
                return kRegexLoopsNewline;
    out->alt = ext.alt;
    out->bol = ext.bol;
    out->eol = ext.eol;
    for (uint32_t b = 0; b < ext.alt.n_branches; ++b)
        out->repeat[b] = (uint16_t)plus[b];
    regex_loops_filter(out);
    return nullptr;
}
// krep_gpu_regex_compile_loops: NULL and *out filled, or the refusal and *out zeroed
inline const char *regex_compile_loops(const search_params_t *p, krep_gpu_regex_loops_t *out) { return regex_compile_zeroing(p, out, regex_compile_loops_expand); }

// ---- krep_gpu_regex_compile_groups: repeated and nested groups, held unexpanded as a position (Glushkov) automaton -------------------
// The expression is parsed into a small tree (counted quantifiers copy their operand by parsing it again: X{2,} is X X+, X{1,3} is
// X X? X?), the atom occurrences of the tree are the POSITIONS, numbered left to right, and first / last / follow come from the
// usual recursion over the tree.  Nothing is multiplied out, so [0-9]{1,3}\.[0-9]{1,3}\.[0-9]{1,3}\.[0-9]{1,3} is 15 positions.
constexpr uint32_t kRegexGroupsMaxPos = 32, kRegexGroupsMaxDepth = 8, kRegexGroupsMaxJumps = 12;
constexpr const char *kRegexGroupsOlder = "regex groups: an older compiler takes the expression (krep_gpu_regex_compile_anchored, _alt, _ext, _loops): it "
                                          "stays theirs";
constexpr const char *kRegexGroupsNewline = "regex groups: a byte class of the expression holds '\\n', so a match can cross a line end and the lines of the text "
                                            "are no longer independent: kept on krep's regex_search";
constexpr const char *kRegexGroupsNullable = "regex groups: the expression matches the empty string ((ab)*, (a|b*)+, a?(b)*): kept on krep's regex_search";
constexpr const char *kRegexGroupsEmptyAlt = "regex groups: an empty alternative or an empty group (a|, |a, (), (a|), a||b) matches the empty string: kept on "
                                             "krep's regex_search";
constexpr const char *kRegexGroupsQuantQuant = "regex groups: a quantifier behind a quantifier ((ab)+?, a{2}{3}, (a)*+): kept on krep's regex_search";
constexpr const char *kRegexGroupsQuantNothing = "regex groups: a quantifier that is not behind an atom or a group";
constexpr const char *kRegexGroupsZero = "regex groups: {0} and {0,0} repeat their operand zero times: kept on krep's regex_search";
constexpr const char *kRegexGroupsAnchor = "regex groups: ^ that is not the first or $ that is not the last byte of a top-level branch ((^a)+, a(b$), a^b) "
                                           "anchors inside the expression: kept on krep's regex_search";
constexpr const char *kRegexGroupsMixedAnchors = "regex groups: the top-level branches do not all carry the same ^ and $: kept on krep's regex_search";
constexpr const char *kRegexGroupsTooManyPos = "regex groups: more than 32 positions (atom occurrences after {n,m} has copied its operand): kept on krep's "
                                               "regex_search";
constexpr const char *kRegexGroupsTooDeep = "regex groups: parentheses nested deeper than 8: kept on krep's regex_search";
constexpr const char *kRegexGroupsTooManyJumps = "regex groups: the follow relation needs more than 12 jump pairs beside its chain and self edges: kept on krep's "
                                                 "regex_search";
constexpr const char *kRegexGroupsNoFilter = "regex groups: no set of at most 8 fixed-length factors, 32 classes in all, lies on every match: kept on krep's "
                                             "regex_search";

struct RegexGNode
{
    enum Kind : uint8_t { kAtom, kCat, kAlt, kPlus, kStar, kOpt } kind;
    int a, b; // kAtom: a = the position; kCat / kAlt: both children; the quantifiers: a = the operand
};
struct RegexGParser
{
    const uint8_t *pat = nullptr;
    size_t n = 0, i = 0;
    bool case_sensitive = true;
    krep_gpu_regex_groups_t *out = nullptr;
    int bol = -1, eol = -1; // the ^ and $ every top-level branch of the search must carry: -1 before the first branch, then what it had
    std::vector<RegexGNode> nodes;
    int add(RegexGNode::Kind k, int a, int b = -1)
    {
        nodes.push_back(RegexGNode{k, a, b});
        return (int)nodes.size() - 1;
    }
};
inline const char *regex_g_alt(RegexGParser &c, uint32_t depth, int *node);
// an atom or a group at the cursor, without its quantifier
inline const char *regex_g_operand(RegexGParser &c, uint32_t depth, int *node)
{
    const uint8_t ch = c.pat[c.i];
    if (ch == '(')
    {
        if (depth >= kRegexGroupsMaxDepth)
            return kRegexGroupsTooDeep;
        ++c.i;
        if (const char *why = regex_g_alt(c, depth + 1, node))
            return why;
        if (c.i >= c.n || c.pat[c.i] != ')')
            return kRegexAltUnbalanced;
        ++c.i;
        return nullptr;
    }
    if (ch == '^' || ch == '$')
        return kRegexGroupsAnchor;
    size_t len;
    if (const char *why = regex_atom(c.pat, c.n, c.i, &len))
        return why;
    if (c.out->n_pos >= kRegexGroupsMaxPos)
        return kRegexGroupsTooManyPos;
    uint8_t *cls = c.out->classes[c.out->n_pos];
    if (!regex_probe_atom(c.pat + c.i, len, c.case_sensitive, cls))
        return kRegexAtomRefused;
    if (regex_class_holds_nl(cls))
        return kRegexGroupsNewline;
    *node = c.add(RegexGNode::kAtom, (int)c.out->n_pos++);
    c.i += len;
    return nullptr;
}
// item = operand quant?
inline const char *regex_g_item(RegexGParser &c, uint32_t depth, int *node)
{
    const size_t start = c.i;
    if (const char *why = regex_g_operand(c, depth, node))
        return why;
    if (c.i >= c.n || !regex_is_quant(c.pat[c.i]))
        return nullptr;
    RegexQuant q;
    switch (regex_quant(c.pat, c.n, &c.i, true, &q))
    {
    case RegexQuantFault::kZero: return kRegexGroupsZero;
    case RegexQuantFault::kBehindQuant: return kRegexGroupsQuantQuant;
    case RegexQuantFault::kNone: break;
    default: return kRegexMalformed;
    }
    const size_t behind = c.i;
    // X{lo,hi}: lo copies in a row, then hi - lo optional ones; X{lo,}: lo - 1 copies and X+ (lo == 0: X*).  *node is the first copy;
    // every further one is the operand parsed again, which gives it positions of its own (the 33rd position ends a large count)
    const uint32_t plain = q.unbounded ? (q.lo ? q.lo - 1 : 0) : q.lo, opt = q.unbounded ? 0 : q.hi - q.lo;
    int acc = -1, copy = *node;
    bool have = true; // `copy` is a copy that no place of the result uses yet
    auto next_copy = [&]() -> const char * {
        if (have)
        {
            have = false;
            return nullptr;
        }
        c.i = start;
        return regex_g_operand(c, depth, &copy);
    };
    auto put = [&](int nd) { acc = acc < 0 ? nd : c.add(RegexGNode::kCat, acc, nd); };
    for (uint32_t k = 0; k < plain; ++k)
    {
        if (const char *why = next_copy())
            return why;
        put(copy);
    }
    if (q.unbounded)
    {
        if (const char *why = next_copy())
            return why;
        put(c.add(q.lo ? RegexGNode::kPlus : RegexGNode::kStar, copy));
    }
    for (uint32_t k = 0; k < opt; ++k)
    {
        if (const char *why = next_copy())
            return why;
        put(c.add(RegexGNode::kOpt, copy));
    }
    c.i = behind;
    *node = acc;
    return nullptr;
}
// seq = item+, up to a '|', a ')' or the end; top: a '$' in front of one of those ends the branch and is the line anchor
inline const char *regex_g_seq(RegexGParser &c, uint32_t depth, bool top, int *node, int *eol)
{
    int acc = -1;
    while (c.i < c.n && c.pat[c.i] != '|' && c.pat[c.i] != ')')
    {
        if (top && c.pat[c.i] == '$' && (c.i + 1 == c.n || c.pat[c.i + 1] == '|'))
        {
            *eol = 1;
            ++c.i;
            break;
        }
        if (regex_is_quant(c.pat[c.i]))
            return kRegexGroupsQuantNothing;
        int item;
        if (const char *why = regex_g_item(c, depth, &item))
            return why;
        acc = acc < 0 ? item : c.add(RegexGNode::kCat, acc, item);
    }
    if (acc < 0)
        return kRegexGroupsEmptyAlt;
    *node = acc;
    return nullptr;
}
// alt = seq ('|' seq)*.  Depth 0 is the top level of a pattern: it ends with the pattern, not with a ')', every branch may stand
// between ^ and $, and all top-level branches of the search carry the same pair (c.bol / c.eol)
inline const char *regex_g_alt(RegexGParser &c, uint32_t depth, int *node)
{
    const bool top = depth == 0;
    int acc = -1;
    for (;;)
    {
        int bol = 0, eol = 0, seq;
        if (top && c.i < c.n && c.pat[c.i] == '^')
        {
            bol = 1;
            ++c.i;
        }
        if (const char *why = regex_g_seq(c, depth, top, &seq, &eol))
            return why;
        if (top && c.bol < 0)
        {
            c.bol = bol;
            c.eol = eol;
        }
        else if (top && (c.bol != bol || c.eol != eol))
            return kRegexGroupsMixedAnchors;
        acc = acc < 0 ? seq : c.add(RegexGNode::kAlt, acc, seq);
        if (c.i >= c.n || c.pat[c.i] == ')')
        {
            if ((c.i >= c.n) != top) // a ')' nobody opened, or a group the pattern ends in
                return kRegexAltUnbalanced;
            break;
        }
        ++c.i; // the '|'
    }
    *node = acc;
    return nullptr;
}
// nullable / first / last of a node; the follow edges of everything below it go into out->follow
struct RegexGSets { bool nullable; uint32_t first, last; };
inline RegexGSets regex_g_sets(const RegexGParser &c, int nd, krep_gpu_regex_groups_t *out)
{
    const RegexGNode &x = c.nodes[(size_t)nd];
    auto link = [&](uint32_t from, uint32_t to) {
        for (uint32_t i = 0; i < kRegexGroupsMaxPos; ++i)
            if ((from >> i) & 1u)
                out->follow[i] |= to;
    };
    if (x.kind == RegexGNode::kAtom)
        return RegexGSets{false, 1u << x.a, 1u << x.a};
    const RegexGSets A = regex_g_sets(c, x.a, out);
    if (x.kind == RegexGNode::kCat)
    {
        const RegexGSets B = regex_g_sets(c, x.b, out);
        link(A.last, B.first);
        return RegexGSets{A.nullable && B.nullable, A.first | (A.nullable ? B.first : 0u), B.last | (B.nullable ? A.last : 0u)};
    }
    if (x.kind == RegexGNode::kAlt)
    {
        const RegexGSets B = regex_g_sets(c, x.b, out);
        return RegexGSets{A.nullable || B.nullable, A.first | B.first, A.last | B.last};
    }
    if (x.kind != RegexGNode::kOpt)
        link(A.last, A.first);
    return RegexGSets{A.nullable || x.kind != RegexGNode::kPlus, A.first, A.last};
}

// The follow relation as the line walk holds it (kg_regex_loops.hip): follow(S) = ((S & chain) << 1) | (S & self) | the dst of every
// pair whose src meets S.  chain: the positions i whose follow set holds i + 1 (never bit 31: nothing shifts out), self: those that
// hold i; what is left of a follow set is a jump, and positions that share a remainder share a pair.  Returns the number of pairs,
// which may pass `room`: then only the first `room` are written.
inline uint32_t regex_groups_jumps(const krep_gpu_regex_groups_t &g, uint32_t *chain, uint32_t *self, uint32_t *src, uint32_t *dst, uint32_t room)
{
    uint32_t n = 0;
    *chain = *self = 0;
    for (uint32_t i = 0; i < g.n_pos; ++i)
    {
        uint32_t rest = g.follow[i];
        if (i + 1 < kRegexGroupsMaxPos && ((rest >> (i + 1)) & 1u))
        {
            *chain |= 1u << i;
            rest &= ~(1u << (i + 1));
        }
        if ((rest >> i) & 1u)
        {
            *self |= 1u << i;
            rest &= ~(1u << i);
        }
        if (!rest)
            continue;
        uint32_t k = 0;
        while (k < n && k < room && dst[k] != rest)
            ++k;
        if (k < n && k < room)
            src[k] |= 1u << i;
        else
        {
            if (n < room)
            {
                src[n] = 1u << i;
                dst[n] = rest;
            }
            ++n;
        }
    }
    return n;
}

// The filter.  The FACTOR of a position: its class, lengthened along forced edges.  Forward: while no position of the frontier is in
// `last` and everything that can follow the frontier has ONE class, that class is the next byte of every match that passes the
// frontier (a single follow is the plain case; the three digits in front of a '.' of the IP expression are the other).  Backward
// the same with `first` and the predecessors.  A set of positions that every match passes (an atom: itself; a concatenation: the best
// of its children that are not nullable; an alternation: the union; X+: that of X; X?, X*: none) gives a filter: its factors.
struct RegexGFactor { uint32_t L; uint8_t classes[kRegexMaxL][32]; double weight; };
inline void regex_g_factor(const krep_gpu_regex_groups_t &g, uint32_t p, uint32_t cap, RegexGFactor *f)
{
    uint32_t pred[kRegexGroupsMaxPos] = {0};
    for (uint32_t i = 0; i < g.n_pos; ++i)
        for (uint32_t j = 0; j < g.n_pos; ++j)
            if ((g.follow[i] >> j) & 1u)
                pred[j] |= 1u << i;
    // one class for all of `set`: its lowest position, or -1
    auto one_class = [&](uint32_t set) -> int {
        if (!set)
            return -1;
        const int lead = __builtin_ctz(set);
        for (uint32_t i = 0; i < g.n_pos; ++i)
            if (((set >> i) & 1u) && memcmp(g.classes[i], g.classes[lead], 32) != 0)
                return -1;
        return lead;
    };
    auto around = [&](uint32_t set, const uint32_t *rel) {
        uint32_t r = 0;
        for (uint32_t i = 0; i < g.n_pos; ++i)
            if ((set >> i) & 1u)
                r |= rel[i];
        return r;
    };
    int fwd[kRegexMaxL], bwd[kRegexMaxL];
    uint32_t nf = 0, nb = 0;
    for (uint32_t F = 1u << p; 1 + nf < cap && !(F & g.last);)
    {
        F = around(F, g.follow);
        const int cl = one_class(F);
        if (cl < 0)
            break;
        fwd[nf++] = cl;
    }
    for (uint32_t B = 1u << p; 1 + nf + nb < cap && !(B & g.first);)
    {
        B = around(B, pred);
        const int cl = one_class(B);
        if (cl < 0)
            break;
        bwd[nb++] = cl;
    }
    f->L = 0;
    f->weight = 1.0;
    auto put = [&](int pos) {
        memcpy(f->classes[f->L++], g.classes[pos], 32);
        f->weight *= (double)regex_class_size(g.classes[pos]) / 256.0;
    };
    for (uint32_t k = nb; k-- > 0;)
        put(bwd[k]);
    put((int)p);
    for (uint32_t k = 0; k < nf; ++k)
        put(fwd[k]);
}
// a set of positions every match passes, as a filter: ok (at most 8 distinct factors, 32 classes in all), its weight, its shortest factor
struct RegexGReq { bool ok; uint32_t set; double weight; uint32_t shortest; };
inline RegexGReq regex_g_req_of(uint32_t set, const RegexGFactor *fac, krep_gpu_regex_alt_t *filter = nullptr)
{
    krep_gpu_regex_alt_t tmp;
    krep_gpu_regex_alt_t &alt = filter ? *filter : tmp;
    memset(&alt, 0, sizeof alt);
    RegexGReq r{set != 0, set, 0.0, kRegexMaxL};
    uint32_t total = 0;
    for (uint32_t p = 0; p < kRegexGroupsMaxPos && r.ok; ++p)
    {
        if (!((set >> p) & 1u))
            continue;
        krep_gpu_regex_info_t q{};
        q.L = fac[p].L;
        memcpy(q.classes, fac[p].classes, (size_t)q.L * 32);
        const uint32_t before = alt.n_branches;
        r.ok = regex_branch_add(alt.branch, &alt.n_branches, q);
        if (alt.n_branches != before)
        {
            r.weight += fac[p].weight;
            total += q.L;
            r.shortest = q.L < r.shortest ? q.L : r.shortest;
        }
    }
    r.ok = r.ok && total <= kRegexMaxTotalL;
    return r;
}
inline RegexGReq regex_g_req(const RegexGParser &c, int nd, const RegexGFactor *fac)
{
    const RegexGNode &x = c.nodes[(size_t)nd];
    const RegexGReq none{false, 0, 0.0, 0};
    switch (x.kind)
    {
    case RegexGNode::kAtom: return regex_g_req_of(1u << x.a, fac);
    case RegexGNode::kPlus: return regex_g_req(c, x.a, fac);
    case RegexGNode::kStar:
    case RegexGNode::kOpt: return none;
    case RegexGNode::kAlt:
    {
        const RegexGReq A = regex_g_req(c, x.a, fac), B = regex_g_req(c, x.b, fac);
        return A.ok && B.ok ? regex_g_req_of(A.set | B.set, fac) : none;
    }
    default:
    { // a concatenation: the smaller weight; on a tie the one whose shortest factor is longer, then the left one
        const RegexGReq A = regex_g_req(c, x.a, fac), B = regex_g_req(c, x.b, fac);
        if (!A.ok || !B.ok)
            return A.ok ? A : B;
        return (B.weight < A.weight || (B.weight == A.weight && B.shortest > A.shortest)) ? B : A;
    }
    }
}

inline const char *regex_compile_groups_parse(const search_params_t *p, krep_gpu_regex_groups_t *out)
{
    RegexGParser c;
    c.case_sensitive = p->case_sensitive;
    c.out = out;
    int root = -1;
    const char *why = regex_each_pattern(p, [&](const uint8_t *pat, size_t n) -> const char * {
        c.pat = pat;
        c.n = n;
        c.i = 0;
        int nd;
        if (const char *why = regex_g_alt(c, 0, &nd))
            return why;
        root = root < 0 ? nd : c.add(RegexGNode::kAlt, root, nd);
        return nullptr;
    });
    if (why)
        return why;
    const RegexGSets S = regex_g_sets(c, root, out);
    if (S.nullable)
        return kRegexGroupsNullable;
    out->first = S.first;
    out->last = S.last;
    out->bol = c.bol > 0;
    out->eol = c.eol > 0;
    {   // the older compilers keep what is theirs
        krep_gpu_regex_anchored_t a;
        krep_gpu_regex_alt_t b;
        krep_gpu_regex_ext_t e;
        krep_gpu_regex_loops_t l;
        if (!regex_compile_anchored(p, &a) || !regex_compile_alt(p, &b) || !regex_compile_ext(p, &e) || !regex_compile_loops(p, &l))
            return kRegexGroupsOlder;
    }
    uint32_t chain, self, src[kRegexGroupsMaxJumps], dst[kRegexGroupsMaxJumps];
    if (regex_groups_jumps(*out, &chain, &self, src, dst, kRegexGroupsMaxJumps) > kRegexGroupsMaxJumps)
        return kRegexGroupsTooManyJumps;
    // factors of up to 16 classes first; 8 such factors pass the 32 classes of an alternation, so shorter ones are tried behind them
    for (uint32_t cap = kRegexMaxL; cap >= 4; cap /= 2)
    {
        RegexGFactor fac[kRegexGroupsMaxPos];
        for (uint32_t q = 0; q < out->n_pos; ++q)
            regex_g_factor(*out, q, cap, &fac[q]);
        const RegexGReq R = regex_g_req(c, root, fac);
        if (!R.ok)
            continue;
        (void)regex_g_req_of(R.set, fac, &out->filter);
        for (uint32_t b = 0; b < out->filter.n_branches; ++b)
            regex_seq_finish(&out->filter.branch[b], false, false);
        regex_alt_finish(&out->filter, false, false);
        return nullptr;
    }
    return kRegexGroupsNoFilter;
}
// krep_gpu_regex_compile_groups: NULL and *out filled, or the refusal and *out zeroed
inline const char *regex_compile_groups(const search_params_t *p, krep_gpu_regex_groups_t *out) { return regex_compile_zeroing(p, out, regex_compile_groups_parse); }

// ---- the tables the kernels look a text byte up in ---------------------------------------------------------------------------------
// One sequence between its anchors (kg_regex.hip): bit 0 is ^'s newline when bol, bit bol + j class j, bit bol + L $'s newline
inline void rx_seq_table(const krep_gpu_regex_anchored_t &a, uint32_t table[256])
{
    const uint32_t bol = a.bol ? 1u : 0u, eol = a.eol ? 1u : 0u;
    memset(table, 0, 256 * sizeof(uint32_t));
    for (int b = 0; b < 256; ++b)
        for (uint32_t j = 0; j < a.seq.L; ++j)
            table[b] |= ((a.seq.classes[j][b >> 3] >> (b & 7)) & 1u) << (bol + j);
    table['\n'] |= bol | (eol << (bol + a.seq.L));
}
// An alternation (kg_regex_alt.hip; the places of a loops program): branch i in bits [o_i, o_i + Lx_i), Lx_i = L_i + bol + eol places: the
// class { '\n' } in front of and / or behind its classes when the branches stand between line anchors; *init every o_i, *fin every
// o_i + Lx_i - 1
inline void rx_alt_table(const krep_gpu_regex_alt_t &alt, uint32_t bol, uint32_t eol, uint32_t table[256], uint32_t *init, uint32_t *fin)
{
    memset(table, 0, 256 * sizeof(uint32_t));
    *init = *fin = 0;
    uint32_t o = 0;
    for (uint32_t i = 0; i < alt.n_branches; ++i)
    {
        const krep_gpu_regex_info_t &br = alt.branch[i];
        const uint32_t Lx = br.L + bol + eol;
        *init |= 1u << o;
        *fin |= 1u << (o + Lx - 1);
        for (int b = 0; b < 256; ++b)
            for (uint32_t j = 0; j < br.L; ++j)
                table[b] |= ((br.classes[j][b >> 3] >> (b & 7)) & 1u) << (o + bol + j);
        table['\n'] |= (bol << o) | (eol << (o + Lx - 1)); // (bol, eol: 0 or 1)
        o += Lx;
    }
}

// ---- the program of the line walk (kg_regex_loops.hip) ------------------------------------------------------------------------------
// What kg::rx_line_walk runs, whichever compiler took the search.  The state is 32 bits; an attempt starts with init & table[byte],
// a match ends where the state meets fin.  !general: the bits are the PLACES of flat sequences laid out like an alternation's, and a
// step is the shift: a place hands over to the next one, a place of `self` also stays.  general: the bits are the POSITIONS of an
// automaton, and a step is follow(S) = ((S & chain) << 1) | (S & self) | the jump_dst of every pair whose jump_src meets S.  ^ and $
// are the walk's own (no anchor places), and `filter` is the alternation whose occurrences name the candidate lines.
struct RegexWalk
{
    uint32_t table[256];      // bit i of table[b]: byte b is in place / position i
    uint32_t init, fin, self; // first, last, the places or positions that stay
    bool general;
    uint32_t chain, n_jumps, jump_src[kRegexGroupsMaxJumps], jump_dst[kRegexGroupsMaxJumps]; // general only; the unused pairs are 0
    int bol, eol;
    krep_gpu_regex_alt_t filter;
};
// a loops program: the alternation's layout without anchor places, `self` the places that repeat
inline RegexWalk regex_walk_of_loops(const krep_gpu_regex_loops_t &l)
{
    RegexWalk w{};
    rx_alt_table(l.alt, 0, 0, w.table, &w.init, &w.fin);
    uint32_t o = 0;
    for (uint32_t i = 0; i < l.alt.n_branches; ++i)
    {
        w.self |= (uint32_t)l.repeat[i] << o;
        o += l.alt.branch[i].L;
    }
    w.bol = l.bol, w.eol = l.eol;
    w.filter = l.filter;
    return w;
}
// a position automaton: init = first, fin = last, the follow relation as regex_groups_jumps() cuts it
inline RegexWalk regex_walk_of_groups(const krep_gpu_regex_groups_t &g)
{
    RegexWalk w{};
    w.general = true;
    for (int b = 0; b < 256; ++b)
        for (uint32_t i = 0; i < g.n_pos; ++i)
            w.table[b] |= ((g.classes[i][b >> 3] >> (b & 7)) & 1u) << i;
    w.init = g.first;
    w.fin = g.last;
    w.n_jumps = regex_groups_jumps(g, &w.chain, &w.self, w.jump_src, w.jump_dst, kRegexGroupsMaxJumps);
    w.bol = g.bol, w.eol = g.eol;
    w.filter = g.filter;
    return w;
}
// The shift of a loops program written as a follow relation (the test hook krep_gpu_debug_force_regex_general): every place but a
// branch's last hands over along chain, a repeating place is in self already, no jump pairs.  (The last branch's last place is the
// highest bit of fin.)
inline RegexWalk regex_walk_as_general(RegexWalk w)
{
    const uint32_t places = 32u - (uint32_t)__builtin_clz(w.fin);
    w.general = true;
    w.chain = (places >= 32u ? ~0u : (1u << places) - 1u) & ~w.fin;
    return w;
}

// ---- the compilers in the order every search asks them -------------------------------------------------------------------------
// The anchored compiler is asked first (kSeq); only what it refuses goes to the alternation compiler, and what both refuse to the
// expanding compiler, whose result is an alternation too, between the line anchors alt_bol / alt_eol (kAlt: one of the two took it).
// So a search an earlier compiler takes runs the kernel it always ran.  What all three refuse goes to the loops compiler when the
// caller says so (krep_gpu_set_regex_loops), and what is still refused to the groups compiler when the caller says so
// (krep_gpu_set_regex_groups): kWalk either way, the line walk's program.
struct RegexCompiled
{
    enum Kind : uint8_t { kSeq, kAlt, kWalk } kind = kSeq;
    krep_gpu_regex_anchored_t seq{}; // kSeq
    krep_gpu_regex_alt_t alt{};      // kAlt
    int alt_bol = 0, alt_eol = 0;    // kAlt: ^ in front of / $ behind every branch (the expanding compiler only)
    RegexWalk walk{};                // kWalk
    // what the code around the scans asks
    bool line_walked() const { return kind == kWalk; }
    bool has_eol() const { return (kind == kWalk ? walk.eol : kind == kAlt ? alt_eol : seq.eol) != 0; }
    // two occurrences can share a byte (never asked of a line walk, whose matches are chosen line by line)
    bool overlaps() const { return (kind == kAlt ? alt.cross_overlap : seq.seq.self_overlap) != 0; }
    // a byte class holds '\n' (the loops and the groups compiler refuse such an expression)
    bool holds_newline() const
    {
        const krep_gpu_regex_info_t *br = kind == kAlt ? alt.branch : &seq.seq;
        bool nl = false;
        for (uint32_t b = 0; kind != kWalk && b < (kind == kAlt ? alt.n_branches : 1u); ++b)
            for (uint32_t j = 0; j < br[b].L; ++j)
                nl = nl || regex_class_holds_nl(br[b].classes[j]);
        return nl;
    }
};
// a refusal of the two older compilers that is a limit of theirs: one the expanding compiler's own limits do not replace
inline bool regex_older_limit(const char *why)
{
    return why == kRegexSeqTooManyClasses || why == kRegexSeqTooManyPlaces || why == kRegexAltBranchTooLong || why == kRegexAltTooManyBranches ||
           why == kRegexAltTooWide;
}
// a refusal that says a group, nesting or what an expansion multiplies out to: the groups compiler's own reason replaces it
inline bool regex_group_reason(const char *why)
{
    return why == kRegexLoopsGroup || why == kRegexAltNested || why == kRegexAltGroupNotBranch || why == kRegexAltGroupHoldsAlt ||
           why == kRegexExtTooMany || why == kRegexExtTooLong || why == kRegexExtTooWide;
}
// NULL: taken.  Else the reason of a search all three refuse: what it was before the expanding compiler — the alternation compiler's
// when the search says an alternation, else the anchored compiler's — unless only the expanding compiler's own limits are in the way.
// loops: the loops compiler is asked fourth.  Its own reason replaces the earlier one only where that one says "without a bound".
// groups: the groups compiler is asked fifth.  Its own reason replaces the earlier one only where that one is a group reason.
inline const char *regex_compile_search_older(const search_params_t *p, RegexCompiled *out, bool loops)
{
    const char *why = regex_compile_anchored(p, &out->seq);
    if (!why)
        return nullptr;
    if (!p || !p->use_regex)
        return why;
    const char *why_alt = regex_compile_alt(p, &out->alt);
    if (!why_alt)
    {
        out->kind = RegexCompiled::kAlt;
        return nullptr;
    }
    krep_gpu_regex_ext_t ext;
    const char *why_ext = regex_compile_ext(p, &ext);
    if (!why_ext)
    {
        out->kind = RegexCompiled::kAlt;
        out->alt = ext.alt;
        out->alt_bol = ext.bol;
        out->alt_eol = ext.eol;
        return nullptr;
    }
    const char *before = regex_has_alt_syntax(p) ? why_alt : why;
    const char *today = regex_ext_own_limit(why_ext) && !regex_older_limit(before) ? why_ext : before;
    if (!loops)
        return today;
    krep_gpu_regex_loops_t l;
    const char *why_loops = regex_compile_loops(p, &l);
    if (!why_loops)
    {
        out->kind = RegexCompiled::kWalk;
        out->walk = regex_walk_of_loops(l);
        return nullptr;
    }
    return today == kRegexStarPlus || today == kRegexOpenCount ? why_loops : today;
}
inline const char *regex_compile_search(const search_params_t *p, RegexCompiled *out, bool loops = false, bool groups = false)
{
    out->kind = RegexCompiled::kSeq;
    out->alt_bol = out->alt_eol = 0;
    const char *today = regex_compile_search_older(p, out, loops);
    if (!today || !groups || !p || !p->use_regex)
        return today;
    krep_gpu_regex_groups_t g;
    const char *why_groups = regex_compile_groups(p, &g);
    if (!why_groups)
    {
        out->kind = RegexCompiled::kWalk;
        out->walk = regex_walk_of_groups(g);
        return nullptr;
    }
    return regex_group_reason(today) ? why_groups : today;
}

} // namespace kg
