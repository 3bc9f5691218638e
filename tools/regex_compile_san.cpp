// tools/regex_compile_san.cpp — the -E pattern compiler (krep_amd/csrc/kg_regex_compile.h: host code, no HIP) as a stand-alone
// program for AddressSanitizer / UBSan:  python tools/sanitize.py regex   (or by hand:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer tools/regex_compile_san.cpp -o regex_compile_san).
// It feeds the four entry points' compilers (the alternation compiler with one and with two patterns) accepted patterns, every refusal, and 200 000 pattern strings drawn from the bytes the
// grammar cares about (^ $ | ( ) among them), each copied into a heap block of exactly its length so that a read past the pattern is a report.
//
//   regex_compile_san --digest [--blocks N]
// instead walks a fixed corpus (every table below and the random generators), asks the compilers and regex_compile_search about
// every entry and prints 64-bit FNV-1a digests of their answers, one per 1000 entries: tests/golden/regex_compile_digest.json holds
// what the compilers said before their rules were folded into one copy each (tests/test_regex_compile_digest_cpu.py).  The rows:
//   classes, named, bytes, pieces: the four older compilers and regex_compile_search with both switches off;
//   loops.*, groups.*: krep_gpu_regex_compile_loops' and _groups' compilers (every byte of a taken struct, the reason of a refusal);
//   search10.*, search01.*, search11.*: regex_compile_search with the loops switch, the groups switch and both on (who took it, ^, $,
//     the reason), read through verdict_of(), the one place here that knows how RegexCompiled is laid out;
//   walk.*: for every entry the loops or the groups compiler takes, the program the line walk kernel receives (kg::RegexWalk), and for
//     a loops program also what krep_gpu_debug_force_regex_general makes of it;
// each over .named (the tables), .bytes, .pieces and .quants (the three generators).  --digest exits non-zero when the corpus does not
// reach every refusal of the loops and the groups compiler, 1000 taken entries of each, a walk program of more than 8 jump pairs and
// one of none.  The recording is reproduced from commit e0710b6, the last one whose line walk program had no type of its own (its
// kg_regex.hip assembled the fields in regex_prog_create; KG_REGEX_PARENT holds that code), with
//   git show e0710b6:krep_amd/csrc/kg_regex_compile.h > krep_amd/csrc/kg_regex_compile_parent.h
//   g++ -std=c++17 -O2 -DKG_REGEX_PARENT -DKG_REGEX_HEADER='"../krep_amd/csrc/kg_regex_compile_parent.h"' tools/regex_compile_san.cpp -o digest_parent
//   ./digest_parent --digest
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#ifndef KG_REGEX_HEADER
#define KG_REGEX_HEADER "../krep_amd/csrc/kg_regex_compile.h"
#endif
#include KG_REGEX_HEADER

// what regex_compile_search said about a taken search: who took it (0 the anchored compiler, 1 the alternation or the expanding one,
// 2 the loops compiler, 3 the groups compiler), the line anchors, and the struct of the two older kinds
struct Verdict
{
    int took, bol, eol;
    const krep_gpu_regex_anchored_t *seq;
    const krep_gpu_regex_alt_t *alt;
};
#ifdef KG_REGEX_PARENT // that commit: RegexCompiled is four flags beside every compiler's struct, and the walk program is RegexProg's fields
static Verdict verdict_of(const kg::RegexCompiled &rc)
{
    if (rc.is_loops)
        return Verdict{rc.is_groups ? 3 : 2, rc.loops.bol, rc.loops.eol, nullptr, nullptr};
    if (rc.is_alt)
        return Verdict{1, rc.alt_bol, rc.alt_eol, nullptr, &rc.alt};
    return Verdict{0, rc.seq.bol, rc.seq.eol, &rc.seq, nullptr};
}
struct Walk
{
    uint32_t table[256];
    uint32_t init, fin, self;
    bool general;
    uint32_t chain, n_jumps, jump_src[12], jump_dst[12];
    int bol, eol;
    krep_gpu_regex_alt_t filter;
};
static Walk walk_of_loops(const krep_gpu_regex_loops_t &l)
{
    Walk w;
    memset(&w, 0, sizeof w);
    uint32_t o = 0;
    for (uint32_t i = 0; i < l.alt.n_branches; ++i)
    {
        const krep_gpu_regex_info_t &br = l.alt.branch[i];
        w.init |= 1u << o;
        w.fin |= 1u << (o + br.L - 1);
        for (int b = 0; b < 256; ++b)
            for (uint32_t j = 0; j < br.L; ++j)
                w.table[b] |= ((br.classes[j][b >> 3] >> (b & 7)) & 1u) << (o + j);
        w.self |= (uint32_t)l.repeat[i] << o;
        o += br.L;
    }
    w.bol = l.bol;
    w.eol = l.eol;
    w.filter = l.filter;
    return w;
}
static Walk walk_forced_general(const krep_gpu_regex_loops_t &l)
{
    Walk w = walk_of_loops(l);
    const uint32_t o = l.alt.total_L;
    w.general = true;
    w.chain = (o >= 32u ? ~0u : (1u << o) - 1u) & ~w.fin;
    return w;
}
static Walk walk_of_groups(const krep_gpu_regex_groups_t &g)
{
    Walk w;
    memset(&w, 0, sizeof w);
    w.general = true;
    for (int b = 0; b < 256; ++b)
        for (uint32_t i = 0; i < g.n_pos; ++i)
            w.table[b] |= ((g.classes[i][b >> 3] >> (b & 7)) & 1u) << i;
    w.init = g.first;
    w.fin = g.last;
    w.n_jumps = kg::regex_groups_jumps(g, &w.chain, &w.self, w.jump_src, w.jump_dst, kg::kRegexGroupsMaxJumps);
    w.bol = g.bol;
    w.eol = g.eol;
    w.filter = g.filter;
    return w;
}
#else
static Verdict verdict_of(const kg::RegexCompiled &rc)
{
    if (rc.kind == kg::RegexCompiled::kWalk)
        return Verdict{rc.walk.general ? 3 : 2, rc.walk.bol, rc.walk.eol, nullptr, nullptr};
    if (rc.kind == kg::RegexCompiled::kAlt)
        return Verdict{1, rc.alt_bol, rc.alt_eol, nullptr, &rc.alt};
    return Verdict{0, rc.seq.bol, rc.seq.eol, &rc.seq, nullptr};
}
typedef kg::RegexWalk Walk;
static Walk walk_of_loops(const krep_gpu_regex_loops_t &l) { return kg::regex_walk_of_loops(l); }
static Walk walk_of_groups(const krep_gpu_regex_groups_t &g) { return kg::regex_walk_of_groups(g); }
static Walk walk_forced_general(const krep_gpu_regex_loops_t &l) { return kg::regex_walk_as_general(kg::regex_walk_of_loops(l)); }
#endif

// a search over `pats`, each in a heap block of exactly its length: no terminator to lean on
struct Search
{
    std::vector<char *> heap;
    std::vector<const char *> ptrs;
    std::vector<size_t> lens;
    search_params_t p;
    Search(const std::vector<std::string> &pats, bool cs, bool ww)
    {
        for (const std::string &s : pats)
        {
            heap.push_back((char *)malloc(s.size() ? s.size() : 1));
            memcpy(heap.back(), s.data(), s.size());
            ptrs.push_back(heap.back());
            lens.push_back(s.size());
        }
        memset(&p, 0, sizeof p);
        p.pattern = ptrs[0];
        p.pattern_len = lens[0];
        p.patterns = ptrs.data();
        p.pattern_lens = lens.data();
        p.num_patterns = pats.size();
        p.case_sensitive = cs;
        p.use_regex = true;
        p.whole_word = ww;
        p.max_count = SIZE_MAX;
    }
    ~Search()
    {
        for (char *h : heap)
            free(h);
    }
    Search(const Search &) = delete;
    Search &operator=(const Search &) = delete;
};

static int compile(const std::string &pat, bool cs, bool ww, krep_gpu_regex_info_t *info, const char **why,
                   krep_gpu_regex_anchored_t *anchored = nullptr) // anchored: krep_gpu_regex_compile_anchored's compiler instead
{
    Search s({pat}, cs, ww);
    *why = anchored ? kg::regex_compile_anchored(&s.p, anchored) : kg::regex_compile(&s.p, info);
    return *why ? 2 : 0;
}
// krep_gpu_regex_compile_alt's compiler over one or several patterns
static int compile_alt(const std::vector<std::string> &pats, bool cs, bool ww, krep_gpu_regex_alt_t *alt, const char **why)
{
    Search s(pats, cs, ww);
    *why = kg::regex_compile_alt(&s.p, alt);
    (void)kg::regex_has_alt_syntax(&s.p);
    return *why ? 2 : 0;
}
// krep_gpu_regex_compile_ext's compiler over one or several patterns
static int compile_ext(const std::vector<std::string> &pats, bool cs, bool ww, krep_gpu_regex_ext_t *ext, const char **why)
{
    Search s(pats, cs, ww);
    *why = kg::regex_compile_ext(&s.p, ext);
    return *why ? 2 : 0;
}
static bool alt_consistent(const krep_gpu_regex_alt_t &a)
{
    if (a.n_branches < 1 || a.n_branches > 8 || a.Lmin < 1 || a.Lmin > a.Lmax || a.Lmax > 16 || a.total_L > 32 || a.reserved)
        return false;
    unsigned tot = 0;
    for (unsigned i = 0; i < a.n_branches; ++i)
    {
        const unsigned L = a.branch[i].L;
        if (L < a.Lmin || L > a.Lmax || a.branch[i].anchor >= L || a.branch[i].n_anchor > 4)
            return false;
        if (a.branch[i].self_overlap && !a.cross_overlap)
            return false;
        tot += L;
    }
    return tot == a.total_L;
}

// ---- the pattern tables: what the default run asserts about, and the named part of the digest corpus
static const char *ok[] = {"Sherl[oO]ck", "[0-9]{3}-[0-9]{4}", "ERROR [0-9]{3}", "0x[0-9a-f]{8}", ".", "[^a]", "[]a]", "[^]a]", "[a-]",
                           "[[:alpha:]]", "[[:space:]]", "[[:punct:]]", "\\.", "x{3}", "a{16}", "[[.-.]a]", "[[=a=]]b", "a\\{2\\}"};
static const char *no[] = {"a.*b", "(ab)", "a+", "a?", "a|b", "^a", "a$", "a{2,}", "a{2,3}", "{2}a", "a{2}{3}", "\\bword", "\\w", "\\1",
                           "caf\xe9", "a{17}", "a{16}b", "", "[ab", "a{0}", "a\\", "a{", "a{2", "a{x}", "[[:alpha:", "[[.a", "[a[=", "a{99999999999}"};
// the anchored entry point: accepted shapes with their anchors and L, every new refusal, and what the old one still refuses
static const struct { const char *pat; int bol, eol; unsigned L; int overlap; } aok[] = {
    {"^a", 1, 0, 1, 0}, {"a$", 0, 1, 1, 0}, {"^a$", 1, 1, 1, 0}, {"^Sherl[oO]ck", 1, 0, 8, 0}, {"[0-9]{3}$", 0, 1, 3, 0},
    {"^[[:space:]]", 1, 0, 1, 0}, {"\\^a", 0, 0, 2, 0}, {"a\\$", 0, 0, 2, 0}, {"[$^]", 0, 0, 1, 0}, {"^a{15}", 1, 0, 15, 0},
    {"^a{14}$", 1, 1, 14, 0}, {"^ab", 1, 0, 2, 0}, {"ab$", 0, 1, 2, 0}, {"^[a\n]{2}", 1, 0, 2, 1}, {"^[ab]{2}", 1, 0, 2, 0},
    {"[a\n]{2}$", 0, 1, 2, 1}, {"\\$$", 0, 1, 1, 0}, {"[\\]$", 0, 1, 1, 0}, {"^[^a]", 1, 0, 1, 0}, {"Sherl[oO]ck", 0, 0, 8, 0}};
static const char *ano[] = {"^a{16}", "^a{15}$", "a^b", "a$b", "^^a", "a$$", "^$", "^", "$", "^{2}a", "^a|b", "^(a)", "^a.*b", "a+$", "^a{2,3}",
                            "^\\bword", "^[ab", "^a\\", "", "^a{", "^[[:alpha:", "$a", "a{2}^", "^a{0}"};
// the alternation compiler: accepted shapes with their fields, every refusal, several patterns
static const struct { std::vector<std::string> pats; unsigned nb, Lmin, Lmax, total; int overlap; } alt_ok[] = {
    {{"cat|d[oi]g|b.rd"}, 3, 3, 4, 10, 1}, {{"(ERROR)|(WARN[0-9])"}, 2, 5, 5, 10, 0}, {{"ERROR", "WARN[0-9]"}, 2, 5, 5, 10, 0},
    {{"(a)|(b)|(a)"}, 2, 1, 1, 2, 0}, {{"a{16}|b{16}"}, 2, 16, 16, 32, 1}, {{"ab|abc"}, 2, 2, 3, 5, 1}, {{"ab|cd"}, 2, 2, 2, 4, 0},
    {{"a|aa"}, 2, 1, 2, 3, 1}, {{"(Sherl[oO]ck)"}, 1, 8, 8, 8, 0}, {{"a[|]b|c\\|d|[(]x[)]"}, 3, 3, 3, 9, 0}, {{"x|[a-c]{16}"}, 2, 1, 16, 17, 1},
    {{"a|b|c|d|e|f|g|h|a"}, 8, 1, 1, 8, 0}, {{"ERROR|FATAL", "(WARN[0-9])"}, 3, 5, 5, 15, 0}};
static const char *alt_no[] = {"a|", "|a", "()", "a||b", "a|()", "((a))", "(a(b))", "(a", "a)", "a|(b", "x(a|b)y", "(ab)c", "(ab){2}", "(a)(b)", "(a|b)",
                               "^a|b", "a|b$", "(^a)|b", "a|^|b", "a|b|c|d|e|f|g|h|i", "a{17}|b", "a{16}|b{16}|c", "a|b.*", "a+|b", "a|b?", "a{2,3}|b",
                               "a|\\bw", "a|caf\xe9", "a|[bc", "a|b\\", "a|b{0}", "a|{2}", "", "|", "(", ")", "a|[", "a|(", "a|\\", "(a)|", "[(]|("};
// the expanding compiler: accepted shapes with their fields, every refusal
static const struct { std::vector<std::string> pats; int bol, eol; unsigned nb, Lmin, Lmax, total; int overlap; } ext_ok[] = {
    {{"colou?r"}, 0, 0, 2, 5, 6, 11, 0}, {{"https?://"}, 0, 0, 2, 7, 8, 15, 0}, {{"[0-9]{1,3}%"}, 0, 0, 3, 2, 4, 9, 1},
    {{"x(a|bc)y"}, 0, 0, 2, 3, 4, 7, 0}, {{"(ab){2}"}, 0, 0, 1, 4, 4, 4, 1}, {{"(ab){2}|b{0,2}a"}, 0, 0, 4, 1, 4, 10, 1},
    {{"^(ERROR|WARN|FATAL)"}, 1, 0, 3, 4, 5, 14, 0}, {{"\\.(jpg|png)$"}, 0, 1, 2, 4, 4, 8, 0}, {{"^GET", "^POST[0-9]"}, 1, 0, 2, 3, 5, 8, 0},
    {{"^(a{14}|b{14})$"}, 1, 1, 2, 14, 14, 28, 0}, {{"(x|[a-c]{15})$"}, 0, 1, 2, 1, 15, 16, 0}, {{"^[ab]{1,3}$"}, 1, 1, 3, 1, 3, 6, 1},
    {{"^(a|bc)d?$"}, 1, 1, 4, 1, 3, 8, 1}, {{"(a|b|c|d)(e|f)|ae"}, 0, 0, 8, 2, 2, 16, 0}, {{"ab|cd"}, 0, 0, 2, 2, 2, 4, 0}, {{"^ab$"}, 1, 1, 1, 2, 2, 2, 0}};
static const char *ext_no[] = {"ab*", "a+b", "a{2,}", "(a|b)*c", "a?{2}", "a{2}{3}", "a?\?", "a?", "(a|b)?", "a{0}", "a{0,1}", "^$", "^", "$", "x(a|)y", "x()y", "a|",
                               "|a", "a||b", "x((a))", "(a(b|c))d", "x(a", "a)b", "(a|b", "x(^a|b)", "(a|b$)x", "(^a)|(^b)", "a^b", "a$b", "^^a", "a$$", "^a|b",
                               "a|b$", "[ab]{1,9}", "(a|b)(c|d)(e|f)(g|h)", "a{17}", "^a{16}", "^a{15}$", "a{9}(b|c)a{8}", "a{16}|b{16}|c", "^(a{15}|b{15}|c)",
                               "caf\xe9?", "a\\b?", "[ab?", "ab?\\", "{2}a", "a|?b", "(?a)", "^{2}a", "a{2", "a{x}", "a{3,2}", "", "(", ")", "a{1,", "a{1,2", "a{,2}",
                               "a{99999999999,3}", "a{1,99999999999}", "(a{1,1000}){1,1000}", "(a?){1,1000}", "((", "a(", "a(|", "a(b|", "a(b\\"};
// the digest corpus alone: the patterns of REFUSALS, OLD_AND_NEW and of the search every compiler refuses in tests/test_regex_ext_compile_cpu.py
static const std::vector<std::string> py_cases[] = {
    {"ab*"}, {"a+b"}, {"a{2,}"}, {"(a|b)*c"}, {"a?{2}"}, {"a{2}{3}"}, {"a?\?"}, {"(a|b)?{2}"}, {"a?"}, {"(a|b)?"}, {"a?b?"}, {"a{0,1}"}, {"x|a?"}, {"^a?$"},
    {"a{0}"}, {"xa{0,0}"}, {"^$"}, {"^"}, {"$"}, {"x(a|)y"}, {"x()y"}, {"(|a)b"}, {"a|"}, {"|a"}, {"a||b"}, {"x((a))"}, {"(a(b|c))d"}, {"x(a"}, {"a)b"}, {"(a|b"},
    {"x(^a|b)"}, {"(a|b$)x"}, {"(^a)|(^b)"}, {"a^b"}, {"a$b"}, {"^^a"}, {"a$$"}, {"^a|b"}, {"a|b$"}, {"^a|b$"}, {"[ab]{1,9}"}, {"(a|b)(c|d)(e|f)(g|h)"},
    {"a?b?c?d?e"}, {"a{17}"}, {"^a{16}"}, {"^a{15}$"}, {"a{9}(b|c)a{8}"}, {"a{16}|b{16}|c"}, {"^(a{15}|b{15}|c)"}, {"^(a{14}|b{14}|c)$"}, {"caf\xe9?"}, {"a\\b?"},
    {"[ab?"}, {"ab?\\"}, {"{2}a"}, {"a|?b"}, {"(?a)"}, {"^{2}a"}, {"a{2"}, {"a{x}"}, {"a{3,2}"},
    {"Sherl[oO]ck"}, {"^ab"}, {"ab$"}, {"a{3}"}, {"ab|cd"}, {"(ab)|(cd)"}, {"ab", "cd"}, {"a.*b"}, {"a|b.*"}, {"colou?r"}, {"x(a|bc)y"}, {"^(ERROR|WARN)"},
    {"(foo|quux)$"}, {"^GET", "^POST"}, {"[ab]{1,3}c"}, {"(ab){2}"}, {"a?"}, {"^a|b"}, {"a", "^b"}, {"a{2,}"}, {"(a|b)"}, {"a||b"},
    {"a(b|c)*"}, {"ab*"}, {"a", "^b"}, {"^a|b"}, {"a^b"}, {"a{2,}"}, {"a||b"}, {"a{17}"}, {"a|b|c|d|e|f|g|h|i"}, {"a?"}, {"[ab]{1,9}"}, {"a{9}(b|c)a{8}"},
    {"^(a{15}|b{15}|c)"},
    // and what the default run asks beside its tables
    {"a", ""}, {"a", "b*"}, {std::string(1100, 'a') + "|b"}, {"a?b", ""}, {std::string(1100, 'a') + "?b"}};
// the rows of the loops and the groups compiler alone (loops.*, groups.*, search??.*, walk.*): ACCEPTED and REFUSALS of
// tests/test_regex_loops_compile_cpu.py with what its other tests name ...
static const std::vector<std::string> loops_cases[] = {
    {"ERROR.*timeout"}, {"a+b"}, {"[0-9]+"}, {"ab+c"}, {"ab+cd"}, {"a{2,}b"}, {"a{1,}b"}, {"a{3,}"}, {"a*b"}, {"a{0,}b"}, {"colou*r"}, {"^#+ "}, {"b+$"},
    {"^a+$"}, {"x(a+|b)y"}, {"[a-z]+@[a-z]+\\.com"}, {"[0-9]+\\.[0-9]+"}, {"a+", "b+c"}, {"a+b|ab"}, {"(a+b){2}"}, {"[ab]+c?"}, {"^(GET|POST) .+"},
    {"(ab)+"}, {"(a|b)*c"}, {"x(ab){2,}"}, {"(a+)+"}, {"[[:space:]]+x"}, {"a\n+"}, {"a+[b\n]"}, {"a+[[:cntrl:]]"}, {"a*"}, {"a*b*"}, {"x|a*"}, {"^a*$"},
    {"(a|b*)"}, {"colou?r"}, {"ab"}, {"^(ERROR|WARN)"}, {"a{2,3}"}, {"a+*"}, {"a*?"}, {"a+{2}"}, {"a{2,}?"}, {"x((a+))"}, {"x(a+"}, {"a+)b"}, {"(a+|)b"},
    {"a+|"}, {"x(^a+|b)"}, {"a+^b"}, {"^a+|b"}, {"+a"}, {"a|*b"}, {"^+a"}, {"^*"}, {"a{17,}"}, {"^a{16,}"}, {"a{9}b+a{7}"}, {"[ab]{1,9}c+"}, {"a*b*c*d*e"},
    {"a{16}|b{16,}|c"}, {"a{2,"}, {"a{,2}"}, {"a{1001,}"}, {"caf\xe9+"}, {"a\\b+"}, {"[ab+"}, {"ab+\\"}, {"a+", "^b"}, {"a.*b"}, {"a(b|c)+"}};
// ... the named expressions, REFUSALS and the limits of tests/test_regex_groups_compile_cpu.py ...
static const std::string kAz = "abcdefghijklmnopqrstuvwxyz", kIp = "[0-9]{1,3}\\.[0-9]{1,3}\\.[0-9]{1,3}\\.[0-9]{1,3}";
static const std::vector<std::string> groups_cases[] = {
    {"(ab)+"}, {"(a|b)*c"}, {"(a|bc)+d"}, {"((ab)+c)+d"}, {"(a|ab)(c|bcd)"}, {"(a|ab|abc)+c"}, {"x(ab|a)*bc"}, {"(a+|b)+c"}, {"((a|b)c|d)+e"}, {"(ab){2,}"},
    {"(foo|bar){2,3};"}, {"([a-z]+\\.)+com"}, {"^(ab)+"}, {"(ab)+$"}, {"^((GET|POST) |HEAD )/api"}, {"(a|b)(c|d)(e|f)(g|h)"}, {kIp}, {"(ab)+", "c(d|e)*f"},
    {"(ab)+[[:space:]]"}, {"(a\n)+"}, {"(ab)*"}, {"(a|b*)+"}, {"(ab)+|c*"}, {"(ab|)+"}, {"()+a"}, {"(ab)+|"}, {"(ab)+?"}, {"(ab){2}{3}"}, {"(+ab)+"}, {"*(ab)+"},
    {"(ab){0}c"}, {"(ab)+c{0,0}"}, {"(^ab)+"}, {"(ab$)+"}, {"(ab)+^c"}, {"(ab)+$c"}, {"^(ab)+|c"}, {"(ab)+$|(cd)+"}, {"(abcdefghijkabcdefghijkabcdefghijk)+"},
    {"(ab){17}"}, {"(ab){1000,}"}, {"(((((((((a)))))))))+"}, {"(a|b)(c|d)(e|f)(g|h)(i|j)(k|l)(m|n)(o|p)"}, {"(ab)+(c"}, {"(ab)+)"}, {"((ab)+"}, {"(ab){2,"},
    {"(ab){,2}"}, {"(ab){3,2}"}, {"(caf\xe9)+"}, {"(a\\b)+"}, {"([ab)+"}, {"(ab)+\\"}, {"(ab)+", "^(cd)+"}, {"^ab[0-9]$"}, {"ab|cd"}, {"ab", "cd"}, {"colou?r"},
    {"a+b"}, {"x(a+|b)y"}, {"ERROR.*timeout"}, {"(" + kAz + kAz.substr(0, 6) + ")+"}, {"(" + kAz + kAz.substr(0, 7) + ")+"},
    {kAz.substr(0, 12) + "(" + kAz.substr(0, 20) + ")+"}, {"((((((((ab))))))))+"}, {"(((((((((ab)))))))))+"}, {"(a|b)(c|d)(e|f)(g|h)(i|j)(k|l)(m|n)"},
    {"(ab){1,2}(c)+"}, {"(a|b|c|d|e|f|g|h|i)(xy)*"}, {"(a|b|c|d|e|f|g|h)(xy)*"}, {"((ab)+c)+d"}, {"a*"}, {"a.*b"}};
// ... and the quantifier traps: the expanding compiler says "without a bound" before it judges a range, the groups compiler has no such stage
static const char *quant_traps[] = {"a*{2}", "a{2000,}", "a{2,}{3}", "a{,}", "a{2,", "a{0}", "a{0,0}", "a{0,}", "a{3,2}", "a{1001}", "(ab){2000,}", "(ab)+?", "^*a"};


// ---- the two random corpora: pattern strings over the bytes the grammar looks at, and strings of the expanding compiler's grammar
struct Rng
{
    unsigned long long s = 88172645463325252ull;
    unsigned long long next() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; }
};
// one string, and the same string cut in two at a drawn place every other time; the case mode is (s >> 40) & 1 behind the draw
static void draw_bytes(Rng &r, std::string &pat, std::vector<std::string> &pats)
{
    static const char alphabet[] = "ab[]^-:.={},\\0129(|*\n x$";
    pat.clear();
    const int len = (int)(r.next() % 12);
    for (int k = 0; k < len; ++k)
        pat.push_back(alphabet[r.next() % (sizeof alphabet - 1)]);
    pats = {pat};
    if ((r.s >> 33) & 1)
    {
        const size_t cut = pat.empty() ? 0 : (size_t)((r.s >> 20) % (pat.size() + 1));
        pats = {pat.substr(0, cut), pat.substr(cut)};
    }
}
static void draw_pieces(Rng &r, std::vector<std::string> &pats)
{
    static const char *pieces[] = {"a", "b", "[ab]", "[^a]", ".", "\\.", "\n", "?", "{2}", "{1,2}", "{0,3}", "{2,}", "(", ")", "|", "^", "$", "*", "+", "{", "}", ",", "1", "[", "]", "\\"};
    pats.assign(1, std::string());
    const int len = (int)(r.next() % 10);
    for (int k = 0; k < len; ++k)
    {
        const unsigned q = (unsigned)(r.next() % 40);
        pats.back() += pieces[q < 14 ? q % 7 : (q - 14) % (sizeof pieces / sizeof *pieces)]; // (atoms more often than the rest)
        if ((r.s >> 50) % 23 == 0)
            pats.emplace_back(); // several patterns every now and then
    }
}
constexpr int kDraws = 200000;
// the third random corpus (new rows only): expressions around the quantifiers and the groups, of the bytes * + { } , ( ) | most of all
static void draw_quants(Rng &r, std::vector<std::string> &pats)
{
    static const char *atoms[] = {"a", "b", "c", "[ab]", ".", "\\.", "[0-9]"};
    static const char *quants[] = {"", "", "", "*", "+", "?", "{2}", "{2,}", "{1,3}", "{0,}", "{0}", "{,2}", "{3,2}", "{1001}", "{2", "+?", "*{2}", "{2,}{3}"};
    static const char *noise[] = {"(", ")", "|", "^", "$", "{", "}", ",", "*", "+", "\n", "()"};
    const auto pick = [&](const char *const *v, size_t n) { return std::string(v[r.next() % n]); };
    pats.assign(1, std::string());
    const int items = 1 + (int)(r.next() % 5);
    for (int k = 0; k < items; ++k)
    {
        std::string &s = pats.back();
        const unsigned what = (unsigned)(r.next() % 16);
        if (what < 7)
            s += pick(atoms, 7) + pick(quants, 18);
        else if (what < 13)
        { // a group of one to three alternatives of one to three atoms, one level of nesting now and then
            std::string g;
            const int alts = 1 + (int)(r.next() % 3);
            for (int a = 0; a < alts; ++a)
            {
                g += a ? "|" : "";
                const int len = 1 + (int)(r.next() % 3);
                for (int t = 0; t < len; ++t)
                    g += r.next() % 7 == 0 ? "(" + pick(atoms, 7) + pick(atoms, 7) + ")" + pick(quants, 18) : pick(atoms, 7) + pick(quants, 8);
            }
            s += "(" + g + ")" + pick(quants, 18);
        }
        else if (what < 14)
            s += pick(noise, 12);
        else if (what < 15)
            s += k ? "|" : "^";
        else
            pats.emplace_back(); // several patterns every now and then
    }
    if (pats.back().empty() && pats.size() > 1)
        pats.pop_back();
}
constexpr int kQuantDraws = 50000;

// ---- --digest
struct Fnv
{
    uint64_t h = 1469598103934665603ull;
    void bytes(const void *v, size_t n)
    {
        for (size_t i = 0; i < n; ++i)
            h = (h ^ ((const uint8_t *)v)[i]) * 1099511628211ull;
    }
    void byte(uint8_t b) { bytes(&b, 1); }
    // one compiler's answer: which compiler, taken or refused, then the struct or the reason
    void answer(uint8_t who, const char *why, const void *taken, size_t n)
    {
        byte(who);
        byte(why ? 2 : 0);
        if (why)
            bytes(why, strlen(why) + 1);
        else
            bytes(taken, n);
    }
};
// the new rows of one block, and what the corpus has reached so far
static const char *const kRowNames[6] = {"loops", "groups", "search10", "search01", "search11", "walk"};
struct Rows
{
    Fnv f[6];
    void print(const char *corpus, int k) const
    {
        for (int i = 0; i < 6; ++i)
            printf("%s.%s %d %016llx\n", kRowNames[i], corpus, k, (unsigned long long)f[i].h);
    }
};
static struct
{
    unsigned loops_taken = 0, groups_taken = 0, many_jumps = 0, no_jumps = 0;
    std::set<const char *> reasons;
} g_reached;
static void digest_walk(Fnv &f, const Walk &w)
{
    const uint8_t general = w.general ? 1 : 0;
    const int32_t anchors[2] = {w.bol, w.eol};
    f.bytes(w.table, sizeof w.table);
    f.bytes(&w.init, 4), f.bytes(&w.fin, 4), f.bytes(&w.self, 4);
    f.byte(general);
    f.bytes(&w.chain, 4), f.bytes(&w.n_jumps, 4);
    f.bytes(w.jump_src, sizeof w.jump_src), f.bytes(w.jump_dst, sizeof w.jump_dst);
    f.bytes(anchors, sizeof anchors);
    f.bytes(&w.filter, sizeof w.filter);
    g_reached.many_jumps += w.n_jumps > 8;
    g_reached.no_jumps += w.n_jumps == 0;
}
// the four compilers and the combined decision about one search
static void digest_search(Fnv &f, const search_params_t *p)
{
    krep_gpu_regex_info_t info;
    krep_gpu_regex_anchored_t an;
    krep_gpu_regex_alt_t alt;
    krep_gpu_regex_ext_t ext;
    kg::RegexCompiled rc;
    f.answer(1, kg::regex_compile(p, &info), &info, sizeof info);
    f.answer(2, kg::regex_compile_anchored(p, &an), &an, sizeof an);
    f.answer(3, kg::regex_compile_alt(p, &alt), &alt, sizeof alt);
    f.answer(4, kg::regex_compile_ext(p, &ext), &ext, sizeof ext);
    const char *why = kg::regex_compile_search(p, &rc);
    const Verdict v = why ? Verdict{} : verdict_of(rc);
    const int32_t head[3] = {v.took == 1, v.took == 1 ? v.bol : 0, v.took == 1 ? v.eol : 0};
    f.answer(5, why, head, sizeof head);
    if (!why)
        v.took == 1 ? f.bytes(v.alt, sizeof *v.alt) : f.bytes(v.seq, sizeof *v.seq);
}
// the loops and the groups compiler, the combined decision with their switches on, and the walk program of what they take
static void digest_search_new(Rows &R, const search_params_t *p)
{
    krep_gpu_regex_loops_t loops;
    krep_gpu_regex_groups_t groups;
    const char *why_loops = kg::regex_compile_loops(p, &loops), *why_groups = kg::regex_compile_groups(p, &groups);
    R.f[0].answer(6, why_loops, &loops, sizeof loops);
    R.f[1].answer(7, why_groups, &groups, sizeof groups);
    g_reached.reasons.insert(why_loops);
    g_reached.reasons.insert(why_groups);
    for (int k = 0; k < 3; ++k)
    {
        kg::RegexCompiled rc;
        const char *why = kg::regex_compile_search(p, &rc, k != 1, k != 0);
        const Verdict v = why ? Verdict{} : verdict_of(rc);
        const int32_t head[3] = {v.took, v.bol, v.eol};
        R.f[2 + k].answer((uint8_t)(8 + k), why, head, sizeof head);
    }
    if (!why_loops)
    {
        ++g_reached.loops_taken;
        digest_walk(R.f[5], walk_of_loops(loops));
        digest_walk(R.f[5], walk_forced_general(loops));
    }
    if (!why_groups)
    {
        ++g_reached.groups_taken;
        digest_walk(R.f[5], walk_of_groups(groups));
    }
}
struct Digest
{
    Fnv f;  // the rows of the four older compilers
    Rows r;
};
static void digest_entry(Digest &d, const std::vector<std::string> &pats, bool cs, bool ww = false, bool old_rows = true)
{
    Search s(pats, cs, ww);
    if (old_rows)
        digest_search(d.f, &s.p);
    digest_search_new(d.r, &s.p);
}
// did the whole corpus reach what the new rows are there to pin
static int check_reached()
{
    const char *const reasons[] = {kg::kRegexLoopsGroup, kg::kRegexLoopsEmpty, kg::kRegexLoopsNewline, kg::kRegexLoopsNone, kg::kRegexGroupsOlder,
                                   kg::kRegexGroupsNewline, kg::kRegexGroupsNullable, kg::kRegexGroupsEmptyAlt, kg::kRegexGroupsQuantQuant,
                                   kg::kRegexGroupsQuantNothing, kg::kRegexGroupsZero, kg::kRegexGroupsAnchor, kg::kRegexGroupsMixedAnchors,
                                   kg::kRegexGroupsTooManyPos, kg::kRegexGroupsTooDeep, kg::kRegexGroupsTooManyJumps, kg::kRegexGroupsNoFilter};
    int bad = 0;
    for (const char *why : reasons)
        if (!g_reached.reasons.count(why))
        {
            fprintf(stderr, "regex_compile_san --digest: the corpus never reaches the refusal \"%s\"\n", why);
            ++bad;
        }
    if (g_reached.loops_taken < 1000 || g_reached.groups_taken < 1000 || !g_reached.many_jumps || !g_reached.no_jumps)
    {
        fprintf(stderr, "regex_compile_san --digest: the loops compiler takes %u entries, the groups compiler %u (1000 each are wanted); %u walk "
                        "programs of more than 8 jump pairs, %u of none\n",
                g_reached.loops_taken, g_reached.groups_taken, g_reached.many_jumps, g_reached.no_jumps);
        ++bad;
    }
    return bad ? 1 : 0;
}
static int run_digest(int blocks)
{
    Digest d;
    Fnv &f = d.f;
    const char *probe[] = {".", "[^a]", "[[:space:]]", "[[:alpha:]]", "[[:punct:]]", "a", "\\.", "[a-]"};
    for (const char *a : probe)
        for (int cs = 1; cs >= 0; --cs)
        {
            uint8_t cls[32] = {0};
            f.byte(kg::regex_probe_atom((const uint8_t *)a, strlen(a), cs != 0, cls));
            f.bytes(cls, sizeof cls);
        }
    printf("classes 0 %016llx\n", (unsigned long long)f.h);
    // the tables, each entry in the case modes the default run uses for it
    f = Fnv();
    for (const char *s : ok)
        for (int cs = 0; cs < 2; ++cs)
            digest_entry(d, {s}, cs != 0);
    for (const char *s : no)
        digest_entry(d, {s}, true);
    for (const auto &c : aok)
        for (int cs = 0; cs < 2; ++cs)
            digest_entry(d, {c.pat}, cs != 0);
    for (const char *s : ano)
        digest_entry(d, {s}, true);
    for (const auto &c : alt_ok)
        for (int cs = 0; cs < 2; ++cs)
            digest_entry(d, c.pats, cs != 0);
    for (const char *s : alt_no)
        digest_entry(d, {s}, true);
    for (const auto &c : ext_ok)
        for (int cs = 0; cs < 2; ++cs)
            digest_entry(d, c.pats, cs != 0);
    for (const char *s : ext_no)
        digest_entry(d, {s}, true);
    for (const auto &pats : py_cases)
        digest_entry(d, pats, true);
    digest_entry(d, {"ab"}, true, true); // -w
    {
        Search s({"ab"}, true, false); // not a regex search
        s.p.use_regex = false;
        digest_search(f, &s.p);
        digest_search_new(d.r, &s.p);
    }
    {
        Search s({"a", "b"}, true, false); // several patterns announced, the arrays NULL
        s.p.patterns = nullptr;
        s.p.pattern_lens = nullptr;
        digest_search(f, &s.p);
        digest_search_new(d.r, &s.p);
    }
    {
        Search s({"a"}, true, false); // no pattern at all
        s.p.pattern = nullptr;
        s.p.patterns = nullptr;
        s.p.pattern_lens = nullptr;
        s.p.num_patterns = 0;
        digest_search(f, &s.p);
        digest_search_new(d.r, &s.p);
    }
    printf("named 0 %016llx\n", (unsigned long long)f.h);
    // the tables of the new rows alone, in both case modes (the traps: every compiler, whichever switch is on)
    for (int cs = 1; cs >= 0; --cs)
    {
        for (const auto &pats : loops_cases)
            digest_entry(d, pats, cs != 0, false, false);
        for (const auto &pats : groups_cases)
            digest_entry(d, pats, cs != 0, false, false);
        for (const char *s : quant_traps)
            digest_entry(d, {s}, cs != 0, false, false);
    }
    digest_entry(d, {"a+b"}, true, true, false);   // -w
    digest_entry(d, {"(ab)+"}, true, true, false);
    d.r.print("named", 0);
    // the random corpora: the generator always runs through (each corpus continues the state of the one before), the compilers are
    // asked in the first `blocks` blocks of each
    Rng r;
    std::string pat;
    std::vector<std::string> pats;
    for (int i = 0; i < kDraws; ++i)
    {
        if (i % 1000 == 0)
            d = Digest();
        draw_bytes(r, pat, pats);
        if (i / 1000 >= blocks)
            continue;
        const bool cs = (r.s >> 40) & 1;
        digest_entry(d, {pat}, cs);
        if (pats.size() > 1)
            digest_entry(d, pats, cs);
        if (i % 1000 == 999)
        {
            printf("bytes %d %016llx\n", i / 1000, (unsigned long long)f.h);
            d.r.print("bytes", i / 1000);
        }
    }
    for (int i = 0; i < kDraws; ++i)
    {
        if (i % 1000 == 0)
            d = Digest();
        draw_pieces(r, pats);
        if (i / 1000 >= blocks)
            continue;
        digest_entry(d, pats, (r.s >> 40) & 1);
        if (i % 1000 == 999)
        {
            printf("pieces %d %016llx\n", i / 1000, (unsigned long long)f.h);
            d.r.print("pieces", i / 1000);
        }
    }
    for (int i = 0; i < kQuantDraws; ++i)
    {
        if (i % 1000 == 0)
            d = Digest();
        draw_quants(r, pats);
        if (i / 1000 >= blocks)
            continue;
        digest_entry(d, pats, (r.s >> 40) & 1, false, false);
        if (i % 1000 == 999)
            d.r.print("quants", i / 1000);
    }
    return blocks >= kDraws / 1000 ? check_reached() : 0; // (a part of the corpus need not reach everything)
}

int main(int argc, char **argv)
{
    bool digest = false;
    int blocks = kDraws / 1000;
    for (int a = 1; a < argc; ++a)
        if (!strcmp(argv[a], "--digest"))
            digest = true;
        else if (!strcmp(argv[a], "--blocks") && a + 1 < argc)
            blocks = atoi(argv[++a]);
        else
        {
            fprintf(stderr, "usage: regex_compile_san [--digest [--blocks N]]\n");
            return 2;
        }
    if (digest)
        return run_digest(blocks);
    krep_gpu_regex_info_t info;
    const char *why = nullptr;
    int bad = 0;
    for (const char *s : ok)
        for (int cs = 0; cs < 2; ++cs)
            if (compile(s, cs != 0, false, &info, &why) != 0 || info.L < 1 || info.L > 16)
            {
                printf("FAIL: %s refused: %s\n", s, why ? why : "?");
                ++bad;
            }
    for (const char *s : no)
        if (compile(s, true, false, &info, &why) != 2 || !why || !*why)
        {
            printf("FAIL: %s accepted\n", s);
            ++bad;
        }
    if (compile("ab", true, true, &info, &why) != 2)
    {
        printf("FAIL: -w accepted\n");
        ++bad;
    }
    krep_gpu_regex_anchored_t an;
    for (const auto &c : aok)
        for (int cs = 0; cs < 2; ++cs)
            if (compile(c.pat, cs != 0, false, &info, &why, &an) != 0 || an.bol != c.bol || an.eol != c.eol || an.seq.L != c.L ||
                an.seq.self_overlap != c.overlap)
            {
                printf("FAIL: anchored %s: %s\n", c.pat, why ? why : "wrong fields");
                ++bad;
            }
    for (const char *s : ano)
        if (compile(s, true, false, &info, &why, &an) != 2 || !why || !*why)
        {
            printf("FAIL: anchored %s accepted\n", s);
            ++bad;
        }
    for (const char *s : {"^a", "a$", "^a$", "^", "$", "^$"})
        if (compile(s, true, false, &info, &why) != 2 || !why || !*why)
        {
            printf("FAIL: krep_gpu_regex_compile's compiler takes %s\n", s);
            ++bad;
        }
    if (compile("^ab", true, true, &info, &why, &an) != 2)
    {
        printf("FAIL: anchored -w accepted\n");
        ++bad;
    }
    krep_gpu_regex_alt_t alt;
    for (const auto &c : alt_ok)
        for (int cs = 0; cs < 2; ++cs)
            if (compile_alt(c.pats, cs != 0, false, &alt, &why) != 0 || alt.n_branches != c.nb || alt.Lmin != c.Lmin || alt.Lmax != c.Lmax ||
                alt.total_L != c.total || alt.cross_overlap != c.overlap || !alt_consistent(alt))
            {
                printf("FAIL: alt %s: %s\n", c.pats[0].c_str(), why ? why : "wrong fields");
                ++bad;
            }
    for (const char *s : alt_no)
        if (compile_alt({s}, true, false, &alt, &why) != 2 || !why || !*why || alt.n_branches != 0)
        {
            printf("FAIL: alt %s accepted\n", s);
            ++bad;
        }
    if (compile_alt({"a|b"}, true, true, &alt, &why) != 2 || compile_alt({"a", ""}, true, false, &alt, &why) != 2 ||
        compile_alt({"a", "b*"}, true, false, &alt, &why) != 2 || compile_alt({std::string(1100, 'a') + "|b"}, true, false, &alt, &why) != 2)
    {
        printf("FAIL: alt -w, an empty pattern, a refused second pattern or an overlong pattern accepted\n");
        ++bad;
    }
    Rng r;
    unsigned taken = 0, refused = 0, ataken = 0, alt_taken = 0;
    for (int i = 0; i < kDraws; ++i)
    {
        std::string pat;
        std::vector<std::string> pats;
        draw_bytes(r, pat, pats);
        const bool cs = (r.s >> 40) & 1;
        if (compile(pat, cs, false, &info, &why) == 0)
        {
            ++taken;
            if (info.L < 1 || info.L > 16 || info.anchor >= info.L || info.n_anchor > 4)
            {
                printf("FAIL: inconsistent info for a random pattern\n");
                ++bad;
            }
        }
        else
            ++refused;
        // the same string through the anchored compiler: it takes whatever the old one takes, with the same fields, and more
        const bool old_ok = why == nullptr;
        const krep_gpu_regex_info_t old = info;
        if (compile(pat, cs, false, &info, &why, &an) == 0)
        {
            ++ataken;
            if (an.seq.L < 1 || an.seq.L + (an.bol != 0) + (an.eol != 0) > 16 || an.seq.anchor >= an.seq.L || an.seq.n_anchor > 4 ||
                (an.bol != 0) != (pat[0] == '^') || (an.eol && pat.back() != '$') || (old_ok && (an.bol || an.eol || memcmp(&old, &an.seq, sizeof old))))
            {
                printf("FAIL: inconsistent anchored info for a random pattern\n");
                ++bad;
            }
        }
        else if (old_ok)
        {
            printf("FAIL: the anchored compiler refuses what the old one takes\n");
            ++bad;
        }
        // the same string, cut in two at a drawn place every other time, through the alternation compiler: it takes whatever the old
        // one takes as a single branch, and what it takes is consistent
        if (compile_alt(pats, cs, false, &alt, &why) == 0)
        {
            ++alt_taken;
            if (!alt_consistent(alt) || (old_ok && pats.size() == 1 && (alt.n_branches != 1 || memcmp(&old, &alt.branch[0], sizeof old))))
            {
                printf("FAIL: inconsistent alternation info for a random pattern\n");
                ++bad;
            }
        }
        else if ((old_ok && pats.size() == 1) || alt.n_branches != 0)
        {
            printf("FAIL: the alternation compiler refuses a single sequence the old one takes, or leaves a refused struct filled\n");
            ++bad;
        }
    }
    printf("regex_compile_san: %u random patterns taken, %u refused, %u taken with anchors allowed, %u taken as alternations, %d failures\n", taken,
           refused, ataken, alt_taken, bad);
    krep_gpu_regex_ext_t ext;
    for (const auto &c : ext_ok)
        for (int cs = 0; cs < 2; ++cs)
            if (compile_ext(c.pats, cs != 0, false, &ext, &why) != 0 || ext.bol != c.bol || ext.eol != c.eol || ext.alt.n_branches != c.nb ||
                ext.alt.Lmin != c.Lmin || ext.alt.Lmax != c.Lmax || ext.alt.total_L != c.total || ext.alt.cross_overlap != c.overlap ||
                ext.alt.Lmax + ext.bol + ext.eol > 16 || ext.alt.total_L + ext.alt.n_branches * (ext.bol + ext.eol) > 32)
            {
                printf("FAIL: ext %s: %s\n", c.pats[0].c_str(), why ? why : "wrong fields");
                ++bad;
            }
    for (const char *s : ext_no)
        if (compile_ext({s}, true, false, &ext, &why) != 2 || !why || !*why || ext.alt.n_branches != 0 || ext.bol || ext.eol)
        {
            printf("FAIL: ext %s accepted\n", s);
            ++bad;
        }
    if (compile_ext({"colou?r"}, true, true, &ext, &why) != 2 || compile_ext({"a?b", ""}, true, false, &ext, &why) != 2 ||
        compile_ext({"a", "^b"}, true, false, &ext, &why) != 2 || compile_ext({std::string(1100, 'a') + "?b"}, true, false, &ext, &why) != 2)
    {
        printf("FAIL: ext -w, an empty pattern, mixed anchors or an overlong pattern accepted\n");
        ++bad;
    }
    unsigned ext_taken = 0, ext_refused = 0;
    for (int i = 0; i < kDraws; ++i)
    {
        std::vector<std::string> pats;
        draw_pieces(r, pats);
        const bool cs = (r.s >> 40) & 1;
        if (compile_ext(pats, cs, false, &ext, &why) == 0)
        {
            ++ext_taken;
            const unsigned extra = (unsigned)(ext.bol + ext.eol);
            krep_gpu_regex_alt_t plain = ext.alt; // (a branch's self_overlap is that of the sequence alone, cross_overlap knows the anchors)
            for (unsigned b = 0; extra && b < plain.n_branches; ++b)
                plain.branch[b].self_overlap = 0;
            if (!alt_consistent(plain) || ext.alt.Lmax + extra > 16 || ext.alt.total_L + ext.alt.n_branches * extra > 32 || (ext.bol | ext.eol) >> 1)
            {
                printf("FAIL: inconsistent expansion for a random pattern\n");
                ++bad;
            }
            // what the alternation compiler takes, this one takes as the same alternation
            if (compile_alt(pats, cs, false, &alt, &why) == 0 && (extra || memcmp(&alt, &ext.alt, sizeof alt)))
            {
                printf("FAIL: the expanding compiler differs from the alternation compiler on a pattern both take\n");
                ++bad;
            }
        }
        else
        {
            ++ext_refused;
            if (ext.alt.n_branches != 0 || compile_alt(pats, cs, false, &alt, &why) == 0)
            {
                printf("FAIL: the expanding compiler refuses what the alternation compiler takes, or leaves a refused struct filled\n");
                ++bad;
            }
        }
    }
    printf("regex_compile_san: expanding compiler: %u random patterns of its grammar taken, %u refused, %d failures in all\n", ext_taken, ext_refused, bad);
    return bad ? 1 : 0;
}
