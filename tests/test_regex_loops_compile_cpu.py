"""krep_gpu_regex_compile_loops (host only): every accepted shape's sequences of places, repeat masks, anchors and filter equal the ones
written by hand; every refusal with its reason; the filter property against the brute-force model (a line that holds a match holds
an occurrence of the filter); the switch krep_gpu_set_regex_loops through the selector, the compile cache and the split rule; and the
struct's layout as a C host compiles it."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import krep_amd
import regex_loops_model as lm
import regex_ref
from krep_amd import abi
from krep_amd.engine import KrepGpuError
from test_regex_loops_model_cpu import random_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True, scope="module")
def _c_locale():
    with regex_ref.c_locale():
        yield


@pytest.fixture(scope="module")
def eng():
    return krep_amd.load()


def rx(*pats, **kw):
    return abi.Params(list(pats), regex=True, **kw)


def lit(s: bytes):
    """the places of a literal: one byte each, none repeats"""
    return [(s[i:i + 1], False) for i in range(len(s))]


def table_bytes(atoms, cs):
    """the 32-byte sets of a row of atoms, as the struct holds them"""
    rows = []
    for a in atoms:
        t = np.zeros(256, dtype=bool)
        t[list(regex_ref.probe_class(a, cs))] = True
        rows.append(np.packbits(t, bitorder="little").tobytes())
    return b"".join(rows)


def have_sequences(alt, repeat=None):
    return {(bytes(alt.branch[i].classes)[:32 * alt.branch[i].L], int(repeat[i]) if repeat is not None else 0) for i in range(alt.n_branches)}


def want_sequences(seqs, cs):
    return {(table_bytes([a for a, _ in s], cs), sum(1 << j for j, (_, plus) in enumerate(s) if plus)) for s in seqs}


REP = True
# patterns -> (the expanded sequences of places by hand, bol, eol, the filter's sequences by hand)
ACCEPTED = [
    ((b"ERROR.*timeout",), [lit(b"ERRORtimeout"), lit(b"ERROR") + [(b".", REP)] + lit(b"timeout")], 0, 0,
     [lit(b"ERRORtimeout"), [(b".", False)] + lit(b"timeout")]),                      # every match holds "timeout": each factor does
    ((b"a+b",), [[(b"a", REP), (b"b", False)]], 0, 0, [lit(b"ab")]),
    ((b"[0-9]+",), [[(b"[0-9]", REP)]], 0, 0, [[(b"[0-9]", False)]]),
    ((b"ab+c",), [[(b"a", False), (b"b", REP), (b"c", False)]], 0, 0, [lit(b"ab")]),    # a tie between ab and bc: the leftmost
    ((b"ab+cd",), [[(b"a", False), (b"b", REP)] + lit(b"cd")], 0, 0, [lit(b"bcd")]),    # the smaller product wins over the leftmost
    ((b"a{2,}b",), [[(b"a", False), (b"a", REP), (b"b", False)]], 0, 0, [lit(b"aa")]),  # a tie between aa and ab
    ((b"a{1,}b",), [[(b"a", REP), (b"b", False)]], 0, 0, [lit(b"ab")]),
    ((b"a{3,}",), [[(b"a", False), (b"a", False), (b"a", REP)]], 0, 0, [lit(b"aaa")]),
    ((b"a*b",), [lit(b"b"), [(b"a", REP), (b"b", False)]], 0, 0, [lit(b"b"), lit(b"ab")]),
    ((b"a{0,}b",), [lit(b"b"), [(b"a", REP), (b"b", False)]], 0, 0, [lit(b"b"), lit(b"ab")]),
    ((b"colou*r",), [lit(b"color"), lit(b"colo") + [(b"u", REP), (b"r", False)]], 0, 0, [lit(b"color"), lit(b"colou")]),
    ((b"^#+ ",), [[(b"#", REP), (b" ", False)]], 1, 0, [lit(b"# ")]),
    ((b"b+$",), [[(b"b", REP)]], 0, 1, [lit(b"b")]),
    ((b"^a+$",), [[(b"a", REP)]], 1, 1, [lit(b"a")]),
    ((b"x(a+|b)y",), [[(b"x", False), (b"a", REP), (b"y", False)], lit(b"xby")], 0, 0, [lit(b"xa"), lit(b"xby")]),
    ((b"[a-z]+@[a-z]+\\.com",), [[(b"[a-z]", REP), (b"@", False), (b"[a-z]", REP), (b"\\.", False)] + lit(b"com")], 0, 0,
     [[(b"[a-z]", False), (b"\\.", False)] + lit(b"com")]),
    ((b"[0-9]+\\.[0-9]+",), [[(b"[0-9]", REP), (b"\\.", False), (b"[0-9]", REP)]], 0, 0, [[(b"[0-9]", False), (b"\\.", False), (b"[0-9]", False)]]),
    ((b"a+", b"b+c"), [[(b"a", REP)], [(b"b", REP), (b"c", False)]], 0, 0, [lit(b"a"), lit(b"bc")]),
    ((b"a+b|ab",), [[(b"a", REP), (b"b", False)], lit(b"ab")], 0, 0, [lit(b"ab")]),     # two sequences that differ in a flag, one factor
    ((b"(a+b){2}",), [[(b"a", REP), (b"b", False)] * 2], 0, 0, [lit(b"aba")]),           # a+ may stand at both ends of a factor: a b a
    ((b"[ab]+c?",), [[(b"[ab]", REP)], [(b"[ab]", REP), (b"c", False)]], 0, 0, [[(b"[ab]", False)], [(b"[ab]", False), (b"c", False)]]),
    ((b"^(GET|POST) .+",), [lit(b"GET ") + [(b".", REP)], lit(b"POST ") + [(b".", REP)]], 1, 0,
     [lit(b"GET ") + [(b".", False)], lit(b"POST ") + [(b".", False)]]),
]


@pytest.mark.parametrize("cs", [True, False])
def test_sequences_masks_anchors_and_filter_equal_the_hand_written_ones(eng, cs):
    for pats, seqs, bol, eol, flt in ACCEPTED:
        info = eng.regex_compile_loops(rx(*pats, case_sensitive=cs))
        assert (info.bol, info.eol) == (bol, eol), pats
        a = info.alt
        assert a.n_branches == len(seqs) and a.total_L == sum(len(s) for s in seqs), pats
        assert (a.Lmin, a.Lmax) == (min(len(s) for s in seqs), max(len(s) for s in seqs)), pats
        assert have_sequences(a, info.repeat) == want_sequences(seqs, cs), pats
        for i in range(a.n_branches, 8):
            assert a.branch[i].L == 0 and info.repeat[i] == 0
        f = info.filter
        assert f.n_branches == len(flt) and have_sequences(f) == want_sequences(flt, cs), pats
        assert all(1 <= f.branch[i].L <= 16 for i in range(f.n_branches)) and f.total_L <= 32
        # each filter branch is what krep_gpu_regex_compile() makes of that sequence alone
        for i in range(f.n_branches):
            assert f.branch[i].anchor < f.branch[i].L
        # the model's own expansion and filter rule say the same
        mb, me, brs = lm.branches(list(pats), cs)
        assert (mb, me) == (bool(bol), bool(eol)) and len(brs) == a.n_branches, pats
        model_filter = {np.packbits(np.stack(s), axis=1, bitorder="little").tobytes() for s in lm.filter_of(list(pats), cs)}
        assert model_filter == {k for k, _ in have_sequences(f)}, pats


REFUSALS = [
    (b"(ab)+", "behind a group"), (b"(a|b)*c", "behind a group"), (b"x(ab){2,}", "behind a group"), (b"(a+)+", "behind a group"),
    (b"[[:space:]]+x", "holds '\\\\n'"), (b"a\n+", "holds '\\\\n'"), (b"a+[b\n]", "holds '\\\\n'"), (b"a+[[:cntrl:]]", "holds '\\\\n'"),
    (b"a*", "holds no place"), (b"a*b*", "holds no place"), (b"x|a*", "holds no place"), (b"^a*$", "holds no place"), (b"(a|b*)", "holds no place"),
    (b"colou?r", "holds no \\*"), (b"ab", "holds no \\*"), (b"^(ERROR|WARN)", "holds no \\*"), (b"a{2,3}", "holds no \\*"),
    (b"a+*", "quantifier behind a quantifier"), (b"a*?", "quantifier behind a quantifier"), (b"a+{2}", "quantifier behind a quantifier"),
    (b"a{2,}?", "quantifier behind a quantifier"),
    (b"x((a+))", "nested"), (b"x(a+", "unbalanced"), (b"a+)b", "unbalanced"),
    (b"(a+|)b", "empty alternative"), (b"a+|", "empty branch"),
    (b"x(^a+|b)", "inside a group"), (b"a+^b", "in the middle"), (b"^a+|b", "anchors inside"),
    (b"+a", "not behind an atom"), (b"a|*b", "not behind an atom"), (b"^+a", "repeats the anchor"), (b"^*", "repeats the anchor"),
    (b"a{17,}", "more than 16 places"), (b"^a{16,}", "more than 16 places"), (b"a{9}b+a{7}", "more than 16 places"),
    (b"[ab]{1,9}c+", "more than 8 distinct"), (b"a*b*c*d*e", "more than 8 distinct"),
    (b"a{16}|b{16,}|c", "more than 32 places"),
    (b"a{2,", "malformed"), (b"a{,2}", "malformed"), (b"a{1001,}", "malformed"),
    (b"caf\xe9+", "0x01-0x7F"), (b"a\\b+", "operator"), (b"[ab+", "without its"), (b"ab+\\", "trailing backslash"),
]


def test_refusals_carry_a_reason(eng):
    reasons = {}
    for pat, word in REFUSALS:
        with pytest.raises(KrepGpuError, match=word) as e:
            eng.regex_compile_loops(rx(pat))
        reasons[pat] = str(e.value)
        info = abi.RegexLoops()
        assert eng.lib.krep_gpu_regex_compile_loops(rx(pat).ref, C.byref(info)) == 2
        assert bytes(C.string_at(C.addressof(info), C.sizeof(info))) == bytes(C.sizeof(info)), pat  # *out zeroed
    kinds = (b"(ab)+", b"a\n+", b"a*", b"ab", b"a+*", b"x((a+))", b"a{17,}", b"[ab]{1,9}c+", b"a{16}|b{16,}|c")
    assert len({reasons[p] for p in kinds}) == len(kinds)  # each kind its own
    with pytest.raises(KrepGpuError, match="anchors inside"):
        eng.regex_compile_loops(rx(b"a+", b"^b"))
    with pytest.raises(KrepGpuError, match="-w"):
        eng.regex_compile_loops(rx(b"a+b", whole_word=True))
    with pytest.raises(KrepGpuError, match="not a regex"):
        eng.regex_compile_loops(abi.Params([b"a+b"]))
    with pytest.raises(KrepGpuError, match="multibyte"):
        import locale
        old = locale.setlocale(locale.LC_CTYPE)
        try:
            locale.setlocale(locale.LC_CTYPE, "C.UTF-8")
            eng.regex_compile_loops(rx(b"a+b"))
        finally:
            locale.setlocale(locale.LC_CTYPE, old)
    # the older compilers answer for the same expressions as before
    for fn in (eng.regex_compile, eng.regex_compile_anchored, eng.regex_compile_alt):
        with pytest.raises(KrepGpuError, match="automaton"):
            fn(rx(b"a+b"))
    with pytest.raises(KrepGpuError, match="without a bound"):
        eng.regex_compile_ext(rx(b"a+b"))
    with pytest.raises(KrepGpuError, match="without a bound"):
        eng.regex_compile_ext(rx(b"a{2,}"))


def filter_tables(info):
    out = []
    for i in range(info.filter.n_branches):
        br = info.filter.branch[i]
        bits = np.unpackbits(np.frombuffer(bytes(br.classes)[:32 * br.L], dtype=np.uint8).reshape(br.L, 32), axis=1, bitorder="little")
        out.append([row.astype(bool) for row in bits])
    return out


def test_every_line_that_holds_a_match_holds_an_occurrence_of_the_filter(eng):
    rng = np.random.RandomState(4096)
    lines_with_match = 0
    for _ in range(2000):
        pats, text, kw = random_case(rng)
        cs = kw["case_sensitive"]
        info = eng.regex_compile_loops(rx(*pats, case_sensitive=cs))
        flt = filter_tables(info)
        model = lm.filter_of(pats, cs)
        key = lambda f: sorted(np.packbits(np.stack(s), axis=1, bitorder="little").tobytes() for s in f)
        assert key(flt) == key(model), pats
        if text.size == 0:
            continue
        prog = lm.branches(pats, cs)
        for (ls, le), found in zip(lm.line_spans(text), lm.matches(prog, text, cs)):
            if found:
                lines_with_match += 1
                assert lm.filter_occurs(flt, text, ls, le), (pats, text.tobytes(), ls, le)
                for s, e in found:  # ... inside the match itself
                    assert lm.filter_occurs(flt, text, s, e), (pats, text.tobytes(), s, e)
    assert lines_with_match > 1000


def test_the_switch_the_cache_and_the_split_rule(eng, monkeypatch):
    monkeypatch.setenv("KREP_GPU_ASSUME_AVAILABLE", "1")
    monkeypatch.delenv("KREP_GPU_DISABLE", raising=False)
    n = 1 << 20
    text = np.frombuffer(b"abc", dtype=np.uint8)
    assert not eng.get_regex_loops()  # off unless the process asked for it
    try:
        for p, today in ((rx(b"a.*b"), "automaton"), (rx(b"a{2,}"), "varying"), (rx(b"a(b|c)+"), "not a whole branch")):
            assert not eng.can_accelerate(p) and eng.select(p) is None
            with pytest.raises(KrepGpuError, match=today):
                eng.search(p, text)
        assert eng.split_mode(rx(b"a.*b"), n) == abi.SPLIT_WHOLE  # (a search no compiler takes is WHOLE as before)
        eng.set_regex_loops(True)
        assert eng.get_regex_loops()
        for p in (rx(b"a.*b"), rx(b"a{2,}"), rx(b"^#+ ", count_lines=True), rx(b"a+", b"b+c"), rx(b"[0-9]+\\.[0-9]+", case_sensitive=False)):
            assert eng.can_accelerate(p) and eng.select(p) is not None
            assert eng.split_mode(p, n) == abi.SPLIT_WHOLE
        # what the older compilers take is theirs as before, what all four refuse reports what it reported before
        assert eng.split_mode(rx(b"colou?r"), n) == abi.SPLIT_PIECES and eng.can_accelerate(rx(b"colou?r"))
        for p, today in ((rx(b"a(b|c)+"), "not a whole branch"), (rx(b"a*"), "automaton"), (rx(b"a+b", whole_word=True), "-w")):
            assert not eng.can_accelerate(p) and eng.select(p) is None
            with pytest.raises(KrepGpuError, match=today):
                eng.search(p, text)
        assert eng.batch_can_accelerate(rx(b"a.*b")) and eng.batch_can_accelerate(rx(b"b+$"))
        assert not eng.batch_can_accelerate(rx(b"b+$", case_sensitive=False)) and "REG_NOTEOL" in eng.last_error()
        eng.set_regex_loops(False)
        assert not eng.can_accelerate(rx(b"a.*b")) and eng.select(rx(b"a.*b")) is None  # (the cache keys on the switch)
        assert not eng.batch_can_accelerate(rx(b"a.*b"))
        eng.set_regex_loops(True)
        assert eng.can_accelerate(rx(b"a.*b"))
    finally:
        eng.set_regex_loops(False)
    assert not eng.can_accelerate(rx(b"a.*b"))


def test_the_symbols_are_exported_and_declared(eng):
    boundary = open(os.path.join(ROOT, "include", "krep_gpu.h")).read()
    hooks = open(os.path.join(ROOT, "include", "krep_gpu_debug.h")).read()
    for n, decl, where in (("krep_gpu_regex_compile_loops", "int krep_gpu_regex_compile_loops(", boundary),
                           ("krep_gpu_set_regex_loops", "void krep_gpu_set_regex_loops(int on);", boundary),
                           ("krep_gpu_get_regex_loops", "int krep_gpu_get_regex_loops(void);", boundary),
                           ("krep_gpu_debug_force_regex_loops_road", "void krep_gpu_debug_force_regex_loops_road(int road);", hooks),
                           ("krep_gpu_debug_regex_loops_roads", "void krep_gpu_debug_regex_loops_roads(", hooks)):
        assert hasattr(eng.lib, n) and decl in where, n


def test_struct_layout_matches_a_c11_probe(tmp_path):
    names = ["alt", "bol", "eol", "repeat", "filter"]
    exprs = ["sizeof(krep_gpu_regex_loops_t)"] + [f"offsetof(krep_gpu_regex_loops_t, {f})" for f in names]
    want = [C.sizeof(abi.RegexLoops)] + [getattr(abi.RegexLoops, f).offset for f in names]
    src = tmp_path / "loops_abi.c"
    src.write_text('#include "krep_gpu.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void) { printf("'
                   + " ".join(["%zu"] * len(exprs)) + '\\n", ' + ", ".join(exprs) + "); return 0; }\n")
    exe = tmp_path / "loops_abi"
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-pedantic", "-Werror", f"-I{os.path.join(ROOT, 'include')}",
                        str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == want, (got, want)
    assert C.sizeof(abi.RegexLoops) == 2 * C.sizeof(abi.RegexAlt) + 8 + 16
