"""krep_gpu_regex_compile_groups (host only, through Engine.regex_compile_groups): the named expressions are taken, every refusal has
its reason, the older compilers keep what is theirs, the limits (32 positions, depth 8, 12 jump pairs), the switch
krep_gpu_set_regex_groups through the selector and the compile cache, the returned automaton simulated in Python against the compiled
reference's records, the filter property, and the struct's layout as a C host compiles it."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import krep_amd
import regex_groups_model as gm
import regex_ref
from krep_amd import abi
from krep_amd.engine import KrepGpuError
from test_regex_groups_model_cpu import ALPHABET, IP, NAMED, named_text, random_groups_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# of the named expressions this one multiplies out to four sequences: the expanding compiler takes it, so it stays that compiler's
EXT_TAKES = [b"(a|ab)(c|bcd)"]


@pytest.fixture(autouse=True, scope="module")
def _c_locale():
    with regex_ref.c_locale():
        yield


@pytest.fixture(scope="module")
def eng():
    return krep_amd.load()


def rx(*pats, **kw):
    return abi.Params(list(pats), regex=True, **kw)


def check_against_reference(g, pats, cs, texts):
    """the automaton the library returned, simulated, gives the reference's records; every record holds a filter occurrence"""
    au = gm.from_compiled(g)
    assert 1 <= len(g["filter"]) <= 8 and all(1 <= len(f) <= 16 for f in g["filter"]) and sum(len(f) for f in g["filter"]) <= 32
    found = 0
    for text in texts:
        ref = gm.ref_call(pats, text, case_sensitive=cs)
        got = gm.run_automaton(au, text, case_sensitive=cs)
        assert ref[0] == got[0] and np.array_equal(ref[1], got[1]), (pats, cs, text.tobytes(), ref, got)
        assert gm.filter_misses(g["filter"], text, ref[1]) == [], (pats, cs, text.tobytes(), g["filter"])
        found += ref[0]
    return found


@pytest.mark.parametrize("k", range(len(NAMED)))
def test_the_named_expressions_are_taken_and_their_automaton_gives_the_reference_records(eng, k):
    pats, alphabet = NAMED[k]
    if pats in [[p] for p in EXT_TAKES]:
        eng.regex_compile_ext(rx(*pats))
        with pytest.raises(KrepGpuError, match="an older compiler takes"):
            eng.regex_compile_groups(rx(*pats))
        return
    rng = np.random.RandomState(7300 + k)
    texts = [named_text(rng, k, alphabet) for _ in range(120)]
    for cs in (True, False):
        g = eng.regex_compile_groups(rx(*pats, case_sensitive=cs))
        assert g["n_pos"] == len(g["classes"]) == len(g["follow"]) <= 32
        assert (g["bol"], g["eol"]) == (pats[0].startswith(b"^"), pats[0].endswith(b"$"))
        model = gm.automaton(pats, cs)
        assert g["n_pos"] == len(model.atoms) and [bytes(np.flatnonzero(t).astype(np.uint8)) for t in model.tables] == g["classes"]
        assert check_against_reference(g, pats, cs, texts) > 10, pats


def test_the_ip_expression_is_fifteen_positions_and_filters_on_a_factor_around_the_dot(eng):
    g = eng.regex_compile_groups(rx(IP))
    assert g["n_pos"] == 15 and g["first"] == {0} and g["last"] == {12, 13, 14}
    assert g["filter"] == [[b"0123456789", b".", b"0123456789"]]
    assert eng.regex_compile_groups(rx(b"(foo|bar){2,3};"))["filter"] == [[b"f", b"o", b"o"], [b"b", b"a", b"r"]]
    assert eng.regex_compile_groups(rx(b"((ab)+c)+d"))["filter"] == [[b"a", b"b", b"c", b"d"]]


REFUSALS = [
    (b"(ab)+[[:space:]]", "holds '\\\\n'"), (b"(a\n)+", "holds '\\\\n'"),
    (b"(ab)*", "matches the empty string"), (b"(a|b*)+", "matches the empty string"), (b"(ab)+|c*", "matches the empty string"),
    (b"(ab|)+", "empty alternative or an empty group"), (b"()+a", "empty alternative or an empty group"), (b"(ab)+|", "empty alternative"),
    (b"(ab)+?", "quantifier behind a quantifier"), (b"(ab){2}{3}", "quantifier behind a quantifier"),
    (b"(+ab)+", "not behind an atom or a group"), (b"*(ab)+", "not behind an atom or a group"),
    (b"(ab){0}c", "zero times"), (b"(ab)+c{0,0}", "zero times"),
    (b"(^ab)+", "anchors inside"), (b"(ab$)+", "anchors inside"), (b"(ab)+^c", "anchors inside"), (b"(ab)+$c", "anchors inside"),
    (b"^(ab)+|c", "do not all carry the same"), (b"(ab)+$|(cd)+", "do not all carry the same"),
    (b"(" + b"abcdefghijk" * 3 + b")+", "more than 32 positions"), (b"(ab){17}", "more than 32 positions"), (b"(ab){1000,}", "more than 32 positions"),
    (b"(" * 9 + b"a" + b")" * 9 + b"+", "nested deeper than 8"),
    (b"(a|b)(c|d)(e|f)(g|h)(i|j)(k|l)(m|n)(o|p)", "more than 12 jump pairs"),
    (b"(ab)+(c", "unbalanced"), (b"(ab)+)", "unbalanced"), (b"((ab)+", "unbalanced"),
    (b"(ab){2,", "malformed"), (b"(ab){,2}", "malformed"), (b"(ab){3,2}", "malformed"),
    (b"(caf\xe9)+", "0x01-0x7F"), (b"(a\\b)+", "operator"), (b"([ab)+", "without its"), (b"(ab)+\\", "trailing backslash"),
]


def test_refusals_carry_a_reason(eng):
    reasons = {}
    for pat, word in REFUSALS:
        with pytest.raises(KrepGpuError, match=word) as e:
            eng.regex_compile_groups(rx(pat))
        reasons[pat] = str(e.value)
        info = abi.RegexGroups()
        assert eng.lib.krep_gpu_regex_compile_groups(rx(pat).ref, C.byref(info)) == 2
        assert bytes(C.string_at(C.addressof(info), C.sizeof(info))) == bytes(C.sizeof(info)), pat  # *out zeroed
    kinds = (b"(a\n)+", b"(ab)*", b"(ab|)+", b"(ab)+?", b"(+ab)+", b"(ab){0}c", b"(^ab)+", b"^(ab)+|c", b"(ab){17}",
             b"(" * 9 + b"a" + b")" * 9 + b"+", b"(a|b)(c|d)(e|f)(g|h)(i|j)(k|l)(m|n)(o|p)", b"(ab)+(c", b"(ab){2,")
    assert len({reasons[p] for p in kinds}) == len(kinds)  # each kind its own
    with pytest.raises(KrepGpuError, match="do not all carry the same"):
        eng.regex_compile_groups(rx(b"(ab)+", b"^(cd)+"))
    with pytest.raises(KrepGpuError, match="-w"):
        eng.regex_compile_groups(rx(b"(ab)+", whole_word=True))
    with pytest.raises(KrepGpuError, match="not a regex"):
        eng.regex_compile_groups(abi.Params([b"(ab)+"]))
    with pytest.raises(KrepGpuError, match="multibyte"):
        import locale
        old = locale.setlocale(locale.LC_CTYPE)
        try:
            locale.setlocale(locale.LC_CTYPE, "C.UTF-8")
            eng.regex_compile_groups(rx(b"(ab)+"))
        finally:
            locale.setlocale(locale.LC_CTYPE, old)


def test_the_older_compilers_keep_what_is_theirs(eng):
    for fn, pats in ((eng.regex_compile_anchored, (b"^ab[0-9]$",)), (eng.regex_compile_alt, (b"ab|cd",)), (eng.regex_compile_alt, (b"ab", b"cd")),
                     (eng.regex_compile_ext, (b"colou?r",)), (eng.regex_compile_ext, (b"(a|ab)(c|bcd)",)), (eng.regex_compile_loops, (b"a+b",)),
                     (eng.regex_compile_loops, (b"x(a+|b)y",)), (eng.regex_compile_loops, (b"ERROR.*timeout",))):
        fn(rx(*pats))
        with pytest.raises(KrepGpuError, match="an older compiler takes"):
            eng.regex_compile_groups(rx(*pats))
    # ... and answer for the new expressions as before
    with pytest.raises(KrepGpuError, match="behind a group"):
        eng.regex_compile_loops(rx(b"(ab)+"))
    with pytest.raises(KrepGpuError, match="more than 8 distinct"):
        eng.regex_compile_ext(rx(IP))
    with pytest.raises(KrepGpuError, match="nested"):
        eng.regex_compile_ext(rx(b"^((GET|POST) |HEAD )/api"))


def test_the_limits(eng):
    az = b"abcdefghijklmnopqrstuvwxyz"
    g = eng.regex_compile_groups(rx(b"(" + az + az[:6] + b")+"))  # 32 positions, the last one hands back to position 0
    assert g["n_pos"] == 32 and g["follow"][31] == {0} and g["first"] == {0} and g["last"] == {31}
    with pytest.raises(KrepGpuError, match="more than 32 positions"):
        eng.regex_compile_groups(rx(b"(" + az + az[:7] + b")+"))
    g = eng.regex_compile_groups(rx(az[:12] + b"(" + az[:20] + b")+"))  # ... and to a position in the middle
    assert g["n_pos"] == 32 and g["follow"][31] == {12}
    assert eng.regex_compile_groups(rx(b"(" * 8 + b"ab" + b")" * 8 + b"+"))["n_pos"] == 2
    with pytest.raises(KrepGpuError, match="nested deeper than 8"):
        eng.regex_compile_groups(rx(b"(" * 9 + b"ab" + b")" * 9 + b"+"))
    # every (x|y)(z|w) boundary is two jump pairs: six boundaries are taken, seven are not
    assert eng.regex_compile_groups(rx(b"(a|b)(c|d)(e|f)(g|h)(i|j)(k|l)(m|n)"))["n_pos"] == 14
    with pytest.raises(KrepGpuError, match="more than 12 jump pairs"):
        eng.regex_compile_groups(rx(b"(a|b)(c|d)(e|f)(g|h)(i|j)(k|l)(m|n)(o|p)"))
    # counted quantifiers copy their operand, whichever way: behaviour is compared, not bits
    for pat, text, want in ((b"(ab){2,}", b"ab abab ababab", [[3, 7], [8, 14]]), (b"(ab){1,2}(c)+", b"abababcc", [[2, 8]])):
        g = eng.regex_compile_groups(rx(pat))
        assert gm.run_automaton(gm.from_compiled(g), text)[1].tolist() == want


def test_random_expressions_their_automaton_and_their_filter(eng):
    """400 generated expressions that REACH this compiler (one an older compiler keeps is drawn again): at most one quarter may be
    refused, for positions, jump pairs or the filter's width; every other one is simulated against the reference"""
    rng = np.random.RandomState(20261022)
    refused, taken, older, found = 0, 0, 0, 0
    while taken + refused < 400:
        pats, cs = random_groups_case(rng)
        try:
            g = eng.regex_compile_groups(rx(*pats, case_sensitive=cs))
        except KrepGpuError as e:
            if "an older compiler takes" in str(e):
                older += 1  # (a group that multiplies out to a few flat sequences)
            else:
                assert any(w in str(e) for w in ("32 positions", "jump pairs", "fixed-length factors")), (pats, str(e))
                refused += 1
            continue
        taken += 1
        texts = [ALPHABET[rng.randint(0, ALPHABET.size, size=rng.randint(0, 31))].copy() for _ in range(6)]
        found += check_against_reference(g, pats, cs, texts)
    assert refused <= 100 and taken + refused == 400 and found > 500, (refused, taken, older, found)


def test_an_expression_without_a_filter_is_refused(eng):
    """nine alternatives in front of an optional tail: every match passes one of nine positions, none of which can be lengthened, and
    a filter holds at most eight sequences"""
    with pytest.raises(KrepGpuError, match="no set of at most 8 fixed-length factors"):
        eng.regex_compile_groups(rx(b"(a|b|c|d|e|f|g|h|i)(xy)*"))
    assert len(eng.regex_compile_groups(rx(b"(a|b|c|d|e|f|g|h)(xy)*"))["filter"]) == 8


def test_the_switch_and_the_cache(eng, monkeypatch):
    monkeypatch.setenv("KREP_GPU_ASSUME_AVAILABLE", "1")
    monkeypatch.delenv("KREP_GPU_DISABLE", raising=False)
    text = np.frombuffer(b"abc", dtype=np.uint8)
    n = 1 << 20
    assert not eng.get_regex_groups() and not eng.get_regex_loops()  # off unless the process asked for it
    today = ((rx(b"(ab)+"), "not a whole branch"), (rx(IP), "more than 8 distinct"), (rx(b"^((GET|POST) |HEAD )/api"), "anchors inside"),
             (rx(b"(ab)*"), "not a whole branch"), (rx(b"a*"), "automaton"), (rx(b"(ab)+", whole_word=True), "-w"), (rx(b"a.*b"), "automaton"))

    def reasons():
        out = []
        for p, _ in today:
            assert not eng.can_accelerate(p) and eng.select(p) is None
            with pytest.raises(KrepGpuError) as e:
                eng.search(p, text)
            out.append(str(e.value))
        return out

    try:
        off = reasons()
        for (p, word), why in zip(today, off):
            assert word in why, (word, why)
        eng.set_regex_groups(True)
        assert eng.get_regex_groups() and not eng.get_regex_loops()  # (independent of the loops switch)
        for p in (rx(b"(ab)+"), rx(IP), rx(b"^((GET|POST) |HEAD )/api", count_lines=True), rx(b"(ab)+", b"c(d|e)*f"), rx(b"(ab)+$", case_sensitive=False)):
            assert eng.can_accelerate(p) and eng.select(p) is not None
            assert eng.split_mode(p, n) == abi.SPLIT_WHOLE
        # what an older compiler takes is theirs as before; the loops compiler is not asked while its own switch is off
        assert eng.can_accelerate(rx(b"(a|ab)(c|bcd)")) and eng.split_mode(rx(b"colou?r"), n) == abi.SPLIT_PIECES
        for p, word in ((rx(b"a.*b"), "automaton"), (rx(b"a*"), "automaton"), (rx(b"(ab)+", whole_word=True), "-w"),
                        (rx(b"(ab)*"), "matches the empty string"), (rx(b"(ab)+[[:space:]]"), "holds '\\\\n'"),
                        (rx(b"(a|b)(c|d)(e|f)(g|h)(i|j)(k|l)(m|n)(o|p)"), "jump pairs")):
            assert not eng.can_accelerate(p) and eng.select(p) is None
            with pytest.raises(KrepGpuError, match=word):
                eng.search(p, text)
        assert eng.batch_can_accelerate(rx(b"(ab)+")) and eng.batch_can_accelerate(rx(b"(ab)+$"))
        assert not eng.batch_can_accelerate(rx(b"(ab)+$", case_sensitive=False)) and "REG_NOTEOL" in eng.last_error()
        eng.set_regex_loops_windows(True)
        assert eng.split_mode(rx(b"(ab)+"), n) == abi.SPLIT_PIECES
        eng.set_regex_loops_windows(False)
        eng.set_regex_loops(True)  # both: each compiler what is its own
        assert eng.can_accelerate(rx(b"a.*b")) and eng.can_accelerate(rx(b"(ab)+"))
        eng.set_regex_loops(False)
        eng.set_regex_groups(False)
        assert reasons() == off  # (the cache keys on the switch: everything answers as before)
    finally:
        eng.set_regex_groups(False)
        eng.set_regex_loops(False)
        eng.set_regex_loops_windows(False)


def test_the_symbols_are_exported_and_declared(eng):
    boundary = open(os.path.join(ROOT, "include", "krep_gpu.h")).read()
    hooks = open(os.path.join(ROOT, "include", "krep_gpu_debug.h")).read()
    for n, decl, where in (("krep_gpu_regex_compile_groups", "int krep_gpu_regex_compile_groups(", boundary),
                           ("krep_gpu_set_regex_groups", "void krep_gpu_set_regex_groups(int on);", boundary),
                           ("krep_gpu_get_regex_groups", "int krep_gpu_get_regex_groups(void);", boundary),
                           ("krep_gpu_debug_force_regex_general", "void krep_gpu_debug_force_regex_general(int on);", hooks)):
        assert hasattr(eng.lib, n) and decl in where, n


def test_struct_layout_matches_a_c11_probe(tmp_path):
    names = ["n_pos", "classes", "first", "last", "follow", "bol", "eol", "filter"]
    exprs = ["sizeof(krep_gpu_regex_groups_t)"] + [f"offsetof(krep_gpu_regex_groups_t, {f})" for f in names]
    want = [C.sizeof(abi.RegexGroups)] + [getattr(abi.RegexGroups, f).offset for f in names]
    src = tmp_path / "groups_abi.c"
    src.write_text('#include "krep_gpu.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void) { printf("'
                   + " ".join(["%zu"] * len(exprs)) + '\\n", ' + ", ".join(exprs) + "); return 0; }\n")
    exe = tmp_path / "groups_abi"
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-pedantic", "-Werror", f"-I{os.path.join(ROOT, 'include')}",
                        str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == want, (got, want)
