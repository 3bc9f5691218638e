"""krep_gpu_regex_compile_alt (host only): the branches and the fields of every accepted shape, every refusal with its reason, the
two older compilers unchanged, cross_overlap against brute force, and what the selectors and the split rule say."""
import ctypes as C

import numpy as np
import pytest

import krep_amd
import regex_alt_model as am
import regex_model
import regex_ref
from krep_amd import abi
from krep_amd.engine import KrepGpuError


@pytest.fixture(autouse=True, scope="module")
def _c_locale():
    """the reference runs in the C locale (it never calls setlocale()); Python's start-up put the process into the environment's"""
    with regex_ref.c_locale():
        yield


@pytest.fixture(scope="module")
def eng():
    return krep_amd.load()


def rx(*pats, **kw):
    return abi.Params(list(pats), regex=True, **kw)


# patterns -> (the merged branches, cross_overlap)
ACCEPTED = [
    ((b"cat|d[oi]g|b.rd",), [b"cat", b"d[oi]g", b"b.rd"], 1),           # b.rd + dog share the d
    ((b"(ERROR)|(WARN[0-9])",), [b"ERROR", b"WARN[0-9]"], 0),
    ((b"ERROR", b"WARN[0-9]"), [b"ERROR", b"WARN[0-9]"], 0),            # several patterns: what the CLI joins as (p1)|(p2)
    ((b"ERROR|FATAL", b"(WARN[0-9])"), [b"ERROR", b"FATAL", b"WARN[0-9]"], 0),
    ((b"(a)|(b)|(a)",), [b"a", b"b"], 0),                               # identical branches are merged
    ((b"[ab]|[ba]|c",), [b"[ab]", b"c"], 0),                            # ... by their class tables
    ((b"a{16}|b{16}",), [b"a{16}", b"b{16}"], 1),                       # total_L = 32; a{16} overlaps itself
    ((b"ab|abc",), [b"ab", b"abc"], 1), ((b"ab|cd",), [b"ab", b"cd"], 0), ((b"a|aa",), [b"a", b"aa"], 1),
    ((b"abcd|bc",), [b"abcd", b"bc"], 1), ((b"bc|abcd",), [b"bc", b"abcd"], 1),
    ((b"a[|]b|c\\|d|[(]x[)]",), [b"a[|]b", b"c\\|d", b"[(]x[)]"], 0),     # | ( ) in brackets or behind a backslash are ordinary
    ((b"(Sherl[oO]ck)",), [b"Sherl[oO]ck"], 0),
    ((b"x|[a-c]{16}",), [b"x", b"[a-c]{16}"], 1),
]


@pytest.mark.parametrize("cs", [True, False])
def test_branches_fields_and_overlap(eng, cs):
    for pats, brs, ov in ACCEPTED:
        info = eng.regex_compile_alt(rx(*pats, case_sensitive=cs))
        Ls = [len(regex_model.classes(b, cs)) for b in brs]
        assert info.n_branches == len(brs) and (info.Lmin, info.Lmax, info.total_L) == (min(Ls), max(Ls), sum(Ls)), pats
        assert info.cross_overlap == ov and info.reserved == 0, pats
        for i, b in enumerate(brs):
            alone = eng.regex_compile(rx(b, case_sensitive=cs))  # each branch exactly what the single compiler makes of it
            assert bytes(C.string_at(C.addressof(info.branch[i]), C.sizeof(alone))) == bytes(C.string_at(C.addressof(alone), C.sizeof(alone)))
        for i in range(len(brs), 8):
            assert info.branch[i].L == 0
        # the helper the GPU tests lean on says the same
        model = am.branches(list(pats), cs)
        assert [len(m) for m in model] == Ls and am.cross_overlap(model) == bool(ov), pats


REFUSALS = [
    (b"a|", "empty branch"), (b"|a", "empty branch"), (b"()", "empty branch"), (b"a||b", "empty branch"), (b"a|()", "empty branch"),
    (b"((a))", "nested"), (b"(a(b))", "nested"),
    (b"(a", "unbalanced"), (b"a)", "unbalanced"), (b"a|(b", "unbalanced"),
    (b"x(a|b)y", "not a whole branch"), (b"(ab)c", "not a whole branch"), (b"(ab){2}", "not a whole branch"), (b"(a)(b)", "not a whole branch"),
    (b"(a|b)", "holds an alternation"),
    (b"^a|b", "anchors inside"), (b"a|b$", "anchors inside"), (b"(^a)|b", "anchors inside"), (b"a|^|b", "anchors inside"),
    (b"a|b|c|d|e|f|g|h|i", "more than 8 branches"),
    (b"a{17}|b", "more than 16"), (b"b|" + b"a" * 17, "more than 16"),
    (b"a{16}|b{16}|c", "more than 32"),
    # what the single-sequence compiler refuses, in a branch
    (b"a|b.*", "automaton"), (b"a+|b", "automaton"), (b"a|b?", "automaton"), (b"a{2,3}|b", "varying"), (b"a|\\bw", "operator"),
    (b"a|caf\xe9", "0x01-0x7F"), (b"a|[bc", "without its"), (b"a|b\\", "trailing backslash"), (b"a|b{0}", "optional"), (b"a|{2}", "not behind an atom"),
]


def test_refusals_carry_a_reason(eng):
    reasons = {}
    for pat, word in REFUSALS:
        with pytest.raises(KrepGpuError, match=word) as e:
            eng.regex_compile_alt(rx(pat))
        reasons[pat] = str(e.value)
    new = (b"a|", b"((a))", b"(a", b"(ab)c", b"(a|b)", b"^a|b", b"a|b|c|d|e|f|g|h|i", b"a{17}|b", b"a{16}|b{16}|c")
    assert len({reasons[p] for p in new}) == len(new)  # each kind its own
    assert all(reasons[p].endswith("kept on krep's regex_search") for p in new)
    with pytest.raises(KrepGpuError, match="-w"):
        eng.regex_compile_alt(rx(b"a|b", whole_word=True))
    with pytest.raises(KrepGpuError, match="empty"):
        eng.regex_compile_alt(rx(b"a", b""))
    with pytest.raises(KrepGpuError, match="1024"):
        eng.regex_compile_alt(rx(b"a|" + b"b" * 1100))
    with pytest.raises(KrepGpuError, match="not a regex"):
        eng.regex_compile_alt(abi.Params([b"a|b"]))
    # nine branches of which two are the same are eight
    assert eng.regex_compile_alt(rx(b"a|b|c|d|e|f|g|h|a")).n_branches == 8
    with pytest.raises(KrepGpuError, match="multibyte"):
        import locale
        old = locale.setlocale(locale.LC_CTYPE)
        try:
            locale.setlocale(locale.LC_CTYPE, "C.UTF-8")
            eng.regex_compile_alt(rx(b"a|b"))
        finally:
            locale.setlocale(locale.LC_CTYPE, old)


def test_the_two_older_compilers_keep_refusing(eng):
    for pat in (b"a|b", b"(ab)"):
        with pytest.raises(KrepGpuError, match="automaton"):
            eng.regex_compile(rx(pat))
        with pytest.raises(KrepGpuError, match="automaton"):
            eng.regex_compile_anchored(rx(pat))
    for fn in (eng.regex_compile, eng.regex_compile_anchored):
        with pytest.raises(KrepGpuError, match="several regex patterns are an alternation"):
            fn(rx(b"ab", b"cd"))


def test_selectors_and_split_ask_the_alt_compiler_second(eng, monkeypatch):
    monkeypatch.setenv("KREP_GPU_ASSUME_AVAILABLE", "1")
    monkeypatch.delenv("KREP_GPU_DISABLE", raising=False)
    n = 1 << 20
    for p in (rx(b"ab|cd"), rx(b"ab|abc"), rx(b"ab", b"cd"), rx(b"(Sherl[oO]ck)"), rx(b"cat|d[oi]g|b.rd", case_sensitive=False)):
        assert eng.can_accelerate(p) and eng.select(p) is not None
    assert eng.split_mode(rx(b"ab|cd"), n) == abi.SPLIT_PIECES
    assert eng.split_mode(rx(b"ab|abc"), n) == abi.SPLIT_WHOLE
    assert eng.split_mode(rx(b"ab|abc", count_lines=True), n) == abi.SPLIT_PIECES
    assert eng.split_mode(rx(b"ab", b"abc"), n) == abi.SPLIT_WHOLE and eng.split_mode(rx(b"ab", b"cd"), n) == abi.SPLIT_PIECES
    assert not eng.can_accelerate(rx(b"a|b.*")) and eng.select(rx(b"a|b.*")) is None
    assert not eng.can_accelerate(rx(b"ab|cd", whole_word=True)) and eng.select(rx(b"ab", b"c+")) is None
    # one cache entry serves every pattern of a search: the second pattern decides here
    assert eng.can_accelerate(rx(b"ab", b"cd")) and not eng.can_accelerate(rx(b"ab", b"c*")) and eng.can_accelerate(rx(b"ab", b"cd"))
    assert eng.split_mode(rx(b"ab", b"cd"), n) == abi.SPLIT_PIECES and eng.split_mode(rx(b"ab", b"bd"), n) == abi.SPLIT_WHOLE
    # a single sequence is still the anchored compiler's: the plan's algorithm is regex_search either way
    assert eng.split_mode(rx(b"[ab]{3}"), n) == abi.SPLIT_WHOLE and eng.split_mode(rx(b"^ab"), n) == abi.SPLIT_PIECES


def test_the_reason_of_a_pattern_both_compilers_refuse(eng, monkeypatch):
    """the alt compiler's when the search says an alternation (an unbracketed, unescaped | or (, or several patterns), else the
    anchored compiler's, as before"""
    monkeypatch.setenv("KREP_GPU_ASSUME_AVAILABLE", "1")
    text = np.frombuffer(b"abc", dtype=np.uint8)
    for p, word in ((rx(b"a||b"), "empty branch"), (rx(b"((a))"), "nested"), (rx(b"a", b"^b"), "anchors inside"),
                    (rx(b"a^b"), "not the first"), (rx(b"a[|]b*"), "automaton"), (rx(b"a\\|^b"), "not the first")):
        assert not eng.can_accelerate(p)
        with pytest.raises(KrepGpuError, match=word):
            eng.search(p, text)  # (refused before any device is touched: the failure road reports the reason)


ATOMS = [b"a", b"b", b"c", b"d", b"e", b"f", b"g", b"h", b"[ab]", b"[^a-h]", b"c{2}"]


def witness(brs):
    """a text in which two occurrences share a byte, built from the class intersections of the first (i, j, d) that allows it"""
    for i, a in enumerate(brs):
        for j, b in enumerate(brs):
            for d in range(1 if i == j else 0, len(a)):
                if all((a[d + t] & b[t]).any() for t in range(min(len(a) - d, len(b)))):
                    n = max(len(a), d + len(b))
                    t = np.zeros(n, dtype=np.uint8)
                    for k in range(n):
                        ok = np.ones(256, dtype=bool)
                        if k < len(a):
                            ok &= a[k]
                        if 0 <= k - d < len(b):
                            ok &= b[k - d]
                        t[k] = np.flatnonzero(ok)[0]
                    return t, i, j, d
    return None


def test_cross_overlap_against_brute_force(eng):
    rng = np.random.RandomState(31)
    alphabet = np.frombuffer(b"abcdefgh\x00", dtype=np.uint8)
    flags = [0, 0]
    for _ in range(300):
        srcs = [b"".join(ATOMS[rng.randint(len(ATOMS))] for _ in range(rng.randint(1, 4))) for _ in range(rng.randint(2, 4))]
        info = eng.regex_compile_alt(rx(b"|".join(srcs)))
        brs = am.branches([b"|".join(srcs)])
        assert info.n_branches == len(brs)
        flags[info.cross_overlap] += 1
        if info.cross_overlap:
            t, i, j, d = witness(brs)  # branch i at 0 and branch j at d < L_i: two occurrences (of two branches when d == 0)
            assert 0 in regex_model.occurrences(brs[i], t) and d in regex_model.occurrences(brs[j], t) and (i != j or d) and d < len(brs[i]), srcs
        else:
            assert witness(brs) is None
            for _ in range(200):
                text = alphabet[rng.randint(0, alphabet.size, size=40)]
                used = np.zeros(40, dtype=np.int32)
                for s, L in am.all_occurrences(brs, text):
                    used[s:s + L] += 1
                assert used.max(initial=0) <= 1, (srcs, text.tobytes())
    assert min(flags) >= 20, flags
