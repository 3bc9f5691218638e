"""krep_gpu_regex_compile_ext (host only): every accepted shape's branches equal the hand-written expansion, bol / eol, every refusal
with its reason, cross_overlap against brute force, what the selectors and the split rule say, and the three older compilers
answering exactly as before."""
import ctypes as C

import numpy as np
import pytest

import krep_amd
import regex_ext_model as em
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


def raw(info):
    return bytes(C.string_at(C.addressof(info), C.sizeof(info)))


# patterns -> (the expansion written by hand, as an unanchored alternation; bol; eol; cross_overlap)
ACCEPTED = [
    ((b"colou?r",), b"color|colour", 0, 0, 0),
    ((b"https?://",), b"http://|https://", 0, 0, 0),
    ((b"[0-9]{1,3}%",), b"[0-9]%|[0-9]{2}%|[0-9]{3}%", 0, 0, 1),
    ((b"x(a|bc)y",), b"xay|xbcy", 0, 0, 0),
    ((b"(GET|POST) /api",), b"GET /api|POST /api", 0, 0, 0),
    ((b"(ab){2}",), b"abab", 0, 0, 1),
    ((b"(ab){2}|b{0,2}a",), b"abab|a|ba|bba", 0, 0, 1),
    ((b"(a|ab)(c|bcd)?",), b"a|ac|abcd|ab|abc|abbcd", 0, 0, 1),
    ((b"[ab]{1,3}c",), b"[ab]c|[ab]{2}c|[ab]{3}c", 0, 0, 1),
    ((b"a(b?|c)d",), b"ad|abd|acd", 0, 0, 0),                             # a quantifier inside a group
    ((b"(a|b){2}",), b"aa|ab|ba|bb", 0, 0, 1),
    ((b"([ab]|[ba])c",), b"[ab]c", 0, 0, 0),                                # identical class tables merge
    ((b"^(ERROR|WARN|FATAL)",), b"ERROR|WARN|FATAL", 1, 0, 0),
    ((b"\\.(jpg|png)$",), b"\\.jpg|\\.png", 0, 1, 0),
    ((b"^GET", b"^POST"), b"GET|POST", 1, 0, 0),
    ((b"^GET", b"^POST[0-9]"), b"GET|POST[0-9]", 1, 0, 0),
    ((b"^a|^b",), b"a|b", 1, 0, 0),
    ((b"^(ab|cd)",), b"ab|cd", 1, 0, 0),
    ((b"(foo|quux)$",), b"foo|quux", 0, 1, 0),
    ((b"^(a|bc)d?$",), b"a|ad|bc|bcd", 1, 1, 1),                            # a and ad start alike: the same start always counts
    ((b"^(a{14}|b{14})$",), b"a{14}|b{14}", 1, 1, 0),                       # all 32 places; ^ rules out a{14} inside itself
    ((b"(x|[a-c]{15})$",), b"x|[a-c]{15}", 0, 1, 0),                        # $ rules out [a-c]{15} inside itself
    ((b"^(j[[:space:]]ab|\nc)",), b"j[[:space:]]ab|\nc", 1, 0, 0),
    ((b"^[ab]{1,3}$",), b"[ab]|[ab]{2}|[ab]{3}", 1, 1, 1),
    ((b"^(ab|a)c?$",), b"ab|abc|a|ac", 1, 1, 1),
    ((b"^(a|b\n)b",), b"ab|b\nb", 1, 0, 1),                                 # b\nb: the newline lets ^ab start inside it
    ((b"(a|b)[ab\n]?$",), b"a|b|a[ab\n]|b[ab\n]", 0, 1, 1),
    ((b"ab|cd",), b"ab|cd", 0, 0, 0),                                       # what the older compilers take is taken here too
    ((b"^ab$",), b"ab", 1, 1, 0),
]


@pytest.mark.parametrize("cs", [True, False])
def test_branches_equal_the_hand_written_expansion(eng, cs):
    for pats, by_hand, bol, eol, ov in ACCEPTED:
        ext = eng.regex_compile_ext(rx(*pats, case_sensitive=cs))
        want = eng.regex_compile_alt(rx(by_hand, case_sensitive=cs))
        assert (ext.bol, ext.eol) == (bol, eol), pats
        a = ext.alt
        assert (a.n_branches, a.Lmin, a.Lmax, a.total_L, a.reserved) == (want.n_branches, want.Lmin, want.Lmax, want.total_L, 0), pats
        assert {raw(a.branch[i]) for i in range(a.n_branches)} == {raw(want.branch[i]) for i in range(want.n_branches)}, pats
        for i in range(a.n_branches, 8):
            assert a.branch[i].L == 0
        assert a.cross_overlap == ov, pats
        if not (bol or eol):
            assert a.cross_overlap == want.cross_overlap, pats
        # the model's own expansion says the same
        mb, me, brs = em.branches(list(pats), cs)
        assert (mb, me) == (bool(bol), bool(eol)) and sorted(len(b) for b in brs) == sorted(a.branch[i].L for i in range(a.n_branches)), pats
        have = {bytes(np.packbits(np.stack(b), axis=1, bitorder="little").tobytes()) for b in brs}
        assert have == {bytes(a.branch[i].classes)[:32 * a.branch[i].L] for i in range(a.n_branches)}, pats


REFUSALS = [
    (b"ab*", "without a bound"), (b"a+b", "without a bound"), (b"a{2,}", "without a bound"), (b"(a|b)*c", "without a bound"),
    (b"a?{2}", "quantifier behind a quantifier"), (b"a{2}{3}", "quantifier behind a quantifier"), (b"a??", "quantifier behind a quantifier"),
    (b"(a|b)?{2}", "quantifier behind a quantifier"),
    (b"a?", "holds no byte class"), (b"(a|b)?", "holds no byte class"), (b"a?b?", "holds no byte class"), (b"a{0,1}", "holds no byte class"),
    (b"x|a?", "holds no byte class"), (b"^a?$", "holds no byte class"),
    (b"a{0}", "zero times"), (b"xa{0,0}", "zero times"),
    (b"^$", "on their own"), (b"^", "on their own"), (b"$", "on their own"),
    (b"x(a|)y", "empty alternative"), (b"x()y", "empty alternative"), (b"(|a)b", "empty alternative"),
    (b"a|", "empty branch"), (b"|a", "empty branch"), (b"a||b", "empty branch"),
    (b"x((a))", "nested"), (b"(a(b|c))d", "nested"),
    (b"x(a", "unbalanced"), (b"a)b", "unbalanced"), (b"(a|b", "unbalanced"),
    (b"x(^a|b)", "inside a group"), (b"(a|b$)x", "inside a group"), (b"(^a)|(^b)", "inside a group"),
    (b"a^b", "in the middle"), (b"a$b", "in the middle"), (b"^^a", "in the middle"), (b"a$$", "in the middle"),
    (b"^a|b", "anchors inside"), (b"a|b$", "anchors inside"), (b"^a|b$", "anchors inside"),
    (b"[ab]{1,9}", "more than 8 distinct"), (b"(a|b)(c|d)(e|f)(g|h)", "more than 8 distinct"), (b"a?b?c?d?e", "more than 8 distinct"),
    (b"a{17}", "more than 16 places"), (b"^a{16}", "more than 16 places"), (b"^a{15}$", "more than 16 places"), (b"a{9}(b|c)a{8}", "more than 16 places"),
    (b"a{16}|b{16}|c", "more than 32 places"), (b"^(a{15}|b{15}|c)", "more than 32 places"), (b"^(a{14}|b{14}|c)$", "more than 32 places"),
    (b"caf\xe9?", "0x01-0x7F"), (b"a\\b?", "operator"), (b"[ab?", "without its"), (b"ab?\\", "trailing backslash"),
    (b"{2}a", "not behind an atom"), (b"a|?b", "not behind an atom"), (b"(?a)", "not behind an atom"), (b"^{2}a", "repeats the anchor"),
    (b"a{2", "malformed"), (b"a{x}", "malformed"), (b"a{3,2}", "malformed"),
]


def test_refusals_carry_a_reason(eng):
    reasons = {}
    for pat, word in REFUSALS:
        with pytest.raises(KrepGpuError, match=word) as e:
            eng.regex_compile_ext(rx(pat))
        reasons[pat] = str(e.value)
    kinds = (b"ab*", b"a{2,}", b"a?{2}", b"a?", b"a{0}", b"x(a|)y", b"x((a))", b"x(^a|b)", b"a^b", b"[ab]{1,9}", b"a{17}", b"a{16}|b{16}|c")
    assert len({reasons[p] for p in kinds}) == len(kinds)  # each kind its own
    assert all(reasons[p].endswith("kept on krep's regex_search") for p in kinds)
    with pytest.raises(KrepGpuError, match="anchors inside"):
        eng.regex_compile_ext(rx(b"a", b"^b"))
    with pytest.raises(KrepGpuError, match="-w"):
        eng.regex_compile_ext(rx(b"colou?r", whole_word=True))
    with pytest.raises(KrepGpuError, match="empty"):
        eng.regex_compile_ext(rx(b"a?b", b""))
    with pytest.raises(KrepGpuError, match="1024"):
        eng.regex_compile_ext(rx(b"a?" + b"b" * 1100))
    with pytest.raises(KrepGpuError, match="not a regex"):
        eng.regex_compile_ext(abi.Params([b"colou?r"]))
    # nine sequences of which two are the same are eight
    assert eng.regex_compile_ext(rx(b"(a|b|c|d)(e|f)|ae")).alt.n_branches == 8
    with pytest.raises(KrepGpuError, match="multibyte"):
        import locale
        old = locale.setlocale(locale.LC_CTYPE)
        try:
            locale.setlocale(locale.LC_CTYPE, "C.UTF-8")
            eng.regex_compile_ext(rx(b"colou?r"))
        finally:
            locale.setlocale(locale.LC_CTYPE, old)


OLD_AND_NEW = [(b"Sherl[oO]ck",), (b"^ab",), (b"ab$",), (b"a{3}",), (b"ab|cd",), (b"(ab)|(cd)",), (b"ab", b"cd"), (b"a.*b",), (b"a|b.*",),
               (b"colou?r",), (b"x(a|bc)y",), (b"^(ERROR|WARN)",), (b"(foo|quux)$",), (b"^GET", b"^POST"), (b"[ab]{1,3}c",), (b"(ab){2}",),
               (b"a?",), (b"^a|b",), (b"a", b"^b"), (b"a{2,}",), (b"(a|b)",), (b"a||b",)]
# what the three older compilers said about each before this one existed: None = taken, else a word of the reason
BEFORE = {
    "regex_compile": [None, "anchored", "anchored", None, "automaton", "automaton", "several", "automaton", "automaton",
                      "automaton", "automaton", "anchored", "automaton", "several", "varying", "automaton",
                      "automaton", "anchored", "several", "varying", "automaton", "automaton"],
    "regex_compile_anchored": [None, None, None, None, "automaton", "automaton", "several", "automaton", "automaton",
                               "automaton", "automaton", "automaton", "automaton", "several", "varying", "automaton",
                               "automaton", "automaton", "several", "varying", "automaton", "automaton"],
    "regex_compile_alt": [None, "anchors inside", "anchors inside", None, None, None, None, "automaton", "automaton",
                          "automaton", "not a whole branch", "anchors inside", "holds an alternation", "anchors inside", "varying", "not a whole branch",
                          "automaton", "anchors inside", "anchors inside", "varying", "holds an alternation", "empty branch"],
}


@pytest.mark.parametrize("name", sorted(BEFORE))
def test_the_three_older_compilers_answer_as_before(eng, name):
    fn = getattr(eng, name)
    for pats, word in zip(OLD_AND_NEW, BEFORE[name]):
        if word is None:
            fn(rx(*pats))
        else:
            with pytest.raises(KrepGpuError, match=word):
                fn(rx(*pats))
    # and what they take is, field by field, what it was: a sequence the alternation compiler and this one both take is the same
    for pats in ((b"ab|cd",), (b"ab", b"cd"), (b"cat|d[oi]g|b.rd",)):
        assert raw(eng.regex_compile_alt(rx(*pats))) == raw(eng.regex_compile_ext(rx(*pats)).alt)
    one = eng.regex_compile_anchored(rx(b"^Sherl[oO]ck$"))
    ext = eng.regex_compile_ext(rx(b"^Sherl[oO]ck$"))
    assert (ext.bol, ext.eol, ext.alt.n_branches) == (1, 1, 1) and bytes(ext.alt.branch[0].classes) == bytes(one.seq.classes)


def test_selectors_and_split(eng, monkeypatch):
    monkeypatch.setenv("KREP_GPU_ASSUME_AVAILABLE", "1")
    monkeypatch.delenv("KREP_GPU_DISABLE", raising=False)
    n = 1 << 20
    for p in (rx(b"colou?r"), rx(b"https?://"), rx(b"x(a|bc)y"), rx(b"^(ERROR|WARN)"), rx(b"(foo|quux)$"), rx(b"^GET", b"^POST[0-9]"),
              rx(b"[ab]{1,3}c", case_sensitive=False), rx(b"^(a{14}|b{14})$", count_lines=True)):
        assert eng.can_accelerate(p) and eng.select(p) is not None
    assert eng.split_mode(rx(b"^(ab|cd)"), n) == abi.SPLIT_PIECES
    assert eng.split_mode(rx(b"[ab]{1,3}c"), n) == abi.SPLIT_WHOLE
    assert eng.split_mode(rx(b"^[ab]{1,3}$"), n) == abi.SPLIT_WHOLE  # the three lengths at one start count as an overlap
    assert eng.split_mode(rx(b"^[ab]{1,3}$", count_lines=True), n) == abi.SPLIT_PIECES
    assert eng.split_mode(rx(b"colou?r"), n) == abi.SPLIT_PIECES and eng.split_mode(rx(b"(x|[a-c]{15})$"), n) == abi.SPLIT_PIECES
    for p in (rx(b"a(b|c)*"), rx(b"colou?r", whole_word=True), rx(b"^a|b"), rx(b"a", b"^b"), rx(b"a?"), rx(b"[ab]{1,9}")):
        assert not eng.can_accelerate(p) and eng.select(p) is None
    # one cache entry serves the whole search: the case mode and the second pattern decide
    assert eng.can_accelerate(rx(b"^a", b"^b")) and not eng.can_accelerate(rx(b"^a", b"b")) and eng.can_accelerate(rx(b"^a", b"^b"))


def test_the_reason_of_a_search_every_compiler_refuses(eng, monkeypatch):
    """what it was before this compiler existed, unless only this compiler's own limits are in the way"""
    monkeypatch.setenv("KREP_GPU_ASSUME_AVAILABLE", "1")
    text = np.frombuffer(b"abc", dtype=np.uint8)
    for p, word in ((rx(b"a(b|c)*"), "not a whole branch"), (rx(b"ab*"), "automaton"), (rx(b"a", b"^b"), "anchors inside"),
                    (rx(b"^a|b"), "anchors inside"), (rx(b"a^b"), "not the first"), (rx(b"a{2,}"), "varying"), (rx(b"a||b"), "empty branch"),
                    (rx(b"a{17}"), "more than 16 byte classes"), (rx(b"a|b|c|d|e|f|g|h|i"), "more than 8 branches"),
                    # this compiler's own limits
                    (rx(b"a?"), "holds no byte class"), (rx(b"[ab]{1,9}"), "more than 8 distinct"), (rx(b"a{9}(b|c)a{8}"), "more than 16 places"),
                    (rx(b"^(a{15}|b{15}|c)"), "more than 32 places")):
        assert not eng.can_accelerate(p)
        with pytest.raises(KrepGpuError, match=word):
            eng.search(p, text)  # (refused before any device is touched: the failure road reports the reason)


def shares_a_byte(prog, text, cs=True):
    used = np.zeros(text.size + 1, dtype=np.int32)
    starts = {}
    for s, L in em.all_occurrences(prog, text, cs):
        used[s:s + L] += 1
        starts[s] = starts.get(s, 0) + 1
    return used.max(initial=0) > 1 or any(v > 1 for v in starts.values())


ATOMS = [b"a", b"b", b"c", b"[ab]", b"[a\n]", b"\n", b"[^a-c]", b"b?", b"a{1,2}", b"(a|bc)", b"(b|\n)?"]


def test_cross_overlap_against_brute_force(eng):
    """cross_overlap == 0: in no text do two occurrences share a byte or a start.  (1 may be conservative: the same start on two
    branches always counts, whatever the anchors.)"""
    rng = np.random.RandomState(32)
    alphabet = np.frombuffer(b"abc\n\nd", dtype=np.uint8)
    flags = [0, 0]
    done = 0
    while done < 300:
        bol, eol = (b"^" if rng.randint(2) else b""), (b"$" if rng.randint(2) else b"")
        brs = [bol + b"c" + b"".join(ATOMS[rng.randint(len(ATOMS))] for _ in range(rng.randint(1, 3))) + eol for _ in range(rng.randint(1, 3))]
        pat = b"|".join(brs)
        try:
            info = eng.regex_compile_ext(rx(pat))
        except KrepGpuError:
            continue
        done += 1
        prog = em.branches([pat])
        assert info.alt.n_branches == len(prog[2]), pat
        flags[info.alt.cross_overlap] += 1
        if not info.alt.cross_overlap:
            for _ in range(150):
                text = alphabet[rng.randint(0, alphabet.size, size=30)]
                assert not shares_a_byte(prog, text), (pat, text.tobytes())
    assert min(flags) >= 20, flags
    # the anchors rule an overlap out only where the newline they need cannot stand
    for pat, ov in ((b"^[ab]{2}c?", 1), (b"^ab?a", 0), (b"ab?a", 1), (b"^[a\n]b?a", 1), (b"ab?a$", 0), (b"a[b\n]?a$", 1),
                    (b"^(aba|b)", 0), (b"(aba|b)", 1), (b"(aba|b)$", 0), (b"(a\na|b?\n)$", 1)):
        assert eng.regex_compile_ext(rx(pat)).alt.cross_overlap == ov, pat
