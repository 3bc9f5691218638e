"""tests/regex_loops_model.py against the compiled reference's regex_search: the per-line rule the device scan reproduces for what
krep_gpu_regex_compile_loops() takes (*, + and {n,} behind an atom, beside ?, {n,m}, inner groups and one pair of line anchors):
lines are independent, the leftmost start of a line that has a match, its longest end over all branches, the walk resumes at that
end.  Every pattern the generator emits is one the compiler accepts; the test asserts that, so no case is skipped."""
import numpy as np
import pytest

import krep_amd
import regex_loops_model as lm
import regex_ref
from krep_amd import abi


@pytest.fixture(autouse=True, scope="module")
def _c_locale():
    with regex_ref.c_locale():
        yield


@pytest.fixture(scope="module")
def eng():
    return krep_amd.load()


ATOMS = [b"a", b"a", b"b", b"b", b"c", b"d", b".", b"[ab]", b"[^a]", b"[a-c]", b"B"]
QUANTS = [b"", b"", b"", b"*", b"+", b"+", b"{2,}", b"{1,}", b"{0,}", b"?", b"{1,2}", b"{2}"]
ALPHABET = np.frombuffer(b"aabbcdA\n\n", dtype=np.uint8)  # five letters (one of them in both cases), and the newline


def pick(rng, seq):
    return seq[rng.randint(len(seq))]


def random_seq(rng, lo, hi):
    return b"".join(pick(rng, ATOMS) + pick(rng, QUANTS) for _ in range(rng.randint(lo, hi + 1)))


def random_branch(rng):
    items = []
    for _ in range(rng.randint(1, 4)):
        if rng.randint(4) == 0:
            items.append(b"(" + b"|".join(random_seq(rng, 1, 2) for _ in range(rng.randint(1, 3))) + b")" + pick(rng, (b"", b"", b"?", b"{1,2}")))
        else:
            items.append(pick(rng, ATOMS) + pick(rng, QUANTS))
    return b"".join(items)


def random_case(rng):
    """only what the grammar and the limits of the compiler admit (lm.accepted: the model's own expansion, not the compiler)"""
    while True:
        bol, eol = (b"^" if rng.randint(4) == 0 else b""), (b"$" if rng.randint(4) == 0 else b"")
        brs = [bol + random_branch(rng) + eol for _ in range(rng.randint(1, 3))]
        k = rng.randint(1, len(brs) + 1)
        pats = [b"|".join(brs[:k])] + brs[k:]  # several patterns, as the CLI joins them, every now and then
        cs = bool(rng.randint(3))
        if lm.accepted(pats, cs):
            break
    text = ALPHABET[rng.randint(0, ALPHABET.size, size=rng.randint(0, 41))].copy()
    kw = dict(case_sensitive=cs)
    mode = rng.randint(3)
    if mode == 1:
        kw["count_lines"] = True
    elif mode == 2:
        kw["track_positions"] = False
    if rng.randint(2):
        kw["max_count"] = int(pick(rng, (0, 1, 2)))
    return pats, text, kw


def test_model_equals_the_reference_on_random_patterns_of_the_grammar(eng):
    assert regex_ref.available(), "the compiled reference (oracle/_ref/libkrep_ref_avx2.so) is missing"
    rng = np.random.RandomState(20261020)
    seen = {"lines": 0, "count_only": 0, "positions": 0, "several": 0, "icase": 0, "bol": 0, "eol": 0, "group": 0, "star": 0, "plus": 0,
            "open": 0, "in_group": 0, "optional": 0, "range": 0, "mc0": 0, "mc1": 0, "mc2": 0, "unlimited": 0, "empty_text": 0}
    for _ in range(10000):
        pats, text, kw = random_case(rng)
        eng.regex_compile_loops(abi.Params(pats, regex=True, case_sensitive=kw["case_sensitive"]))  # (raises when it is refused)
        ref = lm.ref_call(pats, text, **kw)
        got = lm.run(pats, text, **kw)
        assert ref[0] == got[0] and np.array_equal(ref[1], got[1]), (pats, kw, text.tobytes(), ref, got)
        whole = b" ".join(pats)
        seen["lines"] += bool(kw.get("count_lines"))
        seen["count_only"] += kw.get("track_positions") is False
        seen["positions"] += not kw.get("count_lines") and kw.get("track_positions") is None
        seen["several"] += len(pats) > 1
        seen["icase"] += not kw["case_sensitive"]
        seen["bol"] += pats[0].startswith(b"^")
        seen["eol"] += pats[0].endswith(b"$")
        seen["group"] += b"(" in whole
        seen["star"] += b"*" in whole
        seen["plus"] += b"+" in whole
        seen["open"] += b",}" in whole
        seen["in_group"] += any(q in part for part in whole.split(b"(")[1:] for q in (b"*", b"+", b",}") if q in part.split(b")")[0])
        seen["optional"] += b"?" in whole
        seen["range"] += b"{1,2}" in whole
        for mc in (0, 1, 2):
            seen["mc%d" % mc] += kw.get("max_count", abi.SIZE_MAX) == mc
        seen["unlimited"] += "max_count" not in kw
        seen["empty_text"] += text.size == 0
    assert all(v > 300 for k, v in seen.items() if k != "empty_text") and seen["empty_text"] > 50, seen


# the patterns the rule was first checked with
FIRST = [[b"a+b"], [b"ab*c"], [b"a.*b"], [b"[ab]+c?"], [b"^a+"], [b"b+$"], [b"a{2,}b"], [b"x(a+|b)y"], [b"a+", b"b+c"]]


@pytest.mark.parametrize("k", range(len(FIRST)))
def test_the_first_patterns(k):
    pats = FIRST[k]
    rng = np.random.RandomState(900 + k)
    alphabet = np.frombuffer(b"aabbcxy\n" if k == 7 else b"aabbc\n", dtype=np.uint8)
    for _ in range(300):
        text = alphabet[rng.randint(0, alphabet.size, size=rng.randint(0, 41))].copy()
        for kw in (dict(), dict(case_sensitive=False), dict(count_lines=True), dict(track_positions=False), dict(max_count=1),
                   dict(max_count=2), dict(max_count=0, track_positions=False), dict(max_count=0)):
            ref = lm.ref_call(pats, text, **kw)
            got = lm.run(pats, text, **kw)
            assert ref[0] == got[0] and np.array_equal(ref[1], got[1]), (pats, kw, text.tobytes(), ref, got)


@pytest.mark.parametrize("pats, text, want", [
    ([b"ERROR.*timeout"], b"ERROR: a timeout, a timeout\nERROR\ntimeout ERROR", [(0, 27)]),       # the longest end, never across a line
    ([b"a+b"], b"aab ab b aaa\nb", [(0, 3), (4, 6)]),
    ([b"ab*c"], b"ac abbbc abb", [(0, 2), (3, 8)]),
    ([b"[0-9]+\\.[0-9]+"], b"v1.25 and 10.0.3", [(1, 5), (10, 14)]),                                # the walk resumes at the end: .3 has no digit in front
    ([b"colou*r"], b"color colour colouuur colo", [(0, 5), (6, 12), (13, 21)]),
    ([b"x(a+|b)y"], b"xaay xby xbby xy", [(0, 4), (5, 8)]),
    ([b"[ab]+c?"], b"abcab c", [(0, 3), (3, 5)]),
    ([b"^a+"], b"aa a\nba\na", [(0, 2), (8, 9)]),
    ([b"b+$"], b"abb\nbb b", [(1, 3), (7, 8)]),
    ([b"a{2,}b"], b"ab aab aaab", [(3, 6), (7, 11)]),
    ([b"a*b"], b"b aab", [(0, 1), (2, 5)]),
])
def test_fixed_cases(pats, text, want):
    t = np.frombuffer(text, dtype=np.uint8)
    ref = lm.ref_call(pats, t)
    got = lm.run(pats, t)
    assert ref[0] == got[0] and ref[1].tolist() == got[1].tolist(), (ref, got)
    assert got[1].tolist() == [list(w) for w in want]
    assert lm.ref_call(pats, t, count_lines=True)[0] == lm.run(pats, t, count_lines=True)[0]


def test_the_end_of_the_text_ends_a_line_in_a_case_sensitive_search_only():
    t = np.frombuffer(b"abb\nabb", dtype=np.uint8)
    for cs, want in ((True, [[1, 3], [5, 7]]), (False, [[1, 3]])):
        ref = lm.ref_call([b"b+$"], t, case_sensitive=cs)
        got = lm.run([b"b+$"], t, case_sensitive=cs)
        assert ref[1].tolist() == got[1].tolist() == want
