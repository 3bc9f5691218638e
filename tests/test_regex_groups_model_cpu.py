"""tests/regex_groups_model.py against the compiled reference's regex_search: the per-line rule the device scan reproduces for what
krep_gpu_regex_compile_groups() takes (repeated and nested groups): lines are independent, the leftmost start of a line that has a
match, its longest end over ALL paths of the position automaton, the walk resumes at that end."""
import numpy as np
import pytest

import regex_groups_model as gm
import regex_ref
from krep_amd import abi

IP = rb"[0-9]{1,3}\.[0-9]{1,3}\.[0-9]{1,3}\.[0-9]{1,3}"
# (patterns, what the random texts are drawn from: the bytes of an alphabet, or a list of units)
NAMED = [
    ([b"(ab)+"], b"aabbc\n"), ([b"(a|b)*c"], b"aabbc\n"), ([b"(a|bc)+d"], b"abcd\n"), ([b"((ab)+c)+d"], [b"ab", b"c", b"d", b"abc", b"\n", b"a"]),
    ([b"(a|ab)(c|bcd)"], b"abcd\n"), ([b"(a|ab|abc)+c"], b"abc\n"), ([b"x(ab|a)*bc"], b"xaabbc\n"), ([b"(a+|b)+c"], b"aabbc\n"),
    ([b"((a|b)c|d)+e"], b"abccde\n"), ([b"(ab){2,}"], b"aabb\n"), ([b"(foo|bar){2,3};"], [b"foo", b"bar", b";", b"fo", b"\n", b"barfoo;"]), 
    ([rb"([a-z]+\.)+com"], [b"ab.", b"com", b".", b"c", b"\n", b"x.y.com"]),
    ([b"^(ab)+"], b"aabbc\n"), ([b"(ab)+$"], b"aabbc\n"), ([b"^((GET|POST) |HEAD )/api"], 
     [b"GET /api", b"POST /api", b"\nHEAD /api", b"\n", b"GET", b" /ap", b"HEAD /api", b"\nPOST "]), 
    ([b"(a|b)(c|d)(e|f)(g|h)"], [b"aceg", b"bdfh", b"a", b"c", b"\n", b"adeh", b"g", b"bc"]),
    
    ([IP], [b"1", b"23", b".", b"1.2.3.4", b" ", b"\n", b"1234.5.67.890"]), ([b"(ab)+", b"c(d|e)*f"], b"abcdef\n"),
]
MODES = (dict(), dict(track_positions=False), dict(count_lines=True), dict(case_sensitive=False), dict(max_count=0), dict(max_count=1),
         dict(max_count=3), dict(max_count=0, track_positions=False), dict(case_sensitive=False, count_lines=True))


@pytest.fixture(autouse=True, scope="module")
def _c_locale():
    with regex_ref.c_locale():
        yield


def named_text(rng, k, alphabet):
    """a short random text"""
    if isinstance(alphabet, bytes):
        a = np.frombuffer(alphabet, dtype=np.uint8)
        return a[rng.randint(0, a.size, size=rng.randint(0, 41))].copy()
    units = alphabet
    return np.frombuffer(b"".join(units[rng.randint(len(units))] for _ in range(rng.randint(0, 9))), dtype=np.uint8).copy()


def agree(pats, text, kw):
    ref = gm.ref_call(pats, text, **kw)
    got = gm.run(pats, text, **kw)
    assert ref[0] == got[0] and np.array_equal(ref[1], got[1]), (pats, kw, text.tobytes(), ref, got)
    return ref


@pytest.mark.parametrize("k", range(len(NAMED)))
def test_the_named_expressions(k):
    assert regex_ref.available(), "the compiled reference (oracle/_ref/libkrep_ref_avx2.so) is missing"
    pats, alphabet = NAMED[k]
    rng = np.random.RandomState(7100 + k)
    found = 0
    for _ in range(150):
        text = named_text(rng, k, alphabet)
        for kw in MODES:
            found += agree(pats, text, kw)[0]
    assert found > 50, (pats, found)


def test_dollar_at_a_text_end_without_newline():
    t = np.frombuffer(b"abab\nxabab", dtype=np.uint8)
    for cs, want in ((True, [[0, 4], [6, 10]]), (False, [[0, 4]])):
        assert agree([b"(ab)+$"], t, dict(case_sensitive=cs))[1].tolist() == want
    assert agree([b"(ab)+$"], t, dict(case_sensitive=False, count_lines=True))[0] == 1


LETTERS = [b"a", b"a", b"b", b"b", b"c", b"[ab]", b"."]
QUANTS = [b"", b"", b"", b"", b"+", b"*", b"?", b"{2}", b"{1,2}", b"{2,}"]
ALPHABET = np.frombuffer(b"aaabbbc\n", dtype=np.uint8)


def pick(rng, seq):
    return seq[rng.randint(len(seq))]


def random_expr(rng, depth, budget):
    """an alternation of sequences of atoms and groups, groups to `depth`; budget[0]: the atoms that may still be written"""
    alts = []
    for _ in range(rng.randint(1, 3 if depth else 2)):
        items = []
        for _ in range(rng.randint(1, 4)):
            if budget[0] <= 0:
                break
            if depth and rng.randint(3) == 0:
                items.append(b"(" + random_expr(rng, depth - 1, budget) + b")" + pick(rng, QUANTS))
            else:
                budget[0] -= 1
                items.append(pick(rng, LETTERS) + pick(rng, QUANTS[:7]))
        if not items:
            budget[0] -= 1
            items.append(pick(rng, LETTERS[:5]))
        alts.append(b"".join(items))
    return b"|".join(alts)


def random_groups_case(rng):
    """an expression of the grammar with at least one group (depth <= 3, <= 12 atoms) that the model's own parser admits"""
    while True:
        body = b"(" + random_expr(rng, 2, [10]) + b")" + pick(rng, QUANTS) + (pick(rng, LETTERS[:5]) if rng.randint(2) else b"")
        if rng.randint(3) == 0:
            body = pick(rng, LETTERS[:5]) + body
        pats = [(b"^" if rng.randint(6) == 0 else b"") + body + (b"$" if rng.randint(6) == 0 else b"")]
        cs = bool(rng.randint(4))
        try:
            au = gm.automaton(pats, cs)
        except gm.Refused:
            continue
        if len(au.atoms) <= 12:
            return pats, cs


def test_model_equals_the_reference_on_random_expressions_of_the_grammar():
    assert regex_ref.available(), "the compiled reference (oracle/_ref/libkrep_ref_avx2.so) is missing"
    rng = np.random.RandomState(20261021)
    seen = {"nested": 0, "loop_on_group": 0, "icase": 0, "anchored": 0, "found": 0}
    for _ in range(400):
        pats, cs = random_groups_case(rng)
        whole = pats[0]
        seen["nested"] += b"((" in whole or whole.count(b"(") > 1
        seen["loop_on_group"] += any(q in whole for q in (b")+", b")*", b"){2,}"))
        seen["icase"] += not cs
        seen["anchored"] += whole.startswith(b"^") or whole.endswith(b"$")
        for _ in range(6):
            text = ALPHABET[rng.randint(0, ALPHABET.size, size=rng.randint(0, 31))].copy()
            kw = dict(case_sensitive=cs)
            mode = rng.randint(4)
            if mode == 1:
                kw["count_lines"] = True
            elif mode == 2:
                kw["track_positions"] = False
            if rng.randint(2):
                kw["max_count"] = int(pick(rng, (0, 1, 3)))
            seen["found"] += agree(pats, text, kw)[0] > 0
    assert seen["nested"] > 100 and seen["loop_on_group"] > 100 and seen["icase"] > 50 and seen["anchored"] > 50 and seen["found"] > 500, seen
