"""tests/regex_ext_model.py against the compiled reference's regex_search: the rule the device scan reproduces for what
krep_gpu_regex_compile_ext() expands (?, {n}, {n,m}, inner groups, one pair of line anchors around every top-level branch): the
longest occurring sequence at a position, greedy non-overlapping selection, anchors that consume nothing, -c by the starts' lines."""
import numpy as np
import pytest

import regex_ext_model as em
import regex_ref
from krep_amd import abi


@pytest.fixture(autouse=True, scope="module")
def _c_locale():
    with regex_ref.c_locale():
        yield


ATOMS = [b"a", b"b", b"c", b".", b"[ab]", b"[^a]", b"[a\n]", b"[[:space:]]", b"\n", b"\\."]
QUANTS = [b"", b"", b"", b"?", b"{2}", b"{1,2}", b"{0,2}", b"{1,3}", b"{2,3}"]
ALPHABETS = [np.frombuffer(a, dtype=np.uint8) for a in (b"aabbc.\n \x00\xe9", b"ab\n", b"abc\n\n", b"aAbB.\n")]


def pick(rng, seq):
    return seq[rng.randint(len(seq))]


def random_seq(rng, lo, hi):
    return b"".join(pick(rng, ATOMS) + pick(rng, QUANTS) for _ in range(rng.randint(lo, hi + 1)))


def random_branch(rng):
    items = []
    for _ in range(rng.randint(1, 4)):
        if rng.randint(3) == 0:
            items.append(b"(" + b"|".join(random_seq(rng, 1, 2) for _ in range(rng.randint(1, 4))) + b")" + pick(rng, QUANTS))
        else:
            items.append(pick(rng, ATOMS) + pick(rng, QUANTS))
    return b"".join(items)


def random_case(rng):
    while True:
        bol, eol = (b"^" if rng.randint(3) == 0 else b""), (b"$" if rng.randint(3) == 0 else b"")
        brs = [bol + random_branch(rng) + eol for _ in range(rng.randint(1, 4))]
        k = rng.randint(1, len(brs) + 1)
        pats = [b"|".join(brs[:k])] + brs[k:]  # several patterns, as the CLI joins them, every now and then
        try:
            if all(len(s) for s in em.expand(pats)[2]):  # (a sequence without a class matches the empty string: not this rule's)
                break
        except OverflowError:  # (wider than the model expands)
            pass
    text = pick(rng, ALPHABETS)
    text = text[rng.randint(0, text.size, size=rng.randint(1, 50))].copy()
    kw = dict(case_sensitive=bool(rng.randint(3)))
    mode = rng.randint(3)
    if mode == 1:
        kw["count_lines"] = True
    elif mode == 2:
        kw["track_positions"] = False
    if rng.randint(2):
        kw["max_count"] = int(pick(rng, (0, 1, 5)))
    return pats, text, kw


def test_model_equals_the_reference_on_random_patterns_of_the_grammar():
    assert regex_ref.available(), "the compiled reference (oracle/_ref/libkrep_ref_avx2.so) is missing"
    rng = np.random.RandomState(20261020)
    seen = {"lines": 0, "count_only": 0, "several": 0, "icase": 0, "bol": 0, "eol": 0, "group": 0, "optional": 0, "range": 0,
            "mc0": 0, "mc1": 0, "mc5": 0}
    for _ in range(10000):
        pats, text, kw = random_case(rng)
        ref = em.ref_call(pats, text, **kw)
        got = em.run(pats, text, **kw)
        assert ref[0] == got[0] and np.array_equal(ref[1], got[1]), (pats, kw, text.tobytes(), ref, got)
        whole = b" ".join(pats)
        seen["lines"] += bool(kw.get("count_lines"))
        seen["count_only"] += kw.get("track_positions") is False
        seen["several"] += len(pats) > 1
        seen["icase"] += not kw["case_sensitive"]
        seen["bol"] += pats[0].startswith(b"^")
        seen["eol"] += pats[0].endswith(b"$")
        seen["group"] += b"(" in whole
        seen["optional"] += b"?" in whole
        seen["range"] += b"," in whole
        for mc in (0, 1, 5):
            seen["mc%d" % mc] += kw.get("max_count", abi.SIZE_MAX) == mc
    assert all(v > 500 for v in seen.values()), seen


# the eight patterns the rule was first checked with
FIRST = [[b"colou?r"], [b"^(ab|a)c?$"], [b"x(a|bc)y"], [b"[ab]{1,3}c"], [b"(a|ab)(c|bcd)?"], [b"^(a|b\n)b"], [b"(a|b)[ab\n]?$"],
         [b"(ab){2}|b{0,2}a"]]


@pytest.mark.parametrize("k", range(len(FIRST)))
def test_the_first_eight_patterns(k):
    pats = FIRST[k]
    rng = np.random.RandomState(700 + k)
    alphabet = np.frombuffer(b"abcdxy\n" if k in (1, 2, 3, 4, 5, 6, 7) else b"colur \n", dtype=np.uint8)
    for _ in range(300):
        text = alphabet[rng.randint(0, alphabet.size, size=rng.randint(1, 40))].copy()
        for kw in (dict(), dict(case_sensitive=False), dict(count_lines=True), dict(track_positions=False), dict(max_count=1),
                   dict(max_count=0, track_positions=False)):
            ref = em.ref_call(pats, text, **kw)
            got = em.run(pats, text, **kw)
            assert ref[0] == got[0] and np.array_equal(ref[1], got[1]), (pats, kw, text.tobytes(), ref, got)


@pytest.mark.parametrize("pats, text, want", [
    ([b"colou?r"], b"color colour colouur", [(0, 5), (6, 12)]),
    ([b"x(a|bc)y"], b"xay xbcy xby", [(0, 3), (4, 8)]),
    ([b"[ab]{1,3}c"], b"ababc", [(1, 5)]),                       # the leftmost start that holds an occurrence, its longest length
    ([b"^(ab|a)c?$"], b"ab\nac\na\nabc\nxab", [(0, 2), (3, 5), (6, 7), (8, 11)]),
    ([b"(a|ab)(c|bcd)?"], b"abcd", [(0, 4)]),                    # the longest sequence at the position: a + bcd
    ([b"^GET", b"^POST"], b"GET\nxGET\nPOST", [(0, 3), (9, 13)]),
])
def test_fixed_cases(pats, text, want):
    t = np.frombuffer(text, dtype=np.uint8)
    ref = em.ref_call(pats, t)
    got = em.run(pats, t)
    assert ref[0] == got[0] and ref[1].tolist() == got[1].tolist(), (ref, got)
    assert got[1].tolist() == [list(w) for w in want]
    assert em.ref_call(pats, t, count_lines=True)[0] == em.run(pats, t, count_lines=True)[0]


def test_the_end_of_the_text_ends_a_line_in_a_case_sensitive_search_only():
    t = np.frombuffer(b"foo\nquux", dtype=np.uint8)
    for cs, want in ((True, [[0, 3], [4, 8]]), (False, [[0, 3]])):
        ref = em.ref_call([b"(foo|quux)$"], t, case_sensitive=cs)
        got = em.run([b"(foo|quux)$"], t, case_sensitive=cs)
        assert ref[1].tolist() == got[1].tolist() == want
