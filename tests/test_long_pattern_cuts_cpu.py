"""CPU side of tests/long_pattern_cuts.py (no GPU): the brute-force record list the GPU tests compare against IS the reference's
(aho_corasick_search, aho_corasick.c:299-466, through the compiled reference / its restatement), the sweep plants
every (phrase length, offset to the cut) once — inside the band a stand-in entry can lose and outside it — and no plant was
overwritten by a later one."""
import numpy as np
import pytest

import long_pattern_cuts as lpc
import oracle_lib as ol
from krep_amd import abi


@pytest.fixture(scope="module")
def engine():
    import krep_amd
    return krep_amd.load()


@pytest.fixture(scope="module", params=["every pattern >= 4 bytes", "with 1..3-byte words"])
def case(request, engine):
    return lpc.build(engine, with_short="1..3" in request.param)


def test_phrases_and_dictionaries_have_the_stated_shape(case):
    ph = case.phrases
    assert [len(p) for p in ph] == list(lpc.PHRASE_LENS) + [lpc.TWIN_LEN]
    assert ph[-1][-16:] == ph[2][-16:] and ph[-1][:-16] != ph[2][-lpc.TWIN_LEN:-16]  # two stand-ins in one exact entry
    pats = set(case.patterns)
    for p in ph:
        assert p in pats and b"  " not in p and b"\n" not in p and p == p.strip()
        last = p.split(b" ")[-1]
        assert last in pats and len(last) >= 4  # two patterns at one END, different starts
        assert sum(1 for q in pats if q != p and len(q) <= 16 and q[-4:] == p[-4:]) >= 4  # the trie branches behind the final gram
    short = [q for q in case.patterns if len(q) < 4]
    assert len(short) in (0, 8) and len(case.patterns) - len(short) >= 300 + len(ph)  # (8: what sends the plan down the split road)


def test_every_length_and_offset_is_planted_once_and_survives(case):
    text = bytes(case.text)
    assert len(text) == lpc.TEXT_LEN
    seen = {}
    for q in case.plants:
        assert q.start == q.cut - q.k and lpc.WINDOW <= q.cut <= len(text) - lpc.WINDOW
        assert text[q.start:q.start + q.L] == case.phrases[q.phrase], q  # survived the later plants
        assert text[q.start - 1:q.start] in (b" ", b"\n") and text[q.start + q.L:q.start + q.L + 1] in (b" ", b"\n"), q
        seen[(q.phrase, q.k)] = seen.get((q.phrase, q.k), 0) + 1
    for pi, p in enumerate(case.phrases):
        L = len(p)
        ks = [k for (i, k), n in seen.items() if i == pi and n == 1]
        assert sorted(ks) == list(range(-2, L + 3))
        band = [k for k in ks if lpc.in_band(L, k)]
        assert band == [] or sorted(band) == list(range(1, L - 15))
        assert len(band) == L - 16 and len(ks) - len(band) == 21  # (17: a band of one offset)
        # ... and the text holds the phrase at its plants only
        rec = lpc.brute_force(case.text, [p])
        assert sorted(rec[:, 0].tolist()) == sorted(q.start for q in case.plants if q.phrase == pi)
    cuts = [q.cut for q in case.plants]
    assert len(set(cuts)) == len(cuts)
    kinds = {(c % lpc.UNIT) if c % lpc.UNIT in (0, 1, lpc.UNIT - 1) else "odd" for c in cuts}
    assert kinds == {0, 1, lpc.UNIT - 1, "odd"} and all(c % 2 == 1 for c in cuts if c % lpc.UNIT not in (0, 1, lpc.UNIT - 1))
    for pi in range(len(case.phrases)):  # every phrase meets a cut on a unit boundary inside its band (the twin stands in for none)
        assert any(q.phrase == pi and lpc.in_band(q.L, q.k) and q.cut % lpc.UNIT in (0, 1, lpc.UNIT - 1) for q in case.plants)


@pytest.mark.parametrize("kw", [dict(), dict(case_sensitive=False), dict(whole_word=True)], ids=["plain", "-i", "-w"])
def test_brute_force_is_the_reference(case, kw):
    o = ol.checker()
    pats = [p.upper() for p in case.patterns] if kw.get("case_sensitive") is False else case.patterns
    n, want = o.call(abi.RA_AHO_CORASICK, abi.Params(pats, **kw), case.text)
    got = lpc.brute_force(case.text, pats, **kw)
    if not kw:
        assert np.array_equal(got, case.expected)
    assert n == len(got) and np.array_equal(got, want.astype(np.int64))
    # every plant is a record, under every option (a blank or a newline on either side: a whole word)
    starts = set(map(tuple, got.tolist()))
    assert all((q.start, q.start + q.L) in starts for q in case.plants)


def test_owned_records_partition_the_list(case):
    c = case.plants[len(case.plants) // 2].cut
    lo, hi = lpc.owned(case.expected, c - lpc.WINDOW, c), lpc.owned(case.expected, c, c + lpc.WINDOW)
    both = lpc.owned(case.expected, c - lpc.WINDOW, c + lpc.WINDOW)
    assert len(lo) + len(hi) == len(both) and len(lo) and len(hi)
    key = lambda a: a[np.lexsort((a[:, 0], a[:, 1]))]
    assert np.array_equal(key(np.concatenate([lo, hi])), both)


def test_a_duplicate_word_is_planted_at_every_offset_and_reported_twice(engine):
    cs = lpc.build_duplicate(engine)
    dup = cs.phrases[0]
    assert cs.patterns.count(dup) == 2 and 10 <= len(dup) <= 16
    assert [q.k for q in cs.plants] == list(range(-1, len(dup) + 2))
    raw = bytes(cs.text)
    assert all(raw[q.start:q.start + q.L] == dup for q in cs.plants) and raw.count(dup) == len(cs.plants)
    rec = list(map(tuple, cs.expected.tolist()))
    assert all(rec.count((q.start, q.start + q.L)) == 2 for q in cs.plants)
    n, want = ol.checker().call(abi.RA_AHO_CORASICK, abi.Params(cs.patterns), cs.text)
    assert n == len(cs.expected) and np.array_equal(cs.expected, want.astype(np.int64))


def test_the_frequent_word_dictionary_keeps_the_plants_and_the_reference(engine, case):
    cs = lpc.build(engine, frequent=True)
    assert np.array_equal(cs.text, case.text) and cs.plants == case.plants and cs.phrases == case.phrases
    assert set(cs.patterns[300:]) == set(p for p in case.patterns[300:] if len(p) >= 4) and len(cs.expected) > 50 * len(cs.plants)
    n, want = ol.checker().call(abi.RA_AHO_CORASICK, abi.Params(cs.patterns), cs.text)
    assert n == len(cs.expected) and np.array_equal(cs.expected, want.astype(np.int64))
