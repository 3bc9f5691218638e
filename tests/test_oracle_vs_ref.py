"""Differential pin of the oracle restatement against the UNMODIFIED reference compiled into
oracle/_ref (count, result->count and every offset, in order).  oracle/Makefile builds _ref only where the reference's
sources are present; elsewhere the reference's answers recorded in tests/golden/ref_answers.json stand in for it
(oracle_lib.RefAnswers)."""
import random

import numpy as np
import pytest

import oracle_lib as ol
from krep_amd import abi

LEVELS = [abi.REF_SCALAR, abi.REF_SSE42, abi.REF_AVX2, abi.REF_AVX512, abi.REF_NEON]
ALPHAS = [b"ab", b"ab\n", b"abAB \n", b"abc_ \n-", bytes(range(97, 123)) + b" \n"]
SIZES = [0, 1, 2, 3, 5, 8, 15, 16, 17, 31, 32, 33, 40, 63, 64, 65, 70, 100, 127, 128, 129, 200, 300, 1000]


REC = ol.RefAnswers("test_oracle_vs_ref")


def _answer(engine, algo, pats, kw, text):
    ret, pos = engine.call(algo, abi.Params(pats, **kw), text)
    return ol.answer_digest(ret, pos)


def _case(rng):
    alpha = rng.choice(ALPHAS)
    n = rng.choice(SIZES)
    text = bytes(rng.choice(alpha) for _ in range(n))
    algo = rng.choice([abi.RA_BMH, abi.RA_KMP, abi.RA_MEMCHR, abi.RA_MEMCHR_SHORT, abi.RA_SSE42,
                       abi.RA_AVX2, abi.RA_AVX512, abi.RA_NEON, abi.RA_AHO_CORASICK])
    m = {abi.RA_MEMCHR: [1], abi.RA_MEMCHR_SHORT: [2, 3], abi.RA_AVX2: [2, 5, 16, 17, 18, 20, 32],
         abi.RA_AVX512: [3, 17, 33, 34, 40, 64], abi.RA_NEON: [1, 2, 3, 4, 5, 8, 9, 15, 16, 17, 20]}.get(algo, [1, 2, 3, 4, 5, 8, 9, 16])
    m = rng.choice(m)

    def mk(k):
        if n >= k and rng.random() < 0.7:
            s = rng.randrange(0, n - k + 1)
            return text[s:s + k]
        return bytes(rng.choice(alpha) for _ in range(k))

    kw = dict(case_sensitive=rng.random() < 0.6, whole_word=rng.random() < 0.3,
              max_count=rng.choice([abi.SIZE_MAX] * 3 + [0, 1, 2, 3, 5]))
    mode = rng.choice(["pos", "lines", "count"])
    if mode == "lines":
        kw.update(count_lines=True)
    elif mode == "count":
        kw.update(count_lines=True, only_match=True)
    if algo == abi.RA_AHO_CORASICK:
        pats = [mk(rng.choice([1, 2, 3, 4, 6])) for _ in range(rng.choice([2, 3, 5, 8]))]
    else:
        pats = [mk(m)]
    return algo, pats, kw, text


@pytest.mark.parametrize("seed", range(8))
def test_oracle_equals_reference(seed):
    rng = random.Random(1000 + seed)
    o = ol.oracle()
    refs = [ol.ref(l) for l in LEVELS if ol.ref_available(l)]
    checked = 0
    for i in range(500):
        algo, pats, kw, text = _case(rng)
        live = []
        for r in refs:
            if not r.has(algo):
                continue
            a = r.call(algo, abi.Params(pats, **kw), text)
            b = o.call(algo, abi.Params(pats, **kw), text)
            assert a[0] == b[0] and np.array_equal(a[1], b[1]), (r.name, abi.RA_NAMES[algo], pats, kw, text)
            live.append(ol.answer_digest(*a))
        want, builds = REC.want(f"equals/{seed}/{i}", live)
        assert _answer(o, algo, pats, kw, text) == want, (abi.RA_NAMES[algo], pats, kw, text)
        checked += builds
    REC.save()
    assert checked > 500


def test_memchr_batch_boundary_quirk():
    """max_count == 4096 with more matches: the reference stores the 4097th match FIRST
    (krep.c:3976-3991 + :4026-4038).  The restatement must reproduce the same list."""
    r = ol.ref(abi.REF_SCALAR) or ol.ref(abi.REF_AVX2)
    o = ol.oracle()
    text = (b"x#" * 5000)
    for mc in (4095, 4096, 4097, 8192, 100):
        b = o.call(abi.RA_MEMCHR, abi.Params([b"#"], max_count=mc), text)
        live = []
        if r is not None:
            a = r.call(abi.RA_MEMCHR, abi.Params([b"#"], max_count=mc), text)
            assert a[0] == b[0] and np.array_equal(a[1], b[1]), mc
            live.append(ol.answer_digest(*a))
        assert ol.answer_digest(*b) == REC.want(f"memchr_batch/{mc}", live)[0], mc
    REC.save()
    b = o.call(abi.RA_MEMCHR, abi.Params([b"#"], max_count=4096), text)  # == the reference's list (above)
    assert b[1][0, 0] == 2 * 4096 + 1  # the out-of-order record


def test_select_mirror_matches_reference():
    rng = random.Random(7)
    o = ol.oracle()
    pats = [b"a", b"ab", b"abc", b"abab", b"aaaa", b"abcabc", b"Sherlock", b"x" * 16, b"y" * 17,
            b"z" * 32, b"q" * 33, b"w" * 64, b"e" * 65, b"abcdefg", b"aabaab", b"ababab"]
    for lvl in LEVELS:
        r = ol.ref(lvl)
        for pat in pats:
            for cs in (True, False):
                p = abi.Params([pat], case_sensitive=cs)
                live = [ol.answer_digest(r.select(p))] if r is not None else []
                assert ol.answer_digest(o.select(p, lvl)) == REC.want(f"select/{lvl}/{pat.decode()}/{int(cs)}", live)[0], (lvl, pat, cs)
        p = abi.Params([b"ab", b"cd"])
        if r is not None:
            assert r.select(p) == abi.RA_AHO_CORASICK
        assert o.select(p, lvl) == abi.RA_AHO_CORASICK
    REC.save()


def test_larger_random_texts():
    rng = np.random.RandomState(5)
    o = ol.oracle()
    text = rng.choice(np.frombuffer(b"abc \n", dtype=np.uint8), size=300_000).astype(np.uint8)
    for lvl in LEVELS:
        r = ol.ref(lvl)
        has = r.has if r is not None else ol.RefEngine.exports(lvl).__contains__
        for algo, pat in ((abi.RA_BMH, b"abc a"), (abi.RA_MEMCHR, b"\n"), (abi.RA_MEMCHR_SHORT, b"ab"),
                          (abi.RA_KMP, b"aab"), (abi.RA_SSE42, b"abab"), (abi.RA_AVX2, b"abc abc abc abc abc"),
                          (abi.RA_AHO_CORASICK, None)):
            if not has(algo):
                continue
            pats = [pat] if pat else [b"ab", b"abc", b"c a", b"bcab", b"a"]
            for ki, kw in enumerate((dict(), dict(count_lines=True), dict(whole_word=True), dict(case_sensitive=False, max_count=1000))):
                b = o.call(algo, abi.Params(pats, **kw), text)
                live = []
                if r is not None:
                    a = r.call(algo, abi.Params(pats, **kw), text)
                    assert a[0] == b[0] and np.array_equal(a[1], b[1]), (r.name, abi.RA_NAMES[algo], kw)
                    live.append(ol.answer_digest(*a))
                assert ol.answer_digest(*b) == REC.want(f"larger/{lvl}/{abi.RA_NAMES[algo]}/{ki}", live)[0], (lvl, abi.RA_NAMES[algo], kw)
    REC.save()
