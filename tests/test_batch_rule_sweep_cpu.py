"""The batch rule over its whole matrix (kg::batch_unsupported_reason).  Host logic only, no GPU.

tests/test_batch_separable_cpu.py asks the reference about 28 named classes.  The rule decides over build level x --algo override x
force_no_simd x -o x -w x -i x -c x pattern length x self-overlap; here EVERY cell of that matrix is asked: a refused cell names a
reason that file pins (and a single text is still taken), a taken cell is newline-separable on random pairs according to the
reference itself.  Cells that reach the same reference function with the same pattern and flags are one computation and are
checked once.  The same for random dictionaries and for expressions drawn from a small grammar, and the property the batch's own
-c derivation rests on: the reference's -c count is the number of distinct lines among the starts of its record list.

PAIRS = 25 random pairs per distinct literal class (items of 0..200 bytes): the whole module stays under two minutes."""
import zlib

import numpy as np
import pytest

import batch_model as bm
import oracle_lib as ol
import regex_ref
from krep_amd import abi
from test_batch_separable_cpu import REFUSED

PAIRS = 25
LENGTHS = [1, 2, 3, 4, 5, 8, 15, 16, 17, 20, 31, 32, 33, 40, 64, 65]
LEVELS = [abi.REF_SCALAR, abi.REF_SSE42, abi.REF_AVX2, abi.REF_AVX512, abi.REF_NEON]
OVERRIDES = [abi.ALGO_AUTO, abi.ALGO_BM, abi.ALGO_KMP]
REASONS = sorted({r for _, r in REFUSED if r}, key=len, reverse=True)  # (the longest first: one reason is a part of another)
# ... those a single literal without a newline and without max_count can meet
LITERAL_REASONS = sorted({r for s, r in REFUSED if r and not s.regex and len(s.pats) == 1 and b"\n" not in s.pats[0]
                          and "max_count" not in s.kw})


def shapes(m):
    """border-free abbb.., periodic abab.., first byte == last byte ab..ba, one repeated byte"""
    return [b"a" + b"b" * (m - 1), (b"ab" * m)[:m], (b"a" + b"b" * (m - 2) + b"a")[:m] if m > 1 else b"a", b"a" * m]


def border(p):
    return next((b for b in range(len(p) - 1, 0, -1) if p[:b] == p[len(p) - b:]), 0)


def pinned(why):
    return next((r for r in REASONS if r in why), None)


def seed_of(*key):
    return zlib.crc32(repr(key).encode()) & 0x7FFFFFFF


def length(rng, hi):
    return 0 if rng.randint(10) == 0 else int(rng.randint(0, hi + 1))


@pytest.fixture(autouse=True, scope="module")
def _c_locale():
    with regex_ref.c_locale():
        yield


@pytest.fixture(scope="module")
def eng():
    import krep_amd
    mp = pytest.MonkeyPatch()
    mp.setenv("KREP_GPU_ASSUME_AVAILABLE", "1")  # (as tests/test_batch_separable_cpu.py: the rule is host logic)
    mp.delenv("KREP_GPU_DISABLE", raising=False)
    e = krep_amd.load()
    yield e
    e.set_thread_config(None)
    mp.undo()


def verdicts(eng, s):
    """-> (batch taken, its reason, single text taken) under the search's configuration"""
    s.configure(eng)
    try:
        p = s.params()
        ok = eng.batch_can_accelerate(p)
        why = eng.last_error()
        return ok, why, eng.can_accelerate(p)
    finally:
        eng.set_thread_config(None)


def literal_search(pat, level, override, nosimd, cs, ww, om, lines):
    ov = border(pat)
    alphabet = b"ab \n" + (b"" if cs else b"AB") + (b"_-" if ww else b"")
    kw = dict(case_sensitive=cs, whole_word=ww)
    if lines:
        kw["count_lines"] = True
    return bm.Search("%s L%d o%d n%d cs%d w%d o%d c%d" % (pat.decode(), level, override, nosimd, cs, ww, om, lines), [pat], level=level,
                     only_matching=om, algo_override=override, force_no_simd=nosimd, alphabet=alphabet,
                     plants=[pat, pat + pat[ov:], b" " + pat + b" "], **kw)


@pytest.fixture(scope="module")
def literal_matrix(eng):
    """every cell asked once -> (cells, taken cells, {class key: the first taken Search of the class}, {reason: refused cells})"""
    cells = taken = 0
    classes, produced = {}, {}
    for m in LENGTHS:
        for pat in shapes(m):  # (the four shapes of one byte are one pattern: the cell is counted four times, checked once)
            for flags in range(16):
                cs, ww, om, lines = bool(flags & 1), bool(flags & 2), bool(flags & 4), bool(flags & 8)
                for level in LEVELS:
                    for override in OVERRIDES:
                        for nosimd in (False, True):
                            s = literal_search(pat, level, override, nosimd, cs, ww, om, lines)
                            ok, why, single = verdicts(eng, s)
                            cells += 1
                            if not ok:
                                r = pinned(why)
                                assert r is not None and r in LITERAL_REASONS, (s, why)
                                assert single, (s, "refused for a single text as well")
                                produced[r] = produced.get(r, 0) + 1
                                continue
                            taken += 1
                            s.configure(eng)
                            try:
                                algo = eng.mirror_select(s.params(), 1 << 20)
                            finally:
                                eng.set_thread_config(None)
                            classes.setdefault((algo, pat, cs, ww, om, lines), s)
    return cells, taken, classes, produced


def test_the_literal_matrix_is_the_whole_matrix(literal_matrix):
    cells, taken, classes, produced = literal_matrix
    print("literal cells %d, taken %d (%.1f %%), distinct classes %d, refused by reason %r" % (cells, taken, 100.0 * taken / cells, len(classes), produced))
    assert cells == 16 * 4 * 16 * 5 * 3 * 2 == 30720
    assert taken >= 0.95 * cells, (taken, cells)
    # every reason a literal cell can be refused for is met: a rule that stops refusing a class does not pass by leaving the matrix
    assert sorted(produced) == LITERAL_REASONS, (produced, LITERAL_REASONS)
    assert len(classes) > 500


def test_every_taken_literal_class_is_separable(eng, literal_matrix):
    _, _, classes, _ = literal_matrix
    for key, s in classes.items():
        rng = np.random.RandomState(seed_of("literal", key))
        for k in range(PAIRS):
            A, B = bm.random_item(rng, s, length(rng, 200)), bm.random_item(rng, s, length(rng, 200))
            assert bm.separable(eng, s, A, B), (s, key, k, A.tobytes(), B.tobytes())
    assert ol.checker().restatement_budget_ok()


def distinct_lines(text, records):
    """the number of distinct lines among the record starts: what the batch derives an item's -c count from"""
    nl = np.nonzero(bm.as_array(text) == 10)[0]
    return np.unique(np.searchsorted(nl, records.reshape(-1, 2)[:, 0].astype(np.int64), side="left")).size


def plain(s):
    """the same search without count_lines: the one whose record list the batch cuts under -c"""
    kw = {k: v for k, v in s.kw.items() if k != "count_lines"}
    return bm.Search(s.name + " (records)", s.pats, s.level, s.only_matching, s.regex, s.alphabet, s.plants, s.algo_override,
                     s.force_no_simd, **kw)


def test_the_count_under_c_is_the_distinct_lines_of_the_record_starts(eng, literal_matrix):
    """krep_gpu_search_batch scans every pack for RECORDS and derives -c from them (batch_line_flags + the prefix sum): exact iff the
    reference's -c count is the number of distinct lines its own record list starts on — and, on a pack, iff that number adds up"""
    _, _, classes, _ = literal_matrix
    checked = 0
    for key, s in classes.items():
        if not key[5]:
            continue
        rec = plain(s)
        rng = np.random.RandomState(seed_of("lines", key))
        for k in range(PAIRS):
            A, B = bm.random_item(rng, s, length(rng, 400)), bm.random_item(rng, s, length(rng, 400))
            P = bm.pack([A, B])[0]
            n = {}
            for name, T in (("A", A), ("B", B), ("pack", P)):
                n[name] = distinct_lines(T, bm.reference(eng, rec, T)[1])
                if name != "pack":  # (25 texts: A; B is the second item of the pack and is checked on the way)
                    assert bm.reference(eng, s, T)[0] == n[name], (s, key, k, name, T.tobytes())
            assert n["pack"] == n["A"] + n["B"], (s, key, k, A.tobytes(), B.tobytes())
        checked += 1
    assert checked > 100
    assert ol.checker().restatement_budget_ok()


def test_max_count_is_refused_and_the_refusal_is_needed(eng):
    """the source names max_count as follow-up work: until an item's list is cut per item, every cell with a max_count is refused"""
    for level in LEVELS:
        for override in OVERRIDES:
            for pat in (b"ab", b"abab", b"a" * 20, b"ab" * 20):
                for mc in (0, 1, 5):
                    for kw in ({}, dict(count_lines=True), dict(whole_word=True), dict(case_sensitive=False)):
                        s = bm.Search("max_count", [pat], level=level, algo_override=override, max_count=mc, **kw)
                        ok, why, _ = verdicts(eng, s)
                        assert not ok and pinned(why) == "max_count", (s, level, override, pat, mc, kw, why)
    dic = bm.Search("max_count, dictionary", [b"ab", b"ba"], max_count=1)
    ok, why, _ = verdicts(eng, dic)
    assert not ok and pinned(why) == "max_count"
    # what a pack would get wrong: the limit is one for the whole text, two items alone reach it twice
    one = bm.Search("max_count 1", [b"ab"], max_count=1)
    assert bm.reference(eng, one, b"ab")[0] == 1 and bm.reference(eng, one, b"ab\nab")[0] == 1
    assert not bm.separable(eng, one, b"ab", b"ab")
    assert not bm.separable(eng, dic, b"ab", b"ba")


DICT_SIZES, DICT_LENGTHS, DICT_ALPHABETS = [2, 3, 5, 9, 30], [1, 2, 3, 4, 5, 8, 17, 24], [b"ab", b"abc", b"abAB", b"ab_ "]


def test_random_dictionaries(eng):
    rng = np.random.RandomState(20261019)
    taken = 0
    for d in range(300):
        alpha = np.frombuffer(DICT_ALPHABETS[rng.randint(len(DICT_ALPHABETS))], dtype=np.uint8)
        pats = [alpha[rng.randint(0, alpha.size, size=DICT_LENGTHS[rng.randint(len(DICT_LENGTHS))])].tobytes()
                for _ in range(DICT_SIZES[rng.randint(len(DICT_SIZES))])]
        kw = dict(case_sensitive=bool(rng.randint(2)), whole_word=bool(rng.randint(2)))
        if rng.randint(2):
            kw["count_lines"] = True
        s = bm.Search("dictionary %d" % d, pats, alphabet=alpha.tobytes() + b"\n", plants=pats[:4], **kw)
        ok, why, _ = verdicts(eng, s)
        if not ok:
            assert pinned(why) is not None, (s, pats, kw, why)
            continue
        taken += 1
        for k in range(40):
            A, B = bm.random_item(rng, s, length(rng, 60)), bm.random_item(rng, s, length(rng, 60))
            assert bm.separable(eng, s, A, B), (s, pats, kw, k, A.tobytes(), B.tobytes())
    print("dictionaries 300, taken %d" % taken)
    assert taken >= 200
    assert ol.checker().restatement_budget_ok()


ATOMS = [b"a", b"b", b"c", b"[ab]", b"[^a]", b".", b"[a-c]", b"[[:alpha:]]", b"[^[:space:]]", b"[ a]", b"\\."]
SUFFIXES = [b"", b"", b"", b"?", b"{2}", b"{1,2}", b"{0,1}"]


def expression(rng):
    def seq(lo=1, hi=3):
        return b"".join(ATOMS[rng.randint(len(ATOMS))] + SUFFIXES[rng.randint(len(SUFFIXES))] for _ in range(rng.randint(lo, hi + 1)))

    def alt():
        return b"|".join(seq(1, 2) for _ in range(rng.randint(2, 4)))

    shape = rng.randint(3)
    body = seq(1, 4) if shape == 0 else alt() if shape == 1 else seq(0, 2) + b"(" + alt() + b")" + seq(0, 2)
    anchor = rng.randint(8)
    if anchor == 3:
        return b"^" + body
    if anchor == 4:
        return body + b"$"
    if anchor == 5:
        return b"^" + body + b"$"
    if anchor == 6:
        return b"^(" + body + b")$"
    if anchor == 7:  # anchored branches
        return b"|".join((b"^" if rng.randint(2) else b"") + seq(1, 2) + (b"$" if rng.randint(2) else b"") for _ in range(rng.randint(2, 4)))
    return body


def test_generated_expressions(eng):
    rng = np.random.RandomState(20261020)
    made = taken = 0
    while made < 1500:
        pat = expression(rng)
        kw = dict(case_sensitive=bool(rng.randint(2)))
        if rng.randint(2):
            kw["count_lines"] = True
        try:
            regex_ref.Compiled(pat, kw["case_sensitive"])
        except ValueError:
            continue  # regcomp rejects it
        made += 1
        s = bm.Search(pat.decode(), [pat], regex=True, alphabet=b"abcAB .\n", **kw)
        ok, why, _ = verdicts(eng, s)
        if not ok:
            assert why, s
            continue
        taken += 1
        for k in range(40):
            A, B = bm.random_item(rng, s, length(rng, 12)), bm.random_item(rng, s, length(rng, 12))
            assert bm.separable(eng, s, A, B), (s, kw, k, A.tobytes(), B.tobytes())
    print("expressions %d, taken %d (%.1f %%)" % (made, taken, 100.0 * taken / made))
    assert taken >= 0.25 * made, (taken, made)
