"""When is a batch of texts one text?  (krep_gpu_batch_can_accelerate, include/krep_gpu.h "a batch of texts in one scan")

krep_gpu_search_batch packs its items with one '\\n' between neighbours and scans the pack once.  That is exact iff the search is
newline-separable: result(A + '\\n' + B) = result(A), then result(B) shifted by |A| + 1.  Host logic only, no GPU: for every class
the library TAKES the reference itself (tests/batch_model.py: the compiled reference, the restatement under -o) is separable on
random pairs; for every class it REFUSES the reason is pinned, and for five of them a concrete (A, B) shows the refusal is needed."""
import numpy as np
import pytest

import batch_model as bm
import regex_ref
from krep_amd import abi

PAIRS = 200  # random (A, B) per class, lengths 0..300

WORDS = [b"a", b"b", b"ab", b"ba", b"aa", b"bb", b"aab", b"aba", b"abb", b"baa", b"bab", b"bba", b"aaa", b"bbb", b"abab", b"baba",
         b"aabb", b"bbaa", b"abba", b"baab"]

S = bm.Search
TAKEN = [
    S("border-free literal", [b"aab"], alphabet=b"ab\n", plants=[b"aab"]),
    S("border-free literal, 8 bytes", [b"Sherlock"], alphabet=bytes(range(97, 123)) + b"  \n", plants=[b"Sherlock"]),
    S("bordered literal: simd_sse42_search greedy", [b"abab"], alphabet=b"ab\n", plants=[b"ababab"]),
    S("bordered literal: kmp_search greedy", [b"abab"], level=abi.REF_SCALAR, alphabet=b"ab\n", plants=[b"ababab"]),
    S("boyer_moore_search", [b"aXbY"], level=abi.REF_SCALAR, alphabet=b"abXY\n", plants=[b"aXbY"]),
    S("single byte", [b"a"], alphabet=b"ab\n"),
    S("-i", [b"abA"], case_sensitive=False, alphabet=b"abAB \n", plants=[b"aBa", b"ABA"]),
    S("-i, memchr_short_search", [b"ab"], case_sensitive=False, alphabet=b"abAB \n"),
    S("-w", [b"ab"], whole_word=True, alphabet=b"abc_ \n-", plants=[b"ab", b" ab ", b"-ab"]),
    S("-w greedy", [b"abab"], whole_word=True, alphabet=b"ab \n-", plants=[b"abab", b"ababab", b" abab"]),
    S("20 bytes: simd_avx2_search", [b"abababababababababab"], alphabet=b"ab\n", plants=[b"ab" * 12]),
    S("neon_search", [b"abcab"], level=abi.REF_NEON, alphabet=b"abc\n", plants=[b"abcabcab"]),
    S("-o simd_sse42_search", [b"abba"], only_matching=True, alphabet=b"ab\n", plants=[b"abbabba"]),
    S("-o boyer_moore_search", [b"abab"], only_matching=True, case_sensitive=False, alphabet=b"abAB\n", plants=[b"ababab"]),
    S("-o -w boyer_moore_search", [b"abab"], only_matching=True, case_sensitive=False, whole_word=True, alphabet=b"abAB \n",
      plants=[b"abab", b" abab "]),
    S("-o memchr_short_search, 2 bytes", [b"ab"], only_matching=True, case_sensitive=False, alphabet=b"abAB\n"),
    S("20-pattern dictionary", WORDS, alphabet=b"ab\n"),
    S("20-pattern dictionary -w", WORDS, whole_word=True, alphabet=b"ab \n"),
    S("20-pattern dictionary -i", WORDS, case_sensitive=False, alphabet=b"abAB\n"),
    S("Sherl[oO]ck", [b"Sherl[oO]ck"], regex=True, alphabet=bytes(range(97, 123)) + b"  \n", plants=[b"Sherlock", b"SherlOck"]),
    S("^ab", [b"^ab"], regex=True, alphabet=b"ab\n", plants=[b"ab"]),
    S("ab$", [b"ab$"], regex=True, alphabet=b"ab\n", plants=[b"ab"]),
    S("^ab$", [b"^ab$"], regex=True, alphabet=b"ab\n", plants=[b"ab", b"\nab\n"]),
    S("^ab -i", [b"^ab"], regex=True, case_sensitive=False, alphabet=b"abAB\n", plants=[b"aB"]),
    S("ab|abc", [b"ab|abc"], regex=True, alphabet=b"abc\n", plants=[b"abc"]),
    S("colou?r", [b"colou?r"], regex=True, alphabet=b"colur \n", plants=[b"color", b"colour"]),
    S("a|aa: a regex plan that is WHOLE", [b"a|aa"], regex=True, alphabet=b"ab\n"),
    S("-e ab -e ba", [b"ab", b"ba"], regex=True, alphabet=b"ab\n"),
]
# each of them with -c as well, but for the two that -c turns into a refused class (below)
TAKEN = TAKEN + [s.with_lines() for s in TAKEN if s.level != abi.REF_NEON and not s.name.startswith("-o memchr_short_search")]

REFUSED = [
    (S("a newline in the pattern", [b"a\nb"]), "a pattern holds '\\n'"),
    (S("a newline in one pattern of several", [b"ab", b"a\nb"]), "a pattern holds '\\n'"),
    (S("[[:space:]]x", [b"[[:space:]]x"], regex=True), "a byte class of the expression holds '\\n'"),
    (S("ab$ -i", [b"ab$"], regex=True, case_sensitive=False), "REG_NOTEOL"),
    (S("(a|b)c$ -i", [b"(a|b)c$"], regex=True, case_sensitive=False), "REG_NOTEOL"),
    (S("-c simd_avx512_search", [b"x" * 40], level=abi.REF_AVX512, count_lines=True), "replays the end of the TEXT"),
    (S("-c -w simd_avx2_search", [b"x" * 20], count_lines=True, whole_word=True), "replays the end of the TEXT"),
    (S("-c neon_search", [b"xyz"], level=abi.REF_NEON, count_lines=True), "replays the end of the TEXT"),
    (S("simd_avx512_search", [b"x" * 40], level=abi.REF_AVX512), "last full 64-byte block"),
    (S("-w simd_avx2_search", [b"x" * 20], whole_word=True), "scalar tail"),
    (S("-w neon_search", [b"xyz"], level=abi.REF_NEON, whole_word=True), "scalar tail"),
    (S("-c -o memchr_short_search", [b"ab"], only_matching=True, case_sensitive=False, count_lines=True), "next line start"),
    (S("-o memchr_short_search, 3 bytes", [b"abc"], only_matching=True, case_sensitive=False), "failed candidate"),
    (S("-o neon_search, bordered", [b"aa"], level=abi.REF_NEON, only_matching=True), "the scalar tail is boyer_moore_search"),
    (S("-o simd_avx2_search, bordered", [b"ab" * 10], only_matching=True), "the scalar tail is boyer_moore_search"),
    (S("max_count", [b"ab"], max_count=5), "max_count"),
    (S("max_count 0 neon_search", [b"xyz"], level=abi.REF_NEON, max_count=0, track_positions=False), "max_count"),
    (S("a regex no compiler takes", [b"a.*b"], regex=True), ""),
]


@pytest.fixture(autouse=True, scope="module")
def _c_locale():
    with regex_ref.c_locale():
        yield


@pytest.fixture()
def eng(monkeypatch):
    import krep_amd
    monkeypatch.setenv("KREP_GPU_ASSUME_AVAILABLE", "1")  # (as the compile tests do: the rule is host logic)
    monkeypatch.delenv("KREP_GPU_DISABLE", raising=False)
    e = krep_amd.load()
    yield e
    e.set_thread_config(None)


def batchable(eng, s):
    s.configure(eng)
    try:
        return eng.batch_can_accelerate(s.params()), eng.last_error()
    finally:
        eng.set_thread_config(None)


@pytest.mark.parametrize("s", TAKEN, ids=lambda s: s.name)
def test_every_class_taken_is_separable(eng, s):
    ok, why = batchable(eng, s)
    assert ok, (s, why)
    rng = np.random.RandomState(sum(s.name.encode()) * 7919 % (1 << 31))
    for k in range(PAIRS):
        na, nb = (0 if rng.randint(8) == 0 else rng.randint(0, 301)), (0 if rng.randint(8) == 0 else rng.randint(0, 301))
        A, B = bm.random_item(rng, s, na), bm.random_item(rng, s, nb)
        assert bm.separable(eng, s, A, B), (s, k, A.tobytes(), B.tobytes())


@pytest.mark.parametrize("s,reason", REFUSED, ids=lambda x: x.name if isinstance(x, bm.Search) else None)
def test_every_refusal_names_its_reason(eng, s, reason):
    ok, why = batchable(eng, s)
    assert not ok and why and reason in why, (s, ok, why)
    # ... and the verdict for a single text is what it was: only the batch refuses these
    s.configure(eng)
    try:
        assert eng.can_accelerate(s.params()) == bool(reason), s
    finally:
        eng.set_thread_config(None)


def test_the_refusals_are_needed(eng):
    """concrete pairs that are NOT separable: what a pack would get wrong if these classes were taken"""
    # a pattern with a newline matches ACROSS the separator
    nl = bm.Search("a newline in the pattern", [b"a\nb"])
    assert not batchable(eng, nl)[0]
    assert not bm.separable(eng, nl, b"xa", b"bx")
    assert bm.reference(eng, nl, b"xa")[0] == 0 and bm.reference(eng, nl, b"bx")[0] == 0 and bm.reference(eng, nl, b"xa\nbx")[0] == 1
    # ab$ under -i: alone, the end of the text "ab" ends no line (REG_NOTEOL); in the pack a newline follows
    eol = bm.Search("ab$ -i", [b"ab$"], regex=True, case_sensitive=False)
    assert not batchable(eng, eol)[0]
    assert bm.reference(eng, eol, b"ab")[0] == 0 and bm.reference(eng, eol, b"ab\nx")[0] == 1
    assert not bm.separable(eng, eol, b"ab", b"x")
    # ... while the case-sensitive search is separable on the same pair
    assert bm.separable(eng, bm.Search("ab$", [b"ab$"], regex=True), b"ab", b"x")
    # memchr_short_search under -o, 3 bytes: the failed candidate on A's last byte steps over B's first byte
    ms3 = bm.Search("-o memchr_short_search, 3 bytes", [b"abc"], only_matching=True, case_sensitive=False)
    assert not batchable(eng, ms3)[0]
    assert bm.reference(eng, ms3, b"abcz")[0] == 1 and bm.reference(eng, ms3, b"xxa\nabcz")[0] == 0
    assert not bm.separable(eng, ms3, b"xxa", b"abcz")
    # neon_search under -o, a pattern that overlaps itself: every occurrence in the 16-byte blocks, non-overlapping ones in the tail
    no = bm.Search("-o neon_search, bordered", [b"aa"], level=abi.REF_NEON, only_matching=True)
    assert not batchable(eng, no)[0]
    assert not bm.separable(eng, no, b"x" * 13, b"aaaa")
    # [[:space:]]x: the separator itself is a space
    sp = bm.Search("[[:space:]]x", [b"[[:space:]]x"], regex=True)
    assert not batchable(eng, sp)[0]
    assert not bm.separable(eng, sp, b"a", b"x")


def test_pack_and_split_are_inverse():
    rng = np.random.RandomState(5)
    items = [rng.randint(97, 100, size=n).astype(np.uint8) for n in (0, 3, 0, 0, 7, 1, 0)]
    packed, off = bm.pack(items)
    assert packed.size == sum(a.size for a in items) + len(items) - 1 and int(off[-1]) == packed.size + 1
    for i, a in enumerate(items):
        assert np.array_equal(packed[int(off[i]):int(off[i]) + a.size], a)
        assert i == len(items) - 1 or packed[int(off[i]) + a.size] == 10
    recs = np.array([[int(off[1]), int(off[1]) + 2], [int(off[4]) + 1, int(off[4]) + 3], [int(off[4]) + 5, int(off[4]) + 7],
                     [int(off[5]), int(off[5]) + 1]], dtype=np.uint64)
    parts = bm.split(recs, items)
    assert [p.tolist() for p in parts] == [[], [[0, 2]], [], [], [[1, 3], [5, 7]], [[0, 1]], []]
