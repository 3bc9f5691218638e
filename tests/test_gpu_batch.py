"""A batch of texts in one scan (krep_gpu_search_batch, kg_batch.hip): the items packed with a '\\n' between neighbours, one scan,
the record list cut per item on the device.  For every item the batch must give what the operator gives for the item ALONE
(gpu.search) and what the reference gives (tests/batch_model.py: the compiled reference, the restatement under -o): the count,
every (start, end) relative to the item's first byte, the reference's emission order.  Each test uses well under 2 MiB."""
import numpy as np
import pytest

import batch_model as bm
import regex_ref
from krep_amd import abi
from krep_amd.engine import KrepGpuError

pytestmark = pytest.mark.gpu

S = bm.Search
WORDS = [b"a", b"b", b"ab", b"ba", b"aa", b"bb", b"aab", b"aba", b"abb", b"baa", b"bab", b"bba", b"aaa", b"bbb", b"abab", b"baba",
         b"aabb", b"bbaa", b"abba", b"baab"]
TEXT = bytes(range(97, 123)) + b"  \n"
# one search of every class the batch takes (tests/test_batch_separable_cpu.py shows each is separable); `plants[0]` is a match
CLASSES = [
    S("border-free literal", [b"Sherlock"], alphabet=TEXT, plants=[b"Sherlock"]),
    S("bordered literal: simd_sse42_search greedy", [b"abab"], alphabet=b"ab \n", plants=[b"abab", b"ababab"]),
    S("bordered literal: kmp_search greedy", [b"abab"], level=abi.REF_SCALAR, alphabet=b"ab \n", plants=[b"abab", b"ababab"]),
    S("single byte", [b"a"], alphabet=b"abcdefgh\n", plants=[b"a"]),
    S("-i", [b"abA"], case_sensitive=False, alphabet=b"abAB \n", plants=[b"aBa"]),
    S("-w", [b"ab"], whole_word=True, alphabet=b"abc_ \n-", plants=[b"ab", b" ab "]),
    S("-w greedy", [b"abab"], whole_word=True, alphabet=b"ab \n-", plants=[b"abab", b" abab "]),
    S("20 bytes: simd_avx2_search", [b"Sherlock Holmes and."], alphabet=TEXT, plants=[b"Sherlock Holmes and."]),
    S("-o simd_sse42_search", [b"abba"], only_matching=True, alphabet=b"ab\n", plants=[b"abba", b"abbabba"]),
    S("-o boyer_moore_search", [b"abab"], only_matching=True, case_sensitive=False, alphabet=b"abAB\n", plants=[b"abab", b"ababab"]),
    S("-o memchr_short_search, 2 bytes", [b"ab"], only_matching=True, case_sensitive=False, alphabet=b"abAB\n", plants=[b"ab"]),
    S("20-pattern dictionary", WORDS, alphabet=b"abcdefghijklmnop \n", plants=[b"abab"]),
    S("20-pattern dictionary -w", WORDS, whole_word=True, alphabet=b"abcdefghijklmnop \n", plants=[b"abab"]),
    S("Sherl[oO]ck", [b"Sherl[oO]ck"], regex=True, alphabet=TEXT, plants=[b"SherlOck", b"Sherlock"]),
    S("^ab", [b"^ab"], regex=True, alphabet=b"ab\n", plants=[b"ab"]),
    S("ab$", [b"ab$"], regex=True, alphabet=b"ab\n", plants=[b"ab"]),
    S("ab|abc", [b"ab|abc"], regex=True, alphabet=b"abc\n", plants=[b"abc"]),
    S("colou?r", [b"colou?r"], regex=True, alphabet=b"colur \n", plants=[b"colour", b"color"]),
    S("a|aa: a regex plan that is WHOLE", [b"a|aa"], regex=True, alphabet=b"abcd\n", plants=[b"aaa"]),
]
CLASSES = CLASSES + [s.with_lines() for s in CLASSES if not s.name.startswith("-o memchr_short_search")]


@pytest.fixture(autouse=True, scope="module")
def _c_locale():
    with regex_ref.c_locale():
        yield


@pytest.fixture(scope="module")
def gpu():
    import krep_amd
    e = krep_amd.load()
    assert e.device_count() >= 1 and e.available(), e.unavailable_reason()
    yield e
    e.batch_pack_limit(0)
    e.set_thread_config(None)


edge_items, check_batch = bm.edge_items, bm.check_batch  # (shared with tests/test_gpu_batch_roads.py)


@pytest.mark.parametrize("s", CLASSES, ids=lambda s: s.name)
def test_edge_shapes(gpu, s):
    items = edge_items(s)
    got, info = check_batch(gpu, s, items)
    assert info.scans == 1
    if not s.kw.get("count_lines"):
        assert info.total_records == sum(c for c, _ in got)
        # the generator did what it says: matches at the first byte and up to the last byte of some item
        assert any(p.size and p[0, 0] == 0 for _, p in got)
        assert any(p.size and p[-1, 1] == it.size for (_, p), it in zip(got, items))
    else:
        assert sum(c for c, _ in got) > 0


def test_a_pattern_split_across_two_items_is_not_found(gpu):
    s = S("border-free literal", [b"Sherlock"], alphabet=b"xyz \n")
    items = [np.frombuffer(t, dtype=np.uint8) for t in (b"xx Sher", b"lock yy", b"Sherlock", b"S", b"herlock", b"", b"Sherloc", b"", b"k")]
    got, _ = check_batch(gpu, s, items)
    assert [c for c, _ in got] == [0, 0, 1, 0, 0, 0, 0, 0, 0]
    assert got[2][1].tolist() == [[0, 8]]


SKEW = [(S("single byte", [b"a"], alphabet=b"aaab\n"), 128 << 10), (S("20-pattern dictionary", WORDS, alphabet=b"ab\n"), 48 << 10),
        (S("a|aa", [b"a|aa"], regex=True, alphabet=b"aab\n"), 256 << 10)]
SKEW = SKEW + [(s.with_lines(), n) for s, n in SKEW]


@pytest.mark.parametrize("s,size", SKEW, ids=lambda x: x.name if isinstance(x, bm.Search) else None)
def test_skew_one_item_holds_every_match(gpu, s, size):
    """200 empty or match-free items around ONE that holds every record of the batch — more than the first record buffer takes
    (65536), so the scan runs again at the exact size; the segmentation must not loop per item over its records"""
    rng = np.random.RandomState(3)
    free = S("free", [], alphabet=b"xyz\n")
    items = [np.zeros(0, dtype=np.uint8) if k % 2 else bm.random_item(rng, free, int(rng.randint(1, 200))) for k in range(201)]
    items[100] = bm.random_item(rng, s, size + 5)
    got, info = check_batch(gpu, s, items, single_every=50)
    assert all(c == 0 for k, (c, _) in enumerate(got) if k != 100) and got[100][0] > 0
    assert info.total_records > 65536 and info.scans == 1


def test_whole_word_at_item_edges(gpu):
    s = S("-w", [b"ab"], whole_word=True)
    items = [np.frombuffer(t, dtype=np.uint8) for t in (b"zz c", b"ab cd", b"ab", b"xab", b"ab", b"abc", b"c", b"ab_", b"_", b"ab")]
    for q in (s, s.with_lines()):
        got, _ = check_batch(gpu, q, items)
        # an item that ends in a word byte does not glue to the pattern that begins the next one; an item that IS the pattern matches
        assert [c for c, _ in got] == [0, 1, 1, 0, 1, 0, 0, 0, 0, 1]
    d = S("20-pattern dictionary -w", WORDS, whole_word=True)
    check_batch(gpu, d, items)


@pytest.mark.parametrize("pat", [b"^ab", b"ab$", b"^ab$"])
def test_line_anchors_at_item_edges(gpu, pat):
    s = S(pat.decode(), [pat], regex=True)
    texts = (b"ab\nxab\nab", b"ab", b"", b"xab\nab", b"ab\n", b"\nab", b"abx\nxab", b"ab\nab\nab", b"x", b"ab")
    items = [np.frombuffer(t, dtype=np.uint8) for t in texts]
    for q in (s, s.with_lines()):
        got, _ = check_batch(gpu, q, items)
        assert got[1][0] == 1 and got[2][0] == 0 and got[9][0] == 1  # the first and the last line of an item are lines of their own
    want = {b"^ab": [2, 1, 0, 1, 1, 1, 1, 3, 0, 1], b"ab$": [3, 1, 0, 2, 1, 1, 1, 3, 0, 1], b"^ab$": [2, 1, 0, 1, 1, 1, 0, 3, 0, 1]}[pat]
    assert [c for c, _ in gpu_counts(gpu, s, items)] == want


def gpu_counts(gpu, s, items):
    s.configure(gpu)
    try:
        return gpu.search_batch(s.params(), items)
    finally:
        gpu.set_thread_config(None)


def test_multi_pattern_emission_order_inside_an_item(gpu):
    s = S("20-pattern dictionary", WORDS, alphabet=b"ab\n")
    rng = np.random.RandomState(8)
    items = [bm.random_item(rng, s, n) for n in (300, 0, 17, 1025, 5, 64)]
    got, _ = check_batch(gpu, s, items)  # equal to the reference's list, order included
    for _, p in got:
        if p.shape[0] > 1:
            ends, starts = p[:, 1].astype(np.int64), p[:, 0].astype(np.int64)
            assert np.all(np.diff(ends) >= 0)                                  # end ascending
            same = np.diff(ends) == 0
            assert np.all(np.diff(starts)[same] > 0)                           # ... and the longest first among equal ends
    assert any(np.any(np.diff(p[:, 1].astype(np.int64)) == 0) for _, p in got if p.shape[0] > 1)


def test_more_items_than_the_offset_table_in_lds_holds(gpu):
    """5000 items: the rebase kernel finds a record's item by binary search in global memory instead of LDS (4096 entries)"""
    s = S("border-free literal", [b"aab"], alphabet=b"ab\n", plants=[b"aab"])
    rng = np.random.RandomState(21)
    items = [bm.random_item(rng, s, int(rng.randint(0, 40))) for _ in range(5000)]
    got, info = check_batch(gpu, s, items, single_every=250)
    assert info.total_records > 1000
    check_batch(gpu, s.with_lines(), items, single_every=250)


@pytest.mark.parametrize("s", [CLASSES[0], CLASSES[1], CLASSES[11], CLASSES[13], CLASSES[0].with_lines(), CLASSES[11].with_lines()],
                         ids=lambda s: s.name)
def test_several_packs(gpu, s):
    items = edge_items(s, seed=12)
    one, info1 = check_batch(gpu, s, items, single_every=48)
    gpu.batch_pack_limit(64 << 10)
    try:
        many, info = check_batch(gpu, s, items, single_every=48)
    finally:
        gpu.batch_pack_limit(0)
    assert info1.scans == 1 and info.scans > 1
    assert info.total_records == info1.total_records and info.packed_bytes == info1.packed_bytes - (info.scans - 1)
    for (c1, p1), (c2, p2) in zip(one, many):
        assert c1 == c2 and np.array_equal(p1, p2)


def test_refusals_come_before_any_device_work(gpu):
    for p, reason in ((abi.Params([b"ab"], max_count=5), "max_count"), (abi.Params([b"a\nb"]), "a pattern holds '\\n'"),
                      (abi.Params([b"[[:space:]]x"], regex=True), "a byte class of the expression holds '\\n'")):
        assert not gpu.batch_can_accelerate(p) and reason in gpu.last_error()
        rc, res, n, first = bm.raw_call(gpu, p, [b"xabx", b"a\nb x", b""])
        assert rc == 2 and reason in gpu.last_error(), gpu.last_error()
        assert res == [(bm.POISON,) * 3] * 3 and n == 1 and first == 77
        with pytest.raises(KrepGpuError):
            gpu.search_batch(p, [b"xabx"])


def test_records_are_appended_behind_what_the_list_holds(gpu):
    """first_record indexes records->positions: a list that already holds a record keeps it, the batch's records follow"""
    rc, res, n, first = bm.raw_call(gpu, abi.Params([b"ab"]), [b"xabxab", b"", b"ab"])
    assert rc == 0 and res == [(2, 1, 2), (0, 3, 0), (1, 3, 1)] and n == 4 and first == 77
    rc, res, n, first = bm.raw_call(gpu, abi.Params([b"ab"], count_lines=True), [b"xabxab\nab", b"", b"ab"])
    assert rc == 0 and res == [(2, 1, 0), (0, 1, 0), (1, 1, 0)] and n == 1 and first == 77
    assert gpu.search_batch(abi.Params([b"ab"]), []) == []
