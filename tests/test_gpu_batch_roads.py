"""krep_gpu_search_batch on the roads tests/test_gpu_batch.py does not take: one class per reference function the rule takes, newlines at
item edges, the edge of the offset table in LDS, a batch that goes through the staging ring (a second pinned chunk, four fill threads),
an item beyond the pack limit, the caller's arguments (cfg, records == NULL, track_positions), one engine reused across batches of other
sizes and densities, and the four failure points.  Every comparison is exact: the count and every (start, end) in emission order, against
the compiled reference on each item alone and against the operator on each item alone (batch_model.check_batch)."""
import numpy as np
import pytest

import batch_model as bm
import regex_ref
from krep_amd import abi

pytestmark = pytest.mark.gpu

S = bm.Search
WORDS = [b"a", b"b", b"ab", b"ba", b"aa", b"bb", b"aab", b"aba", b"abb", b"baa", b"bab", b"bba", b"aaa", b"bbb", b"abab", b"baba",
         b"aabb", b"bbaa", b"abba", b"baab"]
TEXT = bytes(range(97, 123)) + b"  \n"
MIB = 1 << 20
EMPTY = np.zeros(0, dtype=np.uint8)
L20, L40 = b"Sherlock Holmes and.", b"Sherlock Holmes and the Hound of Baskerv"
# (search, the reference function a long text reaches — None: not a single literal): the classes tests/test_gpu_batch.py CLASSES lacks
ROADS = [
    (S("boyer_moore_search", [b"aXbY"], level=abi.REF_SCALAR, alphabet=b"abXY \n", plants=[b"aXbY"]), abi.RA_BMH),
    (S("--algo bm on an AVX2 build", [b"Sherlock"], algo_override=abi.ALGO_BM, alphabet=TEXT, plants=[b"Sherlock"]), abi.RA_BMH),
    (S("--algo kmp on an AVX2 build", [b"abab"], algo_override=abi.ALGO_KMP, alphabet=b"ab \n", plants=[b"abab", b"ababab"]), abi.RA_KMP),
    (S("force_no_simd", [b"Sherlock"], force_no_simd=True, alphabet=TEXT, plants=[b"Sherlock"]), abi.RA_BMH),
    (S("memchr_short_search, scalar build", [b"ab"], level=abi.REF_SCALAR, alphabet=b"abcd \n", plants=[b"ab"]), abi.RA_MEMCHR_SHORT),
    (S("memchr_short_search -i", [b"ab"], case_sensitive=False, alphabet=b"abAB \n", plants=[b"aB"]), abi.RA_MEMCHR_SHORT),
    (S("memchr_search -w", [b"a"], whole_word=True, alphabet=b"ab \n-", plants=[b"a", b" a "]), abi.RA_MEMCHR),
    (S("memchr_search -i", [b"a"], case_sensitive=False, alphabet=b"abAB\n", plants=[b"A"]), abi.RA_MEMCHR),
    (S("neon_search, border-free", [b"abc"], level=abi.REF_NEON, alphabet=b"abc\n", plants=[b"abc"]), abi.RA_NEON),
    (S("neon_search, bordered", [b"abcab"], level=abi.REF_NEON, alphabet=b"abc\n", plants=[b"abcab", b"abcabcab"]), abi.RA_NEON),
    (S("neon_search -o, border-free", [b"abc"], level=abi.REF_NEON, only_matching=True, alphabet=b"abc\n", plants=[b"abc"]), abi.RA_NEON),
    (S("simd_avx2_search -o, border-free, 20 bytes", [L20], only_matching=True, alphabet=TEXT, plants=[L20]), abi.RA_AVX2),
    (S("SSE4.2 build, 16 bytes", [L20[:16]], level=abi.REF_SSE42, alphabet=TEXT, plants=[L20[:16]]), abi.RA_SSE42),
    (S("AVX-512 build, 20 bytes: simd_avx2_search", [L20], level=abi.REF_AVX512, alphabet=TEXT, plants=[L20]), abi.RA_AVX2),
    (S("AVX-512 build, 40 bytes -i: boyer_moore_search", [L40], level=abi.REF_AVX512, case_sensitive=False, alphabet=TEXT + b"SH",
       plants=[L40.lower()]), abi.RA_BMH),
    (S("-o -w boyer_moore_search", [b"abab"], only_matching=True, case_sensitive=False, whole_word=True, alphabet=b"abAB \n",
       plants=[b"abab", b" abab "]), abi.RA_BMH),
    (S("20-pattern dictionary -i", WORDS, case_sensitive=False, alphabet=b"abABcdefghijklmnop \n", plants=[b"aBAb"]), None),
    (S("dictionary with one 24-byte pattern", [b"ab", b"Sherlock Holmes and the."], alphabet=TEXT, plants=[b"Sherlock Holmes and the."]), None),
    (S("dictionary of patterns of at most 4 bytes", [b"he", b"she", b"hers", b"q"], alphabet=TEXT, plants=[b"hers"]), None),
    (S("-e ab -e ba", [b"ab", b"ba"], regex=True, alphabet=b"abcdefgh\n", plants=[b"ab"]), None),
    (S("^ab -i", [b"^ab"], regex=True, case_sensitive=False, alphabet=b"abAB\n", plants=[b"aB"]), None),
    (S("(a|b)c$", [b"(a|b)c$"], regex=True, alphabet=b"abc\n", plants=[b"ac"]), None),
]


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
    e.inject_failure(0)
    e.batch_pack_limit(0)
    e.set_thread_config(None)


def batchable(gpu, s):
    s.configure(gpu)
    try:
        return gpu.batch_can_accelerate(s.params()), gpu.last_error()
    finally:
        gpu.set_thread_config(None)


def arrays(texts):
    return [np.frombuffer(t, dtype=np.uint8) for t in texts]


# ------------------------------------------------------------------------------------------------ 1. one class per reference function
@pytest.mark.parametrize("s,algo", ROADS, ids=lambda x: x.name if isinstance(x, bm.Search) else None)
def test_one_class_per_reference_function(gpu, s, algo):
    ok, why = batchable(gpu, s)
    assert ok, (s, why)
    if algo is not None:
        s.configure(gpu)
        try:
            assert gpu.mirror_select(s.params(), MIB) == algo, s  # the road the name promises
        finally:
            gpu.set_thread_config(None)
    tiny = gpu.tiny_launches()
    items = bm.edge_items(s)
    got, info = bm.check_batch(gpu, s, items)
    assert info.scans == 1 and info.total_records == sum(c for c, _ in got)
    if not s.name.endswith("$"):  # (a match at the first byte of an item needs a '\n' behind it there)
        assert any(p.size and p[0, 0] == 0 for _, p in got)
    assert any(p.size and p[-1, 1] == it.size for (_, p), it in zip(got, items))
    if s.name.startswith("dictionary of patterns of at most 4 bytes"):
        assert gpu.tiny_launches() > tiny  # every pattern <= 4 bytes: the register-compare kernel scans the pack
    q = s.with_lines()
    ok, why = batchable(gpu, q)
    if ok:  # -c as well where the rule takes it (neon_search and -o memchr_short_search: refused, with a reason)
        got, info = bm.check_batch(gpu, q, items)
        assert info.scans == 1 and sum(c for c, _ in got) > 0
    else:
        assert why and s.level == abi.REF_NEON, (q, why)


# ------------------------------------------------------------------------------------------------ 2. newlines at item edges
@pytest.mark.parametrize("s", [S("ab", [b"ab"]), S("20-pattern dictionary", WORDS)], ids=lambda s: s.name)
def test_newlines_at_item_edges(gpu, s):
    items = arrays((b"ab\n", b"\nab", b"\n", b"\n\n", b"", b"ab\n\nab", b"ab"))
    got, _ = bm.check_batch(gpu, s, items)
    lined, _ = bm.check_batch(gpu, s.with_lines(), items)
    if s.name == "ab":
        assert [c for c, _ in got] == [1, 1, 0, 0, 0, 2, 1]
        assert [p.tolist() for _, p in got] == [[[0, 2]], [[1, 3]], [], [], [], [[0, 2], [4, 6]], [[0, 2]]]
    # the first record of an item opens a line of its own even where the item before it ended in '\n' (items 0 -> 1), and two records of
    # an item on two lines with an empty line between them are two lines (item 5); 3 dictionary words start on every "ab": one line each
    assert [c for c, _ in lined] == [1, 1, 0, 0, 0, 2, 1]


# ------------------------------------------------------------------------------------------------ 3. the LDS table's edge
@pytest.mark.parametrize("n_items", [4095, 4096])
def test_the_offset_table_at_and_over_its_lds_size(gpu, n_items):
    """n_items + 1 offsets: 4096 fill the table batch_rebase keeps in LDS, 4097 do not (the binary search runs in global memory)"""
    s = S("border-free literal", [b"aab"], alphabet=b"ab\n", plants=[b"aab"])
    rng = np.random.RandomState(n_items)
    items = [bm.random_item(rng, s, int(rng.randint(0, 13))) for _ in range(n_items)]
    items[-1] = np.frombuffer(b"xaabaab", dtype=np.uint8)  # the last item holds records: its base is the table's last entry but one
    lds, glob = gpu.batch_rebase_launches()
    got, info = bm.check_batch(gpu, s, items, single_every=512)
    assert info.total_records > 200 and got[-1][1].tolist() == [[1, 4], [4, 7]]
    lds1, glob1 = gpu.batch_rebase_launches()
    assert (lds1 - lds, glob1 - glob) == ((1, 0) if n_items + 1 <= 4096 else (0, 1))
    bm.check_batch(gpu, s.with_lines(), items, single_every=512)


def test_batches_of_empty_items_and_of_one_item(gpu):
    s = S("border-free literal", [b"aab"], alphabet=b"ab\n", plants=[b"aab"])
    for q in (s, s.with_lines()):
        got, info = bm.check_batch(gpu, q, [EMPTY] * 300, single_every=100)
        assert [c for c, _ in got] == [0] * 300 and info.total_records == 0 and info.packed_bytes == 299
        got, info = bm.check_batch(gpu, q, [EMPTY])
        assert got[0][0] == 0 and info.packed_bytes == 0
        got, info = bm.check_batch(gpu, q, arrays([b"a"]))
        assert got[0][0] == 0 and info.packed_bytes == 1
    one = S("single byte", [b"a"])
    assert [c for c, _ in bm.check_batch(gpu, one, arrays([b"a"]))[0]] == [1]
    assert [c for c, _ in bm.check_batch(gpu, one.with_lines(), arrays([b"a"]))[0]] == [1]


# ------------------------------------------------------------------------------------------------ 4. through the ring
@pytest.fixture(scope="module")
def ring_items():
    """about 36 MiB: 2000 items of 0..2 KiB with runs of 20 empty ones, a 9 MiB item at index 400 and a 25 MiB item at index 1200;
    `Sherlock` about once per 64 KiB, and at both ends of the two large items"""
    rng = np.random.RandomState(36)
    alpha, plant = np.frombuffer(TEXT, dtype=np.uint8), np.frombuffer(b"Sherlock", dtype=np.uint8)
    items = []
    for k in range(2002):
        n = 9 * MIB if k == 400 else 25 * MIB if k == 1200 else 0 if k % 250 >= 230 else int(rng.randint(0, 2049))
        t = alpha[rng.randint(0, alpha.size, size=n)] if n else EMPTY
        for at in rng.randint(0, max(n - 8, 1), size=n >> 16):
            t[at:at + 8] = plant
        if n >= MIB:
            t[:8] = plant
            t[n - 8:] = plant
        elif n >= 8 and rng.randint(32) == 0:
            t[rng.randint(0, n - 7):][:8] = plant
        items.append(t)
    return items


def test_a_batch_through_the_staging_ring(gpu, ring_items):
    """packed size > 33 MiB: Stager::gather fills a first chunk of 32 MiB with four threads (each entering the pack at a quarter of the
    chunk, in the middle of one of the large items) and a second chunk, which begins inside the 25 MiB item, in the other pinned buffer"""
    s = S("border-free literal", [b"Sherlock"], alphabet=TEXT, plants=[b"Sherlock"])
    packed = sum(it.size for it in ring_items) + len(ring_items) - 1
    assert packed > 33 * MIB + 8 * MIB // 4
    got, info = bm.check_batch(gpu, s, ring_items, single_every=200)  # (the two large items lie on multiples of 200)
    assert info.scans == 1 and info.packed_bytes == packed
    for k in (400, 1200):
        n = ring_items[k].size
        assert got[k][1][0].tolist() == [0, 8] and got[k][1][-1].tolist() == [n - 8, n] and got[k][0] > n >> 17
    assert info.total_records == sum(c for c, _ in got) > 500


def test_the_same_batch_for_a_dictionary_under_c(gpu, ring_items):
    s = S("20-pattern dictionary -c", WORDS, alphabet=TEXT, count_lines=True)
    got, info = bm.check_batch(gpu, s, ring_items, single_every=200)
    assert info.scans == 1 and info.total_records > 65536
    assert got[1200][0] > 100000


# ------------------------------------------------------------------------------------------------ 5. an item beyond the limit
def cut(sizes, limit):
    """the documented rule: a pack is cut between items and never inside one; an item beyond the limit is a pack of its own"""
    packs, i = [], 0
    while i < len(sizes):
        j, used = i, 0  # `used`: the bytes of the pack so far, the separator behind its last item included
        while j < len(sizes) and (j == i or used + sizes[j] <= limit):
            used += sizes[j] + 1
            j += 1
        packs.append((i, j))
        i = j
    return packs


def test_an_item_beyond_the_pack_limit_is_a_pack_of_its_own(gpu):
    K = 1 << 10
    sizes = [10 * K, 200 * K, 0, 5 * K, 70 * K, 64 * K - 1, 2, 64 * K]
    assert cut(sizes, 64 * K) == [(0, 1), (1, 2), (2, 4), (4, 5), (5, 6), (6, 7), (7, 8)]
    s = S("border-free literal", [b"ab"], alphabet=b"xyz \n", plants=[b"ab"])
    rng = np.random.RandomState(5)
    items = []
    for n in sizes:
        t = bm.random_item(rng, s, n)
        t[:2] = np.frombuffer(b"ab", dtype=np.uint8)[:n]
        t[max(n - 2, 0):] = np.frombuffer(b"ab", dtype=np.uint8)[:n]
        for at in rng.randint(0, max(n - 2, 1), size=n >> 12):
            t[at:at + 2] = np.frombuffer(b"ab", dtype=np.uint8)
        items.append(t)
    one, info1 = bm.check_batch(gpu, s, items)
    assert info1.scans == 1 and all(c >= 2 for (c, _), n in zip(one, sizes) if n > 2)
    gpu.batch_pack_limit(64 * K)
    try:
        many, info = bm.check_batch(gpu, s, items)
        rc, res, n, first, recs, rinfo = bm.raw_call(gpu, s.params(), items, want=True)
        lined, linfo = bm.check_batch(gpu, s.with_lines(), items)
    finally:
        gpu.batch_pack_limit(0)
    assert info.scans == rinfo.scans == linfo.scans == len(cut(sizes, 64 * K)) == 7
    assert info.total_records == info1.total_records and info.packed_bytes == info1.packed_bytes - (info.scans - 1)
    for (c1, p1), (c2, p2) in zip(one, many):
        assert c1 == c2 and np.array_equal(p1, p2)
    # first_record runs on across the packs: every item's records lie behind those of all items before it, whatever pack they were in
    assert rc == 0 and first == 77 and n == 1 + info.total_records
    at = 1
    for (c, fr, nr), (c1, p1) in zip(res, one):
        assert (c, fr, nr) == (c1, at, c1) and np.array_equal(recs[fr:fr + nr], p1)
        at += nr


# ------------------------------------------------------------------------------------------------ 6. the caller's arguments
def test_an_explicit_cfg_wins_over_the_thread_configuration(gpu):
    s = S("abab", [b"abab"], alphabet=b"ab\n", plants=[b"ababab"])
    om = S("abab -o", [b"abab"], only_matching=True, alphabet=b"ab\n", plants=[b"ababab"])
    rng = np.random.RandomState(6)
    items = arrays([b"abababab", b"", b"xababab"]) + [bm.random_item(rng, s, 300) for _ in range(5)]
    plain = [bm.reference(gpu, s, it) for it in items]
    only = [bm.reference(gpu, om, it) for it in items]
    assert [c for c, _ in plain] != [c for c, _ in only] and plain[0][0] == 2 and only[0][0] == 3  # greedy walk / every occurrence
    gpu.set_thread_config(s.config(gpu))  # only_matching = 0 on the thread, 1 in cfg
    try:
        for cfg, want in ((om.config(gpu), only), (None, plain)):
            rc, res, n, first, recs, _ = bm.raw_call(gpu, s.params(), items, cfg=cfg, want=True)
            assert rc == 0 and first == 77
            assert [r[0] for r in res] == [c for c, _ in want]
            for (c, fr, nr), (_, p) in zip(res, want):
                assert np.array_equal(recs[fr:fr + nr], p.reshape(-1, 2))
    finally:
        gpu.set_thread_config(None)


def test_without_records_and_without_track_positions(gpu):
    s = S("ab", [b"ab"], alphabet=b"ab \n", plants=[b"ab"])
    rng = np.random.RandomState(66)
    items = arrays([b"xabxab", b"", b"ab"]) + [bm.random_item(rng, s, 200) for _ in range(4)]
    counts = [bm.reference(gpu, s, it)[0] for it in items]
    assert counts[:3] == [2, 0, 1]
    # records == NULL with track_positions set: the counts, and no record is reported anywhere
    rc, res, n, first = bm.raw_call(gpu, s.params(), items, records=False)
    assert rc == 0 and res == [(c, 0, 0) for c in counts]
    # track_positions false, no -c: the counts, no records, the caller's list as it was
    rc, res, n, first, recs, info = bm.raw_call(gpu, abi.Params([b"ab"], track_positions=False), items, want=True)
    assert rc == 0 and res == [(c, 1, 0) for c in counts] and n == 1 and recs.tolist() == [[77, 78]]
    assert info.total_records == sum(counts)


# ------------------------------------------------------------------------------------------------ 7. reuse
def test_one_engine_across_batches_of_other_sizes_and_densities(gpu):
    """the scratch buffers grow between calls (items: 10 -> 5000; the line scratch is first allocated by a -c call that comes late, with
    more records than its smallest size), and the cached plan meets a dense pack between two sparse ones"""
    s = S("single byte", [b"a"], alphabet=b"bcdefghijklmnopqrstuvwxyz  \n", plants=[b"a"])
    dense = S("single byte", [b"a"], alphabet=b"aaab\n")
    gpu.release_device_resources()  # (the scratch of the tests before this one is gone: the sizes below are what grows it)
    rng = np.random.RandomState(77)

    def sparse(n):
        return [bm.random_item(rng, s, int(rng.randint(0, 40))) for _ in range(n)]

    skew = sparse(30)
    skew[17] = bm.random_item(rng, dense, (128 << 10) + 5)
    few = sparse(10)
    for items, every in ((few, 1), (sparse(5000), 1000), (sparse(3), 1), (sparse(7000), 1000)):
        bm.check_batch(gpu, s, items, single_every=every)
    got, info = bm.check_batch(gpu, s.with_lines(), skew, single_every=17)  # -c, > 65536 records, between two record calls
    assert info.total_records > 65536 and got[17][0] > 1000
    bm.check_batch(gpu, s, few)
    got, info = bm.check_batch(gpu, s, skew, single_every=17)               # dense between two sparse ones
    assert info.total_records > 65536 and got[17][0] == info.total_records - sum(c for k, (c, _) in enumerate(got) if k != 17)
    bm.check_batch(gpu, s, few)
    bm.check_batch(gpu, s.with_lines(), few)


# ------------------------------------------------------------------------------------------------ 8. failure points
KINDS = {1: "device allocation", 2: "host->device copy", 3: "kernel launch", 4: "device->host copy"}


@pytest.mark.parametrize("limit", [0, 64 << 10], ids=["one pack", "several packs"])
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_a_failure_appends_nothing_and_writes_no_result(gpu, kind, limit):
    s = S("border-free literal", [b"Sherlock"], alphabet=TEXT, plants=[b"Sherlock"])
    items = bm.edge_items(s, seed=13, n_items=28)
    poisoned = [(bm.POISON,) * 3] * len(items)
    gpu.batch_pack_limit(limit)
    try:
        for q in (s, s.with_lines()):
            gpu.release_device_resources()  # so that allocation and plan creation happen again, under the injection
            gpu.inject_failure(kind)
            try:
                rc, res, n, first, recs, _ = bm.raw_call(gpu, q.params(), items, want=True)
                why = gpu.last_error()
            finally:
                gpu.inject_failure(0)
            assert rc == 2 and why, (KINDS[kind], q)
            assert res == poisoned and n == 1 and first == 77 and recs.tolist() == [[77, 78]], (KINDS[kind], q, why)
        # ... and the next call works again
        got, info = bm.check_batch(gpu, s, items, single_every=7)
        assert info.scans == (1 if not limit else len(cut([it.size for it in items], limit))) and info.total_records > 28
        bm.check_batch(gpu, s.with_lines(), items, single_every=7)
    finally:
        gpu.inject_failure(0)
        gpu.batch_pack_limit(0)
