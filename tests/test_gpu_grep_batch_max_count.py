"""krep_gpu_grep_batch under a max_count (krep_gpu_set_batch_max_count): what `krep -m N [-o | -c] PATTERN` prints for every item of
a batch, from the device.  Expected bytes: batch_grep_model.definition() fed per item with what search_file() hands its formatter —
the reference's records for the item ALONE under that max_count, cut to their first N and put in (start, end) order
(tests/test_batch_grep_max_count_cpu.py pins that to the stock CLI); the operator on the item alone must give the same list.  Every
test turns the process-wide switch on and off again.  Each test uses a few MiB at most."""
import numpy as np
import pytest

import batch_cut_model as cm
import batch_grep_model as bg
import batch_model as bm
import regex_ref
from krep_amd import abi
from krep_amd.engine import KrepGpuError
from test_abi_grep_batch import POISON, raw_call
from test_gpu_batch_format import classes, names_for, shaped_items

pytestmark = pytest.mark.gpu

S = bm.Search
NESTED = [b"he", b"she", b"hers", b"abcd", b"bc", b"c"]


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
    e.inject_failure(0)
    e.set_thread_config(None)


@pytest.fixture(autouse=True)
def switch(gpu):
    assert not gpu.get_batch_max_count()
    gpu.set_batch_max_count(True)
    yield
    gpu.set_batch_max_count(False)


def limited(s, M, **extra):
    kw = dict(s.kw)
    kw.update(extra)
    kw["max_count"] = M
    return S("%s -m %d" % (s.name, M), s.pats, s.level, s.only_matching, s.regex, s.alphabet, s.plants, s.algo_override, s.force_no_simd,
             **kw)


def arr(b):
    return np.frombuffer(bytes(b), dtype=np.uint8)


def grep(gpu, s, items, names, color=False, want_info=False):
    return gpu.grep_batch(s.params(), items, names, color=color, cfg=s.config(gpu), want_info=want_info)


def search_file_lists(gpu, q, items, M, operator_every=4):
    """per item what search_file() formats under -m M: the function's list for the item alone, its first M, in (start, end) order —
    from the reference, and (every few items) from the operator on the item alone"""
    out = []
    for i, it in enumerate(items):
        r = cm.by_start(np.asarray(bm.reference(gpu, q, it)[1], dtype=np.uint64).reshape(-1, 2)[:M])
        if i % operator_every == 0:
            q.configure(gpu)
            try:
                one = gpu.search(q.params(), it)
            finally:
                gpu.set_thread_config(None)
            assert np.array_equal(cm.by_start(one[1][:M]), r), (q, i)
        out.append(r)
    return out


def check(gpu, q, items, recs, names, mode, color, counts=None):
    want, where = bg.definition(items, recs, names, mode, color, counts)
    got, per, info = grep(gpu, q, items, names, color, want_info=True)
    assert got == want, (q, mode, color, len(got), len(want), next((k for k in range(len(want)) if got[k:k + 1] != want[k:k + 1]), None))
    assert [(o, n) for _, o, n in per] == where
    assert [c for c, _, _ in per] == ([r.shape[0] for r in recs] if counts is None else counts)
    return info


@pytest.mark.parametrize("M", [1, 2, 3])
@pytest.mark.parametrize("mode", ["lines", "matches"])
@pytest.mark.parametrize("idx", range(5), ids=[s.name for s in classes(False)])
def test_edge_shapes(gpu, idx, mode, M):
    q = limited(classes(mode == "matches")[idx], M)
    items = shaped_items(q)
    recs = search_file_lists(gpu, q, items, M)
    info = check(gpu, q, items, recs, names_for(len(items)), mode, color=(M == 2))
    assert info.scans == 1 and info.total_records > sum(r.shape[0] for r in recs) > 0


@pytest.mark.parametrize("idx", range(5), ids=[s.name for s in classes(False)])
def test_count_prints_min_count_m(gpu, idx):
    s = classes(False)[idx]
    items = shaped_items(s)[:24]
    for M in (1, 3):
        q = limited(s, M, count_lines=True)
        counts = [int(bm.reference(gpu, q, it)[0]) for it in items]
        assert 0 in counts and M in counts
        check(gpu, q, items, [bm.NONE] * len(items), names_for(len(items)), "count", False, counts)


def test_kmp_extra_record_is_not_printed(gpu):
    s = S("kmp_search", [b"abab"], algo_override=abi.ALGO_KMP, alphabet=b"ab \n")
    items = [arr(b"abab x\n" * T) for T in (2, 3, 4, 9)] + [arr(b"")]
    q = limited(s, 3)
    q.configure(gpu)
    try:
        found = gpu.search_batch(q.params(), items)
    finally:
        gpu.set_thread_config(None)
    assert [p.shape[0] for _, p in found] == [2, 3, 4, 4, 0]  # the search keeps it ...
    recs = search_file_lists(gpu, q, items, 3, operator_every=1)
    assert [r.shape[0] for r in recs] == [2, 3, 3, 3, 0]       # ... search_file() drops it
    for mode in ("lines", "matches"):
        qq = limited(S(s.name, s.pats, only_matching=(mode == "matches"), algo_override=abi.ALGO_KMP, alphabet=s.alphabet), 3)
        check(gpu, qq, items, recs, names_for(len(items)), mode, False)


def test_memchr_prints_the_sorted_set(gpu):
    s = S("single byte", [b"a"], alphabet=b"ab\n")
    items = [arr(b"a\n" * n) for n in (4095, 4096, 4097, 6000)]
    q = limited(s, 4096)
    recs = search_file_lists(gpu, q, items, 4096, operator_every=1)
    assert recs[2][-1, 0] == 2 * 4096 and recs[2][-2, 0] == 2 * 4094  # R[M] behind R[M-2]: R[M-1] is not printed
    check(gpu, q, items, recs, names_for(4), "lines", False)
    check(gpu, limited(S(s.name, s.pats, only_matching=True, alphabet=s.alphabet), 4096), items, recs, names_for(4), "matches", True)
    big = [arr(b"a\n" * 8193), arr(b"a a\n")]
    q = limited(s, 8192)
    check(gpu, q, big, search_file_lists(gpu, q, big, 8192, operator_every=1), names_for(2), "lines", False)


ZERO = [
    S("boyer_moore_search", [b"aXbY"], level=abi.REF_SCALAR, alphabet=b"abXY\n", plants=[b"aXbY"]),
    S("memchr_short_search", [b"ab"], case_sensitive=False, alphabet=b"abAB \n", plants=[b"aB"]),
    S("memchr_search", [b"a"], alphabet=b"ab\n", plants=[b"a"]),
    S("kmp_search", [b"abab"], level=abi.REF_SCALAR, alphabet=b"ab \n", plants=[b"abab"]),
    S("dictionary", NESTED, alphabet=b"abcdehrs \n", plants=[b"ushers"]),
    S("ab|abc", [b"ab|abc"], regex=True, alphabet=b"abc\n", plants=[b"abc"]),
]


@pytest.mark.parametrize("s", ZERO, ids=lambda s: s.name)
def test_the_zero_corner_prints_zero(gpu, s):
    items = [arr(s.plants[0] + b" x\n" + s.plants[0]), arr(b""), arr(b"zz")]
    names = [b"f0", b"f1", b"f2"]
    for extra in (dict(count_lines=True), dict(count_lines=True, only_match=True, track_positions=False)):
        got, per = grep(gpu, limited(s, 0, **extra), items, names)
        assert got == b"f0:0\nf1:0\nf2:0\n" and [c for c, _, _ in per] == [0, 0, 0]
    got, per = grep(gpu, limited(s, 0), items, names)
    assert got == b"" and per == [(0, 0, 0)] * 3


@pytest.mark.parametrize("M", [1, 2])
def test_a_dictionary_prints_the_first_by_end_in_start_order(gpu, M):
    s = S("nested dictionary", NESTED, alphabet=b"abcdehrs \n")
    items = [arr(b"abcd"), arr(b"x abcd ushers\nabcd"), arr(b""), arr(b"ushers"), arr(b"bc abcd")]
    q = limited(s, M)
    recs = search_file_lists(gpu, q, items, M, operator_every=1)
    assert recs[0].tolist() == [[1, 3], [2, 3]][:M]
    check(gpu, q, items, recs, names_for(len(items)), "lines", True)
    o = limited(S(s.name, s.pats, only_matching=True, alphabet=s.alphabet), M)
    check(gpu, o, items, search_file_lists(gpu, o, items, M, operator_every=1), names_for(len(items)), "matches", False)
    if M == 2:  # two lines, and kept records that lie on one line
        items = [arr(b"bc\nabcd"), arr(b"abcd c")]
        recs = search_file_lists(gpu, o, items, M, operator_every=1)
        check(gpu, o, items, recs, [b"p", b"q"], "matches", False)


def test_skew_one_item_holds_every_record(gpu):
    s = S("single byte", [b"a"], alphabet=b"a\n")
    items = [arr(b"") if k % 2 else arr(b"xyz\nzz") for k in range(201)]
    line = np.full(64, 97, dtype=np.uint8)
    line[-1] = 10
    items[100] = np.tile(line, (1 << 20) // 64)
    q = limited(s, 1)
    recs = [bm.NONE] * 201
    recs[100] = np.array([[0, 1]], dtype=np.uint64)
    info = check(gpu, q, items, recs, names_for(201), "lines", False)
    assert info.total_records == (1 << 20) - (1 << 14)
    got, per = grep(gpu, q, items, names_for(201))
    assert len(got) == len(names_for(201)[100]) + 1 + 64


@pytest.mark.parametrize("n_items,home", [(4095, 0), (4096, 1)])
def test_the_table_in_lds_and_in_global_memory(gpu, n_items, home):
    s = S("single byte", [b"a"], alphabet=b"ab\n")
    rng = np.random.RandomState(n_items)
    items = [bm.random_item(rng, s, int(rng.randint(0, 12))) for _ in range(n_items)]
    q = limited(s, 1)
    recs = search_file_lists(gpu, q, items, 1, operator_every=1000)
    before = gpu.batch_cut_launches()
    check(gpu, q, items, recs, names_for(n_items), "lines", False)
    after = gpu.batch_cut_launches()
    assert after[home] == before[home] + 1 and after[1 - home] == before[1 - home]
    grep(gpu, s, items, names_for(n_items))  # (no max_count: no launch)
    grep(gpu, limited(s, 1, count_lines=True), items, names_for(n_items))  # (COUNT keeps no record: no launch)
    assert gpu.batch_cut_launches() == after


@pytest.mark.parametrize("mode", ["lines", "matches", "count"])
def test_several_packs_equal_one_pack(gpu, mode):
    s = classes(mode == "matches")[3]
    q = limited(s, 2, count_lines=True) if mode == "count" else limited(s, 2)
    rng = np.random.RandomState(9)
    items = [bm.random_item(rng, s, int(n)) for n in rng.randint(0, 6000, size=120)]
    names = names_for(len(items))
    one, per_one, info_one = grep(gpu, q, items, names, want_info=True)
    gpu.batch_pack_limit(64 << 10)
    try:
        many, per_many, info = grep(gpu, q, items, names, want_info=True)
    finally:
        gpu.batch_pack_limit(0)
    assert info_one.scans == 1 and info.scans > 1 and many == one and per_many == per_one and len(one) > 500
    assert info.total_records == info_one.total_records


def test_bytes_are_appended_behind_what_out_holds(gpu):
    p = abi.Params([b"ab"], max_count=1)
    rc, per, out = raw_call(gpu, p, [b"xab ab\nab", b"", b"ab"], [b"a", b"b", b"c"])
    assert rc == 0 and per == [(1, 0, 9), (0, 9, 0), (1, 9, 5)] and out[1] == 5 + 14 and out[3][:5] == b"12345"


@pytest.mark.parametrize("kind", [1, 2, 3, 4])
def test_injected_failures_leave_the_output_untouched(gpu, kind):
    s = limited(classes(False)[3], 1)
    items = [b"xx Sherlock yy\nlock", b"", b"er\n"]
    names = [b"a", b"b", b"c"]
    want, _ = grep(gpu, s, items, names)
    assert want == b"a:xx Sherlock yy\nc:er\n"
    gpu.inject_failure(kind)
    try:
        rc, per, out = raw_call(gpu, s.params(), items, names, cfg=s.config(gpu))
        assert rc == 2 and gpu.last_error()
        assert per == [(POISON,) * 3] * 3 and out[1] == 5 and out[3][:5] == b"12345"
        with pytest.raises(KrepGpuError):
            grep(gpu, s, items, names)
    finally:
        gpu.inject_failure(0)
    assert grep(gpu, s, items, names)[0] == want


def test_reuse_limited_unlimited_limited(gpu):
    s = classes(False)[3]
    rng = np.random.RandomState(4)
    large = [bm.random_item(rng, s, int(n)) for n in rng.randint(0, 9000, size=300)]
    small = large[:10]
    names = names_for(len(large))
    a = grep(gpu, limited(s, 2), large, names)
    free = grep(gpu, s, large, names)
    b = grep(gpu, limited(s, 1), small, names[:10])
    c = grep(gpu, limited(s, 2), large, names)
    assert a == c and len(free[0]) > len(a[0]) > len(b[0]) > 0
    assert grep(gpu, s, large, names) == free
    q = limited(s, 2)
    check(gpu, q, large, search_file_lists(gpu, q, large, 2, operator_every=60), names, "lines", False)


@pytest.mark.parametrize("M", [10, 11])
def test_the_o_stale_rule_sees_the_cut_count(gpu, M):
    """30 matches, 22 of them behind the item's last newline: at -m 10 the list holds 10 records and every number is true; at -m 11 it
    holds more than 10 and the records behind the last newline print the stale number"""
    s = S("literal", [b"ab"], only_matching=True, force_no_simd=True, alphabet=b"ab \n")
    items = [arr(b"ab x\n" * 8 + b"ab " * 22), arr(b"ab x\n" * 3 + b"ab ab")]
    q = limited(s, M)
    recs = search_file_lists(gpu, q, items, M, operator_every=1)
    assert recs[0].shape[0] == M
    check(gpu, q, items, recs, [b"f", b"g"], "matches", False)
    got, _ = grep(gpu, q, items, [b"f", b"g"])
    last = [ln for ln in got.splitlines() if ln.startswith(b"f:")][-1]
    assert last.startswith(b"f:9:" if M == 10 else b"f:8:")
