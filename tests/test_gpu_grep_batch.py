"""krep_gpu_grep_batch: what `krep [-o | -c] PATTERN` prints for every item of a batch, from the device (kg_batch.hip,
kg_batch_format.hip).  Expected bytes: tests/batch_grep_model.py definition() fed per item with the reference's records
(batch_model.reference).  Searches: a literal, -i, -w, a nested dictionary (the order-by-start step, repeated bytes in lines mode) and a
regex alternation; plain and colour strings for both forms; COUNT with zero counts and empty items; several packs; failure injection;
reuse of one engine with a larger and a smaller batch, krep_gpu_search_batch before and after.  Each test uses a few MiB at most."""
import numpy as np
import pytest

import batch_grep_model as bg
import batch_model as bm
import regex_ref
from krep_amd.engine import KrepGpuError
from test_abi_grep_batch import POISON, raw_call
from test_gpu_batch_format import classes, names_for, reference_records, shaped_items

pytestmark = pytest.mark.gpu

S = bm.Search


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


def grep(gpu, s, items, names, color=False, want_info=False):
    return gpu.grep_batch(s.params(), items, names, color=color, cfg=s.config(gpu), want_info=want_info)


def check(gpu, s, items, recs, names, mode, color, counts=None):
    want, where = bg.definition(items, recs, names, mode, color, counts)
    got, per, info = grep(gpu, s, items, names, color, want_info=True)
    assert got == want, (s, mode, color, len(got), len(want), next((k for k in range(len(want)) if got[k:k + 1] != want[k:k + 1]), None))
    assert [(o, n) for _, o, n in per] == where
    assert [c for c, _, _ in per] == ([r.shape[0] for r in recs] if counts is None else counts)
    return info


@pytest.mark.parametrize("color", [False, True], ids=["plain", "color"])
@pytest.mark.parametrize("mode", ["lines", "matches"])
@pytest.mark.parametrize("idx", range(5), ids=[s.name for s in classes(False)])
def test_edge_shapes(gpu, idx, mode, color):
    s = classes(mode == "matches")[idx]
    items = shaped_items(s)
    recs = reference_records(gpu, s, items, (idx, mode == "matches"))
    info = check(gpu, s, items, recs, names_for(len(items)), mode, color)
    assert info.scans == 1 and info.total_records == sum(r.shape[0] for r in recs)


@pytest.mark.parametrize("idx", range(5), ids=[s.name for s in classes(False)])
def test_count_prints_every_item(gpu, idx):
    """-c: FILE:COUNT for every item, zero counts and empty items included; colour does not touch it (krep.c:3016)"""
    s = classes(False)[idx].with_lines()
    items = shaped_items(s)[:24]
    counts = [int(bm.reference(gpu, s, it)[0]) for it in items]
    assert 0 in counts and any(counts) and any(bm.as_array(it).size == 0 for it in items)
    recs = [bm.NONE] * len(items)
    for color in (False, True):
        check(gpu, s, items, recs, names_for(len(items)), "count", color, counts)


@pytest.mark.parametrize("mode", ["lines", "matches", "count"])
def test_several_packs_equal_one_pack(gpu, mode):
    s = classes(mode == "matches")[3]  # the nested dictionary: every pack is ordered by start
    s = s.with_lines() if mode == "count" else s
    rng = np.random.RandomState(9)
    items = [bm.random_item(rng, s, int(n)) for n in rng.randint(0, 6000, size=120)]
    names = names_for(len(items))
    one, per_one, info_one = grep(gpu, s, items, names, want_info=True)
    assert info_one.scans == 1 and len(one) > 1000
    gpu.batch_pack_limit(64 << 10)
    try:
        many, per_many, info = grep(gpu, s, items, names, want_info=True)
    finally:
        gpu.batch_pack_limit(0)
    assert info.scans > 1 and many == one and per_many == per_one
    at = 0
    for _, o, n in per_many:  # the items' bytes follow one another without a gap, across the packs
        assert o == at
        at += n
    assert at == len(many)


@pytest.mark.parametrize("kind", [1, 2, 3, 4])
def test_injected_failures_leave_the_output_untouched(gpu, kind):
    s = classes(False)[3]
    items = [b"xx Sherlock yy\nlock", b"", b"er\n"]
    names = [b"a", b"b", b"c"]
    want, _ = grep(gpu, s, items, names)
    assert want
    gpu.inject_failure(kind)
    try:
        rc, per, out = raw_call(gpu, s.params(), items, names, cfg=s.config(gpu))
        assert rc == 2 and gpu.last_error()
        assert per == [(POISON,) * 3] * 3 and out[1] == 5 and out[3][:5] == b"12345"  # out->len and the bytes in front of it
        with pytest.raises(KrepGpuError):
            grep(gpu, s, items, names)
    finally:
        gpu.inject_failure(0)
    assert grep(gpu, s, items, names)[0] == want  # the next call succeeds


def test_reuse_with_a_larger_then_a_smaller_batch(gpu):
    s = classes(False)[0]
    om = classes(True)[0]
    rng = np.random.RandomState(4)
    small = [bm.random_item(rng, s, int(n)) for n in rng.randint(0, 300, size=10)]
    large = [bm.random_item(rng, s, int(n)) for n in rng.randint(0, 9000, size=400)]
    s.configure(gpu)
    try:
        before = gpu.search_batch(s.params(), large)
    finally:
        gpu.set_thread_config(None)
    for items in (small, large, small):
        for q, mode in ((s, "lines"), (om, "matches")):
            recs = [np.asarray(bm.reference(gpu, q, it)[1], dtype=np.uint64).reshape(-1, 2) for it in items]
            check(gpu, q, items, recs, names_for(len(items)), mode, True)
    s.configure(gpu)
    try:
        after = gpu.search_batch(s.params(), large)
    finally:
        gpu.set_thread_config(None)
    assert len(before) == len(after) and all(a[0] == b[0] and np.array_equal(a[1], b[1]) for a, b in zip(before, after))


@pytest.mark.parametrize("n_items", [4095, 4097])
def test_many_small_items(gpu, n_items):
    s = S("single byte", [b"a"], alphabet=b"ab\n")
    rng = np.random.RandomState(n_items)
    texts = [b"", b"a", b"ba\n", b"xa\na", b"zz", b"a\n\na"]
    items = [texts[int(k)] for k in rng.randint(0, len(texts), size=n_items)]
    recs = [np.array([(k, k + 1) for k, c in enumerate(t) if c == 97], dtype=np.uint64).reshape(-1, 2) for t in items]
    names = [b"%d" % (k % 97) for k in range(n_items)]
    lds0, glob0 = gpu.batch_format_launches()
    check(gpu, s, items, recs, names, "lines", False)
    lds1, glob1 = gpu.batch_format_launches()
    assert (lds1 - lds0, glob1 - glob0) == ((1, 0) if n_items + 1 <= 4096 else (0, 1))  # one analysis per pack, no size query
