"""krep_gpu_grep_batch for loops regexes (krep -E with *, + and {n,}; krep_gpu_set_regex_loops): what `krep -E [-o | -c] PATTERN`
prints for every item of a batch, from the device.  Expected bytes: tests/batch_grep_model.py definition() fed per item with the
compiled reference's records for the item ALONE.  Every mode plain and coloured with the (offset, nbytes) table and the counts;
several packs; the dense road of the filter scan inside a pack; a refused search; a scan that fails in the middle of a batch; -m N
with krep_gpu_set_batch_max_count as well.  The module turns the switches on and, whatever happens, off again.  Each test uses a few
hundred KiB at most."""
import numpy as np
import pytest

import batch_grep_model as bg
import batch_model as bm
import only_matching_model as om
import regex_loops_output_cases as lc
import regex_ref
from krep_amd.engine import KrepGpuError
from test_abi_grep_batch import POISON, raw_call
from test_gpu_batch_format import names_for
from test_gpu_grep_batch_max_count import limited
from test_gpu_regex_loops import AUTO, background, put_line, word_text

pytestmark = pytest.mark.gpu

S = bm.Search
N_ITEMS, EMPTY, OPEN, LONG, MANY = 60, 7, 11, 23, 31  # the batch of sixty and the items with a shape of their own
BATCH_KEYS = ["a+b", "error-timeout", "eol", "bol", "inner"]


@pytest.fixture(autouse=True, scope="module")
def _c_locale():
    with regex_ref.c_locale():
        yield


@pytest.fixture(scope="module")
def gpu():
    import krep_amd
    e = krep_amd.load()
    assert e.device_count() >= 1 and e.available(), e.unavailable_reason()
    assert regex_ref.available(), "the compiled reference (oracle/_ref/libkrep_ref_avx2.so) is missing"
    assert not e.get_regex_loops() and not e.get_batch_max_count()
    e.set_regex_loops(True)
    try:
        yield e
    finally:
        e.set_regex_loops(False)
        e.set_batch_max_count(False)
        e.force_regex_loops_road(AUTO)
        e.batch_pack_limit(0)
        e.inject_failure(0)
        e.set_thread_config(None)


def search(row, only_matching=False) -> bm.Search:
    return S(row.key, row.pats, only_matching=only_matching, regex=True, alphabet=row.alphabet + b"\n", case_sensitive=row.cs)


def arr(b) -> np.ndarray:
    return np.frombuffer(bytes(b), dtype=np.uint8)


def sixty_items(row):
    """sixty items of 0 .. 600 bytes over the row's alphabet with its lines and decoys put in; an empty item; an item without any
    newline whose match ends it; an item that is one 4096-byte line with a 3000-byte match; an item of 13 lines without a final
    newline (13 records or more: the per-item stale rule, its last line's records behind the item's last newline)"""
    rng = np.random.RandomState(600 + lc.ROWS.index(row))
    extra = row.lines + row.decoys
    items = []
    for k in range(N_ITEMS):
        t = background(rng, int(rng.randint(0, 601)), row.alphabet + b"\n")
        for j in range(int(rng.randint(0, 4))):
            line = extra[(k + j) % len(extra)]
            if t.size > len(line) + 2:
                put_line(t, int(rng.randint(1, t.size - len(line))), line)
        items.append(t)
    tail = lc.tail_line(row)[0]
    long_match = row.make(3000)
    items[EMPTY] = np.zeros(0, dtype=np.uint8)
    items[OPEN] = arr(tail)
    items[LONG] = arr(lc.cyc(lc.QUIET, 1096) + long_match if row.eol else long_match + lc.cyc(lc.QUIET, 1096))
    items[MANY] = arr(b"\n".join([tail] * 13))
    assert items[LONG].size == 4096 and 10 not in items[LONG] and 10 not in items[OPEN]
    return items


_REF = {}


def reference_records(gpu, row, items, what):
    """the reference's records per item, once per (row, batch) and shared"""
    key = (row.key, what)
    if key not in _REF:
        s = search(row)
        _REF[key] = [np.asarray(bm.reference(gpu, s, it)[1], dtype=np.uint64).reshape(-1, 2) for it in items]
    return _REF[key]


def grep(gpu, s, items, names, color=False, want_info=False):
    return gpu.grep_batch(s.params(), items, names, color=color, cfg=s.config(gpu), want_info=want_info)


def check(gpu, s, items, recs, names, mode, color, counts=None):
    want, where = bg.definition(items, recs, names, mode, color, counts)
    got, per, info = grep(gpu, s, items, names, color, want_info=True)
    assert got == want, (s, mode, color, len(got), len(want), next((k for k in range(len(want)) if got[k:k + 1] != want[k:k + 1]), None))
    assert [(o, n) for _, o, n in per] == where
    assert [c for c, _, _ in per] == ([r.shape[0] for r in recs] if counts is None else counts)
    return info


@pytest.mark.parametrize("mode", ["lines", "matches", "count"])
@pytest.mark.parametrize("key", BATCH_KEYS)
def test_every_mode_of_a_batch_of_sixty(gpu, key, mode):
    row = lc.BY_KEY[key]
    items = sixty_items(row)
    recs = reference_records(gpu, row, items, "sixty")
    # what the batch holds, by the reference alone
    assert recs[EMPTY].shape[0] == 0 and recs[OPEN][-1, 1] == items[OPEN].size
    assert [int(e - s) for s, e in recs[LONG]] == [3000]
    last_nl = int(np.flatnonzero(items[MANY] == 10)[-1])
    assert recs[MANY].shape[0] >= 12 > om.STALE_AFTER and (recs[MANY][:, 0] > last_nl).sum() == len(row.tail)
    assert sum(1 for r in recs if r.shape[0]) >= 20
    names = names_for(N_ITEMS)
    if mode == "count":
        s = search(row).with_lines()
        counts = [int(bm.reference(gpu, s, it)[0]) for it in items]
        assert 0 in counts and counts[MANY] == 13 and counts[LONG] == 1
        for color in (False, True):
            check(gpu, s, items, [bm.NONE] * N_ITEMS, names, "count", color, counts)
        return
    s = search(row, only_matching=(mode == "matches"))
    assert gpu.batch_can_accelerate(s.params()), gpu.last_error()
    for color in (False, True):
        info = check(gpu, s, items, recs, names, mode, color)
        assert info.scans == 1 and info.total_records == sum(r.shape[0] for r in recs)


@pytest.mark.parametrize("mode", ["lines", "matches"])
def test_several_packs_equal_one_pack(gpu, mode):
    row = lc.BY_KEY["decimal"]
    s = search(row, only_matching=(mode == "matches"))
    rng = np.random.RandomState(9)
    items = [background(rng, int(n), row.alphabet + b"\n") for n in rng.randint(0, 6000, size=120)]
    names = names_for(len(items))
    recs = reference_records(gpu, row, items, "packs")
    info_one = check(gpu, s, items, recs, names, mode, False)
    one, per_one = grep(gpu, s, items, names)
    assert info_one.scans == 1 and len(one) > 1000
    gpu.batch_pack_limit(64 << 10)
    try:
        many, per_many, info = grep(gpu, s, items, names, want_info=True)
    finally:
        gpu.batch_pack_limit(0)
    assert info.scans > 1 and many == one and per_many == per_one and info.total_records == info_one.total_records
    at = 0
    for _, o, n in per_many:  # the items' bytes follow one another without a gap, across the packs
        assert o == at
        at += n
    assert at == len(many)


def test_the_dense_road_in_a_pack(gpu):
    """[a-z]+ over thirty items of word text: the filter occurs on most bytes, the filter scan of the pack takes the dense road"""
    row = lc.BY_KEY["words"]
    rng = np.random.RandomState(30)
    items = [word_text(rng, int(n)) for n in rng.randint(500, 4000, size=30)]
    recs = reference_records(gpu, row, items, "dense")
    names = names_for(len(items))
    assert sum(r.shape[0] for r in recs) > 5000
    for mode in ("matches", "lines"):
        before = gpu.regex_loops_roads()
        check(gpu, search(row, only_matching=(mode == "matches")), items, recs, names, mode, mode == "lines")
        after = gpu.regex_loops_roads()
        assert after[1] > before[1] and after[0] == before[0], (mode, before, after)


def test_a_refused_search_stays_refused(gpu):
    """$ under -i: the end of the text does not end a line there (REG_NOTEOL), an item's end would"""
    s = S("b+$ -i", [b"b+$"], regex=True, alphabet=b"abb \n", case_sensitive=False)
    assert not gpu.batch_can_accelerate(s.params())
    why = gpu.last_error()
    assert why
    with pytest.raises(KrepGpuError) as err:
        grep(gpu, s, [b"abb", b"a\nbb"], [b"one", b"two"])
    assert why in str(err.value)
    rc, per, out = raw_call(gpu, s.params(), [b"abb", b"a\nbb"], [b"one", b"two"], cfg=s.config(gpu))
    assert rc == 2 and gpu.last_error() == why and per == [(POISON,) * 3] * 2 and out == (True, 5, 8, b"12345678")


def test_a_scan_that_fails_inside_a_batch_leaves_the_output_untouched(gpu):
    """one item holds a candidate line of 4097 bytes: the call returns 2 with the scan's reason, out->len and per_item are untouched
    (include/krep_gpu.h, "the grep output of a batch"), and the next call without that item succeeds"""
    row = lc.BY_KEY["a+b"]
    s = search(row)
    good = [arr(b"xaab ab\nab"), arr(b""), arr(b"c ab\n"), arr(b"aaab")]
    bad = good[:2] + [arr(b"c ab\n" + b"a" * 4096 + b"b\nab")] + good[2:]
    names = [b"n%d" % k for k in range(5)]
    rc, per, out = raw_call(gpu, s.params(), bad, names, cfg=s.config(gpu))
    assert rc == 2 and "4096" in gpu.last_error(), gpu.last_error()
    assert per == [(POISON,) * 3] * 5 and out[1] == 5 and out[3][:5] == b"12345"  # out->len and the bytes in front of it
    with pytest.raises(KrepGpuError, match="4096"):
        grep(gpu, s, bad, names)
    recs = [np.asarray(bm.reference(gpu, s, it)[1], dtype=np.uint64).reshape(-1, 2) for it in good]
    for mode in ("lines", "matches"):
        check(gpu, search(row, only_matching=(mode == "matches")), good, recs, names[:4], mode, True)


@pytest.mark.parametrize("M", [1, 3])
@pytest.mark.parametrize("key", ["a+b", "colou*r"])
def test_max_count_in_a_batch(gpu, key, M):
    """krep -r -m N: every item's list cut to its first N records on the device; total_records stays the uncut number"""
    row = lc.BY_KEY[key]
    items = sixty_items(row)
    uncut = reference_records(gpu, row, items, "sixty")
    names = names_for(N_ITEMS)
    gpu.set_batch_max_count(True)
    try:
        for mode in ("lines", "matches"):
            q = limited(search(row, only_matching=(mode == "matches")), M)
            recs = [np.asarray(bm.reference(gpu, q, it)[1], dtype=np.uint64).reshape(-1, 2)[:M] for it in items]
            assert all(np.array_equal(r, u[:M]) for r, u in zip(recs, uncut)) and any(u.shape[0] > M for u in uncut)
            info = check(gpu, q, items, recs, names, mode, mode == "matches")
            assert info.total_records == sum(u.shape[0] for u in uncut) > sum(r.shape[0] for r in recs)
    finally:
        gpu.set_batch_max_count(False)
    assert not gpu.get_batch_max_count() and gpu.get_regex_loops()
