"""The order of the refusals of krep_gpu_search_batch and krep_gpu_grep_batch (kg_batch.hip, "what both calls share":
BatchWalk::enter and the calls' own checks).  Host logic only, no GPU: KREP_GPU_ASSUME_AVAILABLE=1 lets a call pass the device step, KREP_GPU_DISABLE=1 makes that step the fault.

Every case presents TWO faults at once and asserts that the earlier one of the documented order is the reason reported, with status 2
and with results / per_item / out / records->count untouched.  All pairs of faults that can be built are run (so every adjacent pair
and every non-adjacent one), plus the pairs across two items of krep_gpu_grep_batch's one loop.  The reason substrings below were
read off the library as it stood BEFORE the entry was folded into one step; they are literals on purpose.

search_batch:  1 NULL params / items / results   2 the batch rule   3 "no pattern"   4 an item with a NULL text and a length
               5 no usable device   6 n_items == 0 -> 0   7 no trie -> zeros
grep_batch:    1 NULL params / items / fmt / per_item / out   2 the batch rule   3 "no pattern"   4 track_positions false outside -c
               5 a prefix in fmt->line / fmt->match   6 a format string NULL with a length   7 per item: NULL text, then its prefix
               8 out->len > capacity   9 no usable device   10 n_items == 0 -> 0

What cannot be built: step 3 on its own.  A search without a pattern is refused by the batch rule already (kg::unsupported_reason
answers "no pattern" for it before any other rule is asked, and several patterns with NULL arrays get its "several patterns
announced" text), so the pair (2, 3) does not exist and "no pattern" below stands for steps 2 and 3 alike: one params struct either
has a pattern or has none.  Steps 6 and 7 of search_batch and step 10 of grep_batch are answers, not faults: they are checked against
the device step in front of them (0 with a device assumed, 2 without one)."""
import ctypes as C
import itertools

import pytest

import krep_amd
from krep_amd import abi

POISON = 0xDEADBEEF
ITEMS = [b"xabx", b"a\nb"]
NO_DEVICE = "disabled by KREP_GPU_DISABLE"

# fault -> the reason it is refused with, in the order of the steps
SEARCH_ORDER = [("null", "search_batch: NULL params / items / results"),
                ("rule", "batch: a pattern holds '\\n'"),
                ("nopat", "no pattern"),
                ("nulltext0", "search_batch: item 0 has a NULL text and a length of 4"),
                ("nodev", NO_DEVICE)]
GREP_ORDER = [("null", "grep_batch: NULL params / items / fmt / per_item / out"),
              ("rule", "batch: a pattern holds '\\n'"),
              ("nopat", "no pattern"),
              ("track", "grep_batch: track_positions == false outside -c"),
              ("lineprefix", "grep_batch: the prefix of fmt->line / fmt->match must be empty"),
              ("fmtstr", "grep_batch: a string of the format is NULL with a length, or longer than 2^20 bytes"),
              ("nulltext0", "grep_batch: item 0 has a NULL text and a length of 4"),
              ("prefix0", "grep_batch: the prefix of item 0 is NULL with a length"),
              ("out", "grep_batch: out holds 9 bytes in a block of 8"),
              ("nodev", NO_DEVICE)]
# the same loop one item later: item 0's second check beats item 1's first
GREP_CROSS = [(("prefix0", "nulltext1"), "grep_batch: the prefix of item 0 is NULL with a length"),
              (("nulltext0", "prefix1"), "grep_batch: item 0 has a NULL text and a length of 4"),
              (("nulltext0", "nulltext1"), "grep_batch: item 0 has a NULL text and a length of 4"),
              (("prefix0", "prefix1"), "grep_batch: the prefix of item 0 is NULL with a length")]


def pairs(order):
    return [(a, b) for a, b in itertools.combinations([f for f, _ in order], 2) if {a, b} != {"rule", "nopat"}]


def expected(order, faults):
    return next(reason for f, reason in order if f in faults)


@pytest.fixture(scope="module")
def eng():
    return krep_amd.load()


def device(monkeypatch, faults):
    if "nodev" in faults:
        monkeypatch.setenv("KREP_GPU_DISABLE", "1")
        monkeypatch.delenv("KREP_GPU_ASSUME_AVAILABLE", raising=False)
    else:
        monkeypatch.setenv("KREP_GPU_ASSUME_AVAILABLE", "1")
        monkeypatch.delenv("KREP_GPU_DISABLE", raising=False)


def params_for(faults, pats=(b"ab",)):
    pats = [] if "nopat" in faults else [b"a\nb"] if "rule" in faults else list(pats)
    return abi.Params(pats, **(dict(track_positions=False) if "track" in faults else {}))


def item_array(e, faults, items):
    arr, n, held = e.batch_items(items)
    for i in range(n):
        if "nulltext%d" % i in faults:
            arr[i].text = None  # (the length stays)
    return arr, n, held


def search_call(e, faults, items=ITEMS, pats=(b"ab",), trie=True):
    """krep_gpu_search_batch with the faults built in, poisoned results and a record list that holds one record (77, 78)
    -> (rc, last_error, results, records->count, that record's start)"""
    p = params_for(faults, pats)
    arr, n, held = item_array(e, faults, items)
    res = (abi.BatchResult * max(n, 1))()
    for r in res:
        r.count = r.first_record = r.n_records = POISON
    rec = e.lib.krep_gpu_match_result_init(16)
    rec.contents.positions[0].start_offset, rec.contents.positions[0].end_offset = 77, 78
    rec.contents.count = 1
    dummy = C.c_int(0)
    if trie and p.s.num_patterns > 1:
        p.s.ac_trie = C.cast(C.pointer(dummy), C.c_void_p)
    try:
        rc = e.lib.krep_gpu_search_batch(p.ref, None, arr, n, None if "null" in faults else res, rec, None)
        return (rc, e.last_error(), [(r.count, r.first_record, r.n_records) for r in res[:n]], int(rec.contents.count),
                int(rec.contents.positions[0].start_offset))
    finally:
        p.s.ac_trie = None
        e.lib.krep_gpu_match_result_free(rec)
        del held


def grep_call(e, faults, items=ITEMS, pats=(b"ab",), trie=True):
    """krep_gpu_grep_batch with the faults built in, poisoned per_item and an `out` of 8 bytes that already holds 5 (9 under "out")
    -> (rc, last_error, per_item, (the block is where it was, out->len, out->capacity, its 8 bytes))"""
    libc = C.CDLL(None)
    libc.malloc.restype, libc.malloc.argtypes, libc.free.restype, libc.free.argtypes = C.c_void_p, [C.c_size_t], None, [C.c_void_p]
    p = params_for(faults, pats)
    arr, n, held = item_array(e, faults, items)
    fmt, keep = e.grep_format([b"f%d" % i for i in range(n)], "lines")
    pre, lens = keep[0], keep[1]
    for i in range(n):
        if "prefix%d" % i in faults:
            pre[i], lens[i] = None, 3
    if "lineprefix" in faults:
        fmt.line.prefix, fmt.line.prefix_len = b"x:", 2
    if "fmtstr" in faults:
        fmt.match.after_number, fmt.match.after_number_len = None, 3
    per = (abi.GrepItem * max(n, 1))()
    for q in per:
        q.count = q.out_offset = q.out_bytes = POISON
    block = libc.malloc(8)
    C.memmove(block, b"12345678", 8)
    out = abi.GrepOutput(block, 9 if "out" in faults else 5, 8)
    dummy = C.c_int(0)
    if trie and p.s.num_patterns > 1:
        p.s.ac_trie = C.cast(C.pointer(dummy), C.c_void_p)
    try:
        rc = e.lib.krep_gpu_grep_batch(p.ref, None, arr, n, C.byref(fmt), None if "null" in faults else per, C.byref(out), None)
        state = (out.bytes == block, out.len, out.capacity, C.string_at(out.bytes, 8))
        return rc, e.last_error(), [(q.count, q.out_offset, q.out_bytes) for q in per[:n]], state
    finally:
        p.s.ac_trie = None
        libc.free(out.bytes)
        del held, keep


def search_untouched(res, count, first, n):
    return res == [(POISON,) * 3] * n and count == 1 and first == 77


def grep_untouched(per, state, n, faults=()):
    return per == [(POISON,) * 3] * n and state == (True, 9 if "out" in faults else 5, 8, b"12345678")


@pytest.mark.parametrize("faults", pairs(SEARCH_ORDER), ids="+".join)
def test_search_batch_reports_the_earlier_of_two_faults(eng, monkeypatch, faults):
    device(monkeypatch, faults)
    rc, why, res, count, first = search_call(eng, faults)
    assert rc == 2 and expected(SEARCH_ORDER, faults) in why, (faults, why)
    assert search_untouched(res, count, first, len(ITEMS)), (faults, res, count, first)


@pytest.mark.parametrize("faults", pairs(GREP_ORDER), ids="+".join)
def test_grep_batch_reports_the_earlier_of_two_faults(eng, monkeypatch, faults):
    device(monkeypatch, faults)
    rc, why, per, state = grep_call(eng, faults)
    assert rc == 2 and expected(GREP_ORDER, faults) in why, (faults, why)
    assert grep_untouched(per, state, len(ITEMS), faults), (faults, per, state)


@pytest.mark.parametrize("faults,reason", GREP_CROSS, ids=["+".join(f) for f, _ in GREP_CROSS])
def test_grep_batch_checks_text_and_prefix_of_an_item_in_one_loop(eng, monkeypatch, faults, reason):
    device(monkeypatch, faults)
    rc, why, per, state = grep_call(eng, faults)
    assert rc == 2 and reason in why, (faults, why)
    assert grep_untouched(per, state, len(ITEMS)), (faults, per, state)


def test_search_batch_item_1_alone_is_named(eng, monkeypatch):
    device(monkeypatch, ())
    rc, why, res, count, first = search_call(eng, ("nulltext1",))
    assert rc == 2 and "search_batch: item 1 has a NULL text and a length of 3" in why, why
    assert search_untouched(res, count, first, 2)


def test_an_empty_batch_is_answered_behind_the_device_step(eng, monkeypatch):
    device(monkeypatch, ())
    rc, why, _, count, first = search_call(eng, (), items=[])
    assert rc == 0 and not why and count == 1 and first == 77
    rc, why, _, state = grep_call(eng, (), items=[])
    assert rc == 0 and not why and state == (True, 5, 8, b"12345678")
    device(monkeypatch, ("nodev",))
    rc, why, _, count, first = search_call(eng, ("nodev",), items=[])
    assert rc == 2 and NO_DEVICE in why and count == 1 and first == 77
    rc, why, _, state = grep_call(eng, ("nodev",), items=[])
    assert rc == 2 and NO_DEVICE in why and state == (True, 5, 8, b"12345678")
    # and behind every refusal in front of that step
    device(monkeypatch, ())
    rc, why, _, count, first = search_call(eng, ("rule",), items=[])
    assert rc == 2 and "holds '\\n'" in why
    rc, why, _, state = grep_call(eng, ("out",), items=[])
    assert rc == 2 and "out holds 9 bytes in a block of 8" in why and state == (True, 9, 8, b"12345678")


def test_no_trie_is_answered_behind_the_device_step_and_needs_no_device_work(eng, monkeypatch):
    pats = (b"ab", b"xa")
    device(monkeypatch, ())  # (a device is assumed and none is there: an answer that touched it would fail)
    rc, why, res, count, first = search_call(eng, (), pats=pats, trie=False)
    assert rc == 0 and not why and res == [(0, 1, 0)] * 2 and count == 1 and first == 77
    rc, why, per, state = grep_call(eng, (), pats=pats, trie=False)
    assert rc == 0 and not why and per == [(0, 0, 0)] * 2 and state == (True, 5, 8, b"12345678")
    device(monkeypatch, ("nodev",))
    rc, why, res, count, first = search_call(eng, ("nodev",), pats=pats, trie=False)
    assert rc == 2 and NO_DEVICE in why and search_untouched(res, count, first, 2)
    rc, why, per, state = grep_call(eng, ("nodev",), pats=pats, trie=False)
    assert rc == 2 and NO_DEVICE in why and grep_untouched(per, state, 2)
    # an item with a NULL text is refused in front of the no-trie answer
    device(monkeypatch, ())
    rc, why, res, count, first = search_call(eng, ("nulltext0",), pats=pats, trie=False)
    assert rc == 2 and "item 0 has a NULL text" in why and search_untouched(res, count, first, 2)
