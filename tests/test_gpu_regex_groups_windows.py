"""A groups search (krep -E with repeated and nested groups: the general step of kg_regex_loops.hip) in WINDOWS, behind
krep_gpu_set_regex_loops_windows: windows cut at 4099 and 8191 bytes with 4096 bytes of context concatenate to the one-window list, -c
folds through krep_gpu_combine_line_counts, and search_buffer streams a 100 001-byte text in pieces.  The compiled reference answers
every case.  The module turns the three switches on and, whatever happens, off again."""
import numpy as np
import pytest

import regex_ref
from krep_amd import abi
from test_gpu_regex_groups import SHAPES
from test_gpu_regex_loops import AUTO, DENSE, SPARSE, expected, planted, put_line, rx
from test_gpu_regex_loops_windows import fold, scan_window

pytestmark = pytest.mark.gpu

ROWS = [0, 2, 6]  # (ab)+, ((ab)+c)+d, the IP expression
LONG = {0: b"ab" * 2048, 2: b"ababc" * 819 + b"d", 6: b"10.0.0.1 " * 455 + b"1"}  # a candidate line of exactly 4096 bytes each
_texts = {}


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
    e.set_regex_loops(True)
    e.set_regex_groups(True)
    e.set_regex_loops_windows(True)
    try:
        yield e
    finally:
        e.set_regex_loops_windows(False)
        e.set_regex_groups(False)
        e.set_regex_loops(False)
        e.force_regex_loops_road(AUTO)
        e.set_stream_chunk(0)
        e.set_thread_config(None)


def text_of(row, n=20001):
    """the row's planted text with its 4096-byte line from 6000 on, built once and left unchanged"""
    if (row, n) not in _texts:
        pats, alphabet, plants, decoys = SHAPES[row]
        assert len(LONG[row]) == 4096
        t = planted(np.random.RandomState(500 + row), n, alphabet, plants, decoys)
        for at in range(6000, n - 4200, 30000):
            put_line(t, at, LONG[row])
        t.setflags(write=False)
        _texts[row, n] = t
    return _texts[row, n]


@pytest.mark.parametrize("row", ROWS)
@pytest.mark.parametrize("piece", [4099, 8191])
def test_windows_concatenate_to_the_one_window_list_and_fold_to_its_line_count(gpu, piece, row):
    pats = SHAPES[row][0]
    text = text_of(row)
    n = int(text.size)
    want = expected(pats, text)
    want_c = expected(pats, text, count_lines=True)[0]
    assert want[0] > 12 and max(int(e - s) for s, e in want[1]) >= (4096 if row != 6 else 8)
    wins = [(lo, min(lo + piece, n)) for lo in range(0, n, piece)]
    for road in (SPARSE, DENSE):
        gpu.force_regex_loops_road(road)
        plan, plan_c = gpu.plan(rx(pats)), gpu.plan(rx(pats, count_lines=True))
        try:
            whole = scan_window(plan, text, 0, n)[1]
            assert whole == [tuple(r) for r in want[1].tolist()], (pats, road)
            got, outs = [], []
            for lo, hi in wins:
                out, rec = scan_window(plan, text, lo, hi)
                assert all(lo <= s < hi for s, _ in rec) and out.count == out.total_matches == len(rec)
                got += rec
                outs.append(scan_window(plan_c, text, lo, hi)[0])
            assert got == whole, (pats, road, len(got), len(whole))
            assert fold(gpu, outs) == want_c, (pats, road)
        finally:
            gpu.force_regex_loops_road(AUTO)
            plan.close()
            plan_c.close()


@pytest.mark.parametrize("row", ROWS)
def test_search_buffer_streams_a_text_in_pieces(gpu, row):
    pats = SHAPES[row][0]
    text = text_of(row, 100001)
    try:
        for kw in (dict(), dict(count_lines=True), dict(max_count=7)):
            want = expected(pats, text, **kw)
            assert gpu.split_mode(rx(pats, **kw), text.size) == abi.SPLIT_PIECES
            gpu.set_stream_chunk(8192)  # about a dozen pieces, each staged with 4097 bytes on both sides
            rc, cnt, pos = gpu.search_buffer(rx(pats, **kw), text)
            assert gpu.last_status() == abi.STATUS_OK, gpu.last_error()
            assert rc == 0 and cnt == want[0] and np.array_equal(pos, want[1]), (pats, kw, cnt, want[0])
        assert expected(pats, text)[0] > 30
    finally:
        gpu.set_stream_chunk(0)
