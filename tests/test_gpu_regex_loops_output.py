"""Loops plans (krep -E with *, + and {n,}; krep_gpu_set_regex_loops) through the output drivers of krep_amd/engine.py --
Plan.grep_lines plain and coloured, Plan.grep_only_matching plain and coloured, krep_gpu_format_matches' retry road -- byte for byte
against the output models on the records of the compiled reference.  The rows, their texts and the expected bytes are those of
tests/regex_loops_output_cases.py, which tests/test_regex_loops_output_cases_cpu.py pins to the stock CLI.

What the rows bring that no older plan does: records of 1 .. 4096 bytes in one list, records that touch, lines of exactly 4096 bytes,
more than 2048 records in one line, and a longest match of 4097 by which no guess of the output's size holds.  The module turns the
switch on and, whatever happens, off again."""
import functools

import numpy as np
import pytest

import color_line_model as cm
import regex_loops_output_cases as lc
import regex_ref
from krep_amd import abi
from krep_amd.engine import KrepGpuError, match_format
from test_gpu_regex_loops import AUTO, DENSE, SPARSE, background, put_line

pytestmark = pytest.mark.gpu

PAD = 0xEE
NAME = b"f.txt"
KEYS = [r.key for r in lc.ROWS]


@pytest.fixture(autouse=True, scope="module")
def _c_locale():
    """the reference runs in the C locale (it never calls setlocale()); Python's start-up put the process into the environment's"""
    with regex_ref.c_locale():
        yield


@pytest.fixture(scope="module")
def gpu():
    import krep_amd
    e = krep_amd.load()
    assert e.device_count() >= 1 and e.available(), e.unavailable_reason()
    assert regex_ref.available(), "the compiled reference (oracle/_ref/libkrep_ref_avx2.so) is missing"
    e.set_regex_loops(True)
    try:
        yield e
    finally:
        e.set_regex_loops(False)
        e.force_regex_loops_road(AUTO)
        e.force_regex_grid(0)
        e.inject_failure(0)
        e.set_thread_config(None)


def to_device(a, shift=0):
    import torch
    t = torch.full((a.size + shift + 64,), PAD, dtype=torch.uint8, device="cuda")
    t[shift:shift + a.size] = torch.from_numpy(a.copy())
    return t, t.data_ptr() + shift


@functools.lru_cache(maxsize=None)
def want(key, nl, mode, filename=NAME, max_count=None) -> bytes:
    _, raw, _, rec = lc.case(key, nl)
    return lc.expected(raw, rec, mode, filename, max_count)


def first_diff(got: bytes, expected: bytes):
    """for a failure's message: (the lengths, the first offset at which the bytes differ)"""
    n = min(len(got), len(expected))
    return len(got), len(expected), next((k for k in range(n) if got[k] != expected[k]), n)


def driver(plan, plan_o, mode, d_text, n, filename=NAME, max_count=None) -> bytes:
    if mode.startswith("o"):
        return plan_o.grep_only_matching(d_text, n, filename=filename, max_count=max_count, color=mode.endswith("color"))
    return plan.grep_lines(d_text, n, filename=filename, max_count=max_count, color=mode.endswith("color"))


def plans(gpu, row, max_count=None):
    return gpu.plan(lc.params(row, max_count)), gpu.plan(lc.params(row, max_count), only_matching=True)


# ------------------------------------------------------------------------------------------------------------ the resident text
@pytest.mark.parametrize("key", KEYS)
@pytest.mark.parametrize("road", [SPARSE, DENSE], ids=["sparse", "dense"])
def test_resident_text_through_every_output_mode(gpu, road, key):
    """grep_lines with and without a filename, coloured, grep_only_matching plain and coloured, max_count 1, 7 and beyond the count, on
    the text that ends in a newline; the text without one 3 and 13 bytes into its allocation; the filter scan forced onto each road"""
    row = lc.BY_KEY[key]
    gpu.force_regex_loops_road(road)
    plan, plan_o = plans(gpu, row)
    try:
        assert plan.longest_match() == 4097 and plan_o.longest_match() == 4097
        before = gpu.regex_loops_roads()
        text, _, _, rec = lc.case(key, True)
        hold, d_text = to_device(text)
        for mode in lc.MODES:
            for filename in (NAME, None):
                got = driver(plan, plan_o, mode, d_text, text.size, filename)
                assert got == want(key, True, mode, filename), (key, mode, filename, first_diff(got, want(key, True, mode, filename)))
            for mc in (1, 7, len(rec) + 5):
                got = driver(plan, plan_o, mode, d_text, text.size, NAME, mc)
                assert got == want(key, True, mode, NAME, mc), (key, mode, mc, first_diff(got, want(key, True, mode, NAME, mc)))
        del hold
        text = lc.case(key, False)[0]
        for shift in (3, 13):
            hold, d_text = to_device(text, shift)
            assert d_text % 16 == shift
            for mode in lc.MODES:
                got = driver(plan, plan_o, mode, d_text, text.size)
                assert got == want(key, False, mode), (key, shift, mode, first_diff(got, want(key, False, mode)))
            del hold
        after = gpu.regex_loops_roads()
        assert after[road - 1] > before[road - 1] and after[2 - road] == before[2 - road], (key, road, before, after)
    finally:
        gpu.force_regex_loops_road(AUTO)
        plan.close()
        plan_o.close()


def test_the_plan_max_count_cuts_the_list_like_the_argument(gpu):
    """max_count as the PLAN carries it (krep -m N): the scan stops the list, the drivers get no argument"""
    for key in ("a+b", "bol", "colou*r-i", "decimal"):
        row = lc.BY_KEY[key]
        text = lc.case(key, True)[0]
        hold, d_text = to_device(text)
        for mc in (1, 7):
            plan, plan_o = plans(gpu, row, mc)
            try:
                for mode in lc.MODES:
                    got = driver(plan, plan_o, mode, d_text, text.size)
                    assert got == want(key, True, mode, NAME, mc), (key, mode, mc, first_diff(got, want(key, True, mode, NAME, mc)))
            finally:
                plan.close()
                plan_o.close()
        del hold


def test_the_retry_road_of_the_only_matching_output(gpu):
    """Records of 1 and of 3800 bytes in one list: a capacity one byte short comes back as overflow with the exact size, nothing is
    written behind the capacity that was given, and the call with that size gives the right bytes"""
    import torch
    rows = [r for r in lc.ROWS if r.shortest == 1]
    assert len(rows) >= 5
    for row in rows:
        text, _, _, rec = lc.case(row.key, True)
        assert {1, 3800} <= {e - s for s, e in rec}
        expected = want(row.key, True, "o-color")
        hold, d_text = to_device(text)
        plan = gpu.plan(lc.params(row), only_matching=True)
        try:
            pos = torch.empty(2 * (len(rec) + 1), dtype=torch.int64, device="cuda")
            out = plan.scan(d_text, text.size, d_positions=pos.data_ptr(), capacity=len(rec) + 1)
            assert out.stored == len(rec) and not out.overflow
            if not lc.single(row):
                gpu.order_by_start(pos.data_ptr(), len(rec), text.size)
            fmt = match_format(NAME, True)
            short = torch.full((len(expected) + 64,), PAD, dtype=torch.uint8, device="cuda")
            res = gpu.format_matches(d_text, text.size, pos.data_ptr(), len(rec), abi.SIZE_MAX, fmt, short.data_ptr(), len(expected) - 1)
            assert res.overflow and res.out_bytes == len(expected), (row.key, res.out_bytes, len(expected))
            assert bytes(short[len(expected) - 1:].cpu().numpy()) == bytes([PAD]) * 65  # nothing behind the capacity it was given
            res = gpu.format_matches(d_text, text.size, pos.data_ptr(), len(rec), abi.SIZE_MAX, fmt, short.data_ptr(), int(res.out_bytes))
            got = bytes(short[: int(res.out_bytes)].cpu().numpy())
            assert not res.overflow and got == expected, (row.key, first_diff(got, expected))
            assert bytes(short[len(expected):].cpu().numpy()) == bytes([PAD]) * 64
        finally:
            plan.close()
        del hold


# ------------------------------------------------------------------------------------------------------------ the output's alignment
def sweep_text(row):
    """8 KiB over the row's alphabet: matches of 40 bytes at starts of every residue mod 16, matches of 1000 bytes at six residues"""
    rng = np.random.RandomState(40)
    t = lc.background(row, rng, 8192)
    starts = [(100 + 61 * k, 40) for k in range(16)] + [(1200 + 1101 * k, 1000) for k in range(6)]
    assert len({s % 16 for s, n in starts if n == 40}) == 16 and len({s % 16 for s, n in starts if n == 1000}) == 6
    for s, n in starts:
        put_line(t, s, row.make(n))
    return t, starts


@pytest.mark.parametrize("key", ["a+b", "class-c"])
def test_output_alignment_sweep(gpu, key):
    """filenames of every length 1 .. 16 and none: every record's bytes land at another offset mod 16 in the output, while the
    matches start at every offset mod 16 in the text -- the gather's 16-byte path for a chunk that lies wholly inside one match meets
    every source and output misalignment.  a+b: a long match is a run of one byte, a chunk copied from the wrong place shows only at
    the match's end; [ab]+c?: its long matches repeat with a period of 7 bytes, every chunk shows it"""
    row = lc.BY_KEY[key]
    text, starts = sweep_text(row)
    raw = text.tobytes()
    rec = [(int(s), int(e)) for s, e in lc.records(row, text)]
    assert all((s, s + n) in set(rec) for s, n in starts)
    plan, plan_o = plans(gpu, row)
    hold, d_text = to_device(text)
    try:
        for name in [None] + [b"fedcba9876543210"[:k] for k in range(1, 17)]:
            for mode in ("o", "lines-color"):
                got = driver(plan, plan_o, mode, d_text, text.size, name)
                expected = lc.expected(raw, rec, mode, name)
                assert got == expected, (name, mode, first_diff(got, expected))
    finally:
        plan.close()
        plan_o.close()
    del hold


# ------------------------------------------------------------------------------------------------------------ the cap of 2048
def test_more_records_in_a_line_than_the_coloured_line_counts(gpu):
    """4096, 2049, 2048 one-byte records, 2048 records with a blank between them and 1365 touching records in one line, in all four
    modes; the 2049th record is one more -o line and adds only its own, uncoloured byte to the coloured line"""
    got = {}
    for cap in lc.CAPS:
        plan, plan_o = plans(gpu, cap)
        try:
            for nl in (True, False):
                text, raw, rec = lc.cap_case(cap.key, nl)
                hold, d_text = to_device(text, 5)
                for mode in lc.MODES:
                    g = driver(plan, plan_o, mode, d_text, text.size)
                    expected = lc.expected(raw, rec, mode, NAME)
                    assert g == expected, (cap.key, nl, mode, first_diff(g, expected))
                    got[cap.key, nl, mode] = g
                del hold
        finally:
            plan.close()
            plan_o.close()
    for nl in (True, False):
        for mode in ("o", "o-color"):
            a, b = got["cap/ab*-2048", nl, mode], got["cap/ab*-2049", nl, mode]
            assert a != b and b.count(b"\n") == a.count(b"\n") + 1
        a, b = got["cap/ab*-2048", nl, "lines-color"], got["cap/ab*-2049", nl, "lines-color"]
        assert len(b) == len(a) + 1 and b.count(cm.C_MATCH) == a.count(cm.C_MATCH) and b.count(b"a") == a.count(b"a") + 1
        k = b.index(b"a" + cm.RESET + b"\n")  # the 2049th a: behind the last coloured one, in front of the line's close
        assert b[:k] + b[k + 1:] == a
        a, b = got["cap/ab*-2048", nl, "lines"], got["cap/ab*-2049", nl, "lines"]
        assert len(b) == len(a) + 1


# ------------------------------------------------------------------------------------------------------------ refusals
def test_what_the_drivers_refuse_and_the_call_after_it(gpu):
    row = lc.BY_KEY["a+b"]
    text = lc.case("a+b", False)[0]
    plan, plan_o = plans(gpu, row)
    try:
        # a loops plan scans the whole text in one window: the pieces drivers refuse it
        with pytest.raises(KrepGpuError, match="krep_gpu_split_mode"):
            plan.grep_lines_pieces(text, 4099)
        with pytest.raises(KrepGpuError, match="krep_gpu_split_mode"):
            plan_o.grep_only_matching_pieces(text, 4099)
        # a candidate line of 4097 bytes in an ordinary text: the scan refuses it, the drivers pass the reason on
        rng = np.random.RandomState(11)
        bad = background(rng, 30000, b"aac \n")
        put_line(bad, 9000, b"a" * 4096 + b"b")
        put_line(bad, 200, b"xaab")
        hold, d_bad = to_device(bad, 3)
        for color in (False, True):
            with pytest.raises(KrepGpuError, match="more than 4096 bytes"):
                plan.grep_lines(d_bad, bad.size, filename=NAME, color=color)
            with pytest.raises(KrepGpuError, match="more than 4096 bytes"):
                plan_o.grep_only_matching(d_bad, bad.size, filename=NAME, color=color)
        del hold
        # the next call on the same plans with a good text
        hold, d_text = to_device(text, 3)
        for mode in lc.MODES:
            got = driver(plan, plan_o, mode, d_text, text.size)
            assert got == want("a+b", False, mode), (mode, first_diff(got, want("a+b", False, mode)))
        del hold
    finally:
        plan.close()
        plan_o.close()


def test_a_starved_grid_prints_the_same_bytes(gpu):
    """the walk's grid capped at one workgroup (krep_gpu_debug_force_regex_grid): a lane takes line after line"""
    row = lc.BY_KEY["class-c"]
    text = lc.case(row.key, True)[0]
    hold, d_text = to_device(text)
    plan, plan_o = plans(gpu, row)
    try:
        gpu.force_regex_grid(1)
        for road in (SPARSE, DENSE):
            gpu.force_regex_loops_road(road)
            for mode in lc.MODES:
                got = driver(plan, plan_o, mode, d_text, text.size)
                assert got == want(row.key, True, mode), (road, mode, first_diff(got, want(row.key, True, mode)))
    finally:
        gpu.force_regex_grid(0)
        gpu.force_regex_loops_road(AUTO)
        plan.close()
        plan_o.close()
    del hold
