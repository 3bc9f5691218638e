"""Regex plans (krep -E) through the five output drivers of krep_amd/engine.py -- Plan.grep_lines plain and coloured,
Plan.grep_only_matching, Plan.grep_lines_pieces, Plan.grep_only_matching_pieces -- byte for byte against the output models on the
records of the regex models.  The rows, their texts and the expected bytes are those of tests/regex_output_cases.py, which
tests/test_regex_output_cases_cpu.py pins to the compiled reference and the stock CLI; nothing here asks the reference.

What the rows bring that a literal plan cannot: records of different lengths in one list, a list from ONE pattern with | inside
(num_patterns == 1: the drivers skip order_by_start), and matches LONGER than the pattern string (`q[a-c]{15}`: 10 and 16 bytes), by
which the pieces drivers must not size a halo: the texts hold the longest match at every offset cut - Lmax - 1 .. cut + 1 of a cut."""
import functools

import numpy as np
import pytest

import regex_output_cases as rc
import regex_ref
from krep_amd import abi
from krep_amd.engine import KrepGpuError, match_format

pytestmark = pytest.mark.gpu

PAD = 0xEE
NAME = b"f.txt"
PIECE_ROWS = [r.key for r in rc.ROWS if r.mode == rc.PIECES]
WHOLE_ROWS = [r.key for r in rc.ROWS if r.mode == rc.WHOLE]


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
    return e


def to_device(a, shift=0):
    import torch
    t = torch.full((a.size + shift + 64,), PAD, dtype=torch.uint8, device="cuda")
    t[shift:shift + a.size] = torch.from_numpy(a.copy())
    return t, t.data_ptr() + shift


@functools.lru_cache(maxsize=None)
def want(key, nl, mode, filename=NAME, max_count=None) -> bytes:
    _, raw, _, rec = rc.case(key, nl)
    return rc.expected(raw, rec, mode, filename, max_count)


def missing(key, nl, expected: bytes, got: bytes):
    """for a failure's message: the records whose -o line `got` lacks (it is `expected` with lines left out) -> [(start, length,
    the planted copy it is: kind, k = bytes of it in front of its cut)]"""
    _, _, plants, rec = rc.case(key, nl)
    by_start = {p.start: p for p in plants}
    have, out, j = got.split(b"\n"), [], 0
    for i, line in enumerate(expected.split(b"\n")[:-1]):
        if j < len(have) and have[j] == line:
            j += 1
        elif i < len(rec):
            p = by_start.get(rec[i][0])
            out.append((rec[i][0], rec[i][1] - rec[i][0]) + ((p.kind, p.k) if p else ()))
    return out[:40]


def driver(plan, plan_o, mode, d_text, n, filename=NAME, max_count=None) -> bytes:
    if mode.startswith("o"):
        return plan_o.grep_only_matching(d_text, n, filename=filename, max_count=max_count, color=mode.endswith("color"))
    return plan.grep_lines(d_text, n, filename=filename, max_count=max_count, color=mode.endswith("color"))


# ------------------------------------------------------------------------------------------------------------ the resident text
@pytest.mark.parametrize("family", rc.FAMILIES)
def test_resident_text_through_every_output_mode(gpu, family):
    """grep_lines with and without a filename, coloured, grep_only_matching plain and coloured, max_count 1, 7 and beyond the count, on
    a text that ends in a newline; the text without one 3 and 13 bytes into its allocation.  The WHOLE rows are here too."""
    for row in (r for r in rc.ROWS if r.family == family):
        plan, plan_o = gpu.plan(rc.params(row)), gpu.plan(rc.params(row), only_matching=True)
        try:
            assert plan.longest_match() == row.Lmax + row.eol and plan_o.longest_match() == row.Lmax + row.eol, row.key
            text, _, _, rec = rc.case(row.key, True)
            hold, d_text = to_device(text)
            for mode in rc.MODES:
                for filename in (NAME, None):
                    got = driver(plan, plan_o, mode, d_text, text.size, filename)
                    assert got == want(row.key, True, mode, filename), (row.key, mode, filename, len(got))
                for mc in (1, 7, len(rec) + 5):
                    got = driver(plan, plan_o, mode, d_text, text.size, NAME, mc)
                    assert got == want(row.key, True, mode, NAME, mc), (row.key, mode, mc, len(got))
            del hold
            text = rc.case(row.key, False)[0]
            for shift in (3, 13):
                hold, d_text = to_device(text, shift)
                assert d_text % 16 == shift
                for mode in rc.MODES:
                    got = driver(plan, plan_o, mode, d_text, text.size)
                    assert got == want(row.key, False, mode), (row.key, shift, mode, len(got))
                del hold
        finally:
            plan.close()
            plan_o.close()


def test_the_plan_max_count_cuts_the_list_like_the_argument(gpu):
    """max_count as the PLAN carries it (krep -m N): the scan stops the list, the drivers get no argument"""
    for key in ("basic/q16", "anchor/digits-eol", "alt/1-and-16", "ext/colour"):
        row = rc.BY_KEY[key]
        text = rc.case(key, True)[0]
        hold, d_text = to_device(text)
        for mc in (1, 7):
            plan, plan_o = gpu.plan(rc.params(row, mc)), gpu.plan(rc.params(row, mc), only_matching=True)
            try:
                for mode in rc.MODES:
                    assert driver(plan, plan_o, mode, d_text, text.size) == want(key, True, mode, NAME, mc), (key, mode, mc)
            finally:
                plan.close()
                plan_o.close()
        del hold


def test_the_retry_road_of_the_only_matching_output(gpu):
    """Rows whose matches are longer than their pattern string: a guess made from the string's length is short of the bytes.  What
    grep_only_matching's second call relies on: a capacity one byte short comes back as overflow with the exact size and the record
    count, and the call with that size gives the right bytes -- records of 1 and 16 bytes in one list included."""
    import torch
    rows = [r for r in rc.ROWS if r.Lmax > rc.string_len(r)]
    assert len(rows) >= 4
    for row in rows:
        text, _, _, rec = rc.case(row.key, True)
        expected = want(row.key, True, "o-color")
        hold, d_text = to_device(text)
        plan = gpu.plan(rc.params(row), only_matching=True)
        try:
            pos = torch.empty(2 * (len(rec) + 1), dtype=torch.int64, device="cuda")
            out = plan.scan(d_text, text.size, d_positions=pos.data_ptr(), capacity=len(rec) + 1)
            assert out.stored == len(rec) and not out.overflow
            fmt = match_format(NAME, True)
            short = torch.full((len(expected) + 64,), PAD, dtype=torch.uint8, device="cuda")
            res = gpu.format_matches(d_text, text.size, pos.data_ptr(), len(rec), abi.SIZE_MAX, fmt, short.data_ptr(), len(expected) - 1)
            assert res.overflow and res.out_bytes == len(expected), (row.key, res.out_bytes, len(expected))
            assert bytes(short[len(expected) - 1:].cpu().numpy()) == bytes([PAD]) * 65  # nothing behind the capacity it was given
            res = gpu.format_matches(d_text, text.size, pos.data_ptr(), len(rec), abi.SIZE_MAX, fmt, short.data_ptr(), int(res.out_bytes))
            assert not res.overflow and bytes(short[: int(res.out_bytes)].cpu().numpy()) == expected, row.key
            assert plan.grep_only_matching(d_text, text.size, filename=NAME, color=True) == expected
        finally:
            plan.close()
        del hold


# ------------------------------------------------------------------------------------------------------------ the text in pieces
@pytest.mark.parametrize("key", PIECE_ROWS)
def test_pieces_equal_the_model_and_the_resident_driver(gpu, key):
    """grep_lines_pieces (halo_bytes 0, which means a halo of the longest match, and the default) and grep_only_matching_pieces, with and
    without colour, at pieces of 4099 bytes, of a 32-KiB unit and of more than the text.  The $ rows are here: the drivers stage so that
    the scan's refusal of an own_hi closer than L bytes to the end of a buffer that does not end the text never fires."""
    row = rc.BY_KEY[key]
    plan, plan_o = gpu.plan(rc.params(row)), gpu.plan(rc.params(row), only_matching=True)
    try:
        text = rc.case(key, False)[0]
        hold, d_text = to_device(text)
        resident = {mode: driver(plan, plan_o, mode, d_text, text.size) for mode in rc.MODES}
        del hold
        for mode in rc.MODES:
            assert resident[mode] == want(key, False, mode), (key, mode)
        for piece in (rc.P_SMALL, rc.P_UNIT, rc.TOTAL + 1000):
            for color in (False, True):
                mode = "o-color" if color else "o"
                got = plan_o.grep_only_matching_pieces(text, piece, filename=NAME, color=color)
                assert got == resident[mode], (key, piece, mode, len(got), len(resident[mode]), missing(key, False, resident[mode], got))
                mode = "lines-color" if color else "lines"
                for halo in (0, rc.HALO):
                    got = plan.grep_lines_pieces(text, piece, filename=NAME, color=color, halo_bytes=halo)
                    assert got == resident[mode], (key, piece, mode, halo, len(got), len(resident[mode]))
        # the text that ends in a newline, and no filename
        text = rc.case(key, True)[0]
        assert plan_o.grep_only_matching_pieces(text, rc.P_SMALL) == want(key, True, "o", None), key
        assert plan.grep_lines_pieces(text, rc.P_SMALL, halo_bytes=0) == want(key, True, "lines", None), key
        assert plan.grep_lines_pieces(text, rc.P_SMALL, color=True) == want(key, True, "lines-color", None), key
    finally:
        plan.close()
        plan_o.close()
    if not rc.single(row):
        return  # (a finite max_count is refused for several patterns: test_what_the_pieces_drivers_refuse)
    for mc in (1, 7):
        plan, plan_o = gpu.plan(rc.params(row, mc)), gpu.plan(rc.params(row, mc), only_matching=True)
        try:
            for color in (False, True):
                got = plan_o.grep_only_matching_pieces(text, rc.P_SMALL, filename=NAME, color=color)
                assert got == want(key, True, "o-color" if color else "o", NAME, mc), (key, mc, color)
                got = plan.grep_lines_pieces(text, rc.P_SMALL, filename=NAME, color=color, halo_bytes=0 if color else rc.HALO)
                assert got == want(key, True, "lines-color" if color else "lines", NAME, mc), (key, mc, color)
        finally:
            plan.close()
            plan_o.close()


def test_what_the_pieces_drivers_refuse(gpu):
    for key in WHOLE_ROWS:  # the match set is a greedy selection over the whole occurrence list
        row = rc.BY_KEY[key]
        text = rc.case(key, False)[0]
        plan, plan_o = gpu.plan(rc.params(row)), gpu.plan(rc.params(row), only_matching=True)
        try:
            with pytest.raises(KrepGpuError, match="krep_gpu_split_mode"):
                plan.grep_lines_pieces(text, rc.P_SMALL)
            with pytest.raises(KrepGpuError, match="krep_gpu_split_mode"):
                plan_o.grep_only_matching_pieces(text, rc.P_SMALL)
        finally:
            plan.close()
            plan_o.close()
    row = rc.BY_KEY["alt/two-e"]  # several -e with a finite max_count: as for literals
    text = rc.case(row.key, False)[0]
    plan, plan_o = gpu.plan(rc.params(row, 7)), gpu.plan(rc.params(row, 7), only_matching=True)
    try:
        with pytest.raises(KrepGpuError, match="multi-pattern plan with max_count"):
            plan.grep_lines_pieces(text, rc.P_SMALL)
        with pytest.raises(KrepGpuError, match="multi-pattern plan with max_count"):
            plan_o.grep_only_matching_pieces(text, rc.P_SMALL)
    finally:
        plan.close()
        plan_o.close()
