"""The record post-processors with offsets that need 33 to 41 bits: krep_gpu_order_by_start (its radix key is sized from
max_offset), krep_gpu_line_numbers_ex (global - global_base) and the two window formatters with every global quantity shifted by
K = 5 * 2^32.  Expected values: numpy's sorts and newline counts, and the window models of the unshifted row (they read only
text[global_base:end], so they are translation-invariant by their own definition)."""
import numpy as np
import pytest

import high_offset_cases as hc
import lines_window_model as wm
import line_model as lm
import matches_window_model as mw
import only_matching_model as om
import test_gpu_lines_window as lw
import test_gpu_matches_window as tm
from krep_amd import abi
from test_gpu_format import EDGE_TEXT

pytestmark = pytest.mark.gpu

K = 5 << 32


@pytest.fixture(scope="module")
def gpu():
    import krep_amd
    e = krep_amd.load()
    assert e.device_count() >= 1
    return e


def ordered(gpu, recs, max_offset):
    """krep_gpu_order_by_start on a list written by the test; a guard record behind the list must survive"""
    import torch
    a = np.asarray(recs, dtype=np.uint64).reshape(-1, 2)
    guard = np.array([[0x7A5A5A5A5A5A5A5A, 0x7BADBADBADBADBAD]], dtype=np.uint64)
    d = torch.from_numpy(np.concatenate([a, guard]).astype(np.int64)).cuda().contiguous()
    gpu.order_by_start(d.data_ptr(), len(a), max_offset)
    got = d.cpu().numpy().astype(np.uint64)
    assert np.array_equal(got[len(a):], guard)
    return got[: len(a)]


def by_start_stable(a):
    return a[np.argsort(a[:, 0], kind="stable")]


@pytest.mark.parametrize("base", hc.BASES)
def test_order_by_start_of_a_dictionary_list_at_a_high_base(gpu, oracle_engine, base):
    case = next(c for c in hc.all_cases() if c.key == "multi/seven/plain")
    emitted = hc.reference(oracle_engine, gpu, case, base)[1] + np.uint64(base)
    assert len(emitted) > 5000 and not np.array_equal(emitted, by_start_stable(emitted))  # (end-ordered: the sort has work to do)
    got = ordered(gpu, emitted, base + hc.N)
    assert np.array_equal(got, emitted[np.lexsort((emitted[:, 1], emitted[:, 0]))])  # qsort by (start, end)


@pytest.mark.parametrize("n", [0, 1, 2, 255, 256, 257, 70_001])
def test_order_by_start_sizes(gpu, n):
    rng = np.random.RandomState(n)
    for lo, span in ((0, 1000), (hc.B1, 300_000), (hc.B2, 300_000), ((1 << 40) - 5000, 5000)):
        start = (lo + rng.randint(0, span + 1, size=n)).astype(np.uint64)  # many equal starts: the order among them must hold
        a = np.stack([start, start + rng.randint(0, 40, size=n).astype(np.uint64)], axis=1).reshape(-1, 2)
        assert np.array_equal(ordered(gpu, a, lo + span), by_start_stable(a)), (n, lo)


def test_order_by_start_is_stable(gpu):
    for start in (7, (1 << 32) - 1, 1 << 32, hc.B2 + 5):
        a = np.stack([np.full(5000, start, dtype=np.uint64), start + np.arange(5000, dtype=np.uint64)], axis=1)
        assert np.array_equal(ordered(gpu, a, start), a), start
        mixed = np.concatenate([a[:2500], [[start - 1, start + 9]], a[2500:], [[start - 2, start]]]).astype(np.uint64)
        assert np.array_equal(ordered(gpu, mixed, start), by_start_stable(mixed)), start


@pytest.mark.parametrize("k", [8, 32, 33, 40])
def test_order_by_start_key_width_around_a_power_of_two(gpu, k):
    """max_offset = 2^k - 1, 2^k, 2^k + 1 with a record that starts AT max_offset: one key bit too few and it sorts to the front"""
    rng = np.random.RandomState(k)
    for max_offset in ((1 << k) - 1, 1 << k, (1 << k) + 1):
        near = max_offset - rng.randint(0, 200, size=600)
        wide = (rng.random_sample(600) * max_offset).astype(np.uint64)
        start = np.concatenate([near.astype(np.uint64), wide, [max_offset, 0, max_offset, 1 << (k - 1), (1 << (k - 1)) - 1]]).astype(np.uint64)
        start = start[rng.permutation(start.size)]
        a = np.stack([start, start + np.arange(start.size, dtype=np.uint64) % np.uint64(7)], axis=1)
        got = ordered(gpu, a, max_offset)
        assert np.array_equal(got, by_start_stable(a)), (k, max_offset)
        assert int(got[-1, 0]) == max_offset and int(got[0, 0]) == 0


@pytest.mark.parametrize("which", ["random", "edge"])
@pytest.mark.parametrize("base", hc.BASES)
def test_line_numbers_at_a_high_base(gpu, base, which):
    """krep_gpu_line_numbers_ex through Engine.line_numbers(global_base=): 1 + the newlines of the buffer in front of the start, for
    starts on, one in front of and one behind every multiple of 4096 (the newline table's block), at 0 and at text_len; a record
    that starts outside [global_base, global_base + text_len] comes back as line 0.  Buffers at d_text + 0, 3, 7."""
    import torch
    if which == "random":
        text = next(c for c in hc.all_cases() if c.key == "multi/seven/plain").text
    else:
        text = np.frombuffer(EDGE_TEXT, dtype=np.uint8)
    n = text.size
    rng = np.random.RandomState(31 + n)
    local = np.concatenate([np.arange(0, n + 1, 4096), np.arange(4096, n + 1, 4096) - 1, np.arange(0, n, 4096) + 1, [0, 1, n - 1, n],
                            np.flatnonzero(text == 10)[:50], np.flatnonzero(text == 10)[:50] + 1, rng.randint(0, n + 1, size=3000)])
    local = local[(local >= 0) & (local <= n)][rng.permutation(local.size)].astype(np.int64)
    nl = np.flatnonzero(text == 10)
    want = 1 + np.searchsorted(nl, local, side="left")  # the newlines strictly in front of the start
    # (+- 2^32: outside, but a difference taken in 32 bits would land inside the buffer)
    outside = [base + n + 1, base + n + 4096, 1 << 62, base + (1 << 32), base + (1 << 32) + 5, base + (3 << 32) + n]
    outside += [base - 1, base - 4096, 0] if base else []
    outside += [base - (1 << 32) + 5] if base >= 1 << 32 else []
    start = np.concatenate([local.astype(object) + base, outside]).astype(np.uint64)
    want = np.concatenate([want, np.zeros(len(outside), dtype=np.int64)])
    order = rng.permutation(start.size)
    start, want = start[order], want[order]
    recs = np.stack([start, start + np.uint64(1)], axis=1)
    d_pos = torch.from_numpy(recs.astype(np.int64)).cuda().contiguous()
    for shift in (0, 3, 7):
        keep, d_text = lw.to_device(text.tobytes(), shift)
        lines = torch.full((len(recs) + 1,), -7, dtype=torch.int64, device="cuda")
        gpu.line_numbers(d_text, n, d_pos.data_ptr(), len(recs), lines.data_ptr(), global_base=base)
        got = lines.cpu().numpy()
        assert got[-1] == -7
        assert np.array_equal(got[:-1], want), (base, which, shift, np.flatnonzero(got[:-1] != want)[:5])
    if base == 0:  # krep_gpu_line_numbers itself (Engine.line_numbers goes through _ex): the same answer without a base
        import ctypes as C
        lines.fill_(-7)
        assert gpu.lib.krep_gpu_line_numbers(C.c_void_p(d_text), n, C.c_void_p(d_pos.data_ptr()), len(recs), C.c_void_p(lines.data_ptr()), None) == 0
        assert np.array_equal(lines.cpu().numpy()[:-1], want) and lines.cpu().numpy()[-1] == -7


# ---- the window formatters: every global quantity of a row + K ---------------------------------------------------------------
def lines_row_shifted(gpu, text, recs, base, end, own_lo, own_hi, records_hi, fmt=lw.COLOUR, max_lines=None, shift=0):
    """a row of tests/test_gpu_lines_window.py with global_base, global_len, own_lo, own_hi, records_hi and the records + K: the
    model's bytes of the unshifted row, incomplete_line_start1 + K"""
    import torch
    assert base > 0  # (a buffer that starts the text is one only at global_base == 0)
    model = wm.Window(text, recs, base, end - base, own_lo, own_hi, records_hi, fmt, max_lines)
    keep, d_text = lw.to_device(text[base:end], shift)
    pos, m = lw.records_to_device([(s + K, e + K) for s, e in recs])
    win = abi.LinesWindow(base + K, len(text) + K, own_lo + K, own_hi + K, records_hi + K)
    limit = lw.NONE if max_lines is None else max_lines
    open1 = model.incomplete_line_start1 + K if model.incomplete_line_start1 else 0
    want = (len(model.data), model.lines, model.lines_total, model.capped, open1, model.incomplete_first_record)
    q = gpu.format_lines_window(d_text, end - base, win, pos.data_ptr(), m, limit, abi.LineFormat(*fmt))
    assert lw.answer(q) == want and not q.lines.overflow, (lw.answer(q), want)
    size = len(model.data)
    buf = torch.full((size + 64,), lw.PAD, dtype=torch.uint8, device="cuda")
    r = gpu.format_lines_window(d_text, end - base, win, pos.data_ptr(), m, limit, abi.LineFormat(*fmt), buf.data_ptr(), size)
    got = buf.cpu().numpy()
    assert lw.answer(r) == want and not r.lines.overflow
    assert got[:size].tobytes() == model.data and (got[size:] == lw.PAD).all()
    return model


def test_lines_window_rows_shifted_past_2_to_the_32(gpu):
    # (test_f) records_hi around the last owned newline: an incomplete line and a complete one
    text = lw.line_text(7, 5000)
    recs = lw.occurrences(text, b"ab")
    first = next(r for r in recs if r[0] > 4200)
    a, z = lm.line_of(text, first[0])
    lo = 4100
    seen = set()
    for hi in (z - 1, z, z + 1, z + 9):
        if hi > first[0]:
            m = lines_row_shifted(gpu, text, wm.records_in(recs, lo - 1, z + 20), lo - 1, z + 20, lo, a + 1, hi, shift=1)
            seen.add(bool(m.incomplete_line_start1))
    assert seen == {True, False}
    # (test_e) a buffer that ends the text, its last line without a newline; and one byte short of it: the line is reported
    none = bytearray(b"e" * 6000)
    for s in (0, 100, 4095, 5998):
        none[s:s + 2] = b"ab"
    text = lw.line_text(6, 2000) + b"\n" + bytes(none[:4500])
    recs, n = lw.occurrences(text, b"ab"), 2001 + 4500
    start = lm.line_of(text, n - 1)[0]
    m = lines_row_shifted(gpu, text, wm.records_in(recs, start - 1, n), start - 1, n, start, start + 1, n, lw.ODD)
    assert m.lines == 1 and not m.incomplete_line_start1
    m = lines_row_shifted(gpu, text, wm.records_in(recs, start - 1, n - 1), start - 1, n - 1, start, start + 1, n - 1, lw.ODD)
    assert m.incomplete_line_start1 == start + 1
    # (test_odd_addresses) windows over two 4-KiB blocks of the text, odd buffer addresses, and max_lines
    text = lw.line_text(12, 2 * 4096 + 77)
    recs = lw.occurrences(text, b"ab")
    for base, shift in ((1001, 0), (4097, 3), (777, 7)):
        lo = base + 1
        hi = min(lo + 5000, len(text))
        reach = wm.truthful_reach(text, recs, lo, hi)
        for fmt, limit in ((lw.PLAIN, None), (lw.ODD, 3)):
            m = lines_row_shifted(gpu, text, wm.records_in(recs, base, reach), base, reach, lo, hi, reach, fmt, limit, shift)
            assert m.lines > 2


def matches_row_shifted(gpu, buf, win, recs, strings=None, max_items=None, shift=0, out_shift=0):
    """a row of tests/test_gpu_matches_window.py with global_base, global_len, count_to, last_newline1 (when there is one) and the
    records + K: the model's answer for the unshifted row, newlines_before_count_to and stale_line unchanged"""
    want = mw.window(buf, win, recs, strings or (b"", b"", b"", b""), max_items)
    moved = win._replace(global_base=win.global_base + K, global_len=win.global_len + K, count_to=win.count_to + K,
                         last_newline1=win.last_newline1 + K if win.last_newline1 else 0)
    got = tm.device_window(gpu, buf, moved, [(s + K, e + K) for s, e in recs], strings, max_items, shift, out_shift)
    assert got == want, (win, recs[:6], got.data[:200], want.data[:200], got[1:], want[1:])
    return got


def test_matches_window_rows_shifted_past_2_to_the_32(gpu):
    W, BASE = mw.Window, tm.BASE
    text = tm.edge_text(0)
    glen, last1 = len(text), mw.last_newline1(text)
    before = text.count(b"\n", 0, BASE)
    # a buffer inside the text: records around its 4-KiB edges, count_to on and around them
    blen = 8192 + 777
    buf = text[BASE:BASE + blen]
    offs = [0, 0, 5, 4095, 4096, 4097, 8191, 8192, blen - 3, blen - 1]
    recs = [(BASE + o, min(BASE + o + 3, BASE + blen)) for o in offs]
    recs[1] = (BASE, BASE)
    for k, (shift, out_shift) in enumerate(((0, 0), (3, 5), (7, 0))):
        win = W(BASE, glen, BASE + (blen, 4096, 4095)[k], before, last1, 0, 0)
        got = matches_row_shifted(gpu, buf, win, recs, (om.strings(b"f"), om.strings(None), om.strings(b"f", True))[k], None, shift, out_shift)
        assert got.items == len(recs) and got.newlines_before_count_to == text.count(b"\n", 0, win.count_to)
    # a buffer that ends the text: a record that ends at global_len, one that outruns it (clamped), an empty one on the last byte
    base = glen - 4096 - 55
    buf = text[base:]
    recs = [(base, base + 2), (base + 4095, base + 4099), (base + 4096, base + 4096), (glen - 5, glen), (glen - 2, glen + 9), (glen - 1, glen - 1)]
    got = matches_row_shifted(gpu, buf, W(base, glen, glen, text.count(b"\n", 0, base), last1, 0, 0), recs, om.strings(b"f", True), None, 3, 5)
    assert got.newlines_before_count_to == text.count(b"\n")
    # the stale rule by offset: last_newline1 inside the window
    text = b"ab\ncd\nef\ngh ij kl mn\nop qr st uv"
    glen, last1 = len(text), mw.last_newline1(text)
    buf, recs = text[7:30], [(7, 8), (9, 11), (20, 22), (21, 23), (27, 29)]
    assert matches_row_shifted(gpu, buf, W(7, glen, 30, 2, last1, 1, 1), recs, om.strings(None), None, 3, 0) == (b"3:f\n4:gh\n4: o\n4:op\n4:st\n", 5, 4, 4)
    assert matches_row_shifted(gpu, buf, W(7, glen, 30, 2, last1, 1, 0), recs, om.strings(None), None, 0, 5) == (b"3:f\n4:gh\n4: o\n5:op\n5:st\n", 5, 4, 4)
    # 15 and 16 digits of LINE through the carry
    buf = b"a\na\na\nb"
    recs = [(1000, 1001), (1002, 1003), (1004, 1005), (1006, 1007)]
    got = matches_row_shifted(gpu, buf, W(1000, 5000, 1002, 10 ** 15 - 2, 0, 0, 0), recs, om.strings(b"f"))
    assert got.data.startswith(b"f:999999999999999:a\nf:1000000000000000:a\n") and got.newlines_before_count_to == 10 ** 15 - 1
