"""krep_gpu_format_lines_window / Plan.grep_lines_pieces: the matching lines of a text in PIECES on the device.  The bytes of every
window against tests/lines_window_model.py, and the windows of a cut, concatenated, against krep_gpu_format_lines_ex on the whole text
on the same device (and so against tests/color_line_model.py).  Texts of a few KiB; pad bytes 0xEE around text and output."""
import subprocess

import numpy as np
import pytest

import color_line_model as cm
import line_model as lm
import lines_window_model as wm
import oracle_lib as ol
from krep_amd import abi

pytestmark = pytest.mark.gpu

PAD = 0xEE
ODD = (b"#", bytes(range(65, 82)), b"", bytes(range(97, 130)))  # 1, 17, 0 and 33 bytes
COLOUR = cm.strings(lm.FILE, True)
PLAIN = cm.strings(lm.FILE, False)
NONE = abi.SIZE_MAX


@pytest.fixture(scope="module")
def gpu():
    import krep_amd
    e = krep_amd.load()
    assert e.device_count() >= 1
    return e


def to_device(data, shift=0):
    """(tensor that owns the bytes, device pointer of data[0]): PAD in front of and behind the bytes"""
    import torch
    a = np.frombuffer(bytes(data), dtype=np.uint8)
    t = torch.full((a.size + shift + 64,), PAD, dtype=torch.uint8, device="cuda")
    if a.size:
        t[shift:shift + a.size] = torch.from_numpy(a.copy())
    return t, t.data_ptr() + shift


def records_to_device(recs):
    import torch
    a = np.asarray(recs, dtype=np.uint64).reshape(-1, 2)
    t = torch.zeros(2 * len(a) + 2, dtype=torch.int64, device="cuda")
    if len(a):
        t[: 2 * len(a)] = torch.from_numpy(a.astype(np.int64).reshape(-1))
    return t, len(a)


def occurrences(text: bytes, pat: bytes):
    out, i = [], text.find(pat)
    while i >= 0:
        out.append((i, i + len(pat)))
        i = text.find(pat, i + len(pat))
    return out


def answer(r):
    return (int(r.lines.out_bytes), int(r.lines.lines), int(r.lines.lines_total), int(r.lines.capped_lines),
            int(r.incomplete_line_start1), int(r.incomplete_first_record))


def check_window(gpu, text, recs, base, end, own_lo, own_hi, records_hi, fmt=COLOUR, max_lines=None, shift=0, out_shift=0):
    """one call on the buffer text[base:end] against the model: size query, exact capacity, capacity one short -> the model"""
    import torch
    model = wm.Window(text, recs, base, end - base, own_lo, own_hi, records_hi, fmt, max_lines)
    keep, d_text = to_device(text[base:end], shift)
    pos, m = records_to_device(recs)
    win = abi.LinesWindow(base, len(text), own_lo, own_hi, records_hi)
    f = abi.LineFormat(*fmt) if fmt is not None else None
    limit = NONE if max_lines is None else max_lines
    want = (len(model.data), model.lines, model.lines_total, model.capped, model.incomplete_line_start1, model.incomplete_first_record)
    q = gpu.format_lines_window(d_text, end - base, win, pos.data_ptr(), m, limit, f)
    assert answer(q) == want and not q.lines.overflow, (answer(q), want)
    size = len(model.data)
    buf = torch.full((size + 64,), PAD, dtype=torch.uint8, device="cuda")
    r = gpu.format_lines_window(d_text, end - base, win, pos.data_ptr(), m, limit, f, buf.data_ptr() + out_shift, size)
    got = buf.cpu().numpy()
    assert answer(r) == want and not r.lines.overflow
    assert got[out_shift:out_shift + size].tobytes() == model.data
    assert (got[:out_shift] == PAD).all() and (got[out_shift + size:] == PAD).all()  # nothing outside [0, out_bytes)
    if size > 1:
        r = gpu.format_lines_window(d_text, end - base, win, pos.data_ptr(), m, limit, f, buf.data_ptr(), size - 1)
        assert r.lines.overflow == 1 and answer(r) == want
    return model


def whole_text(gpu, text, recs, fmt, max_lines=None):
    """krep_gpu_format_lines_ex on the resident text -> (bytes, LinesOut)"""
    import torch
    keep, d_text = to_device(text)
    pos, m = records_to_device(recs)
    limit = NONE if max_lines is None else max_lines
    f = abi.LineFormat(*fmt)
    size = int(gpu.format_lines_ex(d_text, len(text), pos.data_ptr(), m, limit, f).out_bytes)
    buf = torch.full((size + 64,), PAD, dtype=torch.uint8, device="cuda")
    r = gpu.format_lines_ex(d_text, len(text), pos.data_ptr(), m, limit, f, buf.data_ptr(), size)
    return buf[:size].cpu().numpy().tobytes(), r


def check_pieces(gpu, text, recs, cuts, fmt=COLOUR, max_lines=None, slack=0):
    """the invariant: windows over `cuts` with truthful halos, max_lines passed on as what is left, against the whole-text call"""
    n, left = len(text), max_lines
    out, lines, total, capped = [], 0, 0, 0
    for k, (lo, hi) in enumerate(zip(cuts, cuts[1:])):
        base, reach = max(lo - 1, 0), min(wm.truthful_reach(text, recs, lo, hi) + slack, n)
        mine = wm.records_in(recs, base, reach)
        model = check_window(gpu, text, mine, base, reach, lo, hi, reach, fmt, left, shift=(0, 3, 7)[k % 3], out_shift=(0, 5)[k % 2])
        assert not model.incomplete_line_start1
        out.append(model.data)  # (check_window has compared the device's bytes with it)
        lines, total, capped = lines + model.lines, total + model.lines_total, capped + model.capped
        if left is not None:
            left -= model.lines
    data, r = whole_text(gpu, text, recs, fmt, max_lines)
    assert b"".join(out) == data == cm.ColorLines(text, recs, fmt, max_lines).data
    assert (lines, total, capped) == (int(r.lines), int(r.lines_total), int(r.capped_lines))
    return out


def line_text(seed, n, longest=200):
    rng = np.random.RandomState(seed)
    out = bytearray()
    while len(out) < n:
        body = bytearray(rng.choice(np.frombuffer(b"cdefg ", dtype=np.uint8), int(rng.randint(0, longest))).tobytes())
        for _ in range(int(rng.randint(0, 3))):
            if len(body) >= 2:
                s = int(rng.randint(0, len(body) - 1))
                body[s:s + 2] = b"ab"
        out += body + b"\n"
    return bytes(out[:n])


def test_a_cuts_at_a_newline_and_at_a_block_edge(gpu):
    text = line_text(1, 3 * 4096 + 100)
    nl = text.find(b"\n", 6000)
    assert nl % 4096 not in (0, 1, 4095)
    recs = occurrences(text, b"ab")
    assert len(recs) > 50
    for cut in (nl - 1, nl, nl + 1, 4095, 4096, 4097):
        check_pieces(gpu, text, recs, [0, cut, len(text)])
    check_pieces(gpu, text, recs, [0, 4095, 4096, 4097, nl, nl + 1, len(text)], ODD, slack=5)
    a = np.frombuffer(text, dtype=np.uint8).copy()  # ... and the newlines ON the block edge
    a[[4095, 4096, 4097]] = 10
    a[4090:4092] = a[4098:4100] = (ord("a"), ord("b"))
    text = a.tobytes()
    recs = occurrences(text, b"ab")
    for cut in (4095, 4096, 4097, 4098):
        check_pieces(gpu, text, recs, [0, cut, len(text)], PLAIN)


def test_b_a_line_over_three_blocks_crosses_the_cuts(gpu):
    long = bytearray(b"d" * 9000)
    for s in (0, 17, 1999, 2000, 4000, 5190, 5191, 5193, 8000, 8998):
        long[s:s + 2] = b"ab"
    text = line_text(2, 3000) + b"\n" + bytes(long) + b"\n" + line_text(3, 2500)
    start = 3001
    recs = occurrences(text, b"ab")
    assert lm.line_of(text, start + 4000) == (start, start + 9000)
    for cuts in ([0, 5000, 8192, len(text)], [0, start, start + 1, len(text)], [0, 8191, 8193, 12001, len(text)]):
        for fmt in (COLOUR, ODD):
            check_pieces(gpu, text, recs, cuts, fmt)


def test_c_left_edge_records_on_newlines(gpu):
    text = b"aa\n\nbb\ncc\n\n\ndd"
    recs = [(0, 2), (2, 3), (3, 4), (4, 6), (6, 9), (7, 9), (9, 9), (10, 11), (11, 12), (12, 14)]
    for c in range(1, len(text)):  # own_lo - 1 and own_lo land on every newline and on every record
        check_pieces(gpu, text, recs, [0, c, len(text)], ODD)
    check_pieces(gpu, text, recs, list(range(len(text) + 1)), COLOUR)
    # the record ON the newline at own_lo - 1 is the neighbour's; the one ON the newline at own_lo opens the empty line there
    m = check_window(gpu, text, recs[1:], 2, len(text), 3, 4, len(text), ODD)
    assert m.spans == [(3, 3)] and m.lines == 1
    m = check_window(gpu, text, recs, 0, len(text), 0, 3, len(text), ODD)   # own_lo == 0
    assert m.spans == [(0, 2)]


def test_d_a_window_that_owns_no_matching_line(gpu):
    text = line_text(4, 3000) + b"\n" + b"d" * 5000 + b"ab\n" + line_text(5, 1000)
    recs = occurrences(text, b"ab")
    lo = 3001 + 100
    mine = wm.records_in(recs, lo - 1, 8000)
    assert mine == []                               # no record at all: n == 0
    keep, d_text = to_device(text[lo - 1:8000])
    assert answer(gpu.format_lines_window(d_text, 8000 - lo + 1, abi.LinesWindow(lo - 1, len(text), lo, 7000, 8000), 0, 0)) == (0,) * 6
    mine = wm.records_in(recs, lo - 1, 8200)        # the records of the long line: it starts in front of the window
    assert len(mine) == 1
    m = check_window(gpu, text, mine, lo - 1, 8200, lo, 8000, 8200)
    assert (m.data, m.lines, m.lines_total, m.incomplete_line_start1, m.incomplete_first_record) == (b"", 0, 0, 0, 1)
    mine = wm.records_in(recs, 0, 3000)             # ... and lines that start behind own_hi
    assert len(mine) > 5
    m = check_window(gpu, text, mine, 0, 3000, 0, 0, 3000)
    assert (m.data, m.lines_total) == (b"", 0)


def test_e_texts_without_a_last_newline(gpu):
    none = bytearray(b"e" * 6000)
    for s in (0, 100, 4095, 5998):
        none[s:s + 2] = b"ab"
    tail = line_text(6, 2000) + b"\n" + bytes(none[:4500])
    for text in (bytes(none), tail):
        recs = occurrences(text, b"ab")
        n = len(text)
        start = lm.line_of(text, n - 1)[0]
        check_pieces(gpu, text, recs, [0, n])
        check_pieces(gpu, text, recs, [0, start + 50, n], ODD)
        # the buffer ends the text: the last line is complete; it does not (by one byte): the line is reported
        m = check_window(gpu, text, wm.records_in(recs, max(start - 1, 0), n), max(start - 1, 0), n, start, start + 1, n, ODD)
        assert m.lines == 1 and m.data.endswith(bytes(range(97, 130)) + b"\n")
        mine = wm.records_in(recs, max(start - 1, 0), n - 1)
        m = check_window(gpu, text, mine, max(start - 1, 0), n - 1, start, start + 1, n - 1, ODD)
        assert (m.lines, m.incomplete_line_start1, m.incomplete_first_record) == (0, start + 1, 0 if start == 0 else mine.index(
            min(r for r in mine if r[0] >= start)))
        # ... nor when the buffer ends the text but the list does not reach its end
        m = check_window(gpu, text, mine, max(start - 1, 0), n, start, start + 1, n - 1, ODD)
        assert m.incomplete_line_start1 == start + 1


def test_f_records_hi_around_the_last_owned_newline(gpu):
    text = line_text(7, 5000)
    recs = occurrences(text, b"ab")
    first = next(r for r in recs if r[0] > 4200)
    a, z = lm.line_of(text, first[0])
    lo = 4100
    assert lo < a and z + 20 < len(text)
    for hi, complete in ((z - 1, False), (z, False), (z + 1, True), (z + 9, True)):
        if hi <= first[0]:
            continue
        for listed in (hi, z + 20):  # the list ends at records_hi / holds records behind it
            mine = wm.records_in(recs, lo - 1, listed)
            m = check_window(gpu, text, mine, lo - 1, z + 20, lo, a + 1, hi, COLOUR, shift=1)
            assert (m.incomplete_line_start1 == 0) == complete and (m.spans[-1] == (a, z)) == complete
            if not complete:
                assert m.incomplete_line_start1 == a + 1 and mine[m.incomplete_first_record] == first


def test_g_a_line_of_2100_records_crosses_a_cut(gpu):
    text = line_text(8, 3000) + b"\n" + b"a" * 2100 + b"\n" + line_text(9, 500)
    start = 3001
    recs = sorted(occurrences(text[:start], b"ab") + [(start + i, start + i + 1) for i in range(2100)] +
                  [(s + start + 2101, e + start + 2101) for s, e in occurrences(text[start + 2101:], b"ab")])
    for cuts in ([0, 4096, len(text)], [0, start + 2047, start + 2048, start + 2049, len(text)]):
        for fmt in (COLOUR, ODD):
            out = check_pieces(gpu, text, recs, cuts, fmt)
            line = fmt[0] + (fmt[1] + b"a" + fmt[2]) * lm.CAP + b"a" * (2100 - lm.CAP) + fmt[3] + b"\n"
            assert out[0].endswith(line)  # (and check_pieces: capped_lines sums to the whole text's 1)
    assert cm.ColorLines(text, recs).capped == 1


def test_h_max_lines_runs_out_inside_the_second_of_three_windows(gpu):
    text = line_text(10, 9000, longest=60)
    recs = occurrences(text, b"ab")
    cuts = [0, 3000, 6000, len(text)]
    per = [cm.ColorLines(text, recs).lines_total]
    first = wm.Window(text, wm.records_in(recs, 0, 3100), 0, 3100, 0, 3000, 3100).lines_total
    second = wm.Window(text, wm.records_in(recs, 2999, 6100), 2999, 3101, 3000, 6000, 6100).lines_total
    assert first > 3 and second > 6 and per[0] > first + second + 3
    for fmt in (COLOUR, ODD):
        out = check_pieces(gpu, text, recs, cuts, fmt, max_lines=first + 3)
        assert out[1] and out[2] == b""  # the third window was passed 0
    # a short halo in the second window: its last owned line is incomplete, and reported only in front of the limit
    last = [r for r in recs if lm.line_of(text, r[0])[0] < 6000][-1]
    a, z = lm.line_of(text, last[0])
    end = z  # the buffer stops ON the line's newline
    mine = wm.records_in(recs, 2999, end)
    m = check_window(gpu, text, mine, 2999, end, 3000, 6000, end, COLOUR)
    assert (m.incomplete_line_start1, m.lines) == (a + 1, second - 1)
    m = check_window(gpu, text, mine, 2999, end, 3000, 6000, end, COLOUR, max_lines=second - 1)
    assert (m.incomplete_line_start1, m.incomplete_first_record, m.lines) == (0, len(mine), second - 1)
    m = check_window(gpu, text, mine, 2999, end, 3000, 6000, end, COLOUR, max_lines=0)
    assert (m.data, m.incomplete_line_start1, m.lines_total) == (b"", 0, second - 1)


def test_refusals_leave_the_output_untouched(gpu):
    import torch
    import krep_amd
    text = line_text(11, 600, longest=30)
    recs = occurrences(text, b"ab")
    base, end = 100, 500
    good = wm.records_in(recs, base, end)
    assert len(good) > 3
    keep, d_text = to_device(text[base:end])
    buf = torch.full((4096,), PAD, dtype=torch.uint8, device="cuda")
    ok = abi.LinesWindow(base, len(text), 101, 400, 500)

    def refused(win, lst, match):
        pos, m = records_to_device(lst)
        with pytest.raises(krep_amd.KrepGpuError, match=match):
            gpu.format_lines_window(d_text, end - base, win, pos.data_ptr(), m, NONE, abi.LineFormat(*ODD), buf.data_ptr(), 4096)
        assert gpu.last_error() and bool((buf == PAD).all())

    refused(ok, [good[1], good[0]] + good[2:], "not ascending in start, or a record lies outside")
    refused(ok, good + [(end, end + 2)], "not ascending in start, or a record lies outside")
    refused(ok, [(base - 1, base + 1)] + good, "not ascending in start, or a record lies outside")
    refused(ok, [(good[0][0], good[0][0] - 1)], "not ascending in start, or a record lies outside")
    refused(abi.LinesWindow(base, len(text), base, 400, 500), good, "own_lo == global_base")
    refused(abi.LinesWindow(base, len(text), 101, 450, 449), good, "own_lo <= own_hi <= records_hi")
    refused(abi.LinesWindow(base, len(text), 101, 400, 501), good, "own_lo <= own_hi <= records_hi")
    refused(abi.LinesWindow(base, end - base - 1 + base, 101, 400, 499), good, "does not lie inside a text")
    refused(abi.LinesWindow(300, len(text), 301, 400, 500), [], "does not lie inside a text")  # (checked before n == 0)
    with pytest.raises(krep_amd.KrepGpuError, match="format string"):
        pos, m = records_to_device(good)
        gpu.format_lines_window(d_text, end - base, ok, pos.data_ptr(), m, NONE, abi.LineFormat(b"x" * ((1 << 20) + 1)))
    # the library works on after a refusal
    check_window(gpu, text, good, base, end, 101, 400, 500, ODD)


def test_odd_addresses_of_text_and_output(gpu):
    text = line_text(12, 2 * 4096 + 77)
    recs = occurrences(text, b"ab")
    n = len(text)
    for base, shift, out_shift in ((1001, 0, 1), (1001, 2, 3), (4097, 1, 15), (777, 13, 7)):
        lo = base + 1
        hi = min(lo + 5000, n)
        reach = wm.truthful_reach(text, recs, lo, hi)
        for fmt in (PLAIN, ODD):
            check_window(gpu, text, wm.records_in(recs, base, reach), base, reach, lo, hi, reach, fmt, shift=shift, out_shift=out_shift)


# ---- the driver: Plan.grep_lines_pieces --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def word_text(gpu):
    import wordlist
    W = wordlist.word_list()
    text = gpu.generate_host(48 * 1024 + 13, 0, 5, 20260930, wordlist.pack(W), 80).tobytes()
    assert text.count(b"\n") > 100
    seen = {}
    for w in text.split():
        seen[w] = seen.get(w, 0) + 1
    # words of 4..8 letters without a border (no prefix that is also a suffix), 15..300 occurrences each, in a fixed order
    words = sorted(w for w, c in seen.items() if 4 <= len(w) <= 8 and 15 <= c <= 300 and w.isalpha()
                   and not any(w[:k] == w[-k:] for k in range(1, len(w))))
    assert len(words) >= 5
    return text, words[:5]


def resident(gpu, plan, text, **kw):
    keep, d_text = to_device(text)
    return plan.grep_lines(d_text, len(text), **kw)


@pytest.mark.parametrize("kind", ["literal", "dictionary"])
def test_driver_on_word_text(gpu, word_text, kind, tmp_path):
    text, words = word_text
    pats = words[:1] if kind == "literal" else words
    path = tmp_path / "words.txt"
    cli = ol.ref_cli()
    if cli:
        path.write_bytes(text)
    plan = gpu.plan(abi.Params(pats))
    for color in (False, True):
        want = resident(gpu, plan, text, filename=str(path), color=color)
        assert want.count(b"\n") > 10
        for piece in (4096, 5000):
            assert plan.grep_lines_pieces(text, piece, filename=str(path), color=color) == want, (kind, color, piece)
        assert plan.grep_lines_pieces(np.frombuffer(text, dtype=np.uint8), 5000, color=color) == resident(gpu, plan, text, color=color)
        if cli:
            args = [pats[0].decode()] if len(pats) == 1 else [x for p in pats for x in ("-e", p.decode())]
            r = subprocess.run([cli, "-t", "1", "--color=always" if color else "--color=never"] + args + [str(path)],
                               capture_output=True, timeout=120)
            assert r.returncode == 0 and r.stdout == want
    plan.close()


def test_driver_literal_with_max_count(gpu, word_text):
    text, words = word_text
    for mc in (1, 7, 40):
        plan = gpu.plan(abi.Params(words[:1], max_count=mc))
        want = resident(gpu, plan, text, filename="f")
        assert want.count(b"\n") >= 1
        for piece in (4096, 5000):
            assert plan.grep_lines_pieces(text, piece, filename="f") == want, (mc, piece)
        plan.close()


def test_driver_lines_longer_than_the_halo(gpu):
    long1 = bytearray(b"d" * 20000)   # records at both ends: reported incomplete by its piece, staged again
    long1[5:7] = long1[19990:19992] = b"ab"
    long2 = bytearray(b"e" * 15000)   # its only record lies far behind the halo: no call can report it
    long2[14000:14002] = b"ab"
    text = line_text(13, 3000) + b"\n" + bytes(long1) + b"\n" + line_text(14, 2000) + b"\n" + bytes(long2) + b"\n" + line_text(15, 3000)
    plan = gpu.plan(abi.Params([b"ab"]))
    for color in (False, True):
        want = resident(gpu, plan, text, filename="f", color=color)
        assert want == cm.ColorLines(text, occurrences(text, b"ab"), cm.strings(b"f", color)).data
        for piece, halo in ((4096, 4096), (5000, 100), (3000, 1)):
            assert plan.grep_lines_pieces(text, piece, filename="f", color=color, halo_bytes=halo) == want, (color, piece, halo)
    plan.close()
    tail = text + b"ab" + b"f" * 9000 + b"ab"  # ... and a last line without a newline
    plan = gpu.plan(abi.Params([b"ab"]))
    assert plan.grep_lines_pieces(tail, 4096, halo_bytes=64) == resident(gpu, plan, tail)
    plan.close()


def test_driver_refuses_a_dictionary_with_max_count(gpu, word_text):
    import krep_amd
    text, words = word_text
    plan = gpu.plan(abi.Params(words, max_count=5))
    with pytest.raises(krep_amd.KrepGpuError, match="max_count"):
        plan.grep_lines_pieces(text, 4096)
    plan.close()
