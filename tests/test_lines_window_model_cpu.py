"""tests/lines_window_model.py against tests/color_line_model.py on the whole text: the window contract of
krep_gpu_format_lines_window, without a device.  The windows of any cut of a text, with truthful halos, concatenate to the
whole-text output; with the halo cut short the model reports the right line, and submitting that line again repairs the output."""
import random

import pytest

import color_line_model as cm
import line_model as lm
import lines_window_model as wm

ODD = (b"#", bytes(range(65, 82)), b"", bytes(range(97, 130)))
FORMATS = {"plain": cm.strings(lm.FILE, False), "colour": cm.strings(lm.FILE, True), "odd": ODD}


def random_text(rng, n):
    alpha = rng.choice([b"ab\n", b"abc  \n", b"ab", b"ab\n\n", b"abcdefgh" * 4 + b"\n"])
    text = bytearray(rng.choice(alpha) for _ in range(n))
    if rng.random() < 0.4:
        text[-1] = 10
    elif text[-1] == 10 and rng.random() < 0.5:
        text[-1] = 97
    return bytes(text)


def random_records(rng, text):
    """ascending in (start, end): overlapping, nested, empty, over a newline, ON a newline, in runs on one line"""
    n, recs = len(text), []
    for _ in range(rng.choice([0, 1, 3, 10, 40, 120])):
        s = rng.randrange(0, n)
        recs.append((s, min(n + 3, s + rng.choice([0, 1, 1, 2, 3, 7, 30]))))
    for i, c in enumerate(text):
        if c == 10 and rng.random() < 0.1:
            recs.append((i, i + rng.choice([0, 1, 2])))
    return sorted(set(recs))


def random_cuts(rng, n):
    k = rng.randrange(1, 7)
    inner = sorted(set(rng.randrange(1, n) for _ in range(k - 1))) if n > 1 else []
    return [0] + inner + [n]


def cases(count=300, seed=20261017):
    rng = random.Random(seed)
    for k in range(count):
        text = random_text(rng, rng.choice([1, 2, 7, 40, 200, 900]))
        recs = random_records(rng, text)
        yield k, rng, text, recs


@pytest.mark.parametrize("name", sorted(FORMATS))
def test_windows_with_truthful_halos_concatenate_to_the_whole_text(name):
    fmt, seen = FORMATS[name], 0
    for k, rng, text, recs in cases():
        for mc in (None, rng.choice([0, 1, 2, 5])):
            whole = cm.ColorLines(text, recs, fmt, mc)
            cuts = random_cuts(rng, len(text))
            data, lines, total, capped, windows, again = wm.run_pieces(text, recs, cuts, fmt, mc, slack=rng.choice([0, 0, 1, 9]))
            assert data == whole.data, (k, cuts, mc)
            assert (lines, total, capped, again) == (len(whole.spans), whole.lines_total, whole.capped, 0), (k, cuts, mc)
            seen += windows
    assert seen > 1000


def test_cuts_at_every_offset_of_a_small_text():
    text = b"ab\n\nabab\nb\n\nab"
    recs = [(0, 2), (1, 5), (2, 3), (3, 3), (4, 6), (6, 8), (8, 9), (9, 10), (11, 11), (12, 14), (13, 20)]
    whole = cm.ColorLines(text, recs, ODD)
    for c1 in range(1, len(text)):
        for c2 in range(c1 + 1, len(text)):
            assert wm.run_pieces(text, recs, [0, c1, c2, len(text)], ODD)[0] == whole.data, (c1, c2)
            for h in (0, 1, 3):
                data, lines, total, _, _, _ = wm.run_pieces(text, recs, [0, c1, c2, len(text)], ODD, halo=h)
                assert data == whole.data and lines == total == whole.lines_total, (c1, c2, h)


def test_a_short_halo_reports_the_right_line_and_resubmission_repairs_the_output():
    resubmitted = 0
    for k, rng, text, recs in cases(200, 7):
        fmt = FORMATS[rng.choice(sorted(FORMATS))]
        for mc in (None, rng.choice([1, 2, 5])):
            whole = cm.ColorLines(text, recs, fmt, mc)
            cuts = random_cuts(rng, len(text))
            # (run_pieces checks that the reported line is the line of the record incomplete_first_record names)
            data, lines, _, capped, _, again = wm.run_pieces(text, recs, cuts, fmt, mc, halo=rng.choice([0, 1, 2, 8]))
            assert data == whole.data and lines == len(whole.spans) and capped == whole.capped, (k, cuts, mc)
            resubmitted += again
    assert resubmitted > 50


def test_the_report_names_the_line_and_its_first_record():
    text = b"aa\nbbbbbbbbbb\ncc\n"
    recs = [(0, 1), (2, 3), (4, 5), (6, 7), (14, 15)]
    # the window owns [0, 5): lines 0 and 3; the buffer ends at 8, inside the second line
    w = wm.Window(text, wm.records_in(recs, 0, 8), 0, 8, 0, 5, 8)
    assert (w.data, w.lines, w.lines_total) == (b"aa\n", 1, 1)  # (the record ON the newline at 2 is line 0's)
    assert (w.incomplete_line_start1, w.incomplete_first_record) == (4, 2)
    # behind max_lines the line would not have been emitted: no report
    w = wm.Window(text, wm.records_in(recs, 0, 8), 0, 8, 0, 5, 8, max_lines=1)
    assert (w.lines, w.incomplete_line_start1, w.incomplete_first_record) == (1, 0, 4)
    # records_hi ON the newline (13): incomplete; one behind it: complete
    assert wm.Window(text, wm.records_in(recs, 2, 13), 2, 12, 3, 4, 13).incomplete_line_start1 == 4
    w = wm.Window(text, wm.records_in(recs, 2, 14), 2, 12, 3, 4, 14)
    assert (w.data, w.incomplete_line_start1) == (b"bbbbbbbbbb\n", 0)
    # a last line without a newline is complete only where the buffer ends the text and the list with it
    t2 = b"aa\nbbb"
    assert wm.Window(t2, [(4, 5)], 2, 4, 3, 4, 6).data == b"bbb\n"
    assert wm.Window(t2, [(4, 5)], 2, 3, 3, 4, 5).incomplete_line_start1 == 4
    assert wm.Window(t2 + b"b", [(4, 5)], 2, 4, 3, 4, 6).incomplete_line_start1 == 4


def test_refusals():
    text = b"ab\nab\nab\n"
    for args in ((1, 5, 1, 3, 6), (0, 5, 0, 4, 3), (2, 8, 3, 5, 7)):  # own_lo == global_base > 0; own_hi > records_hi; past the text
        with pytest.raises(wm.Refused):
            wm.Window(text, [], *args)
    for recs in ([(4, 5), (3, 5)], [(7, 8)], [(1, 2)], [(4, 3)]):       # unsorted; behind / in front of the buffer; end < start
        with pytest.raises(wm.Refused):
            wm.Window(text, recs, 2, 4, 3, 5, 6)
