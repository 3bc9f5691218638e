"""The window contract of the -o output (krep_gpu_format_matches_window) as tests/matches_window_model.py states it, without a
device: for the table rows and the 288 seeded cases of only_matching_model, and for several cuts of each record list, the chained
windows concatenate to only_matching_model.only_matching_output on the whole text (which test_only_matching_model_cpu.py pins to
the stock CLI).  Also here: what the model refuses, and the held-back schedule of Plan.grep_only_matching_pieces
(krep_amd.engine.StaleSchedule) driven over the model: rule undecided -> held -> decided both ways."""
import bisect
import random

import pytest

import matches_window_model as mw
import only_matching_model as om
from krep_amd import abi
from krep_amd.engine import StaleSchedule

_LISTS = []


@pytest.fixture(scope="module")
def lists(oracle_engine):
    """(case, its record list cut and ordered) for every case, computed once"""
    if not _LISTS:
        for case in om.table_cases() + om.random_cases():
            _LISTS.append((case, om.lm.cut_to_max_count(case.emitted(oracle_engine, abi), case.max_count)))
    return _LISTS


def cuts_of(text, recs, rng):
    n = len(recs)
    at_last_newline = sum(1 for s, _ in recs if s < mw.last_newline1(text))
    some = sorted(rng.randrange(0, n + 1) for _ in range(min(n, 4)))
    return {"each": list(range(1, n)), "random": some, "empty": sorted(some + some + [0, n]), "last-newline": [at_last_newline]}


def test_chained_windows_concatenate_to_the_whole_text(lists):
    rng = random.Random(7)
    assert len(lists) >= 288 + 14
    stale = cut_cases = 0
    for case, recs in lists:
        text, n = case.text, len(recs)
        stale += om.stale_records(text, recs) > 0
        for name, cuts in cuts_of(text, recs, rng).items():
            for color, limits in ((False, (None, 0, 1, n // 2 + 1)), (True, (None, n // 2 + 1))):
                fmt = om.strings(om.FILE, color)
                for limit in limits:
                    want = om.only_matching_output(text, recs, fmt, limit)
                    got, items = mw.chain(text, recs, cuts, fmt, limit)
                    assert got == want and items == (n if limit is None else min(n, limit)), (case.key, name, cuts, color, limit)
                    cut_cases += 1
    assert stale >= 30 and cut_cases >= 6000  # the stale rule is on the ground the cuts cover


def test_one_window_by_hand():
    text = b"ab\ncd\n\nef"
    W = mw.Window
    # the whole text as one window is the whole-text call
    recs = [(0, 1), (1, 2), (2, 4), (4, 5), (7, 9)]
    r = mw.window(text, W(0, 9, 9, 0, 7, 0, 0), recs, om.strings(b"F"))
    assert r == (b"F:1:a\nF:1:b\nF:1: c\nF:2:d\nF:4:ef\n", 5, 3, 2)
    # a buffer inside the text: the carry counts the lines in front of it; a start ON a newline belongs to the line it ends
    r = mw.window(text[2:6], W(2, 9, 5, 0, 7, 0, 0), [(2, 4), (4, 5)])
    assert r == (b"1: c\n2:d\n", 2, 1, 2)
    r = mw.window(text[5:9], W(5, 9, 9, 1, 7, 2, 1), [(5, 6), (6, 7), (7, 9), (8, 20)])  # on the last newline: true; behind it: stale
    assert r == (b"2: \n3: \n3:ef\n3:f\n", 4, 3, 3)
    # all stale: the value that came in, 1 when there is none; stale_rule = 0: true numbers
    assert mw.window(text[7:], W(7, 9, 7, 3, 7, 2, 1), [(7, 8), (8, 8)]) == (b"2:e\n2:\n", 2, 3, 2)
    assert mw.window(text[7:], W(7, 9, 7, 3, 7, 0, 1), [(7, 8)]) == (b"1:e\n", 1, 3, 0)
    assert mw.window(text[7:], W(7, 9, 7, 3, 7, 2, 0), [(7, 8)]) == (b"4:e\n", 1, 3, 2)
    # max_items cuts the output, not the list: the stale value still comes from all n records
    r = mw.window(text, W(0, 9, 0, 0, 7, 0, 1), [(0, 1), (4, 5), (7, 8)], max_items=1)
    assert r == (b"1:a\n", 1, 0, 2)
    # no records: the carries move on
    assert mw.window(text[:6], W(0, 9, 6, 5, 7, 4, 1), []) == (b"", 0, 7, 4)
    assert mw.window(b"", W(3, 9, 3, 5, 7, 4, 1), []) == (b"", 0, 5, 4)
    # 16 digits through the carry
    r = mw.window(b"a\na", W(10, 20, 13, 10 ** 15 - 2, 0, 0, 0), [(10, 11), (12, 13)])
    assert r.data == b"999999999999999:a\n1000000000000000:a\n" and r.newlines_before_count_to == 10 ** 15 - 1


def test_what_a_window_refuses():
    text = b"ab\nab\nab\n"
    W = mw.Window
    ok = W(3, 9, 6, 1, 9, 0, 0)
    assert mw.window(text[3:6], ok, [(3, 5)]).data == b"2:ab\n"
    for win, buf, recs in (
            (ok, text[3:6], [(4, 5), (3, 5)]),            # descending
            (ok, text[3:6], [(2, 4)]),                    # a start in front of the buffer
            (ok, text[3:6], [(6, 8)]),                    # a start at its end
            (ok, text[3:6], [(4, 3)]),                    # end < start
            (ok, text[3:6], [(4, 7)]),                    # the match outruns a buffer that does not end the text
            (ok._replace(count_to=2), text[3:6], []),     # count_to outside the buffer
            (ok._replace(count_to=7), text[3:6], []),
            (ok._replace(last_newline1=10), text[3:6], []),
            (ok._replace(global_len=5), text[3:6], []),   # the buffer outruns the text
            (ok._replace(global_len=10 ** 16, last_newline1=0), text[3:6], []),
            (ok._replace(newlines_before=10 ** 16 - 2), text[3:6], [])):  # a LINE of 17 digits
        with pytest.raises(mw.Refused):
            mw.window(buf, win, recs)
    # a match that outruns the TEXT is clamped where the buffer ends the text
    assert mw.window(text[6:], W(6, 9, 9, 2, 9, 0, 0), [(6, 20)]).data == b"3:ab \n"


def drive(text, recs, piece_bytes, max_count, fmt, longest):
    """Plan.grep_only_matching_pieces with the model in the place of the device call: the pieces of the text in order, the
    records that START in a piece, StaleSchedule, the held records each in a window of its own -> (bytes, most records held)"""
    total, last1 = len(text), mw.last_newline1(text)
    sched = StaleSchedule(abi.SIZE_MAX if max_count is None else max_count, last1)
    state = {"nl": 0, "stale": 0, "held": 0}
    out, starts = [], [s for s, _ in recs]

    def call(buf, base, count_to, sub, rule):
        r = mw.window(buf, mw.Window(base, total, count_to, state["nl"], last1, state["stale"], int(rule)), sub, fmt)
        out.append(r.data)
        return r

    def held_calls(records, rule):
        for s, e in records:
            assert s >= last1 and state["nl"] == text.count(b"\n")
            state["stale"] = call(text[s:max(min(e, total), s + 1)], s, s, [(s, e)], rule).stale_line

    for lo in range(0, total, piece_bytes):
        hi = min(lo + piece_bytes, total)
        base, end = max(lo - 1, 0), min(hi + longest, total)
        mine = recs[bisect.bisect_left(starts, lo):bisect.bisect_left(starts, hi)]
        flush, now, rule = sched.add(len(mine), lambda: mine)
        state["held"] = max(state["held"], len(sched.held))
        held_calls(flush, rule)
        r = call(text[base:end], base, hi - 1 if hi < total else total, mine[:now], rule)  # count_to: the next piece's base
        state["nl"], state["stale"] = r.newlines_before_count_to, r.stale_line
    flush, rule = sched.end()
    held_calls(flush, rule)
    return b"".join(out), state["held"]


def test_the_held_back_schedule_of_the_driver(lists):
    fmt = om.strings(om.FILE)
    held_cases = 0
    for idx, (case, recs) in enumerate(lists):
        if len(case.pats) > 1 and case.max_count is not None:
            continue  # (the driver refuses a dictionary with max_count)
        longest = max(max(e - s for s, e in recs), 1) if recs else 1
        want = om.only_matching_output(case.text, recs, fmt)
        for piece in (1, 7, 64, len(case.text) + 5) if len(case.text) <= 400 else (7, 64, 1000):
            got, held = drive(case.text, recs, piece, case.max_count, fmt, longest)
            assert got == want and held <= 10, (case.key, piece)
            held_cases += held > 0
    assert held_cases >= 20
    # the three schedules by hand: a long last line with at most 10 records in all (held, decided at the end: true numbers) ...
    text = b"a\na\n" + b"a" * 8
    recs = [(i, i + 1) for i, c in enumerate(text) if c == 97]
    assert drive(text, recs, 3, None, fmt, 1) == (om.only_matching_output(text, recs, fmt), 8) and len(recs) == 10
    assert om.only_matching_output(text, recs, fmt).endswith(b":3:a\n")
    # ... the 11th record in the last line (held, then decided: stale numbers) ...
    text += b"a"
    recs.append((12, 13))
    assert drive(text, recs, 3, None, fmt, 1) == (om.only_matching_output(text, recs, fmt), 8)
    assert om.only_matching_output(text, recs, fmt).endswith(b":2:a\n")
    assert drive(text, recs[:10], 3, 10, fmt, 1) == (om.only_matching_output(text, recs[:10], fmt), 0)  # -m 10: never applies
    # ... and the count past 10 before the last line: nothing is ever held
    text = b"a\n" * 12 + b"aa"
    recs = [(i, i + 1) for i, c in enumerate(text) if c == 97]
    assert drive(text, recs, 5, None, fmt, 1) == (om.only_matching_output(text, recs, fmt), 0)


def test_the_schedule_step_by_step():
    s = StaleSchedule(abi.SIZE_MAX, 100)
    assert s.add(3, lambda: [(1, 2), (99, 101), (100, 101)]) == ([], 2, False) and s.held == [(100, 101)]
    assert s.add(0, None) == ([], 0, False)
    assert s.add(2, lambda: [(105, 106), (107, 108)]) == ([], 0, False) and len(s.held) == 3  # nothing is emitted behind a held record
    assert s.add(6, None) == ([(100, 101), (105, 106), (107, 108)], 6, True) and s.held == [] and s.count == 11
    assert s.add(4, None) == ([], 4, True) and s.end() == ([], True)
    s = StaleSchedule(abi.SIZE_MAX, 100)  # the text ends first: the rule does not apply
    assert s.add(1, lambda: [(100, 101)]) == ([], 0, False) and s.end() == ([(100, 101)], False)
    assert StaleSchedule(10, 100).add(10, None) == ([], 10, False)   # max_count <= 10, or a text without a newline: decided
    assert StaleSchedule(abi.SIZE_MAX, 0).add(5, None) == ([], 5, False)
    s = StaleSchedule(11, 100)
    assert s.add(11, None) == ([], 11, True)
