"""Generated -E expressions (tests/regex_generated_cases.py) through the device line walks of kg_regex_loops.hip, short lines and long:
every case the host compilers take, on a text of 10 to 11 KB with a line of 4097 and one of about 5000 bytes, against the compiled
reference's regex_search (oracle/_ref, through tests/regex_ref.py) — records, -c, the count alone and a max_count that falls inside
a long line's matches, on both roads.  The groups cases reach 12 jump pairs and 32 positions: every group of four of rl_follow and
of rl_pred runs.  Every loops case also runs by the general step.  Chunks of the cases with 9..12 pairs run with the long lines'
scratch in two rounds, on a text placed 1 and 3 bytes into its allocation between bytes that would lengthen a match, and on a grid
of one workgroup.  tests/test_regex_generated_cases_cpu.py says why the list is good enough.  The module turns the three switches on
and, whatever happens, off again, and resets the budget, road, grid and general hooks."""
import numpy as np
import pytest

import regex_generated_cases as gc
import regex_ref
from krep_amd import abi
from test_gpu_regex_loops import AUTO, DENSE, SPARSE, rx, scan_records, to_device

pytestmark = pytest.mark.gpu

GUARD = 64  # records of slack behind the ones a scan may write


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
    e.set_regex_long_lines(True)
    try:
        yield e
    finally:
        e.set_regex_long_lines(False)
        e.set_regex_groups(False)
        e.set_regex_loops(False)
        e.set_regex_loops_windows(False)
        e.set_regex_long_budget(0)
        e.force_regex_general(False)
        e.force_regex_loops_road(AUTO)
        e.force_regex_grid(0)


def inside_a_long_line(c) -> int:
    """a max_count that cuts the records of a long line in two (of the first long line that holds two); else half of all records"""
    records = gc.ref_answer(c)[1]
    starts = records[:, 0].astype(np.int64)
    for a, b in c.long_spans:
        idx = np.flatnonzero((starts >= a) & (starts < b))
        if idx.size >= 2:
            return int(idx[idx.size // 2])
    return max(1, records.shape[0] // 2)


def modes(c):
    return (dict(), dict(count_lines=True), dict(track_positions=False), dict(max_count=inside_a_long_line(c)))


def check(gpu, c, note="", **kw):
    """test_gpu_regex_loops.check for a case, with a message that names the case and the first differing record"""
    want = gc.ref_answer(c, **kw)
    got = gpu.search(rx(c.pats, case_sensitive=c.cs, **kw), c.text)
    what = " ".join(x for x in (c.label(), str(kw) if kw else "", note.strip()) if x)
    assert gpu.last_status() == abi.STATUS_OK, "%s: %s" % (what, gpu.last_error())
    assert got[0] == want[0], "%s: count %d, want %d; %s" % (what, got[0], want[0], gc.first_difference(got[1], want[1]))
    assert np.array_equal(got[1], want[1]), "%s: %s" % (what, gc.first_difference(got[1], want[1]))
    return want


def both_roads(gpu, c, note=""):
    """every mode on the forced sparse and the forced dense road; the long walk ran, and for a groups case the general step"""
    long_before, general_before = gpu.regex_long_walks(), gpu.regex_general_walks()
    try:
        for road in (SPARSE, DENSE):
            gpu.force_regex_loops_road(road)
            for kw in modes(c):
                check(gpu, c, "%s road %d" % (note, road), **kw)
    finally:
        gpu.force_regex_loops_road(AUTO)
    assert gpu.regex_long_walks() > long_before, c.label()
    assert (gpu.regex_general_walks() > general_before) == (c.kind == "groups"), c.label()


def records_of(c, pos, n):
    return pos[:2 * n].astype(np.uint64).reshape(-1, 2)


def wide_chunk(k):
    """every third of the taken groups cases with 9..12 jump pairs in the order of their positions, from the k-th on (k < 3): some 24"""
    some = sorted((c for c in gc.taken("groups") if 9 <= c.pairs <= 12), key=lambda c: c.n_pos)[k::3]
    assert 15 <= len(some) <= 30 and any(c.pairs == 12 for c in some) and any(c.n_pos >= 29 for c in some)
    return some


def both_long_lines_hold_a_record(c) -> bool:
    starts = gc.ref_answer(c)[1][:, 0].astype(np.int64)
    return all(((starts >= a) & (starts < b)).any() for a, b in c.long_spans)


# ------------------------------------------------------------------------------------------------------------ 1. every case
@pytest.mark.parametrize("k", range(gc.n_chunks("groups")))
def test_every_groups_case_on_both_roads(gpu, k):
    for c in gc.chunk("groups", k):
        both_roads(gpu, c)


@pytest.mark.parametrize("k", range(gc.n_chunks("loops")))
def test_every_loops_case_on_both_roads_and_by_the_general_step(gpu, k):
    for c in gc.chunk("loops", k):
        both_roads(gpu, c)
        # one plan built as always and one under the hook, on the same device text: the same counts and record arrays, the reference's
        hold, d_text = to_device(c.text, 5)
        for kw in (dict(), dict(count_lines=True)):
            want = gc.ref_answer(c, **kw)
            old_plan = gpu.plan(rx(c.pats, case_sensitive=c.cs, **kw))
            gpu.force_regex_general(True)
            try:
                new_plan = gpu.plan(rx(c.pats, case_sensitive=c.cs, **kw))
            finally:
                gpu.force_regex_general(False)
            try:
                before = gpu.regex_general_walks()
                old = scan_records(old_plan, d_text, c.text.size)
                assert gpu.regex_general_walks() == before, c.label()
                new = scan_records(new_plan, d_text, c.text.size)
                assert gpu.regex_general_walks() > before, c.label()
                assert old[0].count == new[0].count == want[0], "%s %s: the shift %d, the general step %d, the reference %d" % (
                    c.label(), kw, old[0].count, new[0].count, want[0])
                assert np.array_equal(old[1], new[1]), "%s %s: the shift against the general step: %s" % (
                    c.label(), kw, gc.first_difference(old[1].reshape(-1, 2), new[1].reshape(-1, 2)))
                if not kw:
                    assert np.array_equal(records_of(c, new[1], want[0]), want[1]), "%s: the general step: %s" % (
                        c.label(), gc.first_difference(records_of(c, new[1], want[0]), want[1]))
            finally:
                old_plan.close()
                new_plan.close()
        del hold


# ------------------------------------------------------------------------------------------------------------ 2. rounds
def test_the_long_lines_of_a_chunk_of_9_to_12_pairs_in_two_rounds(gpu):
    """a budget of 6000 scratch words: the two long lines (4097 and about 5000 words) make two rounds, so the emitting launch repeats
    the backward pass (kept == 0), and the cap of one line is 6000 bytes.  (A long line without a match may be no candidate line
    on the sparse road, and is not listed then: the launches are counted where both long lines hold a record.)"""
    counted = 0
    try:
        gpu.set_regex_long_budget(4 * 6000)
        for c in wide_chunk(0):
            both = both_long_lines_hold_a_record(c)
            counted += both
            before = gpu.regex_long_walks()
            check(gpu, c, "in two rounds")
            moved = gpu.regex_long_walks() - before
            assert moved >= 4 or not both, (c.label(), moved)  # two counting and two emitting rounds
            before = gpu.regex_long_walks()
            check(gpu, c, "in two rounds", count_lines=True)
            moved = gpu.regex_long_walks() - before
            assert moved == 1 if both else moved <= 1, (c.label(), moved)  # -c keeps no scratch: one launch
            check(gpu, c, "in two rounds", max_count=inside_a_long_line(c))
    finally:
        gpu.set_regex_long_budget(0)
    assert counted >= 15, counted


# ------------------------------------------------------------------------------------------------------------ 3. placement
def lengthening_byte(c) -> int:
    """a letter of the case that can stand behind a match's last byte and go on with it (else one that can begin a match)"""
    au = c.automaton()
    for positions in ([q for p in sorted(au.last) for q in sorted(au.follow[p])], sorted(au.first)):
        for q in positions:
            for b in c.letters.tolist():
                if au.tables[q][b] and b != 32:
                    return b
    return int(c.letters[0])


def test_a_chunk_of_9_to_12_pairs_placed_1_and_3_bytes_into_its_allocation(gpu):
    """between bytes that would lengthen a match, the record buffer sized to the count and a guard: the reference's records, and
    nothing behind them"""
    for c in wide_chunk(1):
        want = gc.ref_answer(c)
        n = want[0]
        plan = gpu.plan(rx(c.pats, case_sensitive=c.cs))
        try:
            for shift in (1, 3):
                hold, d_text = to_device(c.text, shift, pad=lengthening_byte(c))
                for road in (SPARSE, DENSE):
                    gpu.force_regex_loops_road(road)
                    out, pos = scan_records(plan, d_text, c.text.size, cap=n + GUARD)
                    note = "%s shift %d road %d" % (c.label(), shift, road)
                    assert (out.count, out.stored, out.overflow) == (n, n, 0), (note, out.count, out.stored, n)
                    assert np.array_equal(records_of(c, pos, n), want[1]), "%s: %s" % (note, gc.first_difference(records_of(c, pos, n), want[1]))
                    assert (pos[2 * n:] == -1).all(), "%s: written behind the records: %s" % (note, pos[2 * n:2 * n + 8].tolist())
                del hold
        finally:
            gpu.force_regex_loops_road(AUTO)
            plan.close()


# ------------------------------------------------------------------------------------------------------------ 4. the seam of two sequences
def test_long_lines_that_are_one_sequence_behind_another_under_both_anchors(gpu):
    """^a+b$|^c+d$ and ^e+f$: a long line a..abc..cd holds no match.  The reverse step of the shift must not hand over from the first
    place of a sequence to the last place of the one in front of it: -c, which the backward pass alone answers, would count the line"""
    c = gc.seam_case()
    both_roads(gpu, c)
    assert gc.ref_answer(c, count_lines=True)[0] == 6
    for budget, grid in ((4 * 6000, 0), (0, 1)):
        try:
            gpu.set_regex_long_budget(budget)
            gpu.force_regex_grid(grid)
            for kw in modes(c):
                check(gpu, c, "budget %d grid %d" % (budget, grid), **kw)
        finally:
            gpu.set_regex_long_budget(0)
            gpu.force_regex_grid(0)
    hold, d_text = to_device(c.text, 3)  # ... and by the general step, whose reverse is the other half of rl_pred
    for kw in (dict(), dict(count_lines=True)):
        want = gc.ref_answer(c, **kw)
        gpu.force_regex_general(True)
        try:
            plan = gpu.plan(rx(c.pats, case_sensitive=c.cs, **kw))
        finally:
            gpu.force_regex_general(False)
        try:
            before = gpu.regex_general_walks()
            out, pos = scan_records(plan, d_text, c.text.size)
            assert gpu.regex_general_walks() > before
            assert out.count == want[0], "%s %s by the general step: count %d, want %d" % (c.label(), kw, out.count, want[0])
            if not kw:
                assert np.array_equal(records_of(c, pos, want[0]), want[1]), "%s by the general step: %s" % (
                    c.label(), gc.first_difference(records_of(c, pos, want[0]), want[1]))
        finally:
            plan.close()
    del hold


# ------------------------------------------------------------------------------------------------------------ 5. a starved grid
def test_a_chunk_on_a_grid_of_one_workgroup(gpu):
    try:
        gpu.force_regex_grid(1)
        for c in wide_chunk(2)[:15] + gc.chunk("loops", 3)[:10]:
            both_roads(gpu, c, "one workgroup")
    finally:
        gpu.force_regex_grid(0)
