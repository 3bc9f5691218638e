"""The conditions of tests/ac_road_cases.py, checked without a GPU against the compiled reference alone: every plant of a case is a
record of aho_corasick_search at the stated offsets, the -c plants are alone on their lines, the staging texts hold exactly the
per-unit counts the slot edges need, no unit of the other texts can overflow a slot of 16, and the table covers all 16
(ci, lines, shorts, stride) instantiations and the -w ones.  These are conditions: a text that misses one is changed, not the
condition."""
import numpy as np
import pytest

import ac_road_cases as rc
import oracle_lib
from krep_amd import abi

CASES = rc.all_cases()
U = rc.U


@pytest.fixture(scope="module")
def oracle():
    return oracle_lib.checker()


_memo = {}


def records(oracle, case, step, **over):
    """the reference's full record list of the case's search on the text of `step` (no -c, no max_count unless given)"""
    kw = dict(count_lines=False, only_match=False, max_count=abi.SIZE_MAX)
    kw.update(over)
    key = (id(case.steps[step][0]), tuple(case.pats), case.kw.get("case_sensitive", True), case.kw.get("whole_word", False), tuple(sorted(kw.items())))
    if key not in _memo:
        _memo[key] = rc.reference(oracle, case, case.steps[step][0], **kw)
    return _memo[key]


def test_the_table_covers_every_instantiation():
    keys = [c.key for c in CASES]
    assert len(set(keys)) == len(keys)
    first = [c.steps[0][2] for c in CASES]
    tuples = {(r["ci"], r["lines"], r["shorts"], r["stride"]) for r in first}
    assert tuples == {(ci, ln, sh, st) for ci in (0, 1) for ln in (0, 1) for sh in (0, 1) for st in (1, 2)} and len(tuples) == 16
    assert sum(1 for r in first if r["ww_filter"]) >= 2
    assert all(r["road"] == 5 and r["anch"] == 0 for c in CASES for _, _, r in c.steps)
    # has1 (with and without a copy of the short pattern), has2 + has3, has3 alone, none
    assert {c.d.short_lens for c in CASES} == {0, 1, 4, 6}
    assert any(c.pats.count(b"q") == 2 for c in CASES)
    # the forced stride, the emit pass both ways at two ticket sizes, two tickets of eight, the learned slot
    assert sum(1 for c in CASES if c.env.get("KREP_GPU_AC_STRIDE1")) == 8
    for name in ("four_few", "four130"):
        mine = {c.key: c for c in CASES if c.key.startswith(name + "/")}
        assert [mine[f"{name}/slot16-upt{k}"].steps[0][2]["upt"] for k in (1, 3, 8)] == [1, 3, 8]
        assert mine[f"{name}/slot16-upt8"].steps[0][2]["n_units"] == 11  # > 8: two tickets
        assert [mine[f"{name}/slot16-walk-upt{k}"].steps[0][2]["emit"] for k in (1, 3)] == [2, 2]
        assert [(r["stage_cap"], r["next_stage_cap"], r["emit"]) for _, _, r in mine[f"{name}/learned"].steps] == [(16, 64, 1), (64, 64, 0), (64, 64, 0), (64, 64, 1)]
    for c in CASES:
        for t, _, r in c.steps:
            assert t.size in (rc.N5, rc.N10) and t.size % 16 and r["n_units"] == (t.size + U - 1) // U
        assert not (c.counting and any(b"\n" in p for p in c.pats)), c


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_plants_are_in_the_reference_list(oracle, case):
    ci, ww = not case.kw.get("case_sensitive", True), bool(case.kw.get("whole_word"))
    for step, (text, plants, _) in enumerate(case.steps):
        ret, pos = records(oracle, case, step)
        assert ret == len(pos) > 0
        have = {}
        for s, e in pos.tolist():
            have[(s, e)] = have.get((s, e), 0) + 1
        for pl in plants:
            found = have.get((pl.start, pl.end), 0)
            if (pl.ci_only and not ci) or (ww and not pl.word):
                assert found == 0, (case, pl)
                continue
            assert found == case.pats.count(pl.pat), (case, pl, found)
            assert text[pl.start:pl.end].tobytes() == pl.body
        # the reference's order: end ascending, the longest first
        e, s = pos[:, 1].astype(np.int64), pos[:, 0].astype(np.int64)
        assert np.all((np.diff(e) > 0) | ((np.diff(e) == 0) & (np.diff(s) >= 0)))
        if "max_count" in case.kw:
            assert len(pos) > case.kw["max_count"], (case, len(pos))  # the cut is a real one


@pytest.mark.parametrize("case", [c for c in CASES if not c.unit_counts and not c.sweep], ids=repr)
def test_dictionary_texts_hold_their_edges(oracle, case):
    text, plants, rep = case.steps[0]
    n = text.size
    ret, pos = records(oracle, case, 0)
    s, e = pos[:, 0].astype(np.int64), pos[:, 1].astype(np.int64)
    ww = bool(case.kw.get("whole_word"))
    by_name = {pl.name: pl for pl in plants}
    L = len(case.d.main)
    # byte 0, the last byte, a cell cut, a round cut; ends on even and on odd positions
    assert by_name["byte0"].start == 0 and by_name["last"].end == n
    c, r = by_name["cell"], by_name["round"]
    assert c.start < U + 3 * rc.CELL < c.end and r.start < 2 * U + rc.ROUND < r.end and (2 * U + rc.ROUND) % U
    assert {by_name["even"].end & 1, by_name["odd"].end & 1} == {0, 1}
    for j in range(len(case.d.also)):
        assert {by_name[f"even{j}"].end & 1, by_name[f"odd{j}"].end & 1} == {0, 1}
    # the unit cuts: every split the dictionary names, one per cut; every split of the short patterns and of the four-byte main one
    cuts = [pl for pl in plants if pl.name.startswith("unit")]
    assert len(cuts) == len(case.d.splits) and len({(pl.start + U - 1) // U for pl in cuts}) == len(cuts)
    for pl, (q, k) in zip(cuts, case.d.splits):
        cut = (pl.start + U - 1) // U * U
        assert pl.pat == q and pl.start == cut - k and pl.start < cut < pl.end and pl.alone
    for q in {q for q, _ in case.d.splits if len(q) <= 4} | ({case.d.main} if L > 4 else set()):
        assert {k for p, k in case.d.splits if p == q} == set(range(1, len(q))), (case, q)
    # ... the split that leaves only the last byte behind the cut: the extra candidate of the stride-2 -c kernel
    assert any(pl.end % U == 1 for pl in cuts)
    # two patterns that end on one byte, the longest first; a pattern held twice
    a, b = by_name["nested"], by_name["nested-suffix"]
    assert a.end == b.end and a.start < b.start
    if not ww:
        i = np.flatnonzero((s == a.start) & (e == a.end))[0]
        assert (s[i + 1], e[i + 1]) == (b.start, b.end)
    # lines: every plant marked alone is the only record of its line; the two on one line lie on either side of a unit cut; the first
    # and the last line hold a match
    raw = text.tobytes()
    line_of = np.concatenate(([0], np.cumsum(text == 10)))  # line_of[i]: newlines in front of byte i
    rec_line = line_of[s]
    assert np.array_equal(rec_line, line_of[np.maximum(e - 1, s)])  # no pattern holds a newline: a record lies on one line
    for pl in plants:
        if pl.alone and not (pl.ci_only or (ww and not pl.word)):
            assert np.count_nonzero(rec_line == line_of[pl.start]) == case.pats.count(pl.pat), (case, pl)
    lf, rt = by_name["line-left"], by_name["line-right"]
    cut = rt.start // U * U
    assert cut - 16 < lf.end <= cut <= rt.start < cut + 16
    assert b"\n" not in raw[lf.start:rt.end] and np.count_nonzero(rec_line == line_of[lf.start]) == 2
    assert rec_line[0] == 0 and rec_line[-1] == line_of[n - 1] and line_of[n - 1] > 10
    if case.counting:
        assert rc.reference(oracle, case, text)[0] == len(set(rec_line.tolist()))
    # no unit can overflow a slot of 16, whichever unit the kernel gives an end within two bytes of a cut to
    last = e - 1
    for u in range(rep["n_units"]):
        near = np.count_nonzero((last >= u * U - 2) & (last < (u + 1) * U + 2))
        assert near <= 16, (case, u, near)


@pytest.mark.parametrize("case", [c for c in CASES if c.unit_counts], ids=repr)
def test_staging_texts_hold_their_unit_counts(oracle, case):
    for step, (text, plants, rep) in enumerate(case.steps):
        ret, pos = rc.reference(oracle, case, text)
        assert ret == len(pos) == len(plants)
        last = pos[:, 1].astype(np.int64) - 1
        want = dict(case.unit_counts[step])
        want[0], want[rep["n_units"] - 1] = 1, 1
        slot = rep["stage_cap"]
        for u in range(rep["n_units"]):
            k = np.count_nonzero(last // U == u)
            assert k == want.get(u, 0), (case, step, u, k)
            # (the counted ends lie well inside their unit)
            assert not np.any((last // U == u) & ((last % U < 1000) | (last % U > U - 1000))) or u in (0, rep["n_units"] - 1)
        over = [u for u, k in want.items() if k > slot]
        full = [u for u, k in want.items() if k == slot]
        assert len(over) == rep["overflow_units"] and (slot == 16 and rep["scans"] == 1) <= (len(over) == 1 and len(full) == 1), (case, step)
        if slot == 64 and rep["overflow_units"]:
            assert sorted(want.values())[-2:] == [64, 65]
        if rep["overflow_units"]:
            assert rep["overflow_units"] * 64 > rep["n_units"]  # more than 1 in 64 units: the next scan's slot is 64
        assert np.any(pos[:, 1] % 2 == 0) and np.any(pos[:, 1] % 2 == 1)


@pytest.mark.parametrize("case", [c for c in CASES if c.sweep], ids=repr)
def test_sweep_texts_end_a_match_on_every_offset_of_a_cell(oracle, case):
    text, plants, rep = case.steps[0]
    ret, pos = records(oracle, case, 0)
    assert len(pos) == sum(case.pats.count(pl.pat) for pl in plants)
    last = pos[:, 1].astype(np.int64) - 1
    assert set((last % rc.CELL).tolist()) == set(range(rc.CELL))
    # the units the emit pass takes: far over a slot of 16 (or of 64: every other unit holds at most one match), whichever unit an
    # end beside a cut is given to
    per = np.bincount(last // U, minlength=rep["n_units"])
    over = [u for u in range(rep["n_units"]) if per[u] > 16]
    assert over == rc.units_over(plants) and all(per[u] > 20 for u in over) and all(per[u] <= 2 for u in range(rep["n_units"]) if u not in over)
    assert case.counting or (rep["overflow_units"], rep["emit"], rep["next_stage_cap"]) == (len(over), 1, 64)
    if case.counting:
        lines = np.concatenate(([0], np.cumsum(text == 10)))[pos[:, 0].astype(np.int64)]
        assert rc.reference(oracle, case, text)[0] == len(set(lines.tolist())) > 100
