"""The conditions of tests/ac_tiny_cases.py, checked without a GPU against the compiled reference alone: the table names all 23
dispatched instantiations of ac_tiny_kernel, every plant is in aho_corasick_search's record list with the matches the case's report
was worked out from, the dense texts exceed the staging slot and the sparse ones do not, the text of the one-pass item writer stays
under 20 matches per unit and the dense writer's holds at least 48 (tiny_reopen / ac_tiny_one_pass, kg_ac.hip), every window of a
dense case keeps the dense writer, and the sweep ends a match of each length on every offset it claims.  These are conditions: a text
that misses one is changed, not the condition."""
import numpy as np
import pytest

import ac_tiny_cases as tc
import oracle_lib
from krep_amd import abi

CASES = tc.all_cases()
U = tc.U


@pytest.fixture(scope="module")
def oracle():
    return oracle_lib.checker()


_memo = {}


def records(oracle, case, text=None):
    """the reference's full record list of the case's search (no -c)"""
    text = case.text if text is None else text
    key = (id(text), tuple(case.pats), case.ci)
    if key not in _memo:
        _memo[key] = tc.reference(oracle, case.pats, case.kw, text, count_lines=False)
    return _memo[key]


def per_unit(pos, n):
    return np.bincount((pos[:, 1].astype(np.int64) - 1) // U, minlength=(n + U - 1) // U)


def test_the_table_names_every_instantiation():
    keys = [c.key for c in CASES]
    assert len(set(keys)) == len(keys) == 23
    long = {"none": 0, "long": 1}
    staged = {(c.ci, long[c.dname], c.mode, c.report["emit"] != 0, c.report["stage_cap"] > 0) for c in CASES if c.report["road"] == 4 and c.dname != "five"}
    assert staged == {(ci, lg) + m for ci in (False, True) for lg in (0, 1)
                      for m in (("count", False, False), ("lines", False, False), ("records", False, True), ("records", True, True))}
    assert sorted((c.ci, c.dname) for c in CASES if c.report["road"] == 2) == [(False, "none"), (True, "none")]
    assert sorted((c.ci, c.dname) for c in CASES if c.report["road"] == 3) == [(False, "long"), (False, "none"), (True, "long"), (True, "none")]
    assert [(c.ci, c.mode) for c in CASES if c.dname == "five"] == [(False, "count")]
    for c in CASES:
        n = c.text.size
        assert n == (tc.N_STAGED if c.report["road"] == 4 else tc.N_ONE_PASS) and c.report["n_units"] == (n + U - 1) // U
        assert (c.first is not None) == (c.report["road"] == 3)
        lens = sorted({len(p) for p in c.pats})
        assert lens == {"none": [1, 2, 3, 4], "long": [1, 2, 3, 7], "five": [2, 4, 5]}[c.dname]
        # the window cuts fall inside a lane-cell, above 2^32
        w = c.windows()
        assert w[0][0] == 0 and w[-1][1] == n and all(a[1] == b[0] and a[1] % 16 for a, b in zip(w, w[1:])) and tc.BASE > 1 << 32


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_plants_and_densities(oracle, case):
    n = case.text.size
    ret, pos = records(oracle, case)
    assert ret == len(pos) > 0
    s, e = pos[:, 0].astype(np.int64), pos[:, 1].astype(np.int64)
    # the reference's order: END ascending, the longest first
    assert np.all((np.diff(e) > 0) | ((np.diff(e) == 0) & (np.diff(s) > 0)))
    have = set(zip(s.tolist(), e.tolist()))
    for end in case.plants:
        for p in case.pats:
            if case.word.endswith(p) and len(p) <= end:
                assert (end - len(p), end) in have, (case, end, p)
    # byte 0, the last byte, a cell, a round and a unit seam inside a match; the tail is shorter than a lane's 16 bytes
    L = max(len(p) for p in case.pats if case.word.endswith(p))
    assert s.min() == 0 and (n - L, n) in have and 0 < n % 16 < 16
    for seam in (tc.CELL, tc.ROUND, U, 2 * U):
        assert np.any((s < seam) & (e > seam) & (e - s == L)), (case, seam)
    per = per_unit(pos, n)
    if case.dname != "five":
        assert np.array_equal(per, case.matches_per_unit()), (case, per, case.matches_per_unit())
        assert len(set(e.tolist())) * 2 < len(e)  # several patterns end on one byte
    if case.dname == "five":
        # the fifth class is there: every plant of `elsewhile` ends the long pattern `while` and holds the 4-byte `else` in front of
        # it, the 2-byte `if` occurs by chance, and the long pattern ends in the first dword behind a cell, a round and a unit seam (its
        # first byte is compared one dword earlier: in the bytes carried from the lane, the cell, the round in front)
        for end in case.plants:
            assert (end - 5, end) in have and (end < 9 or (end - 9, end - 5) in have), (case, end)
        assert {2, 4, 5} == set((e - s).tolist())
        for seam in (tc.CELL, tc.ROUND, U):
            assert np.any((e - s == 5) & (e > seam) & (e <= seam + 4)), (case, seam)
    rep = case.report
    # (a match belongs to the unit of its last byte: the lane-cell that holds it)
    if rep["road"] == 4 and rep["stage_cap"] and not rep["emit"]:
        assert 0 < per.max() <= tc.SLOT and rep["overflow_units"] == 0, (case, per)
    if rep["road"] == 4 and rep["emit"]:
        assert per.min() > tc.SLOT + 8 and rep["overflow_units"] == rep["n_units"], (case, per)
    if rep["road"] == 2:
        assert per.max() < 20 and len(pos) < 20 * rep["n_units"], (case, per.max())
    if rep["road"] == 3:
        fret, fpos = records(oracle, case, case.first[0])
        fn = case.first[0].size
        units = (fn + U - 1) // U
        # the first scan (staged: under 64 units) leaves the plan a density of >= 48 per unit, and the ticket the report names
        assert fn < 64 * U <= n and len(fpos) >= 48 * units and rep["upt"] == tc.dense_upt(len(fpos) / units) >= 1
        assert per.min() >= 48
        # ... and every scan, whole or windowed, holds >= 24 per unit of ITS grid: the plan stays with the dense writer
        for lo, hi in case.windows():
            mine = np.count_nonzero((s >= lo) & (s < hi))
            grid = (min(n, hi + 7) - (lo & ~15) + U - 1) // U
            assert mine >= 24 * grid and mine * 2.5 / grid * rep["upt"] <= tc.DENSE_RING, (case, lo, hi, mine, grid)
    if case.mode == "lines":
        lines = np.concatenate(([0], np.cumsum(case.text == 10)))[s]
        want = tc.reference(oracle, case.pats, case.kw, case.text)[0]
        assert want == len(set(lines.tolist())) and 3 < want < len(pos)  # (several matches on one line, several lines)


def test_the_ci_cases_find_more(oracle):
    by = {c.key: c for c in CASES}
    for d in ("none", "long"):
        assert len(records(oracle, by[f"{d}/staged-i"])[1]) > len(records(oracle, by[f"{d}/staged"])[1])


def test_the_sweep_ends_every_length_on_every_offset(oracle):
    offs = tc.sweep_offsets()
    assert set(range(tc.CELL)) <= set(offs) and all(set(range(s - 16, s + 16)) <= set(offs) for s in (tc.CELL, tc.ROUND, U))
    seen = {L: set() for L in (1, 2, 3, 4, 7)}
    texts = tc.sweep_texts()
    assert sorted(o for _, mine in texts for o in mine) == offs
    for text, mine in texts:
        assert text.size == tc.SWEEP_N == 2 * U
        ret, pos = tc.reference(oracle, tc.SWEEP_DICTS["s5"], {}, text)
        s, e = pos[:, 0].astype(np.int64), pos[:, 1].astype(np.int64)
        assert set((e - 1).tolist()) == set(mine)
        for a, b in zip(s.tolist(), e.tolist()):
            assert text[a:b].tobytes() in tc.SWEEP_DICTS["s5"] and text[a:b].tobytes() != b"\x00j"
            seen[b - a].add(b - 1)
        # the halves of the dictionary together hold the same records
        for name in ("s4", "s7"):
            r2, p2 = tc.reference(oracle, tc.SWEEP_DICTS[name], {}, text)
            keep = pos[np.isin(e - s, [len(p) for p in tc.SWEEP_DICTS[name]])]
            assert np.array_equal(p2, keep)
    for L in seen:  # a pattern that would begin before byte 0 is no match
        assert seen[L] == {o for o in offs if o >= L - 1}, L
