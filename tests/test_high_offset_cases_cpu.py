"""The conditions of tests/high_offset_cases.py, checked without a GPU: every case of tests/test_gpu_high_offsets.py really puts a
record across buffer offset X (global 2^32 at the base B1), one that ends on the cut Y and one that starts on the cut Z, its
reference list is not empty, and krep_gpu_mirror_select names the reference function the case is meant for at every base.  No case
may be dropped for an empty answer: the patterns and plants are chosen so that this holds."""
import numpy as np
import pytest

import high_offset_cases as hc
import oracle_lib
import regex_ref
from krep_amd import abi

CASES = hc.all_cases()


@pytest.fixture(scope="module")
def eng():
    import krep_amd
    e = krep_amd.load()
    yield e
    e.set_thread_config(None)


@pytest.fixture(scope="module")
def oracle():
    return oracle_lib.checker()


def test_the_table_holds_every_family():
    keys = [c.key for c in CASES]
    assert len(set(keys)) == len(keys)
    kinds = {k: sum(1 for c in CASES if c.kind == k) for k in ("lit", "seq", "block", "multi", "multi_nl", "regex")}
    from test_gpu_chain import BLOCK_JOBS, JOBS
    assert kinds == dict(lit=35, seq=len(JOBS) + 1, block=len(BLOCK_JOBS), multi=12, multi_nl=1, regex=10), kinds
    for c in CASES:
        assert c.text.size == hc.N and c.text[0] == 10 and all(p[:1] != b"\n" for p in c.pats), c
    assert {c.counter for c in CASES} == {None, "single_launches", "runs_launches", "tiny_launches"}
    seven = next(c for c in CASES if c.key == "multi/seven/plain")
    assert len(seven.pats) == 7 and min(map(len, seven.pats)) == 2 and max(map(len, seven.pats)) == 30
    assert all(len(p) <= 4 for c in CASES if c.key.startswith("multi/tiny") for p in c.pats)


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_selector(eng, case):
    if case.kind == "regex":
        with regex_ref.c_locale():
            assert hc.regex_compiler(eng, case) == case.algo
        return
    for base in hc.BASES:
        assert hc.select(eng, case, base + hc.N) == case.algo, (case, base)


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_plants_are_in_the_reference_list(eng, oracle, case):
    X, Y, Z = hc.X, hc.Y, hc.Z
    for base in hc.BASES:
        # (a -c case: the records of the same search without -c are its witnesses; a dictionary with a newline pattern: its plain list)
        over = dict(count_lines=False) if case.kw.get("count_lines") else {}
        ret, pos = hc.reference(oracle, eng, case, base, **over)
        pos = hc.kept(case, pos)
        assert ret > 0 and len(pos) > 0, (case, base)
        if case.kw.get("count_lines"):
            assert hc.reference(oracle, eng, case, base)[0] > 0, (case, base)
        s, e = pos[:, 0].astype(np.int64), pos[:, 1].astype(np.int64)
        m = max(len(p) for p in case.pats)
        if m == 1:
            assert np.any((s == X - 1) & (e == X)), (case, base)
        else:
            assert np.any((s < X) & (X < e)), (case, base)
        assert (np.any(e == Y) or "max_count" in case.kw) and np.any(s == Z), (case, base)  # (max_count cuts between X and Y)
        if case.kind == "multi" and not case.kw.get("whole_word"):  # (-w: the bytes at X stand inside the long plant, no word)
            assert np.any(s == X), (case, base)  # beside the straddling record
        if base == hc.B1:
            g = pos.astype(object) + base
            assert any(int(a) < (1 << 32) <= int(b) for a, b in g), (case, base)
        if "max_count" in case.kw:
            full = hc.reference(oracle, eng, case, base, max_count=abi.SIZE_MAX)[1]
            assert len(full) > len(pos) == case.kw["max_count"], (case, len(full))  # the cut is a real one, behind X
