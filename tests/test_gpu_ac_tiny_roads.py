"""Every dispatched instantiation of the tiny-dictionary kernel, by name (tests/ac_tiny_cases.py): a case's count, records and order
equal the compiled reference's aho_corasick_search, and Plan.ac_last_scan() — which road answered, -i, -c, the slot, the ticket, the
emit pass, the units that overflowed — equals the report the case is there for.  A report that differs means the case's text misses
its instantiation (or the launch rules changed): the case is mended, never the expectation.  Every case then runs through three
ownership windows at a global base above 2^32 whose cuts fall inside a lane-cell, on the same road: the start-owned lists merged by
(end, start) are the whole list, the counts add up, and under -c krep_gpu_combine_line_counts over the windows is the reference's
count.  The seam sweep ends a match of every length on every offset of a cell and around the cell, round and unit seams."""
import numpy as np
import pytest

import ac_tiny_cases as tc
from krep_amd import abi

pytestmark = pytest.mark.gpu
CASES = tc.all_cases()


@pytest.fixture(scope="module")
def gpu():
    import krep_amd
    e = krep_amd.load()
    assert e.device_count() >= 1
    e.force_stage_cap(0)  # (a forced slot ends ac_learn early: these cases are about the learned one)
    return e


@pytest.fixture(scope="module")
def resident():
    """the texts on the device, one upload each (cases share them)"""
    held = {}

    def get(text):
        import torch
        if id(text) not in held:
            t = torch.full((text.size + 64,), 0xEE, dtype=torch.uint8, device="cuda")
            t[: text.size] = torch.from_numpy(text)
            held[id(text)] = t
        return held[id(text)].data_ptr()
    yield get
    held.clear()


_ref = {}


def reference(oracle, pats, kw, text):
    key = (id(text), tuple(pats), tuple(sorted(kw.items())))
    if key not in _ref:
        _ref[key] = tc.reference(oracle, pats, kw, text)
    return _ref[key]


def records(pos, stored):
    return pos[: 2 * int(stored)].cpu().numpy().astype(np.uint64).reshape(-1, 2)


def scan_records(plan, d, n, want_pos, tag, lo=0, hi=None, base=0):
    """the plan's record list of [lo, hi) — the complete list, as many as the scan counted"""
    import torch
    cap = len(want_pos) + 16
    pos = torch.zeros(2 * cap, dtype=torch.int64, device="cuda")
    o = plan.scan(d, n, lo, n if hi is None else hi, base, pos.data_ptr(), cap, global_len=base + n if base else 0)
    got = records(pos, o.stored)
    assert not o.overflow and len(got) == o.count, (tag, lo, hi, len(got), o.count)
    return got


def report(plan):
    rep = plan.ac_last_scan()
    return {k: rep[k] for k in tc.REPORT_KEYS}


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_tiny_road(gpu, oracle_engine, resident, monkeypatch, case):
    monkeypatch.delenv("KREP_GPU_AC_UPT", raising=False)
    plan = gpu.plan(case.params())  # a fresh plan: its slot and its one-pass roads are as a dictionary starts
    try:
        assert plan.ac_last_scan()["scans"] == 0
        text, n, d = case.text, case.text.size, resident(case.text)
        want_ret, want_pos = reference(oracle_engine, case.pats, case.kw, text)
        if case.first is not None:  # the scan that counts the density (staged, with records)
            ft = case.first[0]
            fret, fpos = reference(oracle_engine, case.pats, case.kw, ft)
            assert np.array_equal(scan_records(plan, resident(ft), ft.size, fpos, (case, "first")), fpos), (case, "first")
            assert plan.ac_last_scan()["road"] == 4, (case, plan.ac_last_scan())
        if case.mode == "records":
            got = scan_records(plan, d, n, want_pos, case)
            assert len(got) == len(want_pos) == want_ret and np.array_equal(got, want_pos), (case, got[:4], want_pos[:4])
        else:
            assert plan.scan(d, n).count == want_ret, case
        assert report(plan) == case.report, (case, plan.ac_last_scan(), case.report)
        # ---- three windows at a global base, on the same road
        outs, parts = [], []
        for lo, hi in case.windows():
            if case.mode == "records":
                part = scan_records(plan, d, n, want_pos, case, lo, hi, tc.BASE)
                mine = want_pos[(want_pos[:, 0] >= lo) & (want_pos[:, 0] < hi)]
                assert len(part) == len(mine), (case, lo, hi, len(part), len(mine))
                parts.append(part)
            else:
                outs.append(plan.scan(d, n, lo, hi, tc.BASE, global_len=tc.BASE + n))
            rep = plan.ac_last_scan()
            assert (rep["road"], rep["ci"], rep["lines"]) == (case.report["road"], case.report["ci"], case.report["lines"]), (case, lo, hi, rep)
        if case.mode == "records":
            cat = np.concatenate(parts)
            cat = cat[np.lexsort((cat[:, 0], cat[:, 1]))]
            assert np.array_equal(cat, want_pos + np.uint64(tc.BASE)), case
        elif case.mode == "lines":
            assert gpu.lib.krep_gpu_combine_line_counts((abi.ScanOut * len(outs))(*outs), len(outs)) == want_ret, case
        else:
            assert sum(o.count for o in outs) == want_ret, (case, [o.count for o in outs], want_ret)
    finally:
        plan.close()


@pytest.mark.parametrize("name", sorted(tc.SWEEP_DICTS))
def test_seam_sweep(gpu, oracle_engine, monkeypatch, name):
    """tickets of two units: the carries of the last lane's bytes run across the cell, the round AND the unit seam (a ticket of one
    unit reads them from memory at its first round).  The whole dictionary `s5` holds 4-byte patterns beside the 7-byte one: a fifth
    class, which the kernel takes for the case-sensitive COUNT alone — a count cannot tell a wrong start or length at a seam, so the
    7-byte look-back is checked with records through the half `s7` (the same compare in the place of class 4) and `s5` checks that
    the fifth class counts every END once.  That is the limit of this case."""
    import torch
    monkeypatch.setenv("KREP_GPU_AC_UPT", "2")
    pats = tc.SWEEP_DICTS[name]
    count_only = name == "s5"  # (a fifth class: the kernel takes the case-sensitive count, ac_scan)
    modes = [({}, "count")] if count_only else [({}, "records"), (dict(case_sensitive=False), "records"), (dict(count_lines=True), "lines")]
    for kw, mode in modes:
        plan = gpu.plan(abi.Params(pats, **kw))
        try:
            for k, (text, _) in enumerate(tc.sweep_texts()):
                n = text.size
                t = torch.full((n + 64,), 0xEE, dtype=torch.uint8, device="cuda")
                t[:n] = torch.from_numpy(text)
                want_ret, want_pos = tc.reference(oracle_engine, pats, kw, text)
                if mode == "records":
                    got = scan_records(plan, t.data_ptr(), n, want_pos, (name, kw, k))
                    assert len(got) == len(want_pos) and np.array_equal(got, want_pos), (name, kw, k, got[:4], want_pos[:4])
                else:
                    assert plan.scan(t.data_ptr(), n).count == want_ret, (name, kw, k)
                rep = plan.ac_last_scan()
                assert (rep["road"], rep["upt"], rep["n_units"]) == (4, 2, 2), (name, kw, k, rep)
        finally:
            plan.close()
