"""Every instantiation of the general multi-pattern kernel and every staging road, by name (tests/ac_road_cases.py): a case's count,
records and order equal the compiled reference's aho_corasick_search, and Plan.ac_last_scan() — which kernel answered, with which
stride, slot, ticket and emit pass — equals the report the case is there for.  A report that differs means the case's dictionary
or text misses its instantiation (or the launch rules changed): the case is mended, never the expectation.  Every case then runs
through three ownership windows at a global base: the start-owned lists merged by (end, start) are the whole list; under -c
krep_gpu_combine_line_counts over the windows is the reference's count."""
import numpy as np
import pytest

import ac_road_cases as rc
from krep_amd import abi

pytestmark = pytest.mark.gpu
CASES = rc.all_cases()


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


def records(pos, stored):
    return pos[: 2 * int(stored)].cpu().numpy().astype(np.uint64).reshape(-1, 2)


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_road(gpu, oracle_engine, resident, monkeypatch, case):
    import torch
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    plan = gpu.plan(case.params())  # a fresh plan: the stride is chosen when the dictionary is built, the slot is learned
    try:
        assert plan.ac_last_scan()["scans"] == 0 and plan.ac_last_scan(1) is None
        seen = {}
        for step, (text, _, expect) in enumerate(case.steps):
            n, d = text.size, resident(text)
            want_ret, want_pos = rc.reference(oracle_engine, case, text)
            seen[id(text)] = (text, want_ret, want_pos)
            tag = (case, step)
            if case.counting:
                assert plan.scan(d, n).count == want_ret, tag
            else:
                want = rc.kept(case, want_pos)
                cap = len(want_pos) + 16
                pos = torch.zeros(2 * cap, dtype=torch.int64, device="cuda")
                o = plan.scan(d, n, 0, n, 0, pos.data_ptr(), cap)
                got = records(pos, o.stored)
                assert o.count == want_ret and not o.overflow and len(got) == len(want), (tag, o.count, want_ret, len(got), len(want))
                assert np.array_equal(got, want), (tag, got[:4], want[:4])
            assert plan.ac_last_scan() == expect, (tag, plan.ac_last_scan(), expect)
        if case.whole_only:
            return
        for text, want_ret, want_pos in seen.values():
            n, d = text.size, resident(text)
            if case.counting:
                outs = [plan.scan(d, n, lo, hi, rc.BASE, global_len=rc.BASE + n) for lo, hi in rc.windows(n)]
                assert gpu.lib.krep_gpu_combine_line_counts((abi.ScanOut * len(outs))(*outs), len(outs)) == want_ret, case
                continue
            cap = len(want_pos) + 16
            pos = torch.zeros(2 * cap, dtype=torch.int64, device="cuda")
            parts = []
            for lo, hi in rc.windows(n):
                pos.zero_()
                o = plan.scan(d, n, lo, hi, rc.BASE, pos.data_ptr(), cap, global_len=rc.BASE + n)
                part = records(pos, o.stored)
                mine = want_pos[(want_pos[:, 0] >= lo) & (want_pos[:, 0] < hi)]
                assert not o.overflow and len(part) == len(mine) == o.count, (case, lo, hi, len(part), len(mine), o.count)
                parts.append(part)
            cat = np.concatenate(parts)
            cat = cat[np.lexsort((cat[:, 0], cat[:, 1]))]
            assert np.array_equal(cat, want_pos + np.uint64(rc.BASE)), case
    finally:
        plan.close()


def test_the_report_of_other_plans(gpu, oracle_engine):
    """a single-literal plan has no report; a tiny dictionary's names its own road, not the general kernel"""
    import torch
    lit = gpu.plan(abi.Params([b"abc"]))
    assert lit.ac_last_scan() is None
    lit.close()
    text = np.frombuffer(b"he said she hid hers\n" * 100, dtype=np.uint8)
    d = torch.from_numpy(text.copy()).cuda()
    tiny = gpu.plan(abi.Params([b"he", b"she", b"hers"]))
    try:
        assert tiny.ac_last_scan()["scans"] == 0
        want = oracle_engine.call(abi.RA_AHO_CORASICK, abi.Params([b"he", b"she", b"hers"]), text)[0]
        assert tiny.scan(d.data_ptr(), text.size).count == want == 500
        rep = tiny.ac_last_scan()
        assert (rep["road"], rep["scans"], rep["short_lens"], rep["emit"]) == (4, 1, 2 | 4, 0), rep
    finally:
        tiny.close()
