"""Scans of a small resident text at a global_base that needs 33 and 35 bits (tests/high_offset_cases.py): every record the library
writes is (offset within the buffer) + global_base, and a 32-bit intermediate anywhere in that sum — the kernels' record stores, the
ordering post-passes, the greedy walks, the carries of krep_gpu_seq_carry_t — passes every other small test.  The expected lists
are the compiled reference's on the text's own bytes, + the base; base 0 is the control.  Which kernel answered: the value
krep_gpu_mirror_select names (asserted in tests/test_high_offset_cases_cpu.py) and, where a family has a launch counter, that one."""
import ctypes as C

import numpy as np
import pytest

import high_offset_cases as hc
import regex_ref
from krep_amd import abi

pytestmark = pytest.mark.gpu

N, CUTS, BASES = hc.N, hc.CUTS, hc.BASES
CASES = hc.all_cases()
# one case per family is also scanned with global_len = 0 ("the buffer ends the text"), which must answer the same
ALSO_ZERO_LEN = {next(c.key for c in CASES if c.kind == k) for k in ("lit", "seq", "block", "multi", "multi_nl", "regex")}
OFFSET_FIELDS = ("resume", "q1", "nl1", "g0")  # of krep_gpu_seq_carry_t: global offsets (q1, nl1, g0 stored + 1), 0 = none


@pytest.fixture(autouse=True, scope="module")
def _c_locale():
    with regex_ref.c_locale():  # the locale the reference runs in: the regex plans are refused in any other
        yield


@pytest.fixture(scope="module")
def gpu():
    import krep_amd
    e = krep_amd.load()
    assert e.device_count() >= 1
    yield e
    e.set_reference_simd(abi.REF_AVX2)
    e.force_rounds(0)
    e.force_stage_cap(0)
    e.set_regex_loops(False)


@pytest.fixture(scope="module")
def resident():
    """the texts on the device, one upload each (cases share them)"""
    held = {}

    def get(case):
        import torch
        key = id(case.text)
        if key not in held:
            t = torch.full((N + 64,), 0xEE, dtype=torch.uint8, device="cuda")
            t[:N] = torch.from_numpy(case.text)
            held[key] = t
        return held[key].data_ptr()
    yield get
    held.clear()


def make_plan(gpu, case):
    gpu.set_reference_simd(case.level)
    gpu.force_rounds(case.rounds)
    gpu.force_stage_cap(case.stage_cap)
    return gpu.plan(case.params(), only_matching=case.om)


def records(pos, stored):
    return pos[: 2 * int(stored)].cpu().numpy().astype(np.uint64).reshape(-1, 2)


def lengths(case, base):
    return (base + N, 0) if case.key in ALSO_ZERO_LEN else (base + N,)


def counter(gpu, case):
    """(the count that must move, the count that must not) of the case's launch counters"""
    return (getattr(gpu, case.counter)() if case.counter else 0, getattr(gpu, case.idle)() if case.idle else 0)


def moved_as_meant(gpu, case, before):
    now = counter(gpu, case)
    return (now[0] > before[0] or not case.counter) and now[1] == before[1]


def window_list(case, base):
    """the windows of a non-sequential case: the cuts, and the whole window.  A regex with ^ does not take buffer byte 0 at a base > 0"""
    first = 1 if (case.algo == "bol" and base > 0) else 0
    cuts = [first] + CUTS[1 + first:]
    return list(zip(cuts[:-1], cuts[1:])), (first, N)


@pytest.mark.parametrize("case", [c for c in CASES if c.kind in ("lit", "multi", "regex")], ids=repr)
def test_windows_at_a_high_base(gpu, oracle_engine, resident, case):
    import torch
    d = resident(case)
    plan = make_plan(gpu, case)
    try:
        for base in BASES:
            want_ret, want_pos = hc.reference(oracle_engine, gpu, case, base)
            windows, whole = window_list(case, base)
            cap = (0 if case.counting else len(want_pos)) + 16
            pos = torch.zeros(2 * cap, dtype=torch.int64, device="cuda")
            for glen in lengths(case, base):
                tag = (case, base, glen)
                if case.counting:
                    before = counter(gpu, case)
                    assert plan.scan(d, N, *whole, base, global_len=glen).count == want_ret, tag
                    assert moved_as_meant(gpu, case, before), (tag, case.counter, case.idle)
                    outs = [plan.scan(d, N, lo, hi, base, global_len=glen) for lo, hi in windows]
                    assert gpu.lib.krep_gpu_combine_line_counts((abi.ScanOut * len(outs))(*outs), len(outs)) == want_ret, tag
                    continue
                before = counter(gpu, case)
                o = plan.scan(d, N, *whole, base, pos.data_ptr(), cap, global_len=glen)
                assert moved_as_meant(gpu, case, before), (tag, case.counter, case.idle)
                want = hc.kept(case, want_pos).astype(object) + base
                got = records(pos, o.stored)
                assert o.count == want_ret and not o.overflow and len(got) == len(want), (tag, o.count, want_ret, len(got), len(want))
                assert np.array_equal(got.astype(object), want), (tag, got[:4], want[:4])
                assert plan.scan(d, N, *whole, base, global_len=glen).count == want_ret, tag  # count only
                if case.whole_only:
                    continue
                parts, total = [], 0
                for lo, hi in windows:
                    pos.zero_()
                    o = plan.scan(d, N, lo, hi, base, pos.data_ptr(), cap, global_len=glen)
                    assert not o.overflow
                    part = records(pos, o.stored)
                    mine = want_pos[(want_pos[:, 0] >= lo) & (want_pos[:, 0] < hi)]
                    assert len(part) == len(mine) == o.count, (tag, lo, hi, len(part), len(mine), o.count)
                    parts.append(part)
                    total += o.total_matches
                cat = np.concatenate(parts)
                if len(case.pats) > 1:  # per-window lists are (end, start)-ordered; the text's order needs the merge
                    cat = cat[np.lexsort((cat[:, 0], cat[:, 1]))]
                assert total == want_ret and np.array_equal(cat.astype(object), want), (tag, total, want_ret)
    finally:
        plan.close()
        gpu.force_rounds(0)
        gpu.force_stage_cap(0)
        gpu.set_reference_simd(abi.REF_AVX2)


def chained(gpu, case):
    cfg = gpu.default_config()
    cfg.reference_simd, cfg.only_matching = case.level, int(case.om)
    gpu.set_thread_config(cfg)
    try:
        return gpu.split_mode(case.params(), hc.B2 + N) == abi.SPLIT_CHAIN
    finally:
        gpu.set_thread_config(None)


def carries_lie_behind(base, carry, tag):
    for f in OFFSET_FIELDS:
        v = int(getattr(carry, f))
        assert v == 0 or v > base, (tag, f, v, base)  # a truncated carry that happens to give the right list is still caught


def chain(gpu, plan, d, base, glen, pieces, cap, tag):
    """the pieces in text order through Plan.scan_seq -> (outs, record lists, carries out); the first piece of a base > 0 takes a
    zeroed record"""
    import torch
    carry = abi.SeqCarry() if base else None
    pos = torch.zeros(2 * max(cap, 1), dtype=torch.int64, device="cuda")
    outs, recs, carries = [], [], []
    for lo, hi in pieces:
        o, carry = plan.scan_seq(d, N, lo, hi, base, pos.data_ptr() if cap else 0, cap, global_len=glen, carry_in=carry)
        assert not o.overflow, tag
        outs.append(o)
        recs.append(records(pos, o.stored) if cap else np.zeros((0, 2), dtype=np.uint64))
        carries.append(carry)
        if base:
            carries_lie_behind(base, carry, tag + (lo, hi))
    return outs, recs, carries


@pytest.mark.parametrize("case", [c for c in CASES if c.kind in ("seq", "multi_nl")], ids=repr)
def test_chained_pieces_at_a_high_base(gpu, oracle_engine, resident, case):
    import krep_amd
    d = resident(case)
    plan = make_plan(gpu, case)
    pieces = [(0, N)] if case.whole_only else list(zip(CUTS[:-1], CUTS[1:]))
    try:
        if chained(gpu, case) and case.kind == "seq":
            # the plain entry point passes no record: a buffer inside the text is refused, never approximated
            with pytest.raises(krep_amd.KrepGpuError, match="krep_gpu_scan_device_seq"):
                plan.scan(d, N, 0, N, hc.B1, global_len=hc.B1 + N)
        for base in BASES:
            want_ret, want_pos = hc.reference(oracle_engine, gpu, case, base)
            listed = not case.counting and not case.count_only
            cap = len(want_pos) + 16 if listed else 0
            for glen in lengths(case, base):
                tag = (case, base, glen)
                before = counter(gpu, case)
                outs, recs, carries = chain(gpu, plan, d, base, glen, pieces, cap, tag)
                assert moved_as_meant(gpu, case, before), (tag, case.counter, case.idle)
                if case.kind == "multi_nl":
                    assert sum(o.line_count for o in outs) == want_ret, tag
                elif case.counting:
                    assert gpu.lib.krep_gpu_combine_line_counts((abi.ScanOut * len(outs))(*outs), len(outs)) == want_ret, tag
                elif case.count_only:
                    assert sum(o.count for o in outs) == want_ret, tag
                else:
                    got, want = np.concatenate(recs), hc.kept(case, want_pos).astype(object) + base
                    assert len(got) == len(want) and np.array_equal(got.astype(object), want), (tag, len(got), len(want))
                    if case.whole_only:
                        assert outs[0].count == want_ret, tag
                if base and case.kind == "seq" and not case.whole_only and chained(gpu, case):
                    assert any(int(c.resume) for c in carries), (tag, "no piece left a resume offset: the chain was not exercised")
    finally:
        plan.close()
        gpu.set_reference_simd(abi.REF_AVX2)


@pytest.mark.parametrize("case", [c for c in CASES if c.kind == "block"], ids=repr)
def test_block_loop_count_lines_and_the_replay_at_a_high_base(gpu, oracle_engine, resident, case):
    """-c through the block loops: the chain's count, the history offsets q1 / nl1 / g0 on every carry, and krep_gpu_replay_tail on the
    last 512 bytes with the true record, which must report what the chain's last piece reported and leave the record it left"""
    L = gpu.lib
    L.krep_gpu_replay_tail.restype = C.c_int
    L.krep_gpu_replay_tail.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.POINTER(abi.SeqCarry),
                                       C.POINTER(abi.SeqCarry), C.POINTER(abi.SeqCarry), C.POINTER(C.c_uint64)]
    d = resident(case)
    plan = make_plan(gpu, case)
    pieces = list(zip(CUTS[:-1], CUTS[1:]))
    import krep_amd
    try:
        assert chained(gpu, case)
        with pytest.raises(krep_amd.KrepGpuError, match="krep_gpu_scan_device_seq"):  # the plain entry point passes no record
            plan.scan(d, N, 0, N, hc.B1, global_len=hc.B1 + N)
        for base in BASES:
            want_ret, _ = hc.reference(oracle_engine, gpu, case, base)
            for glen in lengths(case, base):
                tag = (case, base, glen)
                outs, _, carries = chain(gpu, plan, d, base, glen, pieces, 0, tag)
                assert gpu.lib.krep_gpu_combine_line_counts((abi.ScanOut * len(outs))(*outs), len(outs)) == want_ret, tag
                if base:
                    assert int(carries[-1].q1) > base and int(carries[-2].q1) > base, tag  # (occurrences stand in every piece but the first)
                lines, left = C.c_uint64(0), abi.SeqCarry()
                rc = L.krep_gpu_replay_tail(plan.h, C.c_void_p(d + N - 512), 512, base + N, None, C.byref(carries[-2]), C.byref(carries[-1]),
                                            C.byref(left), C.byref(lines))
                assert rc == 0, (tag, gpu.last_error())
                assert int(lines.value) == outs[-1].line_count, (tag, int(lines.value), outs[-1].line_count)
                assert bytes(left) == bytes(carries[-1]), tag
    finally:
        plan.close()
        gpu.set_reference_simd(abi.REF_AVX2)


def test_refusals_at_a_high_base(gpu, resident):
    """a regex with ^ does not take buffer byte 0 of a buffer inside the text; the loops compiler takes one window with base 0 only"""
    import krep_amd
    bol = next(c for c in CASES if c.key == "regex/bol/rec")
    d = resident(bol)
    plan = make_plan(gpu, bol)
    try:
        with pytest.raises(krep_amd.KrepGpuError, match="regex with \\^"):
            plan.scan(d, N, 0, N, hc.B1, global_len=hc.B1 + N)
    finally:
        plan.close()
    gpu.set_regex_loops(True)
    try:
        plan = gpu.plan(abi.Params([hc.LOOPS_PATTERN], regex=True))
        try:
            with pytest.raises(krep_amd.KrepGpuError, match="walked line by line"):
                plan.scan(d, N, 1, N, hc.B1, global_len=hc.B1 + N)
        finally:
            plan.close()
    finally:
        gpu.set_regex_loops(False)
