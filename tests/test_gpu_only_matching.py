"""krep_gpu_format_matches / Plan.grep_only_matching: the reference's -o output (one FILE:LINE:match per match;
print_matching_items() in only-matching mode, krep.c:517-793) produced on the device, byte for byte — against
tests/only_matching_model.py and against the stock CLI (oracle/_ref/krep -t 1 -o) wherever that binary exists."""
import hashlib
import os

import numpy as np
import pytest

import only_matching_model as om
import oracle_lib as ol
from krep_amd import abi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = ol.ref_cli()
STORE = om.Store()
LIVE = {"table": 0, "rand": 0, "gib": 0}  # cases the live CLI answered
PAD = 0xEE


@pytest.fixture(scope="module")
def gpu():
    import krep_amd
    e = krep_amd.load()
    assert e.device_count() >= 1
    return e


def to_device(text, shift=0):
    """(tensor that owns the bytes, device pointer of text[0]); shift: the text starts that many bytes into the allocation"""
    import torch
    a = np.frombuffer(bytes(text), dtype=np.uint8) if not isinstance(text, np.ndarray) else text
    t = torch.full((a.size + shift + 64,), PAD, dtype=torch.uint8, device="cuda")
    if a.size:
        t[shift:shift + a.size] = torch.from_numpy(a.copy())
    return t, t.data_ptr() + shift


def records_to_device(recs):
    import torch
    a = np.asarray(recs, dtype=np.uint64).reshape(-1, 2)
    return torch.from_numpy(a.astype(np.int64)).cuda().contiguous(), len(a)


def check_raw_call(gpu, d_text, n, recs, strings, max_items, want, out_shift=0):
    """the raw call on a record list against the model's bytes: size query, exact capacity, capacity one short"""
    import torch
    pos, m = records_to_device(recs)
    limit = abi.SIZE_MAX if max_items is None else max_items
    items = min(m, limit)
    fmt = abi.MatchFormat(*strings) if strings is not None else None
    q = gpu.format_matches(d_text, n, pos.data_ptr(), m, limit, fmt)
    assert (q.out_bytes, q.items, q.overflow) == (len(want), items, 0)
    buf = torch.full((len(want) + 64,), PAD, dtype=torch.uint8, device="cuda")
    r = gpu.format_matches(d_text, n, pos.data_ptr(), m, limit, fmt, buf.data_ptr() + out_shift, len(want))
    got = buf.cpu().numpy()
    assert not r.overflow and (r.out_bytes, r.items) == (len(want), items)
    assert got[out_shift:out_shift + len(want)].tobytes() == want
    assert (got[:out_shift] == PAD).all() and (got[out_shift + len(want):] == PAD).all()  # nothing outside [0, out_bytes)
    if len(want) > 1:
        buf.fill_(PAD)
        r = gpu.format_matches(d_text, n, pos.data_ptr(), m, limit, fmt, buf.data_ptr() + out_shift, len(want) - 1)
        assert r.overflow == 1 and (r.out_bytes, r.items) == (len(want), items)
        assert (buf.cpu().numpy()[out_shift + len(want) - 1:] == PAD).all()


def check_case(gpu, chk, case, tmp_path, idx):
    emitted = case.emitted(chk, abi)
    recs = om.lm.cut_to_max_count(emitted, case.max_count)
    n = len(case.text)
    gpu.set_force_no_simd(case.no_simd)
    try:
        plan = gpu.plan(case.params(abi), only_matching=True)
        # with and without FILE:, with and without colour; each on a text base misaligned by another of 0, 3, 7, 13
        for j, (name, color) in enumerate(((om.FILE, False), (None, False), (om.FILE, True), (None, True))):
            strings = om.strings(name, color)
            want = om.only_matching_output(case.text, recs, strings)
            if name is not None and (not color or idx % 4 == 0 or case.want is not None):
                live = None
                if CLI:
                    path = tmp_path / "t.txt"
                    path.write_bytes(case.text)
                    rc, out = om.run_cli(CLI, case, path, color)
                    assert out == want and rc == (0 if out else 1), (case.key, case.cli_args(color))
                    live = om.digest(rc, out)
                    LIVE[case.key.split("/")[0]] += not color
                assert om.digest(0 if want else 1, want) == STORE.want(case.key + ("/color" if color else ""), live), case.key
                if case.want is not None and not color:
                    assert want == case.want
            keep, d_text = to_device(case.text, (0, 3, 7, 13)[(j + idx) % 4])
            check_raw_call(gpu, d_text, n, recs, strings, None, want, out_shift=(0, 5)[(j + idx // 4) % 2])
            if j == idx % 4:
                cut = om.only_matching_output(case.text, recs, strings, 2)  # max_items cuts the output, not the list
                check_raw_call(gpu, d_text, n, recs, strings, 2, cut, out_shift=5)
                check_raw_call(gpu, d_text, n, recs, None, None, om.only_matching_output(case.text, recs))  # fmt = NULL
            got = plan.grep_only_matching(d_text, n, filename=name, max_count=case.max_count, color=color)
            assert got == want, (case.key, case.pats, name, color)
            del keep
        plan.close()
    finally:
        gpu.set_force_no_simd(False)


def test_table_rows(gpu, oracle_engine, tmp_path):
    for idx, case in enumerate(om.table_cases()):
        check_case(gpu, oracle_engine, case, tmp_path, idx)


def test_random_cases(gpu, oracle_engine, tmp_path):
    cases = om.random_cases()
    assert len(cases) >= 240
    for idx, case in enumerate(cases):
        check_case(gpu, oracle_engine, case, tmp_path, idx)


def test_one_line_of_8_mib_with_100000_records(gpu):
    n = 8 << 20
    a = np.full(n, ord("x"), dtype=np.uint8)
    a[0::64] = ord("a")
    a[1::64] = ord("b")
    text = a.tobytes()
    recs = [(i, i + 2) for i in range(0, n, 64)]
    assert len(recs) >= 100_000
    keep, d_text = to_device(a)
    for strings in (om.strings(b"big.txt"), om.strings(None, True)):
        want = om.only_matching_output(text, recs, strings)
        check_raw_call(gpu, d_text, n, recs, strings, None, want)
    plan = gpu.plan(abi.Params([b"ab"]), only_matching=True)
    assert plan.grep_only_matching(d_text, n) == b"1:ab\n" * len(recs)
    # ... and long overlapping records on it: most output chunks lie wholly inside one match
    recs = [(i, i + 1000) for i in range(0, n - 1000, 4096)]
    check_raw_call(gpu, d_text, n, recs, om.strings(b"f"), None, om.only_matching_output(text, recs, om.strings(b"f")), out_shift=3)


def test_matches_with_newlines_inside_and_text_edges(gpu):
    rng = np.random.RandomState(11)
    a = rng.choice(np.frombuffer(b"abcdefgh\n", dtype=np.uint8), size=300_000)
    a[:2] = (ord("a"), ord("b"))
    a[-40:] = ord("c")  # a last line without a newline
    text = a.tobytes()
    starts = sorted(set(int(x) for x in rng.randint(0, len(text) - 1, size=3000)) | {0, len(text) - 1, len(text) - 17})
    recs = [(s, min(len(text), s + int(rng.choice([0, 1, 5, 16, 17, 40, 200])))) for s in starts]
    recs[-1] = (len(text) - 1, len(text) + 5)  # an end behind the text is clamped
    for shift in (0, 9):
        keep, d_text = to_device(a, shift)
        for strings in (om.strings(b"f"), om.strings(None)):
            check_raw_call(gpu, d_text, len(text), recs, strings, None, om.only_matching_output(text, recs, strings), out_shift=shift % 4)
        check_raw_call(gpu, d_text, len(text), recs, om.strings(b"f", True), 1000,
                       om.only_matching_output(text, recs, om.strings(b"f", True), 1000))


def test_48_mib_dictionary_text(gpu):
    import torch
    import bench
    pats = bench.ac_patterns()
    n = (48 << 20) + 123
    buf = torch.empty(n + 64, dtype=torch.uint8, device="cuda")
    gpu.generate(buf.data_ptr(), n, 0, 4, bench.SEED, bench.pack_dict(pats), 4096)
    cap = n // 500
    pos = torch.empty(2 * cap, dtype=torch.int64, device="cuda")
    plan = gpu.plan(abi.Params(pats), only_matching=True)
    out = plan.scan(buf.data_ptr(), n, 0, n, 0, pos.data_ptr(), cap)
    assert not out.overflow and out.stored > 10000
    m = int(out.stored)
    gpu.order_by_start(pos.data_ptr(), m, n)  # the record list ordered on the device
    recs = [tuple(x) for x in pos[: 2 * m].view(-1, 2).cpu().numpy().astype(np.int64).tolist()]
    tb = buf[:n].cpu().numpy().tobytes()
    for strings, mc in ((om.strings(b"dict.txt"), None), (om.strings(None, True), 1000)):
        want = om.only_matching_output(tb, recs, strings, mc)
        q = gpu.format_matches(buf.data_ptr(), n, pos.data_ptr(), m, abi.SIZE_MAX if mc is None else mc, abi.MatchFormat(*strings))
        assert q.out_bytes == len(want)
        dst = torch.full((len(want) + 64,), PAD, dtype=torch.uint8, device="cuda")
        r = gpu.format_matches(buf.data_ptr(), n, pos.data_ptr(), m, abi.SIZE_MAX if mc is None else mc, abi.MatchFormat(*strings),
                               dst.data_ptr() + 1, len(want))
        got = dst.cpu().numpy()
        assert not r.overflow and got[1:1 + len(want)].tobytes() == want and got[0] == PAD and (got[1 + len(want):] == PAD).all()
    assert plan.grep_only_matching(buf.data_ptr(), n, filename="dict.txt") == om.only_matching_output(tb, recs, om.strings(b"dict.txt"))


def test_a_long_stale_suffix_and_the_threshold(gpu):
    rng = np.random.RandomState(3)
    a = rng.choice(np.frombuffer(b"abcd    \n", dtype=np.uint8), size=3 << 20)
    a[-(1 << 20):][a[-(1 << 20):] == 10] = ord("e")  # the last 1 MiB has no newline
    a[(2 << 20) - 7] = 10
    text = a.tobytes()
    last_nl = text.rfind(b"\n")
    assert len(text) - last_nl > (1 << 20)
    recs = [(int(s), int(s) + 2) for s in np.flatnonzero((a[:-1] == ord("a")) & (a[1:] == ord("b")))]
    behind = sum(1 for s, _ in recs if s > last_nl)
    assert behind > 11 and om.stale_records(text, recs) == behind
    keep, d_text = to_device(a, 5)
    true = 1 + text.count(b"\n")
    nums = om.line_numbers(text, recs)
    assert nums[-1] == nums[-behind - 1] < true  # what the suffix prints is the number in front of it, not its own
    for strings in (om.strings(b"f"), om.strings(b"f", True)):
        check_raw_call(gpu, d_text, len(text), recs, strings, None, om.only_matching_output(text, recs, strings))
    # exactly 10 and exactly 11 records on the same text, the last three of them behind the last newline
    tail = [r for r in recs if r[0] > last_nl]
    head = [r for r in recs if r[0] <= last_nl]
    for k in (10, 11):
        lst = head[-(k - 3):] + tail[:3]
        nums = om.line_numbers(text, lst)
        assert len(lst) == k and nums[-1] == (true if k == 10 else nums[k - 4]) and (k == 10 or nums[-1] < true)
        check_raw_call(gpu, d_text, len(text), lst, om.strings(b"f"), None, om.only_matching_output(text, lst, om.strings(b"f")),
                       out_shift=5)
    # all records behind the last newline: 1
    lst = tail[:12]
    want = om.only_matching_output(text, lst, om.strings(None))
    assert want == b"1:ab\n" * 12
    check_raw_call(gpu, d_text, len(text), lst, om.strings(None), None, want)


def test_1_gib_of_the_bench_text_against_the_cli(gpu, tmp_path):
    import torch
    import bench
    n = 1 << 30
    buf = torch.empty(n + 64, dtype=torch.uint8, device="cuda")
    gpu.generate(buf.data_ptr(), n, 0, 2, bench.SEED, bench.PATTERN, bench.PERIOD)
    path = tmp_path / "literal8.txt"
    plan = gpu.plan(abi.Params([bench.PATTERN]), only_matching=True)
    got = plan.grep_only_matching(buf.data_ptr(), n, filename=str(path))
    assert len(got) > 100_000
    got = got.replace(str(path).encode(), om.FILE)
    live = None
    if CLI:
        import subprocess
        buf[:n].cpu().numpy().tofile(str(path))
        r = subprocess.run([CLI, "-t", "1", "-o", "--color=never", bench.PATTERN.decode(), str(path)], capture_output=True, timeout=600)
        os.remove(path)
        out = r.stdout.replace(str(path).encode(), om.FILE)
        assert hashlib.sha256(got).hexdigest() == hashlib.sha256(out).hexdigest() and r.returncode == 0
        live = om.digest(r.returncode, out)
        LIVE["gib"] += 1
    else:
        pos_n = got.count(b"\n")
        text = buf[:n].cpu().numpy().tobytes()
        recs, i = [], text.find(bench.PATTERN)
        while i >= 0:
            recs.append((i, i + len(bench.PATTERN)))
            i = text.find(bench.PATTERN, i + len(bench.PATTERN))
        assert pos_n == len(recs) and got == om.only_matching_output(text, recs, om.strings(om.FILE))
    assert om.digest(0, got) == STORE.want("gib/literal8", live)


def test_refused_record_lists(gpu):
    import torch
    import krep_amd
    text = b"ab\nab\nab\n"
    keep, d_text = to_device(text)
    buf = torch.full((256,), PAD, dtype=torch.uint8, device="cuda")
    for recs in ([(3, 5), (0, 2)], [(0, 2), (9, 11)], [(0, 2), (1 << 40, (1 << 40) + 2)], [(4, 3)]):
        pos, m = records_to_device(recs)
        out = abi.MatchesOut()
        gpu.lib.krep_gpu_clear_error()
        import ctypes as C
        rc = gpu.lib.krep_gpu_format_matches(C.c_void_p(d_text), len(text), C.c_void_p(pos.data_ptr()), m, abi.SIZE_MAX, None,
                                             C.c_void_p(buf.data_ptr()), 256, C.byref(out), None)
        assert rc == 2 and "not ascending in start, or a record lies outside" in gpu.last_error()
        with pytest.raises(krep_amd.KrepGpuError, match="not ascending in start, or a record lies outside"):
            gpu.format_matches(d_text, len(text), pos.data_ptr(), m, abi.SIZE_MAX, abi.MatchFormat(b"f:"), buf.data_ptr(), 256)
        assert (buf.cpu().numpy() == PAD).all()  # the output buffer is untouched
    pos, m = records_to_device([(0, 2), (3, 5)])
    assert gpu.format_matches(d_text, len(text), pos.data_ptr(), m).out_bytes == 10  # the library works on after a refusal
    with pytest.raises(krep_amd.KrepGpuError, match="format string"):
        gpu.format_matches(d_text, len(text), pos.data_ptr(), m, abi.SIZE_MAX, abi.MatchFormat(b"x" * ((1 << 20) + 1)))
    with pytest.raises(krep_amd.KrepGpuError, match="more than one call takes"):
        gpu.format_matches(d_text, len(text), pos.data_ptr(), 1 << 40)
    q = gpu.format_matches(d_text, len(text), pos.data_ptr(), 0)
    assert (q.items, q.out_bytes, q.overflow) == (0, 0, 0)
    q = gpu.format_matches(d_text, len(text), pos.data_ptr(), m, 0)  # max_items = 0: nothing
    assert (q.items, q.out_bytes, q.overflow) == (0, 0, 0)


def test_a_plan_without_only_matching_is_refused(gpu):
    import krep_amd
    keep, d_text = to_device(b"ab\nab\n")
    plan = gpu.plan(abi.Params([b"ab"]))
    with pytest.raises(krep_amd.KrepGpuError, match="only_matching"):
        plan.grep_only_matching(d_text, 6)
    assert gpu.plan(abi.Params([b"ab"]), only_matching=True).grep_only_matching(d_text, 6, filename=b"f") == b"f:1:ab\nf:2:ab\n"


def test_the_live_cli_answered():
    """Where oracle/_ref/krep exists (it travels with the tree to the GPU machine) the table rows, the random cases and the 1 GiB
    case were compared with the live CLI, none with a stored digest."""
    STORE.save()
    if not os.path.exists(os.path.join(ROOT, "oracle", "_ref", "krep")):
        return
    assert CLI, "oracle/_ref/krep is here but cannot run on this host"
    assert LIVE["table"] == len(om.table_cases()) and LIVE["rand"] >= 240 and LIVE["gib"] == 1 and STORE.stored == 0, (LIVE, STORE.stored)
