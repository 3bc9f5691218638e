"""krep_gpu_matching_lines / krep_gpu_format_lines / Plan.grep_lines: the reference's default output (every line that holds a
match, once; print_matching_items() in full-line mode, krep.c:797-1071) produced on the device, byte for byte — against
tests/line_model.py and against the stock CLI (oracle/_ref/krep -t 1 --color=never) wherever that binary exists."""
import hashlib
import os

import numpy as np
import pytest

import line_model as lm
import oracle_lib as ol
from krep_amd import abi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = ol.ref_cli()
STORE = lm.Store()
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


def check_raw_calls(gpu, d_text, n, recs, prefix, max_count, model, out_shift=0):
    """both raw calls on a record list against the model: size query, exact capacity, capacity one short"""
    import torch
    pos, m = records_to_device(recs)
    limit = abi.SIZE_MAX if max_count is None else max_count
    q = gpu.format_lines(d_text, n, pos.data_ptr(), m, limit, prefix)
    assert (q.out_bytes, q.lines, q.lines_total, q.capped_lines, q.overflow) == \
        (len(model.data), len(model.spans), model.lines_total, model.capped, 0)
    buf = torch.full((len(model.data) + 64,), PAD, dtype=torch.uint8, device="cuda")
    r = gpu.format_lines(d_text, n, pos.data_ptr(), m, limit, prefix, buf.data_ptr() + out_shift, len(model.data))
    got = buf.cpu().numpy()
    assert not r.overflow and r.out_bytes == len(model.data)
    assert got[out_shift:out_shift + len(model.data)].tobytes() == model.data
    assert (got[:out_shift] == PAD).all() and (got[out_shift + len(model.data):] == PAD).all()  # nothing outside [0, out_bytes)
    if len(model.data) > 1:
        r = gpu.format_lines(d_text, n, pos.data_ptr(), m, limit, prefix, buf.data_ptr(), len(model.data) - 1)
        assert r.overflow == 1 and r.out_bytes == len(model.data) and r.lines == len(model.spans)
    q = gpu.matching_lines(d_text, n, pos.data_ptr(), m, limit)
    L = len(model.spans)
    assert (q.lines, q.lines_total, q.capped_lines, q.overflow) == (L, model.lines_total, model.capped, 0)
    if m:
        spans = torch.full((2 * L + 2,), -1, dtype=torch.int64, device="cuda")
        first = torch.full((L + 2,), -1, dtype=torch.int64, device="cuda")
        r = gpu.matching_lines(d_text, n, pos.data_ptr(), m, limit, spans.data_ptr(), first.data_ptr(), max(L, 1))
        assert not r.overflow and r.lines == L
        if L:
            assert spans[:2 * L].view(-1, 2).cpu().tolist() == [list(s) for s in model.spans]
            assert first[:L + 1].cpu().tolist() == model.first_record
        assert spans[2 * L:].cpu().tolist() == [-1, -1] and first[L + 1:].cpu().tolist() == [-1]
        if L > 1:
            r = gpu.matching_lines(d_text, n, pos.data_ptr(), m, limit, spans.data_ptr(), first.data_ptr(), L - 1)
            assert r.overflow == 1 and r.lines == L and r.lines_total == model.lines_total


def check_case(gpu, chk, case, tmp_path, idx):
    recs = lm.cut_to_max_count(case.emitted(chk, abi), case.max_count)
    prefix = lm.FILE + b":"
    model = lm.Lines(case.text, recs, prefix, case.max_count)
    live = None
    if CLI:
        path = tmp_path / "t.txt"
        path.write_bytes(case.text)
        rc, out = lm.run_cli(CLI, case, path)
        assert out == model.data and rc == (0 if out else 1), (case.key, case.cli_args())
        live = lm.digest(rc, out)
        LIVE[case.key.split("/")[0]] += 1
    assert lm.digest(0 if model.data else 1, model.data) == STORE.want(case.key, live), case.key
    if case.want is not None:
        assert model.data == prefix + case.want
    shift = (0, 3, 7, 13)[idx % 4]  # a text whose base is not 16-byte aligned
    keep, d_text = to_device(case.text, shift)
    n = len(case.text)
    check_raw_calls(gpu, d_text, n, recs, prefix, case.max_count, model, out_shift=(0, 5)[idx % 2])
    check_raw_calls(gpu, d_text, n, recs, b"", case.max_count, lm.Lines(case.text, recs, b"", case.max_count))
    gpu.set_force_no_simd(case.no_simd)
    try:
        plan = gpu.plan(case.params(abi))
        assert plan.grep_lines(d_text, n, filename=lm.FILE, max_count=case.max_count) == model.data, (case.key, case.pats)
        plan.close()
    finally:
        gpu.set_force_no_simd(False)
    del keep


def test_table_rows(gpu, oracle_engine, tmp_path):
    for idx, case in enumerate(lm.table_cases()):
        check_case(gpu, oracle_engine, case, tmp_path, idx)


def test_random_cases(gpu, oracle_engine, tmp_path):
    cases = lm.random_cases()
    assert len(cases) >= 200
    for idx, case in enumerate(cases):
        check_case(gpu, oracle_engine, case, tmp_path, idx)


def occurrences(text: bytes, pat: bytes):
    """greedy non-overlapping occurrences, as the reference's SIMD literals find them"""
    out, i = [], text.find(pat)
    while i >= 0:
        out.append((i, i + len(pat)))
        i = text.find(pat, i + len(pat))
    return out


def test_one_line_of_8_mib_with_100000_records(gpu):
    n = 8 << 20
    a = np.full(n, ord("x"), dtype=np.uint8)
    a[0::64] = ord("a")
    a[1::64] = ord("b")
    text = a.tobytes()
    recs = [(i, i + 2) for i in range(0, n, 64)]
    assert len(recs) >= 100_000
    keep, d_text = to_device(a)
    for prefix in (b"big.txt:", b""):
        model = lm.Lines(text, recs, prefix)
        assert model.capped == 1 and len(model.data) == len(prefix) + n + 1
        check_raw_calls(gpu, d_text, n, recs, prefix, None, model)
    plan = gpu.plan(abi.Params([b"ab"]))
    assert plan.grep_lines(d_text, n) == text + b"\n"
    # ... and overlapping records on it: the 2048 that count repeat their bytes
    recs = [(i, i + 100) for i in range(0, n - 100, 64)]
    check_raw_calls(gpu, d_text, n, recs, b"", None, lm.Lines(text, recs, b""))


def test_long_lines_and_text_edges(gpu):
    rng = np.random.RandomState(5)
    lines = []
    for k in range(120):  # lines of 5000 bytes, a 1 MiB line between short ones
        body = bytearray(b"c" * (5000 if k % 2 == 0 else int(rng.randint(0, 40))))
        if k == 61:
            body = bytearray(b"d" * (1 << 20))
        for _ in range(int(rng.randint(0, 4))):
            if len(body) >= 2:
                s = int(rng.randint(0, len(body) - 1))
                body[s:s + 2] = b"ab"
        lines.append(bytes(body))
    text = b"ab" + b"\n".join(lines) + b"ab"  # records in the first and in the last 16 bytes
    recs = occurrences(text, b"ab")
    assert recs[0] == (0, 2) and recs[-1][1] == len(text) and len(recs) > 100
    for shift in (0, 9):
        keep, d_text = to_device(text, shift)
        for prefix, mc in ((b"f:", None), (b"", None), (b"a/long/path/name.txt:", 17)):
            check_raw_calls(gpu, d_text, len(text), recs, prefix, mc, lm.Lines(text, recs, prefix, mc), out_shift=shift % 4)
        plan = gpu.plan(abi.Params([b"ab"]))
        assert plan.grep_lines(d_text, len(text), filename="f") == lm.Lines(text, recs, b"f:").data
    # a text with a newline in every block position that matters: at 4095 / 4096 / 4097 and none for the next 3 blocks
    a = np.full(5 * 4096 + 100, ord("e"), dtype=np.uint8)
    a[[4095, 4096, 4097]] = 10
    for s in (0, 4094, 4098, 8191, 8192, 3 * 4096 + 5, a.size - 2):
        a[s:s + 2] = (ord("a"), ord("b"))
    text = a.tobytes()
    recs = occurrences(text, b"ab")
    keep, d_text = to_device(a, 1)
    check_raw_calls(gpu, d_text, len(text), recs, b"", None, lm.Lines(text, recs, b""))


def test_48_mib_dictionary_text(gpu):
    import torch
    import bench
    pats = bench.ac_patterns()
    n = (48 << 20) + 123
    buf = torch.empty(n + 64, dtype=torch.uint8, device="cuda")
    gpu.generate(buf.data_ptr(), n, 0, 4, bench.SEED, bench.pack_dict(pats), 4096)
    cap = n // 500
    pos = torch.empty(2 * cap, dtype=torch.int64, device="cuda")
    out = gpu.plan(abi.Params(pats)).scan(buf.data_ptr(), n, 0, n, 0, pos.data_ptr(), cap)
    assert not out.overflow and out.stored > 10000
    m = int(out.stored)
    gpu.order_by_start(pos.data_ptr(), m, n)
    recs = pos[: 2 * m].view(-1, 2).cpu().numpy().astype(np.int64)
    text = buf[:n].cpu().numpy()
    nl = np.flatnonzero(text == 10)
    k = np.searchsorted(nl, recs[:, 0], side="left")                 # the first newline at or after the start
    line_end = np.where(k < nl.size, nl[np.minimum(k, nl.size - 1)], n)
    line_start = np.where(k > 0, nl[np.maximum(k, 1) - 1] + 1, 0)
    head = np.flatnonzero(np.r_[True, line_start[1:] != line_start[:-1]])
    L = head.size
    q = gpu.matching_lines(buf.data_ptr(), n, pos.data_ptr(), m)
    assert q.lines == q.lines_total == L and not q.overflow
    spans = torch.empty(2 * L, dtype=torch.int64, device="cuda")
    first = torch.empty(L + 1, dtype=torch.int64, device="cuda")
    r = gpu.matching_lines(buf.data_ptr(), n, pos.data_ptr(), m, abi.SIZE_MAX, spans.data_ptr(), first.data_ptr(), L)
    assert not r.overflow and r.lines == L
    assert np.array_equal(spans.view(-1, 2).cpu().numpy(), np.stack([line_start[head], line_end[head]], axis=1))
    assert np.array_equal(first.cpu().numpy(), np.r_[head, m])
    tb = text.tobytes()
    for prefix, mc in ((b"dict.txt:", None), (b"", 1000)):
        model = lm.Lines(tb, [tuple(x) for x in recs.tolist()], prefix, mc)
        check_raw_calls(gpu, buf.data_ptr(), n, recs, prefix, mc, model)
    assert gpu.plan(abi.Params(pats)).grep_lines(buf.data_ptr(), n, filename="dict.txt") == lm.Lines(
        tb, [tuple(x) for x in recs.tolist()], b"dict.txt:").data


def test_1_gib_of_the_bench_text_against_the_cli(gpu, tmp_path):
    import torch
    import bench
    n = 1 << 30
    buf = torch.empty(n + 64, dtype=torch.uint8, device="cuda")
    gpu.generate(buf.data_ptr(), n, 0, 2, bench.SEED, bench.PATTERN, bench.PERIOD)
    path = tmp_path / "literal8.txt"
    got = gpu.plan(abi.Params([bench.PATTERN])).grep_lines(buf.data_ptr(), n, filename=str(path))
    assert len(got) > 100_000
    got = got.replace(str(path).encode() + b":", lm.FILE + b":")
    live = None
    if CLI:
        import subprocess
        buf[:n].cpu().numpy().tofile(str(path))
        r = subprocess.run([CLI, "-t", "1", "--color=never", bench.PATTERN.decode(), str(path)], capture_output=True, timeout=600)
        os.remove(path)
        out = r.stdout.replace(str(path).encode() + b":", lm.FILE + b":")
        assert hashlib.sha256(got).hexdigest() == hashlib.sha256(out).hexdigest() and r.returncode == 0
        live = lm.digest(r.returncode, out)
        LIVE["gib"] += 1
    assert lm.digest(0, got) == STORE.want("gib/literal8", live)


def test_refused_record_lists(gpu):
    import krep_amd
    text = b"ab\nab\nab\n"
    keep, d_text = to_device(text)
    for recs in ([(3, 5), (0, 2)], [(0, 2), (9, 11)], [(0, 2), (1 << 40, (1 << 40) + 2)], [(4, 3)]):
        pos, m = records_to_device(recs)
        for call in (lambda: gpu.format_lines(d_text, len(text), pos.data_ptr(), m),
                     lambda: gpu.matching_lines(d_text, len(text), pos.data_ptr(), m)):
            with pytest.raises(krep_amd.KrepGpuError, match="not ascending in start, or a record lies outside"):
                call()
    pos, m = records_to_device([(0, 2), (3, 5)])
    assert gpu.format_lines(d_text, len(text), pos.data_ptr(), m).out_bytes == 6  # the library works on after a refusal


def test_the_live_cli_answered():
    """Where oracle/_ref/krep exists (it travels with the tree to the GPU box) the table rows, the random cases and the 1 GiB case
    were compared with the live CLI, none with a stored digest."""
    STORE.save()
    if not os.path.exists(os.path.join(ROOT, "oracle", "_ref", "krep")):
        return
    assert CLI, "oracle/_ref/krep is here but cannot run on this host"
    assert LIVE["table"] == len(lm.table_cases()) and LIVE["rand"] >= 200 and LIVE["gib"] == 1 and STORE.stored == 0, (LIVE, STORE.stored)
