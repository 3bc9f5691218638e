"""krep_gpu_format_lines_ex / Plan.grep_lines(color=True): the reference's default output under --color=always (every line that
holds a match, once, with the caller's strings around the line and around every match; print_matching_items() in full-line mode with
color_output_enabled, krep.c:797-1071) produced on the device, byte for byte — against tests/color_line_model.py and against the
stock CLI (oracle/_ref/krep -t 1 --color=always, with a file and with -s) wherever that binary exists."""
import hashlib
import os

import numpy as np
import pytest

import color_line_model as cm
import line_model as lm
import oracle_lib as ol
from krep_amd import abi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = ol.ref_cli()
STORE = cm.Store()
LIVE = {"table": 0, "rand": 0, "gib": 0}  # cases the live CLI answered
PAD = 0xEE
ODD = (b"#", bytes(range(65, 82)), b"", bytes(range(97, 130)))  # 1, 17, 0 and 33 bytes: lengths no reference produces


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


def check_raw_call(gpu, d_text, n, pos, m, fmt, max_count, model, out_shift=0):
    """krep_gpu_format_lines_ex on a record list against the model: size query, exact capacity, capacity one short"""
    import torch
    limit = abi.SIZE_MAX if max_count is None else max_count
    f = abi.LineFormat(*fmt) if fmt is not None else None
    want = model.data
    q = gpu.format_lines_ex(d_text, n, pos.data_ptr(), m, limit, f)
    assert (q.out_bytes, q.lines, q.lines_total, q.capped_lines, q.overflow) == \
        (len(want), len(model.spans), model.lines_total, model.capped, 0)
    buf = torch.full((len(want) + 64,), PAD, dtype=torch.uint8, device="cuda")
    r = gpu.format_lines_ex(d_text, n, pos.data_ptr(), m, limit, f, buf.data_ptr() + out_shift, len(want))
    got = buf.cpu().numpy()
    assert not r.overflow and r.out_bytes == len(want)
    assert got[out_shift:out_shift + len(want)].tobytes() == want
    assert (got[:out_shift] == PAD).all() and (got[out_shift + len(want):] == PAD).all()  # nothing outside [0, out_bytes)
    if len(want) > 1:
        r = gpu.format_lines_ex(d_text, n, pos.data_ptr(), m, limit, f, buf.data_ptr(), len(want) - 1)
        assert r.overflow == 1 and r.out_bytes == len(want) and r.lines == len(model.spans)
        assert (r.lines_total, r.capped_lines) == (model.lines_total, model.capped)


def check_plain_twins(gpu, d_text, n, pos, m, prefix, max_count):
    """only `prefix` set: the bytes of krep_gpu_format_lines; fmt = NULL: those with an empty prefix"""
    import torch
    limit = abi.SIZE_MAX if max_count is None else max_count
    for fmt, pre in ((abi.LineFormat(prefix), prefix), (None, b"")):
        size = int(gpu.format_lines(d_text, n, pos.data_ptr(), m, limit, pre).out_bytes)
        a = torch.full((size + 64,), PAD, dtype=torch.uint8, device="cuda")
        b = torch.full((size + 64,), PAD, dtype=torch.uint8, device="cuda")
        ra = gpu.format_lines(d_text, n, pos.data_ptr(), m, limit, pre, a.data_ptr(), size)
        rb = gpu.format_lines_ex(d_text, n, pos.data_ptr(), m, limit, fmt, b.data_ptr(), size)
        assert torch.equal(a, b) and not rb.overflow
        assert (ra.out_bytes, ra.lines, ra.lines_total, ra.capped_lines) == (rb.out_bytes, rb.lines, rb.lines_total, rb.capped_lines)


def check_records(gpu, d_text, text, recs, max_count, out_shift=0, prefix=lm.FILE + b":"):
    """the three sets of strings and the plain twins on one record list"""
    pos, m = records_to_device(recs)
    base = cm.ColorLines(text, recs, max_count=max_count)
    for k, fmt in enumerate((cm.strings(lm.FILE, True), cm.strings(None, True), ODD)):
        check_raw_call(gpu, d_text, len(text), pos, m, fmt, max_count, base.again(fmt), out_shift if k != 1 else 0)
    check_plain_twins(gpu, d_text, len(text), pos, m, prefix, max_count)


def check_case(gpu, chk, case, tmp_path, idx):
    recs = lm.cut_to_max_count(case.emitted(chk, abi), case.max_count)
    model = cm.ColorLines(case.text, recs, cm.strings(lm.FILE, True), case.max_count)
    live = live_s = None
    string_mode = case.string_mode_ok()
    model_s = cm.ColorLines(case.text, recs, cm.strings(None, True), case.max_count)
    if CLI:
        path = tmp_path / "t.txt"
        path.write_bytes(case.text)
        rc, out = cm.run_cli(CLI, case, path)
        assert out == model.data and rc == (0 if out else 1), (case.key, case.cli_args())
        live = cm.digest(rc, out)
        if string_mode:
            rc, out = cm.run_cli_string(CLI, case)
            assert out == model_s.data and rc == (0 if out else 1), (case.key, case.cli_args())
            live_s = cm.digest(rc, out)
        LIVE[case.key.split("/")[0]] += 1
    assert cm.digest(0 if model.data else 1, model.data) == STORE.want(case.key, live), case.key
    if string_mode:
        assert cm.digest(0 if model_s.data else 1, model_s.data) == STORE.want(case.key + "/string", live_s), case.key
    shift = (0, 3, 7, 13)[idx % 4]  # a text whose base is not 16-byte aligned
    keep, d_text = to_device(case.text, shift)
    n = len(case.text)
    check_records(gpu, d_text, case.text, recs, case.max_count, out_shift=(0, 5)[idx % 2])
    gpu.set_force_no_simd(case.no_simd)
    try:
        plan = gpu.plan(case.params(abi))
        assert plan.grep_lines(d_text, n, filename=lm.FILE, max_count=case.max_count, color=True) == model.data, (case.key, case.pats)
        assert plan.grep_lines(d_text, n, max_count=case.max_count, color=True) == model_s.data, (case.key, case.pats)
        plan.close()
    finally:
        gpu.set_force_no_simd(False)
    del keep


def test_table_rows(gpu, oracle_engine, tmp_path):
    for idx, case in enumerate(cm.table_cases()):
        check_case(gpu, oracle_engine, case, tmp_path, idx)
    sh = b"xx Sherlock yy"
    keep, d_text = to_device(sh)
    plan = gpu.plan(abi.Params([b"Sherlock", b"lock", b"er"]))
    assert plan.grep_lines(d_text, len(sh), filename="f", color=True) == (
        b"\033[1;38;5;81mf\033[0m\033[38;5;244m:\033[38;5;252mxx \033[1;38;5;222mSherlock\033[38;5;252m"
        b"\033[1;38;5;222mer\033[38;5;252m\033[1;38;5;222mlock\033[38;5;252m yy\033[0m\n")
    assert plan.grep_lines(d_text, len(sh), filename="f") == b"f:xx Sherlockerlock yy\n"  # the keyword defaults to off


def test_random_cases(gpu, oracle_engine, tmp_path):
    cases = cm.random_cases()
    assert len(cases) >= 240
    for idx, case in enumerate(cases):
        check_case(gpu, oracle_engine, case, tmp_path, idx)


def occurrences(text: bytes, pat: bytes):
    """greedy non-overlapping occurrences, as the reference's SIMD literals find them"""
    out, i = [], text.find(pat)
    while i >= 0:
        out.append((i, i + len(pat)))
        i = text.find(pat, i + len(pat))
    return out


def test_one_line_of_8_mib_with_131072_records(gpu):
    n = 8 << 20
    a = np.full(n, ord("x"), dtype=np.uint8)
    a[0::64] = ord("a")
    a[1::64] = ord("b")
    text = a.tobytes()
    recs = [(i, i + 2) for i in range(0, n, 64)]
    assert len(recs) == 131072
    keep, d_text = to_device(a)
    pos, m = records_to_device(recs)
    base = cm.ColorLines(text, recs)
    for fmt in (cm.strings(b"big.txt", True), ODD):
        model = base.again(fmt)
        # only the first 2048 records get strings
        assert model.capped == 1 and len(model.data) == len(fmt[0]) + n + lm.CAP * (len(fmt[1]) + len(fmt[2])) + len(fmt[3]) + 1
        check_raw_call(gpu, d_text, n, pos, m, fmt, None, model, out_shift=3)
    plan = gpu.plan(abi.Params([b"ab"]))
    assert plan.grep_lines(d_text, n, color=True) == base.render(cm.strings(None, True))
    check_plain_twins(gpu, d_text, n, pos, m, b"big.txt:", None)
    # ... and overlapping records on it: the 2048 that count repeat their bytes, each inside its own pair of strings
    recs = [(i, i + 100) for i in range(0, n - 100, 64)]
    pos, m = records_to_device(recs)
    base = cm.ColorLines(text, recs)
    for fmt in (cm.strings(None, True), ODD):
        model = base.again(fmt)
        assert len(model.data) == len(fmt[0]) + n + lm.CAP * (len(fmt[1]) + len(fmt[2])) + (lm.CAP - 1) * 36 + len(fmt[3]) + 1
        check_raw_call(gpu, d_text, n, pos, m, fmt, None, model)


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
        for mc in (None, 17):
            check_records(gpu, d_text, text, recs, mc, out_shift=shift % 4, prefix=b"a/long/path/name.txt:")
        plan = gpu.plan(abi.Params([b"ab"]))
        assert plan.grep_lines(d_text, len(text), filename="f", color=True) == cm.ColorLines(text, recs, cm.strings(b"f", True)).data
    # a text with a newline in every block position that matters: at 4095 / 4096 / 4097 and none for the next 3 blocks
    a = np.full(5 * 4096 + 100, ord("e"), dtype=np.uint8)
    a[[4095, 4096, 4097]] = 10
    for s in (0, 4094, 4098, 8191, 8192, 3 * 4096 + 5, a.size - 2):
        a[s:s + 2] = (ord("a"), ord("b"))
    text = a.tobytes()
    recs = occurrences(text, b"ab")
    keep, d_text = to_device(a, 1)
    check_records(gpu, d_text, text, recs, None)


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
    recs = [tuple(x) for x in pos[: 2 * m].view(-1, 2).cpu().numpy().astype(np.int64).tolist()]
    tb = buf[:n].cpu().numpy().tobytes()
    for fmt, mc in ((cm.strings(b"dict.txt", True), None), (ODD, 1000)):
        check_raw_call(gpu, buf.data_ptr(), n, pos, m, fmt, mc, cm.ColorLines(tb, recs, fmt, mc))
    check_plain_twins(gpu, buf.data_ptr(), n, pos, m, b"dict.txt:", None)
    check_plain_twins(gpu, buf.data_ptr(), n, pos, m, b"dict.txt:", 1000)
    assert gpu.plan(abi.Params(pats)).grep_lines(buf.data_ptr(), n, filename="dict.txt", color=True) == cm.ColorLines(
        tb, recs, cm.strings(b"dict.txt", True)).data


def test_1_gib_of_the_bench_text_against_the_cli(gpu, tmp_path):
    import torch
    import bench
    n = 1 << 30
    buf = torch.empty(n + 64, dtype=torch.uint8, device="cuda")
    gpu.generate(buf.data_ptr(), n, 0, 2, bench.SEED, bench.PATTERN, bench.PERIOD)
    path = tmp_path / "literal8.txt"
    got = gpu.plan(abi.Params([bench.PATTERN])).grep_lines(buf.data_ptr(), n, filename=str(path), color=True)
    assert len(got) > 100_000
    swap = lambda b: b.replace(cm.C_FILE + str(path).encode() + cm.RESET, cm.C_FILE + lm.FILE + cm.RESET)  # noqa: E731
    got = swap(got)
    live = None
    if CLI:
        import subprocess
        buf[:n].cpu().numpy().tofile(str(path))
        try:
            r = subprocess.run([CLI, "-t", "1", "--color=always", bench.PATTERN.decode(), str(path)], capture_output=True, timeout=600)
        finally:
            os.remove(path)
        out = swap(r.stdout)
        assert hashlib.sha256(got).hexdigest() == hashlib.sha256(out).hexdigest() and r.returncode == 0
        live = cm.digest(r.returncode, out)
        LIVE["gib"] += 1
    assert cm.digest(0, got) == STORE.want("gib/literal8", live)


def test_refused_record_lists(gpu):
    import krep_amd
    text = b"ab\nab\nab\n"
    keep, d_text = to_device(text)
    fmt = abi.LineFormat(*cm.strings(b"f", True))
    for recs in ([(3, 5), (0, 2)], [(0, 2), (9, 11)], [(0, 2), (1 << 40, (1 << 40) + 2)], [(4, 3)]):
        pos, m = records_to_device(recs)
        for f in (fmt, None):
            with pytest.raises(krep_amd.KrepGpuError, match="not ascending in start, or a record lies outside"):
                gpu.format_lines_ex(d_text, len(text), pos.data_ptr(), m, fmt=f)
    pos, m = records_to_device([(0, 2), (3, 5)])
    # the library works on after a refusal
    assert gpu.format_lines_ex(d_text, len(text), pos.data_ptr(), m, fmt=fmt).out_bytes == 6 + 2 * sum(len(s) for s in cm.strings(b"f", True))
    assert gpu.format_lines_ex(d_text, len(text), pos.data_ptr(), 0, fmt=fmt).out_bytes == 0  # n == 0 leaves everything 0


def test_a_string_of_more_than_2_to_the_20_bytes_is_refused(gpu):
    import krep_amd
    text = b"ab\nab\n"
    keep, d_text = to_device(text)
    pos, m = records_to_device([(0, 2)])
    big = b"x" * ((1 << 20) + 1)
    for k in range(4):
        parts = [b""] * 4
        parts[k] = big
        with pytest.raises(krep_amd.KrepGpuError, match="format string"):
            gpu.format_lines_ex(d_text, len(text), pos.data_ptr(), m, fmt=abi.LineFormat(*parts))
    ok = b"x" * ((1 << 20) - 1)  # the longest string the call takes
    assert gpu.format_lines_ex(d_text, len(text), pos.data_ptr(), m, fmt=abi.LineFormat(b"", b"", b"", ok)).out_bytes == 3 + len(ok)


def test_the_live_cli_answered():
    """Where oracle/_ref/krep exists (it travels with the tree to the GPU box) the table rows, the random cases and the 1 GiB case
    were compared with the live CLI, none with a stored digest."""
    STORE.save()
    if not os.path.exists(os.path.join(ROOT, "oracle", "_ref", "krep")):
        return
    assert CLI, "oracle/_ref/krep is here but cannot run on this host"
    assert LIVE["table"] == len(cm.table_cases()) and LIVE["rand"] >= 200 and LIVE["gib"] == 1 and STORE.stored == 0, (LIVE, STORE.stored)
