"""A loops search (krep -E with *, + and {n,}: kg_regex_loops.hip) in WINDOWS, behind krep_gpu_set_regex_loops_windows: the window scan
(start ownership, 4096 bytes of context on both sides, the -c facts krep_gpu_combine_line_counts folds, the two refusals), the host
executor in streamed pieces and over two shards, and the pieces drivers of the grep output.  The compiled reference (oracle/_ref,
through tests/regex_ref.py) answers every case.  The module turns both switches on and, whatever happens, off again.

max_count in a window: a plan with a finite max_count gives EACH window its own first max_count records (the cut of the whole list is
the caller's, as for every PIECES family); test_a_finite_max_count_cuts_every_window_on_its_own pins that."""
import ctypes as C

import numpy as np
import pytest

import regex_loops_output_cases as lc
import regex_ref
from krep_amd import abi
from krep_amd.engine import KrepGpuError
from test_gpu_regex_loops import AUTO, DENSE, SPARSE, background, cpu_selector, expected, put_line, rx

pytestmark = pytest.mark.gpu

CTX = 4096  # the context a window needs on each side (include/krep_gpu.h)
NAME = b"f.txt"


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
    e.set_regex_loops_windows(True)
    try:
        yield e
    finally:
        e.set_regex_loops_windows(False)
        e.set_regex_loops(False)
        e.force_regex_loops_road(AUTO)
        e.force_regex_grid(0)
        e.set_stream_chunk(0)
        e.set_cpu_fallback(None)
        e.set_thread_config(None)


# ---------------------------------------------------------------------------------------------------------------- the texts
# key: (patterns, case_sensitive, alphabet of the background lines, lines planted among them, the line of exactly 4096 bytes)
CASES = {
    "a+b": ([b"a+b"], True, b"aabc \n", [b"xaaaab", b"aabaab ab"], b"aab " * 1024),
    "ab*": ([b"ab*"], True, b"abbc \n", [b"xabbb", b"abab ab"], b"abb " * 1024),
    "error": ([b"ERROR.*timeout"], True, b"EROtimeu:  \n", [b"ERROR: a timeout", b"xERRORtimeout timeout"], b"ERROR" + b"-" * 4084 + b"timeout"),
    "hashes": ([b"^#+ "], True, b"## a\n", [b"## title", b"# a", b" ## no"], b"### " + b"a# " * 1364),
    "eol": ([b"[a-z]+;$"], True, b"ab;  \n", [b"ab;", b"a b;b ab;", b"ab; "], b"ab; " * 1000 + b"x" * 95 + b";"),
    "eol-i": ([b"[a-z]+;$"], False, b"aB;  \n", [b"Ab;", b"a B;b AB;", b"ab; "], b"aB; " * 1000 + b"X" * 95 + b";"),
    "inner": ([b"x(a+|b)y"], True, b"xaby \n", [b"xayxby", b"xaaaay xby", b"xab xbb"], b"xayxby " * 585 + b"x"),
    "decimal": ([b"[0-9]+\\.[0-9]+"], True, b"0123. x\n", [b"3.14", b"v10.25.7 1.5", b"12. 5"], b"3.14 10.5 " * 409 + b"1.5 7."),
}
AT_LONG = 6000
_texts = {}


def build(key):
    """-> (text, cuts): ~16 KiB of short lines, the planted lines, the 4096-byte line from AT_LONG on, a last line without a newline
    that ends in a match where the pattern has one there.  The cuts follow from the reference's records (built once, left unchanged):
    on a match's first byte, inside it, on the byte behind its end (between two touching matches of `inner`), on a newline and on the
    byte behind it, two cuts inside the long line (three windows own it in turn), a 1-byte window, windows without a newline."""
    if key in _texts:
        return _texts[key]
    pats, cs, alphabet, lines, long_line = CASES[key]
    assert len(long_line) == 4096 and b"\n" not in long_line
    rng = np.random.RandomState(sum(key.encode()))
    t = background(rng, 16000, alphabet)
    put_line(t, AT_LONG, long_line)
    for k, line in enumerate(lines * 3):
        put_line(t, 300 + 700 * k, line)
        put_line(t, 11000 + 500 * k, line)
    head, tail = np.frombuffer(lines[0] + b"\n", dtype=np.uint8), np.frombuffer(b"\n" + lines[0], dtype=np.uint8)
    t[:head.size] = head  # (the first line holds a match: a candidate line on both roads)
    t[t.size - tail.size:] = tail
    t.setflags(write=False)
    rec = expected(pats, t, case_sensitive=cs)[1].astype(np.int64)
    assert rec.shape[0] >= 12, key
    cuts = {AT_LONG + 1000, AT_LONG + 3000, AT_LONG + 3001}  # (the second and third: a 1-byte window inside the long line)
    inside = [(s, e) for s, e in rec.tolist() if s >= AT_LONG + 4100 or e < AT_LONG - 4]
    for s, e in inside[:3] + inside[-2:]:
        cuts |= {s, (s + e + 1) // 2, e}
    nl = np.flatnonzero(t == 10)
    for p in (nl[3], nl[len(nl) // 2], nl[-1]):
        cuts |= {int(p), int(p) + 1}
    _texts[key] = (t, sorted(c for c in cuts if 0 < c < t.size))
    return _texts[key]


def windows_of(cuts, n):
    edges = [0] + list(cuts) + [n]
    return list(zip(edges[:-1], edges[1:]))


def scan_window(plan, text, lo, hi, base=0, global_len=None, ctx=CTX, cap=1 << 14, buf=None):
    """the window [lo, hi) of `text` staged as a buffer of its own with ctx bytes on each side (fewer where the text ends) ->
    (ScanOut, records [(start, end)] with `base` taken off); buf = (b0, b1) stages other bytes"""
    import torch
    n = int(text.size)
    b0, b1 = buf if buf is not None else (max(lo - ctx, 0), min(hi + ctx, n))
    d = torch.from_numpy(text[b0:b1].copy()).cuda()
    pos = torch.full((2 * cap,), -1, dtype=torch.int64, device="cuda")
    out = plan.scan(d.data_ptr(), b1 - b0, lo - b0, hi - b0, base + b0, pos.data_ptr(), cap, global_len=(base + n) if global_len is None else global_len)
    got = pos.cpu().numpy()
    assert not out.overflow and (got[2 * int(out.stored):] == -1).all()
    return out, [(int(s) - base, int(e) - base) for s, e in got[:2 * int(out.stored)].reshape(-1, 2)]


def fold(gpu, outs):
    return int(gpu.lib.krep_gpu_combine_line_counts((abi.ScanOut * len(outs))(*outs), len(outs)))


# ---------------------------------------------------------------------------------------------------------------- the window scan
@pytest.mark.parametrize("key", list(CASES))
@pytest.mark.parametrize("road", [SPARSE, DENSE], ids=["sparse", "dense"])
def test_windows_concatenate_to_the_whole_text_and_fold_to_its_line_count(gpu, road, key):
    pats, cs, *_ = CASES[key]
    text, cuts = build(key)
    n = int(text.size)
    want = expected(pats, text, case_sensitive=cs)
    want_c = expected(pats, text, case_sensitive=cs, count_lines=True)[0]
    wins = windows_of(cuts, n)
    assert any(hi - lo == 1 for lo, hi in wins) and any(not (text[lo:hi] == 10).any() for lo, hi in wins)
    gpu.force_regex_loops_road(road)
    plan, plan_c = gpu.plan(rx(pats, case_sensitive=cs)), gpu.plan(rx(pats, case_sensitive=cs, count_lines=True))
    try:
        whole = scan_window(plan, text, 0, n)[1]  # (the whole text through the same plan: one window that begins and ends it)
        assert whole == [tuple(r) for r in want[1].tolist()], key
        got, outs = [], []
        for lo, hi in wins:
            out, rec = scan_window(plan, text, lo, hi)
            assert all(lo <= s < hi for s, _ in rec), (key, lo, hi, rec[:3])
            assert out.count == out.total_matches == len(rec)
            got += rec
            oc, none = scan_window(plan_c, text, lo, hi)
            assert none == [] and oc.count == oc.line_count
            assert bool(oc.has_newline) == bool((text[lo:hi] == 10).any()), (key, lo, hi)
            outs.append(oc)
        assert got == whole, (key, len(got), len(whole))
        assert fold(gpu, outs) == want_c, (key, [(o.line_count, o.head_line_hit, o.tail_line_hit, o.has_newline) for o in outs], want_c)
        # three windows own the long line in turn: each holds some of its matches (a single 4096-byte match: the first alone)
        in_long = [sum(1 for s, _ in whole if max(lo, AT_LONG) <= s < min(hi, AT_LONG + 4096)) for lo, hi in
                   ((0, AT_LONG + 1000), (AT_LONG + 1000, AT_LONG + 3000), (AT_LONG + 3001, n))]
        assert sum(in_long) >= 1 and (key in ("error", "hashes", "eol", "eol-i") or min(in_long) >= 1), (key, in_long)
    finally:
        gpu.force_regex_loops_road(AUTO)
        plan.close()
        plan_c.close()


def test_the_end_of_the_text_ends_a_line_in_the_buffer_that_ends_it_only(gpu):
    """[a-z]+;$ on a last line without a newline: found in a case-sensitive search (by the window whose buffer ends the text), not under -i"""
    for key, found in (("eol", True), ("eol-i", False)):
        pats, cs, *_ = CASES[key]
        text, _ = build(key)
        n = int(text.size)
        ends = expected(pats, text, case_sensitive=cs)[1][:, 1].tolist()
        assert (n in ends) == found
        plan = gpu.plan(rx(pats, case_sensitive=cs))
        try:
            _, rec = scan_window(plan, text, n - 5, n)  # (the last line is the planted one, three bytes)
            assert (n in [e for _, e in rec]) == found and (not found or rec[-1] == (n - 3, n))
            # the same bytes as a buffer that does NOT end the text: the last line is cut, and it meets the owned range
            with pytest.raises(KrepGpuError, match="does not hold the whole of a line that meets its owned range"):
                scan_window(plan, text, n - 2, n, global_len=n + 100)
        finally:
            plan.close()


def test_a_finite_max_count_cuts_every_window_on_its_own(gpu):
    pats, cs, *_ = CASES["a+b"]
    text, cuts = build("a+b")
    n = int(text.size)
    whole = [tuple(r) for r in expected(pats, text)[1].tolist()]
    plan = gpu.plan(rx(pats, max_count=2))
    try:
        seen_cut = 0
        for lo, hi in windows_of(cuts, n):
            own = [r for r in whole if lo <= r[0] < hi]
            out, rec = scan_window(plan, text, lo, hi)
            assert rec == own[:2] and (out.count, out.stored, out.total_matches) == (min(len(own), 2), min(len(own), 2), len(own)), (lo, hi)
            seen_cut += len(own) > 2
        assert seen_cut >= 3
    finally:
        plan.close()


@pytest.mark.parametrize("base", [(1 << 32) - 8192, 5 * (1 << 32) + 12288])
def test_a_text_at_a_high_global_offset(gpu, base):
    """the text as a slice of a longer one that ends with it: its first line is cut (the buffer does not begin the text), so the windows
    own what stands behind the first newline; the records carry the base"""
    pats, cs, *_ = CASES["a+b"]
    text, cuts = build("a+b")
    n = int(text.size)
    first = int(np.flatnonzero(text == 10)[0]) + 1
    whole = [tuple(r) for r in expected(pats, text)[1].tolist() if r[0] >= first]
    want_c = expected(pats, text[first:], count_lines=True)[0]
    for road in (SPARSE, DENSE):
        gpu.force_regex_loops_road(road)
        plan, plan_c = gpu.plan(rx(pats)), gpu.plan(rx(pats, count_lines=True))
        try:
            got, outs = [], []
            for lo, hi in windows_of([c for c in cuts if c > first], n):
                lo = max(lo, first)
                got += scan_window(plan, text, lo, hi, base=base)[1]
                outs.append(scan_window(plan_c, text, lo, hi, base=base)[0])
            assert got == whole and fold(gpu, outs) == want_c, (base, road)
            with pytest.raises(KrepGpuError, match="does not hold the whole of a line that meets its owned range"):
                scan_window(plan, text, 0, first + 10, base=base)
        finally:
            gpu.force_regex_loops_road(AUTO)
            plan.close()
            plan_c.close()


def test_the_two_refusals_and_the_call_after_each(gpu):
    import torch
    pats = [b"a+b"]
    rng = np.random.RandomState(21)
    text = background(rng, 30000, b"aac \n")
    put_line(text, 3000, b"a" * 299 + b"b")                    # a 300-byte line
    put_line(text, 9000, b"a" * 4096 + b"b")                   # a candidate line of 4097 bytes
    put_line(text, 20000, b"c" * 2990 + b"aaaaaaaaab")         # a 3000-byte candidate line
    for s in (500, 1000, 7990, 24490, 24600, 29000):            # (the background holds no b: these are the other matches)
        put_line(text, s, b"xaab ab")
    n = int(text.size)
    whole = [tuple(r) for r in expected(pats, text)[1].tolist()]  # (the reference walks a line of any length)
    nl = np.flatnonzero(text == 10)
    lines_of = lambda rec: len({int(np.searchsorted(nl, s)) for s, _ in rec})
    for road in (SPARSE, DENSE):
        gpu.force_regex_loops_road(road)
        plan, plan_c = gpu.plan(rx(pats)), gpu.plan(rx(pats, count_lines=True))
        try:
            for pl in (plan, plan_c):
                # 100 bytes of context: the buffer begins, and ends, inside the 300-byte line the window meets
                for buf in ((3050, 3400), (2900, 3250), (3050, 3250)):
                    with pytest.raises(KrepGpuError, match="does not hold the whole of a line that meets its owned range.*stage 4096 bytes"):
                        scan_window(pl, text, 3150, 3200, buf=buf)
                out, rec = scan_window(pl, text, 3150, 3200)
                assert out.total_matches == 0  # (the line's one match starts at 3000)
                out, rec = scan_window(pl, text, 2990, 3200)
                assert (rec == [(3000, 3300)]) if pl is plan else (out.line_count, out.tail_line_hit, out.head_line_hit) == (1, 1, 0)
                # the 4097-byte line across a cut: each window meets it, and its buffer shows all of it
                for lo, hi in ((6000, 11000), (11000, 15000)):
                    with pytest.raises(KrepGpuError, match="a line of more than 4096 bytes: kept on krep's regex_search"):
                        scan_window(pl, text, lo, hi)
                pos = torch.full((64,), -1, dtype=torch.int64, device="cuda")
                d = torch.from_numpy(text[2000:19000].copy()).cuda()
                with pytest.raises(KrepGpuError, match="a line of more than 4096 bytes"):
                    pl.scan(d.data_ptr(), 17000, 4000, 13000, 2000, pos.data_ptr(), 32, global_len=n)
                assert (pos == -1).all().item()  # nothing written
                # a window that keeps clear of it, the long line cut by the end of its buffer: accepted
                own = [r for r in whole if r[0] < 8000]
                out, rec = scan_window(pl, text, 0, 8000)
                assert (rec == own) if pl is plan else (out.line_count == lines_of(own)), road
                assert len(own) >= 4
                # the 3000-byte line in the context, cut by the start of the buffer, not met by the owned range: accepted
                assert 24500 - CTX > 20000 and 24500 > 23001
                own = [r for r in whole if r[0] >= 24500]
                out, rec = scan_window(pl, text, 24500, n)
                assert (rec == own) if pl is plan else (out.line_count == lines_of(own)), road
                assert len(own) >= 4
        finally:
            gpu.force_regex_loops_road(AUTO)
            plan.close()
            plan_c.close()


def test_a_starved_grid_in_windows(gpu):
    pats, cs, *_ = CASES["inner"]
    text, cuts = build("inner")
    n = int(text.size)
    whole = [tuple(r) for r in expected(pats, text)[1].tolist()]
    want_c = expected(pats, text, count_lines=True)[0]
    plan, plan_c = gpu.plan(rx(pats)), gpu.plan(rx(pats, count_lines=True))
    try:
        gpu.force_regex_grid(1)
        for road in (SPARSE, DENSE):
            gpu.force_regex_loops_road(road)
            wins = windows_of(cuts[::3], n)
            assert sum((scan_window(plan, text, lo, hi)[1] for lo, hi in wins), []) == whole
            assert fold(gpu, [scan_window(plan_c, text, lo, hi)[0] for lo, hi in wins]) == want_c
    finally:
        gpu.force_regex_grid(0)
        gpu.force_regex_loops_road(AUTO)
        plan.close()
        plan_c.close()


# ---------------------------------------------------------------------------------------------------------------- the host path
def host_text(key):
    """~40 KiB: the case's text two and a half times (every copy's last line runs into the next copy's first)"""
    text, _ = build(key)
    return np.concatenate([text, text, text[:8500]]).copy()


@pytest.mark.parametrize("key", ["a+b", "error", "hashes", "eol-i", "decimal"])
def test_the_executor_streams_pieces_and_shards_them(gpu, key):
    pats, cs, *_ = CASES[key]
    text = host_text(key)
    jobs = (dict(), dict(count_lines=True), dict(max_count=7), dict(max_count=5, count_lines=True), dict(track_positions=False))
    assert text.size > 9 * 4096
    try:
        for kw in jobs:
            kw = dict(case_sensitive=cs, **kw)
            want = expected(pats, text, **kw)
            found = 1 if kw.get("track_positions") is False else 0
            assert gpu.split_mode(rx(pats, **kw), text.size) == abi.SPLIT_PIECES
            gpu.set_stream_chunk(4096)  # about ten pieces, each staged with 4097 bytes on both sides
            for call in ("search", "buffer"):
                if call == "search":
                    cnt, pos = gpu.search(rx(pats, **kw), text)
                else:  # (search_buffer answers like grep: 0 found, 1 not; without positions its result block stays empty)
                    rc, cnt, pos = gpu.search_buffer(rx(pats, **kw), text)
                    assert rc == found, (key, kw, rc)
                assert gpu.last_status() == abi.STATUS_OK, gpu.last_error()
                assert cnt == want[0] and np.array_equal(pos, want[1]), (key, kw, call, cnt, want[0])
            gpu.set_stream_chunk(0)
            rc, cnt, pos = gpu.search_buffer(rx(pats, **kw), text, num_gpus=2)  # (two logical shards may share a device)
            assert rc == found and gpu.last_status() == abi.STATUS_OK and gpu.last_shard_info().shards == 2, (key, kw, rc)
            assert cnt == want[0] and np.array_equal(pos, want[1]), (key, kw, "two shards", cnt, want[0])
        assert expected(pats, text, case_sensitive=cs)[0] > 30
    finally:
        gpu.set_stream_chunk(0)


def test_the_switch_off_stages_one_piece(gpu):
    """the behaviour the multi-piece cases rest on: without the switch the same call is one window over the whole text"""
    pats, cs, *_ = CASES["a+b"]
    text = host_text("a+b")
    want = expected(pats, text)
    gpu.set_regex_loops_windows(False)
    try:
        assert gpu.split_mode(rx(pats), text.size) == abi.SPLIT_WHOLE
        rc, cnt, pos = gpu.search_buffer(rx(pats), text, num_gpus=2)
        assert rc == 0 and cnt == want[0] and np.array_equal(pos, want[1]) and gpu.last_shard_info().shards == 1
    finally:
        gpu.set_regex_loops_windows(True)
    rc, cnt, pos = gpu.search_buffer(rx(pats), text, num_gpus=2)
    assert rc == 0 and cnt == want[0] and np.array_equal(pos, want[1]) and gpu.last_shard_info().shards == 2


def test_a_candidate_line_of_5000_bytes_goes_to_the_cpu_function(gpu):
    pats = [b"a+b"]
    text = host_text("a+b")
    put_line(text, 21000, b"a" * 4999 + b"b")
    gpu.set_stream_chunk(4096)
    try:
        with pytest.raises(KrepGpuError, match="more than 4096 bytes"):
            gpu.search(rx(pats), text)
        assert gpu.last_status() == abi.STATUS_FAILED
        cb = cpu_selector()
        gpu.set_cpu_fallback(C.cast(cb, C.c_void_p).value)
        for kw in (dict(), dict(count_lines=True)):
            p = rx(pats, **kw)
            comp = regex_ref.Compiled(pats[0])
            p.s.compiled_regex = comp.ptr
            got = gpu.search(p, text)
            w = expected(pats, text, **kw)
            assert gpu.last_status() == abi.STATUS_FELL_BACK and got[0] == w[0] and np.array_equal(got[1], w[1])
            assert w[0] > 30
    finally:
        gpu.set_cpu_fallback(None)
        gpu.set_stream_chunk(0)


# ---------------------------------------------------------------------------------------------------------------- the pieces drivers
def to_device(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()
    return t, t.data_ptr()


@pytest.mark.parametrize("key", [r.key for r in lc.ROWS])
def test_the_pieces_drivers_print_what_the_resident_text_prints(gpu, key):
    row = lc.BY_KEY[key]
    plan, plan_o = gpu.plan(lc.params(row)), gpu.plan(lc.params(row), only_matching=True)
    try:
        for nl in (True, False):
            text = lc.case(key, nl)[0]
            hold, d_text = to_device(text)
            for piece in (4099,) + ((8191,) if nl else ()):
                for filename in (NAME, None):
                    for color in (False, True):
                        want = plan.grep_lines(d_text, text.size, filename=filename, color=color)
                        got = plan.grep_lines_pieces(text, piece, filename=filename, color=color)
                        assert got == want, (key, nl, piece, filename, color, len(got), len(want))
                        want = plan_o.grep_only_matching(d_text, text.size, filename=filename, color=color)
                        got = plan_o.grep_only_matching_pieces(text, piece, filename=filename, color=color)
                        assert got == want, (key, nl, piece, filename, color, "-o", len(got), len(want))
                    assert len(want) > 100
            del hold
    finally:
        plan.close()
        plan_o.close()


def test_the_pieces_drivers_pass_the_scans_refusal_on(gpu):
    row = lc.BY_KEY["a+b"]
    rng = np.random.RandomState(11)
    bad = background(rng, 30000, b"aac \n")
    put_line(bad, 9000, b"a" * 4096 + b"b")
    put_line(bad, 200, b"xaab")
    plan, plan_o = gpu.plan(lc.params(row)), gpu.plan(lc.params(row), only_matching=True)
    try:
        for color in (False, True):
            with pytest.raises(KrepGpuError, match="more than 4096 bytes"):
                plan.grep_lines_pieces(bad, 4099, filename=NAME, color=color)
            with pytest.raises(KrepGpuError, match="more than 4096 bytes"):
                plan_o.grep_only_matching_pieces(bad, 4099, filename=NAME, color=color)
        text = lc.case("a+b", False)[0]
        hold, d_text = to_device(text)
        assert plan.grep_lines_pieces(text, 4099, filename=NAME) == plan.grep_lines(d_text, text.size, filename=NAME)
        assert plan_o.grep_only_matching_pieces(text, 4099) == plan_o.grep_only_matching(d_text, text.size)
        del hold
    finally:
        plan.close()
        plan_o.close()
