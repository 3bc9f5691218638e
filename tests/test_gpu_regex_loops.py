"""krep -E on the device for what krep_gpu_regex_compile_loops() takes (*, + and {n,} behind an atom; kg_regex_loops.hip: the filter
scan that names the candidate lines, on both roads, and the line walk kernel) against the reference's regex_search: the compiled
reference (oracle/_ref, through tests/regex_ref.py) answers every case with the expression the CLI compiles.  The module turns the
switch krep_gpu_set_regex_loops on and, whatever happens, off again: every other test meets the library as it expects it."""
import ctypes as C

import numpy as np
import pytest

import regex_alt_model
import regex_ref
from krep_amd import abi
from krep_amd.engine import KrepGpuError

pytestmark = pytest.mark.gpu

PAD = 0xEE
LANE, CELL, ROUND, UNIT = 16, 1024, 8192, 32768
AUTO, SPARSE, DENSE = 0, 1, 2


@pytest.fixture(autouse=True, scope="module")
def _c_locale():
    """the reference runs in the C locale (it never calls setlocale()); Python's start-up put the process into the environment's"""
    with regex_ref.c_locale():
        yield


@pytest.fixture(scope="module")
def gpu():
    import krep_amd
    e = krep_amd.load()
    assert e.device_count() >= 1 and e.available(), e.unavailable_reason()
    e.set_regex_loops(True)
    try:
        yield e
    finally:
        e.set_regex_loops(False)
        e.force_regex_loops_road(AUTO)
        e.force_regex_grid(0)
        e.inject_failure(0)
        e.set_cpu_fallback(None)


def rx(pats, **kw):
    return abi.Params(list(pats), regex=True, **kw)


_expected = {}


def expected(pats, text, **kw):
    """what regex_search of the compiled reference returns for the expression the CLI compiles (once per case)"""
    key = (tuple(pats), text.tobytes(), tuple(sorted(kw.items())))
    if key not in _expected:
        assert regex_ref.available(), "the compiled reference (oracle/_ref/libkrep_ref_avx2.so) is missing"
        _expected[key] = regex_ref.call(regex_alt_model.joined(pats), text, **kw)
    return _expected[key]


def check(gpu, pats, text, **kw):
    want = expected(pats, text, **kw)
    got = gpu.search(rx(pats, **kw), text)
    assert gpu.last_status() == abi.STATUS_OK, gpu.last_error()
    assert got[0] == want[0], (pats, text.size, kw, got[0], want[0])
    assert np.array_equal(got[1], want[1]), (pats, text.size, kw, got[1][:6], want[1][:6])
    return want


def to_device(a, shift=0, pad=PAD):
    import torch
    t = torch.full((a.size + shift + 64,), pad, dtype=torch.uint8, device="cuda")
    if a.size:
        t[shift:shift + a.size] = torch.from_numpy(a.copy())
    return t, t.data_ptr() + shift


def background(rng, n, alphabet):
    al = np.frombuffer(alphabet, dtype=np.uint8)
    return al[rng.randint(0, al.size, size=n)].copy()


def put_line(t, s, line):
    """`line` as a line of its own from s on: a newline in front of it and one behind it"""
    p = np.frombuffer(b"\n" + line + b"\n", dtype=np.uint8)
    if s - 1 < 0 or s + len(line) + 1 > t.size:
        return
    t[s - 1:s - 1 + len(p)] = p


def planted(rng, n, alphabet, plants, decoys):
    """a text of short random lines over `alphabet` (it holds the newline) with every plant as a line of its own around 16-byte lane,
    1-KiB cell, 8-KiB round and 32-KiB unit boundaries of the filter scan (plant i at the (i + 1)-th boundary of each kind: straddling
    it, ending on it, starting on it), decoy lines (they hold the filter and no match) beside them, a plant as the first line of the
    text and one as a last line without a newline"""
    t = background(rng, n, alphabet)
    lines = list(plants) + list(decoys)
    for i, line in enumerate(lines):
        L = len(line)
        for b in (LANE, CELL, ROUND, UNIT):
            B = b * (i + 1)
            for k, s in enumerate(sorted({B - 1, B - max(1, L // 2), B, B - L, B - L + 1})):
                put_line(t, s + 3 * b * len(lines) * (k % 2), line)  # (kept apart from the next line's copies)
        put_line(t, 40 + 80 * i, line)
    first, last = np.frombuffer(plants[0] + b"\n", dtype=np.uint8), np.frombuffer(b"\n" + plants[-1], dtype=np.uint8)
    if n > first.size + last.size:
        t[:first.size] = first
        t[n - last.size:] = last
    return t


# (patterns, alphabet of the background lines, lines that hold a match, decoy lines: the filter without a match)
SHAPES = [
    ([b"ERROR.*timeout"], b"EROtimeu:  \n", [b"ERROR: a timeout", b"xERRORtimeout timeout", b"ERROR ERROR timeoutimeout."], [b"a timeout, no error", b"timeout ERROR"]),
    ([b"a+b"], b"aabc \n", [b"ab", b"xaaaab", b"aabaab ab"], []),
    ([b"ab*c"], b"abbc \n", [b"ac", b"abbbbc", b"abcac abbc"], [b"abx", b"abbb b"]),
    ([b"[0-9]+\\.[0-9]+"], b"0123. x\n", [b"3.14", b"v10.25.7 1.5", b"x0.0"], [b"12. 5", b".5 5."]),
    ([b"colou*r"], b"colur \n", [b"color", b"colouuur", b"colorcolour colr"], [b"colou", b"coloux colo r"]),
    ([b"x(a+|b)y"], b"xaby \n", [b"xay", b"xaaaay xby", b"xbyxay"], [b"xab", b"xa y xbb"]),
    ([b"[ab]+c?"], b"abc \n", [b"a", b"abbac", b"c ab c abc"], []),
    ([b"^a+"], b"aab \n", [b"a", b"aaaa b aa", b"aab"], [b" a", b"baaa"]),
    ([b"b+$"], b"abb \n", [b"b", b"a bbb", b"bb abb"], [b"b a", b"bbbx"]),
    ([b"a+", b"b+c"], b"abc \n", [b"a", b"bbc", b"xbc aa"], [b"b c"]),
]
LENGTHS = [0, 1, 2, 15, 16, 17, 1023, 1024, 1025, 8193, 32769, 100001]
MODES = (dict(), dict(track_positions=False), dict(count_lines=True), dict(case_sensitive=False))
CAPPED = tuple(dict(max_count=mc, **kw) for mc in (0, 1, 3, 10 ** 9) for kw in (dict(), dict(track_positions=False), dict(count_lines=True)))


@pytest.mark.parametrize("shape", range(len(SHAPES)))
def test_operator_equals_regex_search(gpu, shape):
    pats, alphabet, plants, decoys = SHAPES[shape]
    gpu.regex_compile_loops(rx(pats))
    with pytest.raises(KrepGpuError):
        gpu.regex_compile_ext(rx(pats))  # (the older compilers refuse it: this is the new road)
    rng = np.random.RandomState(3100 + shape)
    gpu.force_regex_loops_road(AUTO)
    for n in LENGTHS:
        text = planted(rng, n, alphabet, plants, decoys)
        for kw in MODES + (CAPPED if n in (1025, 32769) else ()):
            check(gpu, pats, text, **kw)
        if n >= 1024:
            assert expected(pats, text)[0] > (12 if n > UNIT else 2)  # the planted lines are found
            if decoys:  # ... and the decoys hold no match
                t2 = np.frombuffer(b"\n".join(decoys), dtype=np.uint8)
                assert expected(pats, t2)[0] == 0
    # max_count == 0 without -c and without positions: 1 as soon as one match exists
    assert gpu.search(rx(pats, max_count=0, track_positions=False), text)[0] == 1


@pytest.mark.parametrize("road", [SPARSE, DENSE])
def test_both_roads_on_every_shape(gpu, road):
    """each road forced on a text it would and on one it would not choose: the same records, the same -c"""
    rng = np.random.RandomState(77 + road)
    try:
        gpu.force_regex_loops_road(road)
        for pats, alphabet, plants, decoys in SHAPES:
            text = planted(rng, 70001, alphabet, plants, decoys)
            before = gpu.regex_loops_roads()
            for kw in (dict(), dict(count_lines=True), dict(max_count=3), dict(case_sensitive=False, track_positions=False)):
                check(gpu, pats, text, **kw)
            after = gpu.regex_loops_roads()
            assert after[road - 1] - before[road - 1] == 4 and after[2 - road] == before[2 - road], (pats, before, after)
    finally:
        gpu.force_regex_loops_road(AUTO)


def test_the_last_line_ends_without_a_newline_and_the_case_decides(gpu):
    """b+$ on a text that ends in b's without a newline: found in a case-sensitive search, not under -i (REG_NOTEOL)"""
    rng = np.random.RandomState(5)
    for road in (SPARSE, DENSE):
        gpu.force_regex_loops_road(road)
        try:
            for n in (3, 17, 1024, 1027, 32768, 40003):
                for tail in (b"abb", b"bb\n", b"b a", b"\nb"):
                    text = background(rng, n, b"ab \n")
                    text[n - len(tail):] = np.frombuffer(tail, dtype=np.uint8)
                    for kw in (dict(), dict(count_lines=True)):
                        check(gpu, [b"b+$"], text, **kw)
                        check(gpu, [b"b+$"], text, case_sensitive=False, **kw)
                    ends = expected([b"b+$"], text)[1][:, 1].tolist()
                    ends_i = expected([b"b+$"], text, case_sensitive=False)[1][:, 1].tolist()
                    assert (n in ends) == (tail in (b"abb", b"\nb")) and n not in ends_i, (n, tail)
        finally:
            gpu.force_regex_loops_road(AUTO)


def test_long_runs_inside_one_match(gpu):
    """a repeated run of 17, 1 025 and 3 000 bytes inside one match: more than a lane, a cell, and most of the longest line walked"""
    rng = np.random.RandomState(6)
    for run in (17, 1025, 3000):
        for pats, line, alphabet in (([b"a+b"], b"x" + b"a" * run + b"b", b"ac \n"),
                                     ([b"ERROR.*timeout"], b"ERROR" + b"-" * run + b"timeout tail", b"EROtimeu \n"),
                                     ([b"colou*r"], b"colo" + b"u" * run + b"r", b"colur \n"),
                                     ([b"[0-9]+\\.[0-9]+"], b"7" * run + b"." + b"1" * min(run, 1000), b"01. \n"),
                                     ([b"^a+"], b"a" * run + b" a", b"ab \n")):
            text = background(rng, 20000, alphabet)
            for s in (1, 1000, CELL * 8 - run // 2 if run < 8000 else 3000, 20000 - len(line) - 1):
                put_line(text, max(s, 1), line)
            for road in (SPARSE, DENSE):
                gpu.force_regex_loops_road(road)
                try:
                    want = check(gpu, pats, text)
                    check(gpu, pats, text, count_lines=True)
                finally:
                    gpu.force_regex_loops_road(AUTO)
            assert (want[1][:, 1] - want[1][:, 0]).max() >= run


def test_several_matches_in_one_line_and_the_longest_end(gpu):
    cases = [([b"a+b"], b"aab ab xaaab\nab"), ([b"a+b"], b"ab ab ab"),                          # two and three matches: the walk resumes at the end
             ([b"[ab]+c?"], b"abcab c\nabc abc abc"),
             ([b"ab*c|ab"], b"abbc ab abc"),                                                    # the first end is not the longest
             ([b"a.*b"], b"a b ab b a\nb a"), ([b"x(a+|b)y"], b"xayxby xaay"), ([b"a+", b"a+b"], b"aab a"),
             ([b"[0-9]+\\.[0-9]+"], b"v1.25 and 10.0.3")]
    for pats, t in cases:
        text = np.frombuffer(t, dtype=np.uint8)
        for road in (SPARSE, DENSE):
            gpu.force_regex_loops_road(road)
            try:
                for kw in (dict(), dict(count_lines=True), dict(max_count=1), dict(max_count=2), dict(case_sensitive=False)):
                    check(gpu, pats, text, **kw)
            finally:
                gpu.force_regex_loops_road(AUTO)
    assert expected([b"ab*c|ab"], np.frombuffer(b"abbc ab abc", dtype=np.uint8))[1].tolist() == [[0, 4], [5, 7], [8, 11]]
    assert expected([b"a+b"], np.frombuffer(b"ab ab ab", dtype=np.uint8))[1].tolist() == [[0, 2], [3, 5], [6, 8]]


EDGES = [b"", b"\n", b"\n\n\n", b"aab", b"aab\n", b"\naab", b"\n\naab\n\n", b"aab\nxx\naab", b"x\n\n\naab\n\n\nab", b"b\naab\nb", b"a", b"b",
         b"aab" * 50, b"aab\n" * 50 + b"aab"]


def test_edge_texts(gpu):
    """the first line, empty lines, a last line without a newline, a text without any newline, the empty text"""
    for road in (AUTO, SPARSE, DENSE):
        gpu.force_regex_loops_road(road)
        try:
            for t in EDGES:
                text = np.frombuffer(t, dtype=np.uint8)
                for pats in ([b"a+b"], [b"^a+"], [b"b+$"], [b"^a+b$"], [b"a*b"]):
                    for kw in (dict(), dict(count_lines=True), dict(track_positions=False), dict(case_sensitive=False)):
                        check(gpu, pats, text, **kw)
        finally:
            gpu.force_regex_loops_road(AUTO)


def scan_records(plan, d_text, n, cap=1 << 16, **kw):
    import torch
    pos = torch.full((2 * cap,), -1, dtype=torch.int64, device="cuda")
    out = plan.scan(d_text, n, 0, n, 0, pos.data_ptr(), cap, **kw)
    return out, pos.cpu().numpy()


def test_plans_on_unaligned_device_text_positions_capacity_and_line_facts(gpu):
    rng = np.random.RandomState(8)
    pats, alphabet, plants, decoys = SHAPES[1]
    n = 50001
    text = planted(rng, n, alphabet, plants, decoys)
    want = expected(pats, text)
    want_c = expected(pats, text, count_lines=True)
    assert want[0] > 100
    for shift in (0, 1, 7):
        hold, d_text = to_device(text, shift)
        for road in (SPARSE, DENSE):
            gpu.force_regex_loops_road(road)
            plan, plan_c, plan_n, plan_3 = gpu.plan(rx(pats)), gpu.plan(rx(pats, count_lines=True)), gpu.plan(rx(pats, track_positions=False)), \
                gpu.plan(rx(pats, max_count=3))
            try:
                out, pos = scan_records(plan, d_text, n)
                assert (out.count, out.stored, out.total_matches, out.overflow) == (want[0], want[0], want[0], 0)
                assert np.array_equal(pos[:2 * want[0]].astype(np.uint64).reshape(-1, 2), want[1]) and (pos[2 * want[0]:] == -1).all()
                # a position buffer that is too small: the first `cap` records, overflow
                out, pos = scan_records(plan, d_text, n, cap=10)
                assert (out.count, out.stored, out.total_matches, out.overflow) == (want[0], 10, want[0], 1)
                assert np.array_equal(pos.astype(np.uint64).reshape(-1, 2), want[1][:10])
                # no buffer, and no positions wanted: the count alone
                assert plan.scan(d_text, n).count == want[0] and plan_n.scan(d_text, n).count == want[0]
                out, pos = scan_records(plan_n, d_text, n)
                assert out.count == want[0] and out.stored == 0 and (pos == -1).all()
                # max_count: the first three, at their final index
                out, pos = scan_records(plan_3, d_text, n)
                assert (out.count, out.stored, out.total_matches) == (3, 3, want[0]) and (pos[6:] == -1).all()
                assert np.array_equal(pos[:6].astype(np.uint64).reshape(-1, 2), want[1][:3])
                # -c with the line facts of the whole window
                o = plan_c.scan(d_text, n)
                nl = np.flatnonzero(text == 10)
                starts = want[1][:, 0].astype(np.int64)
                assert (o.count, o.line_count) == (want_c[0], want_c[0])
                assert (bool(o.has_newline), bool(o.head_line_hit), bool(o.tail_line_hit)) == (True, bool(starts[0] < nl[0]), bool(starts[-1] > nl[-1]))
            finally:
                gpu.force_regex_loops_road(AUTO)
                for p in (plan, plan_c, plan_n, plan_3):
                    p.close()
        del hold
    # a text without a newline: -c says so on both roads, with and without a match
    for t in (b"xx aab yy", b"xx yy"):
        text = np.frombuffer(t, dtype=np.uint8)
        hold, d_text = to_device(text, 5, pad=10)
        for road in (SPARSE, DENSE):
            gpu.force_regex_loops_road(road)
            plan_c = gpu.plan(rx(pats, count_lines=True))
            try:
                o = plan_c.scan(d_text, text.size)
                hit = b"aab" in t
                assert (o.line_count, bool(o.has_newline), bool(o.head_line_hit), bool(o.tail_line_hit)) == (int(hit), False, hit, hit)
            finally:
                gpu.force_regex_loops_road(AUTO)
                plan_c.close()
        del hold


def word_text(rng, n):
    words = [bytes(rng.randint(97, 123, size=rng.randint(2, 9)).astype(np.uint8)) for _ in range(300)]
    out = bytearray()
    while len(out) < n:
        out += words[rng.randint(len(words))] + (b"\n" if rng.randint(9) == 0 else b" ")
    return np.frombuffer(bytes(out[:n]), dtype=np.uint8).copy()


def test_the_roads_agree_and_auto_picks_by_the_filters_density(gpu):
    rng = np.random.RandomState(9)
    # a sparse text: both roads forced give what auto gives, and auto takes the sparse road
    pats, alphabet, plants, decoys = [b"ERROR.*timeout"], b"abcdefgh \n", SHAPES[0][2], SHAPES[0][3]
    text = planted(rng, 65536, alphabet, plants, decoys)
    results = {}
    for road in (AUTO, SPARSE, DENSE):
        gpu.force_regex_loops_road(road)
        try:
            before = gpu.regex_loops_roads()
            results[road] = [check(gpu, pats, text, **kw) for kw in (dict(), dict(count_lines=True))]
            after = gpu.regex_loops_roads()
            took = (after[0] - before[0], after[1] - before[1])
            assert took == ((2, 0) if road in (AUTO, SPARSE) else (0, 2)), (road, took)
        finally:
            gpu.force_regex_loops_road(AUTO)
    assert results[AUTO][0][0] > 4
    # a 64-KiB word text with [a-z]+: the filter [a-z] occurs on most bytes, auto must pick the dense road
    text = word_text(rng, 65536)
    pats = [b"[a-z]+"]
    before = gpu.regex_loops_roads()
    want = check(gpu, pats, text)
    check(gpu, pats, text, count_lines=True)
    after = gpu.regex_loops_roads()
    assert (after[0] - before[0], after[1] - before[1]) == (0, 2) and want[0] > 8000
    for road in (SPARSE, DENSE):
        gpu.force_regex_loops_road(road)
        try:
            check(gpu, pats, text)
            check(gpu, pats, text, count_lines=True)
            check(gpu, pats, text, max_count=3)
        finally:
            gpu.force_regex_loops_road(AUTO)


def test_starved_grid_a_lane_takes_several_lines(gpu):
    """70 000 three-byte lines, a+, the walk's grid capped at 1 and at 2 workgroups (krep_gpu_debug_force_regex_grid): a lane takes line
    after line, 137 and 274 lines apart, and writes each line's records at that line's own offset"""
    rng = np.random.RandomState(10)
    words = np.frombuffer(b"aa\nab\nbb\nba\nb \n a\n", dtype=np.uint8).reshape(-1, 3)
    text = words[rng.randint(0, words.shape[0], size=70000)].reshape(-1).copy()
    pats = [b"a+"]
    jobs = (dict(), dict(track_positions=False), dict(count_lines=True), dict(max_count=50000))
    wants = [expected(pats, text, **kw) for kw in jobs]
    assert wants[0][0] > 30000
    try:
        for blocks in (1, 2):
            for road in (SPARSE, DENSE):
                gpu.force_regex_grid(blocks)
                gpu.force_regex_loops_road(road)
                for kw, want in zip(jobs, wants):
                    got = gpu.search(rx(pats, **kw), text)
                    assert gpu.last_status() == abi.STATUS_OK
                    assert got[0] == want[0] and np.array_equal(got[1], want[1]), (blocks, road, kw, got[0], want[0])
    finally:
        gpu.force_regex_grid(0)
        gpu.force_regex_loops_road(AUTO)


def cpu_selector():
    """a CPU selector that hands back the reference's own regex_search"""
    ref_fn = C.cast(regex_ref._lib().regex_search, C.c_void_p).value
    select_t = C.CFUNCTYPE(C.c_void_p, C.POINTER(abi.SearchParams))
    return select_t(lambda pp: ref_fn)


def test_a_line_of_4096_bytes_is_walked_and_one_of_4097_is_not(gpu):
    rng = np.random.RandomState(11)
    pats = [b"a+b"]
    for road in (SPARSE, DENSE):
        gpu.force_regex_loops_road(road)
        try:
            for extra, ok in ((0, True), (1, False)):
                text = background(rng, 30000, b"aac \n")
                line = b"a" * (4095 + extra) + b"b"
                put_line(text, 9000, line)
                put_line(text, 200, b"xaab")
                assert len(line) == 4096 + extra
                want = expected(pats, text)
                assert [4096 + extra] == [int(e - s) for s, e in want[1] if e - s > 100]
                hold, d_text = to_device(text, 3)
                plan, plan_c = gpu.plan(rx(pats)), gpu.plan(rx(pats, count_lines=True))
                try:
                    if ok:
                        out, pos = scan_records(plan, d_text, text.size)
                        assert out.count == want[0] and np.array_equal(pos[:2 * want[0]].astype(np.uint64).reshape(-1, 2), want[1])
                        assert plan_c.scan(d_text, text.size).count == expected(pats, text, count_lines=True)[0]
                        check(gpu, pats, text)
                    else:
                        import torch
                        pos = torch.full((2 << 16,), -1, dtype=torch.int64, device="cuda")
                        for pl in (plan, plan_c):
                            with pytest.raises(KrepGpuError, match="a line of more than 4096 bytes: kept on krep's regex_search"):
                                pl.scan(d_text, text.size, 0, text.size, 0, pos.data_ptr(), 1 << 16)
                        assert (pos == -1).all().item()  # nothing written
                        # the operator takes the failure road: without a CPU function FAILED, with one its answer
                        with pytest.raises(KrepGpuError, match="more than 4096 bytes"):
                            gpu.search(rx(pats), text)
                        assert gpu.last_status() == abi.STATUS_FAILED
                        cb = cpu_selector()
                        gpu.set_cpu_fallback(C.cast(cb, C.c_void_p).value)
                        try:
                            for kw in (dict(), dict(count_lines=True)):
                                p = rx(pats, **kw)
                                comp = regex_ref.Compiled(pats[0])
                                p.s.compiled_regex = comp.ptr
                                got = gpu.search(p, text)
                                w = expected(pats, text, **kw)
                                assert gpu.last_status() == abi.STATUS_FELL_BACK and got[0] == w[0] and np.array_equal(got[1], w[1])
                        finally:
                            gpu.set_cpu_fallback(None)
                finally:
                    plan.close()
                    plan_c.close()
                del hold
        finally:
            gpu.force_regex_loops_road(AUTO)


def test_bounded_work_the_worst_line_the_rule_admits(gpu, capsys):
    """One 4096-byte line of a's among 1 000 ordinary lines, a.*b, no match: every start of the long line walks to the line's end, about
    8.4 M state steps in one lane.  It is the worst case the 4096 rule admits, run once; the time is printed (DESIGN §4.9 records it).
    Measured on an MI355X when this test was written: kernel_ms = 1229 and 1234 in two runs."""
    rng = np.random.RandomState(12)
    lines = [bytes(background(rng, rng.randint(5, 60), b"acd ")) for _ in range(1000)]
    lines.insert(500, b"a" * 4096)
    text = np.frombuffer(b"\n".join(lines) + b"\n", dtype=np.uint8)
    pats = [b"a.*b"]
    want = expected(pats, text)
    assert want[0] == 0
    hold, d_text = to_device(text, 1)
    plan = gpu.plan(rx(pats))
    try:
        plan.scan(d_text, text.size)  # (the first scan builds the inner plans)
        out = plan.scan(d_text, text.size, time_it=True)
        assert (out.count, out.total_matches, out.stored) == (0, 0, 0)
        with capsys.disabled():
            print("\n[regex loops] a.*b over one 4096-byte line of a's and 1000 ordinary lines: kernel_ms = %.3f" % out.kernel_ms)
    finally:
        plan.close()
    del hold


def test_a_window_that_is_not_the_whole_text_is_refused(gpu):
    text = np.frombuffer(b"xx aab yy\n" * 400, dtype=np.uint8)
    n = text.size
    hold, d_text = to_device(text)
    assert gpu.split_mode(rx([b"a+b"]), n) == abi.SPLIT_WHOLE and gpu.split_mode(rx([b"a+b"], count_lines=True), n) == abi.SPLIT_WHOLE
    for kw in (dict(), dict(count_lines=True)):
        plan = gpu.plan(rx([b"a+b"], **kw))
        try:
            for args in ((16, n), (0, n - 10), (0, n, 100)):
                with pytest.raises(KrepGpuError, match="scan the whole text in one window"):
                    plan.scan(d_text, n, *args)
            with pytest.raises(KrepGpuError, match="scan the whole text in one window"):
                plan.scan(d_text, n, 0, n, 0, global_len=n + 50)
            assert plan.scan(d_text, n).count == 400
        finally:
            plan.close()
    del hold


def test_search_batch_of_fifty_items_equals_the_reference_per_item(gpu):
    rng = np.random.RandomState(13)
    for pats, alphabet in (([b"a+b"], b"aabc \n"), ([b"ERROR.*timeout"], b"EROtimeu: \n"), ([b"b+$"], b"abb \n"), ([b"^a+"], b"aab \n")):
        items = [background(rng, rng.randint(0, 400), alphabet) for _ in range(50)]
        items[7] = np.zeros(0, dtype=np.uint8)
        items[11] = np.frombuffer(b"ERROR timeout aab", dtype=np.uint8)  # no newline at all, a match that ends the item
        for kw in (dict(), dict(count_lines=True)):
            assert gpu.batch_can_accelerate(rx(pats, **kw)), gpu.last_error()
            got = gpu.search_batch(rx(pats, **kw), items)
            assert len(got) == 50
            for k, (it, (cnt, pos)) in enumerate(zip(items, got)):
                want = expected(pats, it, **kw)
                assert cnt == want[0], (pats, kw, k, cnt, want[0])
                if not kw:
                    assert np.array_equal(pos, want[1]), (pats, k)
    # $ under -i stays refused in a batch
    assert not gpu.batch_can_accelerate(rx([b"b+$"], case_sensitive=False))


def test_the_switch_off_gives_the_library_every_other_test_expects(gpu):
    text = np.frombuffer(b"abcbc abc\n" * 100, dtype=np.uint8)
    gpu.set_regex_loops(False)
    try:
        for pats in ([b"a.*b"], [b"colou*r"]):
            assert not gpu.can_accelerate(rx(pats)) and gpu.select(rx(pats)) is None
            with pytest.raises(KrepGpuError, match="kept on krep's regex_search"):
                gpu.search(rx(pats), text)
            assert gpu.last_status() == abi.STATUS_FAILED
    finally:
        gpu.set_regex_loops(True)
    assert gpu.can_accelerate(rx([b"a.*b"]))
    check(gpu, [b"a.*b"], text)
