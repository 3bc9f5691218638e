"""krep -E on the device for alternations of class sequences (kg_regex_alt.hip) against the reference's regex_search: the compiled
reference (oracle/_ref, through tests/regex_ref.py) answers every case with the expression the CLI compiles; the rule of
tests/regex_alt_model.py must agree with it each time."""
import ctypes as C

import numpy as np
import pytest

import regex_alt_model as am
import regex_model
import regex_ref
from krep_amd import abi
from krep_amd.engine import KrepGpuError

pytestmark = pytest.mark.gpu

PAD = 0xEE
UNIT = 32768


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
    yield e
    e.inject_failure(0)
    e.set_cpu_fallback(None)
    e.force_regex_grid(0)


def rx(pats, **kw):
    return abi.Params(list(pats), regex=True, **kw)


def expected(pats, text, **kw):
    """what regex_search returns for the alternation: the compiled reference answers, the model must agree with it"""
    assert regex_ref.available(), "the compiled reference (oracle/_ref/libkrep_ref_avx2.so) is missing"
    ref = am.ref_call(pats, text, **kw)
    want = am.run(pats, text, **kw)
    assert ref[0] == want[0] and np.array_equal(ref[1], want[1]), ("model != reference", pats, kw, text.size)
    return ref


def check(gpu, pats, text, **kw):
    want = expected(pats, text, **kw)
    got = gpu.search(rx(pats, **kw), text)
    assert gpu.last_status() == abi.STATUS_OK
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


def planted(rng, n, alphabet, plants):
    """a text over `alphabet` with a copy of every plant straddling a 16-byte lane boundary, a 1-KiB cell boundary and a 32-KiB unit
    boundary (plant i at the (i + 1)-th boundary of each kind), and one plant ending on the last byte of the text"""
    t = background(rng, n, alphabet)
    for i, plant in enumerate(plants):
        p = np.frombuffer(plant, dtype=np.uint8)
        spots = [b * (i + 1) - k for b in (16, 1024, 32768) for k in {1, max(1, len(p) - 1), max(1, len(p) // 2)}] + [40 + 64 * i, 5000 + 64 * i]
        if n % len(plants) == i:
            spots += [n - len(p), 0]
        for s in spots:
            if 0 <= s and s + len(p) <= n:
                t[s:s + len(p)] = p
    return t


LOWER = b"abcdefghijklmnopqrstuvwxyz \n"
# (patterns, alphabet of the text, a string for every branch)
SHAPES = [
    ([b"a|bc"], b"abc \n", [b"a", b"bc"]),                                        # lengths 1 and 2
    ([b"cat|d[oi]g|b.rd"], LOWER, [b"cat", b"dig", b"bird"]),
    ([b"x|[a-c]{16}"], b"abcxyz \n", [b"x", b"abcabcabcabcabca"]),                # lengths 1 and 16: the widest spill
    ([b"a{16}|b{16}"], b"abc\n", [b"a" * 16, b"b" * 16]),                         # a full state word
    ([b"ab|abc"], b"abc \n", [b"ab", b"abc"]),                                    # same start: the longest; greedy
    ([b"a|aa"], b"ab\n", [b"a", b"aa"]),
    ([b"[ab]{2}|a{3}"], b"abc\n", [b"ba", b"aaa"]),
    ([b"q[^b]{3}|xy"], b"qbxy\x00c\n", [b"q\x00cc", b"xy"]),                      # a class that holds NUL
    ([b"j[[:space:]]ab|\nc"], b"abcj \n", [b"j\nab", b"\nc"]),                    # a class and a literal newline, for -c
    ([b"ERROR", b"WARN[0-9]"], b"EROWAN0123 \n", [b"ERROR", b"WARN7"]),           # two patterns: (ERROR)|(WARN[0-9])
]
LENGTHS = [0, 1, 15, 16, 17, 31, 32, 33, 1023, 1024, 1025, 32767, 32768, 32769, 300001]
MODES = (dict(), dict(track_positions=False), dict(count_lines=True), dict(case_sensitive=False))
CAPPED = tuple(dict(max_count=mc, **kw) for mc in (0, 1, 5) for kw in (dict(), dict(track_positions=False), dict(count_lines=True)))


@pytest.mark.parametrize("shape", range(len(SHAPES)))
def test_operator_equals_regex_search(gpu, shape):
    pats, alphabet, plants = SHAPES[shape]
    info = gpu.regex_compile_alt(rx(pats))
    assert info.n_branches == len(plants)
    rng = np.random.RandomState(1900 + shape)
    for n in sorted(set(LENGTHS + [info.Lmin - 1, info.Lmin, info.Lmax - 1, info.Lmax])):
        text = planted(rng, n, alphabet, plants)
        for kw in MODES + (CAPPED if n in (33, 1025, 32769) else ()):
            check(gpu, pats, text, **kw)
        if n >= 1024:
            assert expected(pats, text)[0] > 0  # the planted copies are found
    # max_count == 0 without -c and without positions: 1 as soon as one occurrence exists
    assert gpu.search(rx(pats, max_count=0, track_positions=False), text)[0] == 1


def test_nothing_behind_the_text_matches(gpu):
    """q[^b]{3}: texts that end in q plus 0..3 bytes, in an allocation whose pad byte lies in [^b], and as a host text: an occurrence
    needs all its bytes in front of text_len, in the guarded rounds and through the zeros they substitute ([^b] holds NUL)"""
    pats = [b"q[^b]{3}|xy"]
    rng = np.random.RandomState(44)
    for n in (4, 16, 17, 19, 1024, 1026, 8192, 8195, 32768, 32771, 40000):
        for tail in (b"q", b"qc", b"qcc", b"qccc", b"x", b"xy"):
            text = background(rng, n, b"bbbbq\x00cy\n")
            text[max(0, n - 8):] = ord("b")  # (no match reaches into the tail from the background)
            text[n - len(tail):] = np.frombuffer(tail, dtype=np.uint8)
            want = check(gpu, pats, text)
            check(gpu, pats, text, count_lines=True)
            hold, d_text = to_device(text, 3, pad=ord("c"))
            for kw in (dict(), dict(count_lines=True)):
                plan = gpu.plan(rx(pats, **kw))
                try:
                    out = plan.scan(d_text, n)
                    assert out.count == expected(pats, text, **kw)[0], (n, tail, kw)
                finally:
                    plan.close()
            ends = want[1][:, 1] if want[1].size else np.zeros(0)
            assert (n in ends) == (tail in (b"qccc", b"xy")), (n, tail)
            del hold


def test_runs_of_one_byte(gpu):
    """a text of only `a`s: every position starts an occurrence of every branch; the last size takes the pointer-jumping walk"""
    for n in (1, 2, 3, 16, 17, 1025, 32769, 100000):
        text = np.full(n, ord("a"), dtype=np.uint8)
        for pats in ([b"a|aa"], [b"[ab]{2}|a{3}"]):
            for kw in (dict(), dict(track_positions=False), dict(max_count=5), dict(count_lines=True)):
                check(gpu, pats, text, **kw)


def scan_records(plan, d_text, n, own_lo, own_hi, global_base=0, global_len=0):
    import torch
    cap = 1 << 16
    pos = torch.full((2 * cap,), -1, dtype=torch.int64, device="cuda")
    out = plan.scan(d_text, n, own_lo, own_hi, global_base, pos.data_ptr(), cap, global_len=global_len)
    assert not out.overflow and out.stored == out.count
    return out, pos[:2 * int(out.stored)].cpu().numpy().astype(np.uint64).reshape(-1, 2)


def window_lines(brs, text, lo, hi):
    """line_count, has_newline, head_line_hit, tail_line_hit of include/krep_gpu.h for the window [lo, hi): the starts and the newlines
    the window owns; a start ON a newline belongs to the line that newline ends"""
    occ, _ = am.occurrences(brs, text)
    mine = occ[(occ >= lo) & (occ < hi)]
    nl = np.flatnonzero(text[lo:hi] == 10) + lo
    lines = np.unique(np.searchsorted(nl, mine, side="left")).size
    head = bool(mine.size) and (nl.size == 0 or mine[0] <= nl[0])
    tail = bool(mine.size) and (nl.size == 0 or mine[-1] > nl[-1])
    return int(lines), bool(nl.size), bool(head), bool(tail)


WINDOWS = ((15, 33), (16, 32), (17, 31), (1, 16), (1023, 1025), (1024, 2048), (31, 32769), (32768, 39999), (0, 40000))


@pytest.mark.parametrize("shift", [0, 3])
def test_windows_own_by_start(gpu, shift):
    """Start ownership with branches of 1 and 16 bytes: copies of EACH branch start at own_lo - 1 and own_hi - 1, or at own_lo and own_hi
    (two 16-byte copies one byte apart cannot both stand), and end at n; owned is exactly start in [own_lo, own_hi).  x|[a-c]{16} can overlap itself ([a-c]{16} does), so without -c it takes one
    window only: its windows are checked under -c, and the records and the count-only scan of a window with q|a[b-d]{15}, the same
    two lengths without an overlap."""
    n = 40000
    rng = np.random.RandomState(50 + shift)
    for pats, long16, short, records in (([b"q|a[b-d]{15}"], b"abcdbcdbcdbcdbcd", b"q", True), ([b"x|[a-c]{16}"], b"abcabcabcabcabca", b"x", False)):
        brs = am.branches(pats)
        assert gpu.regex_compile_alt(rx(pats)).cross_overlap == (0 if records else 1)
        plan, plan_c = gpu.plan(rx(pats)), gpu.plan(rx(pats, count_lines=True))
        try:
            for own_lo, own_hi in WINDOWS:
                for plant, other, first in ((long16, short, True), (short, long16, True), (long16, short, False), (short, long16, False)):
                    text = background(rng, n, b"yz \n\n")
                    p, o = np.frombuffer(plant, dtype=np.uint8), np.frombuffer(other, dtype=np.uint8)
                    wide = own_hi - own_lo >= 80 and own_lo >= 1 and own_hi + 16 <= n
                    if wide:
                        mid = (own_lo + own_hi) // 2
                        text[mid:mid + len(o)] = o
                    for s in ((own_lo - 1, own_hi - 1, n - len(p)) if first else (own_lo, own_hi, n - len(p))):
                        if 0 <= s and s + len(p) <= n:
                            text[s:s + len(p)] = p
                    occ, lens = am.occurrences(brs, text)
                    keep = (occ >= own_lo) & (occ < own_hi)
                    mine, mlen = occ[keep], lens[keep]
                    if wide and first:
                        assert own_hi - 1 in mine and own_lo - 1 in occ and own_lo - 1 not in mine and n - len(p) in occ
                    elif wide:
                        assert own_lo in mine and own_hi in occ and own_hi not in mine
                    hold, d_text = to_device(text, shift)
                    o_c = plan_c.scan(d_text, n, own_lo, own_hi, 1000, global_len=1000 + n)
                    have = (int(o_c.line_count), bool(o_c.has_newline), bool(o_c.head_line_hit), bool(o_c.tail_line_hit))
                    assert have == window_lines(brs, text, own_lo, own_hi), (pats, own_lo, own_hi, plant)
                    if records:
                        out, rec = scan_records(plan, d_text, n, own_lo, own_hi, global_base=1000, global_len=1000 + n)
                        assert out.count == mine.size and out.total_matches == mine.size, (pats, shift, own_lo, own_hi, plant)
                        assert np.array_equal(rec[:, 0], mine.astype(np.uint64) + 1000)
                        assert np.array_equal(rec[:, 1] - rec[:, 0], mlen.astype(np.uint64))
                        assert plan.scan(d_text, n, own_lo, own_hi).count == mine.size  # count only
                    elif (own_lo, own_hi) != (0, n):
                        with pytest.raises(KrepGpuError, match="overlap"):
                            plan.scan(d_text, n, own_lo, own_hi)
                    else:
                        assert plan.scan(d_text, n).count == expected(pats, text)[0]
                    del hold
        finally:
            plan.close()
            plan_c.close()


def test_three_windows_concatenate_and_combine(gpu):
    rng = np.random.RandomState(60)
    n = 100 * 1024
    cuts = [0, 33333, 65537, n]
    for pats, alphabet, plants in (([b"j[[:space:]]ab|\nc"], b"abdj \n\n", [b"j\nab", b"\nc"]), ([b"q|a[b-d]{15}"], b"yz\n ", [b"q", b"abcdbcdbcdbcdbcd"]),
                                   ([b"x|[a-c]{16}"], b"yz\n ", [b"x", b"abcabcabcabcabca"])):
        text = planted(rng, n, alphabet, plants)
        for c in cuts[1:-1]:  # a 16-byte copy across each cut
            text[c - 5:c - 5 + len(max(plants, key=len))] = np.frombuffer(max(plants, key=len), dtype=np.uint8)
        hold, d_text = to_device(text)
        whole_lines = expected(pats, text, count_lines=True)
        pieces = gpu.split_mode(rx(pats), n) == abi.SPLIT_PIECES
        assert pieces == (pats != [b"x|[a-c]{16}"])
        plan, plan_c = gpu.plan(rx(pats)), gpu.plan(rx(pats, count_lines=True))
        try:
            recs, outs = [], []
            for lo, hi in zip(cuts[:-1], cuts[1:]):
                if pieces:
                    recs.append(scan_records(plan, d_text, n, lo, hi)[1])
                outs.append(plan_c.scan(d_text, n, lo, hi))
            if pieces:
                whole = expected(pats, text)
                assert np.array_equal(np.concatenate(recs), whole[1]) and sum(len(r) for r in recs) == whole[0]
            assert gpu.lib.krep_gpu_combine_line_counts((abi.ScanOut * 3)(*outs), 3) == whole_lines[0], pats
            assert plan_c.scan(d_text, n).line_count == whole_lines[0]
        finally:
            plan.close()
            plan_c.close()
        del hold
    # two occurrences can share a byte: one window only
    text = planted(rng, n, b"abc \n", [b"ab", b"abc"])
    hold, d_text = to_device(text)
    plan = gpu.plan(rx([b"ab|abc"]))
    try:
        assert gpu.split_mode(rx([b"ab|abc"]), n) == abi.SPLIT_WHOLE
        with pytest.raises(KrepGpuError, match="overlap"):
            plan.scan(d_text, n, 4096, 8192)
        out, rec = scan_records(plan, d_text, n, 0, n)
        want = expected([b"ab|abc"], text)
        assert out.count == want[0] and np.array_equal(rec, want[1])
    finally:
        plan.close()
    del hold


def test_starved_grid_a_wave_takes_several_units(gpu):
    """1 and 2 workgroups on 5 units (krep_gpu_debug_force_regex_grid): a wave rebuilds its entry state and its spill for every unit it
    takes, reads that unit's record offset, and adds up its counts"""
    n = 4 * UNIT + 100
    rng = np.random.RandomState(70)

    def sprinkled(alphabet, plants, step):
        t = planted(rng, n, alphabet, plants)
        for k, s in enumerate(range(step, n - 20, step)):
            p = np.frombuffer(plants[k % len(plants)], dtype=np.uint8)
            t[s:s + len(p)] = p
        for b in range(UNIT, n, UNIT):  # the long plant across every unit boundary, a short one directly in front of the next
            p = np.frombuffer(max(plants, key=len), dtype=np.uint8)
            t[b - len(p) // 2:b - len(p) // 2 + len(p)] = p
        return t

    jobs = []
    for pats, alphabet, plants in (([b"q|a[b-d]{15}"], b"yz\n ", [b"q", b"abcdbcdbcdbcdbcd"]), ([b"x|[a-c]{16}"], b"yz\n ", [b"x", b"abcabcabcabcabca"]),
                                   ([b"ab|abc"], b"abc \n", [b"ab", b"abc"]), ([b"ERROR", b"WARN[0-9]"], b"EROWAN0123 \n", [b"ERROR", b"WARN7"])):
        text = sprinkled(alphabet, plants, 701)
        jobs += [(pats, text, kw) for kw in (dict(track_positions=False), dict(), dict(count_lines=True))]
    wants = [expected(pats, text, **kw) for pats, text, kw in jobs]
    assert all(w[0] > 5 for w in wants)
    try:
        for blocks in (1, 2):
            gpu.force_regex_grid(blocks)
            for (pats, text, kw), want in zip(jobs, wants):
                got = gpu.search(rx(pats, **kw), text)
                assert gpu.last_status() == abi.STATUS_OK
                assert got[0] == want[0] and np.array_equal(got[1], want[1]), (blocks, pats, kw, got[0], want[0])
    finally:
        gpu.force_regex_grid(0)


def test_host_operators_and_shards(gpu):
    rng = np.random.RandomState(80)
    n = 3 * (1 << 20) + 77
    share = (n + 2) // 3
    for pats, alphabet, plants, kw, pieces in (
            ([b"q|a[b-d]{15}"], b"yz\n ", [b"q", b"abcdbcdbcdbcdbcd"], dict(), True),
            ([b"ERROR", b"WARN[0-9]"], LOWER, [b"ERROR", b"WARN7"], dict(max_count=3), True),
            ([b"x|[a-c]{16}"], b"yz\n ", [b"x", b"abcabcabcabcabca"], dict(count_lines=True), True),
            ([b"x|[a-c]{16}"], b"yz\n ", [b"x", b"abcabcabcabcabca"], dict(), False),
            ([b"ab|abc"], LOWER, [b"ab", b"abc"], dict(), False),
            ([b"ab|abc"], LOWER, [b"ab", b"abc"], dict(count_lines=True), True)):
        text = planted(rng, n, alphabet, plants)
        long16 = np.frombuffer(max(plants, key=len), dtype=np.uint8)
        # copies that start 1 and 3 bytes in front of the two cuts of three shards, and one inside each of two shards
        for s in (share - 1, 2 * share - 3, share + 100, 2 * share + 64):
            text[s:s + long16.size] = long16
        want = expected(pats, text, **kw)
        p = rx(pats, **kw)
        assert gpu.can_accelerate(p) and gpu.select(p) is not None
        got = gpu.search(p, text)
        assert gpu.last_status() == abi.STATUS_OK
        assert got[0] == want[0] and np.array_equal(got[1], want[1]), (pats, kw, got[0], want[0])
        rc, cnt, pos = gpu.search_buffer(p, text, num_gpus=3)
        assert rc == (0 if want[0] else 1) and gpu.last_status() == abi.STATUS_OK
        assert cnt == want[0] and np.array_equal(pos, want[1]), (pats, kw, cnt, want[0])
        assert (gpu.split_mode(p, n) == abi.SPLIT_PIECES) == pieces and gpu.last_shard_info().shards == (3 if pieces else 1), (pats, kw)
    # a refused alternation takes the failure road
    with pytest.raises(KrepGpuError, match="automaton"):
        gpu.search(rx([b"a|b.*"]), text[:1000])
    assert gpu.last_status() == abi.STATUS_FAILED


def test_injected_failure_falls_back_to_the_registered_regex_search(gpu):
    """the registered CPU selector hands back a regex_search; params (compiled_regex included) reach it untouched"""
    rng = np.random.RandomState(90)
    pats = [b"ERROR", b"WARN[0-9]"]
    text = planted(rng, 200000, LOWER, [b"ERROR", b"WARN7"])
    want = expected(pats, text, track_positions=False)
    seen = {}

    def cpu_regex_search(pp, t, n, res):
        seen["compiled"] = pp.contents.compiled_regex
        seen["n"] = n
        seen["np"] = pp.contents.num_patterns
        return want[0]

    fn = abi.SEARCH_FUNC(cpu_regex_search)
    select_t = C.CFUNCTYPE(C.c_void_p, C.POINTER(abi.SearchParams))
    ref_fn = C.cast(regex_ref._lib().regex_search, C.c_void_p).value
    cb = select_t(lambda pp: ref_fn if seen.get("use_ref") else C.cast(fn, C.c_void_p).value)
    gpu.set_cpu_fallback(C.cast(cb, C.c_void_p).value)
    try:
        p = rx(pats, track_positions=False)
        comp = regex_ref.Compiled(am.joined(pats))
        p.s.compiled_regex = comp.ptr
        gpu.inject_failure(3)
        got = gpu.search(p, text)
        assert gpu.last_status() == abi.STATUS_FELL_BACK and got[0] == want[0]
        assert seen["compiled"] == comp.ptr.value and seen["n"] == text.size and seen["np"] == 2
        # the reference's own function as the fallback, records included
        seen["use_ref"] = True
        p2 = rx(pats)
        p2.s.compiled_regex = comp.ptr
        full = expected(pats, text)
        got = gpu.search(p2, text)
        assert gpu.last_status() == abi.STATUS_FELL_BACK and got[0] == full[0] and np.array_equal(got[1], full[1])
        gpu.inject_failure(0)
        got = gpu.search(p, text)
        assert gpu.last_status() == abi.STATUS_OK and got[0] == want[0]
    finally:
        gpu.inject_failure(0)
        gpu.set_cpu_fallback(None)
