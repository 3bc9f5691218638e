"""krep -E on the device for what krep_gpu_regex_compile_ext() expands (?, {n,m}, inner groups, alternations between line anchors;
kg_regex_alt.hip, the anchored instantiations included) against the reference's regex_search: the compiled reference (oracle/_ref,
through tests/regex_ref.py) answers every case with the expression the CLI compiles; the rule of tests/regex_ext_model.py must
agree with it each time."""
import numpy as np
import pytest

import regex_ext_model as em
import regex_ref
from krep_amd import abi
from krep_amd.engine import KrepGpuError

pytestmark = pytest.mark.gpu

PAD = 0xEE
LANE, CELL, UNIT = 16, 1024, 32768


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
    e.set_stream_chunk(0)


def rx(pats, **kw):
    return abi.Params(list(pats), regex=True, **kw)


_expected = {}


def expected(pats, text, **kw):
    """what regex_search returns: the compiled reference answers (once per case), the model must agree with it"""
    key = (tuple(pats), text.tobytes(), tuple(sorted(kw.items())))
    if key not in _expected:
        assert regex_ref.available(), "the compiled reference (oracle/_ref/libkrep_ref_avx2.so) is missing"
        ref = em.ref_call(pats, text, **kw)
        want = em.run(pats, text, **kw)
        assert ref[0] == want[0] and np.array_equal(ref[1], want[1]), ("model != reference", pats, kw, text.size)
        _expected[key] = ref
    return _expected[key]


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


def put(t, s, plant, bol, eol, decoy=None):
    """a copy of `plant` at s with the newline its anchors ask for in front of / behind it (decoy: that byte instead)"""
    p = np.frombuffer(plant, dtype=np.uint8)
    if s < 0 or s + len(p) > t.size:
        return
    t[s:s + len(p)] = p
    if bol and s > 0:
        t[s - 1] = 10 if decoy is None else decoy
    if eol and s + len(p) < t.size:
        t[s + len(p)] = 10 if decoy is None else decoy


def planted(rng, n, alphabet, plants, bol=False, eol=False, filler=ord(" ")):
    """a text over `alphabet` with copies of every plant around 16-byte lane, 1-KiB cell and 32-KiB unit boundaries (plant i at the
    (i + 1)-th boundary of each kind): straddling it, behind a newline that is the LAST byte of a lane / cell / unit (^), in front of
    a newline that is the last and the first byte of one ($); decoys with another byte where the newline belongs; a copy at byte 0 and
    one that ends on the last byte of the text"""
    t = background(rng, n, alphabet)
    for i, plant in enumerate(plants):
        L = len(plant)
        for b in (LANE, CELL, UNIT):
            B = b * (i + 1)
            for s in {B - 1, B - max(1, L - 1), B - max(1, L // 2), B, B - L - 1, B - L}:
                put(t, s + 3 * b * len(plants), plant, bol, eol)   # (kept apart from the next plant's copies)
                put(t, s, plant, bol, eol)
        put(t, 40 + 64 * i, plant, bol, eol)
        put(t, 5000 + 64 * i, plant, bol, eol)
        if bol or eol:
            put(t, 7000 + 64 * i, plant, bol, eol, decoy=filler)
        if n % len(plants) == i:
            put(t, n - L, plant, bol, eol)
            put(t, 0, plant, bol, eol)
    return t


LOWER = b"abcdefghijklmnopqrstuvwxyz \n"
# (patterns, alphabet of the text, a string for every sequence of the expansion, bol, eol)
SHAPES = [
    ([b"colou?r"], b"colur \n", [b"color", b"colour"], 0, 0),
    ([b"https?://"], b"htps:/ \n", [b"http://", b"https://"], 0, 0),
    ([b"x(a|bc)y"], b"xabcy \n", [b"xay", b"xbcy"], 0, 0),
    ([b"[ab]{1,3}c"], b"abc \n", [b"ac", b"bac", b"abbc"], 0, 0),                        # overlap: the greedy road
    ([b"^(ERROR|WARN)"], b"EROWAN \n", [b"ERROR", b"WARN"], 1, 0),
    ([b"(foo|quux)$"], b"foqux \n", [b"foo", b"quux"], 0, 1),
    ([b"^(a|bc)d?$"], b"abcd\n\n", [b"a", b"ad", b"bc", b"bcd"], 1, 1),
    ([b"^(a{14}|b{14})$"], b"ab\n", [b"a" * 14, b"b" * 14], 1, 1),                        # all 32 places
    ([b"(x|[a-c]{15})$"], b"abcxy \n", [b"x", b"abcabcabcabcabc"], 0, 1),                 # lengths 1 and 15: the widest -c spill
    ([b"^(j[[:space:]]ab|\nc)"], b"abcj \n", [b"j\nab", b"\nc"], 1, 0),                   # classes that hold the newline
    ([b"^GET", b"^POST[0-9]"], b"GETPOS0123 \n", [b"GET", b"POST7"], 1, 0),               # two patterns: (^GET)|(^POST[0-9])
]
LENGTHS = [0, 1, 15, 16, 17, 31, 32, 33, 1023, 1024, 1025, 32767, 32768, 32769, 300001]
MODES = (dict(), dict(track_positions=False), dict(count_lines=True), dict(case_sensitive=False))
CAPPED = tuple(dict(max_count=mc, **kw) for mc in (0, 1, 5) for kw in (dict(), dict(track_positions=False), dict(count_lines=True)))


@pytest.mark.parametrize("shape", range(len(SHAPES)))
def test_operator_equals_regex_search(gpu, shape):
    pats, alphabet, plants, bol, eol = SHAPES[shape]
    info = gpu.regex_compile_ext(rx(pats))
    assert (info.bol, info.eol, info.alt.n_branches) == (bol, eol, len(plants))
    with pytest.raises(KrepGpuError):
        gpu.regex_compile_alt(rx(pats))  # (the older compilers refuse it: this is the new road)
    rng = np.random.RandomState(2100 + shape)
    a = info.alt
    for n in sorted(set(LENGTHS + [a.Lmin - 1, a.Lmin, a.Lmax - 1, a.Lmax])):
        text = planted(rng, n, alphabet, plants, bol, eol)
        for kw in MODES + (CAPPED if n in (33, 1025, 32769) else ()):
            check(gpu, pats, text, **kw)
        if n >= 1024:
            assert expected(pats, text)[0] > 0  # the planted copies are found
    # max_count == 0 without -c and without positions: 1 as soon as one occurrence exists
    assert gpu.search(rx(pats, max_count=0, track_positions=False), text)[0] == 1


def test_the_end_of_the_text_ends_a_line_in_a_case_sensitive_search_only(gpu):
    """(foo|quux)$ with a copy on the last bytes of texts whose length is a multiple of a lane, a cell, a round and a unit, and not:
    found when case-sensitive, not found under -i; the coordinate text_len is one more cell, round or unit then"""
    pats = [b"(foo|quux)$"]
    rng = np.random.RandomState(45)
    for n in (5, 16, 17, 1024, 1027, 8192, 32768, 32771, 65536):
        for tail in (b"foo", b"quux", b"fo", b"quux\n"):
            text = background(rng, n, b"fqux \n")
            text[n - len(tail):] = np.frombuffer(tail, dtype=np.uint8)
            for kw in (dict(), dict(count_lines=True), dict(track_positions=False)):
                want = check(gpu, pats, text, **kw)
                check(gpu, pats, text, case_sensitive=False, **kw)
            ends = expected(pats, text)[1][:, 1].tolist()
            ends_i = expected(pats, text, case_sensitive=False)[1][:, 1].tolist()
            assert (n in ends) == (tail in (b"foo", b"quux")) and n not in ends_i, (n, tail)
            assert (n - 1 in ends_i) == (tail == b"quux\n")
            # the same through a plan on a device buffer whose pad byte is not a newline
            hold, d_text = to_device(text, 3, pad=ord("\n") if tail == b"fo" else PAD)
            for kw in (dict(), dict(count_lines=True)):
                plan = gpu.plan(rx(pats, **kw))
                try:
                    assert plan.scan(d_text, n).count == expected(pats, text, **kw)[0], (n, tail, kw)
                finally:
                    plan.close()
            del hold


def scan_records(plan, d_text, n, own_lo, own_hi, global_base=0, global_len=0):
    import torch
    cap = 1 << 16
    pos = torch.full((2 * cap,), -1, dtype=torch.int64, device="cuda")
    out = plan.scan(d_text, n, own_lo, own_hi, global_base, pos.data_ptr(), cap, global_len=global_len)
    assert not out.overflow and out.stored == out.count
    return out, pos[:2 * int(out.stored)].cpu().numpy().astype(np.uint64).reshape(-1, 2)


def window_lines(prog, text, lo, hi):
    """line_count, has_newline, head_line_hit, tail_line_hit of include/krep_gpu.h for the window [lo, hi): the starts and the newlines
    the window owns; a start ON a newline belongs to the line that newline ends"""
    occ, _ = em.occurrences(prog, text)
    mine = occ[(occ >= lo) & (occ < hi)]
    nl = np.flatnonzero(text[lo:hi] == 10) + lo
    lines = np.unique(np.searchsorted(nl, mine, side="left")).size
    head = bool(mine.size) and (nl.size == 0 or mine[0] <= nl[0])
    tail = bool(mine.size) and (nl.size == 0 or mine[-1] > nl[-1])
    return int(lines), bool(nl.size), bool(head), bool(tail)


WINDOWS = ((15, 33), (16, 32), (17, 31), (1, 16), (1023, 1025), (1024, 2048), (31, 32769), (32768, 39999), (1, 40000), (0, 40000))


@pytest.mark.parametrize("shift", [0, 3])
def test_windows_own_by_start(gpu, shift):
    """Start ownership between anchors: copies of each sequence start at own_lo - 1 and own_hi - 1, or at own_lo and own_hi, and one ends
    at n; owned is exactly start in [own_lo, own_hi), under -c with the four line facts of the window, and for the sets without an
    overlap with the records and the count-only scan as well"""
    n = 40000
    rng = np.random.RandomState(52 + shift)
    for pats, plants, bol, eol in (([b"^(ERROR|WARN)"], [b"ERROR", b"WARN"], 1, 0), ([b"(x|[a-c]{15})$"], [b"x", b"abcabcabcabcabc"], 0, 1),
                                   ([b"^(a{14}|b{14})$"], [b"a" * 14, b"b" * 14], 1, 1), ([b"colou?r"], [b"color", b"colour"], 0, 0),
                                   ([b"^(a|bc)d?$"], [b"ad", b"bcd"], 1, 1)):
        prog = em.branches(pats)
        records = not gpu.regex_compile_ext(rx(pats)).alt.cross_overlap
        assert records == (pats != [b"^(a|bc)d?$"])
        plan, plan_c = gpu.plan(rx(pats)), gpu.plan(rx(pats, count_lines=True))
        try:
            for own_lo, own_hi in WINDOWS:
                for plant, first in ((plants[0], True), (plants[1], True), (plants[0], False), (plants[1], False)):
                    text = background(rng, n, b"yz \n\n")
                    for s in ((own_lo - 1, own_hi - 1, n - len(plant)) if first else (own_lo, own_hi, n - len(plant))):
                        if s >= (1 if bol else 0):
                            put(text, s, plant, bol, eol)
                    if own_hi - own_lo >= 80:
                        put(text, (own_lo + own_hi) // 2, plants[0] if plant == plants[1] else plants[1], bol, eol)
                    occ, lens = em.occurrences(prog, text)
                    keep = (occ >= own_lo) & (occ < own_hi)
                    mine, mlen = occ[keep], lens[keep]
                    hold, d_text = to_device(text, shift)
                    o_c = plan_c.scan(d_text, n, own_lo, own_hi)
                    have = (int(o_c.line_count), bool(o_c.has_newline), bool(o_c.head_line_hit), bool(o_c.tail_line_hit))
                    assert have == window_lines(prog, text, own_lo, own_hi), (pats, own_lo, own_hi, plant, first)
                    if records:
                        out, rec = scan_records(plan, d_text, n, own_lo, own_hi)
                        assert out.count == mine.size and out.total_matches == mine.size, (pats, shift, own_lo, own_hi, plant, first)
                        assert np.array_equal(rec[:, 0], mine.astype(np.uint64))
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
    rng = np.random.RandomState(61)
    n = 100 * 1024
    cuts = [0, 33333, 65537, n]
    for pats, alphabet, plants, bol, eol in (SHAPES[0], SHAPES[2], SHAPES[4], SHAPES[5], SHAPES[7], SHAPES[8], SHAPES[9], SHAPES[10], SHAPES[6]):
        text = planted(rng, n, alphabet, plants, bol, eol)
        for c in cuts[1:-1]:  # the longest copy across each cut, and one that starts on it
            put(text, c - 5, max(plants, key=len), bol, eol)
            put(text, c + 40, min(plants, key=len), bol, eol)
        hold, d_text = to_device(text)
        whole_lines = expected(pats, text, count_lines=True)
        pieces = gpu.split_mode(rx(pats), n) == abi.SPLIT_PIECES
        assert pieces == (pats != [b"^(a|bc)d?$"])
        plan, plan_c = gpu.plan(rx(pats)), gpu.plan(rx(pats, count_lines=True))
        try:
            recs, outs = [], []
            for lo, hi in zip(cuts[:-1], cuts[1:]):
                if pieces:
                    recs.append(scan_records(plan, d_text, n, lo, hi)[1])
                outs.append(plan_c.scan(d_text, n, lo, hi))
            if pieces:
                whole = expected(pats, text)
                assert np.array_equal(np.concatenate(recs), whole[1]) and sum(len(r) for r in recs) == whole[0], pats
            assert gpu.lib.krep_gpu_combine_line_counts((abi.ScanOut * 3)(*outs), 3) == whole_lines[0], pats
            assert plan_c.scan(d_text, n).line_count == whole_lines[0]
        finally:
            plan.close()
            plan_c.close()
        del hold
    # two occurrences can share a byte: one window only
    pats = [b"[ab]{1,3}c"]
    text = planted(rng, n, b"abc \n", [b"ac", b"bac", b"abbc"])
    hold, d_text = to_device(text)
    plan = gpu.plan(rx(pats))
    try:
        assert gpu.split_mode(rx(pats), n) == abi.SPLIT_WHOLE and gpu.split_mode(rx(pats, count_lines=True), n) == abi.SPLIT_PIECES
        with pytest.raises(KrepGpuError, match="overlap"):
            plan.scan(d_text, n, 4096, 8192)
        out, rec = scan_records(plan, d_text, n, 0, n)
        want = expected(pats, text)
        assert out.count == want[0] and np.array_equal(rec, want[1])
    finally:
        plan.close()
    del hold


def test_windows_that_miss_the_deciding_byte_are_refused(gpu):
    """a buffer that is a slice [1000, 1000 + m) of the text: ^ cannot be decided at buffer byte 0, $ not for an occurrence that ends on
    the buffer's last byte; every window that keeps away from those two is taken and owns what the whole text's list says"""
    rng = np.random.RandomState(51)
    n, base, m = 9000, 1000, 5000
    text = background(rng, n, b"abc \n")
    for s in (base, base + 16, base + 64, base + m - 2, base + m - 3, 2000, 3001, 4007):
        put(text, s, b"ab" if s != base + m - 3 else b"ccb", True, True)
    buf = text[base:base + m]
    assert buf[:2].tobytes() == b"ab" and text[base - 1] == 10 and buf[m - 3:].tobytes() == b"ccb" and text[base + m] == 10
    hold, d_buf = to_device(buf, 7)

    def owned(pats, lo, hi):
        rec = expected(pats, text)[1]
        return rec[(rec[:, 0] >= base + lo) & (rec[:, 0] < base + hi)]

    for pats, bad, good in (([b"^(ab|ccb)"], (0, m), (1, m)), ([b"(ab|ccb)$"], (0, m), (0, m - 3)), ([b"(ab|ccb)$"], (0, m - 2), (0, m - 3)),
                            ([b"^(ab|ccb)$"], (0, m - 3), (1, m - 3)), ([b"^(ab|ccb)$"], (1, m), (1, m - 3))):
        plan, plan_c = gpu.plan(rx(pats)), gpu.plan(rx(pats, count_lines=True))
        try:
            for pl in (plan, plan_c):
                with pytest.raises(KrepGpuError, match=r"regex with [\^$]: the window owns"):
                    pl.scan(d_buf, m, bad[0], bad[1], base, global_len=n)
            out, rec = scan_records(plan, d_buf, m, good[0], good[1], base, n)
            want = owned(pats, *good)
            assert want.shape[0] >= 4 and np.array_equal(rec, want), (pats, good, rec[:4], want[:4])
            assert plan.scan(d_buf, m, good[0], good[1], base, global_len=n).count == want.shape[0]
        finally:
            plan.close()
            plan_c.close()
    # the buffer that begins the text takes ^ at its byte 0, the one that ends it takes $ on its last byte
    text[:2] = np.frombuffer(b"ab", dtype=np.uint8)
    text[2] = 10
    text[n - 3:] = np.frombuffer(b"\nab", dtype=np.uint8)
    pats = [b"^(ab|ccb)$"]
    hold2, d_head = to_device(text[:m], 3)
    hold3, d_tail = to_device(text[n - m:], 5)
    plan = gpu.plan(rx(pats))
    try:
        rec = expected(pats, text)[1]
        _, got = scan_records(plan, d_head, m, 0, m - 3, 0, n)
        assert np.array_equal(got, rec[rec[:, 0] < m - 3]) and got[0, 0] == 0
        _, got = scan_records(plan, d_tail, m, 1, m, n - m, n)
        assert np.array_equal(got, rec[rec[:, 0] >= n - m + 1]) and got[-1, 1] == n
    finally:
        plan.close()
    del hold, hold2, hold3


def test_host_operators_shards_and_streamed_pieces(gpu):
    rng = np.random.RandomState(81)
    n = 3 * (1 << 20) + 77
    share = (n + 2) // 3
    jobs = ((SHAPES[0], dict(), True), (SHAPES[4], dict(), True), (SHAPES[5], dict(max_count=3), True), (SHAPES[7], dict(), True),
            (SHAPES[8], dict(count_lines=True), True), (SHAPES[10], dict(case_sensitive=False), True), (SHAPES[3], dict(), False),
            (SHAPES[3], dict(count_lines=True), True), (SHAPES[6], dict(), False))
    for (pats, alphabet, plants, bol, eol), kw, pieces in jobs:
        text = planted(rng, n, alphabet, plants, bol, eol)
        # copies that start 1 and 3 bytes in front of the two cuts of three shards, on a cut, and one inside each of two shards
        for k, s in enumerate((share - 1, 2 * share - 3, share + 100, 2 * share + 64, share, 2 * share - len(plants[0]))):
            put(text, s, plants[k % len(plants)], bol, eol)
        want = expected(pats, text, **kw)
        assert want[0] >= 3
        p = rx(pats, **kw)
        assert gpu.can_accelerate(p) and gpu.select(p) is not None
        got = gpu.search(p, text)
        assert gpu.last_status() == abi.STATUS_OK
        assert got[0] == want[0] and np.array_equal(got[1], want[1]), (pats, kw, got[0], want[0])
        rc, cnt, pos = gpu.search_buffer(p, text, num_gpus=3)
        assert rc == 0 and gpu.last_status() == abi.STATUS_OK
        assert cnt == want[0] and np.array_equal(pos, want[1]), (pats, kw, cnt, want[0])
        assert (gpu.split_mode(p, n) == abi.SPLIT_PIECES) == pieces and gpu.last_shard_info().shards == (3 if pieces else 1), (pats, kw)
    # streamed: 4096-byte pieces whose boundaries carry a newline in front of, and behind, a copy
    m = 10 * 4096 + 123
    gpu.set_stream_chunk(4096)
    try:
        for (pats, alphabet, plants, bol, eol), kw in ((SHAPES[0], dict()), (SHAPES[4], dict()), (SHAPES[5], dict()), (SHAPES[5], dict(case_sensitive=False)),
                                                       (SHAPES[7], dict()), (SHAPES[8], dict(count_lines=True)), (SHAPES[9], dict(count_lines=True)),
                                                       (SHAPES[10], dict())):
            small = planted(rng, m, alphabet, plants, bol, eol)
            for k, c in enumerate(range(4096, m, 4096)):
                put(small, c - (k % 3) * (len(plants[k % len(plants)]) // 2), plants[k % len(plants)], bol, eol)
            want = expected(pats, small, **kw)
            assert want[0] >= 8
            rc, cnt, pos = gpu.search_buffer(rx(pats, **kw), small)
            assert rc == 0 and gpu.last_status() == abi.STATUS_OK and cnt == want[0] and np.array_equal(pos, want[1]), (pats, kw, cnt, want[0])
    finally:
        gpu.set_stream_chunk(0)


def test_starved_grid_a_wave_takes_several_units(gpu):
    """1 and 2 workgroups on 14 units (416 KiB, krep_gpu_debug_force_regex_grid): a wave rebuilds its entry state and its spill for every
    unit it takes and reads that unit's record offset; only the unit at coordinate 0 starts from the newline in front of the text, and
    the newline behind the text is one more unit when the length is a multiple of one"""
    n = 13 * UNIT
    rng = np.random.RandomState(71)
    jobs = []
    for k in (0, 3, 4, 5, 7, 8, 6):
        pats, alphabet, plants, bol, eol = SHAPES[k]
        text = planted(rng, n, alphabet, plants, bol, eol)
        for j, s in enumerate(range(701, n - 20, 701)):
            put(text, s, plants[j % len(plants)], bol, eol)
        for b in range(UNIT, n, UNIT):  # the longest copy across every unit boundary, a newline-anchored one directly on it
            put(text, b - len(max(plants, key=len)) // 2, max(plants, key=len), bol, eol)
            put(text, b + 100 * UNIT // 1000, plants[0], bol, eol)
        put(text, n - len(plants[0]), plants[0], bol, eol)
        jobs += [(pats, text, kw) for kw in (dict(track_positions=False), dict(), dict(count_lines=True))]
    wants = [expected(pats, text, **kw) for pats, text, kw in jobs]
    assert all(w[0] > 13 for w in wants)
    try:
        for blocks in (1, 2):
            gpu.force_regex_grid(blocks)
            for (pats, text, kw), want in zip(jobs, wants):
                got = gpu.search(rx(pats, **kw), text)
                assert gpu.last_status() == abi.STATUS_OK
                assert got[0] == want[0] and np.array_equal(got[1], want[1]), (blocks, pats, kw, got[0], want[0])
    finally:
        gpu.force_regex_grid(0)


def test_an_unbounded_repetition_still_takes_the_failure_road(gpu):
    text = np.frombuffer(b"abcbc abc\n" * 100, dtype=np.uint8)
    for pats in ([b"a(b|c)*"], [b"colou*r"], [b"^a|b"]):
        assert not gpu.can_accelerate(rx(pats)) and gpu.select(rx(pats)) is None
        with pytest.raises(KrepGpuError, match="kept on krep's regex_search"):
            gpu.search(rx(pats), text)
        assert gpu.last_status() == abi.STATUS_FAILED
