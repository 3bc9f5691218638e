"""krep -E with line anchors on the device (kg_regex.hip) against the reference's regex_search: the compiled reference (oracle/_ref,
through tests/regex_ref.py) answers every case; the rule of tests/regex_anchor_model.py must agree with it each time."""
import numpy as np
import pytest

import line_model as lm
import only_matching_model as om
import regex_anchor_model as am
import regex_model
import regex_ref
from krep_amd import abi
from krep_amd.engine import KrepGpuError

pytestmark = pytest.mark.gpu

PAD = 0xEE
LANE, CELL, ROUND, UNIT = 16, 1024, 8192, 32768


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
    e.set_stream_chunk(0)
    e.force_regex_grid(0)


def expected(pat, text, **kw):
    """what regex_search returns: the compiled reference answers every case; the model must agree with it, so a fault in either shows"""
    assert regex_ref.available(), "the compiled reference (oracle/_ref/libkrep_ref_avx2.so) is missing"
    ref = regex_ref.call(pat, text, **kw)
    want = am.run(pat, text, **kw)
    assert ref[0] == want[0] and np.array_equal(ref[1], want[1]), ("model != reference", pat, kw, text.size)
    return ref


def to_device(a, shift=0):
    import torch
    t = torch.full((a.size + shift + 64,), PAD, dtype=torch.uint8, device="cuda")
    if a.size:
        t[shift:shift + a.size] = torch.from_numpy(a.copy())
    return t, t.data_ptr() + shift


def background(rng, n, alphabet):
    al = np.frombuffer(alphabet, dtype=np.uint8)
    return al[rng.randint(0, al.size, size=n)].copy()


def put(t, s, p, before=None, behind=None):
    """copy p to t[s:], the byte in front of it := before, the byte behind it := behind (None: left alone); nothing out of range"""
    if s < 0 or s + len(p) > t.size:
        return
    t[s:s + len(p)] = p
    if before is not None and s >= 1:
        t[s - 1] = before
    if behind is not None and s + len(p) < t.size:
        t[s + len(p)] = behind


STARTS, ENDS = (LANE, CELL, ROUND, UNIT), (3 * LANE, 2 * CELL, 2 * ROUND, 2 * UNIT)


def planted(rng, n, alphabet, plant, filler, starts=STARTS, ends=ENDS, at_one=False):
    """A text over `alphabet` with copies of `plant` between two newlines: at offset 0 with nothing in front (at_one: at offset 1,
    the newline is byte 0), ending on the last byte with nothing behind; for every B of `starts` (a lane, a cell, a round, a unit
    boundary) the newline in front is the last byte before B and the copy opens what B starts; for every B of `ends` the copy ends
    at B and the newline behind it opens what B starts.  Decoys around every B: the same bytes with `filler` (no newline) on both
    sides or on one."""
    t = background(rng, n, alphabet)
    p = np.frombuffer(plant, dtype=np.uint8)
    L = len(p)
    for B in starts + ends:
        put(t, B + 5 * LANE, p, filler, filler)       # decoys
        put(t, B - 7 * LANE, p, filler, filler)
        put(t, B - 3 * LANE - L, p, 10, filler)       # half decoys: one newline only
        put(t, B + 2 * LANE, p, filler, 10)
        put(t, B + 3 * LANE, p, 10, 10)               # a copy in the middle of a cell
    put(t, 5 + L, p, filler, filler)
    for B in starts:
        put(t, B, p, 10, 10)
    for B in ends:
        put(t, B - L, p, 10, 10)
    put(t, 1, p, 10, 10) if at_one else put(t, 0, p, None, 10)
    put(t, n - L, p, 10, None)
    return t


# (pattern, alphabet of the text, a string that matches the class sequence, a byte that is no newline)
def _shapes():
    words = b"abcdefghijklmnopqrstuvwxyz \n"
    cores = [(b"a", b"ab \n", b"a", b"b"),                                          # L = 1
             (b"a[bc]", b"abc \n", b"ac", b" "),
             (b"Sherl[oO]ck", words, b"SherlOck", b" "),                            # the anchor path
             (b"[A-Z][a-z]{7}", words, b"Sherlock", b" "),                          # the table path
             (b"[ab]{3}", b"ab\n", b"aba", b"b"),                                   # the anchors stop its self-overlap
             (b"[a\n]{2}", b"ab\n ", b"aa", b"b"),                                  # overlaps itself even so: the greedy pass
             (b"[[:space:]]a", b"ab\n \t", b" a", b"b"),
             (b".[^a]", b"ab\x00\xe9\n\x80", b"b\x00", b"\x80")]                    # NUL and bytes >= 0x80 in the text
    out = []
    for core, al, plant, fill in cores:
        out += [(b"^" + core, al, plant, fill), (core + b"$", al, plant, fill), (b"^" + core + b"$", al, plant, fill)]
    a = (b"ab \n", b"a" * 15, b"b")
    return out + [(b"^a{15}",) + a, (b"a{15}$",) + a, (b"^a{14}$", a[0], b"a" * 14, a[2])]   # Lx = 16


SHAPES = _shapes()
LENGTHS = [0, 1, 15, 16, 17, 1023, 1024, 1025, 8191, 8192, 8193, 32767, 32768, 32769, 65536, 300001]
MODES = (dict(), dict(track_positions=False), dict(count_lines=True), dict(case_sensitive=False))
MAX_COUNTS = tuple(dict(max_count=mc, **kw) for mc in (0, 1, 5) for kw in (dict(), dict(track_positions=False), dict(count_lines=True)))


@pytest.mark.parametrize("shape", range(len(SHAPES)), ids=[s[0].decode().replace("\n", "\\n") for s in SHAPES])
def test_operator_equals_regex_search(gpu, shape):
    pat, alphabet, plant, fill = SHAPES[shape]
    info = gpu.regex_compile_anchored(regex_ref.params(pat))
    L = info.seq.L
    assert (info.bol, info.eol) == (int(pat.startswith(b"^")), int(pat.endswith(b"$"))) and L == len(plant)
    if b"[ab]{3}" in pat:
        assert info.seq.self_overlap == 0 and gpu.regex_compile(regex_ref.params(b"[ab]{3}")).self_overlap == 1
    if b"[a\n]{2}" in pat:
        assert info.seq.self_overlap == 1
    rng = np.random.RandomState(1900 + shape)
    for n in sorted(set(LENGTHS + [L - 1, L])):
        # (odd lengths: the boundaries change their parts, and the first copy stands at offset 1)
        text = planted(rng, n, alphabet, plant, fill[0], *((ENDS, STARTS, True) if n & 1 else (STARTS, ENDS, False)))
        for kw in MODES + (MAX_COUNTS if n in (L, 17, 1025, 32768, 65536) else ()):
            want = expected(pat, text, **kw)
            got = gpu.search(regex_ref.params(pat, **kw), text)
            assert gpu.last_status() == abi.STATUS_OK
            assert got[0] == want[0], (pat, n, kw, got[0], want[0])
            assert np.array_equal(got[1], want[1]), (pat, n, kw, got[1][:6], want[1][:6])
        if n >= 1024:
            # the planted copies are found, the decoys are not: more occurrences of the bare sequence than of the anchored one
            found = expected(pat, text)
            bare = regex_ref.call(am.split(pat)[1], text, track_positions=False)[0]
            assert 0 < found[0] < bare, (pat, n, found[0], bare)
            starts = set(found[1][:, 0].tolist())
            assert ((n & 1) in starts or not info.bol or info.seq.self_overlap) and (n - L in starts or not info.eol or info.seq.self_overlap)


def test_a_text_without_any_newline(gpu):
    """the two newlines no buffer holds: the one in front of byte 0 and the one behind the last byte (no rounds, cells or units of
    real newlines help); under -i the end of the text ends no line (REG_ICASE is REG_NOTEOL in regexec's eflags, krep.c:1420)"""
    for n in (16, 1024, 8192, 32768, 65536):
        text = np.full(n, ord("c"), dtype=np.uint8)
        text[0], text[n - 1] = ord("a"), ord("b")
        if n >= 64:
            text[n // 2], text[n // 2 + 1] = ord("a"), ord("b")  # decoys: no line starts or ends here
        for pat in (b"^a", b"b$", b"^ac{14}", b"c{14}b$"):
            for kw in (dict(), dict(track_positions=False), dict(count_lines=True), dict(case_sensitive=False)):
                want = expected(pat, text, **kw)
                got = gpu.search(regex_ref.params(pat, **kw), text)
                assert got[0] == want[0] and np.array_equal(got[1], want[1]), (pat, n, kw, got[0], want[0])
            assert expected(pat, text)[0] == 1 and expected(pat, text, case_sensitive=False)[0] == (0 if pat.endswith(b"$") else 1)


def scan_records(plan, d_text, n, own_lo, own_hi, global_base=0, global_len=0):
    import torch
    cap = 1 << 16
    pos = torch.full((2 * cap,), -1, dtype=torch.int64, device="cuda")
    out = plan.scan(d_text, n, own_lo, own_hi, global_base, pos.data_ptr(), cap, global_len=global_len)
    assert not out.overflow and out.stored == out.count
    return out, pos[:2 * int(out.stored)].cpu().numpy().astype(np.uint64).reshape(-1, 2)


def test_three_windows_of_an_unaligned_text(gpu):
    """window boundaries directly behind a newline (the next window's first owned byte starts a line whose newline it does not own),
    directly in front of one (the $ of the last owned start reads a byte the window does not own) and inside a match"""
    n = 3 * UNIT + 999
    words = b"abcdefghijklmnopqrstuvwxyz \n"
    for shift, pat in ((1, b"^Sherl[oO]ck"), (7, b"Sherl[oO]ck$"), (15, b"^[A-Z][a-z]{7}$"), (7, b"^[a-z]{4}")):
        rng = np.random.RandomState(40 + shift)
        sites = (UNIT, UNIT + 333, 2 * UNIT - 8, 2 * UNIT + 4096 + 5)
        text = planted(rng, n, words, b"Sherlock", ord(" "), starts=STARTS[:3] + sites)
        for s in sites:
            assert text[s - 1] == 10 and text[s + 8] == 10 and text[s:s + 8].tobytes() == b"Sherlock"
        hold, d_text = to_device(text, shift)
        whole, whole_lines = expected(pat, text), expected(pat, text, count_lines=True)
        assert whole[0] > 20
        plan, plan_c = gpu.plan(regex_ref.params(pat)), gpu.plan(regex_ref.params(pat, count_lines=True))
        try:
            for a, b in ((0, 1), (1, 2), (2, 3), (3, 0)):
                kinds = [lambda s: s, lambda s: s + 8, lambda s: s + 3, lambda s: s - 1]  # behind a newline, in front of one, inside, ON one
                cuts = [0] + sorted([kinds[a](sites[a]), kinds[b](sites[b])]) + [n]
                recs, outs = [], []
                for lo, hi in zip(cuts[:-1], cuts[1:]):
                    out, rec = scan_records(plan, d_text, n, lo, hi)
                    assert ((rec[:, 0] >= lo) & (rec[:, 0] < hi)).all()
                    recs.append(rec)
                    outs.append(plan_c.scan(d_text, n, lo, hi))
                assert np.array_equal(np.concatenate(recs), whole[1]), (pat, cuts)
                assert gpu.lib.krep_gpu_combine_line_counts((abi.ScanOut * 3)(*outs), 3) == whole_lines[0], (pat, cuts)
            assert plan_c.scan(d_text, n).line_count == whole_lines[0]
        finally:
            plan.close()
            plan_c.close()
        del hold


def test_windows_that_miss_the_deciding_byte_are_refused(gpu):
    """a buffer that is a slice [1000, 1000 + m) of the text: ^ cannot be decided at buffer byte 0, $ not for the occurrence that ends on
    the buffer's last byte; every window that keeps away from those two is taken and owns what the whole text's list says"""
    rng = np.random.RandomState(50)
    n, base, m = 9000, 1000, 5000
    text = planted(rng, n, b"ab\n", b"ab", ord("b"), starts=(base, base + 16), ends=(base + 64, base + m))
    buf = text[base:base + m]
    assert buf[:2].tobytes() == b"ab" and text[base - 1] == 10 and buf[m - 2:].tobytes() == b"ab" and text[base + m] == 10
    hold, d_buf = to_device(buf, 7)

    def owned(pat, lo, hi):
        rec = expected(pat, text)[1]
        return rec[(rec[:, 0] >= base + lo) & (rec[:, 0] < base + hi)]

    for pat, bad, good in ((b"^ab", (0, m), (1, m)), (b"ab$", (0, m), (0, m - 2)), (b"^ab$", (0, m - 2), (1, m - 2)), (b"^ab$", (1, m), (1, m - 2))):
        plan, plan_c = gpu.plan(regex_ref.params(pat)), gpu.plan(regex_ref.params(pat, count_lines=True))
        try:
            for pl in (plan, plan_c):
                with pytest.raises(KrepGpuError, match=r"regex with [\^$]: the window owns"):
                    pl.scan(d_buf, m, bad[0], bad[1], base, global_len=n)
            out, rec = scan_records(plan, d_buf, m, good[0], good[1], base, n)
            want = owned(pat, *good)
            assert want.shape[0] > 10 and np.array_equal(rec, want), (pat, good, rec[:4], want[:4])
            assert plan.scan(d_buf, m, good[0], good[1], base, global_len=n).count == want.shape[0]
        finally:
            plan.close()
            plan_c.close()
    # the buffer that begins the text takes ^ at its byte 0, the one that ends it takes $ on its last byte
    hold2, d_head = to_device(text[:m], 3)
    plan = gpu.plan(regex_ref.params(b"^ab$"))
    try:
        rec = expected(b"^ab$", text)[1]
        _, got = scan_records(plan, d_head, m, 0, m - 2, 0, n)
        assert np.array_equal(got, rec[rec[:, 0] < m - 2]) and got[0, 0] == 0
        hold3, d_tail = to_device(text[n - m:], 5)
        _, got = scan_records(plan, d_tail, m, 1, m, n - m, n)
        assert np.array_equal(got, rec[rec[:, 0] >= n - m + 1]) and got[-1, 1] == n
    finally:
        plan.close()
    del hold, hold2, hold3


def test_host_operators_shards_and_streamed_pieces(gpu):
    rng = np.random.RandomState(60)
    n = 3 * (1 << 20) + 77
    share = (n + 2) // 3
    words = b"abcdefghijklmnopqrstuvwxyz \n"
    text = planted(rng, n, words, b"Sherlock", ord(" "), starts=(LANE, CELL, UNIT, share, 1 << 20), ends=(2 * CELL, 2 * UNIT, 2 * share, 2 << 20))
    long14 = np.frombuffer(b"a" + b"b" * 12 + b"c", dtype=np.uint8)  # ^ab{12}c$: Lx = 16, the copies stand on the two shard cuts
    for s in (share - 1, 2 * share - 13, share + 100):
        put(text, s, long14, 10, 10)
    jobs = ((b"^Sherl[oO]ck", dict()), (b"[A-Z][a-z]{7}$", dict(max_count=3)), (b"^[a-z]{4}", dict(count_lines=True)),
            (b"^[A-Z][a-z]{7}$", dict()), (b"^ab{12}c$", dict()), (b"^[a\n]{2}", dict()), (b"[x-z]{2}$", dict(count_lines=True)))
    for pat, kw in jobs:
        want = expected(pat, text, **kw)
        assert want[0] >= 3
        p = regex_ref.params(pat, **kw)
        assert gpu.can_accelerate(p) and gpu.select(p) is not None
        got = gpu.search(p, text)
        assert gpu.last_status() == abi.STATUS_OK and got[0] == want[0] and np.array_equal(got[1], want[1]), (pat, kw, got[0], want[0])
        rc, cnt, pos = gpu.search_buffer(p, text, num_gpus=3)
        assert rc == 0 and gpu.last_status() == abi.STATUS_OK
        assert cnt == want[0] and np.array_equal(pos, want[1]), (pat, kw, cnt, want[0])
        pieces = gpu.split_mode(p, text.size) == abi.SPLIT_PIECES
        assert pieces == (pat != b"^[a\n]{2}") and gpu.last_shard_info().shards == (3 if pieces else 1)
    # streamed: 4096-byte pieces whose boundaries carry a newline in front of, and behind, a copy
    m = 10 * 4096 + 123
    cuts = tuple(range(4096, m, 4096))
    small = planted(rng, m, words, b"Sherlock", ord(" "), starts=cuts[0::2], ends=cuts[1::2])
    gpu.set_stream_chunk(4096)
    try:
        for pat, kw in ((b"^Sherl[oO]ck", dict()), (b"Sherl[oO]ck$", dict()), (b"^[A-Z][a-z]{7}$", dict()), (b"^[a-z]{4}", dict(count_lines=True)),
                        (b"[a-z]{4}$", dict(count_lines=True)), (b"Sherl[oO]ck$", dict(case_sensitive=False))):
            want = expected(pat, small, **kw)
            assert want[0] >= 2 * len(cuts)
            rc, cnt, pos = gpu.search_buffer(regex_ref.params(pat, **kw), small)
            assert rc == 0 and gpu.last_status() == abi.STATUS_OK and cnt == want[0] and np.array_equal(pos, want[1]), (pat, kw, cnt, want[0])
    finally:
        gpu.set_stream_chunk(0)


def test_starved_grid_with_anchors(gpu):
    """one workgroup on 14 units (~416 KiB): every wave takes several units, resets its state for each and reads the unit's record
    offset; only the unit at coordinate 0 starts from the newline in front of the text"""
    n = 13 * UNIT + 100
    rng = np.random.RandomState(70)
    words = b"abcdefghijklmnopqrstuvwxyz \n"
    text = planted(rng, n, words, b"Sherlock", ord(" "), starts=tuple(range(UNIT, n, 2 * UNIT)) + STARTS[:3], ends=tuple(range(2 * UNIT, n, 2 * UNIT)) + ENDS[:3])
    exact = planted(rng, 13 * UNIT, words, b"Sherlock", ord(" "), starts=(UNIT, 11 * UNIT), ends=(2 * UNIT, 12 * UNIT))  # $ at the end of the last unit
    jobs = [(b"^Sherl[oO]ck", text, dict()), (b"Sherl[oO]ck$", text, dict(track_positions=False)), (b"^[A-Z][a-z]{7}$", text, dict()),
            (b"^[a-z]{4}", text, dict(count_lines=True)), (b"^[a\n]{2}", text, dict()), (b"[A-Z][a-z]{7}$", exact, dict()),
            (b"Sherl[oO]ck$", exact, dict()), (b"[a-z]{4}$", exact, dict(count_lines=True))]
    wants = [expected(pat, t, **kw) for pat, t, kw in jobs]
    assert all(w[0] > 13 for w in wants)
    assert all(w[1][-1, 1] == 13 * UNIT for (_, t, kw), w in zip(jobs, wants) if t is exact and not kw)
    try:
        gpu.force_regex_grid(1)
        for (pat, t, kw), want in zip(jobs, wants):
            got = gpu.search(regex_ref.params(pat, **kw), t)
            assert gpu.last_status() == abi.STATUS_OK
            assert got[0] == want[0] and np.array_equal(got[1], want[1]), (pat, kw, got[0], want[0])
    finally:
        gpu.force_regex_grid(0)


def test_grep_output_of_an_anchored_plan(gpu):
    rng = np.random.RandomState(80)
    text = planted(rng, 70001, b"abcdefghij \n", b"abcd", ord(" "))
    hold, d_text = to_device(text)
    tb = text.tobytes()
    for pat, mc in ((b"^ab[a-d]d", None), (b"^[a-c]{3}", None), (b"^j[ a]", 7), (b"^abcd$", None), (b"^[a\n]{2}", None)):
        want = expected(pat, text)
        assert want[0] > 10
        kw = {} if mc is None else dict(max_count=mc)
        plan = gpu.plan(regex_ref.params(pat, **kw))
        try:
            assert plan.grep_lines(d_text, text.size, filename=b"f.txt") == lm.grep_output(tb, want[1], b"f.txt:", mc), (pat, mc)
        finally:
            plan.close()
        plan = gpu.plan(regex_ref.params(pat, **kw), only_matching=True)  # (-o changes nothing for regex_search: the same records)
        try:
            assert plan.grep_only_matching(d_text, text.size, filename=b"f.txt") == om.grep_o_output(tb, want[1], b"f.txt", False, mc), (pat, mc)
        finally:
            plan.close()
    del hold
