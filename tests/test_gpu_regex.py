"""krep -E on the device (kg_regex.hip) against the reference's regex_search: the compiled reference (oracle/_ref, through
tests/regex_ref.py) answers every case; the rule of tests/regex_model.py must agree with it each time."""
import ctypes as C

import numpy as np
import pytest

import line_model as lm
import regex_model
import regex_ref
from krep_amd import abi
from krep_amd.engine import KrepGpuError

pytestmark = pytest.mark.gpu

PAD = 0xEE


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


def expected(pat, text, **kw):
    """what regex_search returns: the compiled reference answers every case (there is no restatement for regex); the model must
    agree with it, so a fault in either shows"""
    assert regex_ref.available(), "the compiled reference (oracle/_ref/libkrep_ref_avx2.so) is missing"
    ref = regex_ref.call(pat, text, **kw)
    want = regex_model.run(pat, text, **kw)
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


def planted(rng, n, alphabet, plant, L):
    """a text over `alphabet` with `plant` put so that one copy straddles the 16-byte lane boundary, the 1-KiB cell, the 32-KiB
    unit and ends on the last byte of the text (wherever the text is long enough)"""
    t = background(rng, n, alphabet)
    p = np.frombuffer(plant, dtype=np.uint8)
    spots = [b - k for b in (16, 1024, 32768, 65536) for k in {1, max(1, len(p) - 1), max(1, len(p) // 2)}] + [n - len(p), 0, 40, 5000]
    for s in spots:
        if 0 <= s and s + len(p) <= n:
            t[s:s + len(p)] = p
    return t


# (pattern, alphabet of the text, a string that matches it)
SHAPES = [
    (b"a", b"ab \n", b"a"),                                         # L = 1
    (b"a[bc]", b"abc \n", b"ac"),                                   # L = 2
    (b"Sherl[oO]ck", b"abcdefghijklmnopqrstuvwxyz \n", b"SherlOck"),  # L = 8, literal atoms: the anchor path
    (b"[A-Z][a-z]{7}", b"abcdefghijklmnopqrstuvwxyz \n", b"Sherlock"),  # L = 8, no small class: the table path
    (b"0x[0-9a-f]{8}[g-k]{6}", b"0x19afgk \n", b"0x0123abcdghijkg"),  # L = 16
    (b"[ab]{3}", b"ab", b"aba"),                                    # dense, overlaps itself: the greedy pass
    (b"[a\n]b", b"ab\n ", b"\nb"),                                  # a class that holds '\n'
    (b"[[:space:]]a", b"ab\n \t", b"\na"),
    (b".[^a]", b"ab\x00\xe9\n\x80", b"b\x00"),                      # NUL and bytes >= 0x80 in the text
    (b"[^a]", b"a\x00\xe9\n", b"\x00"),
]
LENGTHS = [0, 1, 15, 16, 17, 31, 32, 33, 1023, 1024, 1025, 32767, 32768, 32769, 300001]


@pytest.mark.parametrize("shape", range(len(SHAPES)))
def test_operator_equals_regex_search(gpu, shape):
    pat, alphabet, plant = SHAPES[shape]
    L = gpu.regex_compile(regex_ref.params(pat)).L
    rng = np.random.RandomState(900 + shape)
    for n in sorted(set(LENGTHS + [L - 1, L])):
        text = planted(rng, n, alphabet, plant, L)
        for kw in (dict(), dict(track_positions=False), dict(count_lines=True), dict(case_sensitive=False)):
            want = expected(pat, text, **kw)
            got = gpu.search(regex_ref.params(pat, **kw), text)
            assert gpu.last_status() == abi.STATUS_OK
            assert got[0] == want[0], (pat, n, kw, got[0], want[0])
            assert np.array_equal(got[1], want[1]), (pat, n, kw, got[1][:6], want[1][:6])
        if n >= 1024:
            assert expected(pat, text)[0] > 0  # the planted copies are found


def test_runs_of_one_byte(gpu):
    """a text of only `a`s: every position is an occurrence, the matches are every L-th one"""
    for n in (1, 2, 3, 16, 17, 1025, 32769, 100000):
        text = np.full(n, ord("a"), dtype=np.uint8)
        for pat in (b"a{2}", b"a{3}", b"[ab]{3}"):
            for kw in (dict(), dict(track_positions=False), dict(max_count=5), dict(count_lines=True)):
                want = expected(pat, text, **kw)
                got = gpu.search(regex_ref.params(pat, **kw), text)
                assert got[0] == want[0] and np.array_equal(got[1], want[1]), (pat, n, kw, got[0], want[0])


def test_max_count_and_its_zero_quirk(gpu):
    rng = np.random.RandomState(77)
    text = planted(rng, 70000, b"abcdefghijklmnopqrstuvwxyz \n", b"SherlOck", 8)
    none = np.full(5000, ord("z"), dtype=np.uint8)
    for pat in (b"Sherl[oO]ck", b"[a-z]{4}", b"[ab]{2}"):
        for mc in (0, 1, 5):
            for kw in (dict(), dict(track_positions=False), dict(count_lines=True), dict(count_lines=True, track_positions=True)):
                for t in (text, none):
                    want = expected(pat, t, max_count=mc, **kw)
                    got = gpu.search(regex_ref.params(pat, max_count=mc, **kw), t)
                    assert got[0] == want[0] and np.array_equal(got[1], want[1]), (pat, mc, kw, got[0], want[0])
    # max_count == 0 without -c and without positions: 1 as soon as one occurrence exists (krep.c:1395, :1533)
    assert gpu.search(regex_ref.params(b"Sherl[oO]ck", max_count=0, track_positions=False), text)[0] == 1


def scan_records(plan, d_text, n, own_lo, own_hi, global_base=0, global_len=0):
    import torch
    cap = 1 << 16
    pos = torch.full((2 * cap,), -1, dtype=torch.int64, device="cuda")
    out = plan.scan(d_text, n, own_lo, own_hi, global_base, pos.data_ptr(), cap, global_len=global_len)
    assert not out.overflow and out.stored == out.count
    return out, pos[:2 * int(out.stored)].cpu().numpy().astype(np.uint64).reshape(-1, 2)


def test_windows_and_unaligned_text(gpu):
    """start ownership: a match that starts at own_hi - 1 is owned, one at own_lo - 1 is not; own_lo / own_hi on and around 16-byte
    boundaries; d_text at an odd offset into its allocation"""
    L, n = 8, 40000
    p = np.frombuffer(b"Sherlock", dtype=np.uint8)
    # the anchor path and the table path (no class of at most 4 bytes): both walk the same windows
    for pat, shift in ((b"Sherl[oO]ck", 0), (b"Sherl[oO]ck", 3), (b"[A-Z][a-z]{7}", 0), (b"[A-Z][a-z]{7}", 3)):
        rng = np.random.RandomState(5 + shift)
        assert gpu.regex_compile(regex_ref.params(pat)).n_anchor == (1 if pat.startswith(b"S") else 0)
        for own_lo, own_hi in ((15, 33), (16, 32), (17, 31), (1, 16), (1023, 1025), (1024, 2048), (31, 32769), (32768, 39999), (0, n)):
            for spots in ((own_lo - 1, own_hi - 1, n - L), (own_lo, own_hi, own_lo + 20)):
                text = background(rng, n, b"abcdefghijklmnopqrstuvwxyz \n")
                for s in spots:
                    if 0 <= s and s + L <= n:
                        text[s:s + L] = p
                hold, d_text = to_device(text, shift)
                # (under -i [A-Z] holds the lower-case letters too: that pattern overlaps itself and takes no inner window)
                for kw in ((dict(), dict(case_sensitive=False)) if pat.startswith(b"S") else (dict(),)):
                    occ = regex_model.occurrences(regex_model.classes(pat, **kw), text)
                    mine = occ[(occ >= own_lo) & (occ < own_hi)]
                    if spots[0] == own_lo - 1 and own_hi - own_lo >= L and own_lo >= 1 and own_hi - 1 + L <= n:
                        assert own_hi - 1 in mine and own_lo - 1 not in mine
                    plan = gpu.plan(regex_ref.params(pat, **kw))
                    try:
                        out, rec = scan_records(plan, d_text, n, own_lo, own_hi, global_base=1000, global_len=1000 + n)
                        assert out.count == mine.size and out.total_matches == mine.size, (shift, own_lo, own_hi, spots, kw)
                        assert np.array_equal(rec[:, 0], mine.astype(np.uint64) + 1000) and np.array_equal(rec[:, 1], rec[:, 0] + L)
                        assert plan.scan(d_text, n, own_lo, own_hi).count == mine.size  # count only
                    finally:
                        plan.close()
                del hold


def test_three_windows_concatenate_and_combine(gpu):
    rng = np.random.RandomState(6)
    n = 100 * 1024
    text = planted(rng, n, b"abcdefghij \n\n", b"j\nab", 4)
    hold, d_text = to_device(text)
    cuts = [0, 33333, 65537, n]
    for pat in (b"j[[:space:]]ab", b"[a-c]{2}[ \n]", b"[\n]"):
        whole = expected(pat, text)
        whole_lines = expected(pat, text, count_lines=True)
        plan, plan_c = gpu.plan(regex_ref.params(pat)), gpu.plan(regex_ref.params(pat, count_lines=True))
        try:
            recs, outs = [], []
            for lo, hi in zip(cuts[:-1], cuts[1:]):
                out, rec = scan_records(plan, d_text, n, lo, hi)
                recs.append(rec)
                outs.append(plan_c.scan(d_text, n, lo, hi))
            assert np.array_equal(np.concatenate(recs), whole[1]) and sum(len(r) for r in recs) == whole[0]
            arr = (abi.ScanOut * 3)(*outs)
            assert gpu.lib.krep_gpu_combine_line_counts(arr, 3) == whole_lines[0], pat
            assert plan_c.scan(d_text, n).line_count == whole_lines[0]
        finally:
            plan.close()
            plan_c.close()
    # a pattern that can overlap itself: one window only
    plan = gpu.plan(regex_ref.params(b"[ab]{3}"))
    try:
        assert gpu.split_mode(regex_ref.params(b"[ab]{3}"), n) == abi.SPLIT_WHOLE
        with pytest.raises(KrepGpuError, match="overlap"):
            plan.scan(d_text, n, 4096, 8192)
        assert plan.scan(d_text, n).count == expected(b"[ab]{3}", text)[0]
    finally:
        plan.close()
    del hold


def test_host_operators_and_shards(gpu):
    rng = np.random.RandomState(8)
    text = planted(rng, 3 * (1 << 20) + 77, b"abcdefghijklmnopqrstuvwxyz \n", b"Sherlock", 8)
    # `ab{14}c` is 8 pattern bytes and 16 text bytes: a shard's halo has to follow L, not the pattern's length.  Copies that start
    # 1 and 3 bytes in front of the two cuts of three shards (they end 15 and 13 bytes behind them), and one inside each of two shards
    share = (text.size + 2) // 3
    long16 = np.frombuffer(b"a" + b"b" * 14 + b"c", dtype=np.uint8)
    for s in (share - 1, 2 * share - 3, share + 100, 2 * share + 64):
        text[s:s + 16] = long16
    assert gpu.regex_compile(regex_ref.params(b"ab{14}c")).L == 16
    for pat, kw in ((b"Sherl[oO]ck", dict()), (b"[A-Z][a-z]{7}", dict(max_count=3)), (b"[a-z]{4}", dict(count_lines=True)),
                    (b"[ab]{2}", dict()), (b"[x-z]{2}\n", dict(count_lines=True)), (b"q{16}", dict()), (b"ab{14}c", dict())):
        want = expected(pat, text, **kw)
        p = regex_ref.params(pat, **kw)
        assert gpu.can_accelerate(p) and gpu.select(p) is not None
        got = gpu.search(p, text)
        assert got[0] == want[0] and np.array_equal(got[1], want[1]), (pat, kw, got[0], want[0])
        rc, cnt, pos = gpu.search_buffer(p, text, num_gpus=3)
        assert rc == (0 if want[0] else 1) and gpu.last_status() == abi.STATUS_OK
        assert cnt == want[0] and np.array_equal(pos, want[1]), (pat, kw, cnt, want[0])
        # a pattern that can overlap itself stays in one window whatever the caller asks for; every other one is cut in three
        pieces = gpu.split_mode(p, text.size) == abi.SPLIT_PIECES
        assert pieces == (pat not in (b"[ab]{2}", b"q{16}")) and gpu.last_shard_info().shards == (3 if pieces else 1)
    # a refused expression takes the failure road
    with pytest.raises(KrepGpuError):
        gpu.search(regex_ref.params(b"a.*b"), text[:1000])


def test_injected_failure_falls_back_to_the_registered_regex_search(gpu):
    """the registered CPU selector hands back a regex_search; params (compiled_regex included) reach it untouched"""
    rng = np.random.RandomState(9)
    text = planted(rng, 200000, b"abcdefghijklmnopqrstuvwxyz \n", b"SherlOck", 8)
    pat = b"Sherl[oO]ck"
    want = expected(pat, text, track_positions=False)
    seen = {}

    def cpu_regex_search(pp, t, n, res):
        seen["compiled"] = pp.contents.compiled_regex
        seen["n"] = n
        return want[0]

    fn = abi.SEARCH_FUNC(cpu_regex_search)
    select_t = C.CFUNCTYPE(C.c_void_p, C.POINTER(abi.SearchParams))
    ref_fn = C.cast(regex_ref._lib().regex_search, C.c_void_p).value

    def select(pp):
        return ref_fn if (ref_fn and seen.get("use_ref")) else C.cast(fn, C.c_void_p).value

    cb = select_t(select)
    gpu.set_cpu_fallback(C.cast(cb, C.c_void_p).value)
    try:
        p = regex_ref.params(pat, track_positions=False)
        comp = regex_ref.Compiled(pat)
        p.s.compiled_regex = comp.ptr
        gpu.inject_failure(3)
        got = gpu.search(p, text)
        assert gpu.last_status() == abi.STATUS_FELL_BACK and got[0] == want[0]
        assert seen["compiled"] == comp.ptr.value and seen["n"] == text.size
        # the reference's own function as the fallback, records included
        seen["use_ref"] = True
        p2 = regex_ref.params(pat)
        p2.s.compiled_regex = comp.ptr
        full = expected(pat, text)
        got = gpu.search(p2, text)
        assert gpu.last_status() == abi.STATUS_FELL_BACK and got[0] == full[0] and np.array_equal(got[1], full[1])
        gpu.inject_failure(0)
        got = gpu.search(p, text)
        assert gpu.last_status() == abi.STATUS_OK and got[0] == want[0]
    finally:
        gpu.inject_failure(0)
        gpu.set_cpu_fallback(None)


def test_grep_lines_of_a_regex_plan(gpu):
    rng = np.random.RandomState(10)
    text = planted(rng, 70001, b"abcdefghij \n", b"ab\ncd", 5)
    hold, d_text = to_device(text)
    for pat, mc in ((b"ab[[:space:]]cd", None), (b"[a-c]{3}", None), (b"j[ \n]a", 7), (b"[ab]{2}", None)):
        want = expected(pat, text)
        kw = {} if mc is None else dict(max_count=mc)
        plan = gpu.plan(regex_ref.params(pat, **kw))
        try:
            got = plan.grep_lines(d_text, text.size, filename=b"f.txt")
            assert got == lm.grep_output(text.tobytes(), want[1], b"f.txt:", mc), (pat, mc)
        finally:
            plan.close()
        plan = gpu.plan(regex_ref.params(pat, **kw), only_matching=True)  # (-o changes nothing for regex_search: the same records)
        try:
            out = plan.grep_only_matching(d_text, text.size)
            assert out.count(b"\n") == (want[0] if mc is None else min(mc, want[0])), (pat, mc)
        finally:
            plan.close()
    del hold
