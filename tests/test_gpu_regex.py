"""krep -E on the device (kg_regex.hip) against the reference's regex_search: the compiled reference (oracle/_ref, through
tests/regex_ref.py) answers every case; the rule of tests/regex_model.py must agree with it each time."""
import ctypes as C

import numpy as np
import pytest

import line_model as lm
import only_matching_model as om
import regex_model
import regex_ref
import regex_skip_model as sm
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
    e.force_regex_grid(0)


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
            assert out == om.grep_o_output(text.tobytes(), want[1], None, False, mc), (pat, mc)
            assert out.count(b"\n") == (want[0] if mc is None else min(mc, want[0])) > 0, (pat, mc)
            out = plan.grep_only_matching(d_text, text.size, filename=b"f.txt", color=True)
            assert out == om.grep_o_output(text.tobytes(), want[1], b"f.txt", True, mc), (pat, mc)
        finally:
            plan.close()
    del hold


# ------------------------------------------------------------------------------------ the entry state behind skipped cells
@pytest.fixture(scope="module")
def skip_texts():
    """regex_skip_model.build_text for each of its patterns, built once (tests/test_regex_skip_model_cpu.py pins what they hold)"""
    out = []
    for pat, cs in sm.PATTERNS:
        cl = regex_model.classes(pat, cs)
        out.append((pat, dict() if cs else dict(case_sensitive=False), cl) + sm.build_text(cl))
    return out


@pytest.mark.parametrize("case", range(len(sm.PATTERNS)))
def test_entry_state_behind_skipped_cells(gpu, skip_texts, case):
    """the anchor sits behind the first class, the background holds no anchor byte: most cells are skipped, and a match that straddles
    the boundary behind a skipped cell is found only through the entry state rebuilt from that cell's last 16 bytes; the decoys are
    what a state of 0xFFFF or one left over from the last walked cell reports"""
    pat, cs, cl, text, plants = skip_texts[case]
    info = gpu.regex_compile(regex_ref.params(pat, **cs))
    ai, ab = sm.anchor(cl)
    assert (info.L, info.anchor, info.n_anchor, bytes(info.anchor_bytes[:info.n_anchor])) == (len(cl), ai, ab.size, ab.tobytes())
    assert bool(info.self_overlap) == regex_model.self_overlap(cl)
    g = sm.Geometry(cl, text)
    assert sm.missing(cl, text) == [] and g.skipped.sum() >= 30 and len(g.dependent()) >= max(ai, 10)
    for kw in (dict(), dict(track_positions=False), dict(max_count=3)):
        want = expected(pat, text, **cs, **kw)
        got = gpu.search(regex_ref.params(pat, **cs, **kw), text)
        assert gpu.last_status() == abi.STATUS_OK
        assert got[0] == want[0], (pat, kw, got[0], want[0])
        assert np.array_equal(got[1], want[1]), (pat, kw, sorted(set(got[1][:, 0].tolist()) ^ set(want[1][:, 0].tolist()))[:8])
    assert expected(pat, text, **cs)[0] == g.occ.size  # (the plants stand apart: every occurrence is a match)


def skip_windows(g, plants, ai):
    """three windows that start 5, 9 and 13 bytes into a skipped cell (the grid starts at that cell, so other cells start the units), the
    last of them ending inside the text; then two that start one byte behind the start of a dependent straddler"""
    n = g.text.size
    skipped = [c for c in range(2, g.n_cells - 40) if g.skipped[c]]
    windows = [(skipped[0] * sm.CELL + 5, n), (skipped[len(skipped) // 2] * sm.CELL + 9, n), (skipped[3] * sm.CELL + 13, 100 * sm.CELL + 7)]
    dependents = [p for p in plants if p.kind == "straddler" and p.k <= ai]
    cut = [p for p in dependents if p.k % 16 != 1][:2] or dependents[:1]  # (L = 2 has k = 1 only: that own_lo is a cell boundary)
    return windows + [(p.start + 1, n) for p in cut]


@pytest.mark.parametrize("case", [i for i, (pat, cs) in enumerate(sm.PATTERNS) if pat not in (b"[0-9]{3}-[0-9]{4}", b"[a-f]{8}Q[a-f]{7}")])
def test_entry_state_in_windows_of_an_unaligned_text(gpu, skip_texts, case):
    """the same texts 3 bytes into their allocation, own_lo no multiple of 16: inside a run of skipped cells (the grid starts at
    own_lo & ~15, so the units start elsewhere and other cells are rebuilt), and one byte behind the start of a straddler, which is
    then not owned while its anchor byte is"""
    pat, cs, cl, text, plants = skip_texts[case]
    assert not regex_model.self_overlap(cl)
    n, L, (ai, _) = text.size, len(cl), sm.anchor(cl)
    g = sm.Geometry(cl, text)
    windows = skip_windows(g, plants, ai)
    hold, d_text = to_device(text, 3)
    plan = gpu.plan(regex_ref.params(pat, **cs))
    try:
        for i, (own_lo, own_hi) in enumerate(windows):
            gw = sm.Geometry(cl, text, own_lo, own_hi)
            mine = gw.occ
            if i < 3:
                assert own_lo % 16 and gw.origin % sm.CELL == 0 and g.skipped[own_lo // sm.CELL] and len(gw.dependent()) >= 3
            else:
                assert own_lo - 1 not in mine and own_lo - 1 in g.occ and ai >= 1  # (the straddler is not owned, its anchor byte is)
            out, rec = scan_records(plan, d_text, n, own_lo, own_hi, global_base=1000, global_len=1000 + n)
            assert out.count == mine.size and out.total_matches == mine.size, (pat, own_lo, own_hi, out.count, mine.size)
            assert np.array_equal(rec[:, 0], mine.astype(np.uint64) + 1000) and np.array_equal(rec[:, 1], rec[:, 0] + L)
            assert plan.scan(d_text, n, own_lo, own_hi).count == mine.size  # count only
    finally:
        plan.close()
    del hold


# ------------------------------------------------------------------------------------ -c with newlines inside long matches
NL_PATTERNS = [b"[a-c\n]{16}", b"x[a-c\n]{14}y", b"[\n]a{8}"]


def newline_sites(n):
    """-> [(kind, B)]: every cell boundary of the text (kind unit / round / cell) and three lane boundaries between two of them"""
    out = []
    for B in range(256, n - 256, 256):
        out.append(("unit" if B % sm.UNIT == 0 else "round" if B % sm.ROUND == 0 else "cell" if B % sm.CELL == 0 else "lane", B))
    return out


def newline_text(cl, n, turn, seed, breakers=True):
    """A text over abc, x, y and newline in which every site holds one newline at B - 1 - j, j = 0 .. L - 2, that is in the last L - 1
    bytes in front of a lane, cell, round or unit boundary B, so that its shifted coordinate n + L - 1 lies behind B, and a match that
    starts in front of it (the newline inside the match where its classes allow that), on it or directly behind it; a second match
    stands on the other line of the two the newline parts, and two more newlines close those lines.  The background has an x or y
    in every 7 bytes: no match outside the sites.  `turn` moves every kind of site through the (j, place) pairs: the three unit
    boundaries of a 100-KiB text see all of them in L - 1 turns.  breakers=False: abc only, and only the newlines are put (every
    position of a text without x and y starts a match of a class sequence that holds all of a, b, c and newline).
    -> (text, [(kind, B, j, place, newline)])"""
    L = len(cl)
    rng = np.random.RandomState(seed)
    text = np.frombuffer(b"abc", dtype=np.uint8)[rng.randint(0, 3, size=n)].copy()
    if breakers:
        at = np.arange(3, n, 7)
        text[at] = np.frombuffer(b"xy", dtype=np.uint8)[(at // 7) % 2]

    def match():
        m = np.zeros(L, dtype=np.uint8)
        for i, t in enumerate(cl):
            pick = [b for b in b"abcxy" if t[b]] or [10]
            m[i] = pick[rng.randint(len(pick))]
        return m

    combos = [(j, place) for j in range(L - 1) for place in ("front", "on", "behind")]
    sites = newline_sites(n)
    per_kind = {k: sum(1 for kind, _ in sites if kind == k) for k in ("unit", "round", "cell", "lane")}
    seen = dict.fromkeys(per_kind, 0)
    out = []
    for kind, B in sites:
        j, place = combos[(seen[kind] + turn * per_kind[kind]) % len(combos)]
        seen[kind] += 1
        p = B - 1 - j
        if breakers:
            inside = [d for d in range(1, L) if cl[d][10]]
            if place == "on" and not cl[0][10]:
                place = "front"
            s = p if place == "on" else p + 1 if place == "behind" else p - (inside[rng.randint(len(inside))] if inside else L)
            other = p - 40 if place == "behind" else p + 24
            for q in (other, s):
                text[q - 1], text[q + L] = ord("x"), ord("y")
                text[q:q + L] = match()
            text[p - 56] = text[p + 72] = 10
        text[p] = 10
        out.append((kind, B, j, place, p))
    return text, out


def window_lines(cl, text, lo, hi):
    """line_count, has_newline, head_line_hit, tail_line_hit of include/krep_gpu.h for the window [lo, hi): the starts and the newlines
    the window owns; a start ON a newline belongs to the line that newline ends"""
    occ = regex_model.occurrences(cl, text)
    mine = occ[(occ >= lo) & (occ < hi)]
    nl = np.flatnonzero(text[lo:hi] == 10) + lo
    lines = np.unique(np.searchsorted(nl, mine, side="left")).size  # the line of a start: the owned newlines in front of it
    head = bool(mine.size) and (nl.size == 0 or mine[0] <= nl[0])
    tail = bool(mine.size) and (nl.size == 0 or mine[-1] > nl[-1])
    return int(lines), bool(nl.size), bool(head), bool(tail)


@pytest.mark.parametrize("case", range(len(NL_PATTERNS)))
def test_count_lines_with_newlines_inside_long_matches(gpu, case):
    """-c moves every newline to coordinate n + L - 1: one in the last L - 1 bytes of a lane crosses into the next lane, of a cell
    into the next cell (through x63), of a unit into the next unit (through the guarded load in front of it)"""
    pat = NL_PATTERNS[case]
    cl = regex_model.classes(pat)
    L, n = len(cl), 3 * sm.UNIT + 4321
    assert gpu.regex_compile(regex_ref.params(pat)).L == L and L >= 9
    plan = gpu.plan(regex_ref.params(pat, count_lines=True))
    covered = set()
    try:
        turns = [(t, True) for t in range(L - 1)] + ([(0, False), (7, False)] if case == 0 else [])
        for turn, breakers in turns:
            text, sites = newline_text(cl, n, turn, 3000 + 100 * case + turn, breakers)
            covered |= {(kind, j, place) for kind, _, j, place, _ in sites if breakers}
            want = expected(pat, text, count_lines=True)
            got = gpu.search(regex_ref.params(pat, count_lines=True), text)
            assert gpu.last_status() == abi.STATUS_OK and got[0] == want[0] and got[1].size == 0, (pat, turn, breakers, got[0], want[0])
            assert want[0] == window_lines(cl, text, 0, n)[0] and want[0] > len(sites) // 2
            hold, d_text = to_device(text)
            assert plan.scan(d_text, n).line_count == want[0]
            # three windows: around a unit and a cell boundary, an odd offset, on a planted newline and on the byte behind it
            first, third = sites[len(sites) // 5][4], sites[4 * len(sites) // 5][4]
            lows = [sm.UNIT - 1, sm.UNIT, sm.UNIT + 1, 17 * sm.CELL - 1, 17 * sm.CELL + 1, 33333, first, first + 1]
            highs = [2 * sm.UNIT + 1, 2 * sm.UNIT, 2 * sm.UNIT - 1, 70 * sm.CELL + 1, 70 * sm.CELL - 1, 65537, third + 1, third]
            for pair in (turn % 8, (turn + 5) % 8):
                cuts = [0, lows[pair], highs[pair], n]
                outs = [plan.scan(d_text, n, lo, hi) for lo, hi in zip(cuts[:-1], cuts[1:])]
                for (lo, hi), o in zip(zip(cuts[:-1], cuts[1:]), outs):
                    have = (int(o.line_count), bool(o.has_newline), bool(o.head_line_hit), bool(o.tail_line_hit))
                    assert have == window_lines(cl, text, lo, hi), (pat, turn, breakers, lo, hi)
                assert gpu.lib.krep_gpu_combine_line_counts((abi.ScanOut * 3)(*outs), 3) == want[0], (pat, turn, cuts)
            del hold
    finally:
        plan.close()
    # every j at every kind of boundary, with every place the pattern allows
    places = {"front", "behind"} | ({"on"} if cl[0][10] else set())
    assert covered >= {(kind, j, place) for kind in ("lane", "cell", "round", "unit") for j in range(L - 1) for place in places}


# ------------------------------------------------------------------------------------ a starved grid: several units per wave
def sprinkled(rng, n, alphabet, plant, step):
    t = planted(rng, n, alphabet, plant, len(plant))
    p = np.frombuffer(plant, dtype=np.uint8)
    for s in range(step, n - len(p), step):
        t[s:s + len(p)] = p
    return t


def test_starved_grid_a_wave_takes_several_units(gpu):
    """1 and 2 workgroups on 14 units (krep_gpu_debug_force_regex_grid): a wave resets its state for every unit it takes, reads that
    unit's record offset, and adds up its counts: every instantiation of the kernel"""
    n = 13 * sm.UNIT + 100
    rng = np.random.RandomState(12)
    words = sprinkled(rng, n, b"abcdefghijklmnopqrstuvwxyz \n", b"Sherlock", 7001)
    skip_pat = b"[a-f]{7}S"
    skip_cl = regex_model.classes(skip_pat)
    skips, _ = sm.build_text(skip_cl, n=n, seed=3)
    g = sm.Geometry(skip_cl, skips)
    assert {c // sm.CELLS_PER_UNIT for _, c, _ in g.dependent()} == set(range(13)) and g.skipped.sum() > 13 * 8
    nl_pat = NL_PATTERNS[1]
    newlines, _ = newline_text(regex_model.classes(nl_pat), n, 4, 77)
    ab = background(rng, n, b"ab")
    jobs = [(b"[A-Z][a-z]{7}", words, dict(track_positions=False)), (b"[A-Z][a-z]{7}", words, dict()),        # the table path
            (skip_pat, skips, dict(track_positions=False)), (skip_pat, skips, dict()),                          # the anchor path
            (b"[a-z]{4}", words, dict(count_lines=True)), (nl_pat, newlines, dict(count_lines=True)),           # -c
            (b"[ab]{3}", ab, dict()), (b"[ab]{3}", ab, dict(track_positions=False))]                            # the greedy road
    wants = [expected(pat, text, **kw) for pat, text, kw in jobs]
    assert all(w[0] > 13 for w in wants)
    try:
        for blocks in (1, 2):
            gpu.force_regex_grid(blocks)
            for (pat, text, kw), want in zip(jobs, wants):
                got = gpu.search(regex_ref.params(pat, **kw), text)
                assert gpu.last_status() == abi.STATUS_OK
                assert got[0] == want[0] and np.array_equal(got[1], want[1]), (blocks, pat, kw, got[0], want[0])
    finally:
        gpu.force_regex_grid(0)
