"""The window driver the two krep -E kernels share (rx_window / rx_drive in kg_regex.hip): pairs of patterns with the SAME match set
of which the first runs regex_scan (kg_regex.hip) and the second regex_alt_scan (kg_regex_alt.hip).  Both members of a pair must
fill every field of krep_gpu_scan_out_t alike, store the same records, and agree with what regex_search of the compiled reference
returns (the expected() of test_gpu_regex_alt.py, for the anchored pair that of test_gpu_regex_ext.py: the model must agree with
the reference each time).  Nothing expected comes from the device."""
import numpy as np
import pytest

import regex_alt_model as am
import regex_ext_model as em
import test_gpu_regex_alt as alt
import test_gpu_regex_ext as ext
from krep_amd import abi
from krep_amd.engine import KrepGpuError
from test_gpu_regex_alt import UNIT, _c_locale, gpu, rx, to_device  # noqa: F401  (the fixtures of that suite)

pytestmark = pytest.mark.gpu

N = 4 * UNIT + 100
FIELDS = ("count", "stored", "total_matches", "overflow", "line_count", "has_newline", "head_line_hit", "tail_line_hit")
# (the pattern regex_scan takes, the one only regex_alt_scan takes, alphabet, the strings planted at the boundaries and how many bytes in
#  front of one they start, the strings on byte 0 and on the last byte, anchored, occurrences can overlap)
PAIRS = [
    (b"ab[cd]", b"abc|abd", b"abcd \n", [b"abc", b"abd"], (1, 2), b"abc", b"abd", False, False),
    # the greedy pass of both, kWalkGreedy against the sorted kWalkAlt; c stops a run of [ab], so the plants' matches stand where they say
    (b"[ab][ab]", b"a[ab]|b[ab]", b"abc\n", [b"cabab"], (2, 4), b"aba", b"cbbab", False, True),
    (b"^ab[cd]$", b"^(abc|abd)$", b"abcd\n", [b"abc", b"abd"], (1, 2), b"abc", b"abd", True, False),
]


def make_text(pair):
    """N bytes over the pair's alphabet with a match across every 32-KiB unit boundary, a lane and a cell boundary, one directly behind
    each, one on byte 0 and one on the last byte (an anchored plant stands between newlines, or at an end of the text)"""
    _, _, alphabet, plants, backs, head, tail, anchored, _ = PAIRS[pair]
    t = alt.background(np.random.RandomState(4100 + pair), N, alphabet)

    def put(s, plant):
        p = np.frombuffer(plant, dtype=np.uint8)
        t[s:s + p.size] = p
        if anchored and s > 0:
            t[s - 1] = 10
        if anchored and s + p.size < N:
            t[s + p.size] = 10

    for i, b in enumerate(list(range(UNIT, N, UNIT)) + [16 * 5, 1024 * 3]):
        put(b - backs[i % len(backs)], plants[i % len(plants)])
        put(b + 16, plants[(i + 1) % len(plants)])
    put(0, head)
    put(N - len(tail), tail)
    return t


def windows_of(out):
    return tuple(int(getattr(out, f)) for f in FIELDS)


def scan(plan, d_text, capacity=0, lo=0, hi=None):
    """-> (the eight fields, the stored records)"""
    import torch
    pos = torch.full((2 * max(capacity, 1),), -1, dtype=torch.int64, device="cuda")
    out = plan.scan(d_text, N, lo, N if hi is None else hi, 0, pos.data_ptr() if capacity else 0, capacity)
    rec = pos[:2 * int(out.stored)].cpu().numpy().astype(np.uint64).reshape(-1, 2)
    assert (pos[2 * int(out.stored):] == -1).all()  # nothing behind the stored records
    return windows_of(out), rec


def build_cases():
    out = []
    for pair, (first, second, *_, anchored, overlap) in enumerate(PAIRS):
        text = make_text(pair)
        want = {}
        for pat in (first, second):
            expected = ext.expected if anchored else alt.expected
            w = {"full": expected([pat], text), "lines": expected([pat], text, count_lines=True)}
            for mc in (0, 1, 3):
                for tp in (True, False):
                    w[(mc, tp)] = expected([pat], text, max_count=mc, track_positions=tp)
            if anchored:
                prog = em.branches([pat])
                w["window_lines"] = lambda lo, hi, prog=prog, text=text: ext.window_lines(prog, text, lo, hi)
                w["starts"] = em.occurrences(prog, text)[0]
            else:
                brs = am.branches([pat])
                w["window_lines"] = lambda lo, hi, brs=brs, text=text: alt.window_lines(brs, text, lo, hi)
                w["starts"] = am.occurrences(brs, text)[0]
            want[pat] = w
        a, b = want[first], want[second]
        # the pair has one match set, by the reference
        assert a["full"][0] == b["full"][0] > 20 and np.array_equal(a["full"][1], b["full"][1])
        assert a["lines"][0] == b["lines"][0] > 5 and np.array_equal(a["starts"], b["starts"])
        rec = a["full"][1]
        assert rec[0, 0] == 0 and rec[-1, 1] == N  # byte 0 and the last byte
        for u in range(UNIT, N, UNIT):                 # a match across every unit boundary
            assert ((rec[:, 0] < u) & (rec[:, 1] > u)).any(), (first, u)
        assert overlap == (a["starts"].size > a["full"][0])  # the greedy selection drops occurrences exactly in the overlapping pair
        out.append((text, want))
    return out


@pytest.fixture(scope="module")
def cases():
    """per pair: the text and, from the reference, what every mode must give (computed once, never changed)"""
    return build_cases()


def test_each_pattern_compiles_where_the_pair_supposes(gpu):
    """the first of a pair by regex_compile_anchored (regex_scan), the second only by regex_compile_alt / _ext (regex_alt_scan)"""
    for first, second, *_, anchored, overlap in PAIRS:
        info = gpu.regex_compile_anchored(rx([first]))
        assert (bool(info.bol), bool(info.eol)) == (anchored, anchored) and bool(info.seq.self_overlap) == overlap
        with pytest.raises(KrepGpuError):
            gpu.regex_compile_anchored(rx([second]))
        if anchored:
            with pytest.raises(KrepGpuError):
                gpu.regex_compile_alt(rx([second]))
            x = gpu.regex_compile_ext(rx([second]))
            assert x.bol and x.eol
            info2 = x.alt
        else:
            info2 = gpu.regex_compile_alt(rx([second]))
        assert info2.n_branches == 2 and bool(info2.cross_overlap) == overlap
        assert (gpu.split_mode(rx([first]), N) == abi.SPLIT_WHOLE) == overlap == (gpu.split_mode(rx([second]), N) == abi.SPLIT_WHOLE)


def run_pair(gpu, pair, text, want):
    first, second, *_, overlap = PAIRS[pair]
    hold, d_text = to_device(text)
    got = {}
    for pat in (first, second):
        w = want[pat]
        full_n, full_rec = w["full"]
        g = []
        # count mode: no record buffer
        plan = gpu.plan(rx([pat]))
        try:
            f, rec = scan(plan, d_text)
            assert f[:4] == (full_n, 0, full_n, 0) and rec.size == 0, (pat, f)
            g.append((f, rec))
            # records, capacity = half the count: the first half in order, overflow set
            half = full_n // 2
            f, rec = scan(plan, d_text, half)
            assert f[:4] == (full_n, half, full_n, 1) and np.array_equal(rec, full_rec[:half]), (pat, f)
            g.append((f, rec))
            # ample capacity
            f, rec = scan(plan, d_text, full_n + 7)
            assert f[:4] == (full_n, full_n, full_n, 0) and np.array_equal(rec, full_rec), (pat, f)
            assert f[4] == 0  # line_count belongs to count_lines_mode
            g.append((f, rec))
            # three windows (an overlapping pattern takes one window only, both kernels refuse alike)
            cuts = [0, UNIT + 33, 3 * UNIT - 1, N]
            if overlap:
                with pytest.raises(KrepGpuError, match="overlap"):
                    plan.scan(d_text, N, cuts[1], cuts[2])
            else:
                pieces = [scan(plan, d_text, full_n + 7, lo, hi) for lo, hi in zip(cuts[:-1], cuts[1:])]
                assert np.array_equal(np.concatenate([r for _, r in pieces]), full_rec), pat
                for (f, r), lo, hi in zip(pieces, cuts[:-1], cuts[1:]):
                    mine = int(((full_rec[:, 0] >= lo) & (full_rec[:, 0] < hi)).sum())
                    assert f[:4] == (mine, mine, mine, 0), (pat, lo, hi, f)
                g += pieces
        finally:
            plan.close()
        for mc in (0, 1, 3):
            for tp in (True, False):
                n, rec_want = w[(mc, tp)]
                plan = gpu.plan(rx([pat], max_count=mc, track_positions=tp))
                try:
                    f, rec = scan(plan, d_text, full_n + 7)
                    stored = n if tp else 0
                    assert (f[0], f[1], f[3]) == (n, stored, 0) and np.array_equal(rec, rec_want[:stored]), (pat, mc, tp, f)
                    assert f[2] == full_n, (pat, mc, tp, f)  # total_matches is uncapped
                    g.append((f, rec))
                finally:
                    plan.close()
        # -c, whole and in three windows that krep_gpu_combine_line_counts folds
        plan = gpu.plan(rx([pat], count_lines=True))
        try:
            f, rec = scan(plan, d_text)
            lines = w["lines"][0]
            assert f == (lines, 0, w["starts"].size, 0) + w["window_lines"](0, N), (pat, f)
            assert f[4] == lines
            g.append((f, rec))
            cuts = [0, UNIT + 33, 3 * UNIT - 1, N]
            outs = [plan.scan(d_text, N, lo, hi) for lo, hi in zip(cuts[:-1], cuts[1:])]
            for o, lo, hi in zip(outs, cuts[:-1], cuts[1:]):
                assert windows_of(o)[4:] == w["window_lines"](lo, hi), (pat, lo, hi)
                g.append((windows_of(o), rec))  # (no records under -c)
            assert gpu.lib.krep_gpu_combine_line_counts((abi.ScanOut * 3)(*outs), 3) == lines, pat
        finally:
            plan.close()
        got[pat] = g
    del hold
    # the two kernels through the one driver: every field and every record alike, mode by mode
    assert len(got[first]) == len(got[second])
    for k, ((fa, ra), (fb, rb)) in enumerate(zip(got[first], got[second])):
        assert fa == fb and np.array_equal(ra, rb), (first, second, k, fa, fb)


@pytest.mark.parametrize("grid", [1, 0])
@pytest.mark.parametrize("pair", range(len(PAIRS)))
def test_both_kernels_fill_the_scan_out_alike(gpu, cases, pair, grid):
    """grid 1: one workgroup (krep_gpu_debug_force_regex_grid), a wave takes unit after unit; 0: the kernels' own grid"""
    text, want = cases[pair]
    try:
        gpu.force_regex_grid(grid)
        run_pair(gpu, pair, text, want)
    finally:
        gpu.force_regex_grid(0)
