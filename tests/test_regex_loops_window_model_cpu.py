"""The window rule of a loops search (tests/regex_loops_window_model.py: the records a window owns and its four -c facts, from the text
alone) against the compiled reference, without a device: the per-window quadruples folded by the library's host-only
krep_gpu_combine_line_counts give regex_search's -c, and the windows' records concatenate to its list.  Also the switch
krep_gpu_set_regex_loops_windows: it exists, is off by default, and krep_gpu_split_mode() says PIECES for a loops search only with both
switches on."""
import numpy as np
import pytest

import krep_amd
import regex_loops_model as lm
import regex_loops_window_model as wm
import regex_ref
from krep_amd import abi
from test_regex_loops_model_cpu import ALPHABET, FIRST, random_case


@pytest.fixture(autouse=True, scope="module")
def _c_locale():
    with regex_ref.c_locale():
        yield


@pytest.fixture(scope="module")
def eng():
    e = krep_amd.load()
    loops, windows = e.get_regex_loops(), e.get_regex_loops_windows()
    try:
        yield e
    finally:
        e.set_regex_loops(loops)
        e.set_regex_loops_windows(windows)


def fold(eng, quads) -> int:
    arr = (abi.ScanOut * len(quads))(*[wm.scan_out(q) for q in quads])
    return int(eng.lib.krep_gpu_combine_line_counts(arr, len(quads)))


def random_cuts(rng, n):
    """cut sets that include 1-byte windows, windows without a newline, and no cut at all"""
    if n < 2:
        return []
    kind = rng.randint(4)
    if kind == 0:
        return list(range(1, n))  # every window one byte
    if kind == 1:
        c = rng.randint(1, n)
        return [c, c + 1]  # a 1-byte window inside the text
    return rng.randint(1, n, size=rng.randint(0, 7)).tolist()


def check(eng, pats, text, cs, cuts):
    lines = wm.per_line(pats, text, cs)
    want = lm.ref_call(pats, text, case_sensitive=cs)
    want_c = lm.ref_call(pats, text, case_sensitive=cs, count_lines=True)[0]
    wins = wm.cuts_to_windows(cuts, int(text.size)) if text.size else []
    answers = [wm.window(lines, text, lo, hi) for lo, hi in wins]
    records = [r for rec, _ in answers for r in rec]
    assert records == [tuple(r) for r in want[1].tolist()], (pats, cs, text.tobytes(), cuts)
    quads = [q for _, q in answers]
    assert fold(eng, quads) == want_c, (pats, cs, text.tobytes(), wins, quads, want_c)
    return wins, quads


def test_windows_folded_equal_the_reference_on_random_patterns_of_the_grammar(eng):
    assert regex_ref.available(), "the compiled reference (oracle/_ref/libkrep_ref_avx2.so) is missing"
    rng = np.random.RandomState(20261021)
    seen = {"one_byte": 0, "no_newline": 0, "several": 0, "head_and_open": 0, "bol": 0, "eol": 0, "icase": 0, "uncut": 0}
    for _ in range(3000):
        pats, _, kw = random_case(rng)
        cs = kw["case_sensitive"]
        text = ALPHABET[rng.randint(0, ALPHABET.size, size=rng.randint(0, 61))].copy()
        cuts = random_cuts(rng, int(text.size))
        wins, quads = check(eng, pats, text, cs, cuts)
        seen["one_byte"] += any(hi - lo == 1 for lo, hi in wins)
        seen["no_newline"] += any(not q[3] for q in quads)
        seen["several"] += len(wins) > 2
        seen["head_and_open"] += any(a[2] and b[1] for a, b in zip(quads, quads[1:]))  # a line counted on both sides of a cut
        seen["bol"] += pats[0].startswith(b"^")
        seen["eol"] += pats[0].endswith(b"$")
        seen["icase"] += not cs
        seen["uncut"] += len(wins) == 1
    assert all(v > 100 for v in seen.values()), seen


@pytest.mark.parametrize("k", range(len(FIRST)))
def test_the_first_patterns_at_every_single_cut_and_in_one_byte_windows(eng, k):
    pats = FIRST[k]
    rng = np.random.RandomState(1900 + k)
    alphabet = np.frombuffer(b"aabbcxy\n" if k == 7 else b"aabbc\n", dtype=np.uint8)
    for _ in range(40):
        text = alphabet[rng.randint(0, alphabet.size, size=rng.randint(1, 31))].copy()
        n = int(text.size)
        for cs in (True, False):
            for c in range(1, n):
                check(eng, pats, text, cs, [c])
            check(eng, pats, text, cs, list(range(1, n)))


def test_fixed_windows():
    t = np.frombuffer(b"xayxby\naab ab\n\nb aab", dtype=np.uint8)
    lines = wm.per_line([b"x(a+|b)y"], t)
    assert wm.window(lines, t, 0, 3) == ([(0, 3)], (1, True, True, False))          # the cut between two touching matches
    assert wm.window(lines, t, 3, 7) == ([(3, 6)], (1, True, False, True))          # ... the same line again: head, and its newline
    lines = wm.per_line([b"a+b"], t)
    assert wm.window(lines, t, 7, 8) == ([(7, 10)], (1, True, True, False))          # a 1-byte window on a match's first byte
    assert wm.window(lines, t, 8, 9) == ([], (0, False, False, False))               # ... inside it: the match is the window's before
    assert wm.window(lines, t, 13, 14) == ([], (0, False, False, True))              # a 1-byte window that is a newline
    assert wm.window(lines, t, 14, 20) == ([(17, 20)], (1, False, True, True))       # the line starts behind the window's newline


def test_the_switch_exists_is_off_by_default_and_moves_split_mode(eng):
    import os
    import subprocess
    import sys
    code = ("import krep_amd; e = krep_amd.load(); "
            "print(int(e.get_regex_loops_windows()), int(e.lib.krep_gpu_get_regex_loops_windows()))")
    env = {k: v for k, v in os.environ.items() if k != "KREP_GPU_REGEX_LOOPS_WINDOWS"}
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", code], cwd=root, env=env, capture_output=True, text=True, check=True).stdout.split()
    assert out == ["0", "0"]
    out = subprocess.run([sys.executable, "-c", code], cwd=root, env=dict(env, KREP_GPU_REGEX_LOOPS_WINDOWS="1"), capture_output=True,
                         text=True, check=True).stdout.split()
    assert out == ["1", "1"]
    loops = [abi.Params([b"a+b"], regex=True), abi.Params([b"a+b"], regex=True, count_lines=True),
             abi.Params([b"ERROR.*timeout"], regex=True, case_sensitive=False)]
    fixed = abi.Params([b"ab[cd]"], regex=True)  # (a fixed-length sequence: PIECES whatever the switches say)
    for on_loops in (False, True):
        for on_windows in (False, True):
            eng.set_regex_loops(on_loops)
            eng.set_regex_loops_windows(on_windows)
            assert eng.get_regex_loops_windows() == on_windows
            for p in loops:
                want = abi.SPLIT_PIECES if (on_loops and on_windows) else abi.SPLIT_WHOLE
                assert eng.split_mode(p, 1 << 20) == want, (on_loops, on_windows)
            assert eng.split_mode(fixed, 1 << 20) == abi.SPLIT_PIECES
