"""The two-pass walk of a long line (tests/regex_long_lines_model.py: a backward co-reachability pass, a forward walk pruned by it)
without a device: it gives the match lists of the brute-force matcher regex_groups_model.matches() on random texts, the compiled
reference's records on the lines that make the restarting walk quadratic, in about three steps per byte.  Also the switch
krep_gpu_set_regex_long_lines: it exists, is off by default, reads its environment variable at load and moves no answer of
can_accelerate or split_mode."""
import os
import subprocess
import sys

import numpy as np
import pytest

import krep_amd
import regex_groups_model as gm
import regex_long_lines_model as llm
import regex_ref
from krep_amd import abi

# (expression, the fragments the random texts are made of)
EXPRESSIONS = [(b"a|a[a-z]*!", b"a a b ! ! z \n A"), (b"a.*b", b"a a b c \n A B"), (b"(ab)+", b"ab ab a b \n AB"),
               (b"(foo|bar)+;", b"foo bar ; ; fo \n FOO"), (b"([a-z]+\\.)+com", b"ab . . com c \n COM"), (b"^a+b", b"a a b \n \n A"),
               (b"[a-z]+c$", b"a b c c \n \n C"), (b"(a|ab)(c|bcd)+", b"a ab c bcd b \n BCD"), (b"x(ab)*y", b"x ab ab y a \n X"),
               (b"^(a|b)+c$", b"a b c c \n \n B"), (b"ERROR.*timeout", b"ERROR timeout x x \n error TIMEOUT")]


def random_text(rng, fragments: bytes, limit: int) -> np.ndarray:
    """fragments (separated by blanks, and a blank is one too) drawn until the text would pass its length, at most `limit` bytes"""
    frags = fragments.split(b" ") + [b" "]
    out, size = b"", rng.randint(0, limit + 1)
    while True:
        f = frags[rng.randint(len(frags))]
        if len(out) + len(f) > size:
            return np.frombuffer(out, dtype=np.uint8)
        out += f


@pytest.fixture(autouse=True, scope="module")
def _c_locale():
    with regex_ref.c_locale():
        yield


@pytest.mark.parametrize("k", range(len(EXPRESSIONS)))
def test_the_two_passes_equal_the_brute_force_matcher(k):
    pat, fragments = EXPRESSIONS[k]
    rng = np.random.RandomState(4200 + k)
    hits = 0
    for cs in (True, False):
        au = gm.automaton([pat], cs)
        for _ in range(60):
            text = random_text(rng, fragments, 120)
            want = gm.matches(au, text, cs)
            steps = [0]
            assert llm.matches(au, text, cs, steps) == want, (pat, cs, text.tobytes())
            assert llm.line_counts(au, text, cs) == sum(1 for line in want if line), (pat, cs, text.tobytes())
            assert steps[0] <= 3 * int(text.size) + 1
            hits += sum(len(line) for line in want)
    assert hits > 20, (pat, hits)  # the texts hold matches


@pytest.mark.parametrize("pat", [b"a|a[a-z]*!", b"a.*b"])
def test_the_killer_lines_equal_the_compiled_reference_in_linear_work(pat):
    """8192 a's on one line: every start of the restarting walk runs to the line's end; the two passes take at most 3 steps a byte"""
    assert regex_ref.available(), "the compiled reference (oracle/_ref/libkrep_ref_avx2.so) is missing"
    n = 8192
    for tail in (b"", b"\n", b"b\n"):
        text = np.frombuffer(b"a" * n + tail, dtype=np.uint8)
        want = regex_ref.call(pat, text)
        au = gm.automaton([pat])
        steps = [0]
        got = [m for line in llm.matches(au, text, True, steps) for m in line]
        assert len(got) == want[0] and np.array_equal(np.asarray(got, dtype=np.uint64).reshape(-1, 2), want[1]), (pat, tail)
        assert steps[0] <= 3 * int(text.size) + 1, steps
        assert llm.line_counts(au, text) == regex_ref.call(pat, text, count_lines=True)[0]


def test_the_switch_exists_is_off_by_default_and_moves_no_selector_answer():
    e = krep_amd.load()
    for sym in ("krep_gpu_set_regex_long_lines", "krep_gpu_get_regex_long_lines", "krep_gpu_debug_set_regex_long_budget",
                "krep_gpu_debug_regex_long_walks"):
        assert hasattr(e.lib, sym), sym
    code = ("import krep_amd; e = krep_amd.load(); "
            "print(int(e.get_regex_long_lines()), int(e.lib.krep_gpu_get_regex_long_lines()))")
    env = {k: v for k, v in os.environ.items() if k != "KREP_GPU_REGEX_LONG_LINES"}
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", code], cwd=root, env=env, capture_output=True, text=True, check=True).stdout.split()
    assert out == ["0", "0"]
    out = subprocess.run([sys.executable, "-c", code], cwd=root, env=dict(env, KREP_GPU_REGEX_LONG_LINES="1"), capture_output=True,
                         text=True, check=True).stdout.split()
    assert out == ["1", "1"]
    searches = [abi.Params([b"a+b"], regex=True), abi.Params([b"ERROR.*timeout"], regex=True, count_lines=True),
                abi.Params([b"(ab)+"], regex=True), abi.Params([b"ab[cd]"], regex=True), abi.Params([b"abc"])]
    was = e.get_regex_loops(), e.get_regex_groups(), e.get_regex_loops_windows(), e.get_regex_long_lines()
    try:
        for loops in (False, True):
            for groups in (False, True):
                for windows in (False, True):
                    e.set_regex_loops(loops)
                    e.set_regex_groups(groups)
                    e.set_regex_loops_windows(windows)
                    answers = []
                    for on in (False, True):
                        e.set_regex_long_lines(on)
                        assert e.get_regex_long_lines() == on
                        answers.append([(e.can_accelerate(p), e.split_mode(p, 1 << 20)) for p in searches])
                    assert answers[0] == answers[1], (loops, groups, windows)
    finally:
        e.set_regex_loops(was[0])
        e.set_regex_groups(was[1])
        e.set_regex_loops_windows(was[2])
        e.set_regex_long_lines(was[3])
