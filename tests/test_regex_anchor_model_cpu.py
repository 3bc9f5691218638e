"""The rule of include/krep_gpu.h ("line anchors around a class sequence") against the compiled reference's regex_search: random
texts and flags, every case answered by oracle/_ref — there is no restatement for regex."""
import numpy as np
import pytest

import regex_anchor_model as am
import regex_ref
from krep_amd import abi

PATTERNS = [b"^a", b"a$", b"^a$", b"^ab", b"ab$", b"^ab$", b"^a[ab]", b"a[ab]$", b"^[ab]{3}", b"[ab]{3}$", b"^[ab]{3}$", b"^[ab]{2}",
            b"^[a\n]{2}", b"[a\n]{2}$", b"^[a\n]{2}$", b"^[[:space:]]a", b"[[:space:]]a$", b"^[[:space:]]a$", b"^[[:space:]]",
            b"[[:space:]]$", b"^.[^a]", b".[^a]$", b"^.[^a]$", b"^[^a]", b"[^a]$", b"^[^a]$", b"^[\n]", b"[\n]$", b"^[\n]a$",
            b"^a{2}", b"b{2}$", b"\\^a", b"a\\$", b"[$^]", b"^[ab]{6}", b"^[ab]{5}$"]
ALPHABET = np.frombuffer(b"ab\n \x00\xe9", dtype=np.uint8)
# short lines of mostly a and b: in most texts of 8 bytes and more most patterns above have a line that starts or ends their way
WEIGHTS = np.array([0.36, 0.18, 0.32, 0.06, 0.04, 0.04])
MODES = [dict(), dict(), dict(track_positions=False), dict(count_lines=True), dict(count_lines=True), dict(max_count=0),
         dict(max_count=1), dict(max_count=3), dict(max_count=3, count_lines=True), dict(case_sensitive=False),
         dict(case_sensitive=False, count_lines=True), dict(max_count=1, track_positions=False)]


@pytest.fixture(autouse=True, scope="module")
def _c_locale():
    """the reference runs in the C locale (it never calls setlocale()); Python's start-up put the process into the environment's"""
    with regex_ref.c_locale():
        yield


def test_split_finds_the_anchors():
    assert am.split(b"^a") == (True, b"a", False) and am.split(b"a$") == (False, b"a", True) and am.split(b"^a$") == (True, b"a", True)
    assert am.split(b"a\\$") == (False, b"a\\$", False) and am.split(b"\\$$") == (False, b"\\$", True)
    assert am.split(b"[$^]") == (False, b"[$^]", False) and am.split(b"[\\]$") == (False, b"[\\]", True)
    assert am.split(b"\\^a") == (False, b"\\^a", False) and am.split(b"^[^a]{3}$") == (True, b"[^a]{3}", True)


@pytest.mark.parametrize("seed", range(4))
def test_model_equals_reference_regex_search(seed):
    assert regex_ref.available(), "the compiled reference (oracle/_ref/libkrep_ref_avx2.so) must answer every case: there is no restatement for regex"
    rng = np.random.RandomState(5200 + seed)
    n_cases = n_long = n_long_hit = 0
    for _ in range(2600):
        pat = PATTERNS[rng.randint(len(PATTERNS))]
        n = rng.randint(0, 41)
        # a draw around WEIGHTS: some texts are nearly all of one byte (long runs), most keep the short lines
        w = rng.dirichlet(WEIGHTS * 24)
        text = ALPHABET[rng.choice(ALPHABET.size, size=n, p=w)]
        kw = MODES[rng.randint(len(MODES))]
        want = regex_ref.call(pat, text, **kw)
        got = am.run(pat, text, **kw)
        assert got[0] == want[0], (pat, kw, text.tobytes(), got[0], want[0])
        assert np.array_equal(got[1], want[1]), (pat, kw, text.tobytes(), got[1][:6], want[1][:6])
        n_cases += 1
        if n >= 8:
            n_long += 1
            n_long_hit += want[0] > 0  # (the reference's own answer: agreement on "nothing matches" must not carry the test)
    assert n_cases == 2600
    assert 2 * n_long_hit >= n_long, (n_long_hit, n_long)
