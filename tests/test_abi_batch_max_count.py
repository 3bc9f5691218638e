"""CPU-side checks of the batch's max_count switch (include/krep_gpu.h "max_count behind a switch"): the symbols are exported, the
switch is off by default and read from $KREP_GPU_BATCH_MAX_COUNT when the library is loaded, off gives the pinned refusal, on takes
a finite max_count and leaves every other refusal its own reason.  Host logic only: the refusals come before any device work."""
import ctypes as C
import os
import subprocess
import sys

import pytest

import batch_model as bm
from krep_amd import abi, build
from test_batch_separable_cpu import REFUSED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PINNED = "batch: max_count is a property of each item's own record list; cutting per item is follow-up work"


@pytest.fixture()
def eng(monkeypatch):
    import krep_amd
    monkeypatch.setenv("KREP_GPU_ASSUME_AVAILABLE", "1")  # (the rule is host logic: the refusal comes before the device is asked)
    monkeypatch.delenv("KREP_GPU_DISABLE", raising=False)
    e = krep_amd.load()
    assert not e.get_batch_max_count()
    yield e
    e.set_batch_max_count(False)
    e.set_thread_config(None)


def verdict(eng, s):
    s.configure(eng)
    try:
        return eng.batch_can_accelerate(s.params()), eng.last_error()
    finally:
        eng.set_thread_config(None)


def test_the_symbols_are_exported_and_declared():
    import torch  # noqa: F401  (first, as krep_amd.Engine does: tests/test_abi_exports.py says why)
    lib = C.CDLL(build.build())
    for n in ("krep_gpu_set_batch_max_count", "krep_gpu_get_batch_max_count", "krep_gpu_debug_batch_cut_launches"):
        assert hasattr(lib, n), n
    boundary = open(os.path.join(ROOT, "include", "krep_gpu.h")).read()
    assert "krep_gpu_set_batch_max_count" in boundary and "krep_gpu_get_batch_max_count" in boundary
    assert "KREP_GPU_BATCH_MAX_COUNT" in boundary
    assert "krep_gpu_debug_batch_cut_launches" in open(os.path.join(ROOT, "include", "krep_gpu_debug.h")).read()


def test_the_switch_is_off_by_default_and_read_from_the_environment_at_load():
    code = ("import krep_amd; e = krep_amd.load(); print(int(e.get_batch_max_count())); "
            "e.set_batch_max_count(not e.get_batch_max_count()); print(int(e.get_batch_max_count()))")
    for value, want in ((None, "0\n1\n"), ("1", "1\n0\n"), ("0", "0\n1\n")):
        env = dict(os.environ)
        env.pop("KREP_GPU_BATCH_MAX_COUNT", None)
        if value is not None:
            env["KREP_GPU_BATCH_MAX_COUNT"] = value
        env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
        r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, cwd=ROOT)
        assert r.returncode == 0, r.stderr
        assert r.stdout == want, (value, r.stdout)


def test_off_refuses_with_the_pinned_reason_on_takes_and_off_refuses_again(eng):
    cases = [bm.Search("literal", [b"ab"], max_count=5), bm.Search("-c", [b"ab"], max_count=1, count_lines=True),
             bm.Search("dictionary", [b"ab", b"ba"], max_count=2), bm.Search("zero", [b"ab"], max_count=0),
             bm.Search("kmp", [b"abab"], level=abi.REF_SCALAR, max_count=3), bm.Search("single byte", [b"a"], max_count=4096),
             bm.Search("regex", [b"ab|abc"], regex=True, max_count=1)]
    import regex_ref
    with regex_ref.c_locale():
        for s in cases:
            ok, why = verdict(eng, s)
            assert not ok and why == PINNED, (s, why)
        eng.set_batch_max_count(True)
        assert eng.get_batch_max_count()
        for s in cases:
            ok, why = verdict(eng, s)
            assert ok and why == "", (s, why)
        eng.set_batch_max_count(False)
        for s in cases:
            ok, why = verdict(eng, s)
            assert not ok and why == PINNED, (s, why)


def test_a_refused_batch_call_writes_nothing_whatever_the_switch_says(eng):
    p = abi.Params([b"ab"], max_count=5)
    rc, res, n, first = bm.raw_call(eng, p, [b"xabx", b"ab"])
    assert rc == 2 and eng.last_error() == PINNED
    assert res == [(bm.POISON,) * 3] * 2 and n == 1 and first == 77
    eng.set_batch_max_count(True)
    p = abi.Params([b"a\nb"], max_count=5)
    rc, res, n, first = bm.raw_call(eng, p, [b"xabx", b"a\nb"])
    assert rc == 2 and "holds '\\n'" in eng.last_error()
    assert res == [(bm.POISON,) * 3] * 2 and n == 1 and first == 77


def test_every_other_refusal_keeps_its_reason_with_the_switch_on(eng):
    import regex_ref
    with regex_ref.c_locale():
        before = {s.name: verdict(eng, s) for s, _ in REFUSED}
        eng.set_batch_max_count(True)
        for s, reason in REFUSED:
            ok, why = verdict(eng, s)
            if "max_count" in s.kw:
                continue
            assert (ok, why) == before[s.name] and not ok and reason in why, (s, why)
            # ... and with a max_count as well: the cut lifts no other refusal
            kw = dict(s.kw)
            kw["max_count"] = 3
            m = bm.Search(s.name + " -m 3", s.pats, s.level, s.only_matching, s.regex, s.alphabet, s.plants, s.algo_override,
                          s.force_no_simd, **kw)
            ok, why = verdict(eng, m)
            assert not ok and why == before[s.name][1], (m, why)
        # neon_search with max_count == 0 stays refused, for its position rule and in words of its own
        neon = next(s for s, _ in REFUSED if s.name == "max_count 0 neon_search")
        ok, why = verdict(eng, neon)
        assert not ok and "neon_search" in why and why != PINNED, why
        taken = bm.Search("neon_search -m 1", [b"xyz"], level=abi.REF_NEON, max_count=1)
        assert verdict(eng, taken) == (True, "")
