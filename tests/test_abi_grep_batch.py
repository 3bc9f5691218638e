"""CPU-side checks of the grep output of a batch (include/krep_gpu.h "the grep output of a batch"): the three symbols are exported and
declared, the four new structs have the layout a C host compiles, without a device krep_gpu_grep_batch fails loudly — status 2, a
reason, `out` and `per_item` untouched — and every refusal of krep_gpu_batch_can_accelerate is a refusal here with the same reason."""
import ctypes as C
import os
import subprocess

import pytest

import regex_ref
from krep_amd import abi, build
from test_batch_separable_cpu import REFUSED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON = 0xDEADBEEF


@pytest.fixture(autouse=True, scope="module")
def _c_locale():
    with regex_ref.c_locale():
        yield


@pytest.fixture(scope="module")
def lib():
    import torch  # noqa: F401  (first, as krep_amd.Engine does: tests/test_abi_exports.py says why)
    return C.CDLL(build.build())


def test_the_symbols_are_exported_and_declared(lib):
    boundary = open(os.path.join(ROOT, "include", "krep_gpu.h")).read()
    for n in ("krep_gpu_format_lines_items", "krep_gpu_format_matches_items", "krep_gpu_grep_batch"):
        assert hasattr(lib, n), n
        assert "int " + n + "(" in boundary, n
    hooks = open(os.path.join(ROOT, "include", "krep_gpu_debug.h")).read()
    for n in ("krep_gpu_debug_grep_batch_times", "krep_gpu_debug_batch_format_launches"):
        assert hasattr(lib, n) and n in hooks, n
    # the existing hook keeps its signature
    assert "void krep_gpu_debug_batch_times(double *pack_ms, double *scan_ms, double *segment_ms, double *readback_ms);" in hooks


def test_struct_layouts_match_a_c11_probe(tmp_path):
    fields = [("krep_gpu_pack_view_t", abi.PackView, ["d_item_off", "n_items", "d_prefix_bytes", "d_prefix_off"]),
              ("krep_gpu_grep_format_t", abi.GrepFormat, ["prefixes", "prefix_lens", "line", "match"]),
              ("krep_gpu_grep_item_t", abi.GrepItem, ["count", "out_offset", "out_bytes"]),
              ("krep_gpu_grep_output_t", abi.GrepOutput, ["bytes", "len", "capacity"])]
    exprs, want = [], []
    for cname, py, names in fields:
        exprs.append(f"sizeof({cname})")
        want.append(C.sizeof(py))
        for f in names:
            exprs.append(f"offsetof({cname}, {f})")
            want.append(getattr(py, f).offset)
    src = tmp_path / "grep_abi.c"
    src.write_text('#include "krep_gpu.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void) { printf("'
                   + " ".join(["%zu"] * len(exprs)) + '\\n", ' + ", ".join(exprs) + "); return 0; }\n")
    exe = tmp_path / "grep_abi"
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-pedantic", "-Werror", f"-I{os.path.join(ROOT, 'include')}",
                        str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == want, (got, want)
    assert C.sizeof(abi.PackView) == 32 and C.sizeof(abi.GrepItem) == 24 and C.sizeof(abi.GrepOutput) == 24


def raw_call(e, params, items, names, cfg=None):
    """krep_gpu_grep_batch itself with poisoned per_item and an `out` (a malloc block of 8 bytes) that already holds 5 bytes
    -> (rc, per_item, (the block is where it was, out->len, out->capacity, its first 8 bytes))"""
    libc = C.CDLL(None)
    libc.malloc.restype, libc.malloc.argtypes, libc.free.restype, libc.free.argtypes = C.c_void_p, [C.c_size_t], None, [C.c_void_p]
    fmt, keep = e.grep_format(names, "lines")
    arr, n, held = e.batch_items(items)
    per = (abi.GrepItem * max(n, 1))()
    for p in per:
        p.count = p.out_offset = p.out_bytes = POISON
    block = libc.malloc(8)
    C.memmove(block, b"12345678", 8)
    out = abi.GrepOutput(block, 5, 8)
    dummy = C.c_int(0)
    if params.s.num_patterns > 1 and not params.s.ac_trie:
        params.s.ac_trie = C.cast(C.pointer(dummy), C.c_void_p)
    try:
        rc = e.lib.krep_gpu_grep_batch(params.ref, C.byref(cfg) if cfg is not None else None, arr, n, C.byref(fmt), per, C.byref(out), None)
        state = (out.bytes == block, out.len, out.capacity, C.string_at(out.bytes, 8))
    finally:
        params.s.ac_trie = None
        libc.free(out.bytes)
    del keep, held
    return rc, [(p.count, p.out_offset, p.out_bytes) for p in per[:n]], state


def untouched(per, state, n):
    return per == [(POISON,) * 3] * n and state == (True, 5, 8, b"12345678")


def test_without_a_device_the_call_fails_loudly_and_writes_nothing(monkeypatch):
    import krep_amd
    e = krep_amd.load()
    monkeypatch.setenv("KREP_GPU_DISABLE", "1")  # no usable device, whatever this host has
    monkeypatch.delenv("KREP_GPU_ASSUME_AVAILABLE", raising=False)
    p = abi.Params([b"ab"])
    rc, per, out = raw_call(e, p, [b"xabx", b"", b"ab"], [b"a", b"b", b"c"])
    assert rc == 2 and e.last_error()
    assert untouched(per, out, 3)
    with pytest.raises(krep_amd.KrepGpuError):
        e.grep_batch(p, [b"xabx", b"", b"ab"], [b"a", b"b", b"c"])


def test_every_refusal_of_the_batch_rule_is_a_refusal_here_with_the_same_reason(monkeypatch):
    import krep_amd
    e = krep_amd.load()
    monkeypatch.setenv("KREP_GPU_ASSUME_AVAILABLE", "1")  # (the rule is host logic: the refusal comes before the device is asked)
    monkeypatch.delenv("KREP_GPU_DISABLE", raising=False)
    assert len(REFUSED) >= 18
    for s, reason in REFUSED:
        s.configure(e)
        try:
            assert not e.batch_can_accelerate(s.params())
            why = e.last_error()
            assert why and reason in why, (s, why)
            rc, per, out = raw_call(e, s.params(), [b"xabx", b"a\nb"], [b"one", b"two"])
            assert rc == 2 and e.last_error() == why, (s, e.last_error(), why)
            assert untouched(per, out, 2), s
        finally:
            e.set_thread_config(None)


def test_refusals_of_its_own(monkeypatch):
    import krep_amd
    e = krep_amd.load()
    monkeypatch.setenv("KREP_GPU_ASSUME_AVAILABLE", "1")
    monkeypatch.delenv("KREP_GPU_DISABLE", raising=False)
    # positions are not tracked outside -c: the reference's empty-match line is not produced here
    rc, per, out = raw_call(e, abi.Params([b"ab"], track_positions=False), [b"xabx"], [b"one"])
    assert rc == 2 and "track_positions" in e.last_error() and untouched(per, out, 1)
    # NULL arrays with a count
    assert e.lib.krep_gpu_grep_batch(abi.Params([b"ab"]).ref, None, None, 2, None, None, None, None) == 2 and "NULL" in e.last_error()
    # a prefix in one of the single-text structs: the prefixes are per item
    fmt, keep = e.grep_format([b"one"], "lines")
    fmt.line.prefix, fmt.line.prefix_len = b"x:", 2
    arr, n, held = e.batch_items([b"xabx"])
    per, out = (abi.GrepItem * 1)(), abi.GrepOutput(None, 0, 0)
    assert e.lib.krep_gpu_grep_batch(abi.Params([b"ab"]).ref, None, arr, 1, C.byref(fmt), per, C.byref(out), None) == 2
    assert "prefix" in e.last_error() and out.len == 0 and not out.bytes
