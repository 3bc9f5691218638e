"""CPU-side checks of the batch entry points (include/krep_gpu.h "a batch of texts in one scan"): the two symbols are exported,
the three structs have the layout a C host compiles, and without a device krep_gpu_search_batch fails loudly — status 2, a reason,
nothing written to `results`, nothing appended to `records`."""
import ctypes as C
import os
import subprocess

import pytest

import batch_model as bm
from krep_amd import abi, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import torch  # noqa: F401  (first, as krep_amd.Engine does: tests/test_abi_exports.py says why)
    return C.CDLL(build.build())


def test_the_batch_symbols_are_exported(lib):
    for n in ("krep_gpu_batch_can_accelerate", "krep_gpu_search_batch", "krep_gpu_debug_batch_pack_limit", "krep_gpu_debug_batch_times",
              "krep_gpu_debug_batch_fill_host", "krep_gpu_debug_batch_rebase_launches"):
        assert hasattr(lib, n), n
    boundary = open(os.path.join(ROOT, "include", "krep_gpu.h")).read()
    assert "krep_gpu_search_batch" in boundary and "krep_gpu_batch_can_accelerate" in boundary
    hooks = open(os.path.join(ROOT, "include", "krep_gpu_debug.h")).read()
    assert "krep_gpu_debug_batch_pack_limit" in hooks and "krep_gpu_debug_batch_fill_host" in hooks


def test_struct_layouts_match_a_c11_probe(tmp_path):
    src = tmp_path / "batch_abi.c"
    src.write_text('#include "krep_gpu.h"\n#include <stdio.h>\n#include <stddef.h>\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(krep_gpu_batch_item_t), '
                   'offsetof(krep_gpu_batch_item_t, len), sizeof(krep_gpu_batch_result_t), offsetof(krep_gpu_batch_result_t, first_record), '
                   'offsetof(krep_gpu_batch_result_t, n_records), sizeof(krep_gpu_batch_info_t), offsetof(krep_gpu_batch_info_t, scans), '
                   'offsetof(krep_gpu_batch_info_t, total_records), offsetof(krep_gpu_batch_info_t, kernel_ms), '
                   'sizeof(krep_gpu_batch_result_t[3])); return 0; }\n')
    exe = tmp_path / "batch_abi"
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-pedantic", "-Werror", f"-I{os.path.join(ROOT, 'include')}",
                        str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    want = [C.sizeof(abi.BatchItem), abi.BatchItem.len.offset, C.sizeof(abi.BatchResult), abi.BatchResult.first_record.offset,
            abi.BatchResult.n_records.offset, C.sizeof(abi.BatchInfo), abi.BatchInfo.scans.offset, abi.BatchInfo.total_records.offset,
            abi.BatchInfo.kernel_ms.offset, 3 * C.sizeof(abi.BatchResult)]
    assert got == want, (got, want)
    assert got[:6] == [16, 8, 24, 8, 16, 32]


def test_without_a_device_the_batch_call_fails_loudly_and_writes_nothing(monkeypatch):
    import krep_amd
    e = krep_amd.load()
    monkeypatch.setenv("KREP_GPU_DISABLE", "1")  # no usable device, whatever this host has
    monkeypatch.delenv("KREP_GPU_ASSUME_AVAILABLE", raising=False)
    p = abi.Params([b"ab"])
    assert not e.batch_can_accelerate(p) and e.last_error()
    rc, res, n, first = bm.raw_call(e, p, [b"xabx", b"", b"ab"])
    assert rc == 2 and e.last_error()
    assert res == [(bm.POISON,) * 3] * 3 and n == 1 and first == 77
    with pytest.raises(krep_amd.KrepGpuError):
        e.search_batch(p, [b"xabx", b"", b"ab"])


def test_a_refused_search_fails_before_any_device_work(monkeypatch):
    import krep_amd
    e = krep_amd.load()
    monkeypatch.setenv("KREP_GPU_ASSUME_AVAILABLE", "1")  # (the rule is host logic: the refusal comes before the device is asked)
    monkeypatch.delenv("KREP_GPU_DISABLE", raising=False)
    for p, reason in ((abi.Params([b"ab"], max_count=5), "max_count"), (abi.Params([b"a\nb"]), "holds '\\n'")):
        assert not e.batch_can_accelerate(p) and reason in e.last_error()
        rc, res, n, first = bm.raw_call(e, p, [b"xabx", b"a\nb"])
        assert rc == 2 and reason in e.last_error(), e.last_error()
        assert res == [(bm.POISON,) * 3] * 2 and n == 1 and first == 77
    # NULL items with a count, and an item with a NULL text and a length, are refused as well
    rc = e.lib.krep_gpu_search_batch(abi.Params([b"ab"]).ref, None, None, 2, None, None, None)
    assert rc == 2 and "NULL" in e.last_error()
