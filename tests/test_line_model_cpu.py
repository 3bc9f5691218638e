"""The default output of the reference (every line that holds a match, once) as tests/line_model.py states it, pinned to the
stock CLI (`krep -t 1 --color=never`, oracle/_ref/krep) byte for byte: the rows that show the cursor rule, the 2048-record cap and
-m, and seeded random cases.  Where the CLI cannot be built the digests of its answers in tests/golden/line_output.json stand in.
Also here, without a device: the ctypes mirror of krep_gpu_lines_out_t has the C layout, and both entry points fail loudly."""
import ctypes as C
import os
import subprocess

import pytest

import line_model as lm
import oracle_lib as ol
from krep_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = ol.ref_cli()
STORE = lm.Store()


def check(case, tmp_path, chk):
    mine = lm.grep_output(case.text, case.emitted(chk, abi), lm.FILE + b":", case.max_count)
    rc_mine = 0 if mine else 1
    live = None
    if CLI:
        path = tmp_path / "t.txt"
        path.write_bytes(case.text)
        rc, out = lm.run_cli(CLI, case, path)
        assert out == mine and rc == rc_mine, (case.key, case.pats, case.cli_args(), case.text[:200], out[:200], mine[:200])
        live = lm.digest(rc, out)
    assert lm.digest(rc_mine, mine) == STORE.want(case.key, live), case.key
    if case.want is not None:
        assert mine == lm.FILE + b":" + case.want, case.key
    return bool(mine)


def test_table_rows_match_the_cli(tmp_path, oracle_engine):
    for case in lm.table_cases():
        assert check(case, tmp_path, oracle_engine)
    STORE.save()


def test_random_cases_match_the_cli(tmp_path, oracle_engine):
    cases = lm.random_cases()
    assert len(cases) >= 200
    printed = sum(check(case, tmp_path, oracle_engine) for case in cases)
    STORE.save()
    assert printed > len(cases) // 2
    # the ground the cases are meant to cover
    assert any(c.no_simd for c in cases) and any(not c.cs for c in cases) and any(c.ww for c in cases)
    assert any(len(c.pats) >= 4 for c in cases) and any(c.max_count for c in cases)
    assert any(c.text.endswith(b"\n") for c in cases) and any(not c.text.endswith(b"\n") for c in cases)
    assert any(b"\n\n" in c.text for c in cases)


def test_model_rules_on_hand_made_lists():
    text = b"ab\ncd\n\nef"
    m = lm.Lines(text, [(0, 1), (1, 2), (4, 5), (7, 9)], b"F:")
    assert m.data == b"F:ab\nF:cd\nF:ef\n" and m.spans == [(0, 2), (3, 5), (7, 9)] and m.first_record == [0, 2, 3, 4]
    m = lm.Lines(text, [(0, 1), (1, 2), (4, 5), (7, 9)], b"", 2)
    assert m.data == b"ab\ncd\n" and m.first_record == [0, 2, 3] and m.lines_total == 3
    # a record that starts ON a newline belongs to the line that newline ends and adds nothing; an empty record is passed over
    m = lm.Lines(text, [(0, 1), (2, 4), (3, 3), (6, 8)], b"")
    assert m.data == b"ab\ncd\n\n" and m.spans == [(0, 2), (3, 5), (6, 6)]
    m = lm.Lines(b"a" * 5000, [(i, i + 2) for i in range(4999)], b"")
    assert m.capped == 1 and len(m.data) == 2 * 2048 + (5000 - 2049) + 1


def test_ctypes_struct_has_the_c_layout(tmp_path):
    src = tmp_path / "lines_abi.c"
    src.write_text('#include "krep_gpu.h"\n#include <stdio.h>\n#include <stddef.h>\n'
                   'int main(void) { printf("%zu %zu %zu\\n", sizeof(krep_gpu_lines_out_t), offsetof(krep_gpu_lines_out_t, capped_lines), '
                   'offsetof(krep_gpu_lines_out_t, overflow)); return 0; }\n')
    exe = tmp_path / "lines_abi"
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-pedantic", "-Werror", f"-I{os.path.join(ROOT, 'include')}",
                        str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    sizes = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert sizes == [C.sizeof(abi.LinesOut), abi.LinesOut.capped_lines.offset, abi.LinesOut.overflow.offset], sizes


def test_both_calls_fail_loudly_without_a_device():
    import krep_amd
    e = krep_amd.load()
    if e.device_count() > 0:
        pytest.skip("a GPU is present")
    out = abi.LinesOut()
    text, rec = C.create_string_buffer(b"ab\nab\n"), (C.c_uint64 * 2)(0, 2)
    for call in (lambda: e.lib.krep_gpu_matching_lines(text, 6, rec, 1, abi.SIZE_MAX, None, None, 0, C.byref(out), None),
                 lambda: e.lib.krep_gpu_format_lines(text, 6, rec, 1, abi.SIZE_MAX, b"f:", 2, None, 0, C.byref(out), None)):
        e.lib.krep_gpu_clear_error()
        assert call() == 2 and e.last_error()
    with pytest.raises(krep_amd.KrepGpuError):
        e.format_lines(C.addressof(text), 6, C.addressof(rec), 1)
