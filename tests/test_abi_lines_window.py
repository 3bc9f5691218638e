"""krep_gpu_format_lines_window in the library and in Python, without a device: the symbol is exported, and the ctypes twins of
krep_gpu_lines_window_t / krep_gpu_lines_window_out_t have the C layout of include/krep_gpu.h."""
import ctypes as C
import os
import subprocess

from krep_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_the_call_and_python_has_its_twin():
    import krep_amd
    e = krep_amd.load()
    assert hasattr(e.lib, "krep_gpu_format_lines_window")
    assert callable(getattr(e, "format_lines_window", None))
    assert callable(getattr(krep_amd.engine.Plan, "grep_lines_pieces", None))


def test_ctypes_structs_have_the_c_layout(tmp_path):
    win = ("global_base", "global_len", "own_lo", "own_hi", "records_hi")
    out = ("lines", "incomplete_line_start1", "incomplete_first_record")
    prints = ["sizeof(krep_gpu_lines_window_t)"] + [f"offsetof(krep_gpu_lines_window_t, {f})" for f in win]
    prints += ["sizeof(krep_gpu_lines_window_out_t)"] + [f"offsetof(krep_gpu_lines_window_out_t, {f})" for f in out]
    prints += ["offsetof(krep_gpu_lines_window_out_t, lines.overflow)"]
    src = tmp_path / "lines_window_abi.c"
    src.write_text('#include "krep_gpu.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void) {\n' +
                   "".join(f'    printf("%zu\\n", (size_t){p});\n' for p in prints) + "    return 0;\n}\n")
    exe = tmp_path / "lines_window_abi"
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-pedantic", "-Werror", f"-I{os.path.join(ROOT, 'include')}",
                        str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    sizes = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    want = [C.sizeof(abi.LinesWindow)] + [getattr(abi.LinesWindow, f).offset for f in win]
    want += [C.sizeof(abi.LinesWindowOut)] + [getattr(abi.LinesWindowOut, f).offset for f in out]
    want += [abi.LinesWindowOut.lines.offset + abi.LinesOut.overflow.offset]
    assert sizes == want, (sizes, want)
    assert sizes[0] == 40 and sizes[6] == 56


def test_the_call_fails_loudly_without_a_device():
    import pytest
    import krep_amd
    e = krep_amd.load()
    if e.device_count() > 0:
        return  # (with a device the call is tests/test_gpu_lines_window.py's)
    out = abi.LinesWindowOut()
    text, rec = C.create_string_buffer(b"ab\nab\n"), (C.c_uint64 * 2)(0, 2)
    win = abi.LinesWindow(0, 6, 0, 6, 6)
    e.lib.krep_gpu_clear_error()
    assert e.lib.krep_gpu_format_lines_window(text, 6, C.byref(win), rec, 1, abi.SIZE_MAX, None, None, 0, C.byref(out), None) == 2
    assert e.last_error()
    with pytest.raises(krep_amd.KrepGpuError):
        e.format_lines_window(C.addressof(text), 6, win, C.addressof(rec), 1, fmt=abi.LineFormat(b"f:"))
