"""krep_gpu_format_lines_ex in the library and in Python, without a device: the symbol is exported, the ctypes twin of
krep_gpu_line_format_t has the C layout, and line_format() composes the reference's strings."""
import ctypes as C
import os
import subprocess

import color_line_model as cm
from krep_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_the_call_and_python_has_its_twin():
    import krep_amd
    e = krep_amd.load()
    assert hasattr(e.lib, "krep_gpu_format_lines_ex")
    assert callable(getattr(e, "format_lines_ex", None))
    for name in (None, b"F"):
        f = krep_amd.engine.line_format(name, True)
        assert tuple(C.string_at(p, n) for p, n in ((f.prefix, f.prefix_len), (f.before_match, f.before_match_len),
                                                    (f.after_match, f.after_match_len), (f.line_close, f.line_close_len))) == \
            cm.strings(name, True)
    assert krep_amd.engine.COLOR_TEXT == b"\033[38;5;252m"
    assert krep_amd.engine.line_format(None).prefix_len == 0 and krep_amd.engine.line_format(b"F").prefix == b"F:"
    assert krep_amd.engine.line_format(b"F").before_match_len == 0


def test_ctypes_struct_has_the_c_layout(tmp_path):
    src = tmp_path / "line_format_abi.c"
    src.write_text('#include "krep_gpu.h"\n#include <stdio.h>\n#include <stddef.h>\n'
                   'int main(void) { printf("%zu %zu %zu\\n", sizeof(krep_gpu_line_format_t), '
                   'offsetof(krep_gpu_line_format_t, after_match), offsetof(krep_gpu_line_format_t, line_close_len)); return 0; }\n')
    exe = tmp_path / "line_format_abi"
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-pedantic", "-Werror", f"-I{os.path.join(ROOT, 'include')}",
                        str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    sizes = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert sizes == [C.sizeof(abi.LineFormat), abi.LineFormat.after_match.offset, abi.LineFormat.line_close_len.offset], sizes


def test_the_call_fails_loudly_without_a_device():
    import pytest
    import krep_amd
    e = krep_amd.load()
    if e.device_count() > 0:
        pytest.skip("a GPU is present")
    out = abi.LinesOut()
    text, rec = C.create_string_buffer(b"ab\nab\n"), (C.c_uint64 * 2)(0, 2)
    e.lib.krep_gpu_clear_error()
    assert e.lib.krep_gpu_format_lines_ex(text, 6, rec, 1, abi.SIZE_MAX, None, None, 0, C.byref(out), None) == 2 and e.last_error()
    with pytest.raises(krep_amd.KrepGpuError):
        e.format_lines_ex(C.addressof(text), 6, C.addressof(rec), 1, fmt=abi.LineFormat(b"f:"))
