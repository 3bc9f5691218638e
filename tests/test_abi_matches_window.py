"""krep_gpu_format_matches_window in the library and in Python, without a device: the symbol is exported, the ctypes twins of
krep_gpu_matches_window_t / krep_gpu_matches_window_out_t have the C layout of include/krep_gpu.h, and the call fails loudly.

The layout (LP64): krep_gpu_matches_window_t is 56 bytes — global_base 0, global_len 8, count_to 16, newlines_before 24,
last_newline1 32, stale_line 40, stale_rule 48, reserved 52 (an int that is spelled out, so the struct has no implicit padding);
krep_gpu_matches_window_out_t is 40 bytes — matches 0 (items 0, out_bytes 8, overflow 16), newlines_before_count_to 24,
stale_line 32."""
import ctypes as C
import os
import subprocess

from krep_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_the_call_and_python_has_its_twins():
    import krep_amd
    e = krep_amd.load()
    assert hasattr(e.lib, "krep_gpu_format_matches_window")
    assert callable(getattr(e, "format_matches_window", None))
    assert callable(getattr(krep_amd.engine.Plan, "grep_only_matching_pieces", None))


def test_ctypes_structs_have_the_c_layout(tmp_path):
    win = ("global_base", "global_len", "count_to", "newlines_before", "last_newline1", "stale_line", "stale_rule", "reserved")
    out = ("matches", "newlines_before_count_to", "stale_line")
    prints = ["sizeof(krep_gpu_matches_window_t)"] + [f"offsetof(krep_gpu_matches_window_t, {f})" for f in win]
    prints += ["sizeof(krep_gpu_matches_window_out_t)"] + [f"offsetof(krep_gpu_matches_window_out_t, {f})" for f in out]
    prints += ["offsetof(krep_gpu_matches_window_out_t, matches.out_bytes)", "offsetof(krep_gpu_matches_window_out_t, matches.overflow)"]
    src = tmp_path / "matches_window_abi.c"
    src.write_text('#include "krep_gpu.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void) {\n' +
                   "".join(f'    printf("%zu\\n", (size_t){p});\n' for p in prints) + "    return 0;\n}\n")
    exe = tmp_path / "matches_window_abi"
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-pedantic", "-Werror", f"-I{os.path.join(ROOT, 'include')}",
                        str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    sizes = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    want = [C.sizeof(abi.MatchesWindow)] + [getattr(abi.MatchesWindow, f).offset for f in win]
    want += [C.sizeof(abi.MatchesWindowOut)] + [getattr(abi.MatchesWindowOut, f).offset for f in out]
    want += [abi.MatchesWindowOut.matches.offset + abi.MatchesOut.out_bytes.offset,
             abi.MatchesWindowOut.matches.offset + abi.MatchesOut.overflow.offset]
    assert sizes == want, (sizes, want)
    assert sizes == [56, 0, 8, 16, 24, 32, 40, 48, 52, 40, 0, 24, 32, 8, 16]
    # the fields of the window in the order of the header: a positional constructor fills them as the C initialiser would
    w = abi.MatchesWindow(1, 2, 3, 4, 5, 6, 7)
    assert (w.global_base, w.global_len, w.count_to, w.newlines_before, w.last_newline1, w.stale_line, w.stale_rule) == (1, 2, 3, 4, 5, 6, 7)


def test_the_call_fails_loudly_without_a_device():
    import pytest
    import krep_amd
    e = krep_amd.load()
    if e.device_count() > 0:
        return  # (with a device the call is tests/test_gpu_matches_window.py's)
    out = abi.MatchesWindowOut()
    text, rec = C.create_string_buffer(b"ab\nab\n"), (C.c_uint64 * 2)(0, 2)
    win = abi.MatchesWindow(0, 6, 6, 0, 6, 0, 0)
    e.lib.krep_gpu_clear_error()
    assert e.lib.krep_gpu_format_matches_window(text, 6, C.byref(win), rec, 1, abi.SIZE_MAX, None, None, 0, C.byref(out), None) == 2
    assert e.last_error()
    with pytest.raises(krep_amd.KrepGpuError):
        e.format_matches_window(C.addressof(text), 6, win, C.addressof(rec), 1, fmt=abi.MatchFormat(b"f:"))
    plan_less = krep_amd.engine.Plan(e, None, abi.Params([b"ab"]), only_matching=False)
    with pytest.raises(krep_amd.KrepGpuError, match="only_matching"):
        plan_less.grep_only_matching_pieces(b"ab\nab\n", 4)
