"""The -o output of the reference (one FILE:LINE:match per match) as tests/only_matching_model.py states it, pinned to the stock
CLI (`krep -t 1 -o --color=never`, and `--color=always` on the table and every fourth random case; oracle/_ref/krep) byte for
byte: the rows that show the stale line number behind the last newline of a list of more than 10 records, the blank for a
newline inside a match, -m, and seeded random cases.  Where the CLI cannot be built the digests of its answers in
tests/golden/only_matching_output.json stand in.  Also here, without a device: the library exports krep_gpu_format_matches, the
ctypes mirrors of its two structs have the C layout, the call fails loudly, and Plan.grep_only_matching exists."""
import ctypes as C
import os
import subprocess

import pytest

import only_matching_model as om
import oracle_lib as ol
from krep_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = ol.ref_cli()
STORE = om.Store()


def check(case, tmp_path, chk, color):
    """-> (records in the list, of them behind the last newline of a list of more than 10)"""
    emitted = case.emitted(chk, abi)
    for col in (False, True) if color else (False,):
        mine = om.grep_o_output(case.text, emitted, om.FILE, col, case.max_count)
        rc_mine = 0 if mine else 1
        live = None
        if CLI:
            path = tmp_path / "t.txt"
            path.write_bytes(case.text)
            rc, out = om.run_cli(CLI, case, path, col)
            assert out == mine and rc == rc_mine, (case.key, case.pats, case.cli_args(col), case.text[:200], out[:200], mine[:200])
            live = om.digest(rc, out)
        assert om.digest(rc_mine, mine) == STORE.want(case.key + ("/color" if col else ""), live), case.key
        if case.want is not None and not col:
            assert mine == case.want, (case.key, mine)
    recs = om.lm.cut_to_max_count(emitted, case.max_count)
    return len(recs), om.stale_records(case.text, recs)


def test_table_rows_match_the_cli(tmp_path, oracle_engine):
    for case in om.table_cases():
        n, _ = check(case, tmp_path, oracle_engine, True)
        assert n
    STORE.save()


def test_random_cases_match_the_cli(tmp_path, oracle_engine):
    cases = om.random_cases()
    assert len(cases) >= 240
    seen = [check(case, tmp_path, oracle_engine, idx % 4 == 0) for idx, case in enumerate(cases)]
    STORE.save()
    # the ground the cases are meant to cover: both sides of the threshold of 10 records, and stale numbers
    assert sum(1 for n, _ in seen if 1 <= n <= 10) >= 40 and sum(1 for n, _ in seen if n > 10) >= 40, seen
    print("records 1..10 / more / with stale numbers:", sum(1 for n, _ in seen if 1 <= n <= 10), sum(1 for n, _ in seen if n > 10),
          sum(1 for _, stale in seen if stale))
    assert sum(1 for _, stale in seen if stale) >= 30
    assert any(c.no_simd for c in cases) and any(not c.cs for c in cases) and any(c.ww for c in cases)
    assert any(len(c.pats) >= 4 for c in cases) and {c.max_count for c in cases} >= {None, 1, 2, 3, 7, 10, 11}
    k = len(cases) // 3
    assert sum(c.text.endswith(b"\n") for c in cases) >= k and sum(not c.text.endswith(b"\n") for c in cases) >= k


def test_model_rules_on_hand_made_lists():
    text = b"ab\ncd\n\nef"
    recs = [(0, 1), (1, 2), (2, 4), (4, 5), (7, 9)]
    assert om.line_numbers(text, recs) == [1, 1, 1, 2, 4]  # a start ON a newline: the line that newline ends
    assert om.only_matching_output(text, recs, om.strings(b"F")) == b"F:1:a\nF:1:b\nF:1: c\nF:2:d\nF:4:ef\n"
    assert om.only_matching_output(text, recs, om.strings(None), 2) == b"1:a\n1:b\n"
    many = [(0, 1)] * 6 + [(4, 5)] * 3 + [(7, 8), (8, 9)]  # 11 records: the two behind the last newline print the 2 in front
    assert om.line_numbers(text, many) == [1] * 6 + [2] * 5 and om.stale_records(text, many) == 2
    assert om.line_numbers(text, many[:10]) == [1] * 6 + [2] * 3 + [4] and om.stale_records(text, many[:10]) == 0
    assert om.line_numbers(text, [(7, 8)] * 11) == [1] * 11
    assert om.line_numbers(b"abab", [(0, 1)] * 11 + [(2, 3)]) == [1] * 12
    # max_items cuts the output, not the list: the threshold looks at n
    assert om.only_matching_output(text, many, om.strings(None), 11)[-8:] == b"2:e\n2:f\n"
    col = om.only_matching_output(text, recs[:1], om.strings(b"F", True))
    assert col == b"\033[1;38;5;81mF\033[0m\033[38;5;244m:\033[1;38;5;111m1:\033[0m\033[1;38;5;222ma\033[0m\n"


def test_library_exports_the_call_and_python_has_its_twin():
    import krep_amd
    e = krep_amd.load()
    assert hasattr(e.lib, "krep_gpu_format_matches")
    assert callable(getattr(krep_amd.engine.Plan, "grep_only_matching", None)) and callable(getattr(e, "format_matches", None))
    f = krep_amd.engine.match_format(b"F", True)
    assert tuple(C.string_at(p, n) for p, n in ((f.prefix, f.prefix_len), (f.before_number, f.before_number_len),
                                                (f.after_number, f.after_number_len), (f.after_match, f.after_match_len))) == \
        om.strings(b"F", True)
    assert krep_amd.engine.match_format(None).prefix_len == 0 and krep_amd.engine.match_format(b"F").prefix == b"F:"


def test_ctypes_structs_have_the_c_layout(tmp_path):
    src = tmp_path / "matches_abi.c"
    src.write_text('#include "krep_gpu.h"\n#include <stdio.h>\n#include <stddef.h>\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(krep_gpu_match_format_t), '
                   'offsetof(krep_gpu_match_format_t, after_number), offsetof(krep_gpu_match_format_t, after_match_len), '
                   'sizeof(krep_gpu_matches_out_t), offsetof(krep_gpu_matches_out_t, out_bytes), '
                   'offsetof(krep_gpu_matches_out_t, overflow)); return 0; }\n')
    exe = tmp_path / "matches_abi"
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-pedantic", "-Werror", f"-I{os.path.join(ROOT, 'include')}",
                        str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    sizes = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert sizes == [C.sizeof(abi.MatchFormat), abi.MatchFormat.after_number.offset, abi.MatchFormat.after_match_len.offset,
                     C.sizeof(abi.MatchesOut), abi.MatchesOut.out_bytes.offset, abi.MatchesOut.overflow.offset], sizes


def test_the_call_fails_loudly_without_a_device():
    import krep_amd
    e = krep_amd.load()
    if e.device_count() > 0:
        pytest.skip("a GPU is present")
    out = abi.MatchesOut()
    text, rec = C.create_string_buffer(b"ab\nab\n"), (C.c_uint64 * 2)(0, 2)
    e.lib.krep_gpu_clear_error()
    assert e.lib.krep_gpu_format_matches(text, 6, rec, 1, abi.SIZE_MAX, None, None, 0, C.byref(out), None) == 2 and e.last_error()
    with pytest.raises(krep_amd.KrepGpuError):
        e.format_matches(C.addressof(text), 6, C.addressof(rec), 1, fmt=abi.MatchFormat(b"f:"))
