"""The table and the texts of tests/regex_output_cases.py, pinned without a GPU: every row is accepted by the compiler the table
names and split as it says; every planted match is a record of the model, so a GPU sweep cannot pass by planting nothing; the records
equal the compiled reference's regex_search and the bytes of the three output models equal the stock CLI (`krep -t 1 -E`, four output
modes, -m for the single-pattern rows) byte for byte where oracle/_ref is built.  The digests of the CLI's answers in
tests/golden/regex_output.json stand in where it is not."""
import numpy as np
import pytest

import oracle_lib as ol
import regex_alt_model
import regex_output_cases as rc
import regex_ref
from krep_amd import abi
from krep_amd.engine import KrepGpuError

CLI = ol.ref_cli()
STORE = rc.Store()
VARIANTS = (True, False)  # the text ends in a newline / it does not


@pytest.fixture(autouse=True, scope="module")
def _c_locale():
    """the reference runs in the C locale (it never calls setlocale()); Python's start-up put the process into the environment's"""
    with regex_ref.c_locale():
        yield


@pytest.fixture(scope="module")
def eng():
    import krep_amd
    return krep_amd.load()


def rows_of(family):
    return [r for r in rc.ROWS if r.family == family]


def refused(call, p) -> bool:
    try:
        call(p)
    except KrepGpuError:
        return True
    return False


def test_every_row_is_taken_by_the_compiler_the_table_names(eng):
    assert len({r.key for r in rc.ROWS}) == len(rc.ROWS) and {r.family for r in rc.ROWS} == set(rc.FAMILIES)
    for row in rc.ROWS:
        p = rc.params(row)
        if row.family == "basic":
            info = eng.regex_compile(p)
            got = (info.L, 0, 0, bool(info.self_overlap))
        elif row.family == "anchored":
            assert refused(eng.regex_compile, p), row.key
            info = eng.regex_compile_anchored(p)
            got = (info.seq.L, info.bol, info.eol, bool(info.seq.self_overlap))
        elif row.family == "alt":
            assert refused(eng.regex_compile_anchored, p), row.key
            info = eng.regex_compile_alt(p)
            got = (info.Lmax, 0, 0, bool(info.cross_overlap))
            assert info.n_branches == len(regex_alt_model.branches(row.pats, row.cs)), row.key
        else:
            assert refused(eng.regex_compile_anchored, p) and refused(eng.regex_compile_alt, p), row.key
            info = eng.regex_compile_ext(p)
            got = (info.alt.Lmax, info.bol, info.eol, bool(info.alt.cross_overlap))
        assert got == (row.Lmax, row.bol, row.eol, row.mode == rc.WHOLE), (row.key, got)
        mode = {abi.SPLIT_PIECES: rc.PIECES, abi.SPLIT_WHOLE: rc.WHOLE}[eng.split_mode(p, rc.TOTAL)]
        cfg = eng.default_config()
        cfg.only_matching = 1
        eng.set_thread_config(cfg)
        try:
            under_o = eng.split_mode(p, rc.TOTAL)
        finally:
            eng.set_thread_config(None)
        assert mode == row.mode and under_o == (abi.SPLIT_PIECES if row.mode == rc.PIECES else abi.SPLIT_WHOLE), row.key


def test_longest_match_follows_the_compilers_not_the_pattern_string(eng):
    """Plan.longest_match() (host only: no plan handle is needed): L / Lmax of the compiler that takes the search, + 1 for the byte a $
    looks at; the longest pattern of a literal plan, as before"""
    from krep_amd.engine import Plan
    for row in rc.ROWS:
        assert Plan(eng, None, rc.params(row)).longest_match() == row.Lmax + row.eol, row.key
    assert Plan(eng, None, abi.Params([b"abc", b"hello", b"q[a-c]{15}"])).longest_match() == 10
    assert Plan(eng, None, abi.Params([b"q[a-c]{15}"])).longest_match() == 10  # (not -E: ten literal bytes)
    with pytest.raises(KrepGpuError):
        Plan(eng, None, abi.Params([b"a.*b"], regex=True)).longest_match()  # (all three compilers refuse it: no plan exists either)


def test_the_table_holds_the_kinds_of_rows_the_output_drivers_have_to_meet():
    by = rc.BY_KEY
    longer = [r for r in rc.ROWS if r.Lmax > rc.string_len(r) and r.mode == rc.PIECES]
    assert {r.family for r in longer} == set(rc.FAMILIES)  # a match longer than the pattern string, from every compiler
    assert by["basic/q16"].Lmax == 16 and rc.string_len(by["basic/q16"]) == 10 and by["anchor/bol-q15"].Lmax == 15
    assert by["basic/word"].Lmax < rc.string_len(by["basic/word"])
    assert not by["basic/icase"].cs and sum(1 for r in rc.ROWS if not r.cs) == 1
    assert [r.key for r in rc.ROWS if not rc.single(r)] == ["alt/two-e"]
    whole = {r.key for r in rc.ROWS if r.mode == rc.WHOLE}
    assert whole == {"basic/overlap", "alt/animals", "alt/longest", "ext/percent"}
    # different lengths in one list: the strings of these rows differ in length
    for key in ("alt/1-and-16", "ext/colour", "ext/percent", "alt/longest", "ext/inner", "ext/api", "ext/bol-alt", "ext/branch16"):
        assert len({len(p) for p in by[key].plants}) >= 2, key
    assert {(r.bol, r.eol) for r in rc.ROWS} == {(0, 0), (1, 0), (0, 1), (1, 1)}
    assert any(b"\n" in p for p in by["basic/space"].plants)
    # a match that is longer than its pattern string AND crosses the end of its line: its line is complete where it is not
    row = by["basic/q16-newline"]
    assert row.Lmax > rc.string_len(row) and b"\n" in row.plants[0] and len(row.plants[0]) == row.Lmax
    assert rc.P_UNIT < rc.TOTAL <= 200 * 1024 and rc.TOTAL >= 64 * 1024 and rc.TOTAL > 3 * rc.P_UNIT


@pytest.mark.parametrize("family", rc.FAMILIES)
def test_every_planted_match_is_a_record(family):
    for row in rows_of(family):
        for nl in VARIANTS:
            text, raw, plants, rec = rc.case(row.key, nl)
            have = set(rec)
            assert text.size == rc.TOTAL and raw.endswith(b"\n") == nl
            assert max(len(line) for line in raw.split(b"\n")) <= 12500
            for p in plants:
                if p.kind != "sprinkled":  # (a sprinkled shorter string may grow by the byte behind it: ab -> abc)
                    assert (p.start, p.end) in have and p.end - p.start == row.Lmax, (row.key, nl, p)
            sweep = [p for p in plants if p.kind == "sweep"]
            assert [p.k for p in sweep] == list(range(-1, row.Lmax + 2)) and len({p.cut for p in sweep}) == len(sweep)
            assert all(p.cut % rc.P_SMALL == 0 and p.start == p.cut - p.k for p in sweep)
            assert [p.cut - p.start for p in plants if p.kind == "unit"] == [1, max(row.Lmax - 1, 1), max(row.Lmax // 2, 1)]
            assert rec[0][0] == 0 and rec[-1][1] == rc.TOTAL - int(nl)
            lines = {raw.rfind(b"\n", 0, s) for s, _ in rec}
            assert len(rec) >= 20 and len(lines) >= 10, (row.key, len(rec), len(lines))
            if not (row.bol and row.eol):
                a, z = rc.LONG_LINE
                z = raw.find(b"\n", a)  # (the newline inside a planted ab\ncd ends the line two bytes into the match)
                assert raw[a - 1] == 10 and rc.LONG_LINE[1] - row.Lmax <= z <= rc.LONG_LINE[1] and z - a > 3 * rc.P_SMALL
                inside = [(s, e) for s, e in rec if a <= s <= z]
                assert len(inside) == 1 and (inside[0][0] == a if row.bol else z - 20 <= inside[0][0] < z), (row.key, inside)
            if not row.bol:
                records_hi = rc.EDGE_CUT + rc.HALO - (row.Lmax + row.eol - 1)
                a = raw.rfind(b"\n", 0, records_hi) + 1
                first = min(s for s, _ in rec if s >= a)
                assert rc.EDGE_CUT - rc.P_SMALL <= a < rc.EDGE_CUT and records_hi - row.Lmax <= first < records_hi, (row.key, a, first)
            if regex_ref.available():
                count, ref = regex_ref.call(regex_alt_model.joined(row.pats), text, case_sensitive=row.cs)
                assert count == len(rec) and np.array_equal(ref, np.asarray(rec, dtype=np.uint64)), ("model != reference", row.key, nl)
                for mc in (1, 7):
                    cut = regex_ref.call(regex_alt_model.joined(row.pats), text, case_sensitive=row.cs, max_count=mc)[1]
                    assert np.array_equal(cut, rc.records(row, text, mc)) and np.array_equal(cut, ref[:mc]), (row.key, mc)


@pytest.mark.parametrize("family", rc.FAMILIES)
def test_model_bytes_equal_the_stock_cli(family, tmp_path):
    """the three output models on the records of the regex models against `krep -t 1 -E [-o] --color=never|always [-m N]`"""
    asked = 0
    for row in rows_of(family):
        for nl in VARIANTS:
            text, raw, plants, rec = rc.case(row.key, nl)
            path = tmp_path / "t.txt"
            if CLI:
                path.write_bytes(raw)
            counts = (None,) + ((1, 7, len(rec) + 5) if rc.single(row) and nl else ())
            for mode in rc.MODES:
                for mc in counts:
                    mine = rc.expected(raw, rec, mode, rc.FILE, mc)
                    rc_mine = 0 if mine else 1
                    live = None
                    if CLI:
                        code, out = rc.run_cli(CLI, row, mode, path, mc)
                        assert out == mine and code == rc_mine, (row.key, nl, mode, mc, len(out), len(mine))
                        live = rc.digest(code, out)
                    key = f"{row.key}/{'nl' if nl else 'open'}/{mode}/m{'-' if mc is None else mc if mc <= 7 else 'all'}"
                    assert rc.digest(rc_mine, mine) == STORE.want(key, live), key
                    asked += 1
                    if mc is None:
                        assert mine.count(b"\n") == (len(rec) if mode.startswith("o") else len({raw.rfind(b"\n", 0, s) for s, _ in rec}))
    STORE.save()
    assert asked >= 8 * len(rows_of(family))
