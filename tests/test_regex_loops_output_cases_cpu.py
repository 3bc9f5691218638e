"""The table and the texts of tests/regex_loops_output_cases.py, pinned without a GPU: every row is taken by the loops compiler and by
no older one; with the switch on Plan.longest_match() says 4097 and the split mode is WHOLE (with the switch off it raises: no plan
exists); every text holds what its docstring promises, so that no GPU test passes by planting nothing; the bytes of the three output
models on the reference's records equal the stock CLI (`krep -t 1 -E`, four output modes, -m for the single-pattern rows) byte for
byte where oracle/_ref is built.  The digests of the CLI's answers in tests/golden/regex_loops_output.json stand in where it is not."""
import pytest

import only_matching_model as om
import oracle_lib as ol
import regex_loops_output_cases as lc
import regex_ref
from krep_amd import abi
from krep_amd.engine import KrepGpuError, Plan

CLI = ol.ref_cli()
STORE = lc.Store()
VARIANTS = (True, False)  # the text ends in a newline / it does not
EXTRA = [b"^#+ "]         # taken by the loops compiler too; no row of its own


@pytest.fixture(autouse=True, scope="module")
def _c_locale():
    """the reference runs in the C locale (it never calls setlocale()); Python's start-up put the process into the environment's"""
    with regex_ref.c_locale():
        yield


@pytest.fixture(scope="module")
def eng():
    import krep_amd
    e = krep_amd.load()
    assert not e.get_regex_loops()
    yield e
    e.set_regex_loops(False)
    e.set_thread_config(None)


def refused(call, p) -> bool:
    try:
        call(p)
    except KrepGpuError:
        return True
    return False


def searches():
    """(patterns, case_sensitive) of every row, of the cap texts and of EXTRA, each in both cases"""
    pats = [tuple(r.pats) for r in lc.ROWS] + [tuple(c.pats) for c in lc.CAPS] + [(p,) for p in EXTRA]
    return [(list(p), cs) for p in dict.fromkeys(pats) for cs in (True, False)]


def test_every_row_is_taken_by_the_loops_compiler_and_by_no_older_one(eng):
    assert len({r.key for r in lc.ROWS}) == len(lc.ROWS) == 14
    assert [r.key for r in lc.ROWS if not r.cs] == ["colou*r-i"] and [r.key for r in lc.ROWS if not lc.single(r)] == ["two-e"]
    assert {(r.bol, r.eol) for r in lc.ROWS} == {(0, 0), (1, 0), (0, 1), (1, 1)}
    for pats, cs in searches():
        p = abi.Params(pats, regex=True, case_sensitive=cs)
        eng.regex_compile_loops(p)  # (raises its refusal)
        for older in (eng.regex_compile, eng.regex_compile_anchored, eng.regex_compile_alt, eng.regex_compile_ext):
            assert refused(older, p), (pats, cs, older.__name__)


def test_longest_match_is_4097_and_the_split_mode_is_whole_with_the_switch_on(eng):
    """the `4096 + 1` branch of Plan.longest_match(): host only, no plan handle is needed"""
    cfg = eng.default_config()
    cfg.only_matching = 1
    for pats, cs in searches():
        p = abi.Params(pats, regex=True, case_sensitive=cs)
        assert not eng.get_regex_loops()
        with pytest.raises(KrepGpuError):
            Plan(eng, None, p).longest_match()  # (switch off: no compiler a search asks takes it, no plan exists either)
        eng.set_regex_loops(True)
        try:
            assert Plan(eng, None, p).longest_match() == lc.LONGEST == 4097, (pats, cs)
            assert Plan(eng, None, p, only_matching=True).longest_match() == 4097, (pats, cs)
            assert eng.split_mode(p, lc.TOTAL) == abi.SPLIT_WHOLE, (pats, cs)
            eng.set_thread_config(cfg)
            try:
                assert eng.split_mode(p, lc.TOTAL) == abi.SPLIT_WHOLE, (pats, cs, "-o")
            finally:
                eng.set_thread_config(None)
        finally:
            eng.set_regex_loops(False)
    # what the older compilers take keeps its own answer under the switch, and what nobody takes still raises
    eng.set_regex_loops(True)
    try:
        assert Plan(eng, None, abi.Params([b"q[a-c]{15}"], regex=True)).longest_match() == 16
        assert Plan(eng, None, abi.Params([b"colou?r"], regex=True)).longest_match() == 6
        assert Plan(eng, None, abi.Params([b"q[a-c]{15}"])).longest_match() == 10
        with pytest.raises(KrepGpuError):
            Plan(eng, None, abi.Params([b"(ab)+"], regex=True)).longest_match()  # (an unbounded quantifier behind a group)
    finally:
        eng.set_regex_loops(False)


@pytest.mark.parametrize("key", [r.key for r in lc.ROWS])
def test_every_text_holds_what_it_promises(key):
    row = lc.BY_KEY[key]
    assert lc.records(row, lc.decoy_text(row)).shape[0] == 0, "a decoy line holds a match"
    assert len(row.decoys) >= 1 and len(row.make(row.shortest)) == row.shortest
    for nl in VARIANTS:
        text, raw, plants, rec = lc.case(key, nl)
        have = set(rec)
        assert text.size == lc.TOTAL == 65536 and raw.endswith(b"\n") == nl
        lines = raw.split(b"\n")
        assert max(len(x) for x in lines) == lc.LINE_MAX and sum(1 for x in lines if len(x) == lc.LINE_MAX) == 2
        assert len(rec) >= 20 and len({raw.rfind(b"\n", 0, s) for s, _ in rec}) >= 10, (key, len(rec))
        for p in plants:  # every planted match is a record
            assert (p.start, p.end) in have, (key, nl, p)
        longest = max(e - s for s, e in rec)
        assert longest <= lc.LINE_MAX and (longest >= 1000 or not row.must_long), (key, longest)
        # lengths of 1 (or the grammar's shortest), 17, 1000, 3500 and 3800 bytes in one list
        lengths = {e - s for s, e in rec}
        assert {row.shortest, 17, 1000, 3500, 3800} <= lengths, (key, sorted(lengths)[-6:])
        # the two lines of 4096 bytes: a match in the first bytes of one, in the last 20 bytes of the other
        at = [p for p in plants if p.kind == "line4096"]
        a, b = (raw.rfind(b"\n", 0, p.start) + 1 for p in at)
        assert raw[a + lc.LINE_MAX] == 10 and raw[b + lc.LINE_MAX] == 10 and at[0].start == a and at[1].end == b + lc.LINE_MAX
        assert at[1].start >= b + lc.LINE_MAX - 20 or row.bol
        # records that touch, and a record that is its whole line
        if row.touching:
            t = [p for p in plants if p.kind == "touch"]
            assert len(t) >= 2 and all(x.end == y.start for x, y in zip(t, t[1:]))
        assert any(raw[s - 1] == 10 and raw[e] == 10 for s, e in rec if 0 < s and e < lc.TOTAL)
        # the starts and the ends of the text
        assert rec[0][0] == 0 and rec[-1][1] == lc.TOTAL - int(nl)
        # the stale rule: more than STALE_AFTER records, and those of the last line start behind the last newline of the open text
        behind = [s for s, _ in rec if s > raw.rfind(b"\n")]
        assert len(rec) > om.STALE_AFTER
        if not nl:
            assert len(behind) == len(row.tail) and om.stale_records(raw, rec) == len(behind)
            assert len(behind) >= 3 or row.bol or row.eol or key == "error-timeout", (key, behind)
        else:
            assert not behind
        # the long matches across a cell, a round and the unit boundary
        for kind, size in (("cell", lc.CELL), ("round", lc.ROUND), ("unit", lc.UNIT)):
            over = [p for p in plants if p.kind == kind]
            assert over and all(p.start // size != (p.end - 1) // size and p.end - p.start >= 1000 for p in over), (key, kind)
        assert sum(1 for p in plants if p.kind == "unit") == 1 and lc.TOTAL == 2 * lc.UNIT
        if regex_ref.available():  # -m N: the first N of the same list
            for mc in (1, 7):
                cut = lc.records(row, text, mc)
                assert [tuple(int(v) for v in r) for r in cut] == rec[:mc], (key, mc)
    # at least three rows put three records behind the last newline; the anchored rows cannot
    assert sum(1 for r in lc.ROWS if len(r.tail) >= 3) >= 9


def test_the_cap_texts_hold_the_records_the_table_says():
    assert [c.in_line for c in lc.CAPS] == [4096, 2049, 2048, 2048, 1365]
    for cap in lc.CAPS:
        for nl in VARIANTS:
            text, raw, rec = lc.cap_case(cap.key, nl)
            a = lc.cap_line_at(cap)
            z = a + len(cap.line)
            assert text.size < 10 * 1024 and raw[a:z] == cap.line and raw[a - 1] == 10 and (z == len(raw) or raw[z] == 10)
            inside = [(s, e) for s, e in rec if a <= s < z]
            assert len(inside) == cap.in_line and len(rec) > len(inside), (cap.key, len(inside))
            if cap.key == "cap/inner-1365":
                assert all(x[1] == y[0] for x, y in zip(inside, inside[1:])) and inside[-1][1] == z  # all touching
            if cap.key.startswith("cap/ab*"):
                assert all(e - s == 1 for s, e in inside)
    assert lc.lm.CAP == 2048


def _against_the_cli(row, key, raw, rec, nl, tmp_path, counts):
    asked = 0
    path = tmp_path / "t.txt"
    if CLI:
        path.write_bytes(raw)
    for mode in lc.MODES:
        for mc in counts:
            mine = lc.expected(raw, rec, mode, lc.FILE, mc)
            rc_mine = 0 if mine else 1
            live = None
            if CLI:
                code, out = lc.run_cli(CLI, row, mode, path, mc)
                first = next((k for k in range(min(len(out), len(mine))) if out[k] != mine[k]), min(len(out), len(mine)))
                assert out == mine and code == rc_mine, (key, nl, mode, mc, len(out), len(mine), first)
                live = lc.digest(code, out)
            k = f"{key}/{'nl' if nl else 'open'}/{mode}/m{'-' if mc is None else mc if mc <= 7 else 'all'}"
            assert lc.digest(rc_mine, mine) == STORE.want(k, live), k
            asked += 1
            if mc is None:
                assert mine.count(b"\n") == (len(rec) if mode.startswith("o") else len({raw.rfind(b"\n", 0, s) for s, _ in rec}))
    return asked


@pytest.mark.parametrize("key", [r.key for r in lc.ROWS])
def test_model_bytes_equal_the_stock_cli(key, tmp_path):
    """the three output models on the reference's records against `krep -t 1 -E [-o] --color=never|always [-m N]`"""
    row = lc.BY_KEY[key]
    asked = 0
    for nl in VARIANTS:
        _, raw, _, rec = lc.case(key, nl)
        counts = (None,) + ((1, 7, len(rec) + 5) if lc.single(row) else ())
        asked += _against_the_cli(row, key, raw, rec, nl, tmp_path, counts)
    STORE.save()
    assert asked == (32 if lc.single(row) else 8)


def test_model_bytes_of_the_cap_texts_equal_the_stock_cli(tmp_path):
    for cap in lc.CAPS:
        for nl in VARIANTS:
            _, raw, rec = lc.cap_case(cap.key, nl)
            assert _against_the_cli(cap, cap.key, raw, rec, nl, tmp_path, (None,)) == 4
    STORE.save()
    # what the models say about the pair around the cap: under -o the 2049th record is one more line; in the coloured lines it adds
    # its own byte to the line, uncoloured, and nothing else
    _, raw8, rec8 = lc.cap_case("cap/ab*-2048", True)
    _, raw9, rec9 = lc.cap_case("cap/ab*-2049", True)
    o8, o9 = lc.expected(raw8, rec8, "o-color", lc.FILE), lc.expected(raw9, rec9, "o-color", lc.FILE)
    assert o9.count(b"\n") == o8.count(b"\n") + 1
    c8, c9 = lc.expected(raw8, rec8, "lines-color", lc.FILE), lc.expected(raw9, rec9, "lines-color", lc.FILE)
    assert len(c9) == len(c8) + 1 and c9.count(b"a") == c8.count(b"a") + 1
