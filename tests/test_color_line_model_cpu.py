"""The coloured default output of the reference (`--color=always`: every line that holds a match, once, with the escape strings
around the line and around every match) as tests/color_line_model.py states it, pinned to the stock CLI (`krep -t 1
--color=always`, oracle/_ref/krep) byte for byte: every row of the line model's table and all its seeded random cases with a
filename, and `--color=always -s PATTERN TEXT` (the prefix without a filename) on the cases a command line can carry.  Where the
CLI cannot be built the digests of its answers in tests/golden/color_line_output.json stand in."""
import color_line_model as cm
import line_model as lm
import oracle_lib as ol
from krep_amd import abi

CLI = ol.ref_cli()
STORE = cm.Store()


def check(case, tmp_path, chk):
    """-> (the case printed something, it also took the -s road)"""
    emitted = case.emitted(chk, abi)
    mine = cm.color_output(case.text, emitted, cm.FILE, True, case.max_count)
    rc_mine = 0 if mine else 1
    live = None
    if CLI:
        path = tmp_path / "t.txt"
        path.write_bytes(case.text)
        rc, out = cm.run_cli(CLI, case, path)
        assert out == mine and rc == rc_mine, (case.key, case.pats, case.cli_args(), case.text[:200], out[:200], mine[:200])
        live = cm.digest(rc, out)
    assert cm.digest(rc_mine, mine) == STORE.want(case.key, live), case.key
    if case.want is not None:  # the bytes between the escape strings are the plain row's
        plain = mine
        for esc in (cm.C_FILE, cm.RESET, cm.C_SEP, cm.C_MATCH, cm.C_TEXT):
            plain = plain.replace(esc, b"")
        assert plain == cm.FILE + b":" + case.want, case.key
    # with all four strings empty except the prefix the model is the plain one
    recs = lm.cut_to_max_count(emitted, case.max_count)
    assert cm.ColorLines(case.text, recs, (cm.FILE + b":", b"", b"", b""), case.max_count).data == \
        lm.Lines(case.text, recs, cm.FILE + b":", case.max_count).data
    assert cm.ColorLines(case.text, recs, cm.strings(None, False), case.max_count).data == lm.Lines(case.text, recs, b"", case.max_count).data
    if not case.string_mode_ok():
        return bool(mine), False
    mine = cm.color_output(case.text, emitted, None, True, None)
    rc_mine = 0 if mine else 1
    live = None
    if CLI:
        rc, out = cm.run_cli_string(CLI, case)
        assert out == mine and rc == rc_mine, (case.key, case.pats, case.text[:200], out[:200], mine[:200])
        live = cm.digest(rc, out)
    assert cm.digest(rc_mine, mine) == STORE.want(case.key + "/string", live), case.key
    return bool(mine), True


def test_table_rows_match_the_cli(tmp_path, oracle_engine):
    for case in cm.table_cases():
        assert check(case, tmp_path, oracle_engine)[0]
    STORE.save()


def test_random_cases_match_the_cli(tmp_path, oracle_engine):
    cases = cm.random_cases()
    assert len(cases) >= 240
    seen = [check(case, tmp_path, oracle_engine) for case in cases]
    STORE.save()
    assert sum(p for p, _ in seen) > len(cases) // 2
    assert sum(s for _, s in seen) >= 30, sum(s for _, s in seen)  # the prefix without a filename


def test_model_rules_on_hand_made_lists():
    sh = b"xx Sherlock yy"
    recs = sorted([(3, 11), (5, 7), (7, 11)])
    got = cm.ColorLines(sh, recs, cm.strings(b"F", True)).data
    assert got == (b"\033[1;38;5;81mF\033[0m\033[38;5;244m:\033[38;5;252mxx \033[1;38;5;222mSherlock\033[38;5;252m"
                   b"\033[1;38;5;222mer\033[38;5;252m\033[1;38;5;222mlock\033[38;5;252m yy\033[0m\n")
    assert cm.ColorLines(sh, recs, cm.strings(None, True)).data.startswith(b"\033[38;5;252mxx \033[1;38;5;222mS")
    text = b"ab\ncd\n\nef"
    # a start ON a newline and an empty record add nothing, no strings either; the line they open still gets prefix and close
    m = cm.ColorLines(text, [(0, 1), (2, 4), (3, 3), (6, 8)], (b"P", b"<", b">", b"$"))
    assert m.data == b"P<a>b$\nPcd$\nP$\n" and m.spans == [(0, 2), (3, 5), (6, 6)]
    m = cm.ColorLines(b"a" * 5000, [(i, i + 2) for i in range(4999)], (b"", b"<", b">", b"$"))
    assert m.capped == 1 and m.data == b"<aa>" * 2048 + b"a" * (5000 - 2049) + b"$\n"
    assert cm.ColorLines(text, [(0, 1), (4, 5), (7, 9)], (b"P", b"<", b">", b"$"), 2).data == b"P<a>b$\nPc<d>$\n"
