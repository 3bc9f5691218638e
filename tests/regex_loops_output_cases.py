"""The cases of the OUTPUT tests of the loops regexes (krep -E with *, + and {n,}: krep_gpu_regex_compile_loops behind
krep_gpu_set_regex_loops): one table of patterns, ONE 64-KiB text per row, the records of the compiled reference's regex_search and the
bytes the three output models make of them (regex_output_cases.expected).  TEST SUPPORT: imported by
tests/test_regex_loops_output_cases_cpu.py (which pins the table, the texts and the models' bytes to the compilers, the compiled
reference and the stock CLI, no GPU), by tests/test_gpu_regex_loops_output.py and by tests/test_gpu_grep_batch_loops.py.

What a loops plan hands the formatter kernels that no older plan does: records of 1 .. 4096 bytes in one list, records that touch,
thousands of one-byte records in one line, and a longest match (4097) that no halo or guess can be sized by from the pattern.

A row: key; the patterns (several: several -e); case_sensitive; the background's alphabet; make(n): a string of exactly n bytes that
is one match and, alone on a line, its whole line; the shortest n; `touching`: matches that, written one behind the other, are found
one by one (None: the grammar's maximal runs never touch); `tail`: the matches of the last line, a blank between them (three where a
line can hold three: a ^ or $ row and ERROR.*timeout hold one); lines that hold a match and decoy lines (the filter without a match),
from SHAPES of tests/test_gpu_regex_loops.py where the pattern has a row there; must_long: the reference has to give a record of 1000
bytes or more; bol / eol.

The text of a row (build_text, TOTAL bytes = two 32-KiB units): lines of 20 .. 80 bytes over the alphabet and, each a line of its own
(put_line of tests/test_gpu_regex_loops.py):
  first     make(17) from byte 0;
  mixed     make(shortest) and make(17) between quiet bytes (alone where an anchor asks for it), make(1000), make(3500), make(3800);
  line4096  two lines of exactly 4096 bytes: make(17) and 4079 quiet bytes, the match in front / at the end (where an anchor forbids
            one of them: make(4096), a record that is its whole 4096-byte line);
  touch     the touching matches as one line;
  straddle  make(1000) across a 1-KiB cell boundary and across an 8-KiB round boundary, make(3800) across an 8-KiB round boundary and
            across THE 32-KiB unit boundary (a 64-KiB text has one; the 1000-byte copy cannot lie across it as well), make(3500)
            across a cell boundary; every one of these also crosses the cell boundaries inside it;
  sprinkled the lines and the decoys of the row, every 173 bytes wherever nothing else stands;
  tail      the last line: `tail`, its last match on the last byte of the text (with final_newline: on the byte in front of the
            newline that ends it).  Without a final newline its matches start behind the text's last newline: the stale rule.
No line is longer than 4096 bytes.

CAPS: the five texts of under 10 KiB around the coloured-line cap of 2048 records per line (line_model.CAP)."""
from __future__ import annotations

import functools
import os
import zlib
from collections import namedtuple

import numpy as np

import line_model as lm
import regex_alt_model
import regex_loops_model
import regex_output_cases as rc
import regex_ref
from krep_amd import abi
from test_gpu_regex_loops import CELL, ROUND, SHAPES, UNIT, put_line, word_text

expected, cli_args, run_cli, digest, MODES, single = rc.expected, rc.cli_args, rc.run_cli, rc.digest, rc.MODES, rc.single

Row = namedtuple("Row", "key pats cs alphabet make shortest touching tail lines decoys must_long bol eol")
Plant = namedtuple("Plant", "kind start end")

TOTAL = 2 * UNIT
LINE_MAX = 4096   # the longest line the walk takes (include/krep_gpu.h)
LONGEST = 4097    # Plan.longest_match() of a loops plan
QUIET = b"_~_"    # bytes no row's pattern matches and no alphabet holds
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "regex_loops_output.json")
FILE = rc.FILE


def cyc(seed: bytes, n: int) -> bytes:
    return (seed * (n // len(seed) + 1))[:max(n, 0)]


def _shape(pats):
    """(alphabet, lines with a match, decoy lines) of the pattern's row in SHAPES"""
    for p, alphabet, lines, decoys in SHAPES:
        if p == pats:
            return alphabet, lines, decoys
    raise KeyError(pats)


def _row(key, pats, make, shortest, touching, tail, cs=True, own=None, must_long=True, bol=0, eol=0, decoys=None):
    alphabet, lines, shape_decoys = own if own is not None else _shape(pats)
    decoys = shape_decoys or decoys  # (SHAPES has none where the filter alone is a match: the nearest misses stand in)
    return Row(key, pats, cs, bytes(b for b in alphabet if b != 10), make, shortest, touching, tail, list(lines), list(decoys), must_long,
               bol, eol)


def _two_e(n):
    return b"a" * n if n < 2 or n == 17 else b"b" * (n - 1) + b"c"


def _decimal(n):
    f = max(1, n // 3)
    return cyc(b"0123012", n - 1 - f) + b"." + cyc(b"3210", f)


ROWS = [
    _row("error-timeout", [b"ERROR.*timeout"], lambda n: b"ERROR" + cyc(b": -=+#%", n - 12) + b"timeout", 12, None, [b"ERROR: a timeout"]),
    _row("a+b", [b"a+b"], lambda n: b"a" * (n - 1) + b"b", 2, [b"aab", b"ab"], [b"ab", b"aaab", b"ab"],
         decoys=[b"aaa c", b"b a cb"]),
    _row("ab*", [b"ab*"], lambda n: b"a" + b"b" * (n - 1), 1, [b"abb", b"a", b"ab"], [b"abb", b"a", b"ab"],
         own=(b"abbc ", [b"a", b"xabbb", b"abab ab"], [b"b bb", b"xbbc"])),
    _row("decimal", [b"[0-9]+\\.[0-9]+"], _decimal, 3, None, [b"1.5", b"22.75", b"3.0"]),
    _row("colou*r", [b"colou*r"], lambda n: b"colo" + b"u" * (n - 5) + b"r", 5, [b"color", b"colouur"], [b"color", b"colour", b"colouuur"],
         must_long=False),
    _row("colou*r-i", [b"colou*r"], lambda n: b"CoLo" + cyc(b"uUu", n - 5) + b"R", 5, [b"COLOR", b"colOUUr"], [b"Color", b"COLOUR", b"colouuUr"],
         cs=False, own=(b"colurCOLUR ", [b"Color", b"COLOUUUR", b"colorCOLOUR colr"], [b"COLOU", b"Coloux colo R"]), must_long=False),
    _row("inner", [b"x(a+|b)y"], lambda n: b"x" + b"a" * (n - 2) + b"y", 3, [b"xay", b"xby"], [b"xay", b"xby", b"xaay"], must_long=False),
    _row("class-c", [b"[ab]+c?"], lambda n: cyc(b"abbabaa", n - 1) + (b"c" if n > 1 else b"a"), 1, [b"abc", b"ab"], [b"ab", b"abc", b"a"],
         decoys=[b"c  c", b" cc c "]),
    _row("bol", [b"^a+"], lambda n: b"a" * n, 1, None, [b"aaa"], bol=1),
    _row("eol", [b"b+$"], lambda n: b"b" * n, 1, None, [b"bb"], eol=1),
    _row("bol-eol", [b"^a+b$"], lambda n: b"a" * (n - 1) + b"b", 2, None, [b"aab"],
         own=(b"aab ", [b"ab", b"aaaab"], [b"aab ", b" ab", b"aabb"]), must_long=False, bol=1, eol=1),
    _row("open-count", [b"q[a-c]{2,}"], lambda n: b"q" + cyc(b"abcacbb", n - 1), 3, [b"qab", b"qcc"], [b"qab", b"qcc", b"qabc"],
         own=(b"abcq xyz", [b"qab", b"xqabcabc q", b"qaaqbb qcc"], [b"qa", b"q ab qx"])),
    _row("two-e", [b"a+", b"b+c"], _two_e, 1, [b"aa", b"bbc"], [b"aa", b"bbc", b"a"], must_long=False),
    _row("words", [b"[a-z]+"], lambda n: cyc(b"thequickbrownfxjmpsvlazydg", n), 1, None, [b"the", b"lazy", b"dog"],
         own=(b"", [b"Hello world", b"a"], [b"HELLO 123", b"_-_"])),  # (no alphabet: the word text of tests/test_gpu_regex_loops.py)
]
BY_KEY = {r.key: r for r in ROWS}

# where the lines stand: (kind, the byte the line starts at, the length make() is asked for).  Nothing overlaps (build_text asserts it).
LAYOUT = [
    ("cell", 13 * CELL - 300, 1000), ("round", 2 * ROUND - 500, 1000), ("round", 3 * ROUND - 2000, 3800),
    ("unit", UNIT - 1900, 3800), ("cell", 41 * CELL - 100, 3500),
]
AT_4096 = (2100, 6300)                                   # the two lines of 4096 bytes (the second lies across the first round boundary)
AT_SHORT, AT_17, AT_TOUCH = 10600, 10700, 10800


def params(row: Row, max_count=None) -> abi.Params:
    return rc.params(row, max_count)


def background(row: Row, rng, n: int) -> np.ndarray:
    if row.alphabet:
        al = np.frombuffer(row.alphabet, dtype=np.uint8)
        t = al[rng.randint(0, al.size, size=n)].copy()
    else:
        t = word_text(rng, n)
        t[t == 10] = 32
    at = 0
    while True:
        at += rng.randint(20, 81)
        if at >= n:
            break
        t[at] = 10
        at += 1
    return t


def lines_4096(row: Row):
    """-> [(the line, offset of its match, length of its match)]: the match in the first bytes, the match in the last 20 bytes"""
    m, whole = row.make(17), row.make(LINE_MAX)
    front = (m + cyc(QUIET, LINE_MAX - 17), 0, 17) if not row.eol else (whole, 0, LINE_MAX)
    back = (cyc(QUIET, LINE_MAX - 17) + m, LINE_MAX - 17, 17) if not row.bol else (whole, 0, LINE_MAX)
    return [front, back]


def tail_line(row: Row):
    """-> (the last line, [(offset, length)] of its matches)"""
    spans, at = [], 0
    for m in row.tail:
        spans.append((at, len(m)))
        at += len(m) + 1
    return b" ".join(row.tail), spans


def build_text(row: Row, final_newline: bool):
    """-> (text uint8[TOTAL], [Plant]); the same bytes for the same arguments"""
    rng = np.random.RandomState(zlib.crc32(row.key.encode()) & 0x7FFFFFFF)
    t = background(row, rng, TOTAL)
    assert not set(QUIET) & set(row.alphabet)
    plants, zones = [], []

    def put(kind, s, line, spans):
        assert s >= 1 and s + len(line) + 1 <= TOTAL and len(line) <= LINE_MAX, (row.key, kind, s)
        assert not any(a < s + len(line) + 1 and s - 1 < b for a, b in zones), (row.key, kind, s)
        put_line(t, s, line)
        zones.append((s - 1, s + len(line) + 1))
        plants.extend(Plant(kind, s + o, s + o + n) for o, n in spans)

    first = row.make(17)  # byte 0: no newline in front of it
    t[:18] = np.frombuffer(first + b"\n", dtype=np.uint8)
    zones.append((0, 18))
    plants.append(Plant("first", 0, 17))
    for s, (line, o, n) in zip(AT_4096, lines_4096(row)):
        put("line4096", s, line, [(o, n)])
    anchored = row.bol or row.eol
    for s, n in ((AT_SHORT, row.shortest), (AT_17, 17)):
        m = row.make(n)
        put("mixed", s, m if anchored else b"_" + m + b"~", [(0 if anchored else 1, n)])
    if row.touching:
        spans, at = [], 0
        for m in row.touching:
            spans.append((at, len(m)))
            at += len(m)
        put("touch", AT_TOUCH, b"".join(row.touching), spans)
    for kind, s, n in LAYOUT:
        put(kind, s, row.make(n), [(0, n)])
    line, spans = tail_line(row)
    s = TOTAL - len(line) - int(final_newline)
    t[s - 1] = 10
    t[s:s + len(line)] = np.frombuffer(line, dtype=np.uint8)
    if final_newline:
        t[TOTAL - 1] = 10
    zones.append((s - 1, TOTAL))
    plants.extend(Plant("tail", s + o, s + o + n) for o, n in spans)
    extra = row.lines + row.decoys
    for k, s in enumerate(range(200, TOTAL - 200, 173)):
        line = extra[k % len(extra)]
        if not any(a < s + len(line) + 2 and s - 2 < b for a, b in zones):
            put_line(t, s, line)
            zones.append((s - 1, s + len(line) + 1))
    assert t.size == TOTAL and (t[-1] == 10) == bool(final_newline)
    return t, plants


def records(row, text: np.ndarray, max_count=None) -> np.ndarray:
    """the records regex_search emits: the compiled reference with the expression the CLI compiles.  Where oracle/_ref is not built (a
    CPU-only check of the models against the stored digests) the brute-force model of tests/regex_loops_model.py, which
    tests/test_regex_loops_model_cpu.py pins to the reference; the GPU tests insist on the reference."""
    kw = dict(case_sensitive=row.cs, max_count=abi.SIZE_MAX if max_count is None else max_count)
    if regex_ref.available():
        return regex_ref.call(regex_alt_model.joined(row.pats), text, **kw)[1]
    return regex_loops_model.run(row.pats, text, **kw)[1]


@functools.lru_cache(maxsize=None)
def case(key: str, final_newline: bool):
    """-> (text, text as bytes, plants, the records of the whole search [(start, end)]), built once per process and left unchanged"""
    row = BY_KEY[key]
    text, plants = build_text(row, final_newline)
    text.setflags(write=False)
    with regex_ref.c_locale():
        rec = [(int(s), int(e)) for s, e in records(row, text)]
    return text, text.tobytes(), plants, rec


def decoy_text(row: Row) -> np.ndarray:
    return np.frombuffer(b"\n".join(row.decoys) + b"\n", dtype=np.uint8)


# ---- the cap of 2048 records per coloured line -------------------------------------------------------------------------------------
Cap = namedtuple("Cap", "key pats cs line in_line")
CAPS = [
    Cap("cap/ab*-4096", [b"ab*"], True, b"a" * 4096, 4096),
    Cap("cap/ab*-2049", [b"ab*"], True, b"a" * 2049, 2049),
    Cap("cap/ab*-2048", [b"ab*"], True, b"a" * 2048, 2048),
    Cap("cap/a+-2048", [b"a+"], True, b"a " * 2048, 2048),
    Cap("cap/inner-1365", [b"x(a+|b)y"], True, b"xay" * 1365, 1365),
]
CAP_BY_KEY = {c.key: c for c in CAPS}
ORDINARY = [b"an ordinary line, xy", b"bbb abb xby", b"", b"the last ordinary line ab"]


def cap_text(cap: Cap, final_newline: bool) -> np.ndarray:
    """the cap's line between a few ordinary lines"""
    body = b"\n".join(ORDINARY[:2] + [cap.line] + ORDINARY[2:]) + (b"\n" if final_newline else b"")
    assert len(body) < 10 * 1024 and len(cap.line) <= LINE_MAX
    return np.frombuffer(body, dtype=np.uint8)


def cap_line_at(cap: Cap) -> int:
    return sum(len(x) + 1 for x in ORDINARY[:2])


@functools.lru_cache(maxsize=None)
def cap_case(key: str, final_newline: bool):
    """-> (text, text as bytes, the records [(start, end)])"""
    cap = CAP_BY_KEY[key]
    text = cap_text(cap, final_newline)
    text.setflags(write=False)
    with regex_ref.c_locale():
        rec = [(int(s), int(e)) for s, e in records(cap, text)]
    return text, text.tobytes(), rec


class Store(rc.Store):
    """regex_output_cases.Store over tests/golden/regex_loops_output.json"""

    def _own(self, call, *a):
        keep, lm.GOLDEN = lm.GOLDEN, GOLDEN
        try:
            return call(*a)
        finally:
            lm.GOLDEN = keep
