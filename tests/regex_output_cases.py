"""The cases of the regex OUTPUT tests: one table of -E patterns across the four compilers (class sequences, line anchors,
alternations, the expanding compiler), the text that is built for each of them, the records the numpy models give and the bytes the
three output models make of them.  TEST SUPPORT: imported by tests/test_regex_output_cases_cpu.py (which pins the table, the texts
and the models' bytes to the compilers, the compiled reference and the stock CLI, no GPU) and by tests/test_gpu_regex_output.py.

A row: key; the patterns (several: given as several -e); case_sensitive; the compiler FAMILY that takes the search (basic: a class
sequence, anchored: ^ / $ around one, alt: krep_gpu_regex_compile_alt, ext: krep_gpu_regex_compile_ext); what krep_gpu_split_mode()
calls it (PIECES / WHOLE); Lmax, the longest match in text bytes; bol / eol; the alphabet of the background; strings that match,
the LONGEST first (it is the one the sweep plants).

The text of a row (build_text, TOTAL bytes, a few 32-KiB units): lines of 20 .. 80 bytes over the row's alphabet, and
  sweep     for the piece size P_SMALL the longest string at cut - k for every k in -1 .. Lmax + 1 (k = bytes of it in front of the
            cut, so the starts run from cut - Lmax - 1 to cut + 1), each k at a cut of its own;
  unit      one straddler at each multiple of P_UNIT: 1, Lmax - 1 and Lmax / 2 bytes in front of it;
  long      a line of more than three pieces of P_SMALL whose only match lies in its last 20 bytes (a ^ row: at its start, the only
            place its anchor leaves; a ^...$ row has no such line, its line IS the match);
  edge      a line whose first match starts in the Lmax bytes in front of records_hi of the piece that owns it, for P_SMALL and the
            driver's default halo of 4096 bytes (no ^ row: a match is the start of its line);
  first     a match on byte 0, and
  last      one that ends on the last byte (with final_newline: on the byte in front of the newline that ends the text);
  sprinkled copies of every string between them, for the records the alphabet alone does not give.
Every planted copy has a byte of QUIET (or the newline its ^ asks for) in front, so that no occurrence further left reaches into it.
"""
from __future__ import annotations

import functools
import hashlib
import os
import subprocess
import zlib
from collections import namedtuple

import numpy as np

import color_line_model as cm
import line_model as lm
import only_matching_model as om
import regex_alt_model
import regex_anchor_model
import regex_ext_model
import regex_model
from krep_amd import abi

Row = namedtuple("Row", "key pats cs family mode Lmax bol eol alphabet plants")
Plant = namedtuple("Plant", "kind k cut start end")

PIECES, WHOLE = "PIECES", "WHOLE"
LOWER = b"abcdefghijklmnopqrstuvwxyz "

ROWS = [
    # ---- class sequences (krep_gpu_regex_compile)
    Row("basic/word", [b"[A-Z][a-z]{7}"], True, "basic", PIECES, 8, 0, 0, LOWER, [b"Sherlock", b"Moriarty"]),           # L < the string
    Row("basic/q16", [b"q[a-c]{15}"], True, "basic", PIECES, 16, 0, 0, b"abcq xyz", [b"qabcabcabcabcabc"]),              # L = 16, string = 10
    Row("basic/q16-newline", [b"q[a-c\n]{15}"], True, "basic", PIECES, 16, 0, 0, b"abcq xyz",                            # the same across a line's end:
        [b"qab\ncabcabcabcab", b"qabcabcabcabcabc"]),                                                                     # its line is complete, it is not
    Row("basic/z13", [b"Z[0-9]{12}"], True, "basic", PIECES, 13, 0, 0, b"0123456789Z xy", [b"Z314159265358"]),
    Row("basic/space", [b"ab[[:space:]]cd"], True, "basic", PIECES, 5, 0, 0, b"abcd \t", [b"ab\ncd", b"ab cd", b"ab\tcd"]),  # crosses a newline
    Row("basic/icase", [b"sherl[o0]ck"], False, "basic", PIECES, 8, 0, 0, LOWER + b"SHK", [b"SHERLOCK", b"Sherl0ck", b"sherlock"]),
    Row("basic/overlap", [b"[a-c]{3}"], True, "basic", WHOLE, 3, 0, 0, b"abcdefghijklmnop ", [b"abc", b"cab"]),          # overlaps itself
    # ---- line anchors (krep_gpu_regex_compile_anchored)
    Row("anchor/bol", [b"^ERROR"], True, "anchored", PIECES, 5, 1, 0, b"EROR abcdefgh", [b"ERROR"]),
    Row("anchor/digits-eol", [b"[0-9]{3}$"], True, "anchored", PIECES, 3, 0, 1, b"0123456789abcdef ", [b"123", b"907"]),
    Row("anchor/both", [b"^abcd$"], True, "anchored", PIECES, 4, 1, 1, b"abcd ", [b"abcd"]),
    Row("anchor/bol-q15", [b"^q[a-c]{14}"], True, "anchored", PIECES, 15, 1, 0, b"abcq xyz", [b"qabcabcabcabcab"]),      # L = 15, string = 11
    Row("anchor/semicolon", [b";$"], True, "anchored", PIECES, 1, 0, 1, b"abc;xyz ", [b";"]),
    # ---- alternations of class sequences (krep_gpu_regex_compile_alt)
    Row("alt/animals", [b"cat|d[oi]g|b.rd"], True, "alt", WHOLE, 4, 0, 0, b"catdoigbr ", [b"bird", b"cat", b"dog", b"dig"]),  # bird + dog share a d
    Row("alt/fish", [b"cat|d[oi]g|f.sh"], True, "alt", PIECES, 4, 0, 0, b"catdoigfsh ", [b"fish", b"cat", b"dog", b"dig"]),
    Row("alt/longest", [b"ab|abc"], True, "alt", WHOLE, 3, 0, 0, b"abc xyz", [b"abc", b"ab"]),                           # leftmost-longest
    Row("alt/1-and-16", [b"q|a[b-d]{15}"], True, "alt", PIECES, 16, 0, 0, b"bcd xyzuvwmnoprstefghijkl.,-q", [b"abcdbcdbcdbcdbcd", b"q"]),
    Row("alt/two-e", [b"GET /", b"POST /[a-z]"], True, "alt", PIECES, 7, 0, 0, b"GETPOS /abc", [b"POST /x", b"GET /"]),   # num_patterns > 1
    # ---- ?, {n,m}, inner groups, anchored alternations (krep_gpu_regex_compile_ext)
    Row("ext/colour", [b"colou?r"], True, "ext", PIECES, 6, 0, 0, b"colur ", [b"colour", b"color"]),
    Row("ext/percent", [b"[0-9]{1,3}%"], True, "ext", WHOLE, 4, 0, 0, b"0123456789% abc", [b"100%", b"42%", b"7%"]),
    Row("ext/inner", [b"x(a|bc)y"], True, "ext", PIECES, 4, 0, 0, b"xabcy ", [b"xbcy", b"xay"]),
    Row("ext/api", [b"(GET|POST) /api"], True, "ext", PIECES, 9, 0, 0, b"GETPOS /api", [b"POST /api", b"GET /api"]),
    Row("ext/bol-alt", [b"^(ERROR|WARN)"], True, "ext", PIECES, 5, 1, 0, b"ERORWAN abc", [b"ERROR", b"WARN"]),
    Row("ext/suffix-eol", [b"\\.(jpg|png)$"], True, "ext", PIECES, 4, 0, 1, b".jpgn abc", [b".jpg", b".png"]),
    Row("ext/branch16", [b"z[a-c]{13,14}!"], True, "ext", PIECES, 16, 0, 0, b"abcz! xy",                                  # a 16-byte branch, string = 14
        [b"zabcabcabcabcab!", b"zabcabcabcabca!"]),
]
BY_KEY = {r.key: r for r in ROWS}
FAMILIES = ("basic", "anchored", "alt", "ext")

QUIET = b"_~"                 # bytes no row's first class and no row's alphabet holds
P_SMALL, P_UNIT = 4099, 32768  # the piece sizes the texts are built for
HALO = 4096                   # Plan.grep_lines_pieces' default halo_bytes
TOTAL = 31 * P_SMALL + 1000   # 128069 bytes: three multiples of P_UNIT inside
LONG_LINE = (25 * P_SMALL - 400, 25 * P_SMALL - 400 + 12500)   # [start, newline): over the cuts 25, 26 and 27
EDGE_CUT = 29 * P_SMALL
MODES = ("lines", "lines-color", "o", "o-color")


def sweep_cuts():
    """the multiples of P_SMALL the sweep uses: those in front of the long line that lie no 100 bytes from a multiple of P_UNIT"""
    return [j * P_SMALL for j in range(1, 23) if j % 8]


def params(row: Row, max_count=None) -> abi.Params:
    return abi.Params(row.pats, regex=True, case_sensitive=row.cs, max_count=abi.SIZE_MAX if max_count is None else max_count)


def single(row: Row) -> bool:
    return len(row.pats) == 1


def string_len(row: Row) -> int:
    """what the drivers took for the longest match before they asked the compilers: the longest pattern STRING"""
    return max(len(p) for p in row.pats)


def build_text(row: Row, final_newline: bool):
    """-> (text uint8[TOTAL], [Plant]); the same bytes for the same arguments"""
    rng = np.random.RandomState(zlib.crc32(row.key.encode()) & 0x7FFFFFFF)
    al = np.frombuffer(row.alphabet, dtype=np.uint8)
    assert 10 not in row.alphabet and not set(QUIET) & set(row.alphabet)
    t = al[rng.randint(0, al.size, size=TOTAL)].copy()
    at = 0
    while True:
        at += rng.randint(20, 81)
        if at >= TOTAL:
            break
        t[at] = 10
        at += 1
    quiet = np.frombuffer(QUIET, dtype=np.uint8)
    L, longest = row.Lmax, row.plants[0]
    assert len(longest) == L and all(len(p) <= L for p in row.plants)
    plants, zones = [], []

    def put(kind, k, cut, s, plant=longest):
        p = np.frombuffer(plant, dtype=np.uint8)
        assert 0 <= s and s + len(p) <= TOTAL and not any(a < s + len(p) + 2 and s - 2 < b for a, b in zones), (row.key, kind, k, s)
        t[s:s + len(p)] = p
        if s > 0:
            t[s - 1] = 10 if row.bol else quiet[0]
        if row.eol and s + len(p) < TOTAL:
            t[s + len(p)] = 10
        zones.append((s - 100, s + len(p) + 100))
        plants.append(Plant(kind, k, cut, s, s + len(p)))

    def quiet_line(a, z):
        t[a:z] = quiet[rng.randint(0, quiet.size, size=z - a)]
        t[a - 1] = t[z] = 10
        zones.append((a - 1, z + 1))

    for k, cut in zip(range(-1, L + 2), sweep_cuts()):
        put("sweep", k, cut, cut - k)
    for j, k in ((1, 1), (2, max(L - 1, 1)), (3, max(L // 2, 1))):
        put("unit", k, j * P_UNIT, j * P_UNIT - k)
    if not (row.bol and row.eol):
        a, z = LONG_LINE
        quiet_line(a, z)
        zones.pop()
        put("long", None, None, a if row.bol else z - L if row.eol else z - L - 2)
        zones.append((a - 1, z + 1))
    if not row.bol:
        records_hi = EDGE_CUT + HALO - (L + row.eol - 1)
        s = records_hi - max(1, (L + 1) // 2)
        a, z = EDGE_CUT - 100, (s + L if row.eol else EDGE_CUT - 100 + 4500)
        quiet_line(a, z)
        zones.pop()
        put("edge", None, EDGE_CUT, s, next(p for p in row.plants if len(p) == L and b"\n" not in p))  # (ab\ncd would end the line)
        zones.append((a - 1, z + 1))
    put("first", None, None, 0)
    if final_newline:
        t[TOTAL - 1] = 10
    put("last", None, None, TOTAL - L - int(final_newline))
    for base in range(700, TOTAL - 400, 977):
        plant = row.plants[rng.randint(len(row.plants))]
        s = base + int(rng.randint(0, 300))
        if not any(a < s + len(plant) + 2 and s - 2 < b for a, b in zones):
            put("sprinkled", None, None, s, plant)
    assert (t[-1] == 10) == bool(final_newline)
    return t, plants


@functools.lru_cache(maxsize=None)
def case(key: str, final_newline: bool):
    """-> (text, text as bytes, plants, the records of the whole search [(start, end)]), built once per process and left unchanged"""
    row = BY_KEY[key]
    text, plants = build_text(row, final_newline)
    text.setflags(write=False)
    rec = [(int(s), int(e)) for s, e in records(row, text)]
    return text, text.tobytes(), plants, rec


def records(row: Row, text: np.ndarray, max_count=None) -> np.ndarray:
    """the records regex_search emits, from the numpy model of the row's family (each pinned to the compiled reference by its own
    CPU test, and for these texts by tests/test_regex_output_cases_cpu.py)"""
    kw = dict(case_sensitive=row.cs, max_count=abi.SIZE_MAX if max_count is None else max_count)
    if row.family == "basic":
        return regex_model.run(row.pats[0], text, **kw)[1]
    if row.family == "anchored":
        return regex_anchor_model.run(row.pats[0], text, **kw)[1]
    if row.family == "alt":
        return regex_alt_model.run(row.pats, text, **kw)[1]
    return regex_ext_model.run(row.pats, text, **kw)[1]


def expected(raw: bytes, rec, mode: str, filename=None, max_count=None) -> bytes:
    """the bytes the CLI prints for the records `rec` (emission order = start order for regex_search) in one of MODES; filename None:
    no FILE: in front"""
    if mode == "lines":
        return lm.grep_output(raw, rec, b"" if filename is None else filename + b":", max_count)
    if mode == "lines-color":
        return cm.color_output(raw, rec, filename, True, max_count)
    return om.grep_o_output(raw, rec, filename, mode == "o-color", max_count)


# ---- the stock CLI and the store of its answers ------------------------------------------------------------------------------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "regex_output.json")
FILE = lm.FILE


def cli_args(row: Row, mode: str, max_count=None):
    a = (["-o"] if mode.startswith("o") else []) + ["-t", "1", "-E", "--color=always" if mode.endswith("color") else "--color=never"]
    a += ([] if row.cs else ["-i"]) + (["-m", str(max_count)] if max_count is not None else [])
    if single(row):
        return a + [row.pats[0]]
    for p in row.pats:
        a += ["-e", p]
    return a


def run_cli(cli, row: Row, mode: str, path, max_count=None):
    """-> (exit code, stdout with the path replaced by FILE); `path` holds the text"""
    r = subprocess.run([cli] + cli_args(row, mode, max_count) + [str(path)], capture_output=True, timeout=120)
    return r.returncode, r.stdout.replace(str(path).encode(), FILE)


def digest(rc: int, out: bytes) -> str:
    return hashlib.sha256(b"%d:" % rc + out).hexdigest()[:16]


class Store(lm.Store):
    """line_model.Store over tests/golden/regex_output.json: digests of the stock CLI's answers for the rows of this table"""

    def _own(self, call, *a):
        keep, lm.GOLDEN = lm.GOLDEN, GOLDEN
        try:
            return call(*a)
        finally:
            lm.GOLDEN = keep

    def __init__(self):
        self._own(super().__init__)

    def want(self, key, live=None) -> str:
        return self._own(super().want, key, live)

    def save(self):
        self._own(super().save)
