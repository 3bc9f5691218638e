"""What the reference prints by default with colour (`krep --color=always PATTERN FILE`; print_matching_items() in full-line mode
with color_output_enabled, krep.c:797-1071).  A plain-Python statement of the rule, for the tests of krep_gpu_format_lines_ex /
Plan.grep_lines(color=True).

TEST INFRASTRUCTURE.  The rule is that of tests/line_model.py (its rules 1-4 decide lines, counted records and cursor) with four
caller strings added (tests/test_color_line_model_cpu.py pins it to the stock CLI):
  per emitted line:   prefix
  per counted record (the first 2048 of the line) whose match, cut at line_end, is not empty:
                      text[cursor, start) if start > cursor,  before_match,  text[start, cut end),  after_match;  cursor := cut end
  then                text[cursor, line_end) if cursor < line_end,  line_close,  a newline
A record whose cut match is empty adds nothing, no strings either.  The cursor may move backwards: overlapping records repeat bytes,
each inside its own pair of strings.
"""
from __future__ import annotations

import contextlib
import os
import subprocess

import line_model as lm

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "color_line_output.json")
FILE = lm.FILE

# the reference's colours (data: the escape codes of its header)
RESET, C_FILE, C_SEP, C_MATCH, C_TEXT = b"\033[0m", b"\033[1;38;5;81m", b"\033[38;5;244m", b"\033[1;38;5;222m", b"\033[38;5;252m"


def strings(filename, color=False):
    """(prefix, before_match, after_match, line_close) as the reference composes them; filename None: no FILE: in front"""
    if not color:
        return (b"" if filename is None else filename + b":", b"", b"", b"")
    return (C_TEXT if filename is None else C_FILE + filename + RESET + C_SEP + b":" + C_TEXT, C_MATCH, C_TEXT, RESET)


class ColorLines(lm.Lines):
    """lm.Lines (spans, first_record, capped, lines_total) with .data following the rule above"""

    def __init__(self, text: bytes, records, fmt=(b"", b"", b"", b""), max_count=None):
        super().__init__(text, records, fmt[0], max_count)
        self.text, self.records = text, records
        self.data = self.render(fmt)

    def render(self, fmt) -> bytes:
        """the bytes with these strings (the lines and their records do not depend on them)"""
        prefix, before, after, close = fmt
        text, out = self.text, []
        for l, (a, z) in enumerate(self.spans):
            out.append(prefix)
            cur = a
            for s, e in self.records[self.first_record[l]:self.first_record[l + 1]][:lm.CAP]:
                e = min(e, z)
                if s >= e:
                    continue
                if s > cur:
                    out.append(text[cur:s])
                out += [before, text[s:e], after]
                cur = e
            if cur < z:
                out.append(text[cur:z])
            out += [close, b"\n"]
        return b"".join(out)

    def again(self, fmt) -> "ColorLines":
        """the same lines with other strings, without looking the lines up again"""
        import copy
        m = copy.copy(self)
        m.data = self.render(fmt)
        return m


def color_output(text: bytes, emitted, filename=FILE, color=True, max_count=None) -> bytes:
    """the CLI's stdout for the records a search emitted (in emission order)"""
    return ColorLines(text, lm.cut_to_max_count(emitted, max_count), strings(filename, color), max_count).data


class Case(lm.Case):
    def cli_args(self, color=True):
        a = lm.Case.cli_args(self)
        a[a.index("--color=never")] = "--color=always" if color else "--color=never"
        return a

    def string_mode_ok(self):
        """`krep --color=always -s PATTERN TEXT` can be asked: one case-sensitive pattern without -m, a text that fits a command line"""
        return (len(self.pats) == 1 and self.cs and self.max_count is None and len(self.text) <= 3000
                and b"\0" not in self.text and not self.text.startswith(b"-"))


def _as_color(case):
    return Case(case.key, case.text, case.pats, case.cs, case.ww, case.no_simd, case.max_count, case.want)


def table_cases():
    return [_as_color(c) for c in lm.table_cases()]


def random_cases():
    return [_as_color(c) for c in lm.random_cases()]


def run_cli(cli, case, path):
    """-> (exit code, stdout with the path inside the coloured prefix replaced by FILE); `path` holds case.text"""
    r = subprocess.run([cli] + case.cli_args() + [str(path)], capture_output=True, timeout=120)
    return r.returncode, r.stdout.replace(C_FILE + str(path).encode() + RESET, C_FILE + FILE + RESET)


def run_cli_string(cli, case):
    """-> (exit code, stdout) of `krep --color=always -s PATTERN TEXT`: the prefix without a filename"""
    a = case.cli_args()  # (one pattern: it is the last argument)
    r = subprocess.run([cli] + a[:-1] + ["-s", a[-1], case.text], capture_output=True, timeout=120)
    return r.returncode, r.stdout


digest = lm.digest


@contextlib.contextmanager
def _own_file():
    """line_model.Store reads and writes the file its module names: for the time of a call that is this module's"""
    keep, lm.GOLDEN = lm.GOLDEN, GOLDEN
    try:
        yield
    finally:
        lm.GOLDEN = keep


class Store(lm.Store):
    """line_model.Store over tests/golden/color_line_output.json: digests of the stock CLI's --color=always answers"""

    def __init__(self):
        with _own_file():
            super().__init__()

    def want(self, key, live=None) -> str:
        with _own_file():
            return super().want(key, live)

    def save(self):
        with _own_file():
            super().save()
