"""What the reference prints under -o (`krep -o PATTERN FILE`): one FILE:LINE:match per match.  A plain-Python statement of the
rules, for the tests of krep_gpu_format_matches / Plan.grep_only_matching.

TEST INFRASTRUCTURE.  The rules (tests/test_only_matching_model_cpu.py pins them to the stock CLI):
  1. the list is the search's records cut to their first max_count in emission order, then in (start, end) order; n is its length;
  2. record i prints  prefix before_number LINE ":" after_number MATCH after_match "\\n"  — the four strings are empty without
     colour except prefix = "FILE:"; with colour they are the escape codes of the reference's header around the same fields;
  3. MATCH is text[start:end] with every newline replaced by a blank;
  4. LINE is 1 + the newlines in front of the start (a start ON a newline belongs to the line that newline ends), except: with
     more than 10 records in the list and at least one newline in the text, a record that starts behind the text's last newline
     prints the LINE of the nearest earlier record that starts at or before the last newline, or 1 when there is none.
"""
from __future__ import annotations

import contextlib
import os
import random
import subprocess

import line_model as lm

STALE_AFTER = 10
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "only_matching_output.json")
FILE = lm.FILE

# the reference's colours (data: the escape codes of its header)
RESET, C_FILE, C_SEP, C_LINE, C_MATCH = b"\033[0m", b"\033[1;38;5;81m", b"\033[38;5;244m", b"\033[1;38;5;111m", b"\033[1;38;5;222m"


def strings(filename, color=False):
    """(prefix, before_number, after_number, after_match) as the reference composes them; filename None: no FILE: in front"""
    if not color:
        return (b"" if filename is None else filename + b":", b"", b"", b"")
    return (b"" if filename is None else C_FILE + filename + RESET + C_SEP + b":", C_LINE, RESET + C_MATCH, RESET)


def line_numbers(text: bytes, records):
    """the LINE of every record of the list (rule 4)"""
    true, at, ln = [], 0, 1
    for s, _ in records:  # (counted on from the record before it where the list ascends: the large cases)
        ln = ln + text.count(b"\n", at, s) if s >= at else 1 + text.count(b"\n", 0, s)
        at = s
        true.append(ln)
    last_nl = text.rfind(b"\n")
    if len(records) <= STALE_AFTER or last_nl < 0:
        return true
    out, left = [], 1
    for (s, _), ln in zip(records, true):
        if s <= last_nl:
            left = ln
        out.append(left)
    return out


def stale_records(text: bytes, records) -> int:
    """records that print another number than their true one could be: those behind the last newline of a list of more than 10"""
    last_nl = text.rfind(b"\n")
    return sum(1 for s, _ in records if s > last_nl) if len(records) > STALE_AFTER and last_nl >= 0 else 0


def only_matching_output(text: bytes, records, fmt=(b"", b"", b"", b""), max_items=None) -> bytes:
    """the bytes for a list that is already cut and ordered (what krep_gpu_format_matches takes)"""
    prefix, before, after, tail = fmt
    lines = line_numbers(text, records)
    shown = records if max_items is None else records[:max_items]
    return b"".join(prefix + before + b"%d:" % ln + after + text[s:e].replace(b"\n", b" ") + tail + b"\n"
                    for (s, e), ln in zip(shown, lines))


def grep_o_output(text: bytes, emitted, filename=FILE, color=False, max_count=None) -> bytes:
    """the CLI's stdout for the records a search under -o emitted (in emission order)"""
    return only_matching_output(text, lm.cut_to_max_count(emitted, max_count), strings(filename, color))


class Case(lm.Case):
    def cli_args(self, color=False):
        a = lm.Case.cli_args(self)
        a[a.index("--color=never")] = "--color=always" if color else "--color=never"
        return ["-o"] + a

    def emitted(self, chk, abi):
        """the records the reference's search emits under -o (the restatement: only_matching is a file-static of the reference)"""
        chk.set_only_matching(True)
        try:
            return lm.Case.emitted(self, chk, abi)
        finally:
            chk.set_only_matching(False)


def table_cases():
    f = FILE + b":"
    sh = b"xx Sherlock yy\n"
    three = [b"Sherlock", b"lock", b"er"]
    rows = lambda nums, m: b"".join(f + b"%d:" % k + m + b"\n" for k in nums)  # noqa: E731
    return [
        # 10 records print true numbers; with an 11th the newline index is used and the records behind the last newline go stale
        Case("table/ten", b"xa\nya\n" + b"a" * 8, [b"a"], want=rows([1, 2] + [3] * 8, b"a")),
        Case("table/eleven", b"xa\nya\n" + b"a" * 9, [b"a"], want=rows([1, 2] + [2] * 9, b"a")),
        Case("table/eleven-m10", b"xa\nya\n" + b"a" * 9, [b"a"], max_count=10, want=rows([1, 2] + [3] * 8, b"a")),
        Case("table/all-behind", b"x\n" + b"a" * 11, [b"a"], want=rows([1] * 11, b"a")),
        Case("table/no-newline", b"a" * 12, [b"a"], want=rows([1] * 12, b"a")),
        Case("table/stale-12", b"a\n" * 12 + b"aa", [b"a"], want=rows(list(range(1, 13)) + [12, 12], b"a")),
        Case("table/final-newline", b"a\n" * 12 + b"aa\n", [b"a"], want=rows(list(range(1, 13)) + [13, 13], b"a")),
        Case("table/newline-inside", b"ab\ncd\nab\ncd\n", [b"b\nc"], want=rows([1, 3], b"b c")),
        Case("table/newline-first", b"ab\ncd\nab\ncd\n", [b"\ncd"], want=rows([1, 3], b" cd")),
        Case("table/nested", sh, three, want=rows([1], b"Sherlock") + rows([1], b"er") + rows([1], b"lock")),
        Case("table/m1", sh, three, max_count=1, want=rows([1], b"er")),  # the first in emission order: the one that ends first
        Case("table/m-is-n", sh, three, max_count=3, want=rows([1], b"Sherlock") + rows([1], b"er") + rows([1], b"lock")),
        Case("table/digits", b"a\n" * 101, [b"a"], want=rows(range(1, 102), b"a")),
        Case("table/digits-stale", b"a\n" * 100 + b"b\nab" + b"a" * 20, [b"a"], want=rows(list(range(1, 101)) + [100] * 21, b"a")),
    ]


ALPHABETS = [b"ab\n", b"abA \n", b"abc_ \n", b"aAbB\n", b"ab", b"ab\n\n"]  # those of line_model.random_cases


def random_cases(count=288, seed=20261017):
    rng = random.Random(seed)
    out = []
    for k in range(count):
        alpha = rng.choice(ALPHABETS)
        n = rng.choice([1, 2, 5, 17, 40, 40, 200, 200, 1000, 3000] if k % 3 != 1 else [17, 40, 200, 200, 1000, 3000])
        text = bytearray(rng.choice(alpha) for _ in range(n))
        letters = bytes(c for c in alpha if c != 10)
        if k % 3 == 0:
            text[-1] = 10          # a final newline
        elif k % 3 == 1:           # none, and a last line of some length: where the numbers go stale
            text += bytes(rng.choice(letters) for _ in range(rng.randrange(1, 60)))
        text = bytes(text)
        n = len(text)

        def pick(m):
            m = min(m, n)
            where = rng.random()
            s = 0 if where < 0.2 else (n - m if where < 0.4 else rng.randrange(0, n - m + 1))  # offset 0 / up to text_len
            p = text[s:s + m]
            if where > 0.85 or p[:1] == b"\n" or not p:
                p = bytes(rng.choice(letters) for _ in range(m))
            return p

        kind = k % 6
        mc = rng.choice([None] * (5 if k % 3 != 1 else 9) + [1, 2, 3, 7, 10, 11, 11])
        if kind in (0, 1):       # one literal: SIMD / --no-simd
            out.append(Case(f"rand/{k}", text, [pick(rng.choice([1, 2, 3, 4, 6]))], no_simd=kind == 1, max_count=mc))
        elif kind == 2:
            out.append(Case(f"rand/{k}", text, [pick(rng.choice([1, 2, 3, 5]))], cs=False, max_count=mc))
        elif kind == 3:
            out.append(Case(f"rand/{k}", text, [pick(rng.choice([1, 2, 3]))], ww=True, cs=rng.random() < 0.7, max_count=mc))
        else:                    # a dictionary with nested patterns
            pats = [pick(rng.choice([3, 4, 6]))]
            while len(pats) < rng.randrange(2, 7):
                big = rng.choice(pats)
                if len(big) > 1 and rng.random() < 0.6:
                    a = rng.randrange(0, len(big))
                    p = big[a:rng.randrange(a + 1, len(big) + 1)]
                else:
                    p = pick(rng.choice([1, 2, 3, 5]))
                if p and p[:1] != b"\n" and p not in pats:
                    pats.append(p)
            out.append(Case(f"rand/{k}", text, pats, cs=rng.random() < 0.8, max_count=mc))
    return out


def run_cli(cli, case, path, color=False):
    """-> (exit code, stdout with the path replaced by FILE); `path` holds case.text"""
    r = subprocess.run([cli] + case.cli_args(color) + [str(path)], capture_output=True, timeout=120)
    return r.returncode, r.stdout.replace(str(path).encode(), FILE)


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
    """line_model.Store over tests/golden/only_matching_output.json: digests of the stock CLI's -o answers"""

    def __init__(self):
        with _own_file():
            super().__init__()

    def want(self, key, live=None) -> str:
        with _own_file():
            return super().want(key, live)

    def save(self):
        with _own_file():
            super().save()
