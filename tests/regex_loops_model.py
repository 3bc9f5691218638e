"""Test helper: the rule krep -E follows for what krep_gpu_regex_compile_loops() takes (include/krep_gpu.h, "*, + and {n,} behind an
atom"), as a brute-force Python model with its own expansion of the grammar, written independently of the C one: sequences of places
of which some repeat, matched line by line, leftmost start and longest end.  tests/test_regex_loops_model_cpu.py pins the rule to the
compiled reference's regex_search.  Also the filter rule (the cheapest factor of every branch), over exact fractions.

TEST INFRASTRUCTURE: imported by the regex_loops tests only."""
from __future__ import annotations

import itertools
from fractions import Fraction

import numpy as np

import regex_alt_model
import regex_ref
from krep_amd import abi
from regex_ext_model import _atom_len

LIMIT = 64  # more alternatives than this at any point of an expansion: OverflowError (the library stops at 8)


def _quant(pattern: bytes, i: int):
    """-> (lo, hi or None for no bound, index behind the quantifier); (1, 1, i) when there is none"""
    c = pattern[i:i + 1]
    if c == b"?":
        return 0, 1, i + 1
    if c == b"*":
        return 0, None, i + 1
    if c == b"+":
        return 1, None, i + 1
    if c == b"{":
        k = pattern.index(b"}", i)
        lo, comma, hi = pattern[i + 1:k].partition(b",")
        return int(lo), (int(hi) if hi else (None if comma else int(lo))), k + 1
    return 1, 1, i


def _repeat(alts, lo, hi):
    out = []
    for k in range(lo, hi + 1):
        if len(out) + len(alts) ** k > LIMIT:
            raise OverflowError("the expansion is too wide for this model")
        for combo in itertools.product(alts, repeat=k):
            out.append(tuple(itertools.chain.from_iterable(combo)))
    return out


def _sequence(pattern: bytes, i: int, stop: bytes, groups: bool):
    """the alternatives of the items from i up to one of the bytes of `stop` (or the end): each a tuple of places (atom, repeats)"""
    seqs = [()]
    n = len(pattern)
    while i < n and pattern[i:i + 1] not in stop:
        atom = None
        if groups and pattern[i:i + 1] == b"(":
            alts, i = [], i + 1
            while True:
                part, i = _sequence(pattern, i, b"|)", False)
                alts += part
                i += 1
                if pattern[i - 1:i] == b")":
                    break
        else:
            ln = _atom_len(pattern, i)
            atom = pattern[i:i + ln]
            alts, i = [((atom, False),)], i + ln
        lo, hi, i = _quant(pattern, i)
        if hi is None:
            assert atom is not None, "an unbounded quantifier behind a group"
            tail = ((atom, False),) * max(lo - 1, 0) + ((atom, True),)
            alts = [(), tail] if lo == 0 else [tail]
        else:
            alts = _repeat(alts, lo, hi)
        if len(seqs) * len(alts) > LIMIT:
            raise OverflowError("the expansion is too wide for this model")
        seqs = [s + a for s in seqs for a in alts]
    return seqs, i


def expand(pats):
    """-> (bol, eol, [tuple of places (atom, repeats)]) over the top-level branches of all patterns"""
    out, bol, eol = [], None, None
    for pat in pats:
        i, n = 0, len(pat)
        while True:
            b = pat[i:i + 1] == b"^"
            seqs, i = _sequence(pat, i + int(b), b"|$", True)
            e = pat[i:i + 1] == b"$"
            i += int(e)
            if bol is None:
                bol, eol = b, e
            assert (bol, eol) == (b, e), "mixed anchors"
            out += seqs
            if i >= n:
                break
            assert pat[i:i + 1] == b"|"
            i += 1
    return bool(bol), bool(eol), out


def branches(pats, case_sensitive=True):
    """-> (bol, eol, the merged branches, each a list of places (boolean table [256], repeats))"""
    bol, eol, seqs = expand(pats)
    out = []
    for s in seqs:
        br = []
        for atom, plus in s:
            t = np.zeros(256, dtype=bool)
            t[list(regex_ref.probe_class(atom, case_sensitive))] = True
            br.append((t, plus))
        same = lambda o: len(o) == len(br) and all(np.array_equal(x[0], y[0]) and x[1] == y[1] for x, y in zip(o, br))
        if not any(same(o) for o in out):
            out.append(br)
    return bol, eol, out


def accepted(pats, case_sensitive=True) -> bool:
    """what the compiler's limits say about an expression of the grammar: an unbounded quantifier somewhere, no empty sequence, no
    class with a newline, at most 8 sequences of at most 16 places (^ and $ one each), at most 32 in all"""
    try:
        bol, eol, brs = branches(pats, case_sensitive)
    except OverflowError:
        return False
    extra = int(bol) + int(eol)
    return (any(plus for br in brs for _, plus in br) and all(len(br) for br in brs) and not any(t[10] for br in brs for t, _ in br)
            and len(brs) <= 8 and all(len(br) + extra <= 16 for br in brs) and sum(len(br) + extra for br in brs) <= 32)


def ends(br, text: np.ndarray, s: int, le: int):
    """every e such that text[s, e) is cut into non-empty runs, one per place of br and in order, e <= le"""
    cur = {s}
    for table, plus in br:
        nxt = set()
        for p in cur:
            q = p
            while q < le and table[text[q]]:
                q += 1
                nxt.add(q)
                if not plus:
                    break
        cur = nxt
        if not cur:
            break
    return cur


def line_spans(text: np.ndarray):
    """[0, first newline), every stretch between two newlines, what stands behind the last newline if that is not empty"""
    nl = np.flatnonzero(text == 10).tolist()
    lo = [0] + [p + 1 for p in nl]
    hi = nl + [int(text.size)]
    return [(a, b) for a, b in zip(lo, hi) if not (a == b == text.size)]


def matches(prog, text: np.ndarray, case_sensitive=True):
    """-> [[(start, end)] per line] in the order of the lines"""
    bol, eol, brs = prog
    out = []
    for ls, le in line_spans(text):
        found, resume = [], ls
        end_ok = (not eol) or le < text.size or case_sensitive  # the end of the text ends a line in a case-sensitive search only
        s = resume
        while s < le and end_ok:
            es = set()
            for br in brs:
                es |= {e for e in ends(br, text, s, le) if not eol or e == le}
            if es:
                found.append((s, max(es)))
                s = max(es)
                if bol:
                    break
            else:
                if bol:
                    break
                s += 1
        out.append(found)
    return out


def run(pats, text, case_sensitive=True, count_lines=False, max_count=abi.SIZE_MAX, track_positions=None, **_):
    """-> (returned count, positions[(n, 2) uint64]) as regex_search gives them for `pats`"""
    text = text if isinstance(text, np.ndarray) else np.frombuffer(bytes(text), dtype=np.uint8)
    track = (not count_lines) if track_positions is None else bool(track_positions)
    none = np.zeros((0, 2), dtype=np.uint64)
    if text.size == 0:
        return 0, none
    per_line = matches(branches(pats, case_sensitive), text, case_sensitive)
    kept = [m for line in per_line for m in line]
    if max_count == 0:
        return (0 if (count_lines or track) else int(len(kept) > 0)), none
    if count_lines:
        return int(min(sum(1 for line in per_line if line), max_count)), none
    n = min(len(kept), max_count)
    pos = np.asarray(kept[:n], dtype=np.uint64).reshape(-1, 2) if n else none
    return int(n), (pos if track else none)


def ref_call(pats, text, **kw):
    """regex_search of the compiled reference with the expression the CLI compiles for `pats`"""
    return regex_ref.call(regex_alt_model.joined(pats), text, **kw)


def filter_of(pats, case_sensitive=True):
    """The filter: per branch the factor (a run of places none of which, strictly inside it, repeats) with the smallest product of
    |class| / 256, on a tie the longer, then the leftmost; identical factors merge.  -> [list of boolean tables]"""
    _, _, brs = branches(pats, case_sensitive)
    out = []
    for br in brs:
        best = None
        for a in range(len(br)):
            for b in range(a, len(br)):
                if any(br[k][1] for k in range(a + 1, b)):
                    break
                cost = Fraction(1)
                for k in range(a, b + 1):
                    cost *= Fraction(int(br[k][0].sum()), 256)
                key = (cost, -(b - a + 1), a)
                if best is None or key < best[0]:
                    best = (key, [br[k][0] for k in range(a, b + 1)])
        f = best[1]
        if not any(len(o) == len(f) and all(np.array_equal(x, y) for x, y in zip(o, f)) for o in out):
            out.append(f)
    return out


def filter_occurs(flt, text: np.ndarray, ls: int, le: int) -> bool:
    """does some sequence of the filter occur inside text[ls, le)"""
    for f in flt:
        for p in range(ls, le - len(f) + 1):
            if all(t[text[p + j]] for j, t in enumerate(f)):
                return True
    return False
