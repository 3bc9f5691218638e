"""Test helper: the rule krep -E follows for what krep_gpu_regex_compile_groups() takes (include/krep_gpu.h, "repeated and nested
groups"), as a brute-force Python model with its own recursive parser, written independently of the C one: the position (Glushkov)
automaton of the expression, simulated as a set of positions line by line, leftmost start and longest end over all paths.
tests/test_regex_groups_model_cpu.py pins the rule to the compiled reference's regex_search.  Also a checker of the filter property.

TEST INFRASTRUCTURE: imported by the regex_groups tests only."""
from __future__ import annotations

import numpy as np

import regex_alt_model
import regex_ref
from krep_amd import abi
from regex_ext_model import _atom_len
from regex_loops_model import line_spans

MAX_POS, MAX_DEPTH = 32, 8


class Refused(Exception):
    """an expression outside the grammar or the limits; the text says which"""


class Automaton:
    def __init__(self):
        self.atoms = []       # the atom (pattern bytes) of every position
        self.follow = []      # a set per position
        self.first, self.last = set(), set()
        self.bol = self.eol = False
        self.tables = None    # boolean [256] per position, set by automaton()


class _Parser:
    """item = atom quant? | '(' alt ')' quant?; every sub-expression is (nullable, first, last) over positions made as it is read"""

    def __init__(self, pat: bytes, au: Automaton):
        self.p, self.i, self.au = pat, 0, au

    def peek(self):
        return self.p[self.i:self.i + 1]

    def atom(self):
        ln = _atom_len(self.p, self.i)
        if len(self.au.atoms) >= MAX_POS:
            raise Refused("positions")
        self.au.atoms.append(self.p[self.i:self.i + ln])
        self.au.follow.append(set())
        self.i += ln
        k = len(self.au.atoms) - 1
        return False, {k}, {k}

    def operand(self, depth):
        if self.peek() == b"(":
            if depth >= MAX_DEPTH:
                raise Refused("depth")
            self.i += 1
            r = self.alt(depth + 1, b")")
            if self.peek() != b")":
                raise Refused("unbalanced")
            self.i += 1
            return r
        if self.peek() in (b"^", b"$"):
            raise Refused("anchor")
        return self.atom()

    def link(self, a, b):
        for x in a:
            self.au.follow[x] |= b

    def cat(self, A, B):
        if A is None:
            return B
        self.link(A[2], B[1])
        return A[0] and B[0], A[1] | (B[1] if A[0] else set()), B[2] | (A[2] if B[0] else set())

    def quant(self):
        """-> (lo, hi or None for no bound) and steps over it; None when there is none"""
        c = self.peek()
        if c not in (b"?", b"*", b"+", b"{"):
            return None
        if c == b"{":
            k = self.p.index(b"}", self.i)
            lo, comma, hi = self.p[self.i + 1:k].partition(b",")
            q = int(lo), (int(hi) if hi else (None if comma else int(lo)))
            self.i = k + 1
        else:
            q = {b"?": (0, 1), b"*": (0, None), b"+": (1, None)}[c]
            self.i += 1
        if self.peek() in (b"?", b"*", b"+", b"{"):
            raise Refused("quantifier behind a quantifier")
        if q[1] == 0:
            raise Refused("zero times")
        return q

    def item(self, depth):
        start = self.i
        X = self.operand(depth)
        q = self.quant()
        if q is None:
            return X
        behind, (lo, hi) = self.i, q

        def again():
            self.i = start
            return self.operand(depth)

        def loop(Y, star):
            self.link(Y[2], Y[1])
            return Y[0] or star, Y[1], Y[2]

        copies = [X]
        acc = None
        if hi is None:   # X{lo,}: lo - 1 copies and a loop
            for k in range(max(lo - 1, 0)):
                acc = self.cat(acc, copies.pop() if copies else again())
            acc = self.cat(acc, loop(copies.pop() if copies else again(), lo == 0))
        else:            # X{lo,hi}: lo copies and hi - lo optional ones
            for k in range(hi):
                Y = copies.pop() if copies else again()
                acc = self.cat(acc, Y if k < lo else (True, Y[1], Y[2]))
        self.i = behind
        return acc

    def seq(self, depth, stop, top):
        acc = None
        while self.i < len(self.p) and self.peek() not in stop:
            if top and self.peek() == b"$" and (self.i + 1 == len(self.p) or self.p[self.i + 1:self.i + 2] == b"|"):
                break
            if self.peek() in (b"?", b"*", b"+", b"{"):
                raise Refused("quantifier behind nothing")
            acc = self.cat(acc, self.item(depth))
        if acc is None:
            raise Refused("empty alternative")
        return acc

    def alt(self, depth, stop):
        out = None
        while True:
            S = self.seq(depth, b"|" + stop, False)
            out = S if out is None else (out[0] or S[0], out[1] | S[1], out[2] | S[2])
            if self.peek() != b"|":
                return out
            self.i += 1


def automaton(pats, case_sensitive=True) -> Automaton:
    """the position automaton of the top-level branches of all patterns; Refused for what the grammar and the limits do not admit"""
    au = Automaton()
    anchors = None
    for pat in pats:
        ps = _Parser(pat, au)
        while True:
            b = ps.peek() == b"^"
            ps.i += int(b)
            S = ps.seq(0, b"|)", True)
            e = ps.peek() == b"$"
            ps.i += int(e)
            if anchors is None:
                anchors = (b, e)
            if anchors != (b, e):
                raise Refused("mixed anchors")
            if S[0]:
                raise Refused("nullable")
            au.first |= S[1]
            au.last |= S[2]
            if ps.i >= len(pat):
                break
            if ps.peek() != b"|":
                raise Refused("unbalanced")
            ps.i += 1
    au.bol, au.eol = anchors
    au.tables = []
    for a in au.atoms:
        t = np.zeros(256, dtype=bool)
        t[list(regex_ref.probe_class(a, case_sensitive))] = True
        if t[10]:
            raise Refused("newline")
        au.tables.append(t)
    return au


def from_compiled(g: dict) -> Automaton:
    """the automaton Engine.regex_compile_groups() returned, to be simulated by the same matcher"""
    au = Automaton()
    au.first, au.last, au.follow, au.bol, au.eol = set(g["first"]), set(g["last"]), [set(f) for f in g["follow"]], g["bol"], g["eol"]
    au.tables = []
    for c in g["classes"]:
        t = np.zeros(256, dtype=bool)
        t[list(c)] = True
        au.tables.append(t)
    return au


def longest_end(au: Automaton, text: np.ndarray, s: int, le: int):
    """the largest e <= le such that the automaton accepts text[s, e) (with eol: e == le), or None"""
    S = {p for p in au.first if au.tables[p][text[s]]}
    best, p = None, s + 1
    while S:
        if S & au.last and (not au.eol or p == le):
            best = p
        if p >= le:
            break
        nxt = set()
        for q in S:
            nxt |= au.follow[q]
        S = {q for q in nxt if au.tables[q][text[p]]}
        p += 1
    return best


def matches(au: Automaton, text: np.ndarray, case_sensitive=True):
    """-> [[(start, end)] per line]: ascending starts, the longest end, resume at the end; with bol only the line's first byte"""
    out = []
    for ls, le in line_spans(text):
        found, s = [], ls
        end_ok = (not au.eol) or le < text.size or case_sensitive  # the end of the text ends a line in a case-sensitive search only
        while s < le and end_ok:
            e = longest_end(au, text, s, le)
            if e is not None:
                found.append((s, e))
                s = e
            else:
                s += 1
            if au.bol:
                break
        out.append(found)
    return out


def run_automaton(au, text, case_sensitive=True, count_lines=False, max_count=abi.SIZE_MAX, track_positions=None, **_):
    """-> (returned count, positions[(n, 2) uint64]) as regex_search gives them"""
    text = text if isinstance(text, np.ndarray) else np.frombuffer(bytes(text), dtype=np.uint8)
    track = (not count_lines) if track_positions is None else bool(track_positions)
    none = np.zeros((0, 2), dtype=np.uint64)
    if text.size == 0:
        return 0, none
    per_line = matches(au, text, case_sensitive)
    kept = [m for line in per_line for m in line]
    if max_count == 0:
        return (0 if (count_lines or track) else int(len(kept) > 0)), none
    if count_lines:
        return int(min(sum(1 for line in per_line if line), max_count)), none
    n = min(len(kept), max_count)
    pos = np.asarray(kept[:n], dtype=np.uint64).reshape(-1, 2) if n else none
    return int(n), (pos if track else none)


def run(pats, text, case_sensitive=True, **kw):
    return run_automaton(automaton(pats, case_sensitive), text, case_sensitive=case_sensitive, **kw)


def ref_call(pats, text, **kw):
    """regex_search of the compiled reference with the expression the CLI compiles for `pats`"""
    return regex_ref.call(regex_alt_model.joined(pats), text, **kw)


def filter_misses(flt, text: np.ndarray, records) -> list:
    """the records (start, end) that hold no occurrence of a filter sequence (lists of byte sets) as consecutive bytes: must be empty"""
    bad = []
    for s, e in records:
        s, e = int(s), int(e)
        if not any(all(text[p + j] in f[j] for j in range(len(f))) for f in flt for p in range(s, e - len(f) + 1)):
            bad.append((s, e))
    return bad
