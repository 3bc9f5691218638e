"""Test helper: the two linear passes the device walks a line of more than 4096 bytes with (kg_regex_loops.hip, rx_long_walk;
krep_gpu_set_regex_long_lines), as a Python model over regex_groups_model.Automaton with the state sets as 32-bit masks:
  backward: C[p] = T[text[p]] & (F(p) | pred(C[p + 1])), C[le] = 0, F(p) = last where a match may end behind byte p;
  forward:  an attempt at s starts with S = first & C[s] and steps S = follow(S) & C[p].
Also counts the steps, so that a test can pin the work to a multiple of the line's length.

TEST INFRASTRUCTURE: imported by the regex_long_lines tests only."""
from __future__ import annotations

import numpy as np

from regex_loops_model import line_spans


def _mask(positions) -> int:
    m = 0
    for p in positions:
        m |= 1 << p
    return m


class Program:
    """the automaton as masks: T[byte], first, last, follow / pred per position"""

    def __init__(self, au):
        n = len(au.tables)
        self.first, self.last, self.bol, self.eol = _mask(au.first), _mask(au.last), bool(au.bol), bool(au.eol)
        self.follow = [_mask(f) for f in au.follow]
        self.pred = [_mask(q for q in range(n) if p in au.follow[q]) for p in range(n)]
        self.T = [_mask(i for i in range(n) if au.tables[i][b]) for b in range(256)]

    @staticmethod
    def step(S: int, rel) -> int:
        out, i = 0, 0
        while S:
            if S & 1:
                out |= rel[i]
            S >>= 1
            i += 1
        return out


def line_matches(pg: Program, text: np.ndarray, ls: int, le: int, steps=None):
    """-> [(start, end)] of the line [ls, le), by the two passes; steps (a list of one int) is advanced by every state step"""
    n = le - ls
    C = [0] * (n + 1)
    for p in range(le - 1, ls - 1, -1):
        F = pg.last if (not pg.eol or p + 1 == le) else 0
        C[p - ls] = pg.T[text[p]] & (F | Program.step(C[p + 1 - ls], pg.pred))
    work = n
    found, s = [], ls
    while s < le:
        S = pg.first & C[s - ls]
        best = None
        if S:
            p = s + 1
            while True:
                if S & pg.last and (not pg.eol or p == le):
                    best = p
                if p >= le:
                    break
                S = Program.step(S, pg.follow) & C[p - ls]
                work += 1
                if not S:
                    break
                p += 1
        else:
            work += 1
        if best is not None:
            found.append((s, best))
        if pg.bol:
            break
        s = best if best is not None else s + 1
    if steps is not None:
        steps[0] += work
    return found


def matches(au, text: np.ndarray, case_sensitive=True, steps=None):
    """-> [[(start, end)] per line], what regex_groups_model.matches() gives"""
    pg = Program(au)
    out = []
    for ls, le in line_spans(text):
        end_ok = (not au.eol) or le < text.size or case_sensitive  # the end of the text ends a line in a case-sensitive search only
        out.append(line_matches(pg, text, ls, le, steps) if end_ok and le > ls else [])
    return out


def line_counts(au, text: np.ndarray, case_sensitive=True) -> int:
    """-c by the backward pass alone: a line is counted when some C[s] meets first (with ^: C[ls])"""
    pg = Program(au)
    total = 0
    for ls, le in line_spans(text):
        if le <= ls or not ((not au.eol) or le < text.size or case_sensitive):
            continue
        c, seen = 0, 0
        for p in range(le - 1, ls - 1, -1):
            F = pg.last if (not pg.eol or p + 1 == le) else 0
            c = pg.T[text[p]] & (F | Program.step(c, pg.pred))
            seen |= c
        total += int(bool((c if pg.bol else seen) & pg.first))
    return total
