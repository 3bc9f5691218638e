"""Test helper: the rule krep -E follows for an alternation of fixed-length class sequences (include/krep_gpu.h, "alternations of
class sequences"), in Python.  The classes come from the same libc probing the library uses (regex_ref.probe_class, through
regex_model.classes); tests/test_regex_alt_model_cpu.py pins the rule to the compiled reference's regex_search.

TEST INFRASTRUCTURE: imported by the regex alternation tests only."""
from __future__ import annotations

import numpy as np

import regex_model
import regex_ref
from krep_amd import abi


def split(pattern: bytes):
    """the branches of one pattern of the accepted grammar: cut at every '|' outside brackets and not behind a backslash, one pair
    of parentheses around a branch taken off"""
    out, cur, i, n = [], b"", 0, len(pattern)
    while i < n:
        c = pattern[i:i + 1]
        if c == b"\\":
            cur += pattern[i:i + 2]
            i += 2
        elif c == b"[":
            k = i + len(regex_model.tokenize(pattern[i:])[0][0])
            cur += pattern[i:k]
            i = k
        elif c == b"|":
            out.append(cur)
            cur = b""
            i += 1
        else:
            cur += c
            i += 1
    out.append(cur)
    return [b[1:-1] if b.startswith(b"(") and b.endswith(b")") else b for b in out]


def joined(pats) -> bytes:
    """several patterns as the CLI hands them to regcomp: (p1)|(p2)|..."""
    return pats[0] if len(pats) == 1 else b"|".join(b"(" + p + b")" for p in pats)


def branches(pats, case_sensitive=True):
    """-> the merged branches of all patterns, each a list of L boolean tables [256]"""
    out = []
    for p in pats:
        for b in split(p):
            cl = regex_model.classes(b, case_sensitive)
            if not any(len(o) == len(cl) and all(np.array_equal(x, y) for x, y in zip(o, cl)) for o in out):
                out.append(cl)
    return out


def all_occurrences(brs, text: np.ndarray):
    """-> [(start, length)] of every branch's every occurrence, by start and then by length"""
    out = []
    for cl in brs:
        out += [(int(p), len(cl)) for p in regex_model.occurrences(cl, text)]
    return sorted(set(out))


def occurrences(brs, text: np.ndarray):
    """-> (starts ascending, len(p) = the longest branch that occurs at each)"""
    best = np.zeros(text.size, dtype=np.int64)
    for cl in brs:
        occ = regex_model.occurrences(cl, text)
        best[occ] = np.maximum(best[occ], len(cl))
    starts = np.flatnonzero(best)
    return starts, best[starts]


def cross_overlap(brs) -> bool:
    for i, a in enumerate(brs):
        for j, b in enumerate(brs):
            for d in range(1 if i == j else 0, len(a)):
                if all((a[d + t] & b[t]).any() for t in range(min(len(a) - d, len(b)))):
                    return True
    return False


def run(pats, text, case_sensitive=True, count_lines=False, max_count=abi.SIZE_MAX, track_positions=None, **_):
    """-> (returned count, positions[(n, 2) uint64]) as regex_search gives them for the alternation of `pats`"""
    text = text if isinstance(text, np.ndarray) else np.frombuffer(bytes(text), dtype=np.uint8)
    track = (not count_lines) if track_positions is None else bool(track_positions)
    none = np.zeros((0, 2), dtype=np.uint64)
    if text.size == 0:
        return 0, none
    starts, lens = occurrences(branches(pats, case_sensitive), text)
    if max_count == 0:
        return (0 if (count_lines or track) else int(starts.size > 0)), none
    if count_lines:
        nl_before = np.concatenate(([0], np.cumsum(text == 10)))[starts]
        return int(min(np.unique(nl_before).size, max_count)), none
    kept, cursor = [], 0
    for p, L in zip(starts.tolist(), lens.tolist()):
        if p >= cursor:
            kept.append((p, p + L))
            cursor = p + L
    n = min(len(kept), max_count)
    pos = np.asarray(kept[:n], dtype=np.uint64).reshape(-1, 2) if n else none
    return int(n), (pos if track else none)


def ref_call(pats, text, **kw):
    """regex_search of the compiled reference with the expression the CLI compiles for `pats`"""
    return regex_ref.call(joined(pats), text, **kw)
