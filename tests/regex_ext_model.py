"""Test helper: the rule krep -E follows for what krep_gpu_regex_compile_ext() takes (include/krep_gpu.h, "?, {n,m}, inner groups and
anchored alternations"), as a brute-force numpy / Python model with its own expansion of the grammar, written independently of the
C one.  tests/test_regex_ext_model_cpu.py pins the rule to the compiled reference's regex_search.

TEST INFRASTRUCTURE: imported by the regex_ext tests only."""
from __future__ import annotations

import itertools

import numpy as np

import regex_alt_model
import regex_anchor_model
import regex_ref
from krep_amd import abi


def _atom_len(pattern: bytes, i: int) -> int:
    c = pattern[i:i + 1]
    if c == b"\\":
        return 2
    if c == b"[":  # POSIX 9.3.5: an optional ^, a ] directly behind is literal, [:name:] [.x.] [=x=] are stepped over
        k = i + 1
        k += pattern[k:k + 1] == b"^"
        k += pattern[k:k + 1] == b"]"
        while pattern[k:k + 1] != b"]":
            if pattern[k:k + 1] == b"[" and pattern[k + 1:k + 2] in (b":", b".", b"="):
                k = pattern.index(pattern[k + 1:k + 2] + b"]", k + 2) + 2
            else:
                k += 1
        return k + 1 - i
    return 1


def _quant(pattern: bytes, i: int):
    """-> (lo, hi, index behind the quantifier); (1, 1, i) when there is none"""
    c = pattern[i:i + 1]
    if c == b"?":
        return 0, 1, i + 1
    if c == b"{":
        k = pattern.index(b"}", i)
        lo, _, hi = pattern[i + 1:k].partition(b",")
        return int(lo), int(hi or lo), k + 1
    return 1, 1, i


LIMIT = 64  # more alternatives than this at any point of an expansion: OverflowError (the library stops at 8)


def _repeat(alts, lo, hi):
    """the alternatives of lo..hi items in a row, each item one of `alts` (tuples of atoms)"""
    out = []
    for k in range(lo, hi + 1):
        if len(out) + len(alts) ** k > LIMIT:
            raise OverflowError("the expansion is too wide for this model")
        for combo in itertools.product(alts, repeat=k):
            out.append(tuple(itertools.chain.from_iterable(combo)))
    return out


def _sequence(pattern: bytes, i: int, stop: bytes, groups: bool):
    """the alternatives of the items from i up to one of the bytes of `stop` (or the end) -> (list of atom tuples, index of the stop)"""
    seqs = [()]
    n = len(pattern)
    while i < n and pattern[i:i + 1] not in stop:
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
            alts, i = [(pattern[i:i + ln],)], i + ln
        lo, hi, i = _quant(pattern, i)
        alts = _repeat(alts, lo, hi)
        if len(seqs) * len(alts) > LIMIT:
            raise OverflowError("the expansion is too wide for this model")
        seqs = [s + a for s in seqs for a in alts]
    return seqs, i


def expand(pats):
    """-> (bol, eol, [tuple of atoms]) over the top-level branches of all patterns; the anchors are those of the first branch (the
    tests hand in accepted searches only: every branch carries the same pair)"""
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
    """-> (bol, eol, the merged branches, each a list of L boolean tables [256])"""
    bol, eol, seqs = expand(pats)
    out = []
    for s in seqs:
        cl = []
        for atom in s:
            t = np.zeros(256, dtype=bool)
            t[list(regex_ref.probe_class(atom, case_sensitive))] = True
            cl.append(t)
        if not any(len(o) == len(cl) and all(np.array_equal(x, y) for x, y in zip(o, cl)) for o in out):
            out.append(cl)
    return bol, eol, out


def all_occurrences(prog, text: np.ndarray, case_sensitive=True):
    """-> [(start, length)] of every branch's every occurrence"""
    bol, eol, brs = prog
    out = []
    for cl in brs:
        out += [(int(p), len(cl)) for p in regex_anchor_model.occurrences(cl, bol, eol, text, case_sensitive)]
    return sorted(set(out))


def occurrences(prog, text: np.ndarray, case_sensitive=True):
    """-> (starts ascending, the longest branch that occurs at each)"""
    bol, eol, brs = prog
    best = np.zeros(text.size + 1, dtype=np.int64)
    for cl in brs:
        occ = regex_anchor_model.occurrences(cl, bol, eol, text, case_sensitive)
        best[occ] = np.maximum(best[occ], len(cl))
    starts = np.flatnonzero(best)
    return starts, best[starts]


def run(pats, text, case_sensitive=True, count_lines=False, max_count=abi.SIZE_MAX, track_positions=None, **_):
    """-> (returned count, positions[(n, 2) uint64]) as regex_search gives them for `pats`"""
    text = text if isinstance(text, np.ndarray) else np.frombuffer(bytes(text), dtype=np.uint8)
    track = (not count_lines) if track_positions is None else bool(track_positions)
    none = np.zeros((0, 2), dtype=np.uint64)
    if text.size == 0:
        return 0, none
    starts, lens = occurrences(branches(pats, case_sensitive), text, case_sensitive)
    if max_count == 0:
        return (0 if (count_lines or track) else int(starts.size > 0)), none
    if count_lines:
        nl_before = np.concatenate(([0], np.cumsum(text == 10)))[starts]
        return int(min(np.unique(nl_before).size, max_count)), none
    kept, cursor = [], 0  # the anchors consume nothing
    for p, L in zip(starts.tolist(), lens.tolist()):
        if p >= cursor:
            kept.append((p, p + L))
            cursor = p + L
    n = min(len(kept), max_count)
    pos = np.asarray(kept[:n], dtype=np.uint64).reshape(-1, 2) if n else none
    return int(n), (pos if track else none)


def ref_call(pats, text, **kw):
    """regex_search of the compiled reference with the expression the CLI compiles for `pats`"""
    return regex_ref.call(regex_alt_model.joined(pats), text, **kw)
