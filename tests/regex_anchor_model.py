"""Test helper: the rule krep -E follows for a class sequence between line anchors (include/krep_gpu.h, "line anchors around a
class sequence"), in numpy.  tests/test_regex_anchor_model_cpu.py pins it to the compiled reference's regex_search.

TEST INFRASTRUCTURE: imported by the anchored regex tests only."""
from __future__ import annotations

import numpy as np

import regex_model
from krep_amd import abi


def split(pattern: bytes):
    """-> (bol, the pattern between the anchors, eol) for the accepted grammar: ^ is an anchor as the first byte, $ as the last one
    when the walk over atoms STANDS on it (behind a backslash or inside a bracket it is part of an atom)"""
    bol = pattern[:1] == b"^"
    i, n = int(bol), len(pattern)
    while i < n:
        c = pattern[i:i + 1]
        if c == b"$" and i == n - 1:
            return bol, pattern[int(bol):n - 1], True
        if c == b"\\":
            i += 2
        elif c == b"{":
            i = pattern.index(b"}", i) + 1
        elif c == b"[":
            i += len(regex_model.tokenize(pattern[i:])[0][0])
        else:
            i += 1
    return bol, pattern[int(bol):], False


def occurrences(cl, bol, eol, text: np.ndarray, case_sensitive=True) -> np.ndarray:
    """the positions p with text[p + j] in Cj; with bol: p == 0 or text[p - 1] == '\\n'; with eol: text[p + L] == '\\n', or p + L == len
    in a case-sensitive search (regex_search ORs REG_ICASE into regexec's eflags, where that bit is REG_NOTEOL: under -i the end of
    the text is no end of a line)"""
    occ = regex_model.occurrences(cl, text)
    L, n = len(cl), text.size
    if bol:
        occ = occ[(occ == 0) | (text[np.maximum(occ, 1) - 1] == 10)]
    if eol:
        occ = occ[((occ + L == n) & bool(case_sensitive)) | ((occ + L < n) & (text[np.minimum(occ + L, n - 1)] == 10))]
    return occ


def self_overlap(cl, bol, eol) -> bool:
    L = len(cl)
    return any(all((cl[j] & cl[j + d]).any() for j in range(L - d)) and (not bol or cl[d - 1][10]) and (not eol or cl[L - d][10])
               for d in range(1, L))


def run(pattern: bytes, text, case_sensitive=True, count_lines=False, max_count=abi.SIZE_MAX, track_positions=None, **_):
    """-> (returned count, positions[(n, 2) uint64]) as regex_search gives them"""
    text = text if isinstance(text, np.ndarray) else np.frombuffer(bytes(text), dtype=np.uint8)
    track = (not count_lines) if track_positions is None else bool(track_positions)
    none = np.zeros((0, 2), dtype=np.uint64)
    if text.size == 0:
        return 0, none
    bol, core, eol = split(pattern)
    cl = regex_model.classes(core, case_sensitive)
    L = len(cl)
    occ = occurrences(cl, bol, eol, text, case_sensitive)
    if max_count == 0:
        return (0 if (count_lines or track) else int(occ.size > 0)), none
    if count_lines:
        # the line of a start: the number of newlines in front of it (a start ON a newline belongs to the line that newline ends)
        nl_before = np.concatenate(([0], np.cumsum(text == 10)))[occ]
        return int(min(np.unique(nl_before).size, max_count)), none
    kept, cursor = [], 0  # the anchors consume nothing: the search resumes at p + L
    for p in occ.tolist():
        if p >= cursor:
            kept.append(p)
            cursor = p + L
    k = np.asarray(kept[:max_count] if max_count != abi.SIZE_MAX else kept, dtype=np.uint64)
    pos = np.stack([k, k + np.uint64(L)], axis=1) if k.size else none
    return int(min(len(kept), max_count)), (pos if track else none)
