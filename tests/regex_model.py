"""Test helper: the rule krep -E follows for a fixed-length class sequence (include/krep_gpu.h, "krep -E on the device"), in
Python.  The classes come from the same libc probing the library uses (regex_ref.probe_class); tests/test_regex_model_cpu.py
pins the rule to the compiled reference's regex_search.

TEST INFRASTRUCTURE: imported by the regex tests only."""
from __future__ import annotations

import numpy as np

import regex_ref
from krep_amd import abi


def tokenize(pattern: bytes):
    """-> [(atom bytes, repetitions)] for the accepted grammar (the tests hand in accepted patterns only)"""
    out, i, n = [], 0, len(pattern)
    while i < n:
        c = pattern[i:i + 1]
        if c == b"{":
            k = pattern.index(b"}", i)
            out[-1] = (out[-1][0], int(pattern[i + 1:k]))
            i = k + 1
            continue
        if c == b"\\":
            ln = 2
        elif c == b"[":
            k = i + 1
            if pattern[k:k + 1] == b"^":
                k += 1
            if pattern[k:k + 1] == b"]":
                k += 1
            while pattern[k:k + 1] != b"]":
                if pattern[k:k + 1] == b"[" and pattern[k + 1:k + 2] in (b":", b".", b"="):
                    k = pattern.index(pattern[k + 1:k + 2] + b"]", k + 2) + 2
                else:
                    k += 1
            ln = k + 1 - i
        else:
            ln = 1
        out.append((pattern[i:i + ln], 1))
        i += ln
    return out


def classes(pattern: bytes, case_sensitive=True):
    """-> list of L boolean tables [256]"""
    cl = []
    for atom, rep in tokenize(pattern):
        t = np.zeros(256, dtype=bool)
        t[list(regex_ref.probe_class(atom, case_sensitive))] = True
        cl += [t] * rep
    return cl


def occurrences(cl, text: np.ndarray) -> np.ndarray:
    L, n = len(cl), text.size
    if n < L:
        return np.zeros(0, dtype=np.int64)
    ok = np.ones(n - L + 1, dtype=bool)
    for j, t in enumerate(cl):
        ok &= t[text[j:n - L + 1 + j]]
    return np.flatnonzero(ok)


def self_overlap(cl) -> bool:
    L = len(cl)
    return any(all((cl[j] & cl[j + d]).any() for j in range(L - d)) for d in range(1, L))


def run(pattern: bytes, text, case_sensitive=True, count_lines=False, max_count=abi.SIZE_MAX, track_positions=None, **_):
    """-> (returned count, positions[(n, 2) uint64]) as regex_search gives them"""
    text = text if isinstance(text, np.ndarray) else np.frombuffer(bytes(text), dtype=np.uint8)
    track = (not count_lines) if track_positions is None else bool(track_positions)
    none = np.zeros((0, 2), dtype=np.uint64)
    if text.size == 0:
        return 0, none
    cl = classes(pattern, case_sensitive)
    L = len(cl)
    occ = occurrences(cl, text)
    if max_count == 0:
        return (0 if (count_lines or track) else int(occ.size > 0)), none
    if count_lines:
        # the line of a start: the number of newlines in front of it (a start ON a newline belongs to the line that newline ends)
        nl_before = np.concatenate(([0], np.cumsum(text == 10)))[occ]
        return int(min(np.unique(nl_before).size, max_count)), none
    kept, cursor = [], 0
    for p in occ.tolist():
        if p >= cursor:
            kept.append(p)
            cursor = p + L
    k = np.asarray(kept[:max_count] if max_count != abi.SIZE_MAX else kept, dtype=np.uint64)
    pos = np.stack([k, k + np.uint64(L)], axis=1) if k.size else none
    return int(min(len(kept), max_count)), (pos if track else none)
