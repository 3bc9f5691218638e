"""Test helper: the per-item max_count cut of a batch (krep_gpu_set_batch_max_count, include/krep_gpu.h "max_count behind a switch"),
in numpy, written from the rule's statement and not from the library's code.

For one item: R is its record list under NO max_count in the reference's emission order ((T, 2) uint64), Ln the distinct lines its
record starts lie on, M the max_count.  cut() is what the reference FUNCTION returns for the item alone under M (what
krep_gpu_search_batch reports); grep_cut() is what search_file() hands its formatter behind that function (what krep_gpu_grep_batch
prints from).

TEST INFRASTRUCTURE: imported by the batch max_count tests only (tests/test_batch_*max_count*_cpu.py, tests/test_gpu_*batch_max_count.py)."""
from __future__ import annotations

import numpy as np

import batch_model as bm
from krep_amd import abi

SIZE_MAX = abi.SIZE_MAX
FLUSH = 4096  # memchr_search's batch of stored positions
# the functions whose count-only call (no positions, no -c) answers 1 on the first hit under max_count == 0 (simd_avx2_search does so
# in its block body only: the batch refuses that cell, tests/test_batch_max_count_rule_cpu.py found it)
ZERO_ONE = (abi.RA_BMH, abi.RA_MEMCHR_SHORT, abi.RA_AVX2, abi.RA_REGEX)


def algo_of(eng, s: "bm.Search") -> int:
    """the reference function that does the work on a text not shorter than the pattern, as the batch rule takes it"""
    if s.regex:
        return abi.RA_REGEX
    if len(s.pats) > 1:
        return abi.RA_AHO_CORASICK
    s.configure(eng)
    try:
        return eng.mirror_select(s.params(), 1 << 20)
    finally:
        eng.set_thread_config(None)


def distinct_lines(text, records) -> int:
    nl = np.nonzero(bm.as_array(text) == 10)[0]
    return int(np.unique(np.searchsorted(nl, records.reshape(-1, 2)[:, 0].astype(np.int64), side="left")).size)


def cut(algo: int, kw: dict, total_list: np.ndarray, lines: int, max_count: int):
    """-> (count, records): the function's answer for the item under max_count.  kw: the Search's params (count_lines,
    track_positions); records are empty where the function stores none (count-only, -c)."""
    R = total_list.reshape(-1, 2).astype(np.uint64)
    T, M = R.shape[0], int(max_count)
    count_lines = bool(kw.get("count_lines"))
    track = bool(kw.get("track_positions", True)) and not count_lines
    if M == SIZE_MAX:
        return (lines if count_lines else T), (R if track else bm.NONE)
    if M == 0:
        one = (not track) and (not count_lines) and algo in ZERO_ONE and T > 0
        return (1 if one else 0), bm.NONE
    count = min(lines, M) if count_lines else min(T, M)
    if not track:
        return count, bm.NONE
    if algo == abi.RA_KMP and T > M:
        return count, R[:M + 1]
    if algo == abi.RA_MEMCHR and T > M and M % FLUSH == 0:
        return count, np.concatenate([R[:M - FLUSH], R[M:M + 1], R[M - FLUSH:M - 1]])
    return count, R[:M]


def by_start(R: np.ndarray) -> np.ndarray:
    R = R.reshape(-1, 2)
    return R[np.lexsort((R[:, 1], R[:, 0]))] if R.shape[0] else R


def grep_cut(algo: int, kw: dict, total_list: np.ndarray, lines: int, max_count: int):
    """-> (count, records): what search_file() prints from — the function's list cut to its first max_count records and put in
    (start, end) order; the count capped at max_count (krep.c:2954-2981, :3018-3026)"""
    k = dict(kw)
    k["track_positions"] = True
    count, recs = cut(algo, k, total_list, lines, max_count)
    M = int(max_count)
    if M != SIZE_MAX:
        recs = recs[:M]
    return min(count, M), by_start(recs)
