"""Test helper: what a WINDOW of a loops search reports (include/krep_gpu.h, "*, + and {n,} behind an atom", Split with
krep_gpu_set_regex_loops_windows on), as brute force on top of tests/regex_loops_model.py and from the text alone:

  records      the whole-text records whose start lies in [lo, hi);
  line_count   the lines [ls, le) that hold such a record;
  head         one of those lines has ls <= lo: its owned match starts in front of the window's first newline;
  tail         one of those lines has le >= hi: it is still open where the window ends;
  has_newline  a newline inside text[lo, hi).

tests/test_regex_loops_window_model_cpu.py folds these quadruples with the library's krep_gpu_combine_line_counts and compares with the
compiled reference's -c: the bit rule the line walk kernel implements, pinned without a device.

TEST INFRASTRUCTURE: imported by the regex_loops window tests only."""
from __future__ import annotations

import numpy as np

import regex_loops_model as lm
from krep_amd import abi


def per_line(pats, text: np.ndarray, case_sensitive=True):
    """-> [(ls, le, [(start, end)])] over the lines of the whole text"""
    if text.size == 0:
        return []
    found = lm.matches(lm.branches(pats, case_sensitive), text, case_sensitive)
    return [(ls, le, m) for (ls, le), m in zip(lm.line_spans(text), found)]


def window(lines, text: np.ndarray, lo: int, hi: int):
    """-> (records [(start, end)], (line_count, head, tail, has_newline)) of the window [lo, hi) given per_line()'s answer"""
    records, count, head, tail = [], 0, False, False
    for ls, le, found in lines:
        own = [(s, e) for s, e in found if lo <= s < hi]
        records += own
        if own:
            count += 1
            head = head or ls <= lo
            tail = tail or le >= hi
    return records, (count, head, tail, bool((text[lo:hi] == 10).any()))


def scan_out(quad) -> abi.ScanOut:
    o = abi.ScanOut()
    o.line_count, o.head_line_hit, o.tail_line_hit, o.has_newline = quad[0], int(quad[1]), int(quad[2]), int(quad[3])
    o.count = o.total_matches = quad[0]
    return o


def cuts_to_windows(cuts, n: int):
    """the sorted cut offsets inside (0, n) -> the adjacent windows that cover [0, n)"""
    edges = [0] + sorted(set(c for c in cuts if 0 < c < n)) + [n]
    return list(zip(edges[:-1], edges[1:]))
