"""What `krep [-o | -c] PATTERN` prints for every file of a batch, in batch order (krep_gpu_grep_batch, krep_gpu_format_lines_items,
krep_gpu_format_matches_items; include/krep_gpu.h "the grep output of a batch").  Two statements of the expected bytes:

  (a) definition(): per item the single-text model on the item ALONE with its own name — line_model.grep_output without colour,
      color_line_model.color_output with it, only_matching_model.grep_o_output under -o, "FILE:COUNT" under -c — concatenated;
  (b) from_pack(): what the kernels implement, from the PACK (the items joined by one newline), its offset table and the
      pack-relative record list: the lines of the pack with the prefix of the item the line's first record lies in; under -o the
      line number of the pack minus the newlines in front of the item, and per item its last newline and its stale value (numpy).

TEST INFRASTRUCTURE: imported by tests/test_batch_grep_model_cpu.py, tests/test_gpu_batch_format.py, tests/test_gpu_grep_batch.py."""
from __future__ import annotations

import contextlib
import os

import numpy as np

import batch_model as bm
import color_line_model as clm
import line_model as lm
import only_matching_model as omm

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "batch_grep_output.json")
MODES = ("lines", "matches", "count")


def prefix(name: bytes, mode: str, color: bool) -> bytes:
    """the bytes in front of a line / a match / a count of the file `name`"""
    if mode == "lines":
        return clm.strings(name, color)[0]
    if mode == "matches":
        return omm.strings(name, color)[0]
    return name + b":"  # (krep.c:3016: a count is never coloured)


def strings(mode: str, color: bool):
    """the three other strings of the mode (before / after / close for lines; before_number / after_number / after_match for -o)"""
    return (clm.strings(None, color) if mode == "lines" else omm.strings(None, color))[1:]


def definition(items, records, names, mode: str, color: bool = False, counts=None):
    """(a) -> (bytes, [(offset, nbytes)] per item).  records[i]: item i's own records, relative to its first byte, emission order"""
    out, where, at = [], [], 0
    for i, (it, rec, name) in enumerate(zip(items, records, names)):
        text = bm.as_array(it).tobytes()
        rec = [tuple(int(v) for v in r) for r in np.asarray(rec).reshape(-1, 2)]
        if mode == "count":
            piece = name + b":%d\n" % (len(rec) if counts is None else counts[i])
        elif not rec:
            piece = b""
        elif mode == "matches":
            piece = omm.grep_o_output(text, rec, name, color)
        elif color:
            piece = clm.color_output(text, rec, name, True)
        else:
            piece = lm.grep_output(text, rec, name + b":")
        out.append(piece)
        where.append((at, len(piece)))
        at += len(piece)
    return b"".join(out), where


def pack_records(items, records):
    """the items' own lists -> the pack-relative list in (start, end) order, as the formatters take it"""
    _, off = bm.pack(items)
    parts = [np.asarray(r, dtype=np.uint64).reshape(-1, 2) + off[i] for i, r in enumerate(records)]
    rec = np.concatenate(parts) if parts else bm.NONE
    order = np.lexsort((rec[:, 1], rec[:, 0])) if rec.size else np.zeros(0, dtype=np.int64)
    return rec[order].reshape(-1, 2)


def item_tables(pack: np.ndarray, off: np.ndarray, rec: np.ndarray):
    """per item, from the pack: the newlines in front of its first byte, the offset of its last newline (-1: none), its record range
    [lo, hi) and, under the stale rule (more than 10 records, a newline), what a record behind that newline prints (0: rule off)"""
    nl = np.flatnonzero(pack == 10).astype(np.int64)
    o = off.astype(np.int64)
    starts = rec[:, 0].astype(np.int64) if rec.size else np.zeros(0, dtype=np.int64)
    base = np.searchsorted(nl, o[:-1], "left")
    upto = np.searchsorted(nl, o[1:] - 1, "left")  # newlines in front of the item's end: the separator is not counted
    last_nl = np.where(upto > base, nl[np.maximum(upto, 1) - 1] if nl.size else -1, -1)
    lo, hi = np.searchsorted(starts, o[:-1], "left"), np.searchsorted(starts, o[1:], "left")
    true = 1 + np.searchsorted(nl, starts, "left")  # a start ON a newline belongs to the line that newline ends
    stale = np.zeros(len(o) - 1, dtype=np.int64)
    for i in np.flatnonzero((hi - lo > omm.STALE_AFTER) & (last_nl >= 0)):
        k = lo[i] + np.searchsorted(starts[lo[i]:hi[i]], last_nl[i], "right")  # records that start at or before the last newline
        stale[i] = true[k - 1] - base[i] if k > lo[i] else 1
    return base, last_nl, lo, hi, true, stale


def from_pack(items, rec: np.ndarray, names, mode: str, color: bool = False):
    """(b) -> (bytes, [(offset, nbytes)] per item, capped lines).  rec: pack-relative, (start, end) order"""
    pack, off = bm.pack(items)
    text = pack.tobytes()
    n_items = len(items)
    base, last_nl, lo, hi, true, stale = item_tables(pack, off, rec)
    recs = [(int(s), int(e)) for s, e in rec.reshape(-1, 2)]
    item_of = np.searchsorted(off.astype(np.int64), rec[:, 0].astype(np.int64), "right") - 1 if rec.size else np.zeros(0, dtype=np.int64)
    sizes = np.zeros(len(recs), dtype=np.int64)  # what every record adds
    out, capped = [], 0
    if mode == "matches":
        before, after, tail = strings(mode, color)
        for k, (s, e) in enumerate(recs):
            i = int(item_of[k])
            ln = int(true[k] - base[i])
            if stale[i] and s > last_nl[i]:
                ln = int(stale[i])
            piece = prefix(names[i], mode, color) + before + b"%d:" % ln + after + text[s:e].replace(b"\n", b" ") + tail + b"\n"
            out.append(piece)
            sizes[k] = len(piece)
    else:
        before, after, close = strings(mode, color)
        k = 0
        while k < len(recs):
            a, z = lm.line_of(text, recs[k][0])
            j = k
            while j < len(recs) and lm.line_of(text, recs[j][0])[0] == a:
                j += 1
            capped += j - k > lm.CAP
            piece, cur = [prefix(names[int(item_of[k])], mode, color)], a
            for s, e in recs[k:j][:lm.CAP]:
                e = min(e, z)
                if s >= e:
                    continue
                if s > cur:
                    piece.append(text[cur:s])
                piece += [before, text[s:e], after]
                cur = e
            if cur < z:
                piece.append(text[cur:z])
            piece += [close, b"\n"]
            out.append(b"".join(piece))
            sizes[k] = len(out[-1])  # (booked on the line's first record: an item's bytes begin at its first record)
            k = j
    ends = np.concatenate([[0], np.cumsum(sizes)])
    where = [(int(ends[lo[i]]), int(ends[hi[i]] - ends[lo[i]])) for i in range(n_items)]
    return b"".join(out), where, capped


# ---- the stock CLI, once per file, and the store of its answers -----------------------------------------------------------------
def cli_args(s: bm.Search, mode: str, color: bool):
    a = ["-t", "1", "--color=always" if color else "--color=never"]
    a += ["--no-simd"] if s.force_no_simd else []
    a += [] if s.kw.get("case_sensitive", True) else ["-i"]
    a += ["-w"] if s.kw.get("whole_word") else []
    a += {"lines": [], "matches": ["-o"], "count": ["-c"]}[mode] + (["-E"] if s.regex else [])
    if len(s.pats) == 1:
        return a + [s.pats[0]]
    for p in s.pats:
        a += ["-e", p]
    return a


def run_cli(cli, s: bm.Search, mode: str, color: bool, paths):
    """the CLI once per file (never -r: its walk order is not defined) -> the outputs concatenated, the paths left as they are"""
    import subprocess
    return b"".join(subprocess.run([cli] + cli_args(s, mode, color) + [str(p)], capture_output=True, timeout=120).stdout for p in paths)


digest = lm.digest


@contextlib.contextmanager
def _own_file():
    keep, lm.GOLDEN = lm.GOLDEN, GOLDEN
    try:
        yield
    finally:
        lm.GOLDEN = keep


class Store(lm.Store):
    """line_model.Store over tests/golden/batch_grep_output.json: digests of the stock CLI's answers for whole batches"""

    def __init__(self):
        with _own_file():
            super().__init__()

    def want(self, key, live=None) -> str:
        with _own_file():
            return super().want(key, live)

    def save(self):
        with _own_file():
            super().save()
