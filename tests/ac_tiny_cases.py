"""The case table of the tiny-dictionary kernel's instantiations (tests/test_gpu_ac_tiny_roads.py) and its CPU-side conditions
(tests/test_ac_tiny_cases_cpu.py).

TEST INFRASTRUCTURE.  ac_tiny_kernel<CI, LINES, KEEP, EMIT, LONG, FUSED, FIVE, DENSE> (krep_amd/csrc/kg_ac_tiny.hip) is dispatched in 23
instantiations: the staged road's {count, in-kernel -c, staged records, emit pass} x {-i, not} x {a long length, none} (ac_tiny_launch),
the one-pass item writer x {-i, not}, the one-pass dense writer x {-i, not} x {long, none} (ac_tiny_launch_fused) and the
case-sensitive count of a dictionary with a fifth class.  Which one a scan gets is decided by ac_scan (kg_ac.hip): the mode, the
text's size (the one-pass roads open at 64 units) and the density earlier scans of the plan counted.  Every case names its
instantiation as the part of Plan.ac_last_scan() it must produce — road, ci, lines, emit, stage_cap, upt, overflow_units, n_units —
and the answers are the compiled reference's aho_corasick_search on the same bytes.

The dictionaries are suffix chains (`j`, `zj`, `qzj`, `xqzj`): one planted word ends a match of every length on one byte, so the
order of a lane-cell's walk (END ascending, longest first) is in every record list.  Staged cases scan 2 units + 1 round + 37 bytes
(a unit seam, a round seam, a ragged last round, a tail shorter than a lane's 16 bytes), one-pass cases 64 units + 1 round + 5
bytes.  The background holds none of the patterns' letters: the plants are all the matches.  Sparse texts plant a word at byte 0,
on the last byte and across every kind of seam; dense texts a word every 397 bytes (odd: over a large text the ENDs take every
offset of a 1-KiB cell).  The seam sweep (sweep_texts) ends one match of each length 1, 2, 3, 4, 7 on every offset of the first
cell and on the 16 offsets either side of the cell, round and unit seams of a 2-unit text."""
from __future__ import annotations

import numpy as np

from krep_amd import abi

U, CELL, ROUND = 16384, 1024, 8192
N_STAGED = 2 * U + ROUND + 37   # 40 997
N_ONE_PASS = 64 * U + ROUND + 5  # the one-pass roads open at 64 units (ac_tiny_one_pass)
BASE = (5 << 32) + 3 * 4096      # the global base of the windowed scans
SLOT = 16                        # a fresh plan's staging slot
DENSE_RING = 6144                # 16-bit entries per wave of the dense writer (ac_tiny_dense_ring)
STEP = 397
REPORT_KEYS = ("road", "ci", "lines", "emit", "stage_cap", "upt", "overflow_units", "n_units")
assert N_STAGED == 40997 and N_STAGED % 16 and N_ONE_PASS % 16

W4, W7 = b"xqzj", b"wvyxqzj"
DICTS = {
    "none": ([b"j", b"zj", b"qzj", W4, b"k", b"vk"], W4),
    "long": ([b"j", b"zj", b"qzj", W7, b"k", b"vk"], W7),
    "five": ([b"if", b"else", b"while"], b"elsewhile"),
}
QUIET = b"jzqxkvwy"  # letters of the suffix-chain dictionaries: the background leaves them out


def background(seed, n, quiet=QUIET):
    alpha = bytes(c for c in bytes(range(97, 123)) + b"AEOT0123456789    ..--\n\n" if c not in quiet and c not in quiet.upper())
    rng = np.random.RandomState(seed)
    return np.frombuffer(alpha, dtype=np.uint8)[rng.randint(0, len(alpha), n)].copy()


def _place(t, end, word):
    """`word` with its last byte at end - 1 (cut off in front of byte 0)"""
    w = word[max(len(word) - end, 0):]
    t[end - len(w):end] = np.frombuffer(w, dtype=np.uint8)
    return end


def seam_ends(n, L):
    """ENDs (one past the last byte) of the sparse plants: the word at byte 0, across a cell, a round and every unit seam of a
    staged text (or the first, a middle and the last unit seam of a large one), into the ragged round, on the last byte"""
    units = n // U
    seams = [U * u for u in ((1, 2) if units <= 2 else (1, 2, 31, 32, units))]
    ends = [L, CELL + 2, ROUND + 1] + [s + 1 + (i % 3) for i, s in enumerate(seams)] + [U + ROUND + 2, units * U + ROUND + 1, n]
    return sorted(e for e in set(ends) if e == n or n - e >= L)  # (the plant on the last byte crosses the last seam itself, or stands behind it)


def sparse_text(seed, n, word, every=0):
    """-> (text, ENDs of the planted words, others: (END, matches, matches under -i) of a capital spelling per unit and of `vk`)"""
    t = background(seed, n)
    ends = seam_ends(n, len(word))
    if every:  # a large text: a word every `every` bytes as well, between the units that hold the seam plants
        ends = sorted(set(ends) | set(range(2 * U + 3000, n // U * U - 64, every)))
    for e in ends:
        _place(t, e, word)
    caps = [u * U + 5000 + 3 * u for u in range((n + U - 1) // U) if u * U + 5100 < n][:4]
    for e in caps:
        _place(t, e, word[-2:].upper())
    _place(t, U + 7001, b"vk")
    return t, ends, [(e, 0, 2) for e in caps] + [(U + 7001, 2, 2)]


def dense_text(seed, n, word):
    t = background(seed, n)
    seams = seam_ends(n, len(word))
    keep = sorted(seams + [e for e in range(STEP, n - 16, STEP) if all(abs(e - q) > len(word) + 1 for q in seams)])  # (no plant into a neighbour)
    for e in keep:
        _place(t, e, word)
    return t, keep, []


def windows(n, dense=False):
    """three ownership windows whose cuts fall inside a lane-cell; a dense one-pass case keeps every window dense (ac_tiny_one_pass
    leaves the dense writer behind a scan of fewer than 24 matches per unit)"""
    if dense:
        return [(0, 20 * U + 5), (20 * U + 5, 40 * U + ROUND + 9), (40 * U + ROUND + 9, n)]
    return [(0, 5), (5, U + 1), (U + 1, n)]


def dense_upt(per_unit):
    """tiny_dense_upt (kg_ac.hip)"""
    return min(4, int(DENSE_RING / (2.5 * per_unit)))


class Case:
    """key; pats / kw: the search; mode: count | lines | records; text (+ plants: ENDs of the words, caps: the other plants, sparse_text);
    first: the text a dense one-pass case scans first with records, for the plan to count its density; report: the part of
    Plan.ac_last_scan() the scan of `text` must give"""

    def __init__(self, key, dname, kw, mode, text, plants, caps, report, first=None, dense_windows=False):
        self.key, self.dname, self.kw, self.mode, self.text, self.plants, self.caps = key, dname, dict(kw), mode, text, plants, caps
        self.pats, self.word = DICTS[dname]
        self.report, self.first, self.dense_windows = report, first, dense_windows
        if mode == "lines":
            self.kw["count_lines"] = True

    @property
    def ci(self):
        return not self.kw.get("case_sensitive", True)

    def params(self, **over):
        return abi.Params(self.pats, **dict(self.kw, **over))

    def windows(self):
        return windows(self.text.size, self.dense_windows)

    def matches_per_unit(self):
        """from the plants alone: matches by the unit of their last byte (a word ends one match per pattern it has as a suffix)"""
        per = np.zeros((self.text.size + U - 1) // U, dtype=np.int64)
        k = sum(1 for p in self.pats if self.word.endswith(p))
        for e in self.plants:
            per[(e - 1) // U] += min(k, e) if self.dname != "five" else 0
        for e, cs, ci in self.caps:
            per[(e - 1) // U] += ci if self.ci else cs
        return per

    def __repr__(self):
        return self.key


def _report(road, case_kw, mode, n, **over):
    r = dict(road=road, ci=int(not case_kw.get("case_sensitive", True)), lines=int(mode == "lines"), emit=0, stage_cap=0, upt=1,
             overflow_units=0, n_units=(n + U - 1) // U)
    r.update(over)
    return r


_ALL = []


def all_cases():
    if _ALL:
        return _ALL
    out = []
    texts = {}
    for i, (dname, (pats, word)) in enumerate(DICTS.items()):
        texts[dname, "sparse"] = sparse_text(8100 + i, N_STAGED, word)
        texts[dname, "dense"] = dense_text(8200 + i, N_STAGED, word)
        texts[dname, "big-sparse"] = sparse_text(8300 + i, N_ONE_PASS, word, every=6007)
        texts[dname, "big-dense"] = dense_text(8400 + i, N_ONE_PASS, word)
    CI = (("", {}), ("-i", dict(case_sensitive=False)))
    # ---- the staged road: ac_tiny_kernel<CI, LINES, KEEP, EMIT, LONG>, 16 instantiations (the emit cases run the KEEP one first)
    for dname in ("none", "long"):
        for tag, kw in CI:
            t, P, C = texts[dname, "sparse"]
            out.append(Case(f"{dname}/count{tag}", dname, kw, "count", t, P, C, _report(4, kw, "count", t.size)))
            out.append(Case(f"{dname}/lines{tag}", dname, kw, "lines", t, P, C, _report(4, kw, "lines", t.size)))
            out.append(Case(f"{dname}/staged{tag}", dname, kw, "records", t, P, C, _report(4, kw, "records", t.size, stage_cap=SLOT)))
            t, P, C = texts[dname, "dense"]
            c = Case(f"{dname}/emit{tag}", dname, kw, "records", t, P, C, None)
            c.report = _report(4, kw, "records", t.size, stage_cap=SLOT, emit=2, overflow_units=int(np.count_nonzero(c.matches_per_unit() > SLOT)))
            out.append(c)
    # ---- one pass, items (road 2): <CI, ..., FUSED>, no long length
    for tag, kw in CI:
        t, P, C = texts["none", "big-sparse"]
        out.append(Case(f"none/items{tag}", "none", kw, "records", t, P, C, _report(2, kw, "records", t.size)))
    # ---- one pass, dense (road 3): <CI, ..., LONG, FUSED, false, DENSE>; the plan's first scan (staged, records) counts the density
    for dname in ("none", "long"):
        for tag, kw in CI:
            t, P, C = texts[dname, "big-dense"]
            first = texts[dname, "dense"]
            c = Case(f"{dname}/dense{tag}", dname, kw, "records", t, P, C, None, first=first, dense_windows=True)
            f = Case("first", dname, kw, "records", *first, None)
            c.report = _report(3, kw, "records", t.size, upt=dense_upt(f.matches_per_unit().sum() / len(f.matches_per_unit())))
            out.append(c)
    # ---- a fifth class (4-byte patterns beside a long length): the case-sensitive count, <.., FIVE>
    t, P, C = texts["five", "dense"]
    out.append(Case("five/count", "five", {}, "count", t, P, C, _report(4, {}, "count", t.size)))
    _ALL.extend(out)
    return _ALL


# ---- the seam sweep
SWEEP_N = 2 * U
SWEEP_DICTS = {  # lengths 1, 2, 3, 4, 7 (a fifth class: the count), and its halves with records
    "s5": [b"j", b"zj", b"\x00j", b"qzj", W4, W7],
    "s4": [b"j", b"zj", b"\x00j", b"qzj", W4],
    "s7": [b"j", b"zj", b"\x00j", b"qzj", W7],
}


def sweep_offsets():
    """the last bytes the sweep ends a match of every length on"""
    o = set(range(CELL + 16))
    for seam in (ROUND, U):
        o |= set(range(seam - 16, seam + 16))
    return sorted(o)


def sweep_texts():
    """eight texts of two units: text k ends W7 — and so one match of each length 1, 2, 3, 4, 7 — on the offsets == k mod 8, from text
    offset 0 on, where the word is cut off by the text's first byte (a pattern that would begin before byte 0 is no match, and
    `\\0j` is none in front of the `j` at byte 0: the padding in front of a text is not text).  -> [(text, last bytes)]"""
    out = []
    for k in range(8):
        t = np.full(SWEEP_N, ord("."), dtype=np.uint8)
        t[np.arange(37, SWEEP_N, 61)] = 10
        mine = [o for o in sweep_offsets() if o % 8 == k]
        for o in mine:
            if o >= 7:
                t[o - 7] = ord(".")
            _place(t, o + 1, W7)
        out.append((t, mine))
    return out


def reference(oracle, pats, kw, text, **over):
    """(returned count, records) of the compiled reference's aho_corasick_search"""
    return oracle.call(abi.RA_AHO_CORASICK, abi.Params(pats, **dict(kw, **over)), text)
