"""Test helper: which 1-KiB cells the anchor path of the regex scan (krep_amd/csrc/kg_regex.hip) skips, which occurrences are
reported right only if the entry state rebuilt behind skipped cells is right, and the builder of the texts that hold such
occurrences at every split (tests/test_gpu_regex.py runs them, tests/test_regex_skip_model_cpu.py pins what they hold).

TEST INFRASTRUCTURE: plain numpy, no GPU.  The geometry: the grid starts at own_lo & ~15; a wave unit is 32 cells,
a round 8 cells.  The anchor is the FIRST smallest class of the pattern (kg_regex_compile.h), its bytes count only when it holds
1..4 of them.  A cell is skipped when neither it nor the cell in front of it holds an anchor byte; the first cell of a unit is
never skipped (its entry state is read from the text).  An occurrence is DEPENDENT when it ends in the first L - 1 bytes of a
walked cell that is not the first of its unit, and the cell in front of that one was skipped: the part of it in front of the cell
is known to the kernel only through the state it rebuilds from the last 16 bytes of the skipped cell."""
from __future__ import annotations

import collections
import itertools

import numpy as np

import regex_model

CELL, ROUND, UNIT = 1024, 8192, 32768
CELLS_PER_ROUND, CELLS_PER_UNIT = ROUND // CELL, UNIT // CELL
FAULTS = ("zero", "ones", "stale", "lane62")


def anchor(cl):
    """-> (index of the anchor class, its bytes: empty when the class holds 0 or more than 4)"""
    sizes = [int(t.sum()) for t in cl]
    ai = sizes.index(min(sizes))
    return ai, (np.flatnonzero(cl[ai]).astype(np.uint8) if 1 <= sizes[ai] <= 4 else np.zeros(0, dtype=np.uint8))


def _fits(cl, text, at):
    """text[at : at + len(cl)] lies in the classes cl, one byte each"""
    return at >= 0 and at + len(cl) <= text.size and all(t[text[at + i]] for i, t in enumerate(cl))


class Geometry:
    """the cells of one scan of text with starts owned in [own_lo, own_hi)"""

    def __init__(self, cl, text, own_lo=0, own_hi=None):
        self.cl, self.text, self.L, n = cl, text, len(cl), text.size
        own_hi = n if own_hi is None else min(own_hi, n)
        self.own_lo = own_lo
        self.hi_match = max(min(own_hi, n - self.L + 1), own_lo)
        self.origin = own_lo & ~15
        self.cov_hi = self.hi_match + self.L - 1
        self.n_cells = max(0, -(-(self.cov_hi - self.origin) // CELL))
        self.anchor_index, ab = anchor(cl)
        # a cell is loaded whole (bytes past the text read as 0, never an anchor byte: a pattern holds bytes 0x01-0x7F)
        has = np.zeros(self.n_cells * CELL, dtype=bool)
        body = text[self.origin:self.origin + has.size]
        has[:body.size] = np.isin(body, ab)
        self.anch = has.reshape(self.n_cells, CELL).any(axis=1)
        first = np.arange(self.n_cells) % CELLS_PER_UNIT == 0
        self.skipped = ~first & ~self.anch & ~np.concatenate(([True], self.anch[:-1])) if ab.size else np.zeros(self.n_cells, dtype=bool)
        occ = regex_model.occurrences(cl, text)
        self.occ = occ[(occ >= own_lo) & (occ < self.hi_match)]
        assert not self.skipped[(self.occ + self.L - 1 - self.origin) // CELL].any(), "an occurrence ends in a skipped cell"

    def base(self, c):
        return self.origin + c * CELL

    def rebuilt(self):
        """the cells whose entry state is rebuilt: walked, not the first of a unit, behind a skipped cell"""
        c = np.arange(1, self.n_cells)
        return c[(c % CELLS_PER_UNIT != 0) & ~self.skipped[1:] & self.skipped[:-1]]

    def dependent(self):
        """-> [(start, cell, k)] of the dependent occurrences; k: how many of their bytes lie in front of the cell"""
        reb = set(self.rebuilt().tolist())
        out = []
        for s in self.occ.tolist():
            c, at = divmod(s + self.L - 1 - self.origin, CELL)
            if at < self.L - 1 and c in reb:
                out.append((s, c, self.base(c) - s))
        return out

    def decoys(self):
        """-> (suffix, prefix): the splits k <= anchor index for which a cell with a rebuilt entry state starts with the last
        L - k bytes of a match that is none / for which, moreover, the last walked cell in front of it ends with the first k"""
        suffix, prefix = set(), set()
        for c in self.rebuilt().tolist():
            cb = self.base(c)
            w = max(i for i in range(c) if not self.skipped[i])
            for k in range(1, self.anchor_index + 1):
                if _fits(self.cl[k:], self.text, cb) and not _fits(self.cl, self.text, cb - k):
                    suffix.add(k)
                    if _fits(self.cl[:k], self.text, self.base(w + 1) - k):
                        prefix.add(k)
        return suffix, prefix

    def kernel_hits(self, fault=None):
        """the starts the scan reports when the rebuilt state is right (None: the owned occurrences) or wrong in one of FAULTS:
        replaced by 0, by 0xFFFF, left at the exit of the last walked cell, taken from lane 62's bytes instead of lane 63's"""
        hits = {s for s in self.occ.tolist()} - {s for s, _, _ in self.dependent()}
        for c in self.rebuilt().tolist():
            cb = self.base(c)
            src = {None: cb, "lane62": cb - 16, "stale": self.base(max(i for i in range(c) if not self.skipped[i]) + 1)}.get(fault)
            for k in range(1, self.L):  # a match with k bytes in front of the cell
                s = cb - k
                if not (self.own_lo <= s < self.hi_match and _fits(self.cl[k:], self.text, cb)):
                    continue
                if fault == "ones" or (fault != "zero" and _fits(self.cl[:k], self.text, src - k)):
                    hits.add(s)
        return np.asarray(sorted(hits), dtype=np.int64)


# ---------------------------------------------------------------------------------------------------- the texts of the GPU tests
# (pattern, case_sensitive): n_anchor 1, 2 and 4, L = 2, 5, 8 and 16, the anchor in the middle and at the end
PATTERNS = [(b"[0-9]{3}-[0-9]{4}", True), (b"[a-f]{7}S", True), (b"[0-9]{4}k", False), (b"[a-f]{15}[#%&@]", True),
            (b"[a-f]{8}Q[a-f]{7}", True), (b"[a-f]Z", True)]
TEXT_LEN = 3 * UNIT + ROUND + 300

Plant = collections.namedtuple("Plant", "kind k cell start")  # kind: straddler / unit / decoy / edge; start of the (would-be) match


def background_alphabet(cl):
    """g-z, space and newline without every byte of a class of the pattern (the anchor bytes among them)"""
    return bytes(b for b in b"ghijklmnopqrstuvwxyz \n" if not any(t[b] for t in cl))


def build_text(cl, n=TEXT_LEN, seed=0, omit=()):
    """-> (text, [Plant]).  One plant per cell boundary, each boundary with two anchor-free cells in front of it:
      straddler  a match with k bytes in front of the boundary, k = 1 .. L - 1 (dependent for k <= anchor index);
      unit       a straddler at a unit boundary (not dependent: there the state is read from the text);
      decoy      k <= anchor index: the last L - k bytes of a match behind the boundary with background in front of them (a state of
                 0xFFFF reports it), the first k bytes at the end of the last walked cell in front of the skipped run, which is the
                 anchor-free cell behind a cell with a lone anchor byte (a stale state reports it);
      edge       a match at byte 0 and one that ends on the last byte.
    Once every split has its straddler and its decoy the remaining boundaries take further ones in turn; an admissible round boundary
    inside a unit and the last boundary of the text always take a dependent straddler.  omit: kinds left out, and "prefixes" for
    decoys without their first k bytes (what tests/test_regex_skip_model_cpu.py uses to show that its conditions can fail)."""
    L, (ai, ab) = len(cl), anchor(cl)
    assert ab.size and ai >= 1, "the pattern has no anchor behind its first class"
    rng = np.random.RandomState(seed)
    al = np.frombuffer(background_alphabet(cl), dtype=np.uint8)
    text = al[rng.randint(0, al.size, size=n)].copy()
    others = [np.setdiff1d(np.flatnonzero(t), ab).astype(np.uint8) for t in cl]
    made = itertools.count()

    def match():
        i = next(made)  # every anchor byte takes its turn
        return np.array([ab[i % ab.size] if j == ai else others[j][rng.randint(others[j].size)] for j in range(L)], dtype=np.uint8)

    plants = []

    def put(kind, k, c):
        m, cb = match(), c * CELL
        if kind in omit:
            return
        if kind == "decoy":
            text[(c - 3) * CELL + CELL // 2] = ab[0]
            if "prefixes" not in omit:
                text[cb - CELL - k:cb - CELL] = m[:k]
            text[cb:cb + L - k] = m[k:]
        else:
            text[cb - k:cb - k + L] = m
        plants.append(Plant(kind, k, c, cb - k))

    last = (n - 2 * L) // CELL  # the last boundary with room for a match behind it and the edge plant
    needed = collections.deque([("straddler", k) for k in range(1, L)] + [("decoy", k) for k in range(1, ai + 1)])
    more = itertools.cycle([(kind, k) for k in range(1, ai + 1) for kind in ("straddler", "decoy")])
    more_dependent = itertools.cycle(range(1, ai + 1))
    unit_k = itertools.cycle(sorted({1, L - 1, max(1, L // 2)}))
    a_last = 0  # the last cell that may hold an anchor byte (cell 0: the edge plant)
    for c in range(1, last + 1):
        at = c % CELLS_PER_UNIT
        if at == 0:
            if c >= a_last + 2:
                put("unit", next(unit_k), c)
                a_last = c
            continue
        # a dependent plant: two anchor-free cells in front, the cell in front not the first of a unit, room for the unit and last plants
        if at in (1, CELLS_PER_UNIT - 1) or c < a_last + 3 or last - 3 < c < last:
            continue
        if c == last or at % CELLS_PER_ROUND == 0:
            first = next((p for p in needed if p[0] == "straddler" and p[1] <= ai), None)
            if first:
                needed.remove(first)
            kind, k = first or (needed.popleft() if needed and c != last else ("straddler", next(more_dependent)))
        else:
            kind, k = needed.popleft() if needed else next(more)
        put(kind, k, c)
        a_last = c
    assert not needed, ("the text is too short for its plants", list(needed))
    if "edge" not in omit:
        text[:L] = match()
        text[n - L:] = match()
        plants += [Plant("edge", 0, 0, 0), Plant("edge", 0, (n - L) // CELL, n - L)]
    return text, plants


def missing(cl, text):
    """what a text of build_text() must hold and does not (origin 0, the whole text owned): a list of plain words, empty when all is there"""
    g, L, n = Geometry(cl, text), len(cl), text.size
    ai, out = g.anchor_index, []
    dep = g.dependent()
    occ = set(g.occ.tolist())
    for k in range(1, L):
        if not any((c * CELL - k) in occ for c in range(1, g.n_cells)):
            out.append(f"straddler k={k}")
    for k in range(1, ai + 1):
        if not any(dk == k for _, _, dk in dep):
            out.append(f"dependent k={k}")
    if not any(c % CELLS_PER_ROUND == 0 for _, c, _ in dep):
        out.append("dependent at a round boundary inside a unit")
    if not any(g.base(c - c % CELLS_PER_ROUND) + ROUND > n for _, c, _ in dep):
        out.append("dependent in the guarded last round")
    dep_starts = {s for s, _, _ in dep}
    if not any(s < u <= s + L - 1 and s not in dep_starts for u in range(UNIT, n, UNIT) for s in range(u - L + 1, u) if s in occ):
        out.append("straddler at a unit boundary")
    suffix, prefix = g.decoys()
    out += [f"suffix decoy k={k}" for k in range(1, ai + 1) if k not in suffix]
    out += [f"prefix decoy k={k}" for k in range(1, ai + 1) if k not in prefix]
    out += [w for w, s in (("match at byte 0", 0), ("match on the last byte", n - L)) if s not in occ]
    return out
