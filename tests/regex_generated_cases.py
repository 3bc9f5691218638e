"""Test helper: generated -E expressions with a text each, for the device line walks of kg_regex_loops.hip (the loops walk, the general
step with its jump pairs, the two passes over a line of more than 4096 bytes).  Seeded and deterministic: cases() is a pure function
of this module and of what the two host compilers say.
  groups, narrow: random_groups_case of test_regex_groups_model_cpu.py, unchanged (at most 12 positions);
  groups, wide:   2..5 quantified groups behind each other over the letters a..f: up to 32 positions and 12 jump pairs;
  groups, full:   the same, kept when it has 29..32 positions;
  loops:          random_case of test_regex_loops_model_cpu.py, and a wide variant of 3..6 branches (more than 24 places).
A case holds what Engine.regex_compile_groups / regex_compile_loops said of it (taken, or the reason of the refusal; an expression an
older compiler takes is drawn again) and a text of 10 to 11 KB: some 40 short lines over the expression's own letters and a blank, a
line of 4097 bytes and one of about 5000, with witnesses planted (strings a random walk over the model automaton accepts) and
near-misses (a witness without its last byte).

TEST INFRASTRUCTURE: imported by test_regex_generated_cases_cpu.py and test_gpu_regex_generated.py only."""
from __future__ import annotations

import numpy as np

import krep_amd
import regex_alt_model
import regex_groups_model as gm
import regex_long_lines_model as llm
import regex_loops_model as lm
import regex_ref
import test_regex_groups_model_cpu as tg
import test_regex_loops_model_cpu as tl
from krep_amd import abi
from krep_amd.engine import KrepGpuError

SEED_NARROW, SEED_WIDE, SEED_FULL, SEED_LOOPS, SEED_LOOPS_WIDE = 20261101, 3, 5, 20261103, 20261104
N_NARROW, N_WIDE, N_FULL, N_LOOPS, N_LOOPS_WIDE = 80, 190, 40, 60, 40  # cases that reach their compiler, refused ones included
LONG = 4096                                                        # a line of more bytes than this is a long line
WIDE_LETTERS = [b"a", b"b", b"c", b"d", b"e", b"f", b"[ab]", b"[c-e]", b"."]
REASONS = ("32 positions", "jump pairs", "fixed-length factors")   # what may refuse a generated groups expression
OLDER = "an older compiler takes"


def pairs_of(follow) -> int:
    """the jump pairs regex_groups_jumps() makes of a follow relation: the distinct non-empty remainders follow(i) - {i, i + 1}"""
    return len({frozenset(set(f) - {i, i + 1}) for i, f in enumerate(follow)} - {frozenset()})


class Case:
    """kind "groups" | "loops"; flavour "narrow" | "wide" | "full"; taken / reason: what the host compiler said; groups: n_pos, pairs, top (the
    highest position); loops: places, branches; text (read-only) and long_spans, the (start, end) of its lines of more than 4096 bytes"""

    def __init__(self, kind, flavour, pats, cs):
        self.kind, self.flavour, self.pats, self.cs = kind, flavour, pats, cs
        self.taken, self.reason = False, ""
        self.n_pos = self.pairs = self.top = self.places = self.branches = 0
        self.text, self.long_spans, self.letters = None, [], b""
        self.ref = {}  # ref_answer()'s results

    @property
    def anchored(self) -> bool:
        return self.pats[0].startswith(b"^") or self.pats[0].endswith(b"$")

    def label(self) -> str:
        """what every assertion message carries"""
        size = "%d pairs, %d positions" % (self.pairs, self.n_pos) if self.kind == "groups" else "%d places, %d branches" % (self.places, self.branches)
        return "%s %r%s (%s)" % (self.kind, regex_alt_model.joined(self.pats), "" if self.cs else " -i", size)

    def automaton(self) -> gm.Automaton:
        """the model's automaton: the position automaton of a groups expression, the places of a loops expression's sequences"""
        return gm.automaton(self.pats, self.cs) if self.kind == "groups" else automaton_of_loops(self.pats, self.cs)


def automaton_of_loops(pats, cs) -> gm.Automaton:
    """the sequences of places regex_loops_model expands an expression into, as an automaton: a place hands over to the next one of
    its sequence, a repeating place also to itself"""
    bol, eol, brs = lm.branches(pats, cs)
    au = gm.Automaton()
    au.bol, au.eol, au.tables = bol, eol, []
    for br in brs:
        base = len(au.tables)
        for k, (table, plus) in enumerate(br):
            au.tables.append(table)
            au.follow.append(({base + k} if plus else set()) | ({base + k + 1} if k + 1 < len(br) else set()))
        au.first.add(base)
        au.last.add(base + len(br) - 1)
    return au


# ------------------------------------------------------------------------------------------------------------ expressions
def wide_expr(rng, depth, budget):
    """random_expr of test_regex_groups_model_cpu.py over WIDE_LETTERS"""
    alts = []
    for _ in range(rng.randint(1, 3 if depth else 2)):
        items = []
        for _ in range(rng.randint(1, 4)):
            if budget[0] <= 0:
                break
            if depth and rng.randint(3) == 0:
                items.append(b"(" + wide_expr(rng, depth - 1, budget) + b")" + tg.pick(rng, tg.QUANTS))
            else:
                budget[0] -= 1
                items.append(tg.pick(rng, WIDE_LETTERS) + tg.pick(rng, tg.QUANTS[:7]))
        if not items:
            budget[0] -= 1
            items.append(tg.pick(rng, WIDE_LETTERS[:6]))
        alts.append(b"".join(items))
    return b"|".join(alts)


def wide_groups_case(rng, at_least=0):
    """2..5 groups behind each other, each with a quantifier of its own: what the model's parser admits with at most 32 positions
    (and `at_least` that many)"""
    while True:
        body = b"".join(b"(" + wide_expr(rng, 1, [6]) + b")" + tg.pick(rng, tg.QUANTS) for _ in range(rng.randint(2, 6)))
        pats = [(b"^" if rng.randint(6) == 0 else b"") + body + (b"$" if rng.randint(6) == 0 else b"")]
        cs = bool(rng.randint(4))
        try:
            au = gm.automaton(pats, cs)
        except gm.Refused:
            continue
        if at_least <= len(au.atoms) <= 32:
            return pats, cs


def wide_loops_case(rng):
    """3..6 branches of 3..7 items: what the loops model admits (at most 8 sequences, 32 places) with 5 sequences and 25 places or more"""
    while True:
        bol, eol = (b"^" if rng.randint(4) == 0 else b""), (b"$" if rng.randint(4) == 0 else b"")
        brs = []
        for _ in range(rng.randint(3, 7)):
            items = [tl.pick(rng, tl.ATOMS) + tl.pick(rng, tl.QUANTS) for _ in range(rng.randint(3, 8))]
            if rng.randint(3) == 0:
                items[rng.randint(len(items))] = b"(" + tl.random_seq(rng, 1, 2) + b"|" + tl.random_seq(rng, 1, 2) + b")"
            brs.append(bol + b"".join(items) + eol)
        k = rng.randint(1, len(brs) + 1)
        pats = [b"|".join(brs[:k])] + brs[k:]
        cs = bool(rng.randint(3))
        if not lm.accepted(pats, cs):
            continue
        seqs = lm.branches(pats, cs)[2]
        if len(seqs) >= 5 and sum(len(s) for s in seqs) > 24:
            return pats, cs


# ------------------------------------------------------------------------------------------------------------ texts
def letters_of(pats, cs) -> np.ndarray:
    """the letters the expression names (a range counts with what lies inside it), both cases under -i, and a blank"""
    s = set()
    for pat in pats:
        for i, c in enumerate(pat):
            if chr(c).isalpha():
                s.add(c)
                if pat[i + 1:i + 2] == b"-" and chr(pat[i + 2]).isalpha():
                    s.update(range(c, pat[i + 2] + 1))
    s = s or set(b"ab")
    if not cs:
        s |= set(bytes(s).swapcase())
    return np.frombuffer(bytes(sorted(s)) + b" ", dtype=np.uint8)


def witness(rng, au, letters, cap=16) -> bytes:
    """a string the automaton accepts: a random walk from `first` along `follow`, one byte of each position's class (of the letters
    where the class holds one, never a newline), ended in `last`; behind `cap` bytes the walk takes the shortest way there"""
    n = len(au.tables)
    dist = [0 if p in au.last else None for p in range(n)]
    grew = True
    while grew:
        grew = False
        for p in range(n):
            for q in au.follow[p]:
                if dist[q] is not None and (dist[p] is None or dist[p] > dist[q] + 1):
                    dist[p], grew = dist[q] + 1, True

    def byte_of(p):
        for pool in (letters, np.arange(33, 127), np.arange(1, 256)):
            ok = [int(b) for b in pool if au.tables[p][b] and b != 10]
            if ok:
                return ok[rng.randint(len(ok))]
        raise AssertionError("a position without a byte")

    p = tg.pick(rng, sorted(au.first))
    out = [byte_of(p)]
    while not (p in au.last and (len(out) >= cap or not au.follow[p] or rng.randint(3) == 0)):
        nxt = sorted(au.follow[p])
        p = min(nxt, key=lambda q: dist[q]) if len(out) >= cap else tg.pick(rng, nxt)
        out.append(byte_of(p))
    return bytes(out)


def case_text(rng, au, letters):
    """-> (text, [(start, end) of the long lines])"""
    bg = lambda n: bytes(letters[rng.randint(0, letters.size, size=n)])  # noqa: E731
    wit = lambda: witness(rng, au, letters)                              # noqa: E731

    def short_line(payload):
        room = max(0, 60 - len(payload))
        a = 0 if au.bol else rng.randint(0, room + 1)
        b = 0 if au.eol else rng.randint(0, room - a + 1)
        return bg(a) + payload + bg(b)

    def long_line(n, end_witness):
        buf = bytearray(bg(n))
        spots = sorted(rng.randint(100, n - 200, size=5).tolist())
        for k, at in enumerate(spots):  # three witnesses and two near-misses inside
            w = wit() if k % 2 == 0 else wit()[:-1]
            buf[at:at + len(w)] = w
        if au.bol:
            w = wit()
            buf[:len(w)] = w
        w = wit() if (end_witness or au.eol) else wit()[:-1]
        buf[n - len(w):] = w
        return bytes(buf[:n])

    short = [bg(rng.randint(0, 61)) for _ in range(40)]
    for k, at in enumerate(rng.permutation(40)[:7].tolist()):  # four witness lines, three near-misses
        short[at] = short_line(wit() if k < 4 else wit()[:-1])
    longs = [long_line(LONG + 1, bool(rng.randint(2))), long_line(int(rng.randint(4800, 5300)), True)]
    if rng.randint(2):
        longs.reverse()
    where = rng.randint(3)  # a long line first in the text, last in it, or neither
    at = sorted(rng.randint(1, 40, size=2).tolist())
    if where == 0:
        at[0] = 0
    elif where == 1:
        at[1] = 40
    lines = short[:at[0]] + [longs[0]] + short[at[0]:at[1]] + [longs[1]] + short[at[1]:]
    text = np.frombuffer(b"\n".join(lines) + (b"\n" if rng.randint(2) else b""), dtype=np.uint8).copy()
    text.setflags(write=False)
    spans = [(a, b) for a, b in lm.line_spans(text) if b - a > LONG]
    assert len(spans) == 2
    return text, spans


# ------------------------------------------------------------------------------------------------------------ the case list
_cases = {}


def _rx(pats, cs):
    return abi.Params(list(pats), regex=True, case_sensitive=cs)


def _draw(eng, kind, flavour, draw, seed, n):
    """n cases that reach their compiler; -> (cases, expressions an older compiler took and that were drawn again)"""
    rng = np.random.RandomState(seed)
    out, older = [], 0
    while len(out) < n:
        drawn = draw(rng)
        c = Case(kind, flavour, drawn[0], drawn[-1]["case_sensitive"] if kind == "loops" and flavour == "narrow" else drawn[1])
        try:
            if kind == "groups":
                g = eng.regex_compile_groups(_rx(c.pats, c.cs))
                c.n_pos, c.pairs = g["n_pos"], pairs_of(g["follow"])
                c.top = max(set().union(g["first"], g["last"], *g["follow"]))
            else:
                info = eng.regex_compile_loops(_rx(c.pats, c.cs))
                c.branches = int(info.alt.n_branches)
                c.places = sum(int(info.alt.branch[i].L) for i in range(c.branches))
            c.taken = True
        except KrepGpuError as e:
            if kind == "groups" and OLDER in str(e):
                older += 1
                continue
            c.reason = str(e)
        c.letters = letters_of(c.pats, c.cs)
        if c.taken:
            c.text, c.long_spans = case_text(rng, c.automaton(), c.letters)
        out.append(c)
    return out, older


def cases():
    """-> {"groups": [Case], "loops": [Case], "older": expressions drawn again}; in the C locale (regex_ref.c_locale) and built once"""
    if "groups" not in _cases:
        with regex_ref.c_locale():
            eng = krep_amd.load()
            gn, o1 = _draw(eng, "groups", "narrow", tg.random_groups_case, SEED_NARROW, N_NARROW)
            gw, o2 = _draw(eng, "groups", "wide", wide_groups_case, SEED_WIDE, N_WIDE)
            gf, o3 = _draw(eng, "groups", "full", lambda rng: wide_groups_case(rng, 29), SEED_FULL, N_FULL)
            ln, _ = _draw(eng, "loops", "narrow", tl.random_case, SEED_LOOPS, N_LOOPS)
            lw, _ = _draw(eng, "loops", "wide", wide_loops_case, SEED_LOOPS_WIDE, N_LOOPS_WIDE)
        _cases.update(groups=gn + gw + gf, loops=ln + lw, older=o1 + o2 + o3)
    return _cases


def taken(kind):
    return [c for c in cases()[kind] if c.taken]


CHUNK = 25
DRAWN = {"groups": N_NARROW + N_WIDE + N_FULL, "loops": N_LOOPS + N_LOOPS_WIDE}  # known without drawing: what a test is parametrized by


def n_chunks(kind) -> int:
    return (DRAWN[kind] + CHUNK - 1) // CHUNK


def chunk(kind, k):
    """the taken cases among the drawn cases [k * CHUNK, (k + 1) * CHUNK) of a kind"""
    return [c for c in cases()[kind][k * CHUNK:(k + 1) * CHUNK] if c.taken]


def seam_case() -> Case:
    """A hand-made loops case no random walk plants: under ^ and $, long lines that are a match of one sequence with a match of the
    next sequence behind it (and the other way round).  No such line holds a match; a reverse step of the shift that leaves its
    sequence (the last place of one in front of the first place of the next) finds one under -c."""
    if "seam" not in _cases:
        c = Case("loops", "seam", [b"^a+b$|^c+d$", b"^e+f$"], True)
        info = krep_amd.load().regex_compile_loops(_rx(c.pats, c.cs))
        c.taken, c.branches = True, int(info.alt.n_branches)
        c.places = sum(int(info.alt.branch[i].L) for i in range(c.branches))
        lines = [b"ab", b"abcd", b"a" * 3000 + b"b" + b"c" * 2000 + b"d", b"a" * 4999 + b"b", b"cd", b"c" * 2500 + b"d" + b"a" * 2500 + b"b",
                 b"c" * 4095 + b"d" + b"e" * 3 + b"f", b"ccdab", b"c" * 4096 + b"d", b"ef", b"e" * 4200 + b"f", b"a" * 2100 + b"b" + b"e" * 2100 + b"f"]
        c.text = np.frombuffer(b"\n".join(lines), dtype=np.uint8).copy()
        c.text.setflags(write=False)
        c.long_spans = [(a, b) for a, b in lm.line_spans(c.text) if b - a > LONG]
        c.letters = letters_of(c.pats, c.cs)
        _cases["seam"] = c
    return _cases["seam"]


# ------------------------------------------------------------------------------------------------------------ the model
def model_answer(c: Case):
    """-> (records[(n, 2) uint64], -c count): the brute-force matcher of the case's own model (regex_groups_model / regex_loops_model)
    on the short lines, the two passes of regex_long_lines_model on the long ones.  Lines are independent, so each model reads the
    text with the other's lines turned into empty ones."""
    au = c.automaton()
    only_short, only_long = c.text.copy(), np.full(c.text.size, 10, dtype=np.uint8)
    for a, b in c.long_spans:
        only_short[a:b] = 10
        only_long[a:b] = c.text[a:b]
    # (an open last line stays the open last line of the copy that keeps it; in the other copy it ends on a newline, and is empty)
    if c.kind == "groups":
        per_short = gm.matches(au, only_short, c.cs)
    else:
        per_short = lm.matches(lm.branches(c.pats, c.cs), only_short, c.cs)
    per_long = llm.matches(au, only_long, c.cs)
    rec = sorted(m for line in per_short + per_long for m in line)
    lines = sum(1 for line in per_short if line) + llm.line_counts(au, only_long, c.cs)
    assert lines == sum(1 for line in per_short + per_long if line), c.label()
    return np.asarray(rec, dtype=np.uint64).reshape(-1, 2), lines


def ref_answer(c: Case, **kw):
    """regex_search of the compiled reference over the case's text, with the case's own case_sensitive (asked once per mode)"""
    key = tuple(sorted(kw.items()))
    if key not in c.ref:
        c.ref[key] = regex_ref.call(regex_alt_model.joined(c.pats), c.text, case_sensitive=c.cs, **kw)
    return c.ref[key]


def in_long_lines(c: Case, records) -> np.ndarray:
    """per record: it starts inside a long line"""
    starts = records[:, 0].astype(np.int64)
    inside = np.zeros(starts.size, dtype=bool)
    for a, b in c.long_spans:
        inside |= (starts >= a) & (starts < b)
    return inside


def first_difference(got, want) -> str:
    """the first record two record arrays differ in, for an assertion message"""
    n = min(len(got), len(want))
    d = np.flatnonzero((np.asarray(got[:n]) != np.asarray(want[:n])).any(axis=1)) if n else np.zeros(0, dtype=int)
    k = int(d[0]) if d.size else n
    return "%d records, want %d; first difference at #%d: got %s, want %s" % (
        len(got), len(want), k, got[k].tolist() if k < len(got) else None, want[k].tolist() if k < len(want) else None)
