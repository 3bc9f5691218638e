"""The case table of the general multi-pattern kernel's instantiations (tests/test_gpu_ac_roads.py) and its CPU-side conditions
(tests/test_ac_road_cases_cpu.py).

TEST INFRASTRUCTURE.  ac_scan_kernel<CI, LINES, SHORT, STRIDE, ANCH, WW> (krep_amd/csrc/kg_ac.hip) exists in 16 base instantiations;
which one a dictionary gets is decided by filter_tables() (the stride, from the popcounts of two class tables), ac_launch2() (SHORT,
from the 1..3-byte patterns) and the modes -i / -c; how its matches reach the record list by ac_staged() / ac_learn() / ac_emit()
(the staging slot of 16 or 64 matches per 16-KiB unit, the ticket size, the emit pass over the redo list or over every unit).  Every
case here names the instantiation and the staging road it is there for as the report Plan.ac_last_scan() must give, and the answers
are the compiled reference's aho_corasick_search on the same bytes.

Texts are 5 or 10 units of 16 KiB plus an odd tail.  A dictionary's text is a random background with chance hits and near misses
(the filter sees classes, byte & 31: digits and punctuation share them with letters) and PLANTS, each between dots that no pattern
holds: at byte 0, on the last byte, across a 1-KiB cell cut, an 8-KiB round cut and the 16-KiB unit cuts (at the splits of a
pattern's bytes, each alone on its line: the split that leaves only the last byte behind the cut is the stride-2 -c kernel's extra
candidate), at even and odd offsets, two patterns that end on one byte, a pattern the dictionary holds twice, two matches on one
line on either side of a unit cut, and other spellings for -i.  The staging texts have a quiet background (no letter) and units
with exactly 16 / 17 and 64 / 65 matches; the sweep texts end a match on every offset of a 1-KiB cell (every lane and bit of the
filter's result) in two units dense enough for the emit pass."""
from __future__ import annotations

import numpy as np

from krep_amd import abi

U, CELL, ROUND = 16384, 1024, 8192
N5, N10 = 5 * U + 11, 10 * U + 13
BASE = (5 << 32) + 3 * 4096  # the global base of the windowed scans
AZ = bytes(range(97, 123))
MODES = (("plain", {}), ("i", dict(case_sensitive=False)), ("c", dict(count_lines=True)), ("ic", dict(case_sensitive=False, count_lines=True)))
assert N5 % 16 and N10 % 16


def windows(n):
    """three ownership windows: cuts at 5 and one byte behind the first unit cut"""
    return [(0, 5), (5, U + 1), (U + 1, n)]


def _rand_words(rng, k, m, alpha, taken=()):
    out, seen = [], set(taken)
    while len(out) < k:
        w = bytes(alpha[i] for i in rng.randint(0, len(alpha), m))
        if w not in seen:
            seen.add(w)
            out.append(w)
    return out


class Dict:
    """pats: the dictionary as given to the search (duplicates included); main: the pattern of the positional plants; splits: (pattern,
    bytes in front of the unit cut) of the plants across the unit cuts; also: further patterns planted
    at an even and an odd offset; nested: a pattern and its suffix, both in the dictionary; twice: a pattern the dictionary holds two
    times; quiet: letters the background leaves out (every short pattern holds one of them: the plants are their only occurrences)"""

    def __init__(self, name, pats, main, splits, also, nested, twice, n, stride, quiet=b""):
        self.name, self.pats, self.main, self.splits, self.also, self.nested, self.twice = name, pats, main, splits, also, nested, twice
        self.n, self.stride, self.quiet = n, stride, quiet
        lens = {len(p) for p in pats}
        self.short_lens = sum(1 << (k - 1) for k in (1, 2, 3) if k in lens)
        assert main in pats and nested[0] in pats and nested[1] in pats and nested[0].endswith(nested[1]) and pats.count(twice) == 2
        assert all(p in pats for p, _ in splits) and all(p in pats for p in also) and not any(b"\n" in p or b"." in p for p in pats)


def _dictionaries():
    rng = np.random.RandomState(20261020)
    four = _rand_words(rng, 140, 4, AZ)
    long130 = [b"kelvinator", b"vinator", b"mudlark", b"hedgerowsfar", b"plumb"]
    d = {}
    d["four130"] = Dict("four130", four + long130 + [b"mudlark"], four[0], [(four[0], k) for k in (1, 2, 3)], [four[1], b"hedgerowsfar"],
                        (b"kelvinator", b"vinator"), b"mudlark", N10, 1)
    few4 = _rand_words(rng, 6, 4, AZ, four)
    few = few4 + [b"tangle", b"entangle", b"brackish", b"hollowway", b"cinderpath", b"lamplighter", b"fernseedloft", b"ospreys", b"quill",
                  b"wharf", b"juniper", b"saltmarsh", b"gorse", b"bramblings"]
    d["four_few"] = Dict("four_few", few + [b"ospreys"], few4[0], [(few4[0], k) for k in (1, 2, 3)], [few4[1], b"fernseedloft"], (b"entangle", b"tangle"),
                         b"ospreys", N5, 2)
    three = [b"qzx", b"jqv", b"wqk"]
    d["three_short"] = Dict("three_short", three + [b"hammock", b"glenfiddle", b"lifeboatwqk", b"paddock", b"moleacbank", b"paddock"], b"qzx",
                            [(b"qzx", 1), (b"qzx", 2), (b"hammock", 1), (b"hammock", 3), (b"hammock", 6)], [b"jqv", b"glenfiddle"],
                            (b"lifeboatwqk", b"wqk"), b"paddock", N10, 2, b"q")
    d["two_short"] = Dict("two_short", [b"zq", b"qzx", b"mildewcap", b"flangeblock", b"inkdomeflagon", b"domeflagon", b"haddockboil", b"mildewcap"],
                          b"zq", [(b"zq", 1), (b"qzx", 1), (b"qzx", 2), (b"mildewcap", 1), (b"mildewcap", 4), (b"mildewcap", 8)],
                          [b"qzx", b"flangeblock"], (b"inkdomeflagon", b"domeflagon"), b"mildewcap", N10, 1, b"q")
    one = [b"q", b"mildewcap", b"flangeblock", b"inkdomeflagon", b"domeflagon", b"haddockboil", b"flangeblock"]
    d["one_short"] = Dict("one_short", one, b"mildewcap", [(b"mildewcap", k) for k in range(1, 9)], [b"q", b"haddockboil"],
                          (b"inkdomeflagon", b"domeflagon"), b"flangeblock", N10, 1, b"q")
    # ... and with the short pattern itself held twice: the bitmaps of the short patterns cannot count copies (F_AC_SHORT_DUP)
    d["one_short_dup"] = Dict("one_short_dup", one[:-1] + [b"q"], b"mildewcap", d["one_short"].splits, [b"q", b"haddockboil"],
                              (b"inkdomeflagon", b"domeflagon"), b"q", N10, 1, b"q")
    assert all(len(p) >= 9 or b"q" in p for k in ("two_short", "one_short", "one_short_dup") for p in d[k].pats)
    return d


class Plant:
    """one planted occurrence: [start, start + len(body)) holds `body`, which is the pattern `pat` spelled some way.  ci_only: another
    spelling, found under -i alone; word: a whole word (found under -w); alone: the only match on its line"""

    def __init__(self, name, pat, start, body=None, word=True, alone=False):
        self.name, self.pat, self.start, self.body = name, pat, start, pat if body is None else body
        self.ci_only, self.word, self.alone = self.body != pat, word, alone

    @property
    def end(self):
        return self.start + len(self.pat)

    def __repr__(self):
        return f"{self.name}@{self.start}"


def _put(t, pl, lead=b"......", trail=b"......"):
    lo = max(pl.start - len(lead), 0)
    lead = lead[len(lead) - (pl.start - lo):]
    hi = min(pl.end + len(trail), t.size)
    a = np.frombuffer(lead + pl.body + trail[: hi - pl.end], dtype=np.uint8)
    t[lo:hi] = a
    return pl


def background(seed, n, quiet=b""):
    """random letters (without `quiet`), a few capitals, digits, blanks, dots and newlines: chance hits and near misses"""
    alpha = bytes(c for c in AZ + b"AEIOT" + b"0123456789" + b"    ..--\n\n" if c not in quiet and c not in quiet.upper())
    rng = np.random.RandomState(seed)
    return np.frombuffer(alpha, dtype=np.uint8)[rng.randint(0, len(alpha), n)].copy()


def dictionary_text(d: Dict, seed, sprinkle=0):
    """-> (text, plants).  The unit cuts 1, 2, ... take d.splits in turn, the cut behind them the two matches on one line."""
    n = d.n
    t = background(seed, n, d.quiet)
    P, m = [], d.main
    L = len(m)
    P.append(_put(t, Plant("byte0", m, 0)))
    P.append(_put(t, Plant("last", m, n - L)))
    P.append(_put(t, Plant("cell", m, U + 3 * CELL - L // 2)))
    P.append(_put(t, Plant("round", m, 2 * U + ROUND - (L + 1) // 2)))
    P.append(_put(t, Plant("even", m, 3 * U + 5000)))
    P.append(_put(t, Plant("odd", m, 3 * U + 5101)))
    for j, q in enumerate(d.also):
        P.append(_put(t, Plant(f"even{j}", q, 3 * U + 6000 + 200 * j)))
        P.append(_put(t, Plant(f"odd{j}", q, 3 * U + 7001 + 200 * j)))
    long, suffix = d.nested
    P.append(_put(t, Plant("nested", long, 4 * U + 3000)))
    P.append(Plant("nested-suffix", suffix, 4 * U + 3000 + len(long) - len(suffix), word=False))
    P.append(_put(t, Plant("twice", d.twice, 9000)))
    P.append(_put(t, Plant("capitals", m, U + 9000, m.upper())))
    P.append(_put(t, Plant("mixed", long, 2 * U + 3000, long[:3] + long[3:].upper())))
    cut = 0
    for q, k in d.splits:
        cut += U
        P.append(_put(t, Plant(f"unit{cut // U}/{k}", q, cut - k, alone=True), b"\n......", b"......\n"))
    cut += U
    assert cut + U <= n, (d.name, "no unit cut left for the two matches on one line")
    P.append(_put(t, Plant("line-left", m, cut - 3 - L), b"\n....", b"..."))
    P.append(_put(t, Plant("line-right", m, cut + 3), b"...", b"....\n"))
    assert b"\n" not in t[cut - 3 - L:cut + 3 + L].tobytes()
    if sprinkle:  # a few more per unit (max_count = 77 needs a longer list)
        rng = np.random.RandomState(seed + 1)
        for u in range(n // U):
            for j in range(sprinkle):
                P.append(_put(t, Plant(f"more{u}/{j}", d.pats[rng.randint(0, len(d.pats))], u * U + 11000 + 300 * j)))
    # the first line holds the plant at byte 0, the last line the plant on the last byte
    return t, P


def staging_text(d: Dict, counts: dict, seed):
    """a quiet text of N10 bytes (no letter: the plants are all its matches): unit u holds counts[u] occurrences of d.main in its
    middle, 40 bytes apart; one more at byte 0 and one on the last byte"""
    rng = np.random.RandomState(seed)
    alpha = np.frombuffer(b"0123456789  ..,-:;\n", dtype=np.uint8)
    t = alpha[rng.randint(0, len(alpha), N10)].copy()
    m = d.main
    P = [_put(t, Plant("byte0", m, 0)), _put(t, Plant("last", m, N10 - len(m)))]
    for u, k in counts.items():
        assert 0 < u < N10 // U and 2000 + 40 * k < U - 2000
        for j in range(k):
            P.append(_put(t, Plant(f"u{u}/{j}", m, u * U + 2000 + 40 * j + (j & 1))))  # (even and odd offsets)
    return t, P


def sweep_text(d: Dict, seed):
    """a quiet text of N10 bytes with 1024 occurrences of d.main, 17 bytes apart from the second unit on: 17 is odd, so their last bytes
    take every offset of a 1-KiB cell once — every lane of the filter and every bit of its result, in both table layouts.  Every eighth
    gap holds a newline.  The two units they fill overflow any slot: their records come from the emit pass."""
    rng = np.random.RandomState(seed)
    alpha = np.frombuffer(b"0123456789  ..,-:;", dtype=np.uint8)
    t = alpha[rng.randint(0, len(alpha), N10)].copy()
    m = d.main
    assert len(m) + 6 <= 16
    P = [_put(t, Plant("byte0", m, 0)), _put(t, Plant("last", m, N10 - len(m)))]
    for i in range(CELL):
        P.append(_put(t, Plant(f"s{i}", m, U + 100 + 17 * i), b"...", b"..."))
        if i % 8 == 0:
            t[U + 100 + 17 * i - 4] = 10
    return t, P


def units_over(plants, slot=16):
    """the units that hold more of the plants' last bytes than a slot"""
    per = {}
    for pl in plants:
        per[(pl.end - 1) // U] = per.get((pl.end - 1) // U, 0) + 1
    return sorted(u for u, k in per.items() if k > slot)


def report(d: Dict, kw, n, **over):
    """the report of a case's first scan on a fresh plan: the general kernel, the dictionary's own stride, a slot of 16 for records"""
    lines = bool(kw.get("count_lines")) and not kw.get("only_match")
    shorts = int(d.short_lens != 0)
    stride = over.pop("stride", d.stride)
    r = dict(road=5, ci=int(not kw.get("case_sensitive", True)), lines=int(lines), shorts=shorts, stride=stride, anch=0,
             ww_filter=int(bool(kw.get("whole_word")) and stride == 2 and not shorts), exact=0, g4x_mode=1, stage_cap=0 if lines else 16, upt=1,
             n_units=(n + U - 1) // U, overflow_units=0, emit=0, next_stage_cap=16, short_lens=d.short_lens, scans=1)
    r.update(over)
    return r


class Case:
    """steps: (text, plants, expected report) of the scans one fresh plan makes in turn; env: the environment while the plan is made
    and scans; whole_only: no windows (a max_count is a property of the whole list); unit_counts: the staging texts' per-unit
    counts, {step: {unit: matches}}; sweep: a text of sweep_text()"""

    def __init__(self, key, d, kw, steps, env=None, whole_only=False, unit_counts=None, sweep=False):
        self.key, self.d, self.pats, self.kw, self.steps, self.env = key, d, d.pats, dict(kw), steps, dict(env or {})
        self.whole_only, self.unit_counts, self.sweep = whole_only, unit_counts or {}, sweep

    @property
    def counting(self):
        return bool(self.kw.get("count_lines")) and not self.kw.get("only_match")

    def params(self, **over):
        return abi.Params(self.pats, **dict(self.kw, **over))

    def __repr__(self):
        return self.key


_ALL = []


def all_cases():
    if _ALL:
        return _ALL
    D = _dictionaries()
    out = []
    texts = {name: dictionary_text(d, 7000 + i, sprinkle=7 if name == "four130" else 0) for i, (name, d) in enumerate(D.items())}
    # ---- the 16 base instantiations: every dictionary in the four modes
    for name, d in D.items():
        t, P = texts[name]
        for tag, kw in MODES:
            out.append(Case(f"{name}/{tag}", d, kw, [(t, P, report(d, kw, d.n))]))
    # ---- further modes of the dictionaries without short patterns: -w (the WW instantiations under stride 2), -c -o, max_count
    for tag, kw in MODES:
        kww = dict(kw, whole_word=True)
        t, P = texts["four_few"]
        out.append(Case(f"four_few/w-{tag}", D["four_few"], kww, [(t, P, report(D["four_few"], kww, N5))]))
    d = D["four130"]
    t, P = texts["four130"]
    for tag, kw, whole in (("w", dict(whole_word=True), False), ("co", dict(count_lines=True, only_match=True), False), ("m1", dict(max_count=1), True),
                           ("m77", dict(max_count=77), True)):
        out.append(Case(f"four130/{tag}", d, kw, [(t, P, report(d, kw, N10))], whole_only=whole))
    # ---- the stride-1 filter forced on the dictionaries that own stride 2
    for name in ("four_few", "three_short"):
        t, P = texts[name]
        for tag, kw in MODES:
            out.append(Case(f"{name}/stride1-{tag}", D[name], kw, [(t, P, report(D[name], kw, D[name].n, stride=1))], env={"KREP_GPU_AC_STRIDE1": "1"}))
    # ---- staging roads (records wanted, the learned slot: no forced one)
    for name in ("four_few", "four130"):
        d = D[name]
        c16, c64 = {3: 16, 6: 17}, {2: 64, 7: 65}
        e16, e64 = staging_text(d, c16, 7100), staging_text(d, c64, 7101)
        over = dict(overflow_units=1, emit=1, next_stage_cap=64)
        for upt in (1, 3, 8):  # (8: the eleven units are two tickets)
            out.append(Case(f"{name}/slot16-upt{upt}", d, {}, [e16 + (report(d, {}, N10, upt=upt, **over),)], env={"KREP_GPU_AC_UPT": str(upt)},
                            unit_counts={0: c16}))
        for upt in (1, 3):
            out.append(Case(f"{name}/slot16-walk-upt{upt}", d, {}, [e16 + (report(d, {}, N10, upt=upt, **dict(over, emit=2)),)],
                            env={"KREP_GPU_AC_UPT": str(upt), "KREP_GPU_AC_NO_REDO_LIST": "1"}, unit_counts={0: c16}))
        out.append(Case(f"{name}/slot16-i", d, dict(case_sensitive=False), [e16 + (report(d, dict(case_sensitive=False), N10, **over),)],
                        unit_counts={0: c16}))
        learned = dict(stage_cap=64, next_stage_cap=64)
        steps = [e16 + (report(d, {}, N10, **over),), e16 + (report(d, {}, N10, scans=2, **learned),), e16 + (report(d, {}, N10, scans=3, **learned),),
                 e64 + (report(d, {}, N10, scans=4, overflow_units=1, emit=1, **learned),)]
        out.append(Case(f"{name}/learned", d, {}, steps, unit_counts={0: c16, 1: c16, 2: c16, 3: c64}))
        # (the learned slot under a ticket of three units: slot 64 is never parked)
        steps3 = [e16 + (report(d, {}, N10, upt=3, **over),), e64 + (report(d, {}, N10, upt=3, scans=2, overflow_units=1, emit=1, **learned),)]
        out.append(Case(f"{name}/learned-upt3", d, {}, steps3, env={"KREP_GPU_AC_UPT": "3"}, unit_counts={0: c16, 1: c64}))
    # ---- every offset of a cell as a match's last byte, in every base instantiation
    for i, name in enumerate(("four130", "four_few", "three_short", "two_short", "one_short")):
        d = D[name]
        t, P = sweep_text(d, 7200 + i)
        over = units_over(P)
        assert over == [1, 2]
        for tag, kw in MODES:
            lines = bool(kw.get("count_lines"))
            rep = report(d, kw, N10) if lines else report(d, kw, N10, overflow_units=len(over), emit=1, next_stage_cap=64)
            out.append(Case(f"{name}/sweep-{tag}", d, kw, [(t, P, rep)], sweep=True))
    _ALL.extend(out)
    return _ALL


def reference(oracle, case, text, **over):
    """(returned count, records) of the compiled reference's aho_corasick_search for the case's search on `text`"""
    return oracle.call(abi.RA_AHO_CORASICK, case.params(**over), text)


def kept(case, pos):
    return pos[: min(len(pos), case.kw.get("max_count", abi.SIZE_MAX))]
