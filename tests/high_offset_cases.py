"""The case table of the scans at a high global_base (tests/test_gpu_high_offsets.py) and its CPU-side conditions
(tests/test_high_offset_cases_cpu.py).

TEST INFRASTRUCTURE.  Every record the library writes is (offset within the buffer) + global_base.  One text of N bytes per case is
scanned at the bases 0 (the control), B1 = 2^32 - X (2^32 is buffer offset X: the plant that straddles X crosses it) and
B2 = 5 * 2^32 + 3 * 4096.  Both high bases are multiples of 4096, so everything the reference places by an offset from the text's
start (the 64/32/16-byte block grids, the 256-byte replay window counted from global_len) keeps its place, and text[0] is a
newline that no pattern begins with: nothing the bytes in front of the buffer could say changes an answer.  The expected lists are
the compiled reference's on the N bytes (oracle_lib / regex_ref) + the base — never the library's own answer at base 0.

Plants.  Two occurrences of one pattern that share a byte cannot both stand in a text, and the greedy families never report both:
so every case gets three plants at three cuts of the window list, each between two blanks —
  X = 131072   an occurrence that starts in front of X and ends behind it (a 1-byte pattern: on X - 1, its end is X),
  Y = 200000   an occurrence whose last byte is Y - 1,
  Z = 4097     an occurrence that starts at Z;
a dictionary also holds the two bytes its long plant has AT X as a pattern of their own: a record that starts at X beside the
straddling one."""
from __future__ import annotations

import numpy as np

import cases
from krep_amd import abi

N = 262144 + 4096 + 333
X, Y, Z = 131072, 200_000, 4097
B1 = (1 << 32) - X
B2 = (5 << 32) + 3 * 4096
BASES = (0, B1, B2)
CUTS = [0, 1, Z, X - 1, X, X + 1, Y, N]
LIT_ALPHA, TINY_ALPHA, RX_ALPHA = b"abcd_ \n", b"abc \n", b"abcdq \n"
assert B1 % 4096 == 0 and B2 % 4096 == 0 and B1 + X == 1 << 32 and CUTS == sorted(CUTS)


class Case:
    """kind: "lit" (plain windows), "seq" (Plan.scan_seq in text order), "block" (-c through the block loops: scan_seq + the replay),
    "multi", "multi_nl" (a dictionary with a newline inside a pattern under -c: scan_seq), "regex".
    level / om: the reference build and its only_matching global.  algo: what krep_gpu_mirror_select must name (regex: the compiler
    that takes it).  counter: the Engine method whose count must move while the case is scanned (None: the selector alone says
    which kernel); idle: one whose count must NOT move (the tiny-dictionary kernel while the general one is meant).  rounds / stage_cap: krep_gpu_debug_force_rounds / _force_stage_cap while the case runs (the large-text tile shape
    that the one-pass single-byte kernel takes; staging slots of one record, so that every unit with two hits is scanned again in
    emit mode, where the kernel itself stores the records).  whole_only: the case is scanned in one window (a max_count is a property of the whole list)."""

    def __init__(self, key, kind, pats, kw, text, algo, level=abi.REF_AVX2, om=False, counter=None, whole_only=False, count_only=False,
                 rounds=0, model=None, stage_cap=0, idle=None):
        self.key, self.kind, self.pats, self.kw, self.text, self.algo = key, kind, [bytes(p) for p in pats], dict(kw), text, algo
        self.level, self.om, self.counter, self.whole_only, self.count_only, self.rounds, self.model = level, om, counter, whole_only, count_only, rounds, model
        self.stage_cap, self.idle = stage_cap, idle

    @property
    def counting(self):
        return bool(self.kw.get("count_lines")) and not self.kw.get("only_match")

    def params(self, **over):
        kw = dict(self.kw, **over)
        return abi.Params(self.pats, regex=self.kind == "regex", **kw)

    def __repr__(self):
        return self.key


def plant(t, s, body: bytes, before=b" ", behind=b" "):
    """`body` at s with `before` in front of it and `behind` behind it"""
    a = np.frombuffer(before + body + behind, dtype=np.uint8)
    lo = s - len(before)
    assert 2 <= lo and lo + a.size <= t.size - 2
    t[lo:lo + a.size] = a


def three_plants(t, body: bytes, before=b" ", behind=b" "):
    m = len(body)
    plant(t, Z, body, before, behind)
    plant(t, Y - m, body, before, behind)
    plant(t, X - max(m // 2, 1), body, before, behind)


def background(seed, alpha):
    t = cases.rand_text(np.random.RandomState(seed), N, alpha)
    t[0] = 10
    return t


def without(t, pat: bytes):
    """no occurrence of `pat` left in t (every one loses its first byte to a blank): the plants alone are its occurrences"""
    raw = t.tobytes()
    i = raw.find(pat)
    while i >= 0:
        t[i] = 32
        raw = t.tobytes()
        i = raw.find(pat, i)
    return t


def quiet_then_dense(seed, quiet, dense, start=X + 64):
    """a text that holds nothing of a case's patterns in front of `start` but what is planted there, and the dense alphabet from
    `start` on: the first max_count records of the case reach past the plant on X, and the cut still is a real one"""
    rng = np.random.RandomState(seed)
    t = cases.rand_text(rng, N, quiet)
    t[start:] = cases.rand_text(rng, N - start, dense)
    t[0] = 10
    return t


def literal_cases():
    out = []
    lv = {"avx2": abi.REF_AVX2, "avx512": abi.REF_AVX512, "scalar": abi.REF_SCALAR}
    sse, bmh, short = abi.RA_SSE42, abi.RA_BMH, abi.RA_MEMCHR_SHORT
    t1 = background(101, LIT_ALPHA)
    three_plants(t1, b"d")
    t23 = background(102, LIT_ALPHA)
    three_plants(t23, b"cd")
    t3 = background(103, LIT_ALPHA)
    three_plants(t3, b"cda")
    # five bytes without a border: as many occurrences behind X as in front of it, so that max_count = 50 cuts behind the plant on X
    five = b"dcab_"
    assert not cases.has_border(five)
    t5 = without(background(104, LIT_ALPHA), five)
    for s in range(3000, N - 3000, 4001):
        plant(t5, s, five)
    three_plants(t5, five)
    t5i = t5.copy()
    for s in range(5000, N - 3000, 8003):  # -i: other spellings
        plant(t5i, s, b"DcAb_")
    t20, t40 = background(105, LIT_ALPHA), background(106, LIT_ALPHA)
    p20, p40 = b"abcd_dcba_abdc_cdab_"[:20], (b"abcd_dcba_abdc_cdab_" * 2)[:39] + b"d"
    for t, p in ((t20, p20), (t40, p40)):
        for s in range(2000, N - 3000, 30011):
            plant(t, s, p)
        three_plants(t, p)
        plant(t, X + 64, p)  # two more in the unit behind X: with one-record staging slots that unit is scanned again in emit mode
        plant(t, X + 192, p)
    for name, level in lv.items():
        two = short if name == "scalar" else sse
        fivea = bmh if name == "scalar" else sse
        out.append(Case(f"lit/{name}/1", "lit", [b"d"], {}, t1, abi.RA_MEMCHR, level, counter="single_launches", rounds=4))
        out.append(Case(f"lit/{name}/2", "lit", [b"cd"], {}, t23, two, level))
        out.append(Case(f"lit/{name}/3", "lit", [b"cda"], {}, t3, two, level))
        out.append(Case(f"lit/{name}/5", "lit", [five], {}, t5, fivea, level))
        out.append(Case(f"lit/{name}/5-i", "lit", [five], dict(case_sensitive=False), t5i, bmh, level))
        out.append(Case(f"lit/{name}/5-w", "lit", [five], dict(whole_word=True), t5, fivea, level))
        out.append(Case(f"lit/{name}/5-m50", "lit", [five], dict(max_count=50), t5, fivea, level, whole_only=True))
        out.append(Case(f"lit/{name}/5-c", "lit", [five], dict(count_lines=True), t5, fivea, level))
        out.append(Case(f"lit/{name}/2-emit", "lit", [b"cd"], {}, t23, two, level, stage_cap=1))
        out.append(Case(f"lit/{name}/5-emit", "lit", [five], {}, t5, fivea, level, stage_cap=1))
    out.append(Case("lit/avx2/20", "lit", [p20], {}, t20, abi.RA_AVX2, abi.REF_AVX2))
    out.append(Case("lit/avx512/40", "lit", [p40], {}, t40, abi.RA_AVX512, abi.REF_AVX512))
    out.append(Case("lit/avx2/20-emit", "lit", [p20], {}, t20, abi.RA_AVX2, abi.REF_AVX2, stage_cap=1))
    out.append(Case("lit/avx512/40-emit", "lit", [p40], {}, t40, abi.RA_AVX512, abi.REF_AVX512, stage_cap=1))
    out.append(Case("lit/avx2/1-emit", "lit", [b"d"], {}, t1, abi.RA_MEMCHR, abi.REF_AVX2, stage_cap=1))
    return out


# what krep_gpu_mirror_select names for the rows of JOBS in tests/test_gpu_chain.py (the CPU module asserts it)
SEQ_ALGOS = [abi.RA_SSE42] * 5 + [abi.RA_KMP] + [abi.RA_MEMCHR_SHORT] * 4 + [abi.RA_BMH] * 2 + [abi.RA_SSE42]


def seq_text(seed):
    from test_gpu_chain import _text
    t = _text(np.random.RandomState(seed), N, CUTS[1:-1])
    t[0] = 10
    return t


def seq_cases():
    """the rows of JOBS in tests/test_gpu_chain.py, and a repeated-byte pattern under the greedy family, count-only (kg_runs.hip)"""
    from test_gpu_chain import JOBS
    out = []
    for i, (level, pat, kw, om) in enumerate(JOBS):
        if "max_count" in kw:
            # runs of nine a's in front of X, fewer records than max_count; the clusters of the other rows' text behind it
            t = quiet_then_dense(200 + i, b"b _\n", b"aab _\n")
            runs = kw["max_count"] // 8
            for k in range(runs):
                plant(t, 6000 + k * ((X - 12000) // runs), b"a" * 9)
        else:
            t = seq_text(200 + i)
        three_plants(t, pat, b" " * 8, b" " * 8)  # (clear of the clusters around it: a walk under -o resumes behind a failed candidate)
        out.append(Case(f"seq/{i}/{pat.decode()}", "seq", [pat], kw, t, SEQ_ALGOS[i], level, om, whole_only="max_count" in kw))
    t = seq_text(250)
    three_plants(t, b"aa", b" " * 8, b" " * 8)
    out.append(Case("seq/runs/aa", "seq", [b"aa"], {}, t, abi.RA_SSE42, abi.REF_AVX2, counter="runs_launches", whole_only=True, count_only=True))
    return out


BLOCK_ALGOS = {abi.REF_AVX512: abi.RA_AVX512, abi.REF_AVX2: abi.RA_AVX2, abi.REF_NEON: abi.RA_NEON}


def block_cases():
    """the jobs of test_block_loop_count_lines_in_pieces in tests/test_gpu_chain.py"""
    from test_gpu_chain import BLOCK_JOBS
    out = []
    for i, (level, m, kw) in enumerate(BLOCK_JOBS):
        rng = np.random.RandomState(300 + i)
        t = cases.rand_text(rng, N, b"abcd_ " * 40 + b"\n")  # sparse newlines: the block grid restarts at every counted line
        t[0] = 10
        pat = cases.rand_text(rng, m, b"abcd").tobytes()
        t[N - m:] = np.frombuffer(pat, dtype=np.uint8)  # ... and one that ends the text
        for s in [N - 100, N - 255 - m, N - 257, N - 300, N - 700, 40, N // 3] + list(range(9000, N - 3000, 20011)):
            plant(t, s, pat)
        three_plants(t, pat)
        out.append(Case(f"block/{i}/{m}", "block", [pat], kw, t, BLOCK_ALGOS[level], level))
    return out


def multi_cases():
    out = []
    rng = np.random.RandomState(400)
    t = background(401, b"abcd \n")
    lens = (3, 5, 5, 9, 14, 30)
    pats = [cases.rand_text(rng, m, b"abcd").tobytes() for m in lens]
    long = pats[-1]
    pats.append(long[15:17])  # the two bytes the long plant has at X: a record that starts AT X
    three_plants(t, long)
    tt = background(402, TINY_ALPHA)
    tiny = [b"abca", b"ca", b"b", b"c ab"]
    three_plants(tt, b"abca")  # ... "ca" starts at X
    # max_count = 50: texts that hold nothing of the dictionary in front of X but a few plants, so that the cut falls behind X
    t50 = quiet_then_dense(404, b"xyz \n", b"abcd \n")
    for s in range(8000, X - 3000, 12007):
        plant(t50, s, pats[3])
    three_plants(t50, long)
    tt50 = quiet_then_dense(405, b"xyz \n", TINY_ALPHA)
    for s in range(8000, X - 3000, 15013):
        plant(tt50, s, b"abca")
    three_plants(tt50, b"abca")
    for name, text, text50, dic, counter in (("seven", t, t50, pats, None), ("tiny", tt, tt50, tiny, "tiny_launches")):
        for tag, kw, cap in (("plain", {}, 0), ("i", dict(case_sensitive=False), 0), ("w", dict(whole_word=True), 0), ("m50", dict(max_count=50), 0),
                             ("c", dict(count_lines=True), 0), ("emit", {}, 1)):
            # (-w keeps a tiny dictionary on the general kernel: kg_ac.hip)
            tiny_kernel = counter is not None and not kw.get("whole_word")
            out.append(Case(f"multi/{name}/{tag}", "multi", dic, kw, text50 if "max_count" in kw else text, abi.RA_AHO_CORASICK,
                            counter=counter if tiny_kernel else None, idle=None if tiny_kernel else "tiny_launches",
                            whole_only="max_count" in kw, stage_cap=cap))
    tn = background(403, b"ab \n")
    plant(tn, X - 1, b"a\nb")
    plant(tn, Z, b"a\nb")
    plant(tn, Y - 3, b"a\nb")
    out.append(Case("multi/newline/c", "multi_nl", [b"a\nb", b"ab"], dict(count_lines=True), tn, abi.RA_AHO_CORASICK))
    return out


RX_LONG = b"abcdbcdbcdbcdbcd"


def regex_cases():
    """one pattern per compiler, records and -c; none can overlap itself (such a regex takes one window with base 0 only)"""
    import regex_alt_model
    import regex_anchor_model
    import regex_ext_model
    import regex_model
    out = []
    table = [("fixed", b"q[a-c]{3}", b"qabc", b" ", b" ", regex_model.run, False),
             ("bol", b"^ab[cd]", b"abd", b"\n", b" ", regex_anchor_model.run, False),
             ("eol", b"d[ab]c$", b"dac", b" ", b"\n", regex_anchor_model.run, False),
             ("alt", b"q|a[b-d]{15}", RX_LONG, b" ", b" ", regex_alt_model.run, True),
             ("ext", b"q[ab]{1,2}c?d", b"qabcd", b" ", b" ", regex_ext_model.run, True)]
    for i, (name, pat, body, before, behind, model, listed) in enumerate(table):
        t = background(500 + i, RX_ALPHA)
        three_plants(t, body, before, behind)
        run = (lambda text, _m=model, _p=pat, **kw: _m([_p], text, **kw)) if listed else (lambda text, _m=model, _p=pat, **kw: _m(_p, text, **kw))
        for tag, kw in (("rec", {}), ("c", dict(count_lines=True))):
            out.append(Case(f"regex/{name}/{tag}", "regex", [pat], kw, t, name, model=run))
    return out


LOOPS_PATTERN = b"qa+b"  # the loops compiler takes one window with base 0 only

_ALL = []


def all_cases():
    if not _ALL:
        _ALL.extend(literal_cases() + seq_cases() + block_cases() + multi_cases() + regex_cases())
    return _ALL


def select(eng, case, total_len):
    """what krep_gpu_mirror_select names for the case on a text of total_len bytes, under the case's build and -o"""
    cfg = eng.default_config()
    cfg.reference_simd, cfg.only_matching = case.level, int(case.om)
    eng.set_thread_config(cfg)
    try:
        return eng.mirror_select(case.params(), total_len)
    finally:
        eng.set_thread_config(None)


def regex_compiler(eng, case):
    """the compiler that takes a regex case, asked in the order every search asks them; it must not be able to overlap itself"""
    import krep_amd
    p = case.params()
    try:
        info = eng.regex_compile_anchored(p)
        assert not info.seq.self_overlap
        return "bol" if info.bol else "eol" if info.eol else "fixed"
    except krep_amd.KrepGpuError:
        pass
    try:
        assert not eng.regex_compile_alt(p).cross_overlap
        return "alt"
    except krep_amd.KrepGpuError:
        pass
    assert not eng.regex_compile_ext(p).alt.cross_overlap
    return "ext"


def reference(oracle, eng, case, base, **over):
    """(returned count, records or None) of the compiled reference for the case's N bytes as the text [base, base + N); `over`
    changes a parameter (the CPU module asks for the records of a -c case)"""
    kw = dict(case.kw, **over)
    if case.kind == "regex":
        import regex_ref
        with regex_ref.c_locale():
            want = case.model(case.text, **kw)
            if regex_ref.available():
                ref = regex_ref.call(case.pats[0], case.text, **kw)
                assert ref[0] == want[0] and (ref[1] is None or want[1] is None or np.array_equal(ref[1], want[1])), ("model != reference", case)
        return want
    algo = select(eng, case, base + N)
    oracle.set_only_matching(case.om)
    try:
        return oracle.call(algo, abi.Params(case.pats, **kw), case.text)
    finally:
        oracle.set_only_matching(False)


def kept(case, pos):
    """the records a whole-window scan stores: the first max_count of the reference's"""
    return pos[: min(len(pos), case.kw.get("max_count", abi.SIZE_MAX))]
