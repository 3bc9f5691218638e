"""GPU parity of the multi-pattern scan for patterns of MORE than 16 bytes whose match straddles an ownership cut (tests/long_pattern_cuts.py).

The exact dictionary holds such a pattern as a 16-byte stand-in (kg_ac_anchor.hip exact_table); stage 3 of the anchored scan and the exact-slow
path of the end-gram scan (kg_ac.hip verify_ends) clip its answer by start ownership, and a stand-in clipped as if the pattern were 16 bytes
long is lost when the cut lies 16 .. L - 1 bytes in front of the match's end: the window that owns the start drops it, the next one does not own
it.  Every phrase is planted at cut - k for k = -2 .. L + 2; the two windows on either side of the cut are scanned and compared record for record —
offsets, order, count — with the brute-force list of the builder (pinned to aho_corasick_search by tests/test_long_pattern_cuts_cpu.py), never
with another GPU result.  Also here: the split dictionary's max_count == capacity (kg_scan_ac.hip scan_ac_split)."""
import os

import numpy as np
import pytest

import long_pattern_cuts as lpc
import wordlist
from krep_amd import abi
from test_gpu_anchor import _DevicePlan, forced  # noqa: F401  (the five forced anchored instantiations)

pytestmark = pytest.mark.gpu
BASE = (5 << 32) + 12345  # a global base beyond 2^32
W = lpc.WINDOW


@pytest.fixture(scope="module")
def gpu():
    import krep_amd
    e = krep_amd.load()
    assert e.device_count() >= 1
    return e


@pytest.fixture(scope="module")
def case(gpu):
    return lpc.build(gpu)


@pytest.fixture(scope="module")
def case_short(gpu):
    return lpc.build(gpu, with_short=True)


@pytest.fixture(scope="module")
def case_frequent(gpu):
    return lpc.build(gpu, frequent=True)


@pytest.fixture(scope="module")
def case_duplicate(gpu):
    return lpc.build_duplicate(gpu)


def _sweep(d, plants, expected, base=BASE, copies=1):
    """The two windows on either side of every plant's cut -> the (L, k) of the plants at which a window's list differs from the
    reference's owned records or the plant is not held exactly once (once per copy of its pattern) by the two lists together."""
    bad = []
    for q in plants:
        c = q.cut
        o_lo, lo = d.scan(c - W, c, base)
        o_hi, hi = d.scan(c, c + W, base)
        want_lo, want_hi = lpc.owned(expected, c - W, c) + base, lpc.owned(expected, c, c + W) + base
        both = np.concatenate([lo, hi])
        once = int(np.sum((both[:, 0] == q.start + base) & (both[:, 1] == q.start + q.L + base))) == copies
        if not (once and o_lo.count == len(want_lo) and o_hi.count == len(want_hi) and np.array_equal(lo, want_lo) and np.array_equal(hi, want_hi)):
            bad.append((q.L, q.k))
    return sorted(bad)


def _band(plants):
    return [q for q in plants if lpc.in_band(q.L, q.k)]


def test_anchored_windows_cut_inside_a_long_pattern(gpu, forced, case):
    """(a) the anchored instantiations: four and five classes, tickets of 3 and 8 units, verify at every unit's end"""
    before = gpu.anchored_launches()
    d = _DevicePlan(gpu, case.patterns, {}, case.text)
    try:
        out, rec = d.scan()  # (takes the anchor decision; own_hi == text_len: nothing is cut)
        assert out.count == len(case.expected) and np.array_equal(rec, case.expected)
        assert d.plan.anchor_info()[0] == 2 and gpu.anchored_launches() > before
        before = gpu.anchored_launches()
        bad = _sweep(d, case.plants, case.expected)
        assert not bad, "(L, k) of the plants a window lost or doubled: " + repr(bad)
        assert gpu.anchored_launches() >= before + 2 * len(case.plants)
    finally:
        d.close()


def test_a_real_duplicate_across_cuts_is_reported_once_per_copy(gpu, forced, case_duplicate):
    """The other kind of `multi` entry: a word of at most 16 bytes that the dictionary holds twice.  Its bit of the depth mask IS its
    length; the level walk answers for it all the same and reports it once per copy, from the window that owns its start alone."""
    cs = case_duplicate
    d = _DevicePlan(gpu, cs.patterns, {}, cs.text)
    try:
        out, rec = d.scan()
        assert out.count == len(cs.expected) and np.array_equal(rec, cs.expected)
        assert d.plan.anchor_info()[0] == 2
        bad = _sweep(d, cs.plants, cs.expected, copies=2)
        assert not bad, "(L, k) of the plants a window lost, doubled or reported for one copy only: " + repr(bad)
    finally:
        d.close()


@pytest.mark.parametrize("how", ["anchors switched off per scan", "a dictionary that keeps its end grams"])
def test_end_gram_windows_with_the_exact_dictionary(gpu, case, case_frequent, how):
    """(b) the end-gram instantiation with the exact dictionary present (the exact-slow block of verify_ends): the plan decides for anchors and
    $KREP_GPU_AC_NO_ANCHOR, read per scan, keeps the end-gram filter; and a dictionary of frequent words, which stays on its end grams on word
    text while the frequency of those grams (`wordy`, kg_ac_anchor.hip) builds the exact dictionary.  The phrases' last words share their last
    four bytes with other words of the dictionary: the chain-compressed entry cannot answer such an end."""
    switched = how.startswith("anchors")
    cs = case if switched else case_frequent
    if switched:
        os.environ["KREP_GPU_AC_ANCHOR"] = "1"
    try:
        d = _DevicePlan(gpu, cs.patterns, {}, cs.text)
        try:
            out, rec = d.scan()
            assert out.count == len(cs.expected) and np.array_equal(rec, cs.expected)
            assert d.plan.anchor_info()[0] == (2 if switched else 1), d.plan.anchor_info()
            if switched:
                os.environ["KREP_GPU_AC_NO_ANCHOR"] = "1"
            before = gpu.anchored_launches()
            bad = _sweep(d, cs.plants, cs.expected)
            assert gpu.anchored_launches() == before  # the end-gram instantiation is what ran
            assert not bad, "(L, k) of the plants a window lost or doubled: " + repr(bad)
        finally:
            d.close()
    finally:
        os.environ.pop("KREP_GPU_AC_ANCHOR", None)
        os.environ.pop("KREP_GPU_AC_NO_ANCHOR", None)


@pytest.fixture(scope="module")
def option_lists(case):
    """the reference's lists under -i (patterns in upper case against the lower-case text) and -w, computed once"""
    upper = [p.upper() for p in case.patterns]
    return upper, lpc.brute_force(case.text, upper, case_sensitive=False), lpc.brute_force(case.text, case.patterns, whole_word=True)


def test_anchored_windows_under_options(gpu, forced, case, option_lists):
    """(c) -i, -w and max_count over the band of (a).  max_count cuts a window's list in the emission order: 1, with the window starting at the
    plant (the plant or nothing in front of it is the answer), and 5, with a window that starts as many records in front of the plant as make the
    plant the list's last record — a list that ends between two plants."""
    upper, exp_i, exp_w = option_lists
    band = _band(case.plants)
    assert len(band) == sum(len(p) - 16 for p in case.phrases)
    problems = []  # (every option is run before the verdict)
    for pats, kw, exp in ((upper, dict(case_sensitive=False), exp_i), (case.patterns, dict(whole_word=True), exp_w)):
        d = _DevicePlan(gpu, pats, kw, case.text)
        try:
            out, rec = d.scan()
            assert np.array_equal(rec, exp) and d.plan.anchor_info()[0] == 2, kw
            bad = _sweep(d, band, exp)
            if bad:
                problems.append(repr(kw) + ": (L, k) of the plants a window lost or doubled: " + repr(bad))
        finally:
            d.close()
    exp = case.expected
    for m in (1, 5):
        d = _DevicePlan(gpu, case.patterns, dict(max_count=m), case.text)
        try:
            out, rec = d.scan()
            assert out.count == m and np.array_equal(rec, exp[:m]) and d.plan.anchor_info()[0] == 2
            bad = []
            for q in band:
                lo = q.start
                if m > 1:  # the window start that puts m - 1 owned records in front of the plant in the emission order
                    near = exp[(exp[:, 0] < q.start) & (exp[:, 0] >= q.start - 4 * W)]
                    for lo in sorted(set(near[:, 0].tolist()), reverse=True):
                        own = lpc.owned(exp, lo, q.cut)
                        at = int(np.flatnonzero((own[:, 0] == q.start) & (own[:, 1] == q.start + q.L))[0])
                        if at >= m - 1:
                            break
                    assert at == m - 1, (q, at)
                want = lpc.owned(exp, lo, q.cut)[:m] + BASE
                assert (want[-1] == (q.start + BASE, q.start + q.L + BASE)).all()  # (the plant ends the list)
                out, rec = d.scan(lo, q.cut, BASE)
                if not (out.count == len(want) and np.array_equal(rec, want)):
                    bad.append((q.L, q.k))
            if bad:
                problems.append("max_count %d: (L, k) of the plants whose limited list differs: " % m + repr(sorted(bad)))
        finally:
            d.close()
    assert not problems, "\n".join(problems)


def test_counts_across_a_cut_inside_a_long_pattern(gpu, oracle_engine, case):
    """(c) -c in both forms over one cut per phrase, the two windows' results combined (krep_gpu_combine_line_counts) against the reference's
    count.  The line count owns by END in the kernel and does not run the anchored instantiation: it guards the roads around it.  The occurrence
    count (-c -o) owns by START and goes through the same stage 3 as the records: it lost one match per cut before the stand-in rule was fixed."""
    import torch
    n = len(case.text)
    buf = torch.from_numpy(np.ascontiguousarray(case.text)).cuda()
    cuts = [next(q.cut for q in case.plants if q.phrase == pi and q.k == 1) for pi in range(len(case.phrases))]
    problems = []
    for kw in (dict(count_lines=True), dict(count_lines=True, only_match=True)):
        want = oracle_engine.call(abi.RA_AHO_CORASICK, abi.Params(case.patterns, **kw), case.text)[0]
        if kw.get("only_match"):
            assert want == len(case.expected)
        plan = gpu.plan(abi.Params(case.patterns, **kw))
        try:
            assert plan.scan(buf.data_ptr(), n).count == want
            for c in cuts:
                outs = [plan.scan(buf.data_ptr(), n, 0, c), plan.scan(buf.data_ptr(), n, c, n)]
                got = outs[0].count + outs[1].count if kw.get("only_match") else gpu.lib.krep_gpu_combine_line_counts((abi.ScanOut * 2)(*outs), 2)
                if got != want:
                    problems.append((kw, "cut", c, "counted", int(got), "reference", int(want)))
        finally:
            plan.close()
    assert not problems, repr(problems)


def test_split_dictionary_windows_cut_inside_a_long_pattern(gpu, case_short):
    """(d) with 1..3-byte words in the list the plan scans the phrases in the long part of a split dictionary (kg_scan_ac.hip scan_ac_split)"""
    cs = case_short
    d = _DevicePlan(gpu, cs.patterns, {}, cs.text)
    try:
        out, rec = d.scan()
        assert out.count == len(cs.expected) and np.array_equal(rec, cs.expected)
        assert d.plan.split_state() == 2
        bad = _sweep(d, _band(cs.plants), cs.expected)
        assert d.plan.split_state() == 2
        assert not bad, "(L, k) of the plants a window lost or doubled: " + repr(bad)
    finally:
        d.close()


HOST_LEN = 427 * 3 * 4096  # ~5 MiB; a multiple of 3 * 4096: the shares of three shards end on multiples of 4096


@pytest.fixture(scope="module")
def host_base(gpu):
    w = wordlist.word_list()
    return gpu.generate_host(HOST_LEN, 0, 5, lpc.SEED, wordlist.pack(w), lpc.LINE)


@pytest.mark.parametrize("L", [20, 40])
def test_host_path_pieces_cut_inside_a_long_pattern(gpu, oracle_engine, case, host_base, L):
    """(e) the host path: a text streamed in 1-MiB pieces (gpu.search) and one cut into three shards (search_buffer).  kg_exec.hip piece_layout
    cuts at multiples of the chunk inside a shard and at multiples of ceil(len / shards): multiples of 4096 for this length, so a phrase that
    starts j bytes in front of EVERY multiple of 4096 meets every cut with j bytes in front of it."""
    phrase = case.phrases[lpc.PHRASE_LENS.index(L)]
    share = (HOST_LEN + 2) // 3
    assert share % 4096 == 0 and (1 << 20) % 4096 == 0 and HOST_LEN > 2 * (1 << 20)
    bad = []
    try:
        for j in range(0, L + 2):
            text, starts = lpc.host_text(host_base, phrase, j)
            assert bytes(text).count(phrase) == len(starts)
            p = abi.Params(case.patterns)
            want = oracle_engine.call(abi.RA_AHO_CORASICK, p, text)
            held = set(map(tuple, want[1].astype(np.int64).tolist()))
            assert all((s, s + L) in held for s in starts)
            gpu.set_stream_chunk(1 << 20)
            got = gpu.search(abi.Params(case.patterns), text)
            gpu.set_stream_chunk(0)
            rc, cnt, pos = gpu.search_buffer(abi.Params(case.patterns), text, num_gpus=3)
            assert rc == 0
            if not (got[0] == want[0] and np.array_equal(got[1], want[1])):
                bad.append(("1-MiB pieces", L, j, int(want[0]) - int(got[0])))
            if not (cnt == want[0] and np.array_equal(pos, want[1])):
                bad.append(("three shards", L, j, int(want[0]) - int(cnt)))
    finally:
        gpu.set_stream_chunk(0)
    assert not bad, "(road, L, j, records missing): " + repr(bad)


@pytest.fixture(scope="module")
def long_first(gpu, case_short):
    """A text on which the LONG part of the split dictionary alone has more than 1000 matches in front of the short part's first one: 1100 copies
    of a dictionary word that holds none of the short words, then the word text."""
    short = [p for p in case_short.patterns if len(p) < 4]
    word = next(p for p in case_short.patterns if 6 <= len(p) <= 16 and not any(s in p + b" " + p for s in short))
    head = b"".join(word + (b"\n" if i % 8 == 7 else b" ") for i in range(1100))
    text = np.concatenate([np.frombuffer(head, dtype=np.uint8), case_short.text[: lpc.TEXT_LEN - len(head)]])
    exp = lpc.brute_force(text, case_short.patterns)
    assert len(exp) > 3000 and bool(np.all(exp[:1100, 1] - exp[:1100, 0] == len(word))) and int(exp[1100, 1]) > len(head)
    assert int(np.min(exp[exp[:, 1] - exp[:, 0] < 4][:, 0])) >= len(head)  # the short part's first match lies behind all of them
    return text, exp


@pytest.mark.parametrize("cap", [1, 64, 1000])
def test_split_dictionary_with_max_count_equal_to_capacity(gpu, case_short, long_first, cap):
    """(f) the first max_count records of the MERGED list when max_count equals the caller's capacity: on a text whose first records are the long
    part's alone, and on the word text, where the short part is dense and either part alone fills the list.  Beside it max_count = cap - 1 (the
    limited road as it was) and cap + 1 (more matches than the list holds: overflow, the count right)."""
    import torch
    dense = (case_short.text, case_short.expected)
    assert int(np.sum(dense[1][:1001, 1] - dense[1][:1001, 0] < 4)) > 500  # (dense: most of the first records are the short part's)
    bad = []
    for m in (cap, cap - 1, cap + 1):
        plan = gpu.plan(abi.Params(case_short.patterns, max_count=m))
        pos = torch.zeros(2 * cap, dtype=torch.int64, device="cuda")
        try:
            for name, (text, exp) in (("long part first", long_first), ("short part dense", dense)):
                assert len(exp) > cap + 1
                buf = torch.from_numpy(np.ascontiguousarray(text)).cuda()
                for rep in range(2):
                    pos.fill_(-1)
                    out = plan.scan(buf.data_ptr(), len(text), 0, len(text), 0, pos.data_ptr(), cap)
                    rec = pos[: 2 * out.stored].cpu().numpy().reshape(-1, 2)
                    if m <= cap:
                        ok = out.count == m and out.stored == m and not out.overflow and np.array_equal(rec, exp[:m])
                    else:
                        ok = out.count == m and bool(out.overflow)
                    if not ok:
                        bad.append((name, "max_count", m, "capacity", cap, "scan", rep, int(out.count), int(out.stored), int(out.overflow)))
                if m:
                    assert plan.split_state() == 2, (m, plan.split_state())
        finally:
            plan.close()
    assert not bad, repr(bad)
