"""GPU parity for the multi-pattern scan against the oracle restatement of aho_corasick_search
(count, every (start,end) record, and the reference's emission order: end ascending, longest first)."""
import json
import os

import numpy as np
import pytest

import cases
from krep_amd import abi

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def gpu():
    import krep_amd
    e = krep_amd.load()
    assert e.device_count() >= 1
    return e


def _check(gpu, o, text, pats, kw):
    want = o.call(abi.RA_AHO_CORASICK, abi.Params(pats, **kw), text)
    got = gpu.search(abi.Params(pats, **kw), text)
    assert got[0] == want[0], (pats[:6], kw, len(text), got[0], want[0])
    assert np.array_equal(got[1], want[1]), (pats[:6], kw, got[1][:8], want[1][:8])


def test_reference_vectors(gpu, oracle_engine):
    kat = [v for v in json.load(open(os.path.join(HERE, "golden", "reference_kat.json"))) if v["algos"] == ["ac"]]
    assert len(kat) >= 10
    for v in kat:
        kw = dict(case_sensitive=v["case_sensitive"], max_count=abi.SIZE_MAX if v["max_count"] is None else v["max_count"],
                  track_positions=bool(v["track_positions"]))
        p = abi.Params([s.encode() for s in v["patterns"]], **kw)
        ret, pos = gpu.search(p, v["text"].encode())
        assert ret == v["expect"], v["src"]
        if v["expect_result_count"] is not None:
            assert len(pos) == v["expect_result_count"], v["src"]


@pytest.mark.parametrize("seed", range(5))
def test_random_pattern_sets(gpu, oracle_engine, seed):
    rng = np.random.RandomState(500 + seed)
    for it in range(40):
        alpha = [b"ab", b"abc\n", b"abAB -\n", bytes(range(97, 105)) + b" \n"][it % 4]
        n = [0, 3, 17, 500, 8192, 8195, 40000, 140000][rng.randint(0, 8)]
        text = cases.rand_text(rng, n, alpha)
        k = [2, 3, 5, 9, 40][rng.randint(0, 5)]
        lens = [[1, 2, 3], [2, 3, 4, 6], [4, 5, 8, 16], [1, 4, 9, 30], [3, 3, 3]][rng.randint(0, 5)]
        pats = [cases.pick_pattern(rng, text, lens[rng.randint(0, len(lens))], alpha) for _ in range(k)]
        if rng.rand() < 0.3:
            pats.append(pats[0])  # duplicate pattern: the reference emits it twice
        kw = dict(case_sensitive=bool(rng.rand() < 0.6), whole_word=bool(rng.rand() < 0.25),
                  max_count=[abi.SIZE_MAX, abi.SIZE_MAX, abi.SIZE_MAX, 0, 1, 4, 77][rng.randint(0, 7)])
        mode = ["pos", "pos", "lines", "count"][rng.randint(0, 4)]
        if mode == "lines":
            if any(b"\n" in p for p in pats):
                continue
            kw.update(count_lines=True)
        elif mode == "count":
            kw.update(count_lines=True, only_match=True)
        _check(gpu, oracle_engine, text, pats, kw)


def test_thousand_patterns(gpu, oracle_engine):
    """BASELINE config 4 in miniature: 1000 patterns of length 4..16 over a-z, planted + chance hits."""
    rng = np.random.RandomState(1234)
    az = bytes(range(97, 123))
    pats = [cases.rand_text(rng, rng.randint(4, 17), az).tobytes() for _ in range(1000)]
    text = cases.rand_text(rng, 1 << 21, az + b"  \n")
    for _ in range(3000):
        p = np.frombuffer(pats[rng.randint(0, 1000)], dtype=np.uint8)
        s = rng.randint(0, text.size - p.size)
        text[s:s + p.size] = p
    _check(gpu, oracle_engine, text, pats, dict())
    _check(gpu, oracle_engine, text, pats, dict(count_lines=True))
    _check(gpu, oracle_engine, text, pats, dict(max_count=1000))
    _check(gpu, oracle_engine, text, pats, dict(case_sensitive=False, whole_word=True))


def test_dense_nested(gpu, oracle_engine):
    text = np.frombuffer(b"abc" * 20000, dtype=np.uint8)
    _check(gpu, oracle_engine, text, [b"a", b"b", b"c", b"ab", b"bc", b"abc", b"cab", b"abcabc"], dict())
    try:
        gpu.force_stage_cap(4)
        _check(gpu, oracle_engine, text, [b"a", b"ab", b"abc", b"bca"], dict())
    finally:
        gpu.force_stage_cap(0)


def test_binary_patterns_and_text(gpu, oracle_engine):
    rng = np.random.RandomState(44)
    text = rng.randint(0, 256, size=90_000).astype(np.uint8)
    pats = []
    for m in (1, 2, 3, 5, 9, 16, 17, 40):
        s = rng.randint(0, text.size - m)
        pats.append(text[s:s + m].tobytes())
        for t in rng.randint(0, text.size - m, 5):
            text[t:t + m] = np.frombuffer(pats[-1], dtype=np.uint8)
    _check(gpu, oracle_engine, text, pats, dict())
    _check(gpu, oracle_engine, text, pats, dict(case_sensitive=False, whole_word=True))
    _check(gpu, oracle_engine, text, [p for p in pats if len(p) >= 4 and len(p) <= 16], dict(max_count=9))


@pytest.mark.parametrize("seed", range(4))
def test_long_pattern_sets_chain_verifier(gpu, oracle_engine, seed):
    """Every pattern >= 4 bytes (the exact-class filter + chain-compressed verifier): unary chains with nested
    pattern ends, chains running past depth 16, branching below depth 4, duplicates, -w, -i, -c, tiny texts."""
    rng = np.random.RandomState(900 + seed)
    for it in range(40):
        alpha = [b"ab", b"abcd", b"abAB_ ", bytes(range(97, 123)) + b" \n"][it % 4]
        n = [10, 17, 40, 500, 16384, 16400, 70000, 200000][rng.randint(0, 8)]
        text = cases.rand_text(rng, n, alpha)
        base = cases.pick_pattern(rng, text, [8, 20, 40, 70][rng.randint(0, 4)], alpha)
        pats = [base]
        for _ in range([1, 3, 8, 30][rng.randint(0, 4)]):
            r = rng.rand()
            if r < 0.3 and len(base) > 5:      # a suffix of `base`: ends nested along one chain
                pats.append(base[rng.randint(0, len(base) - 4):])
            elif r < 0.5 and len(base) > 6:    # same tail, different head: the trie branches below depth 4
                cut = rng.randint(1, len(base) - 4)
                pats.append(cases.rand_text(rng, rng.randint(1, 6), alpha).tobytes() + base[cut:])
            elif r < 0.6:
                pats.append(pats[rng.randint(0, len(pats))])  # duplicate
            else:
                pats.append(cases.pick_pattern(rng, text, rng.randint(4, 24), alpha))
        pats = [p for p in pats if len(p) >= 4]
        kw = dict(case_sensitive=bool(rng.rand() < 0.6), whole_word=bool(rng.rand() < 0.25),
                  max_count=[abi.SIZE_MAX, abi.SIZE_MAX, 0, 1, 5][rng.randint(0, 5)])
        mode = ["pos", "pos", "lines", "count"][rng.randint(0, 4)]
        if mode == "lines":
            if any(b"\n" in p for p in pats):
                continue
            kw.update(count_lines=True)
        elif mode == "count":
            kw.update(count_lines=True, only_match=True)
        _check(gpu, oracle_engine, text, pats, kw)


def test_linear_probing_fallback_layout(gpu, oracle_engine, monkeypatch):
    """Dictionaries too large for the two-entry-bucket layout of the 4-gram table keep linear probing; the test hook
    forces that layout for ordinary dictionaries (fresh pattern sets: plans are cached per parameter set)."""
    monkeypatch.setenv("KREP_GPU_AC_LINEAR", "1")
    rng = np.random.RandomState(4242)
    az = bytes(range(97, 123))
    for it in range(6):
        text = cases.rand_text(rng, [40000, 140000, 300000][it % 3], az + b" \n")
        pats = [cases.pick_pattern(rng, text, int(rng.randint(4, 20)), az) for _ in range([30, 300, 900][it % 3])]
        for kw in (dict(), dict(case_sensitive=False), dict(count_lines=True)):
            if kw.get("count_lines") and any(b"\n" in p for p in pats):
                continue
            _check(gpu, oracle_engine, text, pats, kw)


def test_worst_legal_dictionary_1024_patterns_of_up_to_1024_bytes(gpu, oracle_engine):
    """The largest dictionary the reference CLI accepts: 1024 patterns (krep.c:3460-3465, :3552) of up to MAX_PATTERN_LENGTH =
    1024 bytes (krep.c:77, :2042) — ~0.5 M trie states.  Mixed lengths (4 ... 1024, a few 1-3-byte ones in the second set),
    duplicates, nested suffixes, shared tails that branch below depth 4, -i / -w / -c / max_count, every pattern planted,
    against aho_corasick_search of the compiled reference (VERDICT r03 missing #3)."""
    rng = np.random.RandomState(771)
    az = bytes(range(97, 123))
    alpha = az + b"ABCXYZ_ \n"

    def rnd(k, a=az):
        return bytes(a[i] for i in rng.randint(0, len(a), k))

    for variant in range(2):
        lens = list(rng.randint(4, 1025, 600)) + [1024] * 40 + list(rng.randint(4, 24, 300))
        pats = [rnd(int(k)) for k in lens]
        base = pats[:40]
        for b in base[:30]:                       # nested suffixes along one chain
            pats.append(b[int(rng.randint(1, len(b) - 4)):])
        for b in base[10:30]:                     # same tail, different head: branching below depth 4
            pats.append(rnd(int(rng.randint(1, 9))) + b[-int(rng.randint(4, min(len(b), 200))):])
        pats += [pats[3], pats[700], pats[41]]    # duplicates: the reference emits each copy
        if variant == 1:
            pats += [b"q", b"zx", b"kvb"]         # short patterns switch the filter to the wildcard-expanded table
            pats = [p.upper() if i % 7 == 0 else p for i, p in enumerate(pats)]
        pats = pats[:1024]
        while len(pats) < 1024:
            pats.append(rnd(int(rng.randint(4, 400))))
        assert len(pats) == 1024 and max(map(len, pats)) == 1024
        n = 6 << 20
        text = cases.rand_text(rng, n, alpha)
        at = 100
        for i, p in enumerate(pats):              # every pattern planted once, some back to back, some with a word boundary
            if at + len(p) + 2 >= n:
                break
            q = p.swapcase() if (variant == 1 and i % 3 == 0) else p
            text[at:at + len(q)] = np.frombuffer(q, dtype=np.uint8)
            at += len(p) + [0, 1, 37, 900][i % 4]
        no_nl = [p for p in pats if b"\n" not in p]
        assert len(no_nl) == len(pats)
        for kw in (dict(), dict(case_sensitive=False), dict(whole_word=True), dict(count_lines=True),
                   dict(count_lines=True, only_match=True), dict(max_count=100), dict(case_sensitive=False, whole_word=True, count_lines=True)):
            _check(gpu, oracle_engine, text, pats, kw)
        # and a small window whose length is below the longest pattern
        _check(gpu, oracle_engine, text[90:700], pats, dict())


def test_count_lines_pieces_on_different_roads_own_a_straddling_match_once(gpu, oracle_engine, monkeypatch):
    """multi-pattern -c picks its road per piece — in the kernel below 32 MiB of buffer (or when the plan has
    seen a dense text), on the record list above.  Both roads own a match by its END, so a match across the cut between two
    pieces on different roads is counted exactly once: a small piece followed by a >= 32 MiB piece (the default streaming
    layout: a shard's short last chunk, then the next shard's first 128-MiB chunk), the opposite order, and the roads forced
    alternately over many cuts of one buffer ("dense shard, then sparse shard").  Every straddling match is the only one on
    its line, at every split of its bytes; general kernel and register-compare (tiny) dictionary; -w, -i."""
    import torch
    rng = np.random.RandomState(20260926)
    n = 40 << 20
    az = bytes(range(97, 123))
    text = cases.rand_text(rng, n, az + b" \n")
    big = [cases.pick_pattern(rng, text[: 1 << 20], int(rng.randint(5, 14)), az) for _ in range(40)]
    big = [q for q in big if b"\n" not in q and b" " not in q]
    for pats in (big + [b"QXJZKWVQ", b"QXJZ"], [b"QX", b"XJZ", b"JZKW"]):
        strad = pats[-2] if len(pats) > 3 else b"XJZKW"   # (tiny: XJZ ends inside, JZKW ends behind the cut or on it)
        L = len(strad)
        cuts = [(i + 1) * (3 << 20) + 17 * i + 5 for i in range(12)]
        t = text.copy()
        for i, c in enumerate(cuts):
            k = 1 + i % (L - 1)                    # bytes of the straddler in front of the cut
            t[c - 200:c + 200] = ord("-")
            t[c - 120] = t[c + 120] = 10
            t[c - k:c - k + L] = np.frombuffer(strad, dtype=np.uint8)
        d = torch.from_numpy(t).cuda()
        for kw in (dict(), dict(whole_word=True), dict(case_sensitive=False)):
            kwc = dict(count_lines=True, **kw)
            want = oracle_engine.call(abi.RA_AHO_CORASICK, abi.Params(pats, **kwc), t)[0]
            plan = gpu.plan(abi.Params(pats, **kwc))
            assert plan.scan(d.data_ptr(), n).count == want
            halo = 1100
            # (1) buffers of their own: [0, c + halo) is below 32 MiB -> in-kernel road, [c - halo, n) is above -> list road
            for c in cuts[:3]:
                a = plan.scan(d.data_ptr(), c + halo, 0, c, 0, global_len=n)
                b = plan.scan(d.data_ptr() + c - halo, n - (c - halo), halo, n - (c - halo), c - halo, global_len=n)
                arr = (abi.ScanOut * 2)(a, b)
                assert gpu.lib.krep_gpu_combine_line_counts(arr, 2) == want, ("small then large", kw, c)
            # (2) the opposite order: [0, c + halo) large (list), [c - halo, n) small (in the kernel)
            c = cuts[-1]
            a = plan.scan(d.data_ptr(), c + halo, 0, c, 0, global_len=n)
            b = plan.scan(d.data_ptr() + c - halo, n - (c - halo), halo, n - (c - halo), c - halo, global_len=n)
            assert gpu.lib.krep_gpu_combine_line_counts((abi.ScanOut * 2)(a, b), 2) == want, ("large then small", kw)
            # (3) windows of one buffer, the road forced alternately
            edges = [0] + cuts + [n]
            for first_inkernel in (0, 1):
                outs = []
                for j, (lo, hi) in enumerate(zip(edges[:-1], edges[1:])):
                    if (j + first_inkernel) % 2:
                        monkeypatch.setenv("KREP_GPU_AC_LINES_INKERNEL", "1")
                    outs.append(plan.scan(d.data_ptr(), n, lo, hi))
                    monkeypatch.delenv("KREP_GPU_AC_LINES_INKERNEL", raising=False)
                arr = (abi.ScanOut * len(outs))(*outs)
                assert gpu.lib.krep_gpu_combine_line_counts(arr, len(outs)) == want, ("alternating", kw, first_inkernel)
            plan.close()
        del d


def test_count_lines_gap_test_is_exact_per_byte(gpu, oracle_engine):
    """the newline test of the gap between two neighbouring records (kg_tail.hip tail_gap_has_newline) must be exact per
    byte — with the borrow-based zero-byte trick a real '\\n' just in front of the gap flagged the 0x0b bytes behind it."""
    import torch
    rng = np.random.RandomState(77)
    n = 33 << 20
    text = cases.rand_text(rng, n, b"abcdefgh\x0b\x0b \n")
    text[:6] = np.frombuffer(b"\n\x0b\x0ba \n", dtype=np.uint8)
    d = torch.from_numpy(text).cuda()
    for pats, kw in (([b"\x0b", b"zz"], dict(whole_word=True)), ([b"\x0b", b"a\x0b"], dict()), ([b"\x0b", b"\x0ba", b"cd"], dict(whole_word=True))):
        kwc = dict(count_lines=True, **kw)
        want = oracle_engine.call(abi.RA_AHO_CORASICK, abi.Params(pats, **kwc), text)[0]
        plan = gpu.plan(abi.Params(pats, **kwc))
        got = plan.scan(d.data_ptr(), n)
        plan.close()
        assert got.count == want, (pats, kw, got.count, want)


def test_count_lines_on_the_record_list(gpu, oracle_engine, monkeypatch):
    """Multi-pattern -c on a text large enough for the list road (kg_scan_ac.hip scan_ac_lines_on_list: records by the fast
    kernel, lines counted on the end-ordered list by their newline gaps): whole text and ownership windows (the line summary
    of each window folds with krep_gpu_combine_line_counts), -w, -i, max_count, a text without any newline, a newline-free
    half, and the in-kernel road on the same input — all against aho_corasick_search of the compiled reference."""
    import torch
    rng = np.random.RandomState(4711)
    n = 40 << 20
    az = bytes(range(97, 123))
    for variant in ("lines", "few_newlines", "no_newline"):
        alpha = az + (b" \n" if variant == "lines" else b" ")
        text = cases.rand_text(rng, n, alpha)
        if variant == "few_newlines":  # newlines only in the first half: long gaps behind them
            nl = rng.randint(0, n // 2, 3000)
            text[nl] = 10
        pats = []
        while len(pats) < 60:  # (no newline inside a pattern: that class counts emission-order line changes, one window only)
            q = cases.pick_pattern(rng, text[: 1 << 20], int(rng.randint(4, 14)), az)
            if b"\n" not in q:
                pats.append(q)
        pats += [pats[0][1:] + b"q", b"zq" + pats[1]]  # neighbours that overlap / nest their ends
        d = torch.from_numpy(text).cuda()
        for kw in (dict(), dict(whole_word=True), dict(case_sensitive=False), dict(max_count=1000)):
            kwc = dict(count_lines=True, **kw)
            want = oracle_engine.call(abi.RA_AHO_CORASICK, abi.Params(pats, **kwc), text)[0]
            plan = gpu.plan(abi.Params(pats, **kwc))
            whole = plan.scan(d.data_ptr(), n)
            assert whole.count == want, (variant, kw, whole.count, want)
            monkeypatch.setenv("KREP_GPU_AC_LINES_INKERNEL", "1")
            inker = plan.scan(d.data_ptr(), n)
            monkeypatch.delenv("KREP_GPU_AC_LINES_INKERNEL")
            assert (inker.count, inker.line_count, inker.total_matches) == (whole.count, whole.line_count, whole.total_matches)
            if "max_count" in kw:
                plan.close()
                continue
            # the host-buffer operator on the same text, streamed in 33 MiB pieces (each piece takes the list road, the line
            # summaries of the pieces fold on the host) and sharded over three logical devices
            gpu.set_stream_chunk(33 << 20)
            try:
                got_stream = gpu.search(abi.Params(pats, **kwc), text, want_result=False)[0]
                rc, got_shard, _ = gpu.search_buffer(abi.Params(pats, **kwc), text, num_gpus=3, want_result=False)
            finally:
                gpu.set_stream_chunk(0)
            assert got_stream == want and got_shard == want and rc == (0 if want else 1), (variant, kw, got_stream, got_shard, want)
            cuts = [0, 5, (1 << 20) + 3, 17 << 20, (17 << 20) + 1, 33 << 20, n]
            outs = [plan.scan(d.data_ptr(), n, lo, hi) for lo, hi in zip(cuts[:-1], cuts[1:])]
            arr = (abi.ScanOut * len(outs))(*outs)
            assert gpu.lib.krep_gpu_combine_line_counts(arr, len(outs)) == want, (variant, kw)
            assert sum(o.total_matches for o in outs) == whole.total_matches
            plan.close()
        del d
