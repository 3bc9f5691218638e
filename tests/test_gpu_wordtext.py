"""GPU parity on WORD TEXT (generator kind 5, krep_amd/csrc/kg_synth.h): natural-language-like lines — frequent short words,
shared affixes (-tion, -ment, -ing ...), repeated grams — with word dictionaries drawn from the same list, against the
compiled reference (aho_corasick_search, aho_corasick.c:299-466; the single-literal functions through the mirror selector).
Round 6 (VERDICT r05 missing #2): every earlier parity text was i.i.d. letters, on which a gram filter sees ~0.4 % candidates;
here the filter's candidate rate is 10-100x that and the verify stage, its slow paths and the overflow / emit-mode roads of the
staging slots carry the load."""
import numpy as np
import pytest

import cases
import wordlist
from krep_amd import abi

pytestmark = pytest.mark.gpu
SEED, LINE = 20260930, 80


@pytest.fixture(scope="module")
def gpu():
    import krep_amd
    e = krep_amd.load()
    assert e.device_count() >= 1
    return e


@pytest.fixture(scope="module")
def words():
    w = wordlist.word_list()
    return w, wordlist.pack(w)


def _check_ac(gpu, o, text, pats, kw):
    want = o.call(abi.RA_AHO_CORASICK, abi.Params(pats, **kw), text)
    got = gpu.search(abi.Params(pats, **kw), text)
    assert got[0] == want[0], (pats[:4], kw, len(text), got[0], want[0])
    assert np.array_equal(got[1], want[1]), (pats[:4], kw, got[1][:8], want[1][:8])


def test_device_generator_equals_host_twin(gpu, words):
    import torch
    _, blob = words
    n, off = (1 << 20) + 123, 7 * LINE + 33
    buf = torch.empty(n, dtype=torch.uint8, device="cuda")
    gpu.generate(buf.data_ptr(), n, off, 5, SEED, blob, LINE)
    assert np.array_equal(buf.cpu().numpy(), gpu.generate_host(n, off, 5, SEED, blob, LINE))


@pytest.mark.parametrize("kind", ["rare", "uniform", "common"])
def test_word_dictionaries_on_word_text(gpu, oracle_engine, words, kind):
    w, blob = words
    text = gpu.generate_host((3 << 20) + 4321, 0, 5, SEED, blob, LINE)
    pats = wordlist.dictionary(w, kind)
    assert len(pats) == 1000
    before = gpu.anchored_launches()
    _check_ac(gpu, oracle_engine, text, pats, dict())
    if kind != "common":  # (a dictionary of FREQUENT words: its rarest windows are common too, the estimate keeps the end grams)
        assert gpu.anchored_launches() > before  # word dictionaries on word text take the anchored instantiation (kg_ac_anchor.hip)
    _check_ac(gpu, oracle_engine, text, pats, dict(count_lines=True))
    _check_ac(gpu, oracle_engine, text, pats, dict(count_lines=True, only_match=True))
    _check_ac(gpu, oracle_engine, text, pats, dict(whole_word=True))
    _check_ac(gpu, oracle_engine, text, pats, dict(case_sensitive=False, max_count=5000))


def test_frequent_words_and_affixes_as_a_dictionary(gpu, oracle_engine, words):
    """The densest realistic dictionaries: function words, bare affixes (every `tion`, `ment`, `ing` of the text is a match) and
    words that are suffixes of other dictionary words (longest-first order at one END)."""
    w, blob = words
    text = gpu.generate_host((2 << 20) + 99, 5 * LINE, 5, SEED, blob, LINE)
    for pats in ([b"tion", b"ment", b"ness", b"ation", b"ings"], [b"the", b"and", b"that", b"with", b"which"],
                 [b"ing", b"ed", b"ly", b"er"], list(w[:64]), [x for x in w[32:2000] if len(x) >= 4][:300] + [b"tion", b"less"]):
        _check_ac(gpu, oracle_engine, text, pats, dict())
        _check_ac(gpu, oracle_engine, text, pats, dict(count_lines=True))
        _check_ac(gpu, oracle_engine, text, pats, dict(whole_word=True, case_sensitive=False))


def test_single_literals_on_word_text(gpu, oracle_engine, words):
    w, blob = words
    text = gpu.generate_host((2 << 20) + 5, 0, 5, SEED, blob, LINE)
    for level in (abi.REF_AVX2, abi.REF_SCALAR):
        gpu.set_reference_simd(level)
        try:
            for pat in (b"the", b"q", b"e", b" ", b"tion", b"th", w[40000], w[3000], b"of the", w[100] + b" " + w[7]):
                for kw in (dict(), dict(count_lines=True), dict(whole_word=True), dict(case_sensitive=False)):
                    p = abi.Params([pat], **kw)
                    algo = gpu.mirror_select(p, len(text))
                    want = oracle_engine.call(algo, abi.Params([pat], **kw), text)
                    got = gpu.search(p, text)
                    assert got[0] == want[0] and np.array_equal(got[1], want[1]), (pat, kw, level, got[0], want[0])
        finally:
            gpu.set_reference_simd(abi.REF_AVX2)


def test_word_dictionary_device_windows_with_global_base(gpu, oracle_engine, words):
    """The device-resident API on word text in ownership windows (as bench.py's ranks issue them): eight windows with
    global_base / global_len, lists concatenated == the single-window list == the reference."""
    import torch
    w, blob = words
    n = (8 << 20)
    base = 3 * (1 << 30) + 5 * LINE  # a global offset beyond 2^31
    buf = torch.empty(n + 64, dtype=torch.uint8, device="cuda")
    gpu.generate(buf.data_ptr(), n, base, 5, SEED, blob, LINE)
    pats = wordlist.dictionary(w, "uniform")
    host = buf[:n].cpu().numpy()
    _, want = oracle_engine.call(abi.RA_AHO_CORASICK, abi.Params(pats), host)
    want = want.astype(np.int64) + base
    cap = len(want) + 4096
    pos = torch.empty(2 * cap, dtype=torch.int64, device="cuda")
    plan = gpu.plan(abi.Params(pats))
    out = plan.scan(buf.data_ptr(), n, 0, n, base, pos.data_ptr(), cap, global_len=base + n)
    assert out.stored == len(want)
    assert np.array_equal(pos[: 2 * out.stored].view(-1, 2).cpu().numpy(), want)
    parts = []
    G = 8
    for g in range(G):
        lo, hi = g * n // G, (g + 1) * n // G
        o = plan.scan(buf.data_ptr(), n, lo, hi, base, pos.data_ptr(), cap, global_len=base + n)
        parts.append(pos[: 2 * o.stored].view(-1, 2).cpu().numpy().copy())
    cat = np.concatenate(parts)
    # start ownership: the concatenation holds every record once; its order is the emission order inside a window and
    # window order across them — sort both sides by (end, start) to compare as sets with multiplicity
    key = lambda a: a[np.lexsort((a[:, 0], a[:, 1]))]
    assert np.array_equal(key(cat), key(want))
    plan.close()


def test_word_dictionary_with_short_words_is_split_and_merged(gpu, oracle_engine, words):
    """A word list that also holds 1..3-byte words (`of`, `the`, a rare three-letter word ...) gets no anchors as one dictionary; on word
    text the plan scans its >= 4-byte part anchored and its short part on its own and merges the two record lists (kg_scan_ac.hip
    scan_ac_split).  The merged list must be aho_corasick_search's, record for record: END ascending, longest first at one END
    (/root/reference/aho_corasick.c:383-437), under -i, -w and max_count; counting adds the two counts; -c (lines) keeps one scan."""
    import torch
    words, blob = words
    n = 3 * (1 << 20) + 4567
    text = gpu.generate_host(n, 0, 5, SEED, blob, LINE)
    long_part = wordlist.dictionary(words, "rare", n=300) + wordlist.dictionary(words, "common", n=40, seed=3)
    short = [w for w in words if len(w) <= 3]
    assert len(short) >= 6
    pats = long_part + short[:3] + short[-3:] + [b"of", b"th"]
    d = torch.from_numpy(np.ascontiguousarray(text)).cuda()
    for kw in (dict(), dict(case_sensitive=False), dict(whole_word=True), dict(max_count=1000), dict(max_count=3),
               dict(count_lines=True, only_match=True), dict(count_lines=True)):
        want = oracle_engine.call(abi.RA_AHO_CORASICK, abi.Params(pats, **kw), text)
        plan = gpu.plan(abi.Params(pats, **kw))
        cap = int(want[0]) + 8
        pos = torch.zeros(2 * cap, dtype=torch.int64, device="cuda")
        for rep in range(2):
            out = plan.scan(d.data_ptr(), n, 0, n, 0, pos.data_ptr(), cap)
            assert out.count == want[0], (kw, rep, out.count, want[0])
            if len(want[1]):
                got = pos[: 2 * out.stored].view(-1, 2).cpu().numpy().astype(np.uint64)
                assert np.array_equal(got, want[1]), (kw, rep, got[:6], want[1][:6])
        # (-c counts lines over ONE list: the split is never asked for, the state stays undecided)
        assert plan.split_state() == (0 if kw.get("count_lines") and not kw.get("only_match") else 2), (kw, plan.split_state())
        # ownership windows with a global base: the windows' lists concatenate to the whole list
        if not kw:
            base = (3 << 32) + 77
            parts = []
            for lo, hi in ((0, 1 << 20), (1 << 20, (2 << 20) + 17), ((2 << 20) + 17, n)):
                out = plan.scan(d.data_ptr(), n, lo, hi, base, pos.data_ptr(), cap)
                parts.append(pos[: 2 * out.stored].view(-1, 2).cpu().numpy().astype(np.uint64) - base)
            assert np.array_equal(np.concatenate(parts), want[1])
            # a list that does not fit is reported as such, with the right count
            out = plan.scan(d.data_ptr(), n, 0, n, 0, pos.data_ptr(), 1000)
            assert out.overflow and out.count == want[0]
        plan.close()
    # on i.i.d. text the long part gains nothing: one scan
    rng = np.random.RandomState(3)
    iid = cases.rand_text(rng, n, bytes(range(97, 123)) + b"  \n")
    plan = gpu.plan(abi.Params(pats))
    want = oracle_engine.call(abi.RA_AHO_CORASICK, abi.Params(pats), iid)
    di = torch.from_numpy(iid).cuda()
    cap = int(want[0]) + 8
    pos = torch.zeros(2 * cap, dtype=torch.int64, device="cuda")
    out = plan.scan(di.data_ptr(), n, 0, n, 0, pos.data_ptr(), cap)
    assert out.count == want[0] and np.array_equal(pos[: 2 * out.stored].view(-1, 2).cpu().numpy().astype(np.uint64), want[1])
    assert plan.split_state() == 1
    plan.close()


def test_count_lines_of_a_split_dictionary_on_the_merged_list(gpu, oracle_engine, words):
    """-c (distinct lines) of a word dictionary with short words, on a text large enough for the record-list road (>= 32 MiB): the two
    parts' END-owned lists are merged and the line gaps counted on the merged list (kg_scan_ac.hip scan_ac_lines_on_list); the same count
    as aho_corasick_search's count_lines_mode (/root/reference/aho_corasick.c:353-431), also in two ownership windows whose line counts
    combine (krep_gpu_combine_line_counts)."""
    import torch
    words, blob = words
    n = (40 << 20) + 1234
    text = gpu.generate_host(n, 0, 5, SEED, blob, LINE)
    pats = wordlist.dictionary(words, "rare", n=300) + [w for w in words if len(w) <= 3][:4] + [b"of"]
    d = torch.from_numpy(np.ascontiguousarray(text)).cuda()
    for kw in (dict(count_lines=True), dict(count_lines=True, whole_word=True), dict(count_lines=True, case_sensitive=False, max_count=1000)):
        want = oracle_engine.call(abi.RA_AHO_CORASICK, abi.Params(pats, **kw), text)[0]
        plan = gpu.plan(abi.Params(pats, **kw))
        for rep in range(2):
            out = plan.scan(d.data_ptr(), n)
            assert out.count == want, (kw, rep, out.count, want)
        assert plan.split_state() == 2, (kw, plan.split_state())
        if "max_count" not in kw:
            cut = (17 << 20) + 40  # (inside a line)
            outs = [plan.scan(d.data_ptr(), n, 0, cut), plan.scan(d.data_ptr(), n, cut, n)]
            assert gpu.lib.krep_gpu_combine_line_counts((abi.ScanOut * 2)(*outs), 2) == want
        plan.close()


def test_split_scan_falls_back_when_the_merged_list_is_too_long():
    """A merged list beyond 2^28 records (a dense short part), or one whose sort finds no room, sends the plan back to ONE scan of the whole
    dictionary — same records.  The limit is read at library load: a child process with $KREP_GPU_AC_SPLIT_MAX=1000."""
    import os, subprocess, sys
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(here, "_split_fallback_child.py")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "split fallback ok [1, 2]" in r.stdout, (r.stdout[-400:], r.stderr[-800:])
