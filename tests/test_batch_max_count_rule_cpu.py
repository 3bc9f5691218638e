"""The batch's max_count cut against the reference itself (include/krep_gpu.h "max_count behind a switch").  No GPU.

krep_gpu_search_batch scans a pack WITHOUT a limit and cuts every item's list on the device by the rule batch_cut_model.cut() restates.
That is exact iff, for every class the batch takes, the reference function's answer on an item alone under max_count is that
function of its answer on the item alone without one — and iff the same holds for an item's share of a pack's unlimited list.  Both
are asked here of the compiled reference (the restatement where it is not built), for every batchable class of the two existing
matrices (the named classes of test_batch_separable_cpu.py, the literal matrix of test_batch_rule_sweep_cpu.py with its -c bit left
to the variants below), max_count in MS, and the four combinations of -c and track_positions.  A (class, variant, max_count) the
rule refuses with the switch on is not asked (it names its reason); everything else is."""
import numpy as np
import pytest

import batch_cut_model as cm
import batch_model as bm
import oracle_lib as ol
import regex_ref
from krep_amd import abi
from test_batch_rule_sweep_cpu import LENGTHS, LEVELS, OVERRIDES, literal_search, seed_of, shapes, length
from test_batch_separable_cpu import TAKEN

MS = [0, 1, 2, 3, 10, 11, 4096, 8192]
VARIANTS = [dict(), dict(track_positions=False), dict(count_lines=True), dict(count_lines=True, track_positions=True)]
PAIRS = 25


@pytest.fixture(autouse=True, scope="module")
def _c_locale():
    with regex_ref.c_locale():
        yield


@pytest.fixture(scope="module")
def eng():
    import krep_amd
    mp = pytest.MonkeyPatch()
    mp.setenv("KREP_GPU_ASSUME_AVAILABLE", "1")  # (the rule is host logic)
    mp.delenv("KREP_GPU_DISABLE", raising=False)
    e = krep_amd.load()
    e.set_batch_max_count(True)
    yield e
    e.set_batch_max_count(False)
    e.set_thread_config(None)
    mp.undo()


def variant(s, extra, max_count=None):
    kw = {k: v for k, v in s.kw.items() if k not in ("count_lines", "track_positions", "max_count")}
    kw.update(extra)
    if max_count is not None:
        kw["max_count"] = max_count
    return bm.Search(s.name + " %r m=%r" % (sorted(extra), max_count), s.pats, s.level, s.only_matching, s.regex, s.alphabet, s.plants,
                     s.algo_override, s.force_no_simd, **kw)


def taken(eng, s):
    s.configure(eng)
    try:
        return eng.batch_can_accelerate(s.params()), eng.last_error()
    finally:
        eng.set_thread_config(None)


@pytest.fixture(scope="module")
def classes(eng):
    """the base classes (no -c, no max_count): the named ones, then the literal matrix's distinct (function, pattern, flags)"""
    out, seen = [], set()
    for s in TAKEN:
        if not s.kw.get("count_lines"):
            out.append(s)
    for m in LENGTHS:
        for pat in shapes(m):
            for flags in range(8):
                cs, ww, om = bool(flags & 1), bool(flags & 2), bool(flags & 4)
                for level in LEVELS:
                    for override in OVERRIDES:
                        for nosimd in (False, True):
                            s = literal_search(pat, level, override, nosimd, cs, ww, om, False)
                            if not taken(eng, s)[0]:
                                continue
                            key = (cm.algo_of(eng, s), pat, cs, ww, om)
                            if key not in seen:
                                seen.add(key)
                                out.append(s)
    assert len(out) > 250
    return out


def unit_of(eng, base):
    """a piece of text that holds exactly one record of the class and ends its line: k copies hold k records on k lines"""
    for u in [base.pats[0]] + list(base.plants) + [b"a", b"ab", b"color"]:
        for sep in (b"\n", b" \n"):
            c, p = bm.reference(eng, base, (u + sep) * 3)
            if c == 3 and p.reshape(-1, 2).shape[0] == 3:
                return u + sep
    return None


def regimes(T, M):
    r = set()
    if T == 0:
        r.add("T=0")
    if T < M:
        r.add("T<M")
    if T == M:
        r.add("T=M")
    if T == M + 1:
        r.add("T=M+1")
    if T >= 2 * M + 2:
        r.add("T>>M")
    return r


def check_item(eng, base, algo, item, R, M, where):
    """reference(item, M) == cut(reference(item, unlimited)) for the four variants -> variants asked"""
    asked = 0
    Ln = cm.distinct_lines(item, R)
    for extra in VARIANTS:
        s = variant(base, extra, M)
        ok, why = taken(eng, s)
        if not ok:
            assert why and "follow-up work" not in why, (s, why)
            continue
        got_c, got_p = bm.reference(eng, s, item)
        want_c, want_p = cm.cut(algo, s.kw, R, Ln, M)
        assert got_c == want_c, (s, where, M, extra, got_c, want_c, R.shape[0], Ln, bytes(item[:80]))
        assert np.array_equal(got_p.reshape(-1, 2), want_p.reshape(-1, 2)), (s, where, M, extra, R.shape[0])
        asked += 1
    return asked


def test_an_item_alone_under_max_count_is_the_cut_of_its_unlimited_list(eng, classes):
    asked = 0
    for base in classes:
        algo = cm.algo_of(eng, base)
        unit = unit_of(eng, base)
        assert unit is not None, base
        rng = np.random.RandomState(seed_of("cut", base.name))
        made = {}
        for M in MS:
            seen = set()
            for T in sorted({0, max(M - 1, 0), M, M + 1, 3 * M + 2}):
                if T not in made:
                    item = bm.as_array(unit * T)
                    made[T] = (item, bm.reference(eng, variant(base, {}), item)[1].reshape(-1, 2))
                item, R = made[T]
                assert R.shape[0] == T, (base, T, R.shape[0])
                seen |= regimes(T, M)
                asked += check_item(eng, base, algo, item, R, M, "built T=%d" % T)
            # ... and a random item of the class's own alphabet: several records on a line, records at both edges
            item = bm.random_item(rng, base, int(rng.randint(0, 400)))
            R = bm.reference(eng, variant(base, {}), item)[1].reshape(-1, 2)
            seen |= regimes(R.shape[0], M)
            asked += check_item(eng, base, algo, item, R, M, "random")
            want = {"T=0", "T=M+1", "T>>M"} if M == 0 else {"T=0", "T<M", "T=M", "T=M+1", "T>>M"}
            assert want <= seen, (base, M, seen)
    print("classes %d, (item, variant, max_count) cells asked %d" % (len(classes), asked))
    assert asked > 20 * len(classes)
    assert ol.checker().restatement_budget_ok()


def test_an_items_share_of_a_packs_unlimited_list_cut_is_the_item_alone_under_max_count(eng, classes):
    asked = 0
    for base in classes:
        algo = cm.algo_of(eng, base)
        rng = np.random.RandomState(seed_of("pack cut", base.name))
        free = variant(base, {})
        for k in range(PAIRS):
            M = MS[k % len(MS)] if MS[k % len(MS)] < 4096 else int(rng.randint(1, 6))
            A, B = bm.random_item(rng, base, length(rng, 300)), bm.random_item(rng, base, length(rng, 300))
            shares = bm.split(bm.reference(eng, free, bm.pack([A, B])[0])[1].reshape(-1, 2), [A, B])
            for item, R in zip((A, B), shares):
                asked += check_item(eng, base, algo, item, R, M, "pack pair %d" % k)
    print("cells asked through a pack %d" % asked)
    assert asked > 100 * len(classes)
    assert ol.checker().restatement_budget_ok()


def test_the_grep_side_cut_is_search_files_cap(eng):
    """search_file() caps the count and the list at max_count behind the function: kmp_search's extra record and the count-only 1 go"""
    R = np.array([[0, 4], [5, 9], [10, 14], [15, 19], [20, 24]], dtype=np.uint64)
    assert cm.cut(abi.RA_KMP, {}, R, 5, 3)[1].shape[0] == 4
    c, p = cm.grep_cut(abi.RA_KMP, {}, R, 5, 3)
    assert c == 3 and np.array_equal(p, R[:3])
    assert cm.cut(abi.RA_BMH, dict(track_positions=False), R, 5, 0)[0] == 1 and cm.grep_cut(abi.RA_BMH, dict(track_positions=False), R, 5, 0)[0] == 0
    big = np.stack([np.arange(0, 24000, 2), np.arange(1, 24001, 2)], axis=1).astype(np.uint64)
    c, p = cm.cut(abi.RA_MEMCHR, {}, big, 1, 4096)
    assert c == 4096 and np.array_equal(p[0], big[4096]) and np.array_equal(p[1:], big[:4095])
    c, p = cm.grep_cut(abi.RA_MEMCHR, {}, big, 1, 8192)
    assert c == 8192 and np.array_equal(p[:8191], big[:8191]) and np.array_equal(p[8191], big[8192])
