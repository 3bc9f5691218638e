"""What `krep -m N [-o | -c] PATTERN` prints for every file of a batch (krep_gpu_grep_batch with the max_count switch on), without a
device: the expected bytes are batch_grep_model.definition() fed per item with the grep-side cut of the item's unlimited record list
(batch_cut_model.grep_cut: the function's list cut to N, put in (start, end) order), and they are pinned to the stock CLI run once per
file with -m N (never -r) — default, -o and -c, plain and --color=always.  Where the CLI cannot be built the digests of its answers
in tests/golden/batch_grep_max_count.json stand in."""
import contextlib
import os

import numpy as np
import pytest

import batch_cut_model as cm
import batch_grep_model as bg
import batch_model as bm
import line_model as lm
import oracle_lib as ol
import regex_ref
from test_batch_grep_model_cpu import classes, names_for, random_batch

CLI = ol.ref_cli()
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "batch_grep_max_count.json")
MS = [1, 2, 10, 11]


@contextlib.contextmanager
def _own_file():
    keep, lm.GOLDEN = lm.GOLDEN, GOLDEN
    try:
        yield
    finally:
        lm.GOLDEN = keep


class Store(lm.Store):
    """line_model.Store over tests/golden/batch_grep_max_count.json"""

    def __init__(self):
        with _own_file():
            super().__init__()

    def want(self, key, live=None) -> str:
        with _own_file():
            return super().want(key, live)

    def save(self):
        with _own_file():
            super().save()


STORE = Store()


@pytest.fixture(autouse=True, scope="module")
def _c_locale():
    with regex_ref.c_locale():
        yield


@pytest.fixture(scope="module")
def eng():
    import krep_amd
    e = krep_amd.load()
    yield e
    e.set_thread_config(None)


def plain(s):
    kw = {k: v for k, v in s.kw.items() if k != "count_lines"}
    return bm.Search(s.name, s.pats, s.level, s.only_matching, s.regex, s.alphabet, s.plants, s.algo_override, s.force_no_simd, **kw)


def cut_answers(eng, s, items, M):
    """per item (count, records) as search_file() hands them to its formatter under -m M"""
    algo = cm.algo_of(eng, plain(s))
    counts, recs = [], []
    for it in items:
        R = np.asarray(bm.reference(eng, plain(s), it)[1], dtype=np.uint64).reshape(-1, 2)
        c, r = cm.grep_cut(algo, s.kw, R, cm.distinct_lines(it, R), M)
        counts.append(int(c))
        recs.append(r)
    return counts, recs


def stale_item(before, after):
    """`before` matches of 'ab' in front of the last newline, `after` behind it"""
    return np.frombuffer(b"ab x\n" * before + b"ab " * after, dtype=np.uint8).copy()


def cli_batches():
    out = []
    for mode in bg.MODES:
        for ci, s in enumerate(classes(mode)):
            rng = np.random.RandomState(100 + ci)
            items = random_batch(rng, s) + [bm.random_item(rng, s, 300)]
            for M in MS:
                out.append(("%s/%s/m%d" % (mode, s.name, M), s, mode, items, M))
    # -o: more than 10 records before the cut and at most 10 after it (true numbers), and more than 10 after it (stale numbers)
    s = classes("matches")[0]
    for M in (10, 11, 12):
        out.append(("matches/stale/m%d" % M, s, "matches", [stale_item(20, 10), stale_item(9, 6), stale_item(3, 2)], M))
    return out


def test_the_cut_definition_matches_the_cli_with_m_once_per_file(eng, tmp_path):
    batches = cli_batches()
    assert len(batches) >= 3 * 6 * len(MS)
    shorter = 0
    for idx, (key, s, mode, items, M) in enumerate(batches):
        counts, recs = cut_answers(eng, s, items, M)
        free = [bm.reference(eng, plain(s), it)[1].reshape(-1, 2).shape[0] for it in items]
        shorter += sum(r.shape[0] < f for r, f in zip(recs, free))
        assert all(r.shape[0] <= M for r in recs) and all(c <= M for c in counts)
        short = names_for(len(items))
        paths = []
        for k, it in enumerate(items):
            (tmp_path / f"b{idx}" / f"i{k}").mkdir(parents=True)
            p = tmp_path / f"b{idx}" / f"i{k}" / short[k].decode()
            p.write_bytes(bm.as_array(it).tobytes())
            paths.append(p)
        for color in (False, True):
            mine_short, _ = bg.definition(items, recs, short, mode, color, counts)
            live = None
            if CLI:
                import subprocess
                full = [str(p).encode() for p in paths]
                mine, _ = bg.definition(items, recs, full, mode, color, counts)
                out = b"".join(subprocess.run([CLI, "-m", str(M)] + bg.cli_args(s, mode, color) + [str(p)], capture_output=True,
                                              timeout=120).stdout for p in paths)
                assert out == mine, (key, color, M, out[:300], mine[:300])
                for f, sh in zip(full, short):
                    out = out.replace(f, sh)
                live = bg.digest(0, out)
            assert bg.digest(0, mine_short) == STORE.want(key + ("/color" if color else ""), live), key
    assert shorter > 50  # the cut did cut
    STORE.save()


def test_the_stale_rule_sees_the_cut_count():
    """an item with 30 matches, some behind its last newline: at -m 10 every number is true, at -m 11 the rule is on"""
    import only_matching_model as omm
    it = stale_item(8, 22)
    text = it.tobytes()
    R = np.array([(k, k + 2) for k in range(len(text) - 1) if text[k:k + 2] == b"ab"], dtype=np.uint64)
    assert R.shape[0] == 30
    ten = omm.grep_o_output(text, [tuple(map(int, r)) for r in R[:10]], b"f", False)
    eleven = omm.grep_o_output(text, [tuple(map(int, r)) for r in R[:11]], b"f", False)
    assert ten.splitlines()[-1].startswith(b"f:9:") and eleven.splitlines()[-1].startswith(b"f:8:")
