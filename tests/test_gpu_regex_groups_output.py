"""Groups plans (krep -E with repeated and nested groups; krep_gpu_set_regex_groups) through the output drivers: Plan.grep_lines and
Plan.grep_only_matching, plain and coloured, on a 64-KiB text, byte for byte against the output models on the records of the compiled
reference, and Engine.grep_batch in its three modes over three items.  The module turns the switches on and, whatever happens, off
again."""
import numpy as np
import pytest

import batch_grep_model as bg
import batch_model as bm
import regex_output_cases as rc
import regex_ref
from krep_amd import abi
from test_gpu_regex_groups import SHAPES
from test_gpu_regex_loops import AUTO, expected, planted, rx

pytestmark = pytest.mark.gpu

NAME = b"f.txt"
ROWS = [1, 6]  # (a|bc)+d and the IP expression


@pytest.fixture(autouse=True, scope="module")
def _c_locale():
    with regex_ref.c_locale():
        yield


@pytest.fixture(scope="module")
def gpu():
    import krep_amd
    e = krep_amd.load()
    assert e.device_count() >= 1 and e.available(), e.unavailable_reason()
    assert regex_ref.available(), "the compiled reference (oracle/_ref/libkrep_ref_avx2.so) is missing"
    e.set_regex_loops(True)
    e.set_regex_groups(True)
    try:
        yield e
    finally:
        e.set_regex_groups(False)
        e.set_regex_loops(False)
        e.force_regex_loops_road(AUTO)
        e.set_thread_config(None)


@pytest.mark.parametrize("row", ROWS)
def test_grep_lines_and_only_matching_plain_and_coloured(gpu, row):
    import torch
    pats, alphabet, plants, decoys = SHAPES[row]
    text = planted(np.random.RandomState(600 + row), 65536, alphabet, plants, decoys)
    raw = text.tobytes()
    rec = [(int(s), int(e)) for s, e in expected(pats, text)[1]]
    assert len(rec) > 30
    d = torch.from_numpy(text.copy()).cuda()
    plan, plan_o = gpu.plan(rx(pats)), gpu.plan(rx(pats), only_matching=True)
    try:
        assert plan.longest_match() == 4097 and plan.is_loops()
        for mode in rc.MODES:
            for filename in (NAME, None):
                for mc in (None, 7):
                    color = mode.endswith("color")
                    if mode.startswith("o"):
                        got = plan_o.grep_only_matching(d.data_ptr(), text.size, filename=filename, max_count=mc, color=color)
                    else:
                        got = plan.grep_lines(d.data_ptr(), text.size, filename=filename, max_count=mc, color=color)
                    want = rc.expected(raw, rec, mode, filename, mc)
                    assert got == want, (pats, mode, filename, mc, len(got), len(want))
                    assert want
    finally:
        plan.close()
        plan_o.close()


@pytest.mark.parametrize("mode", ["lines", "matches", "count"])
def test_grep_batch_over_three_items(gpu, mode):
    pats, alphabet, plants, decoys = SHAPES[1]
    rng = np.random.RandomState(700)
    items = [planted(rng, 3000, alphabet, plants, decoys), np.zeros(0, dtype=np.uint8), np.frombuffer(b"xx\nbcad bcd\nad", dtype=np.uint8)]
    names = [b"one", b"two", b"three"]
    s = bm.Search("(a|bc)+d", pats, only_matching=(mode == "matches"), regex=True, alphabet=alphabet)
    if mode == "count":
        s = s.with_lines()
    assert gpu.batch_can_accelerate(s.params()), gpu.last_error()
    recs = [np.asarray(bm.reference(gpu, bm.Search("r", pats, regex=True), it)[1], dtype=np.uint64).reshape(-1, 2) for it in items]
    counts = [int(bm.reference(gpu, s, it)[0]) for it in items] if mode == "count" else None
    assert recs[0].shape[0] > 5 and recs[1].shape[0] == 0 and recs[2].tolist() == [[3, 7], [8, 11], [12, 14]]
    for color in (False, True):
        want, where = bg.definition(items, [bm.NONE] * 3 if mode == "count" else recs, names, mode, color, counts)
        got, per, info = gpu.grep_batch(s.params(), items, names, color=color, cfg=s.config(gpu), want_info=True)
        assert got == want, (mode, color, len(got), len(want))
        assert [(o, n) for _, o, n in per] == where
        assert [c for c, _, _ in per] == (counts if counts is not None else [r.shape[0] for r in recs])
