"""The generated cases of tests/regex_generated_cases.py, without a device: whether the list is good enough to run on one
(test_gpu_regex_generated.py).  What the host compilers take of it covers 5..8 and 9..12 jump pairs with anchors and with -i, 29..32
positions, position 31, loops programs of more than 24 places; at most a quarter of the wide draws is refused, each for a known
reason; the compiled reference finds the planted witnesses on short and inside long lines; and on every case the models give the
reference's records and -c count: regex_groups_model / regex_loops_model on the short lines, regex_long_lines_model on the long ones."""
import collections

import numpy as np
import pytest

import regex_generated_cases as gc
import regex_ref


@pytest.fixture(autouse=True, scope="module")
def _c_locale():
    with regex_ref.c_locale():
        yield


@pytest.fixture(scope="module")
def cases():
    assert regex_ref.available(), "the compiled reference (oracle/_ref/libkrep_ref_avx2.so) is missing"
    return gc.cases()


def test_what_the_compilers_take_covers_the_jump_pairs_the_positions_and_the_places(cases, capsys):
    groups, loops = gc.taken("groups"), gc.taken("loops")
    hist = collections.Counter(c.pairs for c in groups)
    with capsys.disabled():
        print("\n[generated -E cases] groups taken: %d, jump pairs 0..12: %s; 29..32 positions: %d; loops taken: %d, of more than 24 places: %d"
              % (len(groups), [hist[k] for k in range(13)], sum(29 <= c.n_pos <= 32 for c in groups), len(loops), sum(c.places > 24 for c in loops)))
    assert len(cases["groups"]) == gc.DRAWN["groups"] and len(cases["loops"]) == gc.DRAWN["loops"]
    assert all(c.pairs <= 12 and c.n_pos <= 32 for c in groups) and max(hist) == 12 and min(hist) == 0
    for lo, hi in ((5, 8), (9, 12)):
        some = [c for c in groups if lo <= c.pairs <= hi]
        assert len(some) >= 40, (lo, hi, len(some))
        assert sum(c.anchored for c in some) >= 10 and sum(not c.cs for c in some) >= 10, (lo, hi, sum(c.anchored for c in some), sum(not c.cs for c in some))
    assert sum(29 <= c.n_pos <= 32 for c in groups) >= 10 and any(c.top == 31 for c in groups)
    # the loops compiler takes every loops case (the generators draw what its limits admit): none is left out
    assert len(loops) == gc.DRAWN["loops"], [c.reason for c in cases["loops"] if not c.taken]
    assert sum(c.places > 24 for c in loops) >= 10 and sum(c.places > 24 and c.branches >= 5 for c in loops) >= 10
    assert all(c.places <= 32 and c.branches <= 8 for c in loops)
    assert sum(not c.cs for c in loops) >= 10 and sum(c.anchored for c in loops) >= 10


def test_at_most_a_quarter_of_the_wide_draws_is_refused_each_for_a_known_reason(cases):
    for flavours in (("narrow",), ("wide", "full")):
        drawn = [c for c in cases["groups"] if c.flavour in flavours]
        refused = [c for c in drawn if not c.taken]
        assert 4 * len(refused) <= len(drawn), (flavours, len(refused), len(drawn))
        for c in refused:
            assert any(w in c.reason for w in gc.REASONS) and gc.OLDER not in c.reason, (c.label(), c.reason)
    assert cases["older"] > 0  # expressions an older compiler takes were met, and drawn again


def test_the_case_list_is_a_pure_function_of_the_module(cases):
    """drawn again from the same seed: the same expressions and the same texts"""
    again, _ = gc._draw(gc.krep_amd.load(), "groups", "full", lambda rng: gc.wide_groups_case(rng, 29), gc.SEED_FULL, gc.N_FULL)
    first = [c for c in cases["groups"] if c.flavour == "full"]
    assert [(c.pats, c.cs, c.taken) for c in again] == [(c.pats, c.cs, c.taken) for c in first]
    assert all(np.array_equal(a.text, b.text) and a.long_spans == b.long_spans for a, b in zip(again, first) if a.taken)


def test_the_texts_are_as_described(cases):
    for c in gc.taken("groups") + gc.taken("loops"):
        spans = gc.lm.line_spans(c.text)
        lengths = sorted(b - a for a, b in spans)
        assert lengths[-2] == gc.LONG + 1 and 4800 <= lengths[-1] < 5300 and lengths[-3] <= 60, (c.label(), lengths[-3:])
        assert 40 <= len(spans) <= 43 and 9000 < c.text.size < 13000, (c.label(), len(spans), c.text.size)
        assert set(np.unique(c.text).tolist()) - {10} <= set(range(1, 256)), c.label()
    ends = collections.Counter((c.long_spans[0][0] == 0, c.long_spans[1][1] >= c.text.size - 1, c.text[-1] == 10) for c in gc.taken("groups"))
    assert sum(v for k, v in ends.items() if k[0]) > 20 and sum(v for k, v in ends.items() if k[1]) > 20  # a long line first, last
    assert sum(v for k, v in ends.items() if k[2]) > 50 and sum(v for k, v in ends.items() if not k[2]) > 50  # closed, open


def test_the_reference_finds_matches_on_short_and_inside_long_lines(cases):
    """the witnesses do their work: for at least 9 cases of 10 the compiled reference alone finds a match on a short line and one
    inside a long line"""
    for kind in ("groups", "loops"):
        both = 0
        for c in gc.taken(kind):
            inside = gc.in_long_lines(c, gc.ref_answer(c)[1])
            both += bool(inside.any() and (~inside).any())
        assert 10 * both >= 9 * len(gc.taken(kind)), (kind, both, len(gc.taken(kind)))


def agree(c):
    want, want_c = gc.ref_answer(c), gc.ref_answer(c, count_lines=True)
    records, lines = gc.model_answer(c)
    assert want[0] == records.shape[0] and np.array_equal(want[1], records), "%s: the model against the reference: %s" % (
        c.label(), gc.first_difference(records, want[1]))
    assert want_c[0] == lines, "%s: -c: the model %d, the reference %d" % (c.label(), lines, want_c[0])


def test_the_seam_case_matches_no_line_that_is_one_sequence_behind_another():
    c = gc.seam_case()
    assert (c.branches, c.places) == (3, 6) and len(c.long_spans) == 7
    agree(c)
    want = gc.ref_answer(c)
    assert want[0] == gc.ref_answer(c, count_lines=True)[0] == 6 and int(gc.in_long_lines(c, want[1]).sum()) == 3
    assert c.text[-1] != 10 and want[1][-1, 1] < c.long_spans[-1][0]  # the open last line is a seam: no match


@pytest.mark.parametrize("k", range(gc.n_chunks("groups")))
def test_the_models_give_the_reference_records_on_every_groups_case(cases, k):
    for c in gc.chunk("groups", k):
        agree(c)


@pytest.mark.parametrize("k", range(gc.n_chunks("loops")))
def test_the_models_give_the_reference_records_on_every_loops_case(cases, k):
    for c in gc.chunk("loops", k):
        agree(c)
