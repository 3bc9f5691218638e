"""The texts tests/test_gpu_regex.py puts to the anchor path of the regex scan hold what they are built for (regex_skip_model.py):
conditions on the builder, checked from the text alone, so that a change to it that loses a straddler or a decoy fails here,
without a GPU."""
import numpy as np
import pytest

import regex_model
import regex_ref
import regex_skip_model as sm


@pytest.fixture(autouse=True, scope="module")
def _c_locale():
    """the classes come from libc in the locale krep runs in"""
    with regex_ref.c_locale():
        yield


def test_anchor_rule_and_skip_rule():
    """the first smallest class, bytes only for 1..4; a cell is skipped iff neither it nor the cell in front holds an anchor byte and it
    does not start a unit"""
    for pat, cs, want_index, want_bytes in ((b"[0-9]{3}-[0-9]{4}", True, 3, b"-"), (b"[0-9]{4}k", False, 4, b"Kk"),
                                            (b"[a-f]{15}[#%&@]", True, 15, b"#%&@"), (b"ab", True, 0, b"a"), (b"[a-e]{2}", True, 0, b""),
                                            (b"[ab][cd]", True, 0, b"ab")):
        ai, ab = sm.anchor(regex_model.classes(pat, cs))
        assert (ai, ab.tobytes()) == (want_index, want_bytes), pat
    cl = regex_model.classes(b"[a-f]Z")
    text = np.full(40 * sm.CELL, ord("g"), dtype=np.uint8)
    for c in (5, 6, 9, 33):
        text[c * sm.CELL + 7] = ord("Z")
    g = sm.Geometry(cl, text)
    walked = {0, 5, 6, 7, 9, 10, 32, 33, 34}
    assert set(np.flatnonzero(~g.skipped).tolist()) == walked and g.rebuilt().tolist() == [5, 9]  # (33 stands behind the first cell of a unit, which is walked)
    # another origin: own_lo & ~15, the units counted from there
    g = sm.Geometry(cl, text, own_lo=3 * sm.CELL + 21, own_hi=39 * sm.CELL)
    assert g.origin == 3 * sm.CELL + 16 and g.n_cells == 36
    assert set(np.flatnonzero(~g.skipped).tolist()) == {0, 1, 2, 3, 5, 6, 29, 30, 32}  # (cell 32 starts the second unit)
    # a pattern without anchor bytes skips nothing
    assert not sm.Geometry(regex_model.classes(b"[a-e]{2}"), text).skipped.any()


@pytest.mark.parametrize("case", range(len(sm.PATTERNS)))
def test_built_text_holds_every_plant(case):
    pat, cs = sm.PATTERNS[case]
    cl = regex_model.classes(pat, cs)
    text, plants = sm.build_text(cl)
    assert text.size == sm.TEXT_LEN == 3 * sm.UNIT + sm.ROUND + 300
    al = sm.background_alphabet(cl)
    ai, ab = sm.anchor(cl)
    assert al and not any(t[b] for t in cl for b in al) and ai >= 1 and ab.size in (1, 2, 4)
    assert sm.missing(cl, text) == []
    # every anchor byte is in use
    g = sm.Geometry(cl, text)
    assert {int(text[s + ai]) for s in g.occ.tolist()} == set(ab.tolist())
    # the model of a right rebuild reports the occurrences; every wrong one reports something else, and what gives it away is a plant:
    # a lost straddler (zero, lane 62's bytes, stale) or a reported decoy (0xFFFF, stale)
    assert np.array_equal(g.kernel_hits(), g.occ) and len(g.dependent()) >= ai
    dep = {s for s, _, _ in g.dependent()}
    decoys = {p.start for p in plants if p.kind == "decoy"}
    for fault in sm.FAULTS:
        got = set(g.kernel_hits(fault).tolist())
        lost, extra = set(g.occ.tolist()) - got, got - set(g.occ.tolist())
        assert lost <= dep
        if fault in ("zero", "lane62", "stale"):
            assert lost == dep, fault
        if fault in ("ones", "stale"):
            assert decoys <= extra, fault
    # ... and each kind of plant is needed: without it a condition fails
    for kind, word in (("straddler", "dependent"), ("unit", "unit boundary"), ("decoy", "suffix decoy"), ("prefixes", "prefix decoy"),
                       ("edge", "byte 0")):
        less, _ = sm.build_text(cl, omit=(kind,))
        assert any(word in m for m in sm.missing(cl, less)), kind


def test_built_text_of_several_units():
    """the text of the starved-grid test: dependent occurrences in every unit but the short last one"""
    cl = regex_model.classes(b"[a-f]{7}S")
    n = 13 * sm.UNIT + 100
    text, _ = sm.build_text(cl, n=n, seed=3)
    g = sm.Geometry(cl, text)
    assert g.n_cells == 13 * sm.CELLS_PER_UNIT + 1
    assert {c // sm.CELLS_PER_UNIT for _, c, _ in g.dependent()} == set(range(13))
    assert all(g.skipped[u * sm.CELLS_PER_UNIT:(u + 1) * sm.CELLS_PER_UNIT].sum() >= 8 for u in range(13))
