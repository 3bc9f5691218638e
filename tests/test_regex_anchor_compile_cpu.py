"""krep_gpu_regex_compile_anchored (host only): the anchors and the real classes of every accepted shape, the self-overlap rule with
anchors, every new refusal with its reason, krep_gpu_regex_compile() unchanged, and what the selectors and the split rule say."""
import ctypes as C

import pytest

import krep_amd
import regex_anchor_model as am
import regex_model
import regex_ref
from krep_amd import abi
from krep_amd.engine import KrepGpuError


@pytest.fixture(autouse=True, scope="module")
def _c_locale():
    """the reference runs in the C locale (it never calls setlocale()); Python's start-up put the process into the environment's"""
    with regex_ref.c_locale():
        yield


@pytest.fixture(scope="module")
def eng():
    return krep_amd.load()


def rx(pat, **kw):
    return abi.Params([pat], regex=True, **kw)


# pattern -> (bol, eol, the atoms between the anchors with their repetitions, self_overlap)
ACCEPTED = [
    (b"^a", 1, 0, [b"a"], 0), (b"a$", 0, 1, [b"a"], 0), (b"^a$", 1, 1, [b"a"], 0),
    (b"^Sherl[oO]ck", 1, 0, [b"S", b"h", b"e", b"r", b"l", b"[oO]", b"c", b"k"], 0),
    (b"[0-9]{3}$", 0, 1, [b"[0-9]"] * 3, 0),      # without the anchor it overlaps itself; no [0-9] is a newline
    (b"^[[:space:]]", 1, 0, [b"[[:space:]]"], 0),
    (b"\\^a", 0, 0, [b"\\^", b"a"], 0), (b"a\\$", 0, 0, [b"a", b"\\$"], 0), (b"[$^]", 0, 0, [b"[$^]"], 0),
    (b"^a{15}", 1, 0, [b"a"] * 15, 0), (b"^a{14}$", 1, 1, [b"a"] * 14, 0),
    (b"^ab", 1, 0, [b"a", b"b"], 0), (b"ab$", 0, 1, [b"a", b"b"], 0),
    (b"^[a\n]{2}", 1, 0, [b"[a\n]"] * 2, 1), (b"^[ab]{2}", 1, 0, [b"[ab]"] * 2, 0),
    (b"[a\n]{2}$", 0, 1, [b"[a\n]"] * 2, 1), (b"^[a\n]{3}$", 1, 1, [b"[a\n]"] * 3, 1),
    (b"^[a\n]b[a\n]", 1, 0, [b"[a\n]", b"b", b"[a\n]"], 0),  # shift 2 meets, but C1 = b is no newline
    (b"\\$$", 0, 1, [b"\\$"], 0), (b"[\\]$", 0, 1, [b"[\\]"], 0), (b"^[^a]", 1, 0, [b"[^a]"], 0),
]


@pytest.mark.parametrize("cs", [True, False])
def test_anchors_classes_and_overlap(eng, cs):
    for pat, bol, eol, atoms, ov in ACCEPTED:
        info = eng.regex_compile_anchored(rx(pat, case_sensitive=cs))
        assert (info.bol, info.eol, info.seq.L) == (bol, eol, len(atoms)), pat
        for j, atom in enumerate(atoms):
            assert info.seq.class_bytes(j) == regex_ref.probe_class(atom, cs), (pat, j)
        assert info.seq.self_overlap == ov, pat
        # the helper the GPU tests lean on says the same
        mb, core, me = am.split(pat)
        cl = regex_model.classes(core, cs)
        assert (mb, me, len(cl)) == (bool(bol), bool(eol), info.seq.L) and am.self_overlap(cl, mb, me) == bool(ov), pat


def test_the_anchor_byte_comes_from_the_real_classes(eng):
    info = eng.regex_compile_anchored(rx(b"^Sherl[oO]ck$"))
    assert (info.seq.anchor, info.seq.n_anchor, bytes(info.seq.anchor_bytes[:1])) == (0, 1, b"S")
    info = eng.regex_compile_anchored(rx(b"^[0-9]{3}-[0-9]{4}"))
    assert (info.seq.L, info.seq.anchor, info.seq.n_anchor, bytes(info.seq.anchor_bytes[:1])) == (8, 3, 1, b"-")
    assert eng.regex_compile_anchored(rx(b"^[A-Z][a-z]{7}$")).seq.n_anchor == 0


def test_unanchored_patterns_compile_to_the_same_fields(eng):
    for pat in (b"Sherl[oO]ck", b"[0-9]{3}-[0-9]{4}", b"[ab]{3}", b"a{16}", b".[^a]", b"[[:space:]]a"):
        for cs in (True, False):
            old, new = eng.regex_compile(rx(pat, case_sensitive=cs)), eng.regex_compile_anchored(rx(pat, case_sensitive=cs))
            assert (new.bol, new.eol) == (0, 0)
            assert bytes(C.string_at(C.addressof(old), C.sizeof(old))) == bytes(C.string_at(C.addressof(new.seq), C.sizeof(old))), pat


NEW_REFUSALS = [(b"^a{16}", "16"), (b"^a{15}$", "16"), (b"a^b", "not the first"), (b"a$b", "not the last"), (b"^^a", "not the first"),
                (b"a$$", "not the last"), (b"^$", "empty"), (b"^", "empty"), (b"$", "empty"), (b"^{2}a", "behind \\^"),
                (b"^a|b", "automaton"), (b"^(a)", "automaton")]


def test_new_refusals_carry_a_reason(eng):
    reasons = {}
    for pat, word in NEW_REFUSALS:
        with pytest.raises(KrepGpuError, match=word) as e:
            eng.regex_compile_anchored(rx(pat))
        assert len(str(e.value)) > 8, pat
        reasons[pat] = str(e.value)
    # each kind its own
    assert len({reasons[p] for p in (b"^a{16}", b"a^b", b"^$", b"^{2}a", b"^a|b")}) == 5
    # what was refused stays refused, anchored or not
    for pat in (b"^a.*b", b"a+$", b"^a{2,3}", b"^\\bword", b"^caf\xe9", b"^[ab", b"^a{0}", b"^a\\", b"", b"a{17}"):
        with pytest.raises(KrepGpuError):
            eng.regex_compile_anchored(rx(pat))
    with pytest.raises(KrepGpuError, match="alternation"):
        eng.regex_compile_anchored(abi.Params([b"^ab", b"cd"], regex=True))
    with pytest.raises(KrepGpuError, match="-w"):
        eng.regex_compile_anchored(rx(b"^ab", whole_word=True))


def test_the_old_compiler_accepts_what_it_accepted(eng):
    for pat in (b"^a", b"a$", b"^a$", b"^Sherl[oO]ck"):
        with pytest.raises(KrepGpuError, match="krep_gpu_regex_compile_anchored"):
            eng.regex_compile(rx(pat))
    for pat in (b"a^b", b"a$b", b"^", b"$", b"^$"):
        with pytest.raises(KrepGpuError):
            eng.regex_compile(rx(pat))
    info = eng.regex_compile(rx(b"Sherl[oO]ck"))
    assert info.L == 8 and [info.class_bytes(j) for j in range(8)] == [b"S", b"h", b"e", b"r", b"l", b"Oo", b"c", b"k"]
    assert (info.anchor, info.n_anchor, bytes(info.anchor_bytes[:1]), info.self_overlap) == (0, 1, b"S", 0)
    assert eng.regex_compile(rx(b"\\^a")).L == 2 and eng.regex_compile(rx(b"a\\$")).L == 2 and eng.regex_compile(rx(b"[$^]")).L == 1


def test_selectors_and_split_follow_the_anchored_compiler(eng, monkeypatch):
    monkeypatch.setenv("KREP_GPU_ASSUME_AVAILABLE", "1")
    monkeypatch.delenv("KREP_GPU_DISABLE", raising=False)
    for pat in (b"^a", b"a$", b"^Sherl[oO]ck$"):
        assert eng.can_accelerate(rx(pat)) and eng.select(rx(pat)) is not None, pat
    assert not eng.can_accelerate(rx(b"a.*b")) and eng.select(rx(b"a.*b")) is None
    assert not eng.can_accelerate(rx(b"^a.*b$")) and eng.select(rx(b"^^a")) is None
    assert not eng.can_accelerate(rx(b"^Sherlock", whole_word=True)) and eng.select(rx(b"a$", whole_word=True)) is None
    assert eng.split_mode(rx(b"^ab"), 1 << 20) == abi.SPLIT_PIECES
    assert eng.split_mode(rx(b"^[ab]{2}"), 1 << 20) == abi.SPLIT_PIECES
    assert eng.split_mode(rx(b"[0-9]{3}$"), 1 << 20) == abi.SPLIT_PIECES
    assert eng.split_mode(rx(b"^[a\n]{2}"), 1 << 20) == abi.SPLIT_WHOLE
    assert eng.split_mode(rx(b"^[a\n]{2}", count_lines=True), 1 << 20) == abi.SPLIT_PIECES
    # unanchored: as before
    assert eng.split_mode(rx(b"[ab]{3}"), 1 << 20) == abi.SPLIT_WHOLE and eng.split_mode(rx(b"Sherl[oO]ck"), 1 << 20) == abi.SPLIT_PIECES
