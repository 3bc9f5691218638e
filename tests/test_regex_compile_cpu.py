"""krep_gpu_regex_compile (host only): every class equals the libc probe, the self-overlap test, every refusal with its reason,
and what krep_gpu_can_accelerate() says about -E."""
import pytest

import krep_amd
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


ATOMS = [b".", b"[^a]", b"[]a]", b"[^]a]", b"[a-]", b"[[:alpha:]]", b"[[:space:]]", b"[[:punct:]]", b"\\.", b"x{3}", b"Q", b"[[.-.]a]",
         b"[[=a=]b]", b"\n"]


@pytest.mark.parametrize("cs", [True, False])
def test_classes_are_libcs(eng, cs):
    for atom in ATOMS:
        info = eng.regex_compile(rx(atom, case_sensitive=cs))
        base = atom[:-3] if atom.endswith(b"{3}") else atom
        want = regex_ref.probe_class(base, cs)
        assert info.L == (3 if atom.endswith(b"{3}") else 1)
        for j in range(info.L):
            assert info.class_bytes(j) == want, (atom, cs, j)
    # the facts a hand-written table would get wrong (glibc, C locale)
    dot = eng.regex_compile(rx(b".", case_sensitive=cs)).class_bytes(0)
    assert dot == regex_ref.probe_class(b".", cs) and 10 not in dot
    assert 10 in eng.regex_compile(rx(b"[[:space:]]")).class_bytes(0)


def test_sequence_anchor_and_overlap(eng):
    info = eng.regex_compile(rx(b"Sherl[oO]ck"))
    assert info.L == 8 and [info.class_bytes(j) for j in range(8)] == [b"S", b"h", b"e", b"r", b"l", b"Oo", b"c", b"k"]
    assert info.anchor == 0 and info.n_anchor == 1 and bytes(info.anchor_bytes[:1]) == b"S" and info.self_overlap == 0
    info = eng.regex_compile(rx(b"[0-9]{3}-[0-9]{4}"))
    assert info.L == 8 and info.anchor == 3 and info.n_anchor == 1 and bytes(info.anchor_bytes[:1]) == b"-"
    info = eng.regex_compile(rx(b"[A-Z][a-z]{7}"))
    assert info.L == 8 and info.n_anchor == 0
    info = eng.regex_compile(rx(b"sherlock", case_sensitive=False))
    assert info.n_anchor == 2 and bytes(info.anchor_bytes[:2]) == b"Ss"
    assert eng.regex_compile(rx(b"a{16}")).L == 16
    for pat, ov in ((b"ab", 0), (b"[ab][ab]", 1), (b"a.a", 1), (b"a", 0), (b"aba", 1), (b"abc", 0)):
        assert eng.regex_compile(rx(pat)).self_overlap == ov, pat


REFUSED = [b"a.*b", b"(ab)", b"a+", b"a?", b"a|b", b"^a", b"a$", b"a)", b"a{2,}", b"a{2,3}", b"{2}a", b"a{2}{3}", b"\\bword", b"\\w",
           b"\\1", b"caf\xe9", b"a{17}", b"a{16}b", b"", b"[ab", b"a{0}", b"a\\"]


def test_refusals_carry_a_reason(eng):
    for pat in REFUSED:
        with pytest.raises(KrepGpuError) as e:
            eng.regex_compile(rx(pat))
        assert len(str(e.value)) > 8, pat
    with pytest.raises(KrepGpuError, match="alternation"):
        eng.regex_compile(abi.Params([b"ab", b"cd"], regex=True))
    with pytest.raises(KrepGpuError, match="-w"):
        eng.regex_compile(rx(b"ab", whole_word=True))
    # a literal search is not this compiler's business
    with pytest.raises(KrepGpuError):
        eng.regex_compile(abi.Params([b"ab"]))


def test_a_multibyte_locale_is_refused(eng):
    """libc matches characters there, not bytes: '.' takes a whole UTF-8 sequence as one atom"""
    import locale
    old = locale.setlocale(locale.LC_CTYPE)
    try:
        for name in ("C.UTF-8", "en_US.UTF-8", "C.utf8"):
            try:
                locale.setlocale(locale.LC_CTYPE, name)
                break
            except locale.Error:
                continue
        else:
            raise AssertionError("no UTF-8 locale can be set on this host (C.UTF-8 is built into glibc since 2.35)")
        with pytest.raises(KrepGpuError, match="multibyte locale"):
            eng.regex_compile(rx(b"Sherl[oO]ck"))
        assert not eng.can_accelerate(rx(b"Sherl[oO]ck"))
    finally:
        locale.setlocale(locale.LC_CTYPE, old)
    assert eng.regex_compile(rx(b"Sherl[oO]ck")).L == 8


def test_can_accelerate_follows_the_compiler(eng, monkeypatch):
    monkeypatch.setenv("KREP_GPU_ASSUME_AVAILABLE", "1")
    monkeypatch.delenv("KREP_GPU_DISABLE", raising=False)
    assert eng.can_accelerate(rx(b"Sherl[oO]ck")) and eng.select(rx(b"Sherl[oO]ck")) is not None
    assert not eng.can_accelerate(rx(b"a.*b")) and eng.select(rx(b"a.*b")) is None
    assert not eng.can_accelerate(rx(b"Sherlock", whole_word=True))
    assert eng.split_mode(rx(b"Sherl[oO]ck"), 1 << 20) == abi.SPLIT_PIECES
    assert eng.split_mode(rx(b"[ab]{3}"), 1 << 20) == abi.SPLIT_WHOLE
    assert eng.split_mode(rx(b"[ab]{3}", count_lines=True), 1 << 20) == abi.SPLIT_PIECES
    # the cost model's CPU side for regex_search: one thread at the scalar rate, whatever the caller runs
    c = eng.cost_estimate(rx(b"Sherl[oO]ck"), 1 << 30, 64)
    assert c.cpu_algo == abi.RA_REGEX and c.cpu_threads == 1
