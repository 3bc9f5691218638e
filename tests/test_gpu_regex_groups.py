"""krep -E on the device for what krep_gpu_regex_compile_groups() takes (repeated and nested groups, held as a position automaton;
kg_regex_loops.hip: the line walk's general step behind the loops scan's filter and roads) against the reference's regex_search: the
compiled reference (oracle/_ref, through tests/regex_ref.py) answers every case with the expression the CLI compiles.  The module
turns the switches krep_gpu_set_regex_groups and krep_gpu_set_regex_loops on and, whatever happens, off again."""
import ctypes as C

import numpy as np
import pytest

import regex_ref
from krep_amd import abi
from krep_amd.engine import KrepGpuError
from test_gpu_regex_loops import (AUTO, CAPPED, DENSE, LENGTHS, MODES, SPARSE, UNIT, background, check, cpu_selector, expected, planted,
                                  put_line, rx, scan_records, to_device)
from test_gpu_regex_loops import SHAPES as LOOPS_SHAPES

pytestmark = pytest.mark.gpu

IP = rb"[0-9]{1,3}\.[0-9]{1,3}\.[0-9]{1,3}\.[0-9]{1,3}"
AZ = b"abcdefghijklmnopqrstuvwxyz"
P32_FRONT = b"(" + AZ + AZ[:6] + b")+"                 # 32 positions, position 31 hands back to position 0
P32_MIDDLE = AZ[:12] + b"(" + AZ[:20] + b")+"          # 32 positions, position 31 hands back to position 12


@pytest.fixture(autouse=True, scope="module")
def _c_locale():
    with regex_ref.c_locale():
        yield


@pytest.fixture(scope="module")
def gpu():
    import krep_amd
    e = krep_amd.load()
    assert e.device_count() >= 1 and e.available(), e.unavailable_reason()
    e.set_regex_loops(True)
    e.set_regex_groups(True)
    try:
        yield e
    finally:
        e.set_regex_groups(False)
        e.set_regex_loops(False)
        e.force_regex_general(False)
        e.force_regex_loops_road(AUTO)
        e.force_regex_grid(0)
        e.inject_failure(0)
        e.set_cpu_fallback(None)


# (patterns, alphabet of the background lines, lines that hold a match, decoy lines: the filter without a match)
SHAPES = [
    ([b"(ab)+"], b"aabc \n", [b"ab", b"xababab", b"abab ab"], []),
    ([b"(a|bc)+d"], b"abcd \n", [b"ad", b"bcabcd", b"xaabcad bcd"], [b"d", b"bd cd"]),
    ([b"((ab)+c)+d"], b"abcd \n", [b"abcd", b"xababcabcd", b"abcababcd abcd"], [b"abc d", b"abcbcd acd"]),
    ([b"(a|ab)(c|bcd)"], b"abcd \n", [b"ac", b"abcd", b"abbcd xabc"], [b"ab", b"a c"]),     # (the expanding compiler's: four flat sequences)
    ([b"(a|ab)(c|bcd)+"], b"abcd \n", [b"ac", b"abcdc", b"abbcdbcd xabcc"], [b"c", b"bcd c"]),
    ([b"x(ab|a)*bc"], b"xabc \n", [b"xbc", b"xababc", b"xaabbc xabc"], [b"bc", b"xab c"]),
    ([IP], b"0123. x\n", [b"10.0.0.1", b"x192.168.001.255:80", b"1.2.3.4.5.6.7.8 9999.1.1.1111"], [b"1.2.3", b"1.2.3. 4"]),
    ([b"^(ab)+"], b"aab \n", [b"ab", b"ababa ab", b"abab"], [b" ab", b"bab"]),
    ([b"(ab)+$"], b"abb \n", [b"ab", b"a abab", b"ab bab"], [b"ab a", b"abx"]),
    ([b"(ab)+", b"c(d|e)*f"], b"abcdef \n", [b"ab", b"cdedf", b"xcf abab"], [b"cde"]),
    ([P32_FRONT], b"abcdef \n", [AZ + AZ[:6], b"x" + (AZ + AZ[:6]) * 3 + b"abc", (AZ + AZ[:6]) * 2 + b" " + AZ + AZ[:6]], [AZ + AZ[:5], AZ[:16]]),
    ([P32_MIDDLE], b"abcdklm \n", [AZ[:12] + AZ[:20], b"x" + AZ[:12] + AZ[:20] * 4 + b"ab", AZ[:12] + AZ[:20] + AZ[:12] + AZ[:20]],
     [AZ[:12] + AZ[:19], AZ[:20]]),
]
OLDER = 3  # the row an older compiler keeps


def takes(gpu, pats):
    """the groups compiler takes the row (the older ones refuse it), or it is the row the expanding compiler keeps"""
    if pats == SHAPES[OLDER][0]:
        gpu.regex_compile_ext(rx(pats))
        return
    gpu.regex_compile_groups(rx(pats))
    for older in (gpu.regex_compile_ext, gpu.regex_compile_loops):
        with pytest.raises(KrepGpuError):
            older(rx(pats))


@pytest.mark.parametrize("shape", range(len(SHAPES)))
def test_operator_equals_regex_search(gpu, shape):
    pats, alphabet, plants, decoys = SHAPES[shape]
    takes(gpu, pats)
    rng = np.random.RandomState(4100 + shape)
    gpu.force_regex_loops_road(AUTO)
    for n in LENGTHS:
        text = planted(rng, n, alphabet, plants, decoys)
        for kw in MODES + (CAPPED if n in (1025, 32769) else ()):
            check(gpu, pats, text, **kw)
        if n >= 1024:
            assert expected(pats, text)[0] > (12 if n > UNIT else 2)  # the planted lines are found
            if decoys:  # ... and the decoys hold no match
                assert expected(pats, np.frombuffer(b"\n".join(decoys), dtype=np.uint8))[0] == 0
    assert gpu.search(rx(pats, max_count=0, track_positions=False), text)[0] == 1


def test_the_thirty_two_positions_are_all_in_use(gpu):
    for pat, back in ((P32_FRONT, 0), (P32_MIDDLE, 12)):
        g = gpu.regex_compile_groups(rx([pat]))
        assert g["n_pos"] == 32 and g["follow"][31] == {back} and g["last"] == {31}
    # the second and third round of the loop pass bit 31: a match of 32, 64 and 96 bytes in one line
    line = (AZ + AZ[:6]) * 3
    text = np.frombuffer(b"x" + line + b"\n" + line[:64] + b"q\n" + line[:32], dtype=np.uint8)
    want = check(gpu, [P32_FRONT], text)
    assert [int(e - s) for s, e in want[1]] == [96, 64, 32]


@pytest.mark.parametrize("road", [SPARSE, DENSE])
def test_both_roads_on_every_shape(gpu, road):
    rng = np.random.RandomState(177 + road)
    try:
        gpu.force_regex_loops_road(road)
        for k, (pats, alphabet, plants, decoys) in enumerate(SHAPES):
            if k == OLDER:
                continue
            text = planted(rng, 70001, alphabet, plants, decoys)
            before = gpu.regex_loops_roads()
            for kw in (dict(), dict(count_lines=True), dict(max_count=3), dict(case_sensitive=False, track_positions=False)):
                check(gpu, pats, text, **kw)
            after = gpu.regex_loops_roads()
            assert after[road - 1] - before[road - 1] == 4 and after[2 - road] == before[2 - road], (pats, before, after)
    finally:
        gpu.force_regex_loops_road(AUTO)


def test_starved_grid_a_lane_takes_several_lines(gpu):
    rng = np.random.RandomState(110)
    words = np.frombuffer(b"ab\nba\nbb\naa\nb \n a\n", dtype=np.uint8).reshape(-1, 3)
    text = words[rng.randint(0, words.shape[0], size=40000)].reshape(-1).copy()
    pats = [b"(ab)+"]
    jobs = (dict(), dict(count_lines=True), dict(max_count=5000))
    wants = [expected(pats, text, **kw) for kw in jobs]
    assert wants[0][0] > 5000
    try:
        for blocks in (1, 3):
            for road in (SPARSE, DENSE):
                gpu.force_regex_grid(blocks)
                gpu.force_regex_loops_road(road)
                for kw, want in zip(jobs, wants):
                    got = gpu.search(rx(pats, **kw), text)
                    assert gpu.last_status() == abi.STATUS_OK
                    assert got[0] == want[0] and np.array_equal(got[1], want[1]), (blocks, road, kw, got[0], want[0])
    finally:
        gpu.force_regex_grid(0)
        gpu.force_regex_loops_road(AUTO)


def test_unaligned_device_text_with_hostile_bytes_around_it(gpu):
    """the text 3 and 13 bytes into its allocation, every byte around it an 'a' / a 'b' in turn: no byte outside the text is read"""
    rng = np.random.RandomState(108)
    pats, alphabet, plants, decoys = SHAPES[0]
    n = 50001
    text = planted(rng, n, alphabet, plants, decoys)
    text[:2] = np.frombuffer(b"b ", dtype=np.uint8)
    text[n - 1] = ord("a")  # (read with the pad byte 'b' behind it, it would be one match more; so would the pad 'a' in front of the text)
    want, want_c = expected(pats, text), expected(pats, text, count_lines=True)
    assert want[0] > 100
    for shift, pad in ((3, ord("b")), (13, ord("a"))):
        hold, d_text = to_device(text, shift, pad=pad)
        assert d_text % 16 == shift
        for road in (SPARSE, DENSE):
            gpu.force_regex_loops_road(road)
            plan, plan_c = gpu.plan(rx(pats)), gpu.plan(rx(pats, count_lines=True))
            try:
                out, pos = scan_records(plan, d_text, n)
                assert (out.count, out.stored, out.total_matches, out.overflow) == (want[0], want[0], want[0], 0)
                assert np.array_equal(pos[:2 * want[0]].astype(np.uint64).reshape(-1, 2), want[1]) and (pos[2 * want[0]:] == -1).all()
                assert plan_c.scan(d_text, n).line_count == want_c[0]
            finally:
                gpu.force_regex_loops_road(AUTO)
                plan.close()
                plan_c.close()
        del hold


def test_a_line_of_4096_bytes_is_walked_and_one_of_4097_is_not(gpu):
    rng = np.random.RandomState(111)
    pats = [b"(ab)+"]
    for road in (SPARSE, DENSE):
        gpu.force_regex_loops_road(road)
        try:
            for line, ok in ((b"ab" * 2048, True), (b"ab" * 2048 + b"a", False)):
                text = background(rng, 30000, b"aac \n")
                put_line(text, 9000, line)
                put_line(text, 200, b"xabab")
                want = expected(pats, text)
                assert [4096] == [int(e - s) for s, e in want[1] if e - s > 100]
                hold, d_text = to_device(text, 3)
                plan, plan_c = gpu.plan(rx(pats)), gpu.plan(rx(pats, count_lines=True))
                try:
                    if ok:
                        out, pos = scan_records(plan, d_text, text.size)
                        assert out.count == want[0] and np.array_equal(pos[:2 * want[0]].astype(np.uint64).reshape(-1, 2), want[1])
                        assert plan_c.scan(d_text, text.size).count == expected(pats, text, count_lines=True)[0]
                    else:
                        for pl in (plan, plan_c):
                            with pytest.raises(KrepGpuError, match="a line of more than 4096 bytes: kept on krep's regex_search"):
                                scan_records(pl, d_text, text.size)
                        with pytest.raises(KrepGpuError, match="more than 4096 bytes"):
                            gpu.search(rx(pats), text)
                        assert gpu.last_status() == abi.STATUS_FAILED
                        # the next call after the refusal, on the same plan
                        good = text.copy()
                        good[9000 + 2000] = 10
                        hold2, d_good = to_device(good, 3)
                        w = expected(pats, good)
                        out, pos = scan_records(plan, d_good, good.size)
                        assert out.count == w[0] and np.array_equal(pos[:2 * w[0]].astype(np.uint64).reshape(-1, 2), w[1])
                        del hold2
                finally:
                    plan.close()
                    plan_c.close()
                del hold
        finally:
            gpu.force_regex_loops_road(AUTO)


def test_the_general_step_walks_a_loops_expression_like_the_old_step(gpu):
    """krep_gpu_debug_force_regex_general: four expressions of the loops compiler, a plan made with the hook on (the general step) and
    one made with it off (the old step) give the same records, and both the reference's"""
    rng = np.random.RandomState(112)

    def run(plan, d_text, n):
        out, pos = scan_records(plan, d_text, n)
        return int(out.count), pos[:2 * int(out.stored)].astype(np.uint64).reshape(-1, 2)

    for k in (0, 2, 5, 9):
        pats, alphabet, plants, decoys = LOOPS_SHAPES[k]
        gpu.regex_compile_loops(rx(pats))
        text = planted(rng, 40001, alphabet, plants, decoys)
        hold, d_text = to_device(text, 5)
        for kw in (dict(), dict(count_lines=True), dict(case_sensitive=False), dict(max_count=3)):
            old_plan = gpu.plan(rx(pats, **kw))
            gpu.force_regex_general(True)
            try:
                new_plan = gpu.plan(rx(pats, **kw))
            finally:
                gpu.force_regex_general(False)
            try:
                want = expected(pats, text, **kw)
                for road in (SPARSE, DENSE):
                    gpu.force_regex_loops_road(road)
                    before = gpu.regex_general_walks()
                    old = run(old_plan, d_text, text.size)
                    assert gpu.regex_general_walks() == before  # the old step ...
                    new = run(new_plan, d_text, text.size)
                    assert gpu.regex_general_walks() > before   # ... and the general one: the hook took effect
                    assert old[0] == new[0] == want[0] and np.array_equal(old[1], new[1]) and np.array_equal(new[1], want[1]), (pats, road, kw)
            finally:
                gpu.force_regex_loops_road(AUTO)
                old_plan.close()
                new_plan.close()
        assert expected(pats, text)[0] > 12
        del hold


@pytest.mark.parametrize("mode", [1, 2, 3, 4])
def test_injected_failures_fall_back_to_the_cpu_function(gpu, mode):
    rng = np.random.RandomState(113)
    pats, alphabet, plants, decoys = SHAPES[1]
    text = planted(rng, 20001, alphabet, plants, decoys)
    cb = cpu_selector()
    gpu.set_cpu_fallback(C.cast(cb, C.c_void_p).value)
    try:
        # (failure 4 is the read-back of the records: a -c search reads none back)
        for kw in (dict(), dict(count_lines=True))[:1 if mode == 4 else 2]:
            p = rx(pats, **kw)
            comp = regex_ref.Compiled(pats[0])
            p.s.compiled_regex = comp.ptr
            gpu.inject_failure(mode)
            got = gpu.search(p, text)
            w = expected(pats, text, **kw)
            assert gpu.last_status() == abi.STATUS_FELL_BACK and got[0] == w[0] and np.array_equal(got[1], w[1]), (mode, kw)
    finally:
        gpu.inject_failure(0)
        gpu.set_cpu_fallback(None)
    check(gpu, pats, text)


def test_the_switch_off_gives_the_library_every_other_test_expects(gpu):
    text = np.frombuffer(b"abab abc\n" * 100, dtype=np.uint8)
    gpu.set_regex_groups(False)
    try:
        for pats in ([b"(ab)+"], [IP]):
            assert not gpu.can_accelerate(rx(pats)) and gpu.select(rx(pats)) is None
            with pytest.raises(KrepGpuError, match="kept on krep's regex_search"):
                gpu.search(rx(pats), text)
            assert gpu.last_status() == abi.STATUS_FAILED
    finally:
        gpu.set_regex_groups(True)
    assert gpu.can_accelerate(rx([b"(ab)+"]))
    check(gpu, [b"(ab)+"], text)
