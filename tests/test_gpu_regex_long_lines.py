"""krep -E loops and groups on lines of more than 4096 bytes (krep_gpu_set_regex_long_lines; kg_regex_loops.hip: the lister, the two
linear passes of rx_long_walk, the rounds of its scratch) against the reference's regex_search: the compiled reference (oracle/_ref,
through tests/regex_ref.py) answers every case with the expression the CLI compiles, count and records, as
test_gpu_regex_loops.py::check does.  The module turns the three switches on and, whatever happens, off again, and resets the budget,
road, grid and general hooks."""
import numpy as np
import pytest

import line_model as lm
import only_matching_model as om
import regex_ref
from krep_amd import abi
from krep_amd.engine import KrepGpuError
from test_gpu_regex_loops import AUTO, DENSE, SPARSE, background, check, expected, rx, scan_records, to_device

pytestmark = pytest.mark.gpu

EDGE_LENGTHS = (4096, 4097, 4098, 8191, 8192, 8193)


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
    e.set_regex_long_lines(True)
    try:
        yield e
    finally:
        e.set_regex_long_lines(False)
        e.set_regex_groups(False)
        e.set_regex_loops(False)
        e.set_regex_loops_windows(False)
        e.set_regex_long_budget(0)
        e.force_regex_general(False)
        e.force_regex_loops_road(AUTO)
        e.force_regex_grid(0)


def lines_text(rng, alphabet, long_lines, n_short=60, first=False, last=False, final_newline=True):
    """short random lines over `alphabet` (no newline in it) with `long_lines` (bytes) among them in their order; first / last: a long
    line is the text's first / last line"""
    short = [bytes(background(rng, rng.randint(0, 60), alphabet)) for _ in range(n_short)]
    at = sorted(rng.randint(1, n_short, size=len(long_lines)).tolist())
    if first and at:
        at[0] = 0
    if last and at:
        at[-1] = n_short
    out, k = [], 0
    for i in range(n_short + 1):
        while k < len(at) and at[k] == i:
            out.append(long_lines[k])
            k += 1
        if i < n_short:
            out.append(short[i])
    return np.frombuffer(b"\n".join(out) + (b"\n" if final_newline else b""), dtype=np.uint8).copy()


def long_line(rng, alphabet, n, head=b"", tail=b""):
    return head + bytes(background(rng, n - len(head) - len(tail), alphabet)) + tail


def all_modes(gpu, pats, text, roads=(SPARSE, DENSE), more=()):
    """records, -c and count-only on every road; -> the reference's records"""
    try:
        for road in roads:
            gpu.force_regex_loops_road(road)
            for kw in (dict(), dict(count_lines=True), dict(track_positions=False)) + tuple(more):
                check(gpu, pats, text, **kw)
    finally:
        gpu.force_regex_loops_road(AUTO)
    return expected(pats, text)


# ------------------------------------------------------------------------------------------------------------ 1. edges
@pytest.mark.parametrize("pats,alphabet", [([b"a+b"], b"aab c"), ([b"(ab)+c"], b"abc ")], ids=["loops", "groups"])
def test_lines_around_4096_and_8192_bytes_on_both_roads(gpu, pats, alphabet):
    rng = np.random.RandomState(1)
    text = lines_text(rng, alphabet, [long_line(rng, alphabet, n) for n in EDGE_LENGTHS])
    want = expected(pats, text)
    starts = want[1][:, 0].astype(np.int64)
    nl = np.flatnonzero(text == 10)
    ls = int(nl[np.flatnonzero(np.diff(nl) - 1 == 8192)[0]]) + 1                    # the 8192-byte line
    inside = int(np.searchsorted(starts, ls + 4000)) + 1                            # a max_count that falls inside its matches
    assert ls < want[1][inside - 1, 0] < ls + 8192 and want[1][inside, 0] < ls + 8192
    before = gpu.regex_long_walks()
    all_modes(gpu, pats, text, more=tuple(dict(max_count=mc, **kw) for mc in (0, 1, inside, 10 ** 9)
                                          for kw in (dict(), dict(count_lines=True), dict(track_positions=False))))
    assert gpu.regex_long_walks() > before
    # the text 1 and 3 bytes into its allocation, bytes around it that would lengthen a match
    for shift in (1, 3):
        hold, d_text = to_device(text[:-1], shift, pad=ord("a"))  # (the last line ends with the text, not with a newline)
        w, wc = expected(pats, text[:-1]), expected(pats, text[:-1], count_lines=True)
        plan, plan_c = gpu.plan(rx(pats)), gpu.plan(rx(pats, count_lines=True))
        try:
            for road in (SPARSE, DENSE):
                gpu.force_regex_loops_road(road)
                out, pos = scan_records(plan, d_text, text.size - 1)
                assert out.count == w[0] and np.array_equal(pos[:2 * w[0]].astype(np.uint64).reshape(-1, 2), w[1]) and (pos[2 * w[0]:] == -1).all()
                o = plan_c.scan(d_text, text.size - 1)
                assert (o.count, o.line_count, bool(o.has_newline)) == (wc[0], wc[0], True)
        finally:
            gpu.force_regex_loops_road(AUTO)
            plan.close()
            plan_c.close()
        del hold


# ------------------------------------------------------------------------------------------------------------ 2. killers
def test_the_lines_that_make_the_restarting_walk_quadratic(gpu):
    a = b"a" * 8192
    text = np.frombuffer(b"xx\n" + a + b"\nyy a!\n", dtype=np.uint8)
    want = all_modes(gpu, [b"a|a[a-z]*!"], text, more=(dict(max_count=5000),))
    assert want[0] == 8193                                                          # 8192 records from one lane, and the short line's
    for bs in ((), (1,), (4096,), (8191,), (1, 4096, 8191)):
        line = bytearray(a)
        for b in bs:
            line[b] = ord("b")
        text = np.frombuffer(b"ab\n" + bytes(line) + b"\na\n", dtype=np.uint8)
        want = all_modes(gpu, [b"a.*b"], text)
        assert want[0] == 1 + int(bool(bs))
    rng = np.random.RandomState(2)
    words = [b"ERROR", b"timeout", b"error", b"time out", b" ", b": ", b"retry", b"x"]
    line = b" ".join(words[k] for k in rng.randint(0, len(words), size=1500))
    assert len(line) > 4096 and line.count(b"ERROR") > 3 and line.count(b"timeout") > 3
    text = lines_text(rng, b"EROtimeu: ", [line, line[::-1], b"timeout " * 600 + b"ERROR", b"ERROR " * 900])
    want = all_modes(gpu, [b"ERROR.*timeout"], text, more=(dict(case_sensitive=False),))
    assert want[0] >= 1


# ------------------------------------------------------------------------------------------------------------ 3. line ends
@pytest.mark.parametrize("where", ["first", "last", "last-open", "only"])
def test_anchors_on_a_long_first_line_last_line_and_a_text_of_one_line(gpu, where):
    rng = np.random.RandomState(3)
    for pats, alphabet, head, tail in (([b"^#+ "], b"# ab", b"### ", b""), ([b"[a-z]+c$"], b"abc ", b"", b" abcc")):
        for n in (4097, 6000):
            line = long_line(rng, alphabet, n, head, tail)
            if where == "only":
                text = np.frombuffer(line, dtype=np.uint8)
            else:
                text = lines_text(rng, alphabet, [line], 20, first=where == "first", last=where != "first", final_newline=where != "last-open")
            assert (text[:n].tobytes() == line) if where in ("first", "only") else (text.tobytes().rstrip(b"\n").endswith(line))
            # (-i: the end of the text ends no line, so a `$` at an open last line finds nothing)
            all_modes(gpu, pats, text, more=(dict(case_sensitive=False), dict(case_sensitive=False, count_lines=True)))
        want, want_i = expected(pats, text), expected(pats, text, case_sensitive=False)
        assert want[0] >= 1
        if where in ("last-open", "only") and pats == [b"[a-z]+c$"]:
            assert want[1][-1, 1] == text.size and (want_i[0] == 0 or want_i[1][-1, 1] < text.size)


# ------------------------------------------------------------------------------------------------------------ 4. the general step
def test_groups_programs_and_a_loops_program_through_the_general_step(gpu):
    rng = np.random.RandomState(4)
    text = np.frombuffer(b"ab\n" + b"ab" * 3000 + b"\nxab ab\n", dtype=np.uint8)
    assert all_modes(gpu, [b"(ab)+"], text)[1].tolist()[1] == [3, 6003]
    names = [b"www", b"example", b"com", b"org", b"a", b"mail", b"x1"]
    dotted = b"".join(names[k] + (b"." if rng.randint(3) else b" ") for k in rng.randint(0, len(names), size=1400))
    semis = b"".join((b"foo", b"bar", b";", b" ", b"fo", b"foobar;")[k] for k in rng.randint(0, 6, size=2200))
    acs = long_line(rng, b"abcd ", 7000)
    for pats, line, alphabet in (([b"([a-z]+\\.)+com"], dotted, b"abcom. "), ([b"(foo|bar)+;"], semis, b"fobar; "), ([b"(a|ab)(c|bcd)+"], acs, b"abcd ")):
        assert len(line) > 4096
        want = all_modes(gpu, pats, lines_text(rng, alphabet, [line, line[1:]], 30), more=(dict(max_count=7),))
        assert want[0] > 20
    # a loops program by the shift and, through the hook, by the general step: the same records
    pats, alphabet = [b"[0-9]+\\.[0-9]+"], b"0123. x"
    text = lines_text(rng, alphabet, [long_line(rng, alphabet, n) for n in (5000, 9001)], 30)
    want = expected(pats, text)
    hold, d_text = to_device(text, 5)
    for kw in (dict(), dict(count_lines=True)):
        old_plan = gpu.plan(rx(pats, **kw))
        gpu.force_regex_general(True)
        try:
            new_plan = gpu.plan(rx(pats, **kw))
        finally:
            gpu.force_regex_general(False)
        try:
            before = gpu.regex_general_walks()
            old = scan_records(old_plan, d_text, text.size)
            assert gpu.regex_general_walks() == before
            new = scan_records(new_plan, d_text, text.size)
            assert gpu.regex_general_walks() > before
            assert old[0].count == new[0].count == expected(pats, text, **kw)[0] and np.array_equal(old[1], new[1])
            if not kw:
                assert np.array_equal(new[1][:2 * want[0]].astype(np.uint64).reshape(-1, 2), want[1])
        finally:
            old_plan.close()
            new_plan.close()
    del hold


# ------------------------------------------------------------------------------------------------------------ 5. more than a wave, 6. rounds and the cap
_many = {}


def many_lines():
    """150 long lines of 4097 .. 12000 bytes among short ones, built once (about 1.2 MB: 150 lines of more than 4096 bytes do not fit
    the 256 KiB the other texts of this module keep to)"""
    if not _many:
        rng = np.random.RandomState(5)
        alphabet = b"0123. xy"
        lengths = np.linspace(4097, 12000, 150).astype(int)
        rng.shuffle(lengths)
        _many["text"] = lines_text(rng, alphabet, [long_line(rng, alphabet, int(n)) for n in lengths], 200)
        _many["text"].setflags(write=False)
    return [b"[0-9]+\\.[0-9]+"], _many["text"]


def test_150_long_lines_more_than_a_wave_and_a_starved_grid(gpu):
    pats, text = many_lines()
    want = all_modes(gpu, pats, text, roads=(AUTO,), more=(dict(max_count=expected(pats, text)[0] // 2),))
    assert want[0] > 10000
    try:
        gpu.force_regex_grid(1)
        all_modes(gpu, pats, text, roads=(AUTO,))
    finally:
        gpu.force_regex_grid(0)


def test_rounds_of_the_scratch_give_the_same_records(gpu):
    pats, text = many_lines()
    try:
        gpu.set_regex_long_budget(4 * 400000)  # 150 lines of 1.2 M bytes: four rounds of 400 000 scratch words
        before = gpu.regex_long_walks()
        check(gpu, pats, text)
        assert gpu.regex_long_walks() - before >= 6  # three counting and three emitting rounds at the least
        before = gpu.regex_long_walks()
        check(gpu, pats, text, count_lines=True)
        assert gpu.regex_long_walks() - before == 1  # -c keeps no scratch: one launch
    finally:
        gpu.set_regex_long_budget(0)


def test_the_cap_of_one_line_follows_the_budget(gpu):
    import torch
    rng = np.random.RandomState(6)
    pats, alphabet = [b"a+b"], b"aab c"
    try:
        for n, ok in ((8192, True), (8193, False)):
            text = lines_text(rng, alphabet, [long_line(rng, alphabet, n)], 20)
            hold, d_text = to_device(text, 1)
            plan, plan_c = gpu.plan(rx(pats)), gpu.plan(rx(pats, count_lines=True))
            try:
                gpu.set_regex_long_budget(4 * 8192)  # the cap is min(1 MiB, budget / 4) = 8192 bytes
                if ok:
                    check(gpu, pats, text)
                    check(gpu, pats, text, count_lines=True)
                else:
                    pos = torch.full((2 << 14,), -1, dtype=torch.int64, device="cuda")
                    for pl in (plan, plan_c):
                        with pytest.raises(KrepGpuError, match="a line of more than 8192 bytes: kept on krep's regex_search"):
                            pl.scan(d_text, text.size, 0, text.size, 0, pos.data_ptr(), 1 << 14)
                    assert (pos == -1).all().item()  # nothing written
                    gpu.set_regex_long_budget(0)     # the default budget: the same line is walked
                    w = expected(pats, text)
                    out, got = scan_records(plan, d_text, text.size)
                    assert out.count == w[0] and np.array_equal(got[:2 * w[0]].astype(np.uint64).reshape(-1, 2), w[1])
                    assert plan_c.scan(d_text, text.size).count == expected(pats, text, count_lines=True)[0]
            finally:
                plan.close()
                plan_c.close()
            del hold
    finally:
        gpu.set_regex_long_budget(0)


# ------------------------------------------------------------------------------------------------------------ 7. plan reuse
def test_one_plan_over_texts_with_without_and_with_more_long_lines(gpu):
    rng = np.random.RandomState(7)
    pats, alphabet = [b"a+b"], b"aab c"
    texts = [lines_text(rng, alphabet, [long_line(rng, alphabet, 5000)], 30), lines_text(rng, alphabet, [], 30),
             lines_text(rng, alphabet, [long_line(rng, alphabet, n) for n in (9000, 20000, 4097, 30000)], 30)]
    plan, plan_c = gpu.plan(rx(pats)), gpu.plan(rx(pats, count_lines=True))
    try:
        for k, text in enumerate(texts * 2):
            hold, d_text = to_device(text, k)
            w = expected(pats, text)
            before = gpu.regex_long_walks()
            out, pos = scan_records(plan, d_text, text.size)
            assert out.count == w[0] and np.array_equal(pos[:2 * w[0]].astype(np.uint64).reshape(-1, 2), w[1]) and (pos[2 * w[0]:] == -1).all()
            assert plan_c.scan(d_text, text.size).count == expected(pats, text, count_lines=True)[0]
            moved = gpu.regex_long_walks() - before
            assert moved == (0 if k % 3 == 1 else 3), (k, moved)  # a counting, an emitting and a -c launch, or none
            del hold
    finally:
        plan.close()
        plan_c.close()


# ------------------------------------------------------------------------------------------------------------ 8. unchanged behaviour
def test_the_switch_off_and_any_window_but_the_whole_text_keep_the_refusal(gpu):
    import torch
    rng = np.random.RandomState(8)
    pats, alphabet = [b"a+b"], b"aab c"
    text = lines_text(rng, alphabet, [long_line(rng, alphabet, 4097)], 200)
    nl = np.flatnonzero(text == 10)
    ls = int(nl[np.flatnonzero(np.diff(nl) - 1 == 4097)[0]]) + 1
    hold, d_text = to_device(text, 2)
    pos = torch.full((2 << 14,), -1, dtype=torch.int64, device="cuda")
    plan = gpu.plan(rx(pats))
    try:
        gpu.set_regex_long_lines(False)
        with pytest.raises(KrepGpuError, match="a line of more than 4096 bytes: kept on krep's regex_search"):
            plan.scan(d_text, text.size, 0, text.size, 0, pos.data_ptr(), 1 << 14)
        with pytest.raises(KrepGpuError, match="more than 4096 bytes"):
            gpu.search(rx(pats), text)
        assert gpu.last_status() == abi.STATUS_FAILED
        gpu.set_regex_long_lines(True)
        gpu.set_regex_loops_windows(True)
        for lo, hi in ((0, ls + 100), (ls + 100, text.size), (1, text.size), (0, text.size - 1)):
            with pytest.raises(KrepGpuError, match="a line of more than 4096 bytes: kept on krep's regex_search"):
                plan.scan(d_text, text.size, lo, hi, 0, pos.data_ptr(), 1 << 14)
        gpu.set_regex_loops_windows(False)
        with pytest.raises(KrepGpuError, match="scan the whole text in one window"):
            plan.scan(d_text, text.size, 0, ls + 100, 0, pos.data_ptr(), 1 << 14)
        assert (pos == -1).all().item()  # nothing written by any of them
        w = expected(pats, text)
        out, got = scan_records(plan, d_text, text.size)  # ... and the whole text is walked
        assert out.count == w[0] and np.array_equal(got[:2 * w[0]].astype(np.uint64).reshape(-1, 2), w[1])
    finally:
        gpu.set_regex_long_lines(True)
        gpu.set_regex_loops_windows(False)
        plan.close()
    del hold


# ------------------------------------------------------------------------------------------------------------ 9. around the scan
def test_a_batch_item_and_the_grep_drivers_take_a_long_line(gpu):
    rng = np.random.RandomState(9)
    pats, alphabet = [b"[0-9]+\\.[0-9]+"], b"0123. x"
    items = [lines_text(rng, alphabet, [], 10), lines_text(rng, alphabet, [long_line(rng, alphabet, 5000)], 10, final_newline=False),
             lines_text(rng, alphabet, [], 5)]
    got = gpu.search_batch(rx(pats), [t.tobytes() for t in items])
    for (count, pos), t in zip(got, items):
        w = expected(pats, t)
        assert count == w[0] and np.array_equal(pos, w[1])
    text = items[1]
    w = expected(pats, text)
    rec = [(int(s), int(e)) for s, e in w[1]]
    nl = np.flatnonzero(text == 10)
    ls = int(nl[np.flatnonzero(np.diff(nl) - 1 == 5000)[0]]) + 1
    assert any(ls <= s < ls + 5000 for s, _ in rec)  # the long line is a matching line
    hold, d_text = to_device(text, 3)
    plan, plan_o = gpu.plan(rx(pats)), gpu.plan(rx(pats), only_matching=True)
    try:
        assert plan.longest_match() == 4097
        assert plan.grep_lines(d_text, text.size, filename=b"f.txt") == lm.grep_output(text.tobytes(), rec, b"f.txt:")
        assert plan_o.grep_only_matching(d_text, text.size, filename=b"f.txt") == om.grep_o_output(text.tobytes(), rec, b"f.txt")
    finally:
        plan.close()
        plan_o.close()
    del hold
