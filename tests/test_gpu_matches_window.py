"""krep_gpu_format_matches_window / Plan.grep_only_matching_pieces: the reference's -o output for a text in pieces.  Every window
against tests/matches_window_model.py; chained windows against krep_gpu_format_matches on the resident whole text; the driver
against Plan.grep_only_matching on the resident text and against the stock CLI (oracle/_ref/krep -t 1 -o) where that binary exists.
Every device call goes through three steps: the size query, the exact capacity, and a capacity one byte short (overflow with the
same sizes and carries); 0xEE pad bytes lie around the text and around the output."""
import ctypes as C
import random

import numpy as np
import pytest

import matches_window_model as mw
import only_matching_model as om
import oracle_lib as ol
from krep_amd import abi

pytestmark = pytest.mark.gpu

CLI = ol.ref_cli()
PAD = 0xEE
W = mw.Window


@pytest.fixture(scope="module")
def gpu():
    import krep_amd
    e = krep_amd.load()
    assert e.device_count() >= 1
    return e


def to_device(data, shift=0):
    """(tensor that owns the bytes, device pointer of data[0]): `shift` pad bytes in front of it, 64 behind"""
    import torch
    a = np.frombuffer(bytes(data), dtype=np.uint8)
    t = torch.full((a.size + shift + 64,), PAD, dtype=torch.uint8, device="cuda")
    if a.size:
        t[shift:shift + a.size] = torch.from_numpy(a.copy())
    return t, t.data_ptr() + shift


def records_to_device(recs):
    import torch
    a = np.asarray(recs, dtype=np.uint64).reshape(-1, 2)
    return torch.from_numpy(a.astype(np.int64)).cuda().contiguous(), len(a)


def device_window(gpu, buf, win, recs, strings=None, max_items=None, shift=0, out_shift=0):
    """one window on the device, in the three steps -> matches_window_model.Out"""
    import torch
    keep, d_text = to_device(buf, shift)
    pos, m = records_to_device(recs)
    d_pos = pos.data_ptr() if m else 0
    limit = abi.SIZE_MAX if max_items is None else max_items
    fmt = abi.MatchFormat(*strings) if strings is not None else None

    def call(d_out=0, capacity=0):
        r = gpu.format_matches_window(d_text, len(buf), abi.MatchesWindow(*win), d_pos, m, limit, fmt, d_out, capacity)
        return (int(r.matches.items), int(r.matches.out_bytes), int(r.newlines_before_count_to), int(r.stale_line)), int(r.matches.overflow)

    sizes, over = call()
    assert over == 0
    size = sizes[1]
    out = torch.full((size + 64,), PAD, dtype=torch.uint8, device="cuda")
    again, over = call(out.data_ptr() + out_shift, size)
    got = out.cpu().numpy()
    assert again == sizes and over == 0
    assert (got[:out_shift] == PAD).all() and (got[out_shift + size:] == PAD).all()  # nothing outside [d_out, d_out + out_bytes)
    if size > 1:
        out.fill_(PAD)
        short, over = call(out.data_ptr() + out_shift, size - 1)
        assert short == sizes and over == 1 and (out.cpu().numpy() == PAD).all()
    assert (keep.cpu().numpy()[:shift] == PAD).all() and (keep.cpu().numpy()[shift + len(buf):] == PAD).all()
    return mw.Out(got[out_shift:out_shift + size].tobytes(), sizes[0], sizes[2], sizes[3])


def check_window(gpu, buf, win, recs, strings=None, max_items=None, shift=0, out_shift=0):
    want = mw.window(buf, win, recs, strings or (b"", b"", b"", b""), max_items)
    got = device_window(gpu, buf, win, recs, strings, max_items, shift, out_shift)
    assert got == want, (win, recs[:8], max_items, shift, out_shift, got.data[:200], want.data[:200], got[1:], want[1:])
    return got


def edge_text(variant, n=13000, seed=5):
    """random bytes with many newlines; around the 4 KiB edges of a buffer that starts at BASE the newlines are placed by hand"""
    rng = np.random.RandomState(seed + variant)
    a = rng.choice(np.frombuffer(b"abcdefg\n", dtype=np.uint8), size=n)
    for edge in (4096, 8192):
        at = BASE + edge
        a[at - 3:at + 3] = ord("x")
        for k in ((-1, 0), (-2, 1))[variant]:  # variant 0: a newline on either side of the edge; 1: one byte further out
            a[at + k] = 10
    return a.tobytes()


BASE = 1003  # not a multiple of 16 or 4096


def test_block_arithmetic_inside_and_at_the_end_of_the_text(gpu):
    for variant in (0, 1):
        text = edge_text(variant)
        glen, last1 = len(text), mw.last_newline1(text)
        before = text.count(b"\n", 0, BASE)
        # a buffer inside the text: records at buffer offsets 0, 4095 / 4096 / 4097, 8191 / 8192 and the last byte
        blen = 8192 + 777
        buf = text[BASE:BASE + blen]
        offs = [0, 0, 5, 4095, 4096, 4097, 8191, 8192, blen - 3, blen - 1]
        recs = [(BASE + o, min(BASE + o + 3, BASE + blen)) for o in offs]
        recs[1] = (BASE, BASE)  # end == start: an empty MATCH
        for k, (shift, out_shift) in enumerate(((0, 0), (3, 5), (7, 0), (0, 5), (3, 0), (7, 5))):
            win = W(BASE, glen, BASE + (blen, 4096, 0, 8191, 4097, 4095)[k], before, last1, 0, 0)
            strings = (om.strings(b"f"), om.strings(None), om.strings(b"f", True))[k % 3]
            got = check_window(gpu, buf, win, recs, strings, None, shift, out_shift)
            assert got.items == len(recs)
            assert got.newlines_before_count_to == text.count(b"\n", 0, win.count_to)
        assert check_window(gpu, buf, W(BASE, glen, BASE, before, last1, 0, 0), recs, om.strings(b"f"), 4, 3, 5).items == 4
        # the same records as the whole-text call numbers them
        want = om.only_matching_output(text, recs, om.strings(b"f"))
        assert check_window(gpu, buf, W(BASE, glen, BASE, before, last1, 0, 0), recs, om.strings(b"f")).data == want
        # a buffer that ends the text: a record that ends at global_len, one that outruns it (clamped), an empty one on the last byte
        base = glen - 4096 - 55
        buf = text[base:]
        recs = [(base, base + 2), (base + 4095, base + 4099), (base + 4096, base + 4096), (glen - 5, glen), (glen - 2, glen + 9),
                (glen - 1, glen - 1)]
        for shift, out_shift in ((0, 5), (3, 0), (7, 5)):
            win = W(base, glen, glen, text.count(b"\n", 0, base), last1, 0, 0)
            got = check_window(gpu, buf, win, recs, om.strings(b"f", True), None, shift, out_shift)
            assert got.newlines_before_count_to == text.count(b"\n")
        assert check_window(gpu, buf, win, recs, om.strings(b"f")).data == om.only_matching_output(text, recs, om.strings(b"f"))


def test_line_number_digits_through_the_carry(gpu):
    buf = b"a\na\na\nb"
    recs = [(1000, 1001), (1002, 1003), (1004, 1005), (1006, 1007)]
    for k, nb in enumerate((8, 9, 98, 99, 10 ** 9 - 2, 10 ** 15 - 2)):
        for count_to in (1000, 1001, 1002, 1007):  # the buffer's start, ON a newline, one past it, the buffer's end
            win = W(1000, 5000, count_to, nb, 0, 0, 0)
            got = check_window(gpu, buf, win, recs, om.strings(None, k % 2 == 1), None, (0, 3, 7)[k % 3], (0, 5)[k % 2])
            assert got.newlines_before_count_to == nb + (0, 0, 1, 3)[(1000, 1001, 1002, 1007).index(count_to)]
        if k % 2 == 0:
            assert got.data == b"".join(b"%d:%s\n" % (nb + 1 + i, b"a" if i < 3 else b"b") for i in range(4))
    got = check_window(gpu, buf, W(1000, 5000, 1000, 10 ** 15 - 2, 0, 0, 0), recs, om.strings(b"f"))
    assert got.data.startswith(b"f:999999999999999:a\nf:1000000000000000:a\n")  # 15 and 16 digits
    import krep_amd
    with pytest.raises(krep_amd.KrepGpuError, match="16 digits"):  # 10^16 - 3 newlines in front and 3 in the buffer: 17 digits
        device_window(gpu, buf, W(1000, 5000, 1000, 10 ** 16 - 3, 0, 0, 0), recs)


def test_the_stale_rule_by_offset(gpu):
    text = b"ab\ncd\nef\ngh ij kl mn\nop qr st uv"  # the last newline at 20
    glen, last1 = len(text), mw.last_newline1(text)
    assert last1 == 21
    f = om.strings(None)
    # last_newline1 in front of the window: every record is stale and prints the value that came in, 1 when that is 0
    buf, recs = text[24:], [(24, 26), (27, 29), (30, 32)]
    assert check_window(gpu, buf, W(24, glen, glen, 4, last1, 3, 1), recs, f, None, 3, 5) == (b"3:qr\n3:st\n3:uv\n", 3, 4, 3)
    assert check_window(gpu, buf, W(24, glen, glen, 4, last1, 0, 1), recs, f, None, 7, 0) == (b"1:qr\n1:st\n1:uv\n", 3, 4, 0)
    assert check_window(gpu, buf, W(24, glen, glen, 4, last1, 3, 0), recs, f) == (b"5:qr\n5:st\n5:uv\n", 3, 4, 3)  # stale_rule = 0
    # ... inside it: a record ON the last newline prints its true number, the one at last_newline1 the stale one
    buf, recs = text[7:30], [(7, 8), (9, 11), (20, 22), (21, 23), (27, 29)]
    assert check_window(gpu, buf, W(7, glen, 30, 2, last1, 1, 1), recs, f, None, 3, 0) == (b"3:f\n4:gh\n4: o\n4:op\n4:st\n", 5, 4, 4)
    assert check_window(gpu, buf, W(7, glen, 30, 2, last1, 1, 0), recs, f, None, 0, 5) == (b"3:f\n4:gh\n4: o\n5:op\n5:st\n", 5, 4, 4)
    # ... the value comes from ALL n records: max_items in front of the record that sets it
    assert check_window(gpu, buf, W(7, glen, 7, 2, last1, 1, 1), recs, f, 1) == (b"3:f\n", 1, 2, 4)
    assert check_window(gpu, buf, W(7, glen, 7, 2, last1, 1, 1), recs, f, 0) == (b"", 0, 2, 4)
    # ... behind it: nothing is stale, and the carry out is the last record's number
    buf, recs = text[0:12], [(0, 2), (3, 5), (9, 11)]
    assert check_window(gpu, buf, W(0, glen, 12, 0, last1, 0, 1), recs, f, None, 7, 5) == (b"1:ab\n2:cd\n4:gh\n", 3, 3, 4)
    # a text without a newline: stale_rule alone changes nothing
    assert check_window(gpu, b"abab", W(0, 4, 4, 0, 0, 0, 1), [(0, 2), (2, 4)], f) == (b"1:ab\n1:ab\n", 2, 0, 0)


def test_a_window_without_records_carries_on(gpu):
    text = b"ab\ncd\n\nef\n"
    for rule in (0, 1):
        assert check_window(gpu, text[2:9], W(2, 10, 7, 11, 10, 4, rule), []) == (b"", 0, 14, 4)
        assert check_window(gpu, text[2:9], W(2, 10, 2, 11, 10, 0, rule), [], om.strings(b"f", True), None, 3) == (b"", 0, 11, 0)
        assert check_window(gpu, b"", W(5, 10, 5, 11, 10, 4, rule), []) == (b"", 0, 11, 4)
    # a record list on a later window still counts from the carry
    assert check_window(gpu, text[7:], W(7, 10, 10, 14, 10, 4, 1), [(7, 9)]).data == b"15:ef\n"


def test_refused_windows(gpu):
    import torch
    import krep_amd
    text = b"ab\nab\nab\nab\n"
    buf = text[3:9]
    keep, d_text = to_device(buf, 3)
    out = torch.full((256,), PAD, dtype=torch.uint8, device="cuda")
    ok = W(3, 12, 9, 1, 12, 0, 0)
    for win, recs, why in (
            (ok, [(6, 8), (3, 5)], "not ascending"),                    # a descending list
            (ok, [(2, 4)], "not ascending in start, or a record lies"),  # a start one byte in front of global_base
            (ok, [(3, 5), (9, 11)], "outside the buffer"),              # a start at global_base + text_len
            (ok, [(4, 3)], "not ascending in start, or a record lies"),  # end < start
            (ok, [(7, 10)], "outruns"),                                 # a match outrunning a buffer that does not end the text
            (ok._replace(count_to=2), [(3, 5)], "count_to"),
            (ok._replace(count_to=10), [(3, 5)], "count_to"),
            (ok._replace(last_newline1=13), [(3, 5)], "last_newline1"),
            (ok._replace(global_len=8), [(3, 5)], "not inside the text"),
            (ok._replace(global_len=10 ** 16, last_newline1=0), [(3, 5)], "too long")):
        pos, m = records_to_device(recs)
        res = abi.MatchesWindowOut()
        w = abi.MatchesWindow(*win)
        gpu.lib.krep_gpu_clear_error()
        rc = gpu.lib.krep_gpu_format_matches_window(C.c_void_p(d_text), len(buf), C.byref(w), C.c_void_p(pos.data_ptr()), m, abi.SIZE_MAX,
                                                    None, C.c_void_p(out.data_ptr()), 256, C.byref(res), None)
        assert rc == 2 and why in gpu.last_error(), (win, recs, gpu.last_error())
        with pytest.raises(mw.Refused):
            mw.window(buf, win, recs)
        assert (out.cpu().numpy() == PAD).all()  # the output buffer is untouched
    pos, m = records_to_device([(3, 5), (6, 8)])
    with pytest.raises(krep_amd.KrepGpuError, match="format string"):
        gpu.format_matches_window(d_text, len(buf), abi.MatchesWindow(*ok), pos.data_ptr(), m, fmt=abi.MatchFormat(b"x" * ((1 << 20) + 1)))
    with pytest.raises(krep_amd.KrepGpuError, match="more than one call takes"):
        gpu.format_matches_window(d_text, len(buf), abi.MatchesWindow(*ok), pos.data_ptr(), 1 << 40)
    res = abi.MatchesWindowOut()
    assert gpu.lib.krep_gpu_format_matches_window(C.c_void_p(d_text), len(buf), None, C.c_void_p(pos.data_ptr()), m, abi.SIZE_MAX, None,
                                                  None, 0, C.byref(res), None) == 2
    assert gpu.lib.krep_gpu_format_matches_window(C.c_void_p(d_text), len(buf), C.byref(abi.MatchesWindow(*ok)), C.c_void_p(pos.data_ptr()),
                                                  m, abi.SIZE_MAX, None, None, 0, None, None) == 2
    # the library works on after a refusal
    assert check_window(gpu, buf, ok, [(3, 5), (6, 8)], om.strings(b"f")).data == b"f:2:ab\nf:3:ab\n"


_LISTS = []


@pytest.fixture(scope="module")
def lists(oracle_engine):
    """the table rows and half of the seeded cases of only_matching_model with their record lists, computed once: every case with a
    last line that has no newline (where the numbers go stale) and every sixth of the others"""
    if not _LISTS:
        seeded = om.random_cases()
        for case in om.table_cases() + seeded[1::3] + seeded[::6]:
            _LISTS.append((case, om.lm.cut_to_max_count(case.emitted(oracle_engine, abi), case.max_count)))
    return _LISTS


def test_chained_windows_equal_the_whole_text_call(gpu, lists):
    import torch
    rng = random.Random(11)
    chains = stale = 0
    for idx, (case, recs) in enumerate(lists):
        text, n = case.text, len(recs)
        if not n:
            continue
        stale += om.stale_records(text, recs) > 0
        last_cut = sum(1 for s, _ in recs if s < mw.last_newline1(text))
        some = sorted(rng.randrange(0, n + 1) for _ in range(min(n, 3)))
        kinds = [some, sorted(some + some[:1] + [0, n]), [last_cut]] + ([list(range(1, n))] if n <= 24 else [])
        keep, d_text = to_device(text, (0, 3, 7)[idx % 3])
        pos, m = records_to_device(recs)
        for j, cuts in enumerate(kinds):
            color = (idx + j) % 2 == 1
            strings = om.strings(om.FILE, color)
            mid = min(n, max(1, (cuts[len(cuts) // 2] if cuts else 0) + 1)) if j % 2 == 0 else None  # ends inside a middle window
            shifts = ((0, 3, 7)[(idx + j) % 3], (0, 5)[j % 2])
            # the whole-text call on the resident text
            q = gpu.format_matches(d_text, len(text), pos.data_ptr(), m, abi.SIZE_MAX if mid is None else mid, abi.MatchFormat(*strings))
            dst = torch.full((int(q.out_bytes) + 64,), PAD, dtype=torch.uint8, device="cuda")
            r = gpu.format_matches(d_text, len(text), pos.data_ptr(), m, abi.SIZE_MAX if mid is None else mid, abi.MatchFormat(*strings),
                                   dst.data_ptr(), int(q.out_bytes))
            whole = dst[: int(r.out_bytes)].cpu().numpy().tobytes()
            got, items = mw.chain(text, recs, cuts, strings, mid,
                                  call=lambda buf, win, sub, fmt, left: device_window(gpu, buf, win, sub, fmt, left, *shifts))
            assert got == whole and items == int(r.items), (case.key, cuts, color, mid)
            assert (got, items) == mw.chain(text, recs, cuts, strings, mid) and got == om.only_matching_output(text, recs, strings, mid)
            chains += 1
    assert chains >= 400 and stale >= 30  # (33 of these lists print stale numbers)


# ---- Plan.grep_only_matching_pieces ----
def split_under_o(gpu, params, n):
    cfg = gpu.default_config()
    cfg.only_matching = 1
    gpu.set_thread_config(cfg)
    try:
        return gpu.split_mode(params, n)
    finally:
        gpu.set_thread_config(None)


def piece_text(seed, n, alphabet=b"ab ab\n", tail=0):
    rng = np.random.RandomState(seed)
    a = rng.choice(np.frombuffer(alphabet, dtype=np.uint8), size=n)
    if tail:
        a[-tail:][a[-tail:] == 10] = ord("b")  # a last line of at least `tail` bytes
    return a.tobytes()


def check_pieces(gpu, case, tmp_path, pieces, colors=(False,)):
    """the driver on every piece size against the resident whole-text road, and that against the CLI where it is here
    -> the output without colour"""
    text = case.text
    keep, d_text = to_device(text)
    plan = gpu.plan(case.params(abi), only_matching=True)
    plain = None
    for color in colors:
        want = plan.grep_only_matching(d_text, len(text), filename=om.FILE, color=color)
        plain = want if plain is None else plain  # (colors[0] is False)
        if CLI:
            path = tmp_path / "t.txt"
            path.write_bytes(text)
            rc, out = om.run_cli(CLI, case, path, color)
            assert out == want, (case.key, case.cli_args(color))
        for piece in pieces:
            got = plan.grep_only_matching_pieces(text, piece, filename=om.FILE, color=color)
            assert got == want, (case.key, piece, color, got[:300], want[:300])
    assert plan.grep_only_matching_pieces(np.frombuffer(text, dtype=np.uint8), 50) == plan.grep_only_matching(d_text, len(text))
    plan.close()
    return plain


SMALL, LARGE = (1, 7), (64, 1000, 1 << 20)


def literal_of_class(gpu, want_mode, n):
    """(pattern, case_sensitive) of a single literal krep_gpu_split_mode() puts in this class under -o"""
    for cs in (True, False):
        for pat in (b"abba", b"ab", b"aba", b"abab"):
            if split_under_o(gpu, abi.Params([pat], case_sensitive=cs), n) == want_mode:
                return pat, cs
    raise AssertionError(("no literal of this class", want_mode))


@pytest.mark.parametrize("mode", ["PIECES", "CHAIN"])
def test_pieces_of_a_single_literal(gpu, tmp_path, mode):
    want_mode = {"PIECES": abi.SPLIT_PIECES, "CHAIN": abi.SPLIT_CHAIN}[mode]
    for n, pieces in ((900, SMALL), (2600, LARGE)):
        text = piece_text(3, n, b"abab \n")
        pat, cs = literal_of_class(gpu, want_mode, n)
        assert split_under_o(gpu, abi.Params([pat], case_sensitive=cs), n) == want_mode
        out = check_pieces(gpu, om.Case(f"pieces/{mode}/{n}", text, [pat], cs=cs), tmp_path, pieces, (False, True))
        assert out.count(b"\n") > (10 if n > 1000 else 0)  # (the stale rule is in force on the larger text)


def test_pieces_case_insensitive_and_whole_word(gpu, tmp_path):
    for n, pieces in ((900, SMALL), (2600, LARGE)):
        text = piece_text(4, n, b"abAB \n")
        assert check_pieces(gpu, om.Case(f"pieces/i/{n}", text, [b"abab"], cs=False), tmp_path, pieces)
        # -w: the byte in front of a piece's first byte decides ("b ab": with 1-byte pieces every match begins a piece)
        text = piece_text(5, n, b"ab  \n")
        out = check_pieces(gpu, om.Case(f"pieces/w/{n}", text, [b"ab"], ww=True), tmp_path, pieces)
        assert 0 < out.count(b"\n") < text.count(b"ab")  # -w passes some and refuses some
        assert check_pieces(gpu, om.Case(f"pieces/wi/{n}", text, [b"B"], ww=True, cs=False), tmp_path, pieces)


def test_pieces_of_a_dictionary_with_nested_patterns(gpu, tmp_path):
    import krep_amd
    for n, pieces in ((900, SMALL), (2600, LARGE)):
        text = piece_text(6, n, b"abc \n")
        out = check_pieces(gpu, om.Case(f"pieces/dict/{n}", text, [b"abcab", b"bca", b"ca", b"abc", b"b c"]), tmp_path, pieces, (False, True))
        assert out.count(b"\n") > (10 if n > 1000 else 0)
    plan = gpu.plan(abi.Params([b"ab", b"b"], max_count=5), only_matching=True)
    with pytest.raises(krep_amd.KrepGpuError, match="max_count"):
        plan.grep_only_matching_pieces(b"ab\nab\n", 4)


@pytest.mark.parametrize("max_count", [None, 1, 10, 11])
def test_pieces_with_max_count(gpu, tmp_path, max_count):
    for n, pieces in ((900, SMALL), (2600, LARGE)):
        text = piece_text(8, n, b"abab \n", tail=40)
        for pat, cs in (literal_of_class(gpu, abi.SPLIT_PIECES, n), literal_of_class(gpu, abi.SPLIT_CHAIN, n)):
            out = check_pieces(gpu, om.Case(f"pieces/m{max_count}/{n}", text, [pat], cs=cs, max_count=max_count), tmp_path, pieces)
            assert 0 < out.count(b"\n") <= (max_count or len(out))
            assert n < 1000 or (out.count(b"\n") == max_count if max_count else out.count(b"\n") > 11)  # the larger text holds more than 11


def test_pieces_and_the_three_stale_schedules(gpu, tmp_path):
    f = om.FILE + b":"
    # a long last line and 10 records in all: held to the end, then true numbers
    text = b"xa\nya\n" + b"a" + b"." * 50 + b"a" * 7
    out = check_pieces(gpu, om.Case("pieces/held-10", text, [b"a"]), tmp_path, SMALL + LARGE, (False, True))
    assert out.count(b"\n") == 10 and out.endswith(f + b"3:a\n")
    # the 11th record lies in the last line: held, then stale numbers
    out = check_pieces(gpu, om.Case("pieces/held-11", text + b".a", [b"a"]), tmp_path, SMALL + LARGE, (False, True))
    assert out.count(b"\n") == 11 and out.endswith(f + b"2:a\n")
    out = check_pieces(gpu, om.Case("pieces/held-11-m10", text + b".a", [b"a"], max_count=10), tmp_path, SMALL + LARGE)
    assert out.count(b"\n") == 10 and out.endswith(f + b"3:a\n")
    # the count passes 10 in front of the last line: nothing is held
    text = b"a\n" * 12 + b"." * 40 + b"aa"
    out = check_pieces(gpu, om.Case("pieces/stale-12", text, [b"a"]), tmp_path, SMALL + LARGE)
    assert out.endswith(f + b"12:a\n" + f + b"12:a\n")
    # all records behind the last newline, and no newline at all
    assert check_pieces(gpu, om.Case("pieces/all-behind", b"x\n" + b"a" * 11, [b"a"]), tmp_path, SMALL).endswith(f + b"1:a\n")
    assert check_pieces(gpu, om.Case("pieces/no-newline", b"a" * 12, [b"a"]), tmp_path, SMALL).count(b"\n") == 12
    # a final newline: nothing starts behind it
    assert check_pieces(gpu, om.Case("pieces/final-newline", b"a\n" * 12 + b"aa\n", [b"a"]), tmp_path, SMALL).endswith(f + b"13:a\n")


def test_what_the_driver_refuses(gpu):
    import krep_amd
    with pytest.raises(krep_amd.KrepGpuError, match="only_matching"):
        gpu.plan(abi.Params([b"ab"])).grep_only_matching_pieces(b"ab\nab\n", 4)
    whole = abi.Params([b"ab"], case_sensitive=False, count_lines=True)  # -c with -o through memchr_short_search: one window only
    assert split_under_o(gpu, whole, 6) == abi.SPLIT_WHOLE
    with pytest.raises(krep_amd.KrepGpuError, match="whole text in one window"):
        gpu.plan(whole, only_matching=True).grep_only_matching_pieces(b"ab\nab\n", 4)
    plan = gpu.plan(abi.Params([b"ab"]), only_matching=True)
    with pytest.raises(krep_amd.KrepGpuError, match="piece_bytes"):
        plan.grep_only_matching_pieces(b"ab\nab\n", 0)
    assert plan.grep_only_matching_pieces(b"", 4) == b"" and plan.grep_only_matching_pieces(b"ab\nab\n", 4, filename=b"f") == b"f:1:ab\nf:2:ab\n"
