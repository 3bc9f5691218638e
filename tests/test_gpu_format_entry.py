"""What the formatter entry points answer AROUND their kernels: the return code, the exact krep_gpu_last_error() text and every field
of *out, for each refusal in front of the first launch, for n == 0, the size query, a capacity one byte short, the exact capacity at
three alignments of d_out, and a refused record list.  Table-driven over krep_gpu_matching_lines, krep_gpu_format_lines, _lines_ex,
_lines_window, krep_gpu_format_matches, _matches_window and the two _items calls, through ctypes (the engine's wrappers turn a
refusal into an exception and drop *out).  The text is three short lines with two records; the pack is two items of one line each.
Expected bytes: line_model / color_line_model / lines_window_model / only_matching_model / matches_window_model /
batch_grep_model; expected messages: as the library's source words them."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import batch_grep_model as bg
import batch_model as bm
import color_line_model as cm
import line_model as lm
import lines_window_model as wm
import matches_window_model as mw
import only_matching_model as om
from krep_amd import abi

pytestmark = pytest.mark.gpu

GUARD = 0x5A
NONE = abi.SIZE_MAX
TEXT = b"one ab two\nno match here\nthree ab x"
RECS = [(4, 6), (31, 33)]
BEHIND = b"0123456789"  # what the whole text holds behind the buffer of the lines window: its last line is incomplete there
ITEMS = [b"xx ab yy", b"ab zz"]
ITEM_RECS = [[(3, 5)], [(0, 2)]]
NAMES = [b"a.txt", b"dir/b.txt"]
LINE_FMT = cm.strings(lm.FILE, True)
MATCH_FMT = om.strings(om.FILE, True)
MW_WIN = mw.Window(0, len(TEXT), len(TEXT), 5, mw.last_newline1(TEXT), 3, 1)
LIST_TEXT = "the record list is not ascending in start, or a record lies outside the text"
LIST_PACK = "the record list is not ascending in start, or a record does not lie inside one item"

assert len(TEXT) < 100 and TEXT.count(b"\n") == 2 and all(TEXT[s:e] == b"ab" for s, e in RECS)


@pytest.fixture(scope="module")
def lib():
    import krep_amd
    e = krep_amd.load()
    assert e.device_count() >= 1
    return e.lib


def flat(s, lead=""):
    """every field of a ctypes struct, nested ones by dotted name"""
    d = {}
    for name, _ in s._fields_:
        v = getattr(s, name)
        if isinstance(v, C.Structure):
            d.update(flat(v, lead + name + "."))
        else:
            d[lead + name] = int(v)
    return d


def on_device(data: bytes, shift=0):
    import torch
    t = torch.full((len(data) + shift + 64,), GUARD, dtype=torch.uint8, device="cuda")
    if data:
        t[shift:shift + len(data)] = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy())
    return t, t.data_ptr() + shift


def words_on_device(values):
    import torch
    a = np.asarray(values, dtype=np.uint64).reshape(-1)
    t = torch.from_numpy(np.concatenate([a, np.zeros(2, dtype=np.uint64)]).view(np.int64).copy()).cuda()
    return t, t.data_ptr()


def void(p):
    return C.c_void_p(p) if p else None


class Driver:
    """one entry point: how it is called with the arguments `a`, what it answers on the good input, how its messages name things"""
    strings = ()           # the fields of its format that the shared check looks at, in the order it looks at them
    null_text = "d_text / d_positions is NULL"
    list_text = LIST_TEXT
    is_pack = False
    win_first = True       # a NULL window / pack view is refused before the pointers and the strings are looked at

    def good(self):
        """-> the arguments of a call that succeeds (keeps what owns the device memory alive in a.keep)"""
        a = SimpleNamespace(keep=[], n=len(RECS), text_len=len(TEXT), fmt=self.format(), d_out=0, cap=0, out=self.Out(), no_out=False,
                            win=self.window(), no_win=False, d_item=0)
        t, a.d_text = on_device(TEXT, 3)
        r, a.d_pos = words_on_device(RECS)
        a.keep += [t, r]
        return a

    def window(self):
        return None

    def with_string(self, a, k, length, null):
        name = self.strings[k]
        if null:
            setattr(a.fmt, name, None)
        setattr(a.fmt, name + "_len", length)

    def zero(self):
        return flat(self.Out())


class MatchingLines(Driver):
    who, Out = "krep_gpu_matching_lines", abi.LinesOut

    def format(self):
        return None

    def call(self, L, a):  # d_out: the spans, `cap` of them; the first records lie behind them in the same block
        return L.krep_gpu_matching_lines(void(a.d_text), a.text_len, void(a.d_pos), a.n, NONE, void(a.d_out),
                                         void(a.d_out + 16 * a.cap if a.d_out else 0), a.cap, None if a.no_out else C.byref(a.out), None)

    def model(self):
        m = lm.Lines(TEXT, RECS)
        data = np.asarray(m.spans, dtype=np.uint64).tobytes() + np.asarray(m.first_record, dtype=np.uint64).tobytes()
        return data, dict(self.zero(), lines=len(m.spans), lines_total=m.lines_total, capped_lines=m.capped)


class FormatLines(Driver):
    who, Out = "krep_gpu_format_lines", abi.LinesOut
    strings = ("prefix",)
    null_string, long_string = "prefix is NULL", "a prefix of 1048576 bytes"

    def format(self):
        return SimpleNamespace(prefix=lm.FILE + b":", prefix_len=len(lm.FILE) + 1)

    def call(self, L, a):
        return L.krep_gpu_format_lines(void(a.d_text), a.text_len, void(a.d_pos), a.n, NONE, a.fmt.prefix, a.fmt.prefix_len, void(a.d_out),
                                       a.cap, None if a.no_out else C.byref(a.out), None)

    def model(self):
        m = lm.Lines(TEXT, RECS, lm.FILE + b":")
        return m.data, dict(self.zero(), lines=len(m.spans), lines_total=m.lines_total, out_bytes=len(m.data), capped_lines=m.capped)


class FormatLinesEx(Driver):
    who, Out = "krep_gpu_format_lines_ex", abi.LinesOut
    strings = ("prefix", "before_match", "after_match", "line_close")
    null_string, long_string = "a string of the format is NULL", "a format string of 1048576 bytes"

    def format(self):
        return abi.LineFormat(*LINE_FMT)

    def call(self, L, a):
        return L.krep_gpu_format_lines_ex(void(a.d_text), a.text_len, void(a.d_pos), a.n, NONE, C.byref(a.fmt), void(a.d_out), a.cap,
                                          None if a.no_out else C.byref(a.out), None)

    def model(self):
        m = cm.ColorLines(TEXT, RECS, LINE_FMT)
        return m.data, dict(self.zero(), lines=len(m.spans), lines_total=m.lines_total, out_bytes=len(m.data), capped_lines=m.capped)


class FormatLinesWindow(FormatLinesEx):
    who, Out = "krep_gpu_format_lines_window", abi.LinesWindowOut
    list_text = "the record list is not ascending in start, or a record lies outside the buffer"
    win_first = False

    def window(self):  # the buffer is the front of a longer text: the third line has no newline in it and is reported incomplete
        return abi.LinesWindow(0, len(TEXT + BEHIND), 0, len(TEXT), len(TEXT))

    def call(self, L, a):
        return L.krep_gpu_format_lines_window(void(a.d_text), a.text_len, None if a.no_win else C.byref(a.win), void(a.d_pos), a.n, NONE,
                                              C.byref(a.fmt), void(a.d_out), a.cap, None if a.no_out else C.byref(a.out), None)

    def model(self):
        m = wm.Window(TEXT + BEHIND, RECS, 0, len(TEXT), 0, len(TEXT), len(TEXT), LINE_FMT)
        assert (m.lines, m.incomplete_line_start1, m.incomplete_first_record) == (1, 26, 1)
        return m.data, {"lines.lines": m.lines, "lines.lines_total": m.lines_total, "lines.out_bytes": len(m.data),
                        "lines.capped_lines": m.capped, "lines.overflow": 0, "incomplete_line_start1": m.incomplete_line_start1,
                        "incomplete_first_record": m.incomplete_first_record}


class FormatMatches(Driver):
    who, Out = "krep_gpu_format_matches", abi.MatchesOut
    strings = ("prefix", "before_number", "after_number", "after_match")
    null_string, long_string = "a string of the format is NULL", "a format string of 1048576 bytes"

    def format(self):
        return abi.MatchFormat(*MATCH_FMT)

    def call(self, L, a):
        return L.krep_gpu_format_matches(void(a.d_text), a.text_len, void(a.d_pos), a.n, NONE, C.byref(a.fmt), void(a.d_out), a.cap,
                                         None if a.no_out else C.byref(a.out), None)

    def model(self):
        data = om.only_matching_output(TEXT, RECS, MATCH_FMT)
        return data, dict(self.zero(), items=len(RECS), out_bytes=len(data))


class FormatMatchesWindow(FormatMatches):
    who, Out = "krep_gpu_format_matches_window", abi.MatchesWindowOut
    list_text = "the record list is not ascending in start, or a record lies outside the buffer or outruns it"

    def window(self):  # carries come in, and the stale rule is on: the record behind the last newline prints the first one's number
        return abi.MatchesWindow(*MW_WIN, 0)

    def call(self, L, a):
        return L.krep_gpu_format_matches_window(void(a.d_text), a.text_len, None if a.no_win else C.byref(a.win), void(a.d_pos), a.n, NONE,
                                                C.byref(a.fmt), void(a.d_out), a.cap, None if a.no_out else C.byref(a.out), None)

    def model(self, recs=RECS):
        m = mw.window(TEXT, MW_WIN, recs, MATCH_FMT)
        return m.data, {"matches.items": m.items, "matches.out_bytes": len(m.data), "matches.overflow": 0,
                        "newlines_before_count_to": m.newlines_before_count_to, "stale_line": m.stale_line}


class PackDriver(Driver):
    null_text = "d_pack / d_positions is NULL"
    list_text = LIST_PACK
    is_pack = True
    null_string, long_string = "a string of the format is NULL", "a format string of 1048576 bytes"

    def good(self):
        pack, off = bm.pack(ITEMS)
        rec = bg.pack_records(ITEMS, ITEM_RECS)
        prefixes = [bg.prefix(nm, self.mode, True) for nm in NAMES]
        a = SimpleNamespace(keep=[], n=int(rec.shape[0]), text_len=int(pack.size), fmt=self.format(), d_out=0, cap=0, out=self.Out(),
                            no_out=False, win=None, no_win=False)
        t, a.d_text = on_device(pack.tobytes(), 3)
        r, a.d_pos = words_on_device(rec)
        o, d_off = words_on_device(off)
        b, d_blob = on_device(b"".join(prefixes))
        p, d_poff = words_on_device(np.concatenate([[0], np.cumsum([len(x) for x in prefixes])]))
        i, a.d_item = words_on_device([NONE] * (len(ITEMS) + 1))
        a.win = abi.PackView(d_off, len(ITEMS), d_blob, d_poff)
        a.keep += [t, r, o, b, p]
        a.item = i
        return a

    def call(self, L, a):
        return self.entry(L)(void(a.d_text), a.text_len, None if a.no_win else C.byref(a.win), void(a.d_pos), a.n, C.byref(a.fmt),
                             void(a.d_out), a.cap, void(a.d_item), None if a.no_out else C.byref(a.out), None)

    def item_offsets(self):
        want, where = bg.definition(ITEMS, ITEM_RECS, NAMES, self.mode, True)
        return [o for o, _ in where] + [len(want)]


class FormatLinesItems(PackDriver):
    who, Out, mode = "krep_gpu_format_lines_items", abi.LinesOut, "lines"
    strings = ("before_match", "after_match", "line_close")

    def entry(self, L):
        return L.krep_gpu_format_lines_items

    def format(self):
        return abi.LineFormat(b"", *bg.strings("lines", True))

    def model(self):
        data, _ = bg.definition(ITEMS, ITEM_RECS, NAMES, "lines", True)
        return data, dict(self.zero(), lines=2, lines_total=2, out_bytes=len(data))


class FormatMatchesItems(PackDriver):
    who, Out, mode = "krep_gpu_format_matches_items", abi.MatchesOut, "matches"
    strings = ("before_number", "after_number", "after_match")

    def entry(self, L):
        return L.krep_gpu_format_matches_items

    def format(self):
        return abi.MatchFormat(b"", *bg.strings("matches", True))

    def model(self):
        data, _ = bg.definition(ITEMS, ITEM_RECS, NAMES, "matches", True)
        return data, dict(self.zero(), items=2, out_bytes=len(data))


DRIVERS = [MatchingLines(), FormatLines(), FormatLinesEx(), FormatLinesWindow(), FormatMatches(), FormatMatchesWindow(), FormatLinesItems(),
           FormatMatchesItems()]
IDS = [d.who[len("krep_gpu_"):] for d in DRIVERS]


def answer(lib, d, a, rc, error, fields):
    """one call: the return code, the error text and *out, which held 0x77 in every byte before"""
    lib.krep_gpu_clear_error()
    C.memset(C.byref(a.out), 0x77, C.sizeof(a.out))
    got = d.call(lib, a)
    text = (lib.krep_gpu_last_error() or b"").decode()
    assert (got, text) == (rc, error), (d.who, got, text)
    if not a.no_out:
        assert flat(a.out) == fields, (d.who, flat(a.out), fields)


def refused(lib, d, a, why):
    answer(lib, d, a, 2, d.who + ": " + why, d.zero())


def out_block(size, misalign=0, guard=32):
    """a device block of GUARD bytes and the offset in it of `size` bytes that begin `misalign` behind a 16-byte boundary"""
    import torch
    t = torch.full((16 + guard + size + guard + 16,), GUARD, dtype=torch.uint8, device="cuda")
    return t, guard + (misalign - (t.data_ptr() + guard)) % 16


@pytest.mark.parametrize("d", DRIVERS, ids=IDS)
def test_refusals_in_front_of_the_first_launch(lib, d):
    a = d.good()
    a.no_out = True
    answer(lib, d, a, 2, d.who + ": out is NULL", None)
    if a.win is not None:  # a NULL window / pack view together with a NULL text and a NULL string: which of the three is reported
        no_win = "the pack view is NULL" if d.is_pack else "win is NULL"
        a = d.good()
        a.no_win = True
        refused(lib, d, a, no_win)
        a.d_text = 0
        refused(lib, d, a, no_win if d.win_first else d.null_text)
        a = d.good()
        a.no_win = True
        d.with_string(a, 0, 1, True)
        refused(lib, d, a, no_win if d.win_first else d.null_string)
    for null in ("d_text", "d_pos"):
        a = d.good()
        setattr(a, null, 0)
        refused(lib, d, a, d.null_text)
    a = d.good()
    a.n = 1 << 40  # refused before anything is read through the pointers
    refused(lib, d, a, "1099511627776 records are more than one call takes")
    if d.is_pack:  # the pack's own rule stands in front of the strings'
        a = d.good()
        a.fmt.prefix_len = 1
        d.with_string(a, 0, 1, True)
        refused(lib, d, a, "fmt->prefix must be empty: the prefixes of a pack are per item (krep_gpu_pack_view_t)")
        a = d.good()
        a.win.n_items = 0
        refused(lib, d, a, "records on a pack without items")


@pytest.mark.parametrize("d", [x for x in DRIVERS if x.strings], ids=[i for x, i in zip(DRIVERS, IDS) if x.strings])
def test_format_strings(lib, d):
    last = len(d.strings) - 1
    for k in sorted({0, last}):
        a = d.good()
        d.with_string(a, k, 1, True)
        refused(lib, d, a, d.null_string)
        a = d.good()
        d.with_string(a, k, 1 << 20, False)  # (refused before the string is read)
        refused(lib, d, a, d.long_string)
    if last:  # two strings that break one rule each: the string in front decides, not the rule
        a = d.good()
        d.with_string(a, 0, 1, True)
        d.with_string(a, last, 1 << 20, False)
        refused(lib, d, a, d.null_string)
        a = d.good()
        d.with_string(a, 0, 1 << 20, False)
        d.with_string(a, last, 1, True)
        refused(lib, d, a, d.long_string)
    a = d.good()  # a string that is NULL and too long at once
    d.with_string(a, last, 1 << 20, True)
    refused(lib, d, a, d.null_string)


def item_words(a):
    return a.item.cpu().numpy().view(np.uint64)[:len(ITEMS) + 1].tolist()


def n_zero_fields(d):
    if isinstance(d, FormatMatchesWindow):  # the one call that still runs on the buffer: its carries go out
        return d.model([])[1]
    return d.zero()


@pytest.mark.parametrize("d", DRIVERS, ids=IDS)
def test_no_records(lib, d):
    a = d.good()
    a.n = 0
    t, at = out_block(64)
    a.d_out, a.cap = t.data_ptr() + at, 4 if isinstance(d, MatchingLines) else 64
    answer(lib, d, a, 0, "", n_zero_fields(d))
    assert bool((t == GUARD).all())
    if d.is_pack:
        assert item_words(a) == [0] * (len(ITEMS) + 1)
    a = d.good()  # ... and the pointers are not looked at then
    a.n, a.d_pos = 0, 0
    if not isinstance(d, FormatMatchesWindow):
        a.d_text = 0
    answer(lib, d, a, 0, "", n_zero_fields(d))


@pytest.mark.parametrize("d", DRIVERS, ids=IDS)
def test_sizes_overflow_and_bytes(lib, d):
    data, fields = d.model()
    units = fields["lines"] if isinstance(d, MatchingLines) else len(data)  # the capacity counts lines there, bytes elsewhere
    overflow = next(k for k in fields if k.endswith("overflow"))
    assert units > 1 and (isinstance(d, MatchingLines) or len(data) > 32)
    # the size query
    a = d.good()
    answer(lib, d, a, 0, "", fields)
    if d.is_pack:  # (the item offsets are written by every call that gets that far)
        assert item_words(a) == d.item_offsets()
    a = d.good()
    t, at = out_block(len(data))
    a.d_out = t.data_ptr() + at  # ... also with a buffer of no capacity
    answer(lib, d, a, 0, "", fields)
    assert bool((t == GUARD).all())
    # one short
    a = d.good()
    a.d_out, a.cap = t.data_ptr() + at, units - 1
    answer(lib, d, a, 0, "", dict(fields, **{overflow: 1}))
    assert bool((t == GUARD).all())
    if d.is_pack:
        assert item_words(a) == d.item_offsets()
    # exact, d_out at three offsets from a 16-byte boundary
    for misalign in (0,) if isinstance(d, MatchingLines) else (0, 1, 15):
        a = d.good()
        t, at = out_block(len(data), misalign)
        a.d_out, a.cap = t.data_ptr() + at, units
        assert a.d_out % 16 == misalign
        answer(lib, d, a, 0, "", fields)
        got = t.cpu().numpy()
        assert got[at:at + len(data)].tobytes() == data, (d.who, misalign)
        assert (got[:at] == GUARD).all() and (got[at + len(data):] == GUARD).all()
        if d.is_pack:
            assert item_words(a) == d.item_offsets()


@pytest.mark.parametrize("d", DRIVERS, ids=IDS)
def test_a_descending_list(lib, d):
    a = d.good()
    rec = bg.pack_records(ITEMS, ITEM_RECS).tolist() if d.is_pack else RECS
    r, a.d_pos = words_on_device(rec[::-1])
    t, at = out_block(256)
    a.d_out, a.cap = t.data_ptr() + at, 8 if isinstance(d, MatchingLines) else 256
    refused(lib, d, a, d.list_text)  # (the window calls had filled fields of *out by then: they are taken back)
    assert bool((t == GUARD).all())
    if d.is_pack:
        assert item_words(a) == [NONE] * (len(ITEMS) + 1)
    a = d.good()  # the library works on behind a refusal
    answer(lib, d, a, 0, "", d.model()[1])
