"""One call of krep_gpu_format_matches_window in plain Python: the bytes, `items` and the two carries of ONE window, from the
window's own inputs only (the buffer, where it lies in the text, the carries in).  For the tests of the call and of
Plan.grep_only_matching_pieces.

TEST INFRASTRUCTURE.  The rules (include/krep_gpu.h; tests/test_matches_window_model_cpu.py chains windows and compares them with
only_matching_model.only_matching_output on the whole text, which is pinned to the stock CLI):
  1. the buffer holds text[global_base : global_base + len(buf)]; the records carry offsets in the whole text;
  2. record i < min(n, max_items) prints  prefix before_number LINE ":" after_number MATCH after_match "\\n", MATCH being
     text[start : min(end, global_len)] with every newline a blank;
  3. the true LINE is 1 + newlines_before + the newlines of the buffer in front of the start;
  4. with stale_rule and a last_newline1, a record with start >= last_newline1 prints S: the largest true LINE among ALL the
     list's records with start < last_newline1, else the stale_line that came in, else 1;
  5. carries out: stale_line = S before the fallback to 1; newlines_before_count_to = newlines_before + the newlines of the
     buffer in front of count_to.
"""
from __future__ import annotations

from collections import namedtuple

MAX_TEXT = 10 ** 16

Window = namedtuple("Window", "global_base global_len count_to newlines_before last_newline1 stale_line stale_rule")
Out = namedtuple("Out", "data items newlines_before_count_to stale_line")


class Refused(Exception):
    """what the call answers with 2"""


def window(buf: bytes, win: Window, records, fmt=(b"", b"", b"", b""), max_items=None) -> Out:
    gb, glen, n = win.global_base, win.global_len, len(buf)
    if glen >= MAX_TEXT or gb + n > glen:
        raise Refused("the buffer is not inside the text")
    if not gb <= win.count_to <= gb + n:
        raise Refused("count_to outside the buffer")
    if win.last_newline1 > glen:
        raise Refused("last_newline1 behind the text")
    if len(records) >= 1 << 40 or any(len(s) > 1 << 20 for s in fmt):
        raise Refused("too many records / a format string too long")
    before = None
    for s, e in records:
        if (before is not None and before > s) or not gb <= s < gb + n or e < s or min(e, glen) > gb + n:
            raise Refused("the record list is not ascending in start, or a record lies outside the buffer or outruns it")
        before = s
    if win.newlines_before + buf.count(b"\n") + 1 >= MAX_TEXT or win.stale_line >= MAX_TEXT:
        raise Refused("a line number of more than 16 digits")
    true = [1 + win.newlines_before + buf.count(b"\n", 0, s - gb) for s, _ in records]
    mine = max([ln for (s, _), ln in zip(records, true) if s < win.last_newline1], default=0)
    stale_out = mine if mine else win.stale_line
    prefix, head, mid, tail = fmt
    shown = len(records) if max_items is None else min(len(records), max_items)
    parts = []
    for (s, e), ln in list(zip(records, true))[:shown]:
        if win.stale_rule and win.last_newline1 and s >= win.last_newline1:
            ln = stale_out if stale_out else 1
        parts.append(prefix + head + b"%d:" % ln + mid + buf[s - gb:min(e, glen) - gb].replace(b"\n", b" ") + tail + b"\n")
    return Out(b"".join(parts), shown, win.newlines_before + buf.count(b"\n", 0, win.count_to - gb), stale_out)


def last_newline1(text: bytes) -> int:
    return text.rfind(b"\n") + 1


def buffer_of(text: bytes, records, lo=None):
    """(global_base, the smallest buffer that holds these records) — from `lo` when the list is empty"""
    if not records:
        return (lo or 0), b""
    base = records[0][0]
    end = max(max(min(e, len(text)) for _, e in records), records[-1][0] + 1)
    return base, text[base:end]


def chain(text: bytes, records, cuts, fmt=(b"", b"", b"", b""), max_items=None, stale_rule=None, call=None):
    """The invariant: the list cut at the record indices `cuts` (ascending, repeats make empty windows), every sub-list in the
    smallest buffer that holds it, count_to = the next buffer's global_base, the carries chained -> (bytes, items).
    call(buf, win, records, fmt, max_items) -> Out: the window itself (this model's by default, the device's in the GPU tests)"""
    call = call or window
    rule = len(records) > 10 if stale_rule is None else stale_rule
    edges = [0] + list(cuts) + [len(records)]
    subs = [records[a:b] for a, b in zip(edges[:-1], edges[1:])]
    bufs, at = [], 0
    for sub in subs:
        base, buf = buffer_of(text, sub, at)
        bufs.append((base, buf))
        at = base
    nl, stale, left, out, items = 0, 0, max_items, [], 0
    if bufs:
        nl = text.count(b"\n", 0, bufs[0][0])  # (what lies in front of the first buffer is the caller's to count)
    for k, (sub, (base, buf)) in enumerate(zip(subs, bufs)):
        nxt = bufs[k + 1][0] if k + 1 < len(bufs) else base + len(buf)
        count_to = min(max(nxt, base), base + len(buf))
        r = call(buf, Window(base, len(text), count_to, nl, last_newline1(text), stale, int(rule)), sub, fmt, left)
        out.append(r.data)
        items += r.items
        if left is not None:
            left -= r.items
        stale = r.stale_line
        nl = r.newlines_before_count_to + text.count(b"\n", count_to, max(nxt, count_to))  # a gap between two buffers
    return b"".join(out), items
