"""krep_gpu_format_lines_window in plain Python: the line output of tests/color_line_model.py for a WINDOW of a text.

TEST INFRASTRUCTURE.  The contract (include/krep_gpu.h), seen from the buffer alone — the model never looks at a byte of the text
outside [global_base, global_base + text_len):
  1. the buffer holds text[global_base : global_base + text_len]; the records carry global offsets, ascending in start, every start
     inside the buffer, end >= start — anything else is refused;
  2. line_start of a record = one past the last newline in [global_base, start); with none it is 0 when global_base == 0, else
     the line starts in front of the buffer: not owned, the record is passed over;
  3. the call owns the lines with line_start in [own_lo, own_hi); records of other lines are passed over;
  4. line_end = the first newline at or after line_start inside the buffer; an owned matching line is complete when that newline
     exists and lies in front of records_hi, or when the buffer ends the text and records_hi == global_len (line_end = global_len
     for a last line without a newline);
  5. an incomplete line (at most one, the last owned one) is neither emitted nor counted; it is reported (global line_start + 1,
     index of its first record) if its index among the owned matching lines is < max_lines;
  6. the bytes, lines, lines_total and capped of the owned complete lines are color_line_model.ColorLines' on them.
"""
from __future__ import annotations

import color_line_model as cm
import line_model as lm

NO_LIMIT = lm.NO_LIMIT


class Refused(ValueError):
    pass


class Window:
    """what one call answers: data, lines, lines_total, capped, incomplete_line_start1, incomplete_first_record"""

    def __init__(self, text: bytes, records, global_base, text_len, own_lo, own_hi, records_hi, fmt=(b"", b"", b"", b""),
                 max_lines=None):
        glen, limit = len(text), (NO_LIMIT if max_lines is None else max_lines)
        end = global_base + text_len
        if not (global_base <= own_lo <= own_hi <= records_hi <= end <= glen):
            raise Refused("window")
        if own_lo == global_base and global_base != 0:
            raise Refused("no byte of left context")
        buf = text[global_base:end]  # all the model reads
        prev = None
        for s, e in records:
            if not (global_base <= s < end) or e < s or (prev is not None and prev > s):
                raise Refused("record list")
            prev = s
        ends_all = end == glen and records_hi == glen
        kept, open_line, open_first = [], None, len(records)
        for i, (s, e) in enumerate(records):
            a = buf.rfind(b"\n", 0, s - global_base) + 1
            if a == 0 and global_base != 0:
                continue                                  # rule 2: the line starts in front of the buffer
            if not (own_lo <= global_base + a < own_hi):
                continue                                  # rule 3: a neighbour's
            z = buf.find(b"\n", a)
            if (z >= 0 and global_base + z < records_hi) or ends_all:
                kept.append((s - global_base, e - global_base))
            elif open_line is None:
                open_line, open_first = global_base + a, i
            else:
                assert open_line == global_base + a       # rule 5: at most one line is incomplete
        m = cm.ColorLines(buf, kept, fmt, None if limit == NO_LIMIT else limit)
        self.data, self.lines, self.lines_total, self.capped = m.data, len(m.spans), m.lines_total, m.capped
        self.spans = [(global_base + a, global_base + z) for a, z in m.spans]
        report = open_line is not None and m.lines_total < limit
        self.incomplete_line_start1 = open_line + 1 if report else 0
        self.incomplete_first_record = open_first if report else len(records)


def records_in(records, lo, hi):
    """the part of a whole text's list a truthful window call is given: every record with lo <= start < hi"""
    return [r for r in records if lo <= r[0] < hi]


def truthful_reach(text: bytes, records, own_lo, own_hi):
    """the least records_hi (> the newline of the last owned matching line, or the text's length) with which a window that owns
    [own_lo, own_hi) leaves nothing incomplete"""
    need = own_hi
    for s, _ in records:
        a, z = lm.line_of(text, s)
        if own_lo <= a < own_hi:
            need = max(need, min(z + 1, len(text)))
    return need


def run_pieces(text: bytes, records, cuts, fmt=(b"", b"", b"", b""), max_lines=None, halo=None, slack=0):
    """The driver of the invariant: windows [c_i, c_i+1) over `cuts` (0 = c0 < ... < ck = len(text)), each with the byte of left
    context, max_lines passed on as what is left.  halo None: every buffer reaches as far as its last owned line needs (+ slack);
    halo = h: records_hi = buffer end = min(own_hi + h, len(text)), and a line reported incomplete is submitted again as a window
    of its own with the halo doubled until it completes.  A call cannot report an owned line whose FIRST record lies at or behind
    records_hi (no record of it is in its list): the driver looks at the line that is open at records_hi itself and, when the
    window owned it and did not report it, submits it whole.  -> (bytes, lines, lines_total, capped, windows, re-submissions)"""
    n, left = len(text), (NO_LIMIT if max_lines is None else max_lines)
    out, lines, total, capped, again = [], 0, 0, 0, 0

    def call(lo, hi, reach_to, left):
        base = max(lo - 1, 0)
        return Window(text, records_in(records, base, reach_to), base, reach_to - base, lo, hi, reach_to, fmt, left), base

    for lo, hi in zip(cuts, cuts[1:]):
        reach_to = min(truthful_reach(text, records, lo, hi) + slack, n) if halo is None else min(hi + halo, n)
        w, base = call(lo, hi, reach_to, left)
        out.append(w.data)
        lines, total, capped = lines + w.lines, total + w.lines_total, capped + w.capped
        if left != NO_LIMIT:
            left -= w.lines
        if w.incomplete_line_start1:
            assert halo is not None
            start = w.incomplete_line_start1 - 1
            h = 2 * max(reach_to - (start + 1), 1)  # (the line is longer than what the window saw of it: twice that)
            first = records_in(records, base, reach_to)[w.incomplete_first_record]
            assert lm.line_of(text, first[0])[0] == start
            while True:
                again += 1
                v, _ = call(start, start + 1, min(start + 1 + h, n), 1)
                if not v.incomplete_line_start1:
                    break
                assert start + 1 + h < n
                h *= 2
            assert v.lines == 1 and v.lines_total == 1
            out.append(v.data)
            lines, total, capped = lines + 1, total + 1, capped + v.capped
            if left != NO_LIMIT:
                left -= 1
        elif halo is not None and reach_to < n and lo <= text.rfind(b"\n", 0, reach_to) + 1 < hi and left > 0:
            start = text.rfind(b"\n", 0, reach_to) + 1  # the line open at records_hi: the window's, and none of its records seen
            z = text.find(b"\n", reach_to)
            v, _ = call(start, start + 1, n if z < 0 else z + 1, 1)
            assert not v.incomplete_line_start1
            out.append(v.data)
            lines, total, capped = lines + v.lines, total + v.lines_total, capped + v.capped
            if left != NO_LIMIT:
                left -= v.lines
    return b"".join(out), lines, total, capped, len(cuts) - 1, again
