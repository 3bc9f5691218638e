"""What the reference prints by default (`krep PATTERN FILE`, no -c, no -o, colour off): every line that holds the start of a
match, once.  A plain-Python statement of the rules, for the tests of krep_gpu_matching_lines / krep_gpu_format_lines.

TEST INFRASTRUCTURE.  The rules (tests/test_line_model_cpu.py pins them to the stock CLI):
  1. a record belongs to the line of its start: line_start = one past the last newline in [0, start), or 0; line_end = the
     first newline at or after line_start, or the text's length;
  2. each distinct line once, ascending, at most max_count lines;
  3. only the first 2048 records of a line take part in its bytes;
  4. the bytes of a line follow a cursor that starts at line_start: per record the text from the cursor to the record's start when
     the start lies behind the cursor, then the match cut at line_end, and the cursor jumps to the cut end (also backwards); a record
     whose cut match is empty is passed over; at the end the text from the cursor to line_end and a newline;
  5. `prefix` ("FILE:" or nothing) in front of every line.
"""
from __future__ import annotations

CAP = 2048
NO_LIMIT = (1 << 64) - 1


def line_of(text: bytes, start: int):
    a = text.rfind(b"\n", 0, start) + 1
    z = text.find(b"\n", a)
    return a, (len(text) if z < 0 else z)


def cut_to_max_count(emitted, max_count):
    """search_file(): the list is cut to its first max_count records in emission order, then ordered by (start, end)"""
    rec = [tuple(int(v) for v in r) for r in emitted]
    if max_count is not None and max_count != NO_LIMIT:
        rec = rec[:max_count]
    return sorted(rec)


class Lines:
    """spans[l] = (line_start, line_end); first_record[l] = index of line l's first record, one more entry closes the last emitted
    line; capped = emitted lines with more than 2048 records; lines_total = distinct lines before max_count; data = the bytes"""

    def __init__(self, text: bytes, records, prefix: bytes = b"", max_count=None):
        limit = NO_LIMIT if max_count is None else max_count
        groups = []  # (line_start, line_end, index of the first record, its records)
        for i, (s, e) in enumerate(records):
            a, z = line_of(text, s)
            if not groups or groups[-1][0] != a:
                groups.append((a, z, i, []))
            groups[-1][3].append((s, e))
        self.lines_total = len(groups)
        emitted = groups[:limit] if limit < len(groups) else groups
        self.spans = [(a, z) for a, z, _, _ in emitted]
        self.first_record = [g[2] for g in emitted]
        self.first_record.append(groups[len(emitted)][2] if len(emitted) < len(groups) else len(records))
        self.capped = sum(1 for g in emitted if len(g[3]) > CAP)
        out = []
        for a, z, _, recs in emitted:
            out.append(prefix)
            cur = a
            for s, e in recs[:CAP]:
                e = min(e, z)
                if s >= e:
                    continue
                if s > cur:
                    out.append(text[cur:s])
                out.append(text[s:e])
                cur = e
            if cur < z:
                out.append(text[cur:z])
            out.append(b"\n")
        self.data = b"".join(out)


def grep_output(text: bytes, emitted, prefix: bytes = b"", max_count=None) -> bytes:
    """the CLI's stdout for the records a search emitted (in emission order)"""
    return Lines(text, cut_to_max_count(emitted, max_count), prefix, max_count).data


# ---- the cases both test files share, the stock CLI that answers them, and the store of its answers ------------------------
import hashlib  # noqa: E402
import json  # noqa: E402
import os  # noqa: E402
import random  # noqa: E402
import subprocess  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "line_output.json")
FILE = b"<file>"  # stands for the haystack's path in a stored answer


class Case:
    def __init__(self, key, text, pats, cs=True, ww=False, no_simd=False, max_count=None, want=None):
        self.key, self.text, self.pats = key, bytes(text), [bytes(p) for p in pats]
        self.cs, self.ww, self.no_simd, self.max_count, self.want = cs, ww, no_simd, max_count, want

    def cli_args(self):
        a = ["-t", "1", "--color=never"] + (["--no-simd"] if self.no_simd else []) + ([] if self.cs else ["-i"])
        a += (["-w"] if self.ww else []) + (["-m", str(self.max_count)] if self.max_count is not None else [])
        if len(self.pats) == 1:
            return a + [self.pats[0]]
        for p in self.pats:
            a += ["-e", p]
        return a

    def params(self, abi):
        return abi.Params(self.pats, case_sensitive=self.cs, whole_word=self.ww,
                          max_count=abi.SIZE_MAX if self.max_count is None else self.max_count)

    def emitted(self, chk, abi):
        """the records the reference's search emits for this case (the compiled reference, function by function)"""
        p = self.params(abi)
        algo = abi.RA_AHO_CORASICK
        if len(self.pats) == 1:
            chk.o.lib.ko_set_force_no_simd(int(self.no_simd))
            try:
                algo = chk.select(p, abi.REF_AVX2)  # oracle/_ref/krep is the AVX2 build
            finally:
                chk.o.lib.ko_set_force_no_simd(0)
        return chk.call(algo, p, self.text)[1]


def table_cases():
    sh, ab = b"xx Sherlock yy", b"abababa tail"
    three = [b"Sherlock", b"lock", b"er"]
    return [
        Case("table/nested", sh, three, want=b"xx Sherlockerlock yy\n"),
        Case("table/overlap", ab, [b"aba"], no_simd=True, want=b"abaabaaba tail\n"),
        Case("table/over-newline", sh + b"\n" + ab, [b"yy\nab"], want=b"xx Sherlock yy\n"),
        Case("table/cap", b"a" * 3000, [b"a"], want=b"a" * 3000 + b"\n"),
        Case("table/cap-overlap", b"a" * 3000, [b"aa"], no_simd=True, want=b"aa" * 2048 + b"a" * 951 + b"\n"),
        Case("table/m1", sh, three, max_count=1, want=b"xx Sherlock yy\n"),
        Case("table/m2", sh, three, max_count=2, want=b"xx Sherlockerlock yy\n"),
    ]


def random_cases(count=240, seed=20261016):
    rng = random.Random(seed)
    out = []
    for k in range(count):
        alpha = rng.choice([b"ab\n", b"abA \n", b"abc_ \n", b"aAbB\n", b"ab", b"ab\n\n"])
        n = rng.choice([1, 2, 5, 17, 40, 200, 200, 1000, 3000])
        text = bytearray(rng.choice(alpha) for _ in range(n))
        if k % 3 == 0:
            text[-1] = 10          # a final newline
        elif k % 3 == 1 and text[-1] == 10:
            text[-1] = alpha[0]    # none
        if k % 7 == 0 and n > 4:
            text[n // 2] = text[n // 2 + 1] = 10  # an empty line
        text = bytes(text)
        letters = bytes(c for c in alpha if c != 10)

        def pick(m):
            m = min(m, n)
            where = rng.random()
            s = 0 if where < 0.2 else (n - m if where < 0.4 else rng.randrange(0, n - m + 1))  # offset 0 / up to text_len
            p = text[s:s + m]
            if where > 0.85 or p[:1] == b"\n" or not p:
                p = bytes(rng.choice(letters) for _ in range(m))
            return p

        kind = k % 6
        mc = rng.choice([None, None, None, 1, 2, 3, 7])
        if kind in (0, 1):       # one literal: the greedy family (SIMD) / all occurrences (--no-simd)
            out.append(Case(f"rand/{k}", text, [pick(rng.choice([1, 2, 3, 4, 6]))], no_simd=kind == 1, max_count=mc))
        elif kind == 2:
            out.append(Case(f"rand/{k}", text, [pick(rng.choice([1, 2, 3, 5]))], cs=False, max_count=mc))
        elif kind == 3:
            out.append(Case(f"rand/{k}", text, [pick(rng.choice([1, 2, 3]))], ww=True, cs=rng.random() < 0.7, max_count=mc))
        else:                    # a dictionary with nested patterns
            pats = [pick(rng.choice([3, 4, 6]))]
            while len(pats) < rng.randrange(2, 7):
                big = rng.choice(pats)
                if len(big) > 1 and rng.random() < 0.6:
                    a = rng.randrange(0, len(big))
                    p = big[a:rng.randrange(a + 1, len(big) + 1)]
                else:
                    p = pick(rng.choice([1, 2, 3, 5]))
                if p and p[:1] != b"\n" and p not in pats:
                    pats.append(p)
            out.append(Case(f"rand/{k}", text, pats, cs=rng.random() < 0.8, max_count=mc))
    return out


def run_cli(cli, case, path):
    """-> (exit code, stdout with the path replaced by FILE); `path` holds case.text"""
    r = subprocess.run([cli] + case.cli_args() + [str(path)], capture_output=True, timeout=120)
    return r.returncode, r.stdout.replace(str(path).encode() + b":", FILE + b":")


def digest(rc, out: bytes) -> str:
    return hashlib.sha256(b"%d:" % rc + out).hexdigest()[:16]


class Store:
    """Digests of the stock CLI's answers (tests/golden/line_output.json): a live answer must equal the stored one, and the stored
    one stands in where the CLI cannot be built.  KREP_RECORD_REF=1 stores the live answers instead."""

    def __init__(self):
        self.record = os.environ.get("KREP_RECORD_REF") == "1"
        self.live = 0    # answers the CLI gave in this process
        self.stored = 0  # answers taken from the file
        self.data = {}
        if os.path.exists(GOLDEN):
            with open(GOLDEN) as f:
                self.data = json.load(f)

    def want(self, key, live=None) -> str:
        if live is not None:
            self.live += 1
            if self.record:
                self.data[key] = live
            else:
                assert self.data.get(key, live) == live, f"{GOLDEN} [{key}] is stale"
            return live
        assert key in self.data, f"no reference CLI here and no stored answer: {GOLDEN} [{key}]"
        self.stored += 1
        return self.data[key]

    def save(self):
        if self.record:
            with open(GOLDEN, "w") as f:
                json.dump(dict(sorted(self.data.items())), f, indent=0, sort_keys=True)
                f.write("\n")
