"""krep -r -m N: the batch under a max_count (krep_gpu_set_batch_max_count) against what a caller could do before.

4096 items of 64 KiB of WORD TEXT (generator kind 5: 80-byte lines of Zipf-drawn words), searched for a frequent word, for the
1000-word dictionary and for the dictionary with -c.  Timed in ONE process, the roads alternating:
  (a) Engine.search_batch with max_count = 1 and = 10              — the call under test (the switch on)
  (b) the loop of Engine.search with the same max_count            — what a caller of the parent commit can do
  (c) Engine.search_batch without max_count                        — the same batch, uncut
and Engine.grep_batch (matching lines) at max_count = 1 against the same call without one: the bytes read back and the stage times.
Host-to-host, every call ends in a device synchronise, so the host clock around a call is its time.  One warm-up of each, then `reps`
alternating repeats; the median and the spread (min .. max) are reported, with the stage times of the library's own clocks
(krep_gpu_debug_batch_times, krep_gpu_debug_grep_batch_times).  (a) and (b) are compared item by item before anything is timed.
usage: python tools/batch_max_count_bench.py [items] [item_kib] [reps]          -> the table of profiles/batch_max_count.txt"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import krep_amd
import wordlist
from krep_amd import abi

n_items = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
item_bytes = (int(sys.argv[2]) if len(sys.argv) > 2 else 64) << 10
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 7
SEED, LINE = 20260930, 80

e = krep_amd.load()
assert e.device_count() >= 1 and e.available(), e.unavailable_reason()  # a measurement path that finds no GPU fails
e.set_batch_max_count(True)
W = wordlist.word_list()
blob = wordlist.pack(W)
whole = e.generate_host(n_items * item_bytes, 0, 5, SEED, blob, LINE)
items = [whole[i * item_bytes:(i + 1) * item_bytes] for i in range(n_items)]  # contiguous views: nothing is copied per call
names = [b"dir%02d/file%05d.txt" % (k % 64, k) for k in range(n_items)]
frequent = next(w for w in W if len(w) >= 4)  # the most frequent word of four bytes or more
DICT = wordlist.dictionary(W, "rare", n=1000)
JOBS = [("frequent word %s" % frequent.decode(), [frequent], {}), ("1000-word dictionary", DICT, {}),
        ("1000-word dictionary -c", DICT, dict(count_lines=True))]


def clock(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def mmm(v):
    return "%.1f (%.1f..%.1f)" % (statistics.median(v), min(v), max(v))


def stages(rows):
    """the median of every stage; the segment stage (index 2) with its spread"""
    return " / ".join(("%.2f (%.2f..%.2f)" % (statistics.median(v), min(v), max(v))) if k == 2 else "%.2f" % statistics.median(v)
                      for k, v in enumerate([[r[k] for r in rows] for k in range(len(rows[0]))]))


print(f"# {n_items} items x {item_bytes >> 10} KiB of word text = {n_items * item_bytes / 2**20:.0f} MiB, {reps} alternating repeats after one warm-up each")
print("# job | -m | (a) batch -m ms median (min..max) | (b) loop -m ms | (c) batch uncut ms | records scanned | records back (a) | "
      "(a) pack / scan / segment / read-back ms | (c) pack / scan / segment / read-back ms")
for name, pats, kw in JOBS:
    free = abi.Params(pats, **kw)
    for M in (1, 10):
        p = abi.Params(pats, max_count=M, **kw)
        assert e.batch_can_accelerate(p), e.last_error()
        a = lambda: e.search_batch(p, items, want_info=True)
        b = lambda: [e.search(p, it) for it in items]
        c = lambda: e.search_batch(free, items, want_info=True)
        (got, info), ref, _ = a(), b(), c()  # warm-up of the three, and the comparison
        for i, ((cnt, pos), (rc, rpos)) in enumerate(zip(got, ref)):
            assert cnt == rc and (kw.get("count_lines") or np.array_equal(pos, rpos)), (name, M, i, cnt, rc)
        back = sum(pos.shape[0] for _, pos in got)
        ta, tb, tc, sa, sc = [], [], [], [], []
        for _ in range(reps):
            t, _ = clock(a)
            ta.append(t)
            sa.append(e.batch_times())
            t, _ = clock(b)
            tb.append(t)
            t, _ = clock(c)
            tc.append(t)
            sc.append(e.batch_times())
        print(f"{name} | {M} | {mmm(ta)} | {mmm(tb)} | {mmm(tc)} | {info.total_records} | {back} | {stages(sa)} | {stages(sc)}")

print("# grep_batch, matching lines | -m | ms median (min..max) | bytes read back | pack / scan / segment / format / read-back ms")
for name, pats, kw in JOBS[:2]:
    rows = []
    for M in (1, None):
        p = abi.Params(pats, **kw) if M is None else abi.Params(pats, max_count=M, **kw)
        g = lambda p=p: e.grep_batch(p, items, names)
        data, _ = g()  # warm-up
        rows.append((M, g, len(data), [], []))
    for _ in range(reps):
        for M, g, _, t, s in rows:
            dt, _ = clock(g)
            t.append(dt)
            s.append(e.grep_batch_times())
    for M, _, nbytes, t, s in rows:
        print(f"{name} | {'none' if M is None else M} | {mmm(t)} | {nbytes} | {stages(s)}")
e.set_batch_max_count(False)
