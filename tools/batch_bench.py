"""A batch of small texts: krep_gpu_search_batch against the loop of one operator call per text.

4096 items of 64 KiB of WORD TEXT (generator kind 5: 80-byte lines of Zipf-drawn words), searched for a `Sherlock`-class literal
(an 8-byte word of the list) and for the 1000-word dictionary.  Timed in ONE process, alternating:
  (a) Engine.search_batch over the items                      — the call under test
  (b) the loop of Engine.search over the same items           — what a caller of the parent commit can do
Both are host-to-host: the items start in host memory and the counts and records end there, every call ends in a device
synchronise, so the host clock around a call is its time.  One warm-up of each, then `reps` alternating repeats; the median and
the spread (min .. max) of each are reported, their ratio, and the share of the batch's time spent in packing (gather into the
pinned ring + DMA), scan, segmentation and read-back (krep_gpu_debug_batch_times).  The results of (a) and (b) are compared item
by item before anything is timed.
usage: python tools/batch_bench.py [items] [item_kib] [reps]          -> the table of profiles/batch_vs_loop.txt"""
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
W = wordlist.word_list()
blob = wordlist.pack(W)
whole = e.generate_host(n_items * item_bytes, 0, 5, SEED, blob, LINE)
items = [whole[i * item_bytes:(i + 1) * item_bytes] for i in range(n_items)]  # contiguous views: nothing is copied per call
literal = next(w for w in wordlist.dictionary(W, "rare", n=300) if len(w) == 8)
JOBS = [("literal %s" % literal.decode(), [literal], {}), ("literal %s -c" % literal.decode(), [literal], dict(count_lines=True)),
        ("1000-word dictionary", wordlist.dictionary(W, "rare", n=1000), {}),
        ("1000-word dictionary -c", wordlist.dictionary(W, "rare", n=1000), dict(count_lines=True))]


def clock(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


print(f"# {n_items} items x {item_bytes >> 10} KiB of word text = {n_items * item_bytes / 2**20:.0f} MiB, {reps} alternating repeats after one warm-up each")
print("# job | batch ms median (min..max) | loop ms median (min..max) | loop / batch | records | scans | batch share: pack / scan / segment / read-back %")
for name, pats, kw in JOBS:
    p = abi.Params(pats, **kw)
    assert e.batch_can_accelerate(p), e.last_error()
    batch = lambda: e.search_batch(p, items, want_info=True)
    loop = lambda: [e.search(p, it) for it in items]
    (got, info), ref = batch(), loop()  # warm-up of both, and the comparison
    for i, ((c, pos), (rc, rpos)) in enumerate(zip(got, ref)):
        assert c == rc and (kw.get("count_lines") or np.array_equal(pos, rpos)), (name, i, c, rc)
    tb, tl, shares = [], [], []
    for _ in range(reps):
        t, _ = clock(batch)
        tb.append(t)
        shares.append(e.batch_times())
        t, _ = clock(loop)
        tl.append(t)
    mb, ml = statistics.median(tb), statistics.median(tl)
    sh = [statistics.median(s[k] for s in shares) for k in range(4)]
    tot = sum(sh) or 1.0
    print(f"{name} | {mb:.1f} ({min(tb):.1f}..{max(tb):.1f}) | {ml:.1f} ({min(tl):.1f}..{max(tl):.1f}) | {ml / mb:.2f} | "
          f"{info.total_records} | {info.scans} | " + " / ".join(f"{100 * x / tot:.0f}" for x in sh) +
          f"  (of {tot:.1f} ms inside the library; the rest is the Python binding)")
