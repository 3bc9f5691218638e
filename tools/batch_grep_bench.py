"""The grep output of a batch: krep_gpu_grep_batch against the search alone and against the per-item loop.

The workload of DESIGN.md §9.3: 4096 items of 64 KiB of WORD TEXT (generator kind 5: 80-byte lines of Zipf-drawn words), searched for
an 8-byte word of the list and for the 1000-word dictionary, printed as matching lines and as -o.  Timed in ONE process, the roads
alternating:
  (a) Engine.grep_batch over the items                                   — the call under test: FILE:line / FILE:LINE:match per item
  (b) Engine.search_batch over the same items                            — the search alone, as the parent commit does it: (a) - (b)
                                                                           is what formatting adds to a batch
  (c) the loop of Plan.grep_lines / Plan.grep_only_matching per item     — what a caller of the parent commit must do to get the same
                                                                           bytes from the device: one upload, two scans and one
                                                                           formatter call per item
All three start from items in host memory and end with their result in host memory; every call ends in a device synchronise, so the
host clock around a call is its time.  One warm-up of each, then `reps` alternating repeats; medians with min .. max, and the library's
own stage breakdown of (a) (krep_gpu_debug_grep_batch_times).  The bytes of (a) and (c) are compared before anything is timed.
usage: python tools/batch_grep_bench.py [items] [item_kib] [reps]          -> the table of profiles/batch_grep_vs_loop.txt"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch

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
names = [b"dir%02d/file%05d.txt" % (k % 64, k) for k in range(n_items)]
literal = next(w for w in wordlist.dictionary(W, "rare", n=300) if len(w) == 8)
words = wordlist.dictionary(W, "rare", n=1000)
JOBS = [("literal %s, lines" % literal.decode(), [literal], False), ("literal %s, -o" % literal.decode(), [literal], True),
        ("1000-word dictionary, lines", words, False), ("1000-word dictionary, -o", words, True)]


def clock(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def med(ts):
    return f"{statistics.median(ts):.1f} ({min(ts):.1f}..{max(ts):.1f})"


print(f"# {n_items} items x {item_bytes >> 10} KiB of word text = {n_items * item_bytes / 2**20:.0f} MiB, {reps} alternating repeats after one warm-up each")
print("# job | (a) grep_batch ms median (min..max) | (b) search_batch ms | (c) per-item loop ms | (a) - (b) | (c) / (a) | output bytes | "
      "records | (a) inside the library: pack / scan / segment / format / read-back ms")
for name, pats, om in JOBS:
    p = abi.Params(pats)
    cfg = e.default_config()
    cfg.only_matching = int(om)
    plan = e.plan(p, only_matching=om)
    dev = torch.empty(item_bytes, dtype=torch.uint8, device="cuda")

    def grep():
        return e.grep_batch(p, items, names, cfg=cfg, want_info=True)

    def search():
        return e.search_batch(p, items, cfg=cfg)

    def loop():
        out = []
        for it, nm in zip(items, names):
            dev.copy_(torch.from_numpy(it))
            out.append(plan.grep_only_matching(dev.data_ptr(), item_bytes, filename=nm) if om else
                       plan.grep_lines(dev.data_ptr(), item_bytes, filename=nm))
        return b"".join(out)

    (got, per, info), _, ref = grep(), search(), loop()  # warm-up of the three, and the comparison
    assert got == ref, (name, len(got), len(ref))
    ta, tb, tc, stages = [], [], [], []
    for _ in range(reps):
        t, _ = clock(grep)
        ta.append(t)
        stages.append(e.grep_batch_times())
        t, _ = clock(search)
        tb.append(t)
        t, _ = clock(loop)
        tc.append(t)
    st = [statistics.median(s[k] for s in stages) for k in range(5)]
    ma, mb, mc = statistics.median(ta), statistics.median(tb), statistics.median(tc)
    print(f"{name} | {med(ta)} | {med(tb)} | {med(tc)} | {ma - mb:.1f} | {mc / ma:.1f} | {len(got)} | {info.total_records} | "
          + " / ".join(f"{x:.1f}" for x in st))
    plan.close()
