"""The matching lines and the -o output on the device, timed: krep_gpu_matching_lines, krep_gpu_format_lines, its coloured
sibling krep_gpu_format_lines_ex (the reference's --color=always strings) and krep_gpu_format_matches beside krep_gpu_line_numbers (the in-tree primitive of the same shape) on the same record list and text,
alternating, in ONE process with the text resident.
Events around the calls, warmed up.  Beside them the floor from the bytes moved: the text once + 16 B per record + 2 x out_bytes
at the measured streaming rate (bench.HBM_MEASURED_GBS).
--windows K adds a row: the same text formatted as K windows of text/K bytes through krep_gpu_format_lines_window (each window's buffer a
slice of the resident text, 4 KiB of left context, a 1 MiB halo, its records a slice of the one list), the K calls of a repetition summed;
and one for the -o form through krep_gpu_format_matches_window (buffer [lo, hi + 4 KiB), the records that start in [lo, hi), carries chained).
usage: python tools/lines_bench.py [--gib 32] [--reps 9] [--warmup 2] [--only literal8|ac1000] [--windows 8] [--out profiles/lines_on_device.txt]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=32.0)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default=None)
    ap.add_argument("--windows", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lines_on_device.txt"))
    args = ap.parse_args()
    import torch
    import bench
    import krep_amd
    from krep_amd import abi
    eng = krep_amd.load()
    n = int(args.gib * (1 << 30))
    lines = [f"# tools/lines_bench.py --gib {args.gib:g} --reps {args.reps} --warmup {args.warmup}: one process, text resident, "
             "events around each call (the calls synchronise), calls alternating",
             f"# {torch.cuda.get_device_name(0)}; floor = (text + 16 B x records + 2 x out_bytes) / {bench.HBM_MEASURED_GBS:g} GB/s; "
             "ms as median [min .. max]"]
    buf = torch.empty(n + 64, dtype=torch.uint8, device="cuda")
    for name in ("literal8", "ac1000"):
        if args.only and args.only != name:
            continue
        wl = bench.workload(name)
        pats = wl["patterns"]
        plant = wl["plant"] if wl["plant"] is not None else bench.pack_dict(pats)
        eng.generate(buf.data_ptr(), n, 0, wl["kind"], wl.get("seed", bench.SEED), plant, wl["period"])
        plan = eng.plan(abi.Params(pats))
        cap = int(plan.scan(buf.data_ptr(), n).total_matches) + 16
        pos = torch.empty(2 * cap, dtype=torch.int64, device="cuda")
        out = plan.scan(buf.data_ptr(), n, d_positions=pos.data_ptr(), capacity=cap)
        assert not out.overflow
        m = int(out.stored)
        if len(pats) > 1:
            eng.order_by_start(pos.data_ptr(), m, n)
        prefix = b"corpus.txt:"
        q = eng.format_lines(buf.data_ptr(), n, pos.data_ptr(), m, abi.SIZE_MAX, prefix)
        L, nbytes = int(q.lines), int(q.out_bytes)
        lineno = torch.empty(m, dtype=torch.int64, device="cuda")
        spans = torch.empty(2 * L, dtype=torch.int64, device="cuda")
        first = torch.empty(L + 1, dtype=torch.int64, device="cuda")
        fmt = abi.MatchFormat(prefix)
        obytes = int(eng.format_matches(buf.data_ptr(), n, pos.data_ptr(), m, abi.SIZE_MAX, fmt).out_bytes)
        cfmt = krep_amd.engine.line_format(prefix[:-1], True)
        cbytes = int(eng.format_lines_ex(buf.data_ptr(), n, pos.data_ptr(), m, abi.SIZE_MAX, cfmt).out_bytes)
        dst = torch.empty(max(nbytes, obytes, cbytes) + 64, dtype=torch.uint8, device="cuda")
        calls = {
            "krep_gpu_line_numbers": lambda: eng.line_numbers(buf.data_ptr(), n, pos.data_ptr(), m, lineno.data_ptr()),
            "krep_gpu_matching_lines": lambda: eng.matching_lines(buf.data_ptr(), n, pos.data_ptr(), m, abi.SIZE_MAX, spans.data_ptr(),
                                                                  first.data_ptr(), L),
            "krep_gpu_format_lines": lambda: eng.format_lines(buf.data_ptr(), n, pos.data_ptr(), m, abi.SIZE_MAX, prefix, dst.data_ptr(),
                                                              nbytes),
            "krep_gpu_format_lines_ex": lambda: eng.format_lines_ex(buf.data_ptr(), n, pos.data_ptr(), m, abi.SIZE_MAX, cfmt,
                                                                    dst.data_ptr(), cbytes),
            "krep_gpu_format_matches": lambda: eng.format_matches(buf.data_ptr(), n, pos.data_ptr(), m, abi.SIZE_MAX, fmt, dst.data_ptr(),
                                                                  obytes),
        }
        if args.windows:
            # the windows of the resident text: buffer [lo - 4 KiB, hi + 1 MiB), the records with base <= start < records_hi, the
            # output of window k behind that of window k - 1; checked once against the whole-text call's bytes
            K, halo = args.windows, 1 << 20
            starts = pos[: 2 * m].view(-1, 2)[:, 0].contiguous()
            wins, at = [], 0
            for k in range(K):
                lo, hi = n * k // K, n * (k + 1) // K
                base, end = max(lo - 4096, 0), min(hi + halo, n)
                i0, i1 = (int(x) for x in torch.searchsorted(starts, torch.tensor([base, end], dtype=torch.int64, device="cuda")))
                win = abi.LinesWindow(base, n, lo, hi, end)
                r = eng.format_lines_window(buf.data_ptr() + base, end - base, win, pos.data_ptr() + 16 * i0, i1 - i0, abi.SIZE_MAX, cfmt)
                assert not r.incomplete_line_start1
                wins.append((base, end, win, i0, i1, at, int(r.lines.out_bytes)))
                at += int(r.lines.out_bytes)
            assert at == cbytes, (at, cbytes)
            dst2 = torch.empty(cbytes + 64, dtype=torch.uint8, device="cuda")

            def windows():
                for base, end, win, i0, i1, at, size in wins:
                    eng.format_lines_window(buf.data_ptr() + base, end - base, win, pos.data_ptr() + 16 * i0, i1 - i0, abi.SIZE_MAX, cfmt,
                                            dst2.data_ptr() + at, size)
            calls["krep_gpu_format_lines_ex"]()
            windows()
            assert torch.equal(dst[:cbytes], dst2[:cbytes]), "the windows do not concatenate to the whole-text output"
            calls[f"krep_gpu_format_lines_window x{K}"] = windows
            # the -o form the same way: window k holds the records that start in [lo, hi) in the buffer [lo, hi + 4 KiB), count_to is
            # the next window's base, the newline count and the stale line number are chained from call to call, live in every repetition
            last1, at = 0, n
            while at > 0 and not last1:
                lo = max(at - (1 << 24), 0)
                hit = (buf[lo:at] == 10).nonzero()
                last1 = lo + int(hit[-1]) + 1 if hit.numel() else 0
                at = lo
            edges = [n * k // K for k in range(K + 1)]
            idx = [int(x) for x in torch.searchsorted(starts, torch.tensor(edges, dtype=torch.int64, device="cuda"))]
            dst3 = torch.empty(obytes + 64, dtype=torch.uint8, device="cuda")

            def matches_windows():
                nl = stale = at = 0
                for k in range(K):
                    lo, hi = edges[k], edges[k + 1]
                    win = abi.MatchesWindow(lo, n, hi, nl, last1, stale, int(m > 10))
                    r = eng.format_matches_window(buf.data_ptr() + lo, min(hi + 4096, n) - lo, win, pos.data_ptr() + 16 * idx[k],
                                                  idx[k + 1] - idx[k], abi.SIZE_MAX, fmt, dst3.data_ptr() + at, obytes - at)
                    assert not r.matches.overflow
                    nl, stale, at = int(r.newlines_before_count_to), int(r.stale_line), at + int(r.matches.out_bytes)
                return at
            calls["krep_gpu_format_matches"]()
            assert matches_windows() == obytes
            assert torch.equal(dst[:obytes], dst3[:obytes]), "the -o windows do not concatenate to the whole-text output"
            calls[f"krep_gpu_format_matches_window x{K}"] = matches_windows
        ms = {k: [] for k in calls}
        for rep in range(args.warmup + args.reps):
            for k, f in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                f()
                e1.record()
                e1.synchronize()
                if rep >= args.warmup:
                    ms[k].append(e0.elapsed_time(e1))
        lines.append(f"{name}: text {n} B, {m} records, {L} lines ({int(q.capped_lines)} capped), out_bytes {nbytes}, "
                     f"coloured out_bytes {cbytes}, -o out_bytes {obytes}")
        for k, v in ms.items():
            moved = n + 16 * m + 2 * {"krep_gpu_format_lines": nbytes, "krep_gpu_format_lines_ex": cbytes, "krep_gpu_format_matches": obytes}.get(k, obytes if "matches_window" in k else cbytes if "window" in k else 0)
            lines.append(f"  {k:26s} {statistics.median(v):9.3f} ms [{min(v):.3f} .. {max(v):.3f}]   floor {moved / bench.HBM_MEASURED_GBS / 1e6:7.3f} ms")
        plan.close()
        del pos, lineno, spans, first, dst
        if args.windows:
            del dst2, dst3, starts
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
