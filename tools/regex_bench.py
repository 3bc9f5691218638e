"""krep -E on the device (kg_regex.hip, kg_regex_alt.hip; the last rows: what krep_gpu_regex_compile_ext expands) beside the literal scan and beside the reference's regex_search on the CPU.
One kind-2 haystack with `Sherlock` planted every 10 000 bytes, resident in HBM; hipEvent times, the median of 10 steady scans
after 2 warm-up scans.  The yardstick comes first: the literal plan for `Sherlock` on the same buffer.  Then the regex patterns,
each with its ratio to the yardstick; and regex_search itself (oracle/_ref, one thread) on the first 256 MiB of the host twin.
  usage: python tools/regex_bench.py [GiB = 8] [CPU MiB = 256] [output = profiles/regex_scan.txt]"""
import locale
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
import krep_amd  # noqa: E402
from krep_amd import abi  # noqa: E402
import regex_ref  # noqa: E402

locale.setlocale(locale.LC_CTYPE, "C")  # the locale krep runs in; krep_gpu_regex_compile() takes no pattern in a multibyte one
gib = float(sys.argv[1]) if len(sys.argv) > 1 else 8.0
cpu_mib = int(sys.argv[2]) if len(sys.argv) > 2 else 256
out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "regex_scan.txt")
n = int(gib * (1 << 30))
SEED, PERIOD = 42, 10000
e = krep_amd.load()
buf = torch.empty(n + 64, dtype=torch.uint8, device="cuda")
cap = n // 64
pos = torch.empty(2 * cap, dtype=torch.int64, device="cuda")
e.generate(buf.data_ptr(), n, 0, 2, SEED, b"Sherlock", PERIOD)
torch.cuda.synchronize()
rows = []


def say(line):
    print(line, flush=True)
    rows.append(line)


def median_ms(plan, want_pos):
    ms, out = [], None
    for i in range(12):
        out = plan.scan(buf.data_ptr(), n, 0, n, 0, pos.data_ptr() if want_pos else 0, cap if want_pos else 0, time_it=True)
        if i >= 2:
            ms.append(out.kernel_ms)
    return statistics.median(ms), out


say(f"# tools/regex_bench.py: {gib:g} GiB kind-2 haystack (seed {SEED}, `Sherlock` every {PERIOD} bytes), hipEvent time of a whole scan,")
say("# median of 10 steady scans after 2 warm-ups; GB/s = text bytes / time; ratio = to the literal plan for `Sherlock` in the same mode")
yard = {}
plan = e.plan(abi.Params([b"Sherlock"]))
for mode, want_pos in (("count", False), ("records", True)):
    ms, out = median_ms(plan, want_pos)
    yard[mode] = ms
    say(f"literal  {'Sherlock':<22} {mode:<8} {ms:8.3f} ms {n / ms / 1e6:7.0f} GB/s  ratio 1.00  matches {out.total_matches}")
plan.close()
literal_matches = out.total_matches

JOBS = [(b"Sherl[oO]ck", "anchor path", ("count", "records")), (b"[A-Z][a-z]{7}", "table path", ("count", "records")),
        (b"[a-z]{4}", "dense", ("count", "-c")), (b"Sherlock", "a literal as a regex", ("count", "records")),
        # line anchors: each row beside its unanchored twin above (few lines of the haystack start with the planted word, most end
        # behind a run of lower-case letters)
        (b"^Sherlock", "anchor path, ^", ("count", "records")), (b"[a-z]{4}$", "dense, $", ("count", "-c")),
        (b"^[A-Z][a-z]{7}$", "table path, ^ and $", ("count", "records")),
        # alternations (kg_regex_alt.hip): each row beside the table-path row of [A-Z][a-z]{7} on the same buffer (-c beside its count row)
        (b"Sherlock|Watson|Holmes", "alternation, 3 branches", ("count", "records", "-c")),
        (b"[A-Z][a-z]{7}|[0-9]{4}", "alternation, [0-9]{4} overlaps itself: greedy pass", ("count", "records", "-c")),
        # what krep_gpu_regex_compile_ext expands: each row beside Sherlock|Watson|Holmes above, the unanchored kernel with the same
        # number of branches (the first row runs that kernel, the other two its anchored instantiations)
        (b"Sherlo?ck|Watson", "expanded: Sherlck, Sherlock, Watson", ("count", "records", "-c")),
        (b"^(Sherlock|Watson|Holmes)", "alternation between anchors, ^", ("count", "records", "-c")),
        (b"(Sherlock|Watson|Holmes)$", "alternation between anchors, $", ("count", "records", "-c"))]
TWIN = {b"^Sherlock": b"Sherlock", b"[a-z]{4}$": b"[a-z]{4}", b"^[A-Z][a-z]{7}$": b"[A-Z][a-z]{7}",
        b"Sherlock|Watson|Holmes": b"[A-Z][a-z]{7}", b"[A-Z][a-z]{7}|[0-9]{4}": b"[A-Z][a-z]{7}",
        b"Sherlo?ck|Watson": b"Sherlock|Watson|Holmes", b"^(Sherlock|Watson|Holmes)": b"Sherlock|Watson|Holmes",
        b"(Sherlock|Watson|Holmes)$": b"Sherlock|Watson|Holmes"}
took = {}
for pat, what, modes in JOBS:
    for mode in modes:
        kw = dict(count_lines=True) if mode == "-c" else dict(track_positions=(mode == "records"))
        plan = e.plan(abi.Params([pat], regex=True, **kw))
        ms, out = median_ms(plan, mode == "records")
        plan.close()
        ref_ms = yard["records" if mode == "records" else "count"]
        took[pat, mode] = ms
        twin_mode = mode if pat not in TWIN or (TWIN[pat], mode) in took else "count"
        twin = f"; {ms / took[TWIN[pat], twin_mode]:4.2f} x the time of {TWIN[pat].decode()}" if pat in TWIN else ""
        say(f"regex    {pat.decode():<22} {mode:<8} {ms:8.3f} ms {n / ms / 1e6:7.0f} GB/s  ratio {ref_ms / ms:4.2f}  "
            f"{'lines' if mode == '-c' else 'matches'} {out.count}  ({what}{twin})")
        if pat in (b"Sherl[oO]ck", b"Sherlock") and mode != "-c":
            assert out.total_matches == literal_matches, (pat, out.total_matches, literal_matches)

if regex_ref.available():
    m = min(n, cpu_mib << 20)
    host = e.generate_host(m, 0, 2, SEED, b"Sherlock", PERIOD)
    say(f"# the reference's regex_search (compiled reference, glibc regexec, ONE thread) on the first {m >> 20} MiB of the same text")
    for pat, _, modes in JOBS:
        for mode in modes:
            if mode == "records":
                continue
            kw = dict(count_lines=True) if mode == "-c" else dict(track_positions=False)
            t0 = time.perf_counter()
            ret, _ = regex_ref.call(pat, host, want_result=False, **kw)
            dt = time.perf_counter() - t0
            say(f"cpu      {pat.decode():<22} {mode:<8} {dt * 1e3:8.0f} ms {m / dt / 1e9:7.3f} GB/s  returned {ret}")
else:
    say("# no compiled reference (oracle/_ref) on this host: the CPU rows are missing")
with open(out_path, "w") as f:
    f.write("\n".join(rows) + "\n")
