"""krep -E with *, + and {n,} on the device (kg_regex_loops.hip: the filter scan that names the candidate lines, the line walk) beside the
literal scan and beside the reference's regex_search on the CPU.  Two texts resident in HBM, one after the other: a kind-2 haystack with
`Sherlock` planted every 10 000 bytes and a kind-5 word text.  hipEvent times of whole scans, the median of 10 steady scans after 2
warm-ups (3 after 1 when a scan takes more than half a second).  The yardstick comes first: the literal plan for `Sherlock` on the same
buffer.  Then every pattern with -c and with records, each road forced in turn (krep_gpu_debug_force_regex_loops_road) and the scan's
own choice; and regex_search itself (oracle/_ref, one thread) on the first 256 MiB of the host twin.  There is no pass bar on these
numbers: the switch krep_gpu_set_regex_loops stays off whatever they say.
--windows N (with krep_gpu_set_regex_loops_windows on): every regex scan is N scans of the same resident text, window k owning the
k-th share of it in a buffer that holds 4096 bytes more on each side, as the host executor stages its pieces; the time of a scan is the
sum of the N hipEvent times, the count the sum of the windows' counts (under -c the lines that hold an owned start, not folded).
--haystack: the first text only.
--groups (with krep_gpu_set_regex_groups on): the rows of the groups compiler instead.  On the haystack `Sherlo+ck` and
`[a-z]+ck` by the old step and, tagged "general", by the general step (krep_gpu_debug_force_regex_general), and `(Sherlock|Watson)+`; on
the word text `([a-z]+ )+ck`; on a third text, the same haystack generator with `192.168.10.254` planted every 10 000 bytes instead of
`Sherlock`, the IP expression.  The output goes to profiles/regex_groups_scan.txt unless one is named.
--long-lines (with krep_gpu_set_regex_groups and krep_gpu_set_regex_long_lines on): the rows of the long-line walk instead (DESIGN
§4.9, "Long lines").  (a) a JSONL-like text, every line 6 - 10 KiB of lower-case words, numbers and JSON punctuation with `ERROR`,
`timeout` and `www.example.com` planted: `ERROR.*timeout` (the loops compiler's) and `([a-z]+\.)+com` (the groups compiler's), -c and
records, both roads, and regex_search on the first CPU MiB of the same text — what such a text gets with the switch off.  (b) the
kind-2 haystack as it is and with the newlines of 1 MiB - 8 KiB in its middle blanked, one line close to the longest admitted: `Sherlo+ck`,
-c and records, both roads.  The output goes to profiles/regex_long_lines.txt unless one is named.
  usage: python tools/regex_loops_bench.py [--windows N] [--haystack] [--groups] [--long-lines] [GiB = 8] [CPU MiB = 256] [output = profiles/regex_loops_scan.txt]"""
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
from krep_amd.engine import KrepGpuError  # noqa: E402
import regex_ref  # noqa: E402
import wordlist  # noqa: E402

locale.setlocale(locale.LC_CTYPE, "C")  # the locale krep runs in; the -E compilers take no pattern in a multibyte one
windows = 1
if "--windows" in sys.argv:
    i = sys.argv.index("--windows")
    windows = max(1, int(sys.argv[i + 1]))
    del sys.argv[i:i + 2]
haystack_only = "--haystack" in sys.argv
if haystack_only:
    sys.argv.remove("--haystack")
groups = "--groups" in sys.argv
if groups:
    sys.argv.remove("--groups")
long_lines = "--long-lines" in sys.argv
if long_lines:
    sys.argv.remove("--long-lines")
gib = float(sys.argv[1]) if len(sys.argv) > 1 else 8.0
cpu_mib = int(sys.argv[2]) if len(sys.argv) > 2 else 256
default_out = "regex_long_lines.txt" if long_lines else "regex_groups_scan.txt" if groups else "regex_loops_scan.txt"
out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", default_out)
n = int(gib * (1 << 30))
SEED, PERIOD = 42, 10000
WORDS = wordlist.pack(wordlist.word_list())
TEXTS = [("kind-2 haystack, `Sherlock` every 10 000 bytes", 2, SEED, b"Sherlock", PERIOD), ("kind-5 word text", 5, 20260930, WORDS, 80)]
PATTERNS = [(b"Sherlo+ck", "filter Sherlo: rare"), (b"Sherlock.*[a-z]", "filter Sherlock.: rare, the match runs to the line's end"),
            (b"[a-z]+ck", "filter [a-z]ck")]
ROADS = [(0, "auto"), (1, "sparse"), (2, "dense")]
BY_TEXT = [PATTERNS] * len(TEXTS)  # (pattern, what it shows[, True: through the general step]) per text
if groups:
    IP = rb"[0-9]{1,3}\.[0-9]{1,3}\.[0-9]{1,3}\.[0-9]{1,3}"
    TEXTS.append(("kind-2 haystack, `192.168.10.254` every 10 000 bytes", 2, SEED, b"192.168.10.254", PERIOD))
    BY_TEXT = [[(b"Sherlo+ck", "old step"), (b"Sherlo+ck", "general step", True), (b"[a-z]+ck", "old step"), (b"[a-z]+ck", "general step", True),
                (b"(Sherlock|Watson)+", "filter Sherlock, Watson: 14 positions")],
               [(b"([a-z]+ )+ck", "filter [a-z] ck: 4 positions")],
               [(IP, "filter [0-9]\\.[0-9]: 15 positions")]]
e = krep_amd.load()
e.set_regex_loops(True)
if groups:
    e.set_regex_groups(True)
if windows > 1:
    e.set_regex_loops_windows(True)
CONTEXT = 4096  # bytes of the text a window's buffer holds on each side of what it owns (include/krep_gpu.h)
buf = torch.empty(n + 64, dtype=torch.uint8, device="cuda")
cap = n // 64
pos = torch.empty(2 * cap, dtype=torch.int64, device="cuda")
rows = []


def say(line):
    print(line, flush=True)
    rows.append(line)


def median_ms(plan, want_pos, parts=1):
    def scan():
        if parts == 1:
            return plan.scan(buf.data_ptr(), n, 0, n, 0, pos.data_ptr() if want_pos else 0, cap if want_pos else 0, time_it=True)
        total = abi.ScanOut()
        for k in range(parts):
            lo, hi = n * k // parts, n * (k + 1) // parts
            b0, b1 = max(lo - CONTEXT, 0), min(hi + CONTEXT, n)
            out = plan.scan(buf.data_ptr() + b0, b1 - b0, lo - b0, hi - b0, b0, pos.data_ptr() if want_pos else 0, cap if want_pos else 0,
                            time_it=True, global_len=n)
            total.kernel_ms += out.kernel_ms
            total.count += out.count
            total.total_matches += out.total_matches
        return total
    out = scan()  # (builds the inner plans and sizes the scratch)
    warm, steady = (1, 3) if out.kernel_ms > 500 else (2, 10)
    ms = []
    for i in range(warm + steady):
        out = scan()
        if i >= warm:
            ms.append(out.kernel_ms)
    median_ms.scans = 1 + warm + steady
    return statistics.median(ms), out


def jsonl_text():
    """the text of row (a) into buf, made on the device: lines of 6 - 10 KiB over lower-case letters, digits, blanks and JSON
    punctuation, the three plants every 20 011 / 30 011 / 50 021 bytes (over whatever stands there, a newline included)"""
    g = torch.Generator(device="cuda").manual_seed(20261021)
    alphabet = torch.tensor(list(b'abcdefghijklmnopqrstuvwxyz0123456789    "":,.{}'), dtype=torch.uint8, device="cuda")
    step = 1 << 28
    for lo in range(0, n, step):
        m = min(step, n - lo)
        buf[lo:lo + m] = alphabet[torch.randint(0, alphabet.numel(), (m,), generator=g, device="cuda")]
    ends = torch.cumsum(torch.randint(6144, 10241, (n // 6144 + 2,), generator=g, device="cuda"), 0)
    buf[ends[ends < n]] = 10
    for plant, period in ((b"ERROR", 20011), (b"timeout", 30011), (b"www.example.com", 50021)):
        at = torch.arange(period, n - len(plant), period, device="cuda")
        for k, c in enumerate(plant):
            buf[at + k] = c
    torch.cuda.synchronize()
    return int((ends < n).sum().item())


def long_rows(patterns, cpu_rows):
    for pat, what in patterns:
        for mode in ("-c", "records"):
            kw = dict(count_lines=True) if mode == "-c" else dict()
            for road, road_name in ROADS[1:]:
                e.force_regex_loops_road(road)
                plan = e.plan(abi.Params([pat], regex=True, **kw))
                try:
                    before = e.regex_long_walks()
                    ms, out = median_ms(plan, mode == "records")
                    say(f"regex    {pat.decode():<18} {mode:<8} {road_name:<8} {ms:10.3f} ms {n / ms / 1e6:8.2f} GB/s  "
                        f"{'lines' if mode == '-c' else 'matches'} {out.count}  long-walk launches a scan {(e.regex_long_walks() - before) // median_ms.scans}  ({what})")
                except KrepGpuError as err:
                    say(f"regex    {pat.decode():<18} {mode:<8} {road_name:<8} refused: {err}")
                finally:
                    plan.close()
                    e.force_regex_loops_road(0)
    if cpu_rows and regex_ref.available():
        m = min(n, cpu_mib << 20)
        host = buf[:m].cpu().numpy()
        say(f"# the reference's regex_search (compiled reference, glibc regexec, ONE thread) on the first {m >> 20} MiB of the same text")
        for pat, _ in patterns:
            for mode in ("count", "-c"):
                kw = dict(count_lines=True) if mode == "-c" else dict(track_positions=False)
                t0 = time.perf_counter()
                ret, _ = regex_ref.call(pat, host, want_result=False, **kw)
                dt = time.perf_counter() - t0
                plan = e.plan(abi.Params([pat], regex=True, **kw))
                got = plan.scan(buf.data_ptr(), m).count  # (the same slice as a text of its own on the device)
                plan.close()
                say(f"cpu      {pat.decode():<18} {mode:<8} {dt * 1e3:10.0f} ms {m / dt / 1e9:8.3f} GB/s  returned {ret}  "
                    f"(the device on the same slice: {got}{'' if got == ret else ' DIFFERS'})")


if long_lines:
    e.set_regex_groups(True)
    e.set_regex_long_lines(True)
    say(f"# tools/regex_loops_bench.py --long-lines: {gib:g} GiB texts, hipEvent time of a whole scan, median of 10 steady scans after 2")
    say("# warm-ups (3 after 1 beyond 0.5 s); GB/s = text bytes / time; krep_gpu_set_regex_long_lines on")
    say(f"## (a) JSONL-like text, {jsonl_text()} lines of 6 - 10 KiB")
    long_rows([(b"ERROR.*timeout", "loops"), (b"([a-z]+\\.)+com", "groups")], True)
    for blank in (False, True):
        e.generate(buf.data_ptr(), n, 0, 2, SEED, b"Sherlock", PERIOD)
        if blank:
            seg = buf[n // 2:n // 2 + (1 << 20) - 8192]
            seg[seg == 10] = 32
        torch.cuda.synchronize()
        say(f"## (b) kind-2 haystack, `Sherlock` every 10 000 bytes" + (", the newlines of 1 MiB - 8 KiB in its middle blanked" if blank else ", as it is"))
        long_rows([(b"Sherlo+ck", "loops")], False)
    e.set_regex_long_lines(False)
    e.set_regex_groups(False)
    e.set_regex_loops(False)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(rows) + "\n")
    sys.exit(0)
say(f"# tools/regex_loops_bench.py: {gib:g} GiB texts, hipEvent time of a whole scan (filter scan, line analysis, line walk), median of 10")
say("# steady scans after 2 warm-ups (3 after 1 beyond 0.5 s); GB/s = text bytes / time; ratio = to the literal plan for `Sherlock` in the")
say("# same mode on the same buffer; road: forced, or auto with the road it took")
if windows > 1:
    say(f"# --windows {windows}: every regex scan is {windows} scans, window k owning the k-th share of the text with {CONTEXT} bytes of context on each")
    say("# side; the time is the sum of their hipEvent times, the count the sum of their counts (-c: not folded across the cuts)")
for (name, kind, seed, needle, period), patterns in list(zip(TEXTS, BY_TEXT))[:1 if haystack_only else None]:
    e.generate(buf.data_ptr(), n, 0, kind, seed, needle, period)
    torch.cuda.synchronize()
    say(f"## {name} (seed {seed})")
    yard = {}
    plan = e.plan(abi.Params([b"Sherlock"]))
    for mode, want_pos in (("count", False), ("records", True)):
        ms, out = median_ms(plan, want_pos)
        yard[mode] = ms
        say(f"literal  {'Sherlock':<18} {mode:<8} {'-':<7} {ms:9.3f} ms {n / ms / 1e6:7.0f} GB/s  ratio 1.00  matches {out.total_matches}")
    plan.close()
    for pat, what, *general in patterns:
        for mode in ("-c", "records"):
            kw = dict(count_lines=True) if mode == "-c" else dict()
            for road, road_name in ROADS:
                e.force_regex_loops_road(road)
                if general:
                    e.force_regex_general(True)  # (read when the plan is made)
                try:
                    plan = e.plan(abi.Params([pat], regex=True, **kw))
                finally:
                    if general:
                        e.force_regex_general(False)
                try:
                    before = e.regex_loops_roads()
                    ms, out = median_ms(plan, mode == "records", windows)
                    after = e.regex_loops_roads()
                    took = "sparse" if after[0] > before[0] else "dense"
                    ref_ms = yard["records" if mode == "records" else "count"]
                    say(f"regex    {pat.decode():<18} {mode:<8} {road_name + ('>' + took if road == 0 else ''):<12} {ms:9.3f} ms {n / ms / 1e6:7.1f} GB/s  "
                        f"ratio {ref_ms / ms:5.3f}  {'lines' if mode == '-c' else 'matches'} {out.count}  ({what})")
                except KrepGpuError as err:
                    say(f"regex    {pat.decode():<18} {mode:<8} {road_name:<12} refused: {err}")
                finally:
                    plan.close()
                    e.force_regex_loops_road(0)
    if regex_ref.available():
        m = min(n, cpu_mib << 20)
        host = e.generate_host(m, 0, kind, seed, needle, period)
        say(f"# the reference's regex_search (compiled reference, glibc regexec, ONE thread) on the first {m >> 20} MiB of the same text")
        for pat in dict.fromkeys(p[0] for p in patterns):
            for mode in ("count", "-c"):
                kw = dict(count_lines=True) if mode == "-c" else dict(track_positions=False)
                t0 = time.perf_counter()
                ret, _ = regex_ref.call(pat, host, want_result=False, **kw)
                dt = time.perf_counter() - t0
                say(f"cpu      {pat.decode():<18} {mode:<8} {dt * 1e3:9.0f} ms {m / dt / 1e9:7.3f} GB/s  returned {ret}")
    else:
        say("# no compiled reference (oracle/_ref) on this host: the CPU rows are missing")
e.set_regex_loops(False)
if groups:
    e.set_regex_groups(False)
if windows > 1:
    e.set_regex_loops_windows(False)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(rows) + "\n")
