"""Two builds of one csrc/*.hip side by side, kernel by kernel (development aid for refactors of device code; needs no GPU).
usage: python tools/kernel_build_compare.py <parent csrc dir> <branch csrc dir> [file.hip, default kg_ac.hip] > profiles/<name>.txt
Per kernel: VGPRs, scratch bytes per lane, waves/SIMD and LDS from the compiler's remarks (as tools/resource_usage.sh), the SGPR and
VGPR spill counts from the assembly's metadata, and whether the instruction stream (comments dropped) is the same text.  Conditions
checked per kernel: no scratch, no VGPR spill, VGPRs not above the parent's, the same LDS."""
import os, re, subprocess, sys, tempfile
from concurrent.futures import ThreadPoolExecutor

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-cuda-compat", "--cuda-device-only", "-S",
         "-Rpass-analysis=kernel-resource-usage"]


def compile_side(csrc, name, out):
    p = subprocess.run([HIPCC] + FLAGS + [name, "-o", out], cwd=csrc, stderr=subprocess.PIPE, text=True, check=True)
    return open(out).read(), p.stderr


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), stdout=subprocess.PIPE, text=True, check=True).stdout.split("\n")
    return {n: re.sub(r"\(.*", "", d).replace("void ", "").replace("kg::", "") for n, d in zip(names, out)}


def parse(asm, remarks):
    k = {}
    for blk in re.split(r"\n  - (?=\.agpr_count)", asm.split("amdhsa.kernels:")[1]):
        f = dict(re.findall(r"^\s+\.(\w+):\s+(\S+)$", "    " + blk, re.M))
        if "name" in f:
            k[f["name"]] = {"sspill": int(f["sgpr_spill_count"]), "vspill": int(f["vgpr_spill_count"])}
    for m in re.finditer(r"Function Name: (\S+).*?VGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?Occupancy \[waves/SIMD\]: (\d+).*?"
                         r"LDS Size \[bytes/block\]: (\d+)", remarks, re.S):
        if m.group(1) in k:
            k[m.group(1)].update(vgpr=int(m.group(2)), scratch=int(m.group(3)), occ=int(m.group(4)), lds=int(m.group(5)))
    for name in k:
        body = re.search(r"^%s:[^\n]*\n(.*?)^\.Lfunc_end" % re.escape(name), asm, re.M | re.S).group(1)
        k[name]["text"] = [s for s in (re.sub(r"\s*;.*", "", l).strip() for l in body.split("\n")) if s]
    return k


def main():
    parent, branch = sys.argv[1], sys.argv[2]
    name = sys.argv[3] if len(sys.argv) > 3 else "kg_ac.hip"
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(2) as ex:
        jobs = [ex.submit(compile_side, d, name, os.path.join(tmp, s + ".s")) for s, d in (("parent", parent), ("branch", branch))]
        P, B = (parse(*j.result()) for j in jobs)
    names = demangle(sorted(P))
    print(f"# {name}: hipcc {' '.join(FLAGS)}; per kernel parent -> branch")
    print("# kernel | VGPRs | scratch B/lane | waves/SIMD | LDS B (static) | sgpr_spill_count | vgpr_spill_count | instruction stream | verdict")
    bad = same = 0
    for n in sorted(P, key=lambda n: names[n]):
        p, b = P[n], B.get(n)
        if b is None:
            print(f"{names[n]} | MISSING in the branch")
            bad += 1
            continue
        ok = b["scratch"] == 0 and b["vspill"] == 0 and b["vgpr"] <= p["vgpr"] and b["lds"] == p["lds"] and b["occ"] >= p["occ"]
        ident = p["text"] == b["text"]
        same += ident
        bad += not ok
        cols = [f"{p[c]} -> {b[c]}" for c in ("vgpr", "scratch", "occ", "lds", "sspill", "vspill")]
        stream = "identical" if ident else f"differs ({len(p['text'])} -> {len(b['text'])} lines)"
        print(" | ".join([names[n]] + cols + [stream, "ok" if ok else "FAIL"]))
    extra = sorted(set(B) - set(P))
    print(f"# {len(P)} kernels, {same} with an identical instruction stream, {bad} failing a condition"
          + (f", {len(extra)} only in the branch" if extra else ""))
    return 1 if bad or extra else 0


if __name__ == "__main__":
    sys.exit(main())
