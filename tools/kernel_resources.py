"""Register / scratch / LDS footprint of every device kernel, from the compiler's own metadata (the assembly `make asm` writes to
build/asm/, one file per device unit, with the Makefile's flags): VGPRs, AGPRs, SGPRs, spilled VGPRs, scratch bytes per lane, LDS
bytes, occupancy (waves per SIMD).  `make asm` runs first, so a missing or stale file is rebuilt.  --all: the sort library's kernels too.
    python tools/kernel_resources.py > profiles/r03_kernel_resources.txt"""
import glob
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names) + "\n", capture_output=True, text=True).stdout.split("\n")
    return [re.sub(r"\((?:[^()]|\([^()]*\))*\)\s*$", "", o).replace("void ", "").replace("nxd::", "").replace("(anonymous namespace)::", "") for o in out]


# The instances of the kernel families carry a set of features as an unsigned template argument (nexus_amd/csrc/device/nx_variants.h:
# kTf* for trace_kernel, kMf* for the rest): printed by name, from the header's own constants, e.g. trace_kernel<anyhit+transmit>.
BITS = {"Tf": [], "Mf": []}
for kind, name, bit in re.findall(r"constexpr unsigned k(Tf|Mf)(\w+) = (\d+)u;", open(os.path.join(ROOT, "nexus_amd/csrc/device/nx_variants.h")).read()):
    if name != "All":
        BITS[kind].append((int(bit), name.lower()))


def named(n):
    m = re.match(r"(\w+)<(.*?)(\d+)u>$", n)
    if not m:
        return n
    bits = BITS["Tf" if m.group(1) == "trace_kernel" else "Mf"]
    return "%s<%s%s>" % (m.group(1), m.group(2), "+".join(name for bit, name in bits if int(m.group(3)) & bit) or "none")


print("%-58s %5s %5s %5s %7s %8s %6s %5s" % ("kernel", "VGPR", "AGPR", "SGPR", "spilled", "scratch", "LDS", "occ"))
made = subprocess.run(["make", "-j16", "asm"], cwd=ROOT, capture_output=True, text=True)
if made.returncode != 0:
    sys.exit("make asm failed:\n" + made.stderr[-2000:])
for src in sorted(glob.glob(os.path.join(ROOT, "nexus_amd/csrc/device/*.hip"))):
    text = open(os.path.join(ROOT, "build/asm", os.path.basename(src)[:-4] + ".s")).read()
    rows = []
    for m in re.finditer(r"- \.agpr_count:\s+(\d+)(.*?)\.wavefront_size", text, re.S):
        blk = m.group(0)
        g = lambda k: (re.search(r"\.%s:\s+(\S+)" % k, blk) or [None, "0"])[1]
        rows.append((g("name"), g("vgpr_count"), g("agpr_count"), g("sgpr_count"), g("vgpr_spill_count"), g("private_segment_fixed_size"), g("group_segment_fixed_size")))
    occ = dict(re.findall(r"; Occupancy: (\d+)\n(?:.*\n){0,12}?\s*\.section\s+\.AMDGPU\.csdata.*\n(?:.*\n){0,3}?\s*\.text\n\s*\.protected\s+(\S+)", text))
    occ_by_kernel = {}
    for m in re.finditer(r"^(\S+):\s+; @\1\n(?:.*\n)*?; Occupancy: (\d+)", text, re.M):
        occ_by_kernel[m.group(1)] = m.group(2)
    names = demangle([r[0] for r in rows])
    for (raw, v, a, s, sp, scr, lds), n in zip(rows, names):
        if "rocprim" in n and "--all" not in sys.argv:
            continue  # the sort library's kernels (device LBVH build)
        print("%-58s %5s %5s %5s %7s %8s %6s %5s" % (named(n)[:58], v, a, s, sp, scr, lds, occ_by_kernel.get(raw, "?")))
