#!/usr/bin/env python3
"""Per kernel of one translation unit, from `hipcc -S` with the project's flags: how many v_readlane_b32 / v_writelane_b32 the
device code holds (scalars the compiler keeps in vector lanes), scratch bytes, vector registers, waves per SIMD, static LDS.
usage: tools/asm_lane_counts.py pba_drivers.hip [filter] [-DFOO=0 ...]      (PBA_VARIANT_CSRC=<dir>: another copy of csrc/)"""
import os, re, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pacbioassembly_amd import build as b
csrc = os.environ.get("PBA_VARIANT_CSRC", b.CSRC)
args = sys.argv[1:]
extra = [a for a in args if a.startswith("-")]
args = [a for a in args if not a.startswith("-")]
src, flt = os.path.join(csrc, args[0]), args[1] if len(args) > 1 else ""
keep = next((a.split("=", 1)[1] for a in extra if a.startswith("--keep=")), None)
extra = [a for a in extra if not a.startswith("--keep=")]
with tempfile.TemporaryDirectory() as tmp:
    out = keep or os.path.join(tmp, "tu.s")
    subprocess.run([b._hipcc()] + [csrc if f == b.CSRC else f for f in b._flags()] + extra +
                   ["-S", "--cuda-device-only", src, "-o", out], check=True, cwd=csrc)
    text = open(out).read()
names = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M)
dem = dict(zip(names, subprocess.run(["c++filt"] + names, capture_output=True, text=True).stdout.splitlines()))
print(f"{'kernel':40s} {'readlane':>8s} {'writelane':>9s} {'scratch':>7s} {'VGPR':>5s} {'waves':>5s} {'LDS':>6s}")
for k in names:
    short = dem[k].split("(")[0].replace("void ", "")
    if flt not in short:
        continue
    body = text[text.index("\n" + k + ":"):]
    body = body[:body.index("; Occupancy:", body.index(".end_amdhsa_kernel")) + 20]   # (the resource comments follow the descriptor)
    def field(pat):
        m = re.search(pat, body)
        return m.group(1) if m else "?"
    cols = [field(p) for p in (r"; ScratchSize: (\d+)", r"; NumVgprs: (\d+)", r"; Occupancy: (\d+)",
                               r"\.amdhsa_group_segment_fixed_size (\d+)")]
    print(f"{short[:40]:40s} {body.count('v_readlane_b32'):8d} {body.count('v_writelane_b32'):9d} "
          f"{cols[0]:>7s} {cols[1]:>5s} {cols[2]:>5s} {cols[3]:>6s}")
