#!/usr/bin/env python3
"""Registers, scratch, LDS and occupancy of every kernel of one HIP source, as the compiler reports
them (-Rpass-analysis=kernel-resource-usage; no GPU needed).  DESIGN.md quotes its output.

    python tools/kernel_resources.py sketchml_amd/csrc/skml_optim.hip [--fail-on-scratch]
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "--cuda-device-only",
         "-Rpass-analysis=kernel-resource-usage"]


def resources(src: str, hipcc: str = "/opt/rocm/bin/hipcc"):
    src = os.path.abspath(src)
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([hipcc, *FLAGS, "-c", src, "-o", os.path.join(tmp, "k.o")], capture_output=True, text=True,
                           cwd=os.path.dirname(os.path.abspath(src)))
    if r.returncode:
        sys.exit(r.stderr)
    rows = []
    for b in re.split(r"remark: [^\n]*Function Name: ", r.stderr)[1:]:
        name = b.split("\n")[0].split()[0]
        name = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip() or name
        name = re.sub(r"\(.*", "", name).replace("skml::", "").replace("void ", "")

        def g(key):
            return int(re.search(re.escape(key) + r": (\d+)", b).group(1))
        rows.append((name, g("VGPRs"), g("AGPRs"), g("ScratchSize [bytes/lane]"), g("LDS Size [bytes/block]"),
                     g("Occupancy [waves/SIMD]")))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("source")
    ap.add_argument("--fail-on-scratch", action="store_true")
    a = ap.parse_args()
    rows = resources(a.source)
    print(f"{'kernel':<48} {'VGPR':>5} {'AGPR':>5} {'scratch':>8} {'LDS':>7} {'waves/SIMD':>11}")
    for name, vg, ag, sc, lds, occ in rows:
        print(f"{name:<48} {vg:>5} {ag:>5} {sc:>8} {lds:>7} {occ:>11}")
    if a.fail_on_scratch and any(r[3] for r in rows):
        sys.exit("a kernel uses scratch")


if __name__ == "__main__":
    main()
