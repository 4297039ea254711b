#!/usr/bin/env python3
"""Builds another revision's libskml.so so that this tree's Python can load it through SKML_LIB,
for A/B timing against that revision (tools/bench_sparse_lowp.py --other-lib, leg (c)).

The revision's tree is exported with `git archive` into OUT/src and built with its own Makefile.
sketchml_amd/_lib.py binds every entry of its table when it loads a library, so a revision that
lacks entries this tree has is linked with stubs of those names that return SKML_E_ARG.

    python tools/build_other_lib.py HEAD~1 gpu_jobs/parent_lib
    python tools/bench_sparse_lowp.py --other-lib gpu_jobs/parent_lib/libskml.so
"""
import glob
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    rev, out = sys.argv[1], os.path.abspath(sys.argv[2])
    src = os.path.join(out, "src")
    os.makedirs(src, exist_ok=True)
    tar = subprocess.run(["git", "-C", ROOT, "archive", rev, "sketchml_amd/csrc", "include"], check=True,
                         stdout=subprocess.PIPE).stdout
    subprocess.run(["tar", "-x", "-C", src], input=tar, check=True)
    subprocess.run(["make", "-s", "-j", str(min(16, os.cpu_count() or 4)), "-C", os.path.join(src, "sketchml_amd", "csrc")],
                   check=True)
    # the names this tree binds (the keys of _lib._SIGS) that the revision's header does not declare
    table = open(os.path.join(ROOT, "sketchml_amd", "_lib.py")).read()
    names = re.findall(r'^\s+"(skml_\w+)": \(', table, re.M)
    header = open(os.path.join(src, "include", "skml.h")).read()
    missing = [n for n in names if not re.search(r"\b" + n + r"\(", header)]
    stubs = os.path.join(out, "stubs.c")
    with open(stubs, "w") as f:
        f.write("/* entries the revision lacks: refused (SKML_E_ARG) */\n")
        f.writelines(f"int {n}(void) {{ return 1; }}\n" for n in missing)
    objs = sorted(glob.glob(os.path.join(src, "sketchml_amd", "lib", "obj", "*.o")))
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", os.path.join(out, "libskml.so"), *objs, "-x", "c",
                    stubs, "-L/opt/rocm/lib", "-lrccl", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    print(f"{os.path.join(out, 'libskml.so')}: {rev}, {len(missing)} stubbed entries: {' '.join(missing)}")


if __name__ == "__main__":
    main()
