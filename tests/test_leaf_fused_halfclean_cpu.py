"""The paired 3-input form of the in-register half-clean stages (sketchml_amd/csrc/skml_halfclean.hpp)
against the plain stages, on the host: tests/halfclean_check.cpp instantiates the shipped template
with a host ops policy for R = 4..64 and both stage counts in use, over every 0-1 cyclic-bitonic
input (R (R - 1) + 2 each) and 20,000 random float bitonic inputs with duplicates, +-inf and equal
runs per case."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ZERO_ONE = sum(2 * (r * (r - 1) + 2) for r in (4, 8, 16, 32, 64))
RANDOM = 5 * 2 * 20000


def test_paired_halfclean_matches_plain_stages():
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "halfclean_check")
        subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "halfclean_check.cpp")],
                       check=True)
        out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip() == f"ok {ZERO_ONE + RANDOM}", out.stdout
