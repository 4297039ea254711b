"""Host-side check of Gradient.sum's batch planner (no GPU): plan_sum_batches of
sketchml_amd/csrc/skml_sparse_sum_plan.hpp as a stand-alone program (tests/sum_plan_check.cpp) under
the address and undefined-behaviour sanitizers, against the restatement below in Python's unbounded
integers.

The sparse decode-sum (skml_sparse_blob.cpp, decode_sum_any) restores its payloads in batches whose
scratch fits a budget; a later batch continues the sum.  The plan is greedy in payload order and a
batch always takes at least one payload, so a payload above the budget still gets summed, alone."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE_MAX = 2**64 - 1
GIB3 = 3 << 30


def plan(need, budget):
    """The batches' end indices: payloads in order, a batch closes before the first payload that
    would take its bytes above the budget, and never before it holds one."""
    ends, count, total = [], 0, 0
    for p, n in enumerate(need):
        if count and total + n > budget:
            ends.append(p)
            count = total = 0
        count += 1
        total += n
    if need:
        ends.append(len(need))
    return ends


def test_the_budget_hook_returns_the_previous_setting():
    """skml_debug_sparse_sum_budget and _lib.sum_budget touch no device: a value that is not positive
    means the library's own budget (reported as 0), and the context manager puts the previous
    setting back, on the way out of a failure too."""
    from sketchml_amd import _lib as L
    assert L.lib.skml_debug_sparse_sum_budget(0) == 0
    try:
        assert L.lib.skml_debug_sparse_sum_budget(4096) == 0
        assert L.lib.skml_debug_sparse_sum_budget(-5) == 4096
        assert L.lib.skml_debug_sparse_sum_budget(77) == 0
        with L.sum_budget(1):
            assert L.lib.skml_debug_sparse_sum_budget(1) == 1
            with pytest.raises(ZeroDivisionError):
                with L.sum_budget(123):
                    assert L.lib.skml_debug_sparse_sum_budget(123) == 123
                    1 // 0
            assert L.lib.skml_debug_sparse_sum_budget(1) == 1
        assert L.lib.skml_debug_sparse_sum_budget(77) == 77
        with L.sum_budget(0):
            assert L.lib.skml_debug_sparse_sum_budget(0) == 0
        assert L.lib.skml_debug_sparse_sum_budget(77) == 77
    finally:
        L.lib.skml_debug_sparse_sum_budget(0)
    assert L.lib.skml_debug_sparse_sum_path(None, None) == L.SKML_E_ARG
    batches, launches = L.sum_path()
    assert 0 <= batches <= launches + 1   # whatever this thread summed last; + 1: a sum that failed inside a batch


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    """Builds the program once; returns run(lines) -> the number of checks it made."""
    d = tmp_path_factory.mktemp("sum_plan")
    exe = str(d / "sum_plan_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", exe, os.path.join(ROOT, "tests", "sum_plan_check.cpp")],
                   check=True)
    count = [0]

    def run(lines):
        count[0] += 1
        script = str(d / f"script{count[0]}.txt")
        with open(script, "w") as f:
            f.write("\n".join(lines) + "\n")
        out = subprocess.run([exe, script], capture_output=True, text=True, timeout=60)
        m = re.fullmatch(r"ok (\d+) checks\n", out.stdout)
        assert out.returncode == 0 and m and not out.stderr, out.stdout + out.stderr
        return int(m.group(1))

    return run


def _line(need, budget, ends=None):
    ends = plan(need, budget) if ends is None else ends
    assert ends == plan(need, budget)
    return " ".join(str(x) for x in ["plan", budget, len(need), *need, len(ends), *ends])


def test_the_restatement_has_the_properties():
    """What the program is compared with is itself held to the contract, in unbounded integers."""
    rng = np.random.default_rng(3)
    for _ in range(300):
        P = int(rng.integers(1, 24))
        need = [int(x) for x in rng.integers(1, 1000, P)]
        budget = int(rng.integers(1, 4000))
        ends = plan(need, budget)
        starts = [0] + ends[:-1]
        assert ends[-1] == P and all(e > s for s, e in zip(starts, ends))  # exactly one batch each, in order
        for s, e in zip(starts, ends):
            assert e - s == 1 or sum(need[s:e]) <= budget
            assert e == P or sum(need[s:e + 1]) > budget                   # greedy


def test_plans_equal_the_restatement(checker):
    rng = np.random.default_rng(4)
    lines = [_line([], 100, [])]
    for _ in range(400):
        P = int(rng.integers(1, 24))
        hi = int(rng.choice([2, 10, 1000, 2**40]))
        need = [int(x) for x in rng.integers(1, hi + 1, P)]
        budget = int(rng.integers(1, 4 * hi + 1))
        lines.append(_line(need, budget))
    assert checker(lines) > 4000


def test_edges_of_the_budget(checker):
    need = [5000, 1, 70000, 1024, 1024, 33]
    P, total = len(need), sum(need)
    lines = [
        _line(need, 1, list(range(1, P + 1))),       # a budget of 1 byte: P batches, none empty
        _line(need, total, [P]),                     # the exact sum: one batch
        _line(need, total - 1, [P - 1, P]),          # one byte less: the last payload moves on
        _line(need, SIZE_MAX, [P]),
        _line([7], 1, [1]), _line([7], 7, [1]), _line([7], 6, [1]),
        _line([4, 4, 4, 4], 8, [2, 4]),              # a batch filled to the byte
        _line([4, 4, 4, 4], 7, [1, 2, 3, 4]),
        _line([9, 1, 1, 9, 1], 2, [1, 3, 4, 5]),     # payloads above the budget between ones that fit
        _line([GIB3, 1], GIB3, [1, 2]),              # the library's own budget
        _line([GIB3 - 1, 1, 1], GIB3, [2, 3]),
    ]
    assert checker(lines) > 60


def test_needs_near_the_top_of_size_t_do_not_wrap(checker):
    """P needs of about SIZE_MAX / P: their running sum stays representable only until the last;
    needs above that wrap any sum that is formed before it is compared."""
    lines = []
    for P in (2, 3, 8, 19):
        each = SIZE_MAX // P
        lines.append(_line([each] * P, SIZE_MAX, [P]))                   # the whole sum just fits
        lines.append(_line([each + 1] * P, SIZE_MAX))                    # the last one would wrap to a small number
        lines.append(_line([each + 1] * P, each + 1, list(range(1, P + 1))))
        lines.append(_line([each] * P, GIB3, list(range(1, P + 1))))
        assert plan([each + 1] * P, SIZE_MAX) == [P - 1, P]
    lines.append(_line([SIZE_MAX, SIZE_MAX, 1, SIZE_MAX], SIZE_MAX, [1, 2, 3, 4]))
    lines.append(_line([SIZE_MAX - 1, 1, 1], SIZE_MAX, [2, 3]))
    lines.append(_line([1, SIZE_MAX, 1], 2, [1, 2, 3]))                  # 1 + SIZE_MAX wraps to 0 <= 2
    lines.append(_line([2, SIZE_MAX - 1, 5], 3, [1, 2, 3]))              # a wrapped sum of 0, then 5 > 3
    assert checker(lines) > 100
