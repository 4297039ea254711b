"""bench.py's plain run (set up, warm up, time --steps encodes, print the line; everything else is
behind --full) and --dump-outputs: the .npy files hold the payload of the last timed step, which is
the encode of a known rotating bucket whatever the warm-up's length was, so the same arguments give
the same files from run to run and from build to build."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 1 << 20
STEPS = 3


@pytest.fixture(scope="module")
def plain_run(tmp_path_factory):
    out = tmp_path_factory.mktemp("bench_dump")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--n", str(N), "--steps", str(STEPS),
                        "--warmup", "2", "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=110, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1]), out


def test_plain_run_reports_the_headline_only(plain_run):
    line, _ = plain_run
    assert line["metric"].startswith("device-resident grad encode GB/s") and line["unit"] == "GB/s"
    assert line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["steps"] == STEPS and line["ms_per_step"] > 0
    # value is the fp32 input rate of the timed steps (both figures are rounded in the line)
    assert line["value"] == pytest.approx(4.0 * N / (line["ms_per_step"] * 1e-3) / 1e9, rel=2e-2)
    assert line["full"] is False and line["roofline"] is None and line["cpu_baseline"] is None
    assert not {"kernels", "decode", "host_path", "other_configs"} & set(line["extras"])


def test_dump_is_the_payload_of_the_last_timed_step(gpu, plain_run):
    import torch
    line, out = plain_run
    files = sorted(os.listdir(out))
    assert files == ["codes.npy", "header.npy", "splits.npy"]
    assert sum(os.path.getsize(os.path.join(out, f)) for f in files) <= 64 * 10**6
    header, splits, codes = (np.load(os.path.join(out, f + ".npy")) for f in ("header", "splits", "codes"))
    assert header.dtype == np.float64 and splits.dtype == np.float64 and codes.dtype == np.float32
    # the timed region starts on rotating bucket 0, so its last step encoded bucket STEPS - 1
    # (seed 6 + 1000 * bucket on rank 0, encode seed 6)
    assert line["config"]["rotating_buffers"] > STEPS
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(6 + 1000 * (STEPS - 1))
    x = torch.randn(N, device="cuda:0", generator=gen)
    q = gpu.QuantileQuantizer(256, seed=6)
    q.quantize(x)
    assert q.codeBits() == 8
    assert header.tolist() == [N, q.getBinNum(), q.getZeroIdx(), 8, 256, q.getMin(), q.getMax()]
    assert np.array_equal(splits, q.getSplits())
    assert np.array_equal(codes.astype(np.int32), q.getBins().cpu().numpy())
