"""bench.py's command line: a plain run is the headline alone (the other options need --full), and --dump-outputs
writes the headline's outputs as float32 / float64 .npy files below 64 MB."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench  # (the repository root is on sys.path: tests/conftest.py)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("opt", [["--workload", "embedder"], ["--streams", "1"], ["--no-cpu-baseline"], ["--min-seconds", "0.1"]])
def test_plain_run_refuses_full_options(opt):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2"] + opt,
                         capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert out.returncode == 2 and "only with --full" in out.stderr, out.stderr[-2000:]


def _outs(nb, N, C=1, K=512, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(nb * N, C, generator=g), torch.randn(nb, C, generator=g), torch.rand(nb * N, C, generator=g),
            torch.randn(nb, C, K, generator=g), torch.randint(0, N, (nb, C), generator=g))


def test_host_outputs_names_dtypes_and_values():
    o = _outs(4, 100)
    arrs = bench._host_outputs({"batch0": o})
    assert sorted(arrs) == sorted(f"batch0_{f}" for f in ("classes", "prediction_bag", "A", "B", "critical_idx"))
    assert arrs["batch0_critical_idx"].dtype == np.float64 and np.array_equal(arrs["batch0_critical_idx"], o[4].numpy())
    for f, t in (("classes", o[0]), ("prediction_bag", o[1]), ("A", o[2]), ("B", o[3])):
        assert arrs["batch0_" + f].dtype == np.float32 and np.array_equal(arrs["batch0_" + f], t.numpy())


def test_host_outputs_sample_a_larger_output_the_same_way_every_time():
    outs = {f"batch{i}": _outs(64, 60000, seed=i) for i in range(3)}   # 3 x 30.9 MB
    a, b = bench._host_outputs(outs), bench._host_outputs(outs)
    assert sum(x.nbytes for x in a.values()) <= bench.DUMP_LIMIT_BYTES < 64 * 10 ** 6
    assert all(np.array_equal(a[k], b[k]) for k in a)
    assert a["batch1_B"].shape == (64, 1, 512)                                    # small outputs stay whole
    full = outs["batch2"][0].numpy().ravel()
    assert a["batch2_classes"].size < full.size and np.isin(a["batch2_classes"], full).all()


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_its_outputs(tmp_path):
    d = tmp_path / "out"
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                          "--dump-outputs", str(d)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    line = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert line["unit"] == "bags/s" and line["value"] > 0 and line["steps"] == 2 and line["higher_is_better"] is True
    assert line["config"]["passes_per_step"] == bench.HEADLINE_PASSES_PER_STEP
    assert line["ms_per_step"] == pytest.approx(line["config"]["timed_region_s"] * 1e3 / 2, rel=0.01)
    assert "summary" not in line and "cpu_baseline" not in line
    files = sorted(os.listdir(d))
    assert len(files) == 15 and sum(os.path.getsize(d / f) for f in files) < 64 * 10 ** 6
    for i in range(3):
        A = np.load(d / f"batch{i}_A.npy")
        assert A.dtype == np.float32 and A.shape == (64 * 10000, 1)
        np.testing.assert_allclose(A.reshape(64, 10000).sum(1), 1.0, atol=1e-4)
        assert np.isfinite(np.load(d / f"batch{i}_prediction_bag.npy")).all()
