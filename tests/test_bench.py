"""bench.py's command line: --steps is the number of timed steps, and --dump-outputs writes what the last timed step
computed, within its size budget, with the same elements on every run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_dump_outputs_keeps_small_arrays_and_samples_large_ones_reproducibly(tmp_path):
    g = torch.Generator().manual_seed(3)
    arrays = [("small", torch.randn(2, 5, generator=g)), ("large", torch.arange(5000, dtype=torch.float64)),
              ("half", torch.randn(300, generator=g).to(torch.bfloat16))]
    budget = 3 * 4 * 100                                   # 100 float32 elements per array
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), arrays, budget=budget)
    small = np.load(tmp_path / "a" / "small.npy")
    assert small.dtype == np.float32 and small.shape == (2, 5) and np.array_equal(small, arrays[0][1].numpy())
    large = np.load(tmp_path / "a" / "large.npy")
    assert large.dtype == np.float32 and large.shape == (100,)
    assert np.all(np.diff(large) > 0) and large.min() >= 0 and large.max() < 5000      # distinct elements, in index order
    half = np.load(tmp_path / "a" / "half.npy")
    assert half.dtype == np.float32 and half.shape == (100,) and np.isin(half, arrays[2][1].float().numpy()).all()
    for name in ("small", "large", "half"):
        assert np.array_equal(np.load(tmp_path / "a" / (name + ".npy")), np.load(tmp_path / "b" / (name + ".npy")))


def test_steps_must_be_positive(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "3", "--dump-outputs", "out"])
    args = bench.parse()
    assert args.steps == 3 and args.dump_outputs == "out"
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "0"])
    with pytest.raises(SystemExit):
        bench.parse()


@pytest.mark.gpu
def test_bench_dumps_the_last_timed_step(gpu, tmp_path):
    out = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "4",
           "--no-side-leg", "--no-cpu-baseline", "--dump-outputs", str(out)]
    run = subprocess.run(cmd, cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-3000:]
    line = json.loads(run.stdout.strip().splitlines()[-1])
    assert line["steps"] == 3 and line["ms_per_step"] > 0
    names = ["losses", "fake_imgs_64", "fake_imgs_128", "fake_imgs_256", "mu", "logvar", "emb_grad", "netG", "netG_ema",
             "netD0", "netD1", "netD2"]
    assert sorted(os.listdir(out)) == sorted(n + ".npy" for n in names)
    assert sum(os.path.getsize(out / (n + ".npy")) for n in names) <= 64 * 10**6
    got = {n: np.load(out / (n + ".npy")) for n in names}
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in got.values())
    losses = line["losses"]
    assert np.array_equal(got["losses"], np.float32([losses["errD_total"], losses["errG_total"], losses["kl"]]))
    for s in (64, 128, 256):
        assert got["fake_imgs_%d" % s].shape == (4, 3, s, s)
    assert got["emb_grad"].shape == (4, 1024) and np.abs(got["emb_grad"]).max() > 0
