"""bench.py's plain run (the headline line only) and --dump-outputs: what the last timed step computed, as .npy files."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "n_gpus", "config")
FULL_ONLY = ("roofline", "roofline_kernels", "device_resident", "api_level", "secondary_configs", "cpu_baseline", "logprob_mae")


def test_dump_outputs_writes_a_fixed_bounded_sample_in_float32(tmp_path):
    import bench
    g = torch.Generator().manual_seed(0)
    xs = torch.randn(1_000_000, 16, generator=g); losses = torch.randn(16, generator=g); params = torch.randn(75_000, generator=g)
    bench.dump_outputs(str(tmp_path / "a"), xs, losses, params)
    bench.dump_outputs(str(tmp_path / "b"), xs, None, params)
    a = {f: np.load(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")}
    assert sorted(a) == ["losses.npy", "params.npy", "samples.npy"] and sorted(os.listdir(tmp_path / "b")) == ["params.npy", "samples.npy"]
    assert all(v.dtype == np.float32 for v in a.values()) and sum(v.nbytes for v in a.values()) <= 64 << 20
    np.testing.assert_array_equal(a["losses.npy"], losses.numpy())
    np.testing.assert_array_equal(a["params.npy"], params.numpy())
    s = a["samples.npy"]
    assert s.shape == (bench.DUMP_SAMPLE_BYTES // 64, 16)
    np.testing.assert_array_equal(s, np.load(tmp_path / "b" / "samples.npy"))            # the same rows every time
    rows = np.sort(np.random.default_rng(bench.DUMP_SAMPLE_SEED).choice(1_000_000, size=s.shape[0], replace=False))
    np.testing.assert_array_equal(s, xs.numpy()[rows])
    bench.dump_outputs(str(tmp_path / "c"), torch.zeros(2_000_000, 64), None, params)     # C4: wider rows, fewer of them
    assert np.load(tmp_path / "c" / "samples.npy").nbytes <= bench.DUMP_SAMPLE_BYTES


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_plain_run_times_exactly_the_steps_asked_and_dumps_the_last_one(tmp_path):
    out = tmp_path / "outputs"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(out)], cwd=ROOT, capture_output=True, text=True, timeout=500)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1
    j = json.loads(lines[0])
    for k in HEADLINE:
        assert k in j, k
    assert not [k for k in FULL_ONLY if k in j]
    assert j["steps"] == 3 and j["warmup"] == 1 and j["timed_blocks"] == 1 and j["higher_is_better"] is True
    assert j["unit"] == "rows/s" and j["dtype"].startswith("f32")
    assert j["ms_per_step"] > 0 and abs(j["value"] - 2 * 1_000_000 / (j["ms_per_step"] * 1e-3)) < 1e-6 * j["value"]
    samples, losses, params = (np.load(out / f) for f in ("samples.npy", "losses.npy", "params.npy"))
    assert samples.dtype == losses.dtype == params.dtype == np.float32
    assert samples.shape[1] == 16 and np.isfinite(samples).all() and np.isfinite(params).all()
    assert losses.shape == (16,) and losses[-1] == np.float32(j["config"]["final_loss"])     # the last timed epoch's losses
