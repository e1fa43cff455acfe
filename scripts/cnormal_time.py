#!/usr/bin/env python3
"""Warm, device-synchronised public ConditionalNormal.fit calls on the GPU at the reference's defaults (n = 100, d = 5,
c = 3: 10 epochs of batch 32 = 40 steps), next to the same 40 steps on the host's CPU (16 threads) through the float32
torch restatement of the reference (tests/cnormal_torch.py: autograd + torch.optim.Adam, the reference's operations --
the reference itself is not part of this repository); and one large-batch figure: n = 1M, batch 65 536,
hidden (128, 128), d = 5, c = 3, as time per step of one epoch (16 steps).  One warm-up per shape, then `reps` timed
runs (median reported).

    python scripts/cnormal_time.py [reps]
"""
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cnormal_torch as ct  # noqa: E402
from probaforms_amd.models import ConditionalNormal  # noqa: E402


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), min(ts)


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    assert torch.cuda.is_available(), "needs a HIP device"
    torch.set_num_threads(16)
    print("device:", torch.cuda.get_device_name(0), "| CPU threads:", torch.get_num_threads())
    rng = np.random.default_rng(105)
    n, d, c = 100, 5, 3
    X = rng.normal(size=(n, d)).astype(np.float32)
    C = rng.normal(size=(n, c)).astype(np.float32)
    m = ConditionalNormal()

    def gpu_fit():
        torch.manual_seed(0)
        m.fit(X, C)
        torch.cuda.synchronize()

    med, lo = timed(gpu_fit, reps)
    steps = len(m.loss_history)
    print("GPU  default n=100 d=5 c=3: %d steps: fit median %.2f ms (min %.2f, %d fits) = %.1f us per step; last loss %.5f"
          % (steps, med * 1e3, lo * 1e3, reps, med / steps * 1e6, float(m.loss_history[-1])), flush=True)

    net = ct.Normal(d, c)
    p0 = m.model._core.flat[:net.P].cpu().numpy()

    def cpu_fit():
        torch.manual_seed(0)
        epochs, _ = ct.replay_draws(torch.get_rng_state(), n, 32, d, 10)
        ct.fit(net, p0, X, C, [b for e in epochs for b in e], 1e-4, 0, torch.float32)

    med, lo = timed(cpu_fit, reps)
    print("CPU  the same 40 steps, float32 torch restatement, 16 threads: median %.2f ms (min %.2f) = %.1f us per step"
          % (med * 1e3, lo * 1e3, med / 40 * 1e6), flush=True)

    n, B = 1 << 20, 65536
    X = rng.normal(size=(n, d)).astype(np.float32)
    C = rng.normal(size=(n, c)).astype(np.float32)
    big = ConditionalNormal(hidden=(128, 128), batch_size=B, n_epochs=1)
    med, lo = timed(lambda: (big.fit(X, C), torch.cuda.synchronize()), max(2, reps // 2))
    steps = len(big.loss_history)
    print("GPU  n=1M d=5 c=3 hidden=(128,128) batch=65536: one epoch of %d steps incl. upload and shuffle: median %.1f ms "
          "(min %.1f) = %.2f ms per step; last loss %.5f"
          % (steps, med * 1e3, lo * 1e3, med / steps * 1e3, float(big.loss_history[-1])), flush=True)


if __name__ == "__main__":
    main()
