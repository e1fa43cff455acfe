#!/usr/bin/env python3
"""Warm, device-synchronised public ConditionalWGAN.fit calls on the GPU, for the two shapes the reference was timed at
on the CPU: the reference's own test shape with every default (n = 100, d = 5, c = 3: 1000 epochs of batch 32 = 4000
iterations + 1000 epoch-end passes) and n = 20 000, d = 16, c = 4, batch 256 (79 iterations per epoch).  One warm-up
fit per shape, then `reps` timed fits (median reported).  --trace runs each shape once with fewer epochs, for
rocprofv3 --kernel-trace.

    python scripts/wgan_time.py [reps] [--trace]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from probaforms_amd.models import ConditionalWGAN  # noqa: E402

SHAPES = [   # (label, n, d, c, constructor kwargs)
    ("default n=100 d=5 c=3", 100, 5, 3, dict()),
    ("n=20000 d=16 c=4 batch=256", 20000, 16, 4, dict(batch_size=256, n_epochs=20)),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("reps", nargs="?", type=int, default=3)
    ap.add_argument("--trace", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    print("device:", torch.cuda.get_device_name(0))
    for label, n, d, c, kw in SHAPES:
        rng = np.random.default_rng(n + d)
        X = rng.normal(size=(n, d)).astype(np.float32)
        C = rng.normal(size=(n, c)).astype(np.float32)
        if a.trace:
            kw = dict(kw, n_epochs=50 if n <= 1000 else 3)
        torch.manual_seed(0)
        m = ConditionalWGAN(**kw)
        m.fit(X, C)
        torch.cuda.synchronize()
        if a.trace:
            print("%s: traced fit, %d epochs" % (label, m.n_epochs), flush=True)
            continue
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            m.fit(X, C)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        iters = m.n_epochs * -(-n // m.batch_size)
        med = statistics.median(ts)
        print("%s: %d epochs, %d iterations: fit median %.3f s (min %.3f, %d fits) = %.3f ms per epoch, %.1f us per "
              "iteration incl. epoch ends; last losses gen %.5f disc %.5f"
              % (label, m.n_epochs, iters, med, min(ts), a.reps, med / m.n_epochs * 1e3, med / iters * 1e6,
                 float(m.gen_loss_history[-1]), float(m.disc_loss_history[-1])), flush=True)


if __name__ == "__main__":
    main()
