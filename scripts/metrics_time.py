#!/usr/bin/env python3
"""Warm, device-synchronised call times of probaforms_amd.metrics (n_iters = 100): maximum_mean_discrepancy and
frechet_distance at n = 1000, 5000, 50 000 rows per sample, d = 2 and 16.  Each call is the public one, numpy in,
(mean, std) out: host index draw, upload, kernels, copy back.  One warm-up call per shape, then `reps` timed calls
(median reported).

    python scripts/metrics_time.py [reps] [--only mmd|fd] [--max-n N]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from probaforms_amd.metrics import frechet_distance, maximum_mean_discrepancy  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("reps", nargs="?", type=int, default=3)
    ap.add_argument("--only", choices=("mmd", "fd"))
    ap.add_argument("--max-n", type=int, default=50000)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    print("device:", torch.cuda.get_device_name(0))
    fns = [("mmd", maximum_mean_discrepancy), ("fd", frechet_distance)]
    for name, fn in fns:
        if a.only and a.only != name:
            continue
        for n in (1000, 5000, 50000):
            if n > a.max_n:
                continue
            for d in (2, 16):
                rng = np.random.default_rng(n + d)
                X = rng.normal(size=(n, d))
                Y = rng.normal(size=(n, d)) + 0.05
                np.random.seed(0)
                fn(X, Y, n_iters=100)
                torch.cuda.synchronize()
                ts = []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    mu, sd = fn(X, Y, n_iters=100)
                    torch.cuda.synchronize()
                    ts.append(time.perf_counter() - t0)
                pairs = (2 * n) ** 2 / 2 * 100
                extra = ("  %.2e pair evaluations per pass" % pairs) if name == "mmd" else ""
                print("%-3s n=%6d d=%2d n_iters=100: median %9.2f ms (min %9.2f, %d calls)  mean=%.6g std=%.3g%s"
                      % (name, n, d, statistics.median(ts) * 1e3, min(ts) * 1e3, a.reps, mu, sd, extra), flush=True)


if __name__ == "__main__":
    main()
