#!/usr/bin/env python3
"""Warm, device-synchronised call times of the eight 1-D metrics (probaforms_amd.metrics.ks1d / div1d), n_iters = 100,
default bins, at n = 1 000 and 10 000 rows per sample, d = 2 and 16.  Each call is the public one, numpy in, (mean, std)
out: host index draw, upload, the per-call sort, kernels, copy back and the host finishing.  One warm-up call per
(metric, shape), then `reps` timed calls (median reported).

    python scripts/metrics1d_time.py [reps] [--max-n N]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from probaforms_amd.metrics import div1d, ks1d  # noqa: E402

NAMES = ("kolmogorov_smirnov_1d", "cramer_von_mises_1d", "anderson_darling_1d", "roc_auc_score_1d",
         "kullback_leibler_1d", "jensen_shannon_1d", "kullback_leibler_1d_kde", "jensen_shannon_1d_kde")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("reps", nargs="?", type=int, default=3)
    ap.add_argument("--max-n", type=int, default=10000)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    print("device:", torch.cuda.get_device_name(0))
    for name in NAMES:
        fn = getattr(ks1d if hasattr(ks1d, name) else div1d, name)
        for n in (1000, 10000):
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
                print("%-24s n=%6d d=%2d n_iters=100: median %9.2f ms (min %9.2f, %d calls)  mean=%.6g std=%.3g"
                      % (name, n, d, statistics.median(ts) * 1e3, min(ts) * 1e3, a.reps, mu, sd), flush=True)


if __name__ == "__main__":
    main()
