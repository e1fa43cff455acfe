#!/usr/bin/env python3
"""Warm, device-synchronised call times of probaforms_amd.metrics.wasserstein, n_iters = 100, at n = 1 000 and 10 000 rows
per sample, d = 2 and 16: wasserstein_1d with p = 1 and p = 2, sliced_wasserstein_distance with its defaults (64
projections, p = 2), and kolmogorov_smirnov_1d from the same process as the yardstick (the same pipeline -- index draw, sort,
draw counts -- with its own scan kernel).  Each call is the public one, numpy in, (mean, std) out.  One warm-up call per
(call, shape), then `reps` timed calls (median reported), and the number of index groups (_boot.run_groups) the call ran as.

    python scripts/wasserstein_time.py [reps] [--max-n N] [--shape NxD] [--only NAME]

Under `rocprofv3 --kernel-trace --stats -- python scripts/wasserstein_time.py 1 --shape 10000x16` the kernels' own times at one
shape: k_wp (p = 2), k_w1 (p = 1) and k_project beside k_scan1d<0> (KS) and k_counts; each call then runs twice (warm-up and one).
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from probaforms_amd.metrics import _boot, _lib, ks1d, wasserstein  # noqa: E402

N_ITERS = 100


def ks_groups(n, d):
    G = _boot.group_size(N_ITERS, 2 * n, _lib.metric1d_workspace_bytes(_lib.M1D_KS, n, n, d, 1, 1))
    return -(-N_ITERS // G)


# name -> (call, number of index groups at n rows per sample and d features)
CALLS = {
    "kolmogorov_smirnov_1d": (lambda X, Y: ks1d.kolmogorov_smirnov_1d(X, Y, n_iters=N_ITERS), ks_groups),
    "wasserstein_1d p=1": (lambda X, Y: wasserstein.wasserstein_1d(X, Y, n_iters=N_ITERS, p=1),
                           lambda n, d: wasserstein.index_groups(n, n, d, N_ITERS, 1)),
    "wasserstein_1d p=2": (lambda X, Y: wasserstein.wasserstein_1d(X, Y, n_iters=N_ITERS, p=2),
                           lambda n, d: wasserstein.index_groups(n, n, d, N_ITERS, 2)),
    "sliced_wasserstein_distance": (lambda X, Y: wasserstein.sliced_wasserstein_distance(X, Y, n_iters=N_ITERS),
                                    lambda n, d: wasserstein.index_groups(n, n, 64, N_ITERS, 2)),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("reps", nargs="?", type=int, default=3)
    ap.add_argument("--max-n", type=int, default=10000)
    ap.add_argument("--shape", default=None, help="one shape only: rows per sample x features, e.g. 10000x16")
    ap.add_argument("--only", default=None, help="time only the calls whose name starts with this")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    print("device:", torch.cuda.get_device_name(0))
    shapes = [(n, d) for n in (1000, 10000) if n <= a.max_n for d in (2, 16)]
    if a.shape is not None:
        shapes = [tuple(int(v) for v in a.shape.split("x"))]
    for name, (fn, groups) in CALLS.items():
        if a.only is not None and not name.startswith(a.only):
            continue
        for n, d in shapes:
            rng = np.random.default_rng(n + d)
            X = rng.normal(size=(n, d))
            Y = rng.normal(size=(n, d)) + 0.05
            np.random.seed(0)
            fn(X, Y)
            torch.cuda.synchronize()
            ts = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                mu, sd = fn(X, Y)
                torch.cuda.synchronize()
                ts.append(time.perf_counter() - t0)
            print("%-28s n=%6d d=%2d n_iters=%d: median %9.2f ms (min %9.2f, %d calls, %d index groups)  mean=%.6g std=%.3g"
                  % (name, n, d, N_ITERS, statistics.median(ts) * 1e3, min(ts) * 1e3, a.reps, groups(n, d), mu, sd),
                  flush=True)


if __name__ == "__main__":
    main()
