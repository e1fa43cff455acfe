#!/usr/bin/env python3
"""Warm timings of probaforms_amd.metrics.twosample.knn_test, n_permutations = 999, nearest_k = 1 and 5, at n = 1 000 and 10 000
rows per sample and d = 2 and 16 features, in one process (profiles/r19_knntest_time.txt):
  (a) knn_test(X, Y, nearest_k=k): numpy in, KnnTest out;
  (k) where (a)'s time goes on the device: pfm_nn_index, pfm_perm_labels and pfm_nn_count between device events in one more
      call, as shares of that call's wall time (the rest is the host: conversion, upload, the seed draw, the ratios);
  (e) energy_test(X, Y) on the same data, the test a user has today;
  (ii) what a user can do today on the same device in float64, a yardstick for time only: one torch.cdist of the pooled sample,
      topk(k + 1, largest=False) with the first column (the row itself) dropped, the labellings from np.random.permutation on
      the host, uploaded as bytes [1 + n_permutations, 2 n], and a gather of the neighbours' labels.  torch's peak allocator
      bytes are reported beside it.
Each variant is warmed for as many calls as are timed; the figure is the median wall time per call with a device synchronisation
at both ends, with the fastest and slowest call.  The statistic's difference between (a) and (ii) is printed: (ii) is a yardstick
for time, tests/test_knntest_gpu.py holds (a) against a float64 scipy restatement.

    python scripts/knntest_time.py [out.txt] [--reps N] [--yard-reps N] [--shape NxD] [--only-tests]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from probaforms_amd.metrics import _lib, twosample  # noqa: E402

N_PERM = 999
KS = (1, 5)


def timed(fn, reps):
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def kernel_shares(fn):
    """one call of fn with pfm_nn_index, pfm_perm_labels and pfm_nn_count between device events -> ({name: ms}, wall ms)"""
    spans = {"nn_index": [], "perm_labels": [], "nn_count": []}
    saved = {name: getattr(_lib, name) for name in spans}

    def wrap(name):
        def call(*a):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            saved[name](*a)
            e1.record()
            spans[name].append((e0, e1))
        return call

    try:
        for name in spans:
            setattr(_lib, name, wrap(name))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
    finally:
        for name, f in saved.items():
            setattr(_lib, name, f)
    return {name: sum(a.elapsed_time(b) for a, b in ev) for name, ev in spans.items()}, wall


def host_labels(nr, nf, n_perm):
    """[1 + n_perm, nr + nf] uint8: 1 on the rows labelled real; the observed labelling first"""
    L = np.zeros((1 + n_perm, nr + nf), np.uint8)
    L[0, :nr] = 1
    for p in range(n_perm):
        L[1 + p, np.random.permutation(nr + nf)[:nr]] = 1
    return L


def torch_test(Zd, nr, nf, n_perm, k):
    """(statistic, p-value) with torch operations on the device"""
    L = torch.from_numpy(host_labels(nr, nf, n_perm)).cuda()
    D = torch.cdist(Zd, Zd, compute_mode="donot_use_mm_for_euclid_dist")
    nbr = D.topk(k + 1, dim=1, largest=False).indices[:, 1:]
    del D
    V = (L[:, nbr] == L[:, :, None]).sum(dim=(1, 2)).double().cpu().numpy() / float((nr + nf) * k)
    return V[0], (1 + int((V[1:] >= V[0]).sum())) / (1 + n_perm)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=None)
    ap.add_argument("--reps", type=int, default=5, help="timed calls of each test (and as many warm-up calls)")
    ap.add_argument("--yard-reps", type=int, default=2, help="timed calls of the yardstick")
    ap.add_argument("--shape", default=None, help="one shape only: rows per sample x features, e.g. 10000x16")
    ap.add_argument("--only-tests", action="store_true", help="skip the yardstick")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    out = open(a.out, "w") if a.out else sys.stdout
    print("median [min .. max] ms per call; warm-up = as many calls as timed; n_permutations = %d; %s"
          % (N_PERM, torch.cuda.get_device_name(0)), file=out)
    shapes = [(n, d) for n in (1000, 10000) for d in (2, 16)]
    if a.shape is not None:
        shapes = [tuple(int(v) for v in a.shape.split("x"))]
    for n, d in shapes:
        rng = np.random.default_rng(n + d)
        X, Y = rng.normal(size=(n, d)), rng.normal(0.02, 1.0, size=(n, d))
        Zd = torch.from_numpy(np.concatenate([X, Y])).cuda()
        print("\nn = %d rows per sample, d = %d" % (n, d), file=out)

        def energy():
            np.random.seed(0)
            return twosample.energy_test(X, Y, n_permutations=N_PERM)

        emed, elo, ehi = timed(energy, a.reps)
        e = energy()
        print("  %-46s %10.2f  [%9.2f .. %9.2f]   statistic %.6g  p %.3f" % ("(e) energy_test", emed, elo, ehi, e.statistic, e.pvalue),
              file=out)
        out.flush()
        for k in KS:
            def ours():
                np.random.seed(0)
                return twosample.knn_test(X, Y, n_permutations=N_PERM, nearest_k=k)

            med, lo, hi = timed(ours, a.reps)
            t = ours()
            print("  %-46s %10.2f  [%9.2f .. %9.2f]   statistic %.6g  p %.3f   (e) / (a) %.2f x"
                  % ("(a) knn_test, nearest_k = %d" % k, med, lo, hi, t.statistic, t.pvalue, emed / med), file=out)
            ms, wall = kernel_shares(ours)
            print("  %-46s %s of a call of %.2f ms" % ("(k) on the device", ", ".join("pfm_%s %.3f ms (%.0f%%)" % (
                name, v, 100 * v / wall) for name, v in ms.items()), wall), file=out)
            out.flush()
            if a.only_tests:
                continue

            def yardstick():
                np.random.seed(0)
                return torch_test(Zd, n, n, N_PERM, k)

            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            tmed, tlo, thi = timed(yardstick, a.yard_reps)
            peak = torch.cuda.max_memory_allocated() - base
            stat, p = yardstick()
            print("  %-46s %10.2f  [%9.2f .. %9.2f]   peak allocator bytes %.1f MB" % ("(ii) torch cdist, topk, gather, host labellings",
                                                                                   tmed, tlo, thi, peak / 1e6), file=out)
            print("  %-46s %10.2f x   |statistic (a) - (ii)| %.3g, p (ii) %.3f" % ("(ii) / (a)", tmed / med, abs(stat - t.statistic), p),
                  file=out)
            out.flush()
    if out is not sys.stdout:
        out.close()


if __name__ == "__main__":
    main()
