#!/usr/bin/env python3
"""Warm timings of probaforms_amd.metrics.twosample.energy_test and mmd_test, n_permutations = 999, at n = 1 000 and 10 000 rows
per sample and d = 2 and 16 features, in one process (profiles/r18_twosample_time.txt):
  (a) energy_test(X, Y) / mmd_test(X, Y): numpy in, TwoSampleTest out;
  (ii) what a user can do today on the same device in float64, a yardstick for time only: the labellings from
      np.random.permutation on the host, uploaded as a weight matrix S [1 + n_permutations, 2 n]; one torch.cdist of the pooled
      sample (for mmd_test its median and exp(-gamma D^2) on top); ((S @ D) * S).sum(1).  torch's peak allocator bytes are
      reported beside it;
  (c) the host's np.random.permutation draws of (ii) alone, as a share of (ii).
Each variant is warmed for as many calls as are timed; the figure is the median wall time per call with a device synchronisation
at both ends, with the fastest and slowest call.  The statistic's difference between (a) and (ii) is printed: (ii) is a yardstick
for time, tests/test_twosample_gpu.py holds (a) against a float64 scipy restatement.

    python scripts/twosample_time.py [out.txt] [--reps N] [--yard-reps N] [--shape NxD] [--only-tests]

Under `rocprofv3 --kernel-trace --stats -- python scripts/twosample_time.py --only-tests --reps 1 --shape 10000x16` the kernels' own
times at one shape: k_perm_labels, k_perm_tiles and k_quad_finish<1> of both tests, and pfm_mmd's median kernels (each test then
runs three times: warm-up, timed, and once more for the printed result).
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from probaforms_amd.metrics import twosample  # noqa: E402

N_PERM = 999


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


def host_weights(nr, nf, n_perm):
    """[1 + n_perm, nr + nf] float64: +nf on the rows labelled real, -nr on the others; the observed labelling first"""
    S = np.full((1 + n_perm, nr + nf), -float(nr))
    S[0, :nr] = nf
    for p in range(n_perm):
        S[1 + p, np.random.permutation(nr + nf)[:nr]] = nf
    return S


def torch_test(Zd, nr, nf, n_perm, gauss):
    """(statistic, p-value, a note where the yardstick went wrong) with torch operations on the device"""
    S = torch.from_numpy(host_weights(nr, nf, n_perm)).cuda()
    D = torch.cdist(Zd, Zd, compute_mode="donot_use_mm_for_euclid_dist")
    note = ""
    if gauss:
        med = float(D.flatten().median())
        if not med > 0:                               # (seen at 20 000 pooled rows: this cdist is then wrong as well)
            med, note = float(Zd.shape[1]) ** 0.5, "its median was %r, sqrt(d) taken instead" % med
        D = torch.exp(-(1.0 / (2 * med ** 2)) * D * D)
    V = ((S @ D) * S).sum(1) / float(nr * nf) ** 2
    V = (V if gauss else -V).cpu().numpy()
    return V[0], (1 + int((V[1:] >= V[0]).sum())) / (1 + n_perm), note


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=None)
    ap.add_argument("--reps", type=int, default=5, help="timed calls of each test (and as many warm-up calls)")
    ap.add_argument("--yard-reps", type=int, default=2, help="timed calls of the yardstick")
    ap.add_argument("--shape", default=None, help="one shape only: rows per sample x features, e.g. 10000x16")
    ap.add_argument("--only-tests", action="store_true", help="skip the yardstick and the permutation-draw timing")
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
        for name, fn, gauss in (("energy_test", twosample.energy_test, False), ("mmd_test", twosample.mmd_test, True)):
            def ours():
                np.random.seed(0)
                return fn(X, Y, n_permutations=N_PERM)

            med, lo, hi = timed(ours, a.reps)
            t = ours()
            print("  %-44s %10.2f  [%9.2f .. %9.2f]   statistic %.6g  p %.3f" % ("(a) " + name, med, lo, hi, t.statistic, t.pvalue),
                  file=out)
            out.flush()
            if a.only_tests:
                continue

            def yardstick():
                np.random.seed(0)
                return torch_test(Zd, n, n, N_PERM, gauss)

            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            tmed, tlo, thi = timed(yardstick, a.yard_reps)
            peak = torch.cuda.max_memory_allocated() - base
            stat, p, note = yardstick()
            print("  %-44s %10.2f  [%9.2f .. %9.2f]   peak allocator bytes %.1f MB" % ("(ii) torch cdist, (S @ D) * S, host labellings",
                                                                                   tmed, tlo, thi, peak / 1e6), file=out)
            print("  %-44s %10.2f x   |statistic (a) - (ii)| %.3g, p (ii) %.3f%s"
                  % ("(ii) / (a)", tmed / med, abs(stat - t.statistic), p, note and "; " + note), file=out)
            if not gauss:
                dmed, dlo, dhi = timed(lambda: host_weights(n, n, N_PERM), a.yard_reps)
                print("  %-44s %10.2f  [%9.2f .. %9.2f]   %.0f%% of (ii)" % ("(c) the host's labellings of (ii) alone", dmed, dlo, dhi,
                                                                          100 * dmed / tmed), file=out)
            out.flush()
    if out is not sys.stdout:
        out.close()


if __name__ == "__main__":
    main()
