#!/usr/bin/env python3
"""Warm timings of probaforms_amd.metrics.energy.energy_distance, n_iters = 100, at n = 1 000 and 10 000 rows per sample and
d = 2 and 16 features, in one process (profiles/r17_energy_time.txt):
  (a) energy_distance(X, Y): numpy in, (mean, std) out;
  (i) maximum_mean_discrepancy(X, Y) on the same inputs: the project's own metric that walks the same (nx + ny)^2 pairs, once
      per replicate, because each replicate has its own median and kernel;
  (ii) the same replicates in torch on the device, a yardstick for time only: per replicate the resampled rows and three
      float64 torch.cdist(...).mean(); the index draws are the same host draws, uploaded once per call.  torch's peak
      allocator bytes are reported beside it;
  (c) the host's index draw of one call alone (numpy randint, what _boot.run_groups does before the kernels can start), as a
      share of (a).
Each variant is warmed for as many calls as are timed; the figure is the median wall time per call with a device synchronisation
at both ends, with the fastest and slowest call.  The largest difference of D^2 between (a) and (ii) is printed: (ii) is a
yardstick for time, tests/test_energy_gpu.py holds (a) against a float64 scipy restatement.

    python scripts/energy_time.py [out.txt] [--reps N] [--yard-reps N] [--shape NxD] [--only-energy]

Under `rocprofv3 --kernel-trace --stats -- python scripts/energy_time.py --only-energy --reps 1 --shape 10000x16` the kernels'
own times at one shape: k_counts, k_energy_tiles and k_quad_finish<3> (the call then runs twice: warm-up and one).
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from probaforms_amd.metrics import _boot, maximum_mean_discrepancy, energy as energy_mod  # noqa: E402

N_ITERS = 100


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


def torch_means(Xd, Yd, n_iters):
    """the replicates' exx, eyy, exy [n_iters, 3] with torch operations on the device, on the reference's draws"""
    nr, nf = Xd.shape[0], Yd.shape[0]
    host = np.empty(n_iters * (nr + nf), np.int32)
    _boot.draw_indices(host, n_iters, nr, nf)
    idx = torch.from_numpy(host).cuda().long()
    ix, iy = idx[:n_iters * nr].view(n_iters, nr), idx[n_iters * nr:].view(n_iters, nf)
    out = torch.empty((n_iters, 3), dtype=torch.float64, device=Xd.device)
    for r in range(n_iters):
        R, F = Xd[ix[r]], Yd[iy[r]]
        # (the matrix-multiplication form of cdist loses the exact zeros of duplicated rows)
        out[r, 0] = torch.cdist(R, R, compute_mode="donot_use_mm_for_euclid_dist").mean()
        out[r, 1] = torch.cdist(F, F, compute_mode="donot_use_mm_for_euclid_dist").mean()
        out[r, 2] = torch.cdist(R, F, compute_mode="donot_use_mm_for_euclid_dist").mean()
    return out.cpu().numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=None)
    ap.add_argument("--reps", type=int, default=5, help="timed calls of energy_distance (and as many warm-up calls)")
    ap.add_argument("--yard-reps", type=int, default=2, help="timed calls of each yardstick")
    ap.add_argument("--shape", default=None, help="one shape only: rows per sample x features, e.g. 10000x16")
    ap.add_argument("--only-energy", action="store_true", help="skip the yardsticks and the index-draw timing")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    out = open(a.out, "w") if a.out else sys.stdout
    print("median [min .. max] ms per call; warm-up = as many calls as timed; n_iters = %d; %s"
          % (N_ITERS, torch.cuda.get_device_name(0)), file=out)
    shapes = [(n, d) for n in (1000, 10000) for d in (2, 16)]
    if a.shape is not None:
        shapes = [tuple(int(v) for v in a.shape.split("x"))]
    for n, d in shapes:
        rng = np.random.default_rng(n + d)
        X, Y = rng.normal(size=(n, d)), rng.normal(0.3, 1.2, size=(n, d))
        Xd, Yd = torch.from_numpy(X).cuda(), torch.from_numpy(Y).cuda()
        print("\nn = %d rows per sample, d = %d" % (n, d), file=out)

        def ours():
            np.random.seed(0)
            return energy_mod.energy_distance(X, Y, n_iters=N_ITERS)

        med, lo, hi = timed(ours, a.reps)
        print("  %-44s %10.2f  [%9.2f .. %9.2f]" % ("(a) energy_distance", med, lo, hi), file=out)
        out.flush()
        if a.only_energy:
            continue

        def mmd():
            np.random.seed(0)
            return maximum_mean_discrepancy(X, Y, n_iters=N_ITERS)

        mmed, mlo, mhi = timed(mmd, a.yard_reps)
        print("  %-44s %10.2f  [%9.2f .. %9.2f]" % ("(i) maximum_mean_discrepancy", mmed, mlo, mhi), file=out)
        print("  %-44s %10.2f x" % ("(i) / (a)", mmed / med), file=out)
        out.flush()

        def yardstick():
            np.random.seed(0)
            return torch_means(Xd, Yd, N_ITERS)

        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        tmed, tlo, thi = timed(yardstick, a.yard_reps)
        peak = torch.cuda.max_memory_allocated() - base
        print("  %-44s %10.2f  [%9.2f .. %9.2f]   peak allocator bytes %.1f MB" % ("(ii) torch cdist(...).mean() on the device",
                                                                               tmed, tlo, thi, peak / 1e6), file=out)
        print("  %-44s %10.2f x" % ("(ii) / (a)", tmed / med), file=out)
        np.random.seed(0)
        E = energy_mod.REPLICATES["energy_distance"](X, Y, N_ITERS)
        diff = np.abs(energy_mod.values_of(E, True) - energy_mod.values_of(yardstick(), True)).max()
        print("  %-44s %.3g (exy about %.3g)" % ("largest |D^2 (a) - D^2 (ii)|", diff, E[:, 2].mean()), file=out)

        host = np.empty(N_ITERS * 2 * n, np.int32)
        dmed, dlo, dhi = timed(lambda: _boot.draw_indices(host, N_ITERS, n, n), a.reps)
        print("  %-44s %10.2f  [%9.2f .. %9.2f]   %.0f%% of (a)" % ("(c) the host's index draw alone", dmed, dlo, dhi,
                                                                  100 * dmed / med), file=out)
        out.flush()
    if out is not sys.stdout:
        out.close()


if __name__ == "__main__":
    main()
