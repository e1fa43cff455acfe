#!/usr/bin/env python3
"""Warm timings of probaforms_amd.metrics.prdc, n_iters = 100, nearest_k = 5, at n = 1 000 and 10 000 rows per sample and d = 2 and
16 features, in one process (profiles/r16_prdc_time.txt):
  (a) prdc(X, Y): numpy in, PRDC of (mean, std) pairs out;
  (b) the same replicates in torch on the device, the yardstick: per replicate the resampled rows, float64 torch.cdist squared,
      kthvalue for the radii and the four comparisons' counts; the index draws are the same host draws, uploaded once per call.
      torch's peak allocator bytes are reported beside it;
  (c) the host's index draw of one call alone (numpy randint, what _boot.run_groups does before the kernels can start), as a
      share of (a).
Each variant is warmed for as many calls as are timed; the figure is the median wall time per call with a device synchronisation
at both ends, with the fastest and slowest call.  The number of counts in which (a) and (b) differ is printed: (b) is a
yardstick for time, tests/test_prdc_gpu.py holds (a) against a float64 numpy restatement.

    python scripts/prdc_time.py [out.txt] [--reps N] [--torch-reps N] [--shape NxD] [--only-prdc]

Under `rocprofv3 --kernel-trace --stats -- python scripts/prdc_time.py --only-prdc --reps 1 --shape 10000x16` the kernels' own
times at one shape: k_knn_radius<6>, k_prdc_sweep and k_prdc_final (the call then runs twice: warm-up and one).
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from probaforms_amd.metrics import _boot, prdc as prdc_mod  # noqa: E402

N_ITERS, K = 100, 5


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


def torch_counts(Xd, Yd, n_iters, k):
    """the replicates' counts [n_iters, 4] with torch operations on the device, on the reference's draws"""
    nr, nf = Xd.shape[0], Yd.shape[0]
    host = np.empty(n_iters * (nr + nf), np.int32)
    _boot.draw_indices(host, n_iters, nr, nf)
    idx = torch.from_numpy(host).cuda().long()
    ix, iy = idx[:n_iters * nr].view(n_iters, nr), idx[n_iters * nr:].view(n_iters, nf)
    out = torch.empty((n_iters, 4), dtype=torch.int64, device=Xd.device)
    for r in range(n_iters):
        R, F = Xd[ix[r]], Yd[iy[r]]
        # (the matrix-multiplication form of cdist loses the exact zeros of duplicated rows)
        rr = torch.cdist(R, R, compute_mode="donot_use_mm_for_euclid_dist").square_().kthvalue(k + 1, dim=1).values
        ss = torch.cdist(F, F, compute_mode="donot_use_mm_for_euclid_dist").square_().kthvalue(k + 1, dim=1).values
        D = torch.cdist(R, F, compute_mode="donot_use_mm_for_euclid_dist").square_()
        inside = D < rr[:, None]
        c = inside.sum(dim=0)
        out[r, 0] = (c > 0).sum()
        out[r, 1] = (D < ss[None, :]).any(dim=1).sum()
        out[r, 2] = c.sum()
        out[r, 3] = inside.any(dim=1).sum()
    return out.cpu().numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=None)
    ap.add_argument("--reps", type=int, default=5, help="timed calls of prdc (and as many warm-up calls)")
    ap.add_argument("--torch-reps", type=int, default=2, help="timed calls of the torch yardstick")
    ap.add_argument("--shape", default=None, help="one shape only: rows per sample x features, e.g. 10000x16")
    ap.add_argument("--only-prdc", action="store_true", help="skip the torch yardstick and the index-draw timing")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    out = open(a.out, "w") if a.out else sys.stdout
    print("median [min .. max] ms per call; warm-up = as many calls as timed; n_iters = %d, nearest_k = %d; %s"
          % (N_ITERS, K, torch.cuda.get_device_name(0)), file=out)
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
            return prdc_mod.prdc(X, Y, n_iters=N_ITERS, nearest_k=K)

        med, lo, hi = timed(ours, a.reps)
        print("  %-44s %10.2f  [%9.2f .. %9.2f]" % ("(a) prdc", med, lo, hi), file=out)
        out.flush()
        if a.only_prdc:
            continue

        def yardstick():
            np.random.seed(0)
            return torch_counts(Xd, Yd, N_ITERS, K)

        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        tmed, tlo, thi = timed(yardstick, a.torch_reps)
        peak = torch.cuda.max_memory_allocated() - base
        print("  %-44s %10.2f  [%9.2f .. %9.2f]   peak allocator bytes %.1f MB" % ("(b) torch cdist + kthvalue on the device",
                                                                               tmed, tlo, thi, peak / 1e6), file=out)
        print("  %-44s %10.2f x" % ("(b) / (a)", tmed / med), file=out)
        np.random.seed(0)
        differ = int((prdc_mod.REPLICATES["prdc"](X, Y, N_ITERS, K) != yardstick()).sum())
        print("  %-44s %d of %d" % ("counts that differ between (a) and (b)", differ, 4 * N_ITERS), file=out)

        host = np.empty(N_ITERS * 2 * n, np.int32)
        dmed, dlo, dhi = timed(lambda: _boot.draw_indices(host, N_ITERS, n, n), a.reps)
        print("  %-44s %10.2f  [%9.2f .. %9.2f]   %.0f%% of (a)" % ("(c) the host's index draw alone", dmed, dlo, dhi,
                                                                  100 * dmed / med), file=out)
        out.flush()
    if out is not sys.stdout:
        out.close()


if __name__ == "__main__":
    main()
