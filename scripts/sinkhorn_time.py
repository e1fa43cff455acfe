#!/usr/bin/env python3
"""Warm timings of probaforms_amd.metrics.sinkhorn.sinkhorn_divergence with its defaults (n_iters = 100, p = 2, reg = 0.1,
n_sinkhorn = 100) at n = 1 000 and 10 000 rows per sample and d = 2 and 16 features, in one process
(profiles/r20_sinkhorn_time.txt):
  (a) sinkhorn_divergence(X, Y): numpy in, (mean, std) out; the median-distance call that sets eps is part of it;
  (k) pfm_sinkhorn alone on the same draws, timed with device events, and that time per pooled pair, replicate and step
      ((2 n)^2 pairs, 100 replicates, 101 steps): the cost of one float64 exp with its share of everything else;
  (i) energy_distance(X, Y) on the same inputs: the project's metric that walks the same pairs once per call;
  (ii) a float64 torch yardstick on the device, for time and memory only: torch.cdist of the pooled rows once, then per
      replicate the same 101 steps as four torch.logsumexp over blocks of that matrix with the replicate's log-weights (-inf for
      a row that is not drawn).  It holds the (2 n)^2 float64 matrix and a temporary of a block's size; it is run for
      --yard-replicates replicates and scaled to 100.  torch's peak allocator bytes are reported beside it.  Where it cannot
      allocate, the line says so.
Each of (a), (i) is warmed (one call, and as many as are timed if a call takes under a second); the figure is the median wall
time per call with a device synchronisation at both ends, with the fastest and slowest call.  The largest difference between the
replicates of (a) and (ii) is printed: (ii) is a yardstick for time, tests/test_sinkhorn_gpu.py holds (a) against a float64
scipy restatement.

    python scripts/sinkhorn_time.py [out.txt] [--reps N] [--yard-replicates N] [--shape NxD] [--only-sinkhorn]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from probaforms_amd.metrics import _boot, _lib, energy as energy_mod, sinkhorn as sk  # noqa: E402
from probaforms_amd.metrics.twosample import _median  # noqa: E402

N_ITERS, N_SINKHORN, P, REG = 100, 100, 2, 0.1


def timed(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    if time.perf_counter() - t0 < 1.0:
        for _ in range(reps - 1):
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


def draws(nr, nf, reps):
    host = np.empty(reps * (nr + nf), np.int32)
    _boot.draw_indices(host, reps, nr, nf)
    idx = torch.from_numpy(host).cuda()
    return idx[:reps * nr], idx[reps * nr:]


def kernel_ms(Xd, Yd, eps, reps_timed):
    """pfm_sinkhorn alone, N_ITERS replicates: median milliseconds between two device events"""
    (nr, d), nf = Xd.shape, Yd.shape[0]
    np.random.seed(0)
    ir, jf = draws(nr, nf, N_ITERS)
    ws = torch.empty(_lib.sinkhorn_workspace_bytes(nr, nf, d, N_ITERS), dtype=torch.uint8, device=Xd.device)
    out = torch.empty((2, N_ITERS), dtype=torch.float64, device=Xd.device)
    ts = []
    for k in range(reps_timed + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        _lib.sinkhorn(Xd, Yd, ir, jf, N_ITERS, P, eps, N_SINKHORN, out[0], out[1], None, ws)
        b.record()
        torch.cuda.synchronize()
        if k:
            ts.append(a.elapsed_time(b))
    return statistics.median(ts), ws.numel()


def torch_replicates(Xd, Yd, eps, reps):
    """value of `reps` replicates with torch operations on the device, on the reference's draws"""
    nr, nf = Xd.shape[0], Yd.shape[0]
    C = torch.cdist(torch.cat([Xd, Yd]), torch.cat([Xd, Yd]), compute_mode="donot_use_mm_for_euclid_dist") ** P
    blocks = {"f": C[:nr, nr:], "g": C[nr:, :nr], "u": C[:nr, :nr], "v": C[nr:, nr:]}
    col = {"f": "g", "g": "f", "u": "u", "v": "v"}
    ir, jf = draws(nr, nf, reps)
    out = np.empty(reps)
    for r in range(reps):
        a = torch.bincount(ir[r * nr:(r + 1) * nr].long(), minlength=nr).double() / nr
        b = torch.bincount(jf[r * nf:(r + 1) * nf].long(), minlength=nf).double() / nf
        lw = {"f": a.log(), "u": a.log(), "g": b.log(), "v": b.log()}           # of the potential's own rows (log 0 = -inf)
        h = {k: torch.zeros_like(lw[k]) for k in lw}

        def softmins():
            return {k: -eps * torch.logsumexp((h[col[k]] / eps + lw[col[k]])[None, :] - blocks[k] / eps, dim=1) for k in h}

        for _ in range(N_SINKHORN):
            s = softmins()
            h = {k: 0.5 * (h[k] + s[k]) for k in h}
        h = softmins()
        out[r] = float((a * (h["f"] - h["u"])).sum() + (b * (h["g"] - h["v"])).sum())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=None)
    ap.add_argument("--reps", type=int, default=5, help="timed calls of sinkhorn_divergence and of energy_distance")
    ap.add_argument("--yard-replicates", type=int, default=2, help="replicates the torch yardstick runs (scaled to n_iters)")
    ap.add_argument("--shape", default=None, help="one shape only: rows per sample x features, e.g. 10000x16")
    ap.add_argument("--only-sinkhorn", action="store_true", help="skip energy_distance and the yardstick")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    out = open(a.out, "w") if a.out else sys.stdout
    print("median [min .. max] ms per call; n_iters = %d, p = %d, reg = %g, n_sinkhorn = %d; %s"
          % (N_ITERS, P, REG, N_SINKHORN, torch.cuda.get_device_name(0)), file=out)
    shapes = [(n, d) for n in (1000, 10000) for d in (2, 16)]
    if a.shape is not None:
        shapes = [tuple(int(v) for v in a.shape.split("x"))]
    for n, d in shapes:
        rng = np.random.default_rng(n + d)
        X, Y = rng.normal(size=(n, d)), rng.normal(0.3, 1.2, size=(n, d))
        Xd, Yd = torch.from_numpy(X).cuda(), torch.from_numpy(Y).cuda()
        eps = float(sk.epsilon_of(_median(Xd, Yd), P, REG))
        print("\nn = %d rows per sample, d = %d, eps = %.4g" % (n, d, eps), file=out)

        def ours():
            np.random.seed(0)
            return sk.sinkhorn_divergence(X, Y)

        med, lo, hi = timed(ours, a.reps)
        print("  %-46s %10.2f  [%9.2f .. %9.2f]" % ("(a) sinkhorn_divergence", med, lo, hi), file=out)
        np.random.seed(0)
        V = sk.REPLICATES["sinkhorn_divergence"](X, Y)
        print("  %-46s value %.6g +- %.3g, largest drift %.3g" % ("    replicates", V[:, 0].mean(), V[:, 0].std(), V[:, 1].max()),
              file=out)
        kms, wsb = kernel_ms(Xd, Yd, eps, 2 if med > 1000 else a.reps)
        print("  %-46s %10.2f   %.2f ps per pair, replicate and step; workspace %.1f MB"
              % ("(k) pfm_sinkhorn alone (device events)", kms, kms * 1e9 / ((2.0 * n) ** 2 * N_ITERS * (N_SINKHORN + 1)), wsb / 1e6),
              file=out)
        out.flush()
        if a.only_sinkhorn:
            continue

        def energy():
            np.random.seed(0)
            return energy_mod.energy_distance(X, Y, n_iters=N_ITERS)

        emed, elo, ehi = timed(energy, a.reps)
        print("  %-46s %10.2f  [%9.2f .. %9.2f]" % ("(i) energy_distance", emed, elo, ehi), file=out)
        print("  %-46s %10.2f x" % ("(a) / (i)", med / emed), file=out)
        out.flush()

        R = a.yard_replicates
        try:
            np.random.seed(0)
            torch_replicates(Xd, Yd, eps, 1)                              # warm-up
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            torch.cuda.synchronize()
            np.random.seed(0)
            t0 = time.perf_counter()
            W = torch_replicates(Xd, Yd, eps, R)
            torch.cuda.synchronize()
            tms = (time.perf_counter() - t0) * 1e3
            peak = torch.cuda.max_memory_allocated() - base
            print("  %-46s %10.2f   (%d replicates took %.2f ms, cdist included)   peak allocator bytes %.1f MB"
                  % ("(ii) torch cdist + logsumexp, scaled to 100", tms * N_ITERS / R, R, tms, peak / 1e6), file=out)
            print("  %-46s %10.2f x" % ("(ii) / (a)", tms * N_ITERS / R / med), file=out)
            print("  %-46s %.3g (value about %.3g)" % ("largest |value (a) - value (ii)|", np.abs(V[:R, 0] - W).max(),
                                                      V[:R, 0].mean()), file=out)
        except torch.cuda.OutOfMemoryError as e:
            print("  %-46s could not allocate: %s" % ("(ii) torch cdist + logsumexp", str(e).split(".")[0]), file=out)
        out.flush()
    if out is not sys.stdout:
        out.close()


if __name__ == "__main__":
    main()
