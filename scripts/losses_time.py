#!/usr/bin/env python3
"""Warm timings of probaforms_amd.metrics.losses at n = 1 000 and 10 000 rows per sample and d = 2 and 16 features, in one
process (profiles/r22_losses_time.txt).  Per shape, float64 tensors on the device, the fake sample requiring a gradient:
  (a) energy_loss(X, Y) forward + backward;
  (b) mmd_loss(X, Y, bandwidth) forward + backward, one bandwidth (the pooled median, taken once outside the timing);
  (v) energy_loss / mmd_loss with no input requiring a gradient: the value sweep alone;
  (i) energy_distance_full_sample(X, Y, squared=True) on the same tensors: the price of the existing forward sweep, its
      read-back to numpy included;
  (ii) a float64 torch-autograd yardstick on the same device, forward + backward, for the energy distance and for the MMD:
      torch.cdist of the pooled rows (the differentiable [N, N] matrix autograd keeps for the backward), and the broadcast
      difference (z_a - z_b, squared and summed, an [N, N, d] temporary), which forms d^2 as the library does.  The VALUE of
      each is compared with (a) / (b): "right to 1e-9" or "WRONG", with the difference.
Each is warmed (one call, and as many as are timed if a call takes under a second); the figure is the median wall time per call
with a device synchronisation at both ends, with the fastest and slowest call, and torch's peak allocator bytes above what was
allocated before the call.  Where a yardstick cannot allocate, the line says so.

    python scripts/losses_time.py [out.txt] [--reps N] [--shape NxD]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from probaforms_amd.metrics import energy as energy_mod, losses  # noqa: E402
from probaforms_amd.metrics.twosample import _median  # noqa: E402


def timed(fn, reps):
    """-> (median, min, max) ms of a call, peak allocator bytes of a call"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    if time.perf_counter() - t0 < 1.0:
        for _ in range(reps - 1):
            fn()
    torch.cuda.synchronize()
    ts = []
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts), torch.cuda.max_memory_allocated() - base


def weights(nr, N, device):
    """+1 / nr on the real rows, -1 / nf on the fake ones, built in float64"""
    w = torch.empty(N, dtype=torch.float64, device=device)
    w[:nr], w[nr:] = 1.0 / nr, -1.0 / (N - nr)
    return w


def pair_loss(D2, nr, kind, gamma):
    """the statistic from a differentiable [N, N] matrix of squared distances"""
    N = D2.shape[0]
    w = weights(nr, N, D2.device)
    if kind == "energy":
        pos = D2 > 0
        g = -torch.where(pos, torch.where(pos, D2, torch.ones_like(D2)).sqrt(), torch.zeros_like(D2))
    else:
        g = torch.exp(-gamma * D2)
    return w @ g @ w


def yard_cdist(X, Y, kind, gamma):
    Z = torch.cat([X, Y])
    D = torch.cdist(Z, Z)                           # the default: the matrix-multiply identity above 25 rows
    if kind == "energy":
        N, nr = Z.shape[0], X.shape[0]
        w = weights(nr, N, D.device)
        return -(w @ D @ w)
    return pair_loss(D * D, X.shape[0], kind, gamma)


def yard_broadcast(X, Y, kind, gamma):
    Z = torch.cat([X, Y])
    diff = Z[:, None, :] - Z[None, :, :]
    return pair_loss((diff * diff).sum(dim=2), X.shape[0], kind, gamma)


def line(out, name, res, extra=""):
    med, lo, hi, peak = res
    print("  %-58s %10.2f  [%9.2f .. %9.2f]   peak %8.1f MB%s" % (name, med, lo, hi, peak / 1e6, extra), file=out)
    out.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=None)
    ap.add_argument("--reps", type=int, default=7, help="timed calls of each")
    ap.add_argument("--shape", default=None, help="one shape only: rows per sample x features, e.g. 10000x16")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    out = open(a.out, "w") if a.out else sys.stdout
    print("median [min .. max] ms per call, forward + backward unless it says otherwise; float64; %s"
          % torch.cuda.get_device_name(0), file=out)
    shapes = [(n, d) for n in (1000, 10000) for d in (2, 16)]
    if a.shape is not None:
        shapes = [tuple(int(v) for v in a.shape.split("x"))]
    for n, d in shapes:
        rng = np.random.default_rng(n + d)
        X = torch.from_numpy(rng.normal(size=(n, d))).cuda()
        Y = torch.from_numpy(rng.normal(0.3, 1.2, size=(n, d))).cuda().requires_grad_(True)
        Yv = Y.detach()
        sigma = _median(X, Yv)
        gamma = 1.0 / (2.0 * sigma * sigma)
        print("\nn = %d rows per sample, d = %d, bandwidth %.4g" % (n, d, sigma), file=out)

        def fb(fn):
            def run():
                Y.grad = None
                fn().backward()
            return run

        ours = {"energy": lambda: losses.energy_loss(X, Y), "mmd": lambda: losses.mmd_loss(X, Y, bandwidth=sigma)}
        value = {}
        for kind, tag in (("energy", "(a) energy_loss"), ("mmd", "(b) mmd_loss, one bandwidth")):
            res = timed(fb(ours[kind]), a.reps)
            value[kind] = float(ours[kind]().detach())
            line(out, tag, res, "   value %.12g" % value[kind])
        line(out, "(v) energy_loss, value only", timed(lambda: losses.energy_loss(X, Yv), a.reps))
        line(out, "(v) mmd_loss, value only", timed(lambda: losses.mmd_loss(X, Yv, bandwidth=sigma), a.reps))
        res = timed(lambda: energy_mod.energy_distance_full_sample(X, Yv, squared=True), a.reps)
        line(out, "(i) energy_distance_full_sample(squared=True), forward only", res,
             "   value %.12g" % energy_mod.energy_distance_full_sample(X, Yv, squared=True))

        for kind in ("energy", "mmd"):
            for name, yard in (("cdist", yard_cdist), ("broadcast difference", yard_broadcast)):
                tag = "(ii) torch %s, %s" % (name, kind)
                try:
                    res = timed(fb(lambda: yard(X, Y, kind, gamma)), a.reps)
                    v = float(yard(X, Y, kind, gamma).detach())
                    off = abs(v - value[kind])
                    verdict = "right to 1e-9" if off <= 1e-9 else "WRONG"
                    line(out, tag, res, "   value %.12g, off by %.3g (%s)" % (v, off, verdict))
                    print("  %-58s %10.2f x" % ("    over ours", res[0] / timed(fb(ours[kind]), 3)[0]), file=out)
                except torch.cuda.OutOfMemoryError as e:
                    print("  %-58s could not allocate: %s" % (tag, str(e).split(".")[0]), file=out)
                Y.grad = None
                torch.cuda.empty_cache()
                out.flush()
    if out is not sys.stdout:
        out.close()


if __name__ == "__main__":
    main()
