#!/usr/bin/env python3
"""Warm timings of probaforms_amd.metrics.losses.sliced_wasserstein_loss at n = 1 000 and 10 000 rows per sample (nr = nf) and
d = 2 and 16 features, P = 64 given directions on the device, p = 2, in one process (profiles/r24_sliced_loss_time.txt).  Per
shape, float64 tensors on the device, the fake sample requiring a gradient:
  (a) sliced_wasserstein_loss(X, Y, directions=theta) forward + backward: the library's LDS sort;
  (v) the same with no input requiring a gradient: the value alone;
  (s) (a) and (v) with losses._MAX_LDS_ROWS = 0: torch.sort orders the samples and the kernels take the order as given; (s) over
      (a) is what the LDS sort buys;
  (e) energy_loss(X, Y) forward + backward and its value alone, the cheapest of the pair-walking losses;
  (ii) a float64 torch-autograd yardstick on the same device, forward + backward: Z @ theta^T, torch.sort per sample, the mean of
      |us - vs|^p (nr = nf: the sorted samples meet one to one).  Its VALUE is compared with (a): "right to 1e-9" or "WRONG".
Each is warmed (one call, and as many as are timed if a call takes under a second); the figure is the median wall time per call
with a device synchronisation at both ends, with the fastest and slowest call, and torch's peak allocator bytes above what was
allocated before the call.

    python scripts/sliced_loss_time.py [out.txt] [--reps N] [--shape NxD] [--projections P] [--only-ours]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from losses_time import line, timed  # noqa: E402
from probaforms_amd.metrics import losses  # noqa: E402


def yardstick(X, Y, theta, p):
    us = torch.sort(X @ theta.t(), dim=0)[0]
    vs = torch.sort(Y @ theta.t(), dim=0)[0]
    diff = us - vs
    return (diff.abs() if p == 1 else diff * diff).mean()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=None)
    ap.add_argument("--reps", type=int, default=7, help="timed calls of each")
    ap.add_argument("--shape", default=None, help="one shape only: rows per sample x features, e.g. 10000x16")
    ap.add_argument("--projections", type=int, default=64)
    ap.add_argument("--only-ours", action="store_true", help="(a) and (v) alone: what a kernel trace should see")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    out = open(a.out, "w") if a.out else sys.stdout
    P, p = a.projections, 2
    print("median [min .. max] ms per call, forward + backward unless it says otherwise; float64; P = %d, p = %d; %s"
          % (P, p, torch.cuda.get_device_name(0)), file=out)
    shapes = [(n, d) for n in (1000, 10000) for d in (2, 16)]
    if a.shape is not None:
        shapes = [tuple(int(v) for v in a.shape.split("x"))]
    for n, d in shapes:
        rng = np.random.default_rng(n + d)
        X = torch.from_numpy(rng.normal(size=(n, d))).cuda()
        Y = torch.from_numpy(rng.normal(0.3, 1.2, size=(n, d))).cuda().requires_grad_(True)
        Yv = Y.detach()
        th = rng.normal(size=(P, d))
        theta = torch.from_numpy(th / np.sqrt((th * th).sum(axis=1))[:, None]).cuda()
        print("\nn = %d rows per sample, d = %d" % (n, d), file=out)

        def fb(fn):
            def run():
                Y.grad = None
                fn().backward()
            return run

        def ours():
            return losses.sliced_wasserstein_loss(X, Y, p=p, directions=theta)

        def ours_value():
            return losses.sliced_wasserstein_loss(X, Yv, p=p, directions=theta)

        res = timed(fb(ours), a.reps)
        value = float(ours().detach())
        line(out, "(a) sliced_wasserstein_loss", res, "   value %.12g" % value)
        line(out, "(v) sliced_wasserstein_loss, value only", timed(ours_value, a.reps))
        if a.only_ours:
            continue
        cap = losses._MAX_LDS_ROWS
        losses._MAX_LDS_ROWS = 0
        try:
            given = timed(fb(ours), a.reps)
            same = float(ours().detach()) == value
            line(out, "(s) the same, torch.sort's order given", given, "   %s" % ("the same value bits" if same else "OTHER BITS"))
            print("  %-58s %10.2f x" % ("    over (a)", given[0] / res[0]), file=out)
            line(out, "(s) value only, torch.sort's order given", timed(ours_value, a.reps))
        finally:
            losses._MAX_LDS_ROWS = cap
        e = timed(fb(lambda: losses.energy_loss(X, Y)), a.reps)
        line(out, "(e) energy_loss", e)
        print("  %-58s %10.2f x" % ("    over (a)", e[0] / res[0]), file=out)
        line(out, "(e) energy_loss, value only", timed(lambda: losses.energy_loss(X, Yv), a.reps))
        try:
            y = timed(fb(lambda: yardstick(X, Y, theta, p)), a.reps)
            v = float(yardstick(X, Y, theta, p).detach())
            off = abs(v - value)
            line(out, "(ii) torch matmul + sort", y, "   value %.12g, off by %.3g (%s)" % (v, off, "right to 1e-9" if off <= 1e-9 else "WRONG"))
            print("  %-58s %10.2f x" % ("    over (a)", y[0] / timed(fb(ours), 3)[0]), file=out)
        except torch.cuda.OutOfMemoryError as e:
            print("  %-58s could not allocate: %s" % ("(ii) torch matmul + sort", str(e).split(".")[0]), file=out)
        Y.grad = None
        torch.cuda.empty_cache()
        out.flush()
    if out is not sys.stdout:
        out.close()


if __name__ == "__main__":
    main()
