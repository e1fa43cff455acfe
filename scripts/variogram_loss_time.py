#!/usr/bin/env python3
"""Warm timings of probaforms_amd.metrics.losses.variogram_score_loss in one process (profiles/r30_variogram_loss_time.txt).
Shapes: n = 65 536 rows, d = 16 features, K = 2, 8, 32 draws per row (training); n = 4 096, d = 16, K = 256 (evaluation);
n = 1 000, d = 5, K = 1 000 (many draws of few features).  Per shape, float64 tensors on the device, order 0.5, unit weights,
tie-free data, the draws requiring a gradient:
  (a) variogram_score_loss, forward + backward;
  (v) the same with no input requiring a gradient: the values alone;
  (k) pfm_variogram_grad alone, scores and grad_x: the kernel, without the autograd node's multiply by the incoming vector.  The
      line adds the bytes the call must move, 2 K n d 8 (the draws in, their gradients out), and the rate that time implies;
  (e) energy_score_loss forward + backward on the same tensors, in the same process;
  (t) a float64 torch-autograd loss on the same device, forward + backward, that forms |x_ki - x_kj|^0.5 as a [K, n, d, d] tensor
      (the square root guarded at 0, which keeps the diagonal's gradient finite), with its allocator peak.
The VALUE of (t) is compared with (a): "right to 1e-9" or "WRONG".  Each is warmed (one call, and as many as are timed if a call
takes under a second); the figure is the median wall time per call with a device synchronisation at both ends, with the fastest and
slowest call, and torch's peak allocator bytes above what was allocated before the call.  A yardstick that cannot allocate says so.

    python scripts/variogram_loss_time.py [out.txt] [--reps N] [--shape NxDxK] [--only-ours]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from losses_time import line, timed  # noqa: E402
from probaforms_amd.metrics import _lib, losses  # noqa: E402

SHAPES = [(65536, 16, 2), (65536, 16, 8), (65536, 16, 32), (4096, 16, 256), (1000, 5, 1000)]


def root(t):
    a = t.abs()
    pos = a > 0
    return torch.where(pos, torch.where(pos, a, torch.ones_like(a)).sqrt(), torch.zeros_like(a))


def yard(X, Y):
    """the variogram score of order 0.5, mean over the rows, from the broadcast differences [K, n, d, d]"""
    m = root(X[:, :, :, None] - X[:, :, None, :]).mean(dim=0)
    v = root(Y[:, :, None] - Y[:, None, :])
    return ((v - m) ** 2).sum(dim=(1, 2)).mean()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=None)
    ap.add_argument("--reps", type=int, default=7, help="timed calls of each")
    ap.add_argument("--shape", default=None, help="one shape only: rows x features x draws, e.g. 65536x16x8")
    ap.add_argument("--only-ours", action="store_true", help="(a), (v) and (k) alone: what a kernel trace should see")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    out = open(a.out, "w") if a.out else sys.stdout
    print("median [min .. max] ms per call, forward + backward unless it says otherwise; float64; order 0.5, unit weights; %s"
          % torch.cuda.get_device_name(0), file=out)
    shapes = SHAPES if a.shape is None else [tuple(int(v) for v in a.shape.split("x"))]
    for n, d, K in shapes:
        rng = np.random.default_rng(n + d + K)
        X = torch.from_numpy(rng.normal(size=(K, n, d))).cuda().requires_grad_(True)
        Y = torch.from_numpy(rng.normal(0.3, 1.2, size=(n, d))).cuda()
        Xv = X.detach()
        print("\nn = %d rows, d = %d, K = %d draws per row; plan: %d rows per workgroup, %d lanes per row, %d LDS bytes, "
              "%d workgroups, %d rows in flight, %d slices" % ((n, d, K) + _lib.variogram_plan(n, K, d)), file=out)

        def fb(f):
            def run():
                X.grad = None
                f().backward()
            return run

        ours = timed(fb(lambda: losses.variogram_score_loss(X, Y)), a.reps)
        value = float(losses.variogram_score_loss(X, Y).detach())
        line(out, "(a) variogram_score_loss", ours, "   value %.12g" % value)
        line(out, "(v) the same, values only", timed(lambda: losses.variogram_score_loss(Xv, Y), a.reps))
        scores, gx = torch.empty(n, dtype=torch.float64, device="cuda"), torch.empty_like(Xv)
        ws = torch.empty(_lib.variogram_grad_workspace_bytes(n, K, d), dtype=torch.uint8, device="cuda")
        kres = timed(lambda: _lib.variogram_grad(Xv, Y, None, 0.5, scores, gx, None, ws), a.reps)
        must = 2.0 * K * n * d * 8
        line(out, "(k) pfm_variogram_grad alone, scores and grad_x", kres,
             "   %.1f MB to move: %.0f GB/s" % (must / 1e6, must / (kres[0] * 1e-3) / 1e9))
        del scores, gx
        if a.only_ours:
            continue
        eres = timed(fb(lambda: losses.energy_score_loss(X, Y)), a.reps)
        line(out, "(e) energy_score_loss", eres)
        print("  %-58s %10.2f x" % ("    (a) over (e)", ours[0] / eres[0]), file=out)
        try:
            res = timed(fb(lambda: yard(X, Y)), a.reps)
            v = float(yard(X, Y).detach())
            off = abs(v - value)
            line(out, "(t) torch autograd over [K, n, d, d]", res,
                 "   value %.12g, off by %.3g (%s)" % (v, off, "right to 1e-9" if off <= 1e-9 * max(1.0, abs(value)) else "WRONG"))
            print("  %-58s %10.2f x" % ("    over (a)", res[0] / ours[0]), file=out)
        except torch.cuda.OutOfMemoryError as e:
            print("  %-58s could not allocate: %s" % ("(t) torch autograd over [K, n, d, d]", str(e).split(".")[0]), file=out)
        X.grad = None
        torch.cuda.empty_cache()
        out.flush()
    if out is not sys.stdout:
        out.close()


if __name__ == "__main__":
    main()
