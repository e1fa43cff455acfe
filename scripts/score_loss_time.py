#!/usr/bin/env python3
"""Warm timings of probaforms_amd.metrics.losses.energy_score_loss and crps_loss in one process
(profiles/r25_score_loss_time.txt).  Shapes: n = 65 536 rows, d = 16 features, K = 2, 8, 32 draws per row (training: a streaming
kernel); n = 4 096, d = 16, K = 256 (evaluation: the pair walk); n = 1 000, d = 1, K = 1 000 through crps_loss.  Per shape,
float64 tensors on the device, the draws requiring a gradient:
  (a) the loss, forward + backward;
  (v) the same with no input requiring a gradient: the values alone;
  (k) pfm_score_grad alone, scores and both gradients: the kernel, without the autograd node's multiply by the incoming vector.
      For K <= 32 the line adds the bytes the call must move, 2 K n d 8 (the draws in, their gradients out), over that time;
  (i) a float64 torch-autograd yardstick on the same device, forward + backward: torch.cdist of every row's draws, an [n, K, K]
      matrix autograd keeps; its diagonal is masked, which is what keeps the coincident pairs' gradient finite;
  (ii) the same from the broadcast difference x_k - x_l, an [n, K, K, d] temporary, with the square root guarded at 0: it forms the
      squared distance as the library does.
The VALUE of each yardstick is compared with (a): "right to 1e-9" or "WRONG".  Each is warmed (one call, and as many as are timed
if a call takes under a second); the figure is the median wall time per call with a device synchronisation at both ends, with the
fastest and slowest call, and torch's peak allocator bytes above what was allocated before the call.  A yardstick that cannot
allocate says so.

    python scripts/score_loss_time.py [out.txt] [--reps N] [--shape NxDxK] [--only-ours]
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

SHAPES = [(65536, 16, 2, "energy"), (65536, 16, 8, "energy"), (65536, 16, 32, "energy"), (4096, 16, 256, "energy"),
          (1000, 1, 1000, "crps")]


def t1_of(Xr, Y):
    return torch.linalg.vector_norm(Xr - Y[:, None, :], dim=2).mean(dim=1)


def yard_cdist(X, Y):
    """fair energy score, mean over the rows, from torch.cdist over [n, K, K]"""
    Xr = X.permute(1, 0, 2)
    K = Xr.shape[1]
    D = torch.cdist(Xr, Xr)
    D = D.masked_fill(torch.eye(K, dtype=torch.bool, device=X.device), 0.0)
    return (t1_of(Xr, Y) - D.sum(dim=(1, 2)) / (2.0 * K * (K - 1))).mean()


def yard_broadcast(X, Y):
    """the same from the broadcast difference [n, K, K, d]"""
    Xr = X.permute(1, 0, 2)
    K = Xr.shape[1]
    diff = Xr[:, :, None, :] - Xr[:, None, :, :]
    d2 = (diff * diff).sum(dim=3)
    pos = d2 > 0
    D = torch.where(pos, torch.where(pos, d2, torch.ones_like(d2)).sqrt(), torch.zeros_like(d2))
    return (t1_of(Xr, Y) - D.sum(dim=(1, 2)) / (2.0 * K * (K - 1))).mean()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=None)
    ap.add_argument("--reps", type=int, default=7, help="timed calls of each")
    ap.add_argument("--shape", default=None, help="one shape only: rows x features x draws, e.g. 65536x16x8")
    ap.add_argument("--only-ours", action="store_true", help="(a), (v) and (k) alone: what a kernel trace should see")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    out = open(a.out, "w") if a.out else sys.stdout
    print("median [min .. max] ms per call, forward + backward unless it says otherwise; float64; fair=True; %s"
          % torch.cuda.get_device_name(0), file=out)
    shapes = SHAPES
    if a.shape is not None:
        n, d, K = (int(v) for v in a.shape.split("x"))
        shapes = [(n, d, K, "energy")]
    for n, d, K, kind in shapes:
        rng = np.random.default_rng(n + d + K)
        X = torch.from_numpy(rng.normal(size=(K, n, d))).cuda().requires_grad_(True)
        Y = torch.from_numpy(rng.normal(0.3, 1.2, size=(n, d))).cuda()
        Xv = X.detach()
        fn = losses.energy_score_loss if kind == "energy" else losses.crps_loss
        plan = _lib.score_plan(n * d if kind == "crps" else n, K, 1 if kind == "crps" else d)
        print("\nn = %d rows, d = %d, K = %d draws per row, %s_loss; plan: %d rows per workgroup, %d lanes per row, %d LDS bytes, "
              "%d workgroups" % ((n, d, K, kind if kind == "crps" else "energy_score") + plan), file=out)

        def fb(f):
            def run():
                X.grad = None
                f().backward()
            return run

        res = timed(fb(lambda: fn(X, Y)), a.reps)
        value = float(fn(X, Y).detach())
        line(out, "(a) %s_loss" % ("crps" if kind == "crps" else "energy_score"), res, "   value %.12g" % value)
        line(out, "(v) the same, values only", timed(lambda: fn(Xv, Y), a.reps))
        Xk, Yk = (Xv.reshape(K, n * d, 1), Y.reshape(n * d, 1)) if kind == "crps" else (Xv, Y)
        scores = torch.empty(Xk.shape[1], dtype=torch.float64, device="cuda")
        gx, gy = torch.empty_like(Xk), torch.empty_like(Yk)
        ws = torch.empty(_lib.score_grad_workspace_bytes(Xk.shape[1], K, Xk.shape[2]), dtype=torch.uint8, device="cuda")
        kres = timed(lambda: _lib.score_grad(Xk, Yk, True, scores, None, gx, gy, ws), a.reps)
        extra = ""
        if K <= 32:
            must = 2.0 * K * n * d * 8
            extra = "   %.1f MB to move: %.0f GB/s" % (must / 1e6, must / (kres[0] * 1e-3) / 1e9)
        line(out, "(k) pfm_score_grad alone, scores and gradients", kres, extra)
        if a.only_ours or kind == "crps" and d != 1:
            continue
        for tag, yard in (("(i) torch cdist [n, K, K]", yard_cdist), ("(ii) torch broadcast difference [n, K, K, d]", yard_broadcast)):
            try:
                res = timed(fb(lambda: yard(X, Y)), a.reps)
                v = float(yard(X, Y).detach())
                off = abs(v - value)
                line(out, tag, res, "   value %.12g, off by %.3g (%s)" % (v, off, "right to 1e-9" if off <= 1e-9 else "WRONG"))
                print("  %-58s %10.2f x" % ("    over (a)", res[0] / timed(fb(lambda: fn(X, Y)), 3)[0]), file=out)
            except torch.cuda.OutOfMemoryError as e:
                print("  %-58s could not allocate: %s" % (tag, str(e).split(".")[0]), file=out)
            X.grad = None
            torch.cuda.empty_cache()
            out.flush()
    if out is not sys.stdout:
        out.close()


if __name__ == "__main__":
    main()
