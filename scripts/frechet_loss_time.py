#!/usr/bin/env python3
"""Warm timings of probaforms_amd.metrics.losses.frechet_loss (pfm_frechet_grad) against energy_loss and against a float64
torch-autograd Frechet loss on the same device, in one process (profiles/r32_frechet_loss_time.txt).  float64 tensors on the device,
the fake sample requiring a gradient (a training loop with a constant real sample: one route).  Shapes: 1 000 and 10 000 rows per
sample at d = 2 and 16; 65 536 rows at d = 16 and d = 64.  Per shape:
  (f)  frechet_loss, forward + backward;                 (fv) the same with no input requiring a gradient: the value alone;
  (f2) frechet_loss with BOTH samples requiring a gradient: both routes;
  (e)  energy_loss, forward + backward;                  (ev) its value alone;
  (t)  the torch yardstick, forward + backward: torch.cov, torch.linalg.eigh twice, the formula of fd.trace_sqrtm; its value is
       compared with ours ("right to 1e-9 of the scale" or "WRONG"), and it is run once under
       torch.cuda.set_sync_debug_mode("error") to see whether it waits for the device (ours is run the same way).
Then the eigen step alone, at d = 2, 16 and 64: pfm_sym_eig on one matrix (the real sample's covariance) with its sweep count, and
pfm_frechet_grad at 512 rows per sample, where the moments and the row kernel are a few workgroups and the call is the core launch
(one workgroup per route, two decompositions each), value alone, one route and both routes.
Each is warmed (one call, and as many as are timed if a call takes under a second); the figure is the median wall time per call with
a device synchronisation at both ends, with the fastest and slowest call, and torch's peak allocator bytes above what was allocated
before the call.

    python scripts/frechet_loss_time.py [out.txt] [--reps N]
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

SHAPES = [(n, d) for n in (1000, 10000) for d in (2, 16)] + [(65536, 16), (65536, 64)]
CORE_DS = (2, 16, 64)
CORE_ROWS = 512


def sample(n, d):
    rng = np.random.default_rng(n + d)
    X = rng.normal(size=(n, d)) @ (np.eye(d) + 0.3 * rng.normal(size=(d, d)) / np.sqrt(d)) + 1.0
    Y = 0.8 * rng.normal(size=(n, d)) + 0.3
    return torch.from_numpy(X).cuda(), torch.from_numpy(Y).cuda()


def yard(X, Y):
    """float64 torch autograd: the formula of fd.trace_sqrtm; its backward goes through eigh's eigenvector derivative"""
    mr, mf = X.mean(dim=0), Y.mean(dim=0)
    Cr, Cf = torch.cov(X.t()).reshape(X.shape[1], X.shape[1]), torch.cov(Y.t()).reshape(X.shape[1], X.shape[1])
    w, V = torch.linalg.eigh(Cr)
    S = (V * w.clamp_min(0.0).sqrt()) @ V.t()
    M = S @ Cf @ S
    lam = torch.linalg.eigvalsh((M + M.t()) * 0.5)
    return ((mr - mf) ** 2).sum() + torch.trace(Cr) + torch.trace(Cf) - 2.0 * lam.clamp_min(0.0).sqrt().sum()


def waits(fn):
    """does fn() run under torch.cuda.set_sync_debug_mode("error")?"""
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        fn()
        return "only enqueues (runs under sync_debug_mode error)"
    except RuntimeError as e:
        return "WAITS FOR THE DEVICE (sync_debug_mode error: %s)" % str(e).split("\n")[0][:60]
    finally:
        torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=None)
    ap.add_argument("--reps", type=int, default=7, help="timed calls of each")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    out = open(a.out, "w") if a.out else sys.stdout
    print("median [min .. max] ms per call, forward + backward unless it says otherwise; float64; %s"
          % torch.cuda.get_device_name(0), file=out)

    def fb(fn, *leaves):
        def run():
            for t in leaves:
                t.grad = None
            fn().backward()
        return run

    for n, d in SHAPES:
        X, Y = sample(n, d)
        Yg, Xg = Y.clone().requires_grad_(True), X.clone().requires_grad_(True)
        print("\nn = %d rows per sample, d = %d" % (n, d), file=out)
        f = timed(fb(lambda: losses.frechet_loss(X, Yg), Yg), a.reps)
        L, rank = losses.frechet_loss(X, Y, return_rank=True)
        ours = float(L)
        line(out, "(f)  frechet_loss, fake rows' gradient", f, "   value %.12g, rank %d; %s"
             % (ours, int(rank), waits(fb(lambda: losses.frechet_loss(X, Yg), Yg))))
        line(out, "(fv) the same, value only", timed(lambda: losses.frechet_loss(X, Y), a.reps))
        line(out, "(f2) frechet_loss, both samples' gradients", timed(fb(lambda: losses.frechet_loss(Xg, Yg), Xg, Yg), a.reps))
        e = timed(fb(lambda: losses.energy_loss(X, Yg), Yg), a.reps)
        line(out, "(e)  energy_loss", e)
        line(out, "(ev) the same, value only", timed(lambda: losses.energy_loss(X, Y), a.reps))
        print("  %-58s %10.2f x" % ("     energy_loss over frechet_loss", e[0] / f[0]), file=out)
        t = timed(fb(lambda: yard(X, Yg), Yg), a.reps)
        v = float(yard(X, Y))
        scale = abs(ours) + float(torch.cov(X.t()).reshape(d, d).trace() + torch.cov(Y.t()).reshape(d, d).trace())
        off = abs(v - ours)
        line(out, "(t)  torch.cov, eigh twice, the same formula", t, "   value %.12g, off by %.3g (%s); %s"
             % (v, off, "right to 1e-9 of the scale" if off <= 1e-9 * scale else "WRONG", waits(fb(lambda: yard(X, Yg), Yg))))
        print("  %-58s %10.2f x" % ("     over ours", t[0] / f[0]), file=out)
        Yg.grad = Xg.grad = None
        torch.cuda.empty_cache()
        out.flush()

    print("\nthe eigen step alone: one workgroup per matrix or route, pure latency", file=out)
    for d in CORE_DS:
        X, Y = sample(CORE_ROWS, d)
        C = torch.cov(X.t()).reshape(1, d, d).contiguous()
        w, V = torch.empty(1, d, dtype=torch.float64, device="cuda"), torch.empty(1, d, d, dtype=torch.float64, device="cuda")
        sweeps = torch.empty(1, dtype=torch.int32, device="cuda")
        ws = torch.empty(_lib.sym_eig_workspace_bytes(1, d), dtype=torch.uint8, device="cuda")
        k = timed(lambda: _lib.sym_eig(C, w, V, sweeps, ws), a.reps)
        line(out, "(k)  pfm_sym_eig, one matrix, d = %d" % d, k, "   %d sweeps" % int(sweeps[0]))
        line(out, "(kt) torch.linalg.eigh on it", timed(lambda: torch.linalg.eigh(C[0]), a.reps))
        Z = torch.cat([X, Y]).contiguous()
        value, grad = torch.empty(1, dtype=torch.float64, device="cuda"), torch.empty_like(Z)
        ws = torch.empty(_lib.frechet_grad_workspace_bytes(2 * CORE_ROWS, d, CORE_ROWS), dtype=torch.uint8, device="cuda")
        rc = d * 2.0 ** -52
        for tag, sides, g in (("value alone", 0, None), ("one route", 2, grad), ("both routes", 3, grad)):
            c = timed(lambda: _lib.frechet_grad(Z, CORE_ROWS, rc, sides, value, g, None, None, None, ws), a.reps)
            line(out, "(c)  pfm_frechet_grad, %d + %d rows, d = %d, %s" % (CORE_ROWS, CORE_ROWS, d, tag), c)
        out.flush()
    if out is not sys.stdout:
        out.close()


if __name__ == "__main__":
    main()
