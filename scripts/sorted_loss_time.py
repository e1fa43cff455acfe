#!/usr/bin/env python3
"""Warm timings of probaforms_amd.metrics.losses.crps_loss by its two routes, method="pairs" (pfm_score_grad) against
method="sorted" (pfm_sort_score), and of pinball_loss, in one process (profiles/r31_sorted_loss_time.txt).  float64 tensors on the
device, the draws requiring a gradient.  Pairs against sorted: n = 1 000, d = 1, K = 1 000; n = 4 096, d = 16, K = 256; n = 65 536,
d = 16, K = 2, 8, 32.  Sorted alone (the pair route stops at K = 1024): n = 1 000, d = 1, K = 8 192, and the same with every draw
of a series equal: the tie scan must cost what distinct draws cost.  pinball_loss at the first two shapes.  Per shape:
  (p)  crps_loss(method="pairs"), forward + backward;    (pv) the same with no input requiring a gradient: the values alone;
  (s)  crps_loss(method="sorted"), forward + backward;   (sv) its values alone;
  (q)  pinball_loss at the levels 0.05, 0.5, 0.95, forward + backward;   (qv) its values alone;
  (t)  the float64 torch-autograd yardstick on the same device, forward + backward: torch.sort along the draws, then the same
       formulas (for the CRPS with c_i = 2 i - K + 1: right for the value whatever the ties are).
The VALUE of (s), (q) and of each yardstick is compared with its counterpart: "right to 1e-9" or "WRONG".  Each is warmed (one
call, and as many as are timed if a call takes under a second); the figure is the median wall time per call with a device
synchronisation at both ends, with the fastest and slowest call, and torch's peak allocator bytes above what was allocated before
the call.

    python scripts/sorted_loss_time.py [out.txt] [--reps N]
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

BOTH = [(1000, 1, 1000), (4096, 16, 256), (65536, 16, 2), (65536, 16, 8), (65536, 16, 32)]
SORTED_ALONE = (1000, 1, 8192)
PINBALL = BOTH[:2]
LEVELS = (0.05, 0.5, 0.95)


def yard_crps(X, Y):
    """fair CRPS, mean over the series, from torch.sort along the draws"""
    K = X.shape[0]
    Ts = torch.sort(X - Y[None], dim=0).values
    c = (2.0 * torch.arange(K, dtype=torch.float64, device=X.device) - (K - 1)).view(K, 1, 1)
    return (Ts.abs().sum(dim=0) / K - (c * Ts).sum(dim=0) / (K * (K - 1.0))).mean()


def yard_pinball(X, Y):
    """the pinball scores of numpy's linear quantiles, mean over levels and series, from torch.sort along the draws"""
    K = X.shape[0]
    Ts = torch.sort(X - Y[None], dim=0).values
    total = 0.0
    for p in LEVELS:
        h = p * (K - 1)
        i = min(int(np.floor(h)), max(K - 2, 0))
        frac = h - i
        qt = torch.lerp(Ts[i], Ts[min(i + 1, K - 1)], frac)
        total = total + (-qt * (p - (qt > 0).to(qt.dtype))).mean()
    return total / len(LEVELS)


def check(v, ref):
    off = abs(v - ref)
    return "   value %.12g, off by %.3g (%s)" % (v, off, "right to 1e-9" if off <= 1e-9 else "WRONG")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=None)
    ap.add_argument("--reps", type=int, default=7, help="timed calls of each")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    out = open(a.out, "w") if a.out else sys.stdout
    print("median [min .. max] ms per call, forward + backward unless it says otherwise; float64; fair=True; %s"
          % torch.cuda.get_device_name(0), file=out)

    def fb(X, f):
        def run():
            X.grad = None
            f().backward()
        return run

    def draws(n, d, K, equal=False):
        rng = np.random.default_rng(n + d + K)
        X = rng.normal(size=(K, n, d))
        if equal:
            X[:] = X[0]
        return torch.from_numpy(X).cuda().requires_grad_(True), torch.from_numpy(rng.normal(0.3, 1.2, size=(n, d))).cuda()

    def head(n, d, K, what):
        plan = _lib.sort_score_plan(n * d, K)
        print("\nn = %d rows, d = %d, K = %d draws per row, %s; sorted plan: %d series per workgroup, pitch %d, %d LDS bytes, "
              "%d workgroups" % ((n, d, K, what) + plan), file=out)

    def sorted_lines(X, Y, ref=None):
        Xv = X.detach()
        s = timed(fb(X, lambda: losses.crps_loss(X, Y, method="sorted")), a.reps)
        v = float(losses.crps_loss(Xv, Y, method="sorted"))
        line(out, '(s)  crps_loss(method="sorted")', s, "   value %.12g" % v if ref is None else check(v, ref))
        sv = timed(lambda: losses.crps_loss(Xv, Y, method="sorted"), a.reps)
        line(out, "(sv) the same, values only", sv)
        return s, sv, v

    def torch_line(X, Y, yard, ref, ours):
        try:
            t = timed(fb(X, lambda: yard(X, Y)), a.reps)
            line(out, "(t)  torch.sort and the same formulas", t, check(float(yard(X, Y).detach()), ref))
            print("  %-58s %10.2f x" % ("     over ours", t[0] / ours[0]), file=out)
        except torch.cuda.OutOfMemoryError as e:
            print("  %-58s could not allocate: %s" % ("(t)  torch.sort and the same formulas", str(e).split(".")[0]), file=out)
        X.grad = None
        torch.cuda.empty_cache()
        out.flush()

    for n, d, K in BOTH:
        X, Y = draws(n, d, K)
        Xv = X.detach()
        head(n, d, K, "crps_loss, pairs against sorted")
        p = timed(fb(X, lambda: losses.crps_loss(X, Y)), a.reps)
        ref = float(losses.crps_loss(Xv, Y))
        line(out, '(p)  crps_loss(method="pairs")', p, "   value %.12g" % ref)
        pv = timed(lambda: losses.crps_loss(Xv, Y), a.reps)
        line(out, "(pv) the same, values only", pv)
        s, sv, _ = sorted_lines(X, Y, ref)
        print("  %-58s %10.2f x forward + backward, %.2f x values only" % ("     pairs over sorted", p[0] / s[0], pv[0] / sv[0]), file=out)
        torch_line(X, Y, yard_crps, ref, s)

    n, d, K = SORTED_ALONE
    res = {}
    for equal in (False, True):
        X, Y = draws(n, d, K, equal)
        head(n, d, K, "crps_loss sorted alone, %s" % ("EVERY DRAW OF A SERIES EQUAL" if equal else "distinct draws"))
        res[equal] = sorted_lines(X, Y)
        torch_line(X, Y, yard_crps, res[equal][2], res[equal][0])
    (sd, vd, _), (se, ve, _) = res[False], res[True]
    for tag, x, y in (("forward + backward", sd, se), ("values only", vd, ve)):
        spread = max(x[2] - x[1], y[2] - y[1])
        print("  all equal against distinct, %s: medians %.3f and %.3f ms, apart by %.3f ms; run-to-run spread (max - min) %.3f ms: %s"
              % (tag, y[0], x[0], abs(y[0] - x[0]), spread, "within it" if abs(y[0] - x[0]) <= spread else "OUTSIDE IT"), file=out)

    for n, d, K in PINBALL:
        X, Y = draws(n, d, K)
        Xv = X.detach()
        head(n, d, K, "pinball_loss at the levels %s" % (LEVELS,))
        ref = float(yard_pinball(Xv, Y))
        q = timed(fb(X, lambda: losses.pinball_loss(X, Y, quantiles=LEVELS)), a.reps)
        line(out, "(q)  pinball_loss", q, check(float(losses.pinball_loss(Xv, Y, quantiles=LEVELS)), ref))
        line(out, "(qv) the same, values only", timed(lambda: losses.pinball_loss(Xv, Y, quantiles=LEVELS), a.reps))
        torch_line(X, Y, yard_pinball, ref, q)
    if out is not sys.stdout:
        out.close()


if __name__ == "__main__":
    main()
