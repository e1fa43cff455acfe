#!/usr/bin/env python3
"""Warm timings of probaforms_amd.metrics.losses.sinkhorn_loss at n = 1 000 and 10 000 rows per sample and d = 2 and 16
features, in one process (profiles/r23_sinkhorn_loss_time.txt).  Per shape, float64 tensors on the device, p = 2,
n_sinkhorn = 100, eps = 0.1 median^2 (the pooled median, taken once outside the timing), the fake sample requiring a gradient:
  (i)   sinkhorn_loss(X, Y, epsilon=eps) forward + backward, and with no input requiring a gradient (the value alone);
  (k)   pfm_sinkhorn_grad alone between device events, without and with the gradient: the share of a call spent in the
        steps and in the gradient sweep;
  (ii)  sinkhorn_divergence_full_sample on the same tensors: the bootstrap step kernel at one replicate, its read-back to
        numpy included;
  (iii) a float64 torch loss on the same device, forward + backward, in the GeomLoss style: torch.cdist of the pooled rows,
        100 logsumexp steps under no_grad, the last step under autograd on costs formed again with their columns detached.  Its value and its
        gradient are compared with (i)'s; torch's peak allocator bytes are reported for every line;
  (iv)  energy_loss(X, Y) forward + backward, for scale.
Each is warmed (one call, and as many as are timed if a call takes under a second); the figure is the median wall time per call
with a device synchronisation at both ends, with the fastest and slowest call.

    python scripts/sinkhorn_loss_time.py [out.txt] [--reps N] [--shape NxD]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from probaforms_amd.metrics import _lib, losses, sinkhorn as sk  # noqa: E402
from probaforms_amd.metrics.twosample import _median  # noqa: E402

P, STEPS, REG = 2, 100, 0.1


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


def kernel_ms(Z, nr, eps, grad, reps):
    """median ms of pfm_sinkhorn_grad between device events"""
    N, d = Z.shape
    value, drift = (torch.empty(1, dtype=torch.float64, device="cuda") for _ in range(2))
    ws = torch.empty(_lib.sinkhorn_grad_workspace_bytes(N, d, nr), dtype=torch.uint8, device="cuda")
    ts = []
    for i in range(reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        _lib.sinkhorn_grad(Z, nr, P, eps, STEPS, value, drift, grad, None, ws)
        b.record()
        torch.cuda.synchronize()
        if i:
            ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def softmin(h, C, eps):
    return -eps * (torch.logsumexp((h[None, :] - C) / eps, dim=1) - np.log(C.shape[1]))


def torch_loss(X, Y, eps):
    nr = X.shape[0]
    Z = torch.cat([X, Y])
    with torch.no_grad():
        C = torch.cdist(Z, Z) ** P
        C_RF, C_FR, C_RR, C_FF = C[:nr, nr:], C[nr:, :nr], C[:nr, :nr], C[nr:, nr:]
        f, u = (torch.zeros(nr, dtype=torch.float64, device=Z.device) for _ in range(2))
        g, v = (torch.zeros(Z.shape[0] - nr, dtype=torch.float64, device=Z.device) for _ in range(2))
        for _ in range(STEPS):
            f, g, u, v = (0.5 * (f + softmin(g, C_RF, eps)), 0.5 * (g + softmin(f, C_FR, eps)),
                          0.5 * (u + softmin(u, C_RR, eps)), 0.5 * (v + softmin(v, C_FF, eps)))
        del C
    C = torch.cdist(Z, Z.detach()) ** P                  # rows differentiable, columns held fixed
    C_RF, C_FR, C_RR, C_FF = C[:nr, nr:], C[nr:, :nr], C[:nr, :nr], C[nr:, nr:]
    return ((softmin(g, C_RF, eps) - softmin(u, C_RR, eps)).mean() + (softmin(f, C_FR, eps) - softmin(v, C_FF, eps)).mean())


def line(out, name, res, extra=""):
    med, lo, hi, peak = res
    print("  %-62s %10.2f  [%9.2f .. %9.2f]   peak %8.1f MB%s" % (name, med, lo, hi, peak / 1e6, extra), file=out)
    out.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=None)
    ap.add_argument("--reps", type=int, default=5, help="timed calls of each")
    ap.add_argument("--shape", default=None, help="one shape only: rows per sample x features, e.g. 10000x16")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    out = open(a.out, "w") if a.out else sys.stdout
    print("median [min .. max] ms per call, forward + backward unless it says otherwise; float64, p = %d, n_sinkhorn = %d; %s"
          % (P, STEPS, torch.cuda.get_device_name(0)), file=out)
    shapes = [(n, d) for n in (1000, 10000) for d in (2, 16)]
    if a.shape is not None:
        shapes = [tuple(int(v) for v in a.shape.split("x"))]
    for n, d in shapes:
        rng = np.random.default_rng(n + d)
        X = torch.from_numpy(rng.normal(size=(n, d))).cuda()
        Y = torch.from_numpy(rng.normal(0.3, 1.2, size=(n, d))).cuda().requires_grad_(True)
        Yv = Y.detach()
        eps = float(sk.epsilon_of(_median(X, Yv), P, REG))
        print("\nn = %d rows per sample, d = %d, eps = %.4g" % (n, d, eps), file=out)

        def ours():
            return losses.sinkhorn_loss(X, Y, p=P, epsilon=eps, n_sinkhorn=STEPS)

        def fb(fn):
            def run():
                Y.grad = None
                fn().backward()
            return run

        both = timed(fb(ours), a.reps)
        S, drift = losses.sinkhorn_loss(X, Y, p=P, epsilon=eps, n_sinkhorn=STEPS, return_drift=True)
        Y.grad = None
        S.backward()
        grad, S = Y.grad.clone(), S.detach()
        line(out, "(i) sinkhorn_loss", both, "   value %.12g, drift %.3g" % (float(S), float(drift)))
        alone = timed(lambda: losses.sinkhorn_loss(X, Yv, p=P, epsilon=eps, n_sinkhorn=STEPS), a.reps)
        line(out, "(i) sinkhorn_loss, value only", alone)
        Z = torch.cat([X, Yv]).contiguous()
        k_value = kernel_ms(Z, n, eps, None, a.reps)
        k_both = kernel_ms(Z, n, eps, torch.empty_like(Z), a.reps)
        print("  %-62s %10.2f  value only; %.2f with the gradient: steps %.1f %%, gradient sweep %.1f %% of the call"
              % ("(k) pfm_sinkhorn_grad alone (device events)", k_value, k_both, 100 * k_value / k_both,
                 100 * (k_both - k_value) / k_both), file=out)
        res = timed(lambda: sk.sinkhorn_divergence_full_sample(X, Yv, p=P, epsilon=eps, n_sinkhorn=STEPS), a.reps)
        metric = sk.sinkhorn_divergence_full_sample(X, Yv, p=P, epsilon=eps, n_sinkhorn=STEPS)
        line(out, "(ii) sinkhorn_divergence_full_sample, forward only", res,
             "   value %.12g, off (i) by %.3g" % (metric.value, abs(metric.value - float(S))))
        print("  %-62s %10.2f x" % ("    (ii) over (i) value only", res[0] / alone[0]), file=out)
        try:
            res = timed(fb(lambda: torch_loss(X, Y, eps)), a.reps)
            Y.grad = None
            T = torch_loss(X, Y, eps)
            T.backward()
            off = abs(float(T.detach()) - float(S))
            goff = float((Y.grad - grad).abs().max())
            verdict = "right to 1e-9" if off <= 1e-9 else "WRONG"
            line(out, "(iii) torch cdist + logsumexp, last step under autograd", res,
                 "   value %.12g, off by %.3g (%s); gradient off by at most %.3g of %.3g"
                 % (float(T.detach()), off, verdict, goff, float(grad.abs().max())))
            print("  %-62s %10.2f x" % ("    (iii) over (i)", res[0] / both[0]), file=out)
        except torch.cuda.OutOfMemoryError as e:
            print("  %-62s could not allocate: %s" % ("(iii) torch cdist + logsumexp", str(e).split(".")[0]), file=out)
        Y.grad = None
        torch.cuda.empty_cache()
        line(out, "(iv) energy_loss", timed(fb(lambda: losses.energy_loss(X, Y)), a.reps))
        Y.grad = None
    if out is not sys.stdout:
        out.close()


if __name__ == "__main__":
    main()
