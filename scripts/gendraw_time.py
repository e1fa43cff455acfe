"""Warm timings of the predictive-statistics workload of CVAE, ConditionalWGAN and ConditionalNormal, three ways, in one
process (profiles/r12_gendraw_time.txt), with the method of scripts/predict_time.py:
  (a) the notebook loop: np.array([model.sample(C) for _ in range(K)]) then numpy mean / std (/ quantile)
  (b) one tiled call: the generator / decoder / net on C.repeat(K, 1) then torch reductions on the device
  (c) model.sample_stats(C, K)
Each variant is warmed for as many calls as are timed; the figure is the median wall time per call with a device
synchronisation at both ends.  The whole table is measured `repeats` times; a row shows the median of the repeats' medians
and their spread (min .. max).  Usage: python scripts/gendraw_time.py [out.txt] [repeats=3]"""
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from probaforms_amd.models import CVAE, ConditionalNormal, ConditionalWGAN  # noqa: E402

Q = (0.05, 0.95)


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
    return statistics.median(ts)


def tiled_draws(m, Cd, K, n, d):
    """[K, n, d] on the device from ONE call of the model's own network on the conditions repeated K times"""
    Ct = Cd.repeat(K, 1)
    if isinstance(m, CVAE):
        return m.decoder(torch.normal(0, 1, (K * n, m.lat_size)), Ct).view(K, n, d)
    if isinstance(m, ConditionalWGAN):
        return m.generator(torch.normal(0, 1, (K * n, m.latent_dim)), Ct).view(K, n, d)
    return m.model(None, Ct)[0].view(K, n, d)


def variants(m, C, K, d):
    n = len(C)
    Cd = torch.from_numpy(C).cuda()
    qd = torch.tensor(Q, device="cuda")

    def loop():
        X = np.array([m.sample(C) for _ in range(K)])
        return X.mean(axis=0), X.std(axis=0)

    def loop_q():
        X = np.array([m.sample(C) for _ in range(K)])
        return X.mean(axis=0), X.std(axis=0), np.quantile(X, Q, axis=0)

    def tiled():
        X = tiled_draws(m, Cd, K, n, d)
        return X.mean(0), X.std(0, unbiased=False)

    def tiled_q():
        X = tiled_draws(m, Cd, K, n, d)
        return X.mean(0), X.std(0, unbiased=False), torch.quantile(X, qd, dim=0)

    def stats():
        return m.sample_stats(C, K)

    def stats_q():
        return m.sample_stats(C, K, quantiles=Q)

    return [("(a) notebook loop + numpy mean/std", loop, 3), ("(a) ... + np.quantile(0.05, 0.95)", loop_q, 3),
            ("(b) one tiled call + torch mean/std", tiled, 10), ("(b) ... + torch.quantile", tiled_q, 10),
            ("(c) sample_stats", stats, 10), ("(c) sample_stats + quantiles", stats_q, 10)]


def main():
    out = open(sys.argv[1], "w") if len(sys.argv) > 1 else sys.stdout
    repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    shapes = [("ConditionalWGAN defaults (generator 100x100 relu, latent 1), d=1 c=1 n=1000 K=1000",
               lambda: ConditionalWGAN(n_epochs=1), 1, 1, 1000, 1000),
              ("CVAE defaults (decoder hidden 10 tanh, latent 2), d=1 c=1 n=1000 K=1000", lambda: CVAE(n_epochs=1), 1, 1, 1000, 1000),
              ("CVAE C5 net (hidden 128 tanh, latent 2), d=16 c=4 n=4096 K=256",
               lambda: CVAE(latent_dim=2, hidden=(128,), n_epochs=1, batch_size=64), 16, 4, 4096, 256),
              ("ConditionalNormal defaults (hidden 10 tanh, full covariance), d=1 c=1 n=1000 K=1000",
               lambda: ConditionalNormal(n_epochs=1), 1, 1, 1000, 1000)]
    print("ms per call: median over %d repeats of the per-repeat median [min .. max of the repeats' medians]; warm-up = as many "
          "calls as timed; %s" % (repeats, torch.cuda.get_device_name(0)), file=out)
    for title, make, d, c, n, K in shapes:
        rng = np.random.default_rng(0)
        torch.manual_seed(0)
        m = make()
        m.fit(rng.standard_normal((256, d)).astype(np.float32), rng.standard_normal((256, c)).astype(np.float32))
        C = rng.standard_normal((n, c)).astype(np.float32)
        print("\n%s" % title, file=out)
        med = {}
        for label, fn, reps in variants(m, C, K, d):
            vals = [timed(fn, reps) for _ in range(repeats)]
            med[label[:3] + ("q" if "quantile" in label else "")] = (statistics.median(vals), min(vals), max(vals))
            print("  %-44s %10.3f  [%9.3f .. %9.3f]" % (label, statistics.median(vals), min(vals), max(vals)), file=out)
            out.flush()
        for suffix, what in (("", "mean/std"), ("q", "with quantiles")):
            a, b, cc = (med.get(k + suffix) for k in ("(a)", "(b)", "(c)"))
            if a and cc:
                line = "  %s: (c)/(a) = %.4f, worst case over the repeats %.4f" % (what, cc[0] / a[0], cc[2] / a[1])
                if b:
                    line += "; (c)/(b) = %.3f, range over the repeats %.3f .. %.3f" % (cc[0] / b[0], cc[1] / b[2], cc[2] / b[1])
                print(line, file=out)
        out.flush()
    if out is not sys.stdout:
        out.close()


if __name__ == "__main__":
    main()
