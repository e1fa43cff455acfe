"""Warm timings of the predictive-statistics workload, three ways, in one process (profiles/r10_predict_time.txt):
  (a) the notebook loop: np.array([model.sample(C) for _ in range(K)]) then numpy mean / std
  (b) the tiled call: nf.sample(C.repeat(K, 1)) then torch.mean / torch.std on the device
  (c) nf.sample_stats(C, K)
Each variant is warmed for as many calls as are timed; the figure is the median wall time per call with a device
synchronisation at both ends.  Usage: python scripts/predict_time.py [out.txt]"""
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from probaforms_amd.models import RealNVP  # noqa: E402


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


def main():
    out = open(sys.argv[1], "w") if len(sys.argv) > 1 else sys.stdout
    shapes = [("regression notebook: default RealNVP, d=1 c=1 n=1000 K=1000", dict(), 1, 1, 1000, 1000),
              ("C2 net: 8 layers hidden=(128,), d=16 c=4 n=4096 K=256", dict(hidden=(128,)), 16, 4, 4096, 256)]
    print("median [min .. max] ms per call; warm-up = as many calls as timed; %s" % torch.cuda.get_device_name(0), file=out)
    for title, kw, d, c, n, K in shapes:
        for prior_rng in ("host", "device"):
            rng = np.random.default_rng(0)
            torch.manual_seed(0)
            m = RealNVP(n_epochs=1, batch_size=64, prior_rng=prior_rng, **kw)
            m.fit(rng.standard_normal((256, d)).astype(np.float32), rng.standard_normal((256, c)).astype(np.float32))
            C = rng.standard_normal((n, c)).astype(np.float32)
            Cd = torch.from_numpy(C).cuda()

            def loop():
                X = np.array([m.sample(C) for _ in range(K)])
                return X.mean(axis=0), X.std(axis=0)

            def loop_q():
                X = np.array([m.sample(C) for _ in range(K)])
                return X.mean(axis=0), X.std(axis=0), np.quantile(X, (0.05, 0.95), axis=0)

            def tiled():
                with torch.no_grad():
                    X = m.nf.sample(Cd.repeat(K, 1)).view(K, n, d)
                    return X.mean(0), X.std(0, unbiased=False)

            def tiled_q():
                with torch.no_grad():
                    X = m.nf.sample(Cd.repeat(K, 1)).view(K, n, d)
                    return X.mean(0), X.std(0, unbiased=False), torch.quantile(X, torch.tensor([0.05, 0.95], device=X.device), dim=0)

            def stats():
                return m.nf.sample_stats(Cd, K)

            def stats_q():
                return m.nf.sample_stats(Cd, K, quantiles=(0.05, 0.95))

            print("\n%s, prior_rng=%s" % (title, prior_rng), file=out)
            for label, fn, reps in [("(a) notebook loop + numpy mean/std", loop, 3),
                                    ("(a) ... + np.quantile(0.05, 0.95)", loop_q, 3),
                                    ("(b) nf.sample(C.repeat(K,1)) + torch mean/std", tiled, 20),
                                    ("(b) ... + torch.quantile", tiled_q, 20),
                                    ("(c) nf.sample_stats", stats, 20),
                                    ("(c) nf.sample_stats + quantiles", stats_q, 20)]:
                med, lo, hi = timed(fn, reps)
                print("  %-52s %10.3f  [%9.3f .. %9.3f]" % (label, med, lo, hi), file=out)
                out.flush()
    if out is not sys.stdout:
        out.close()


if __name__ == "__main__":
    main()
