"""Warm timings of scoring the predictive draws against observed targets, three ways, in one process
(profiles/r13_scores_time.txt), with the method of scripts/predict_time.py:
  (a) model.sample_many(C, K), the download it includes, then CRPS / PIT / quantiles / pinball in numpy by the sorted formula
  (b) model.sample_stats(C, K, quantiles): the same draws and the same sort without the scores (what existed before)
  (c) model.sample_scores(C, Y, K, quantiles)
Each variant is warmed for as many calls as are timed; the figure is the median wall time per call with a device
synchronisation at both ends.  The number to read is (c) - (b), the price of the extra pass over the sorted series.
Usage: python scripts/scores_time.py [out.txt]"""
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from probaforms_amd.models import ConditionalWGAN, RealNVP  # noqa: E402
from probaforms_amd.models._predict import scores_of_draws  # noqa: E402

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
    return statistics.median(ts), min(ts), max(ts)


def main():
    out = open(sys.argv[1], "w") if len(sys.argv) > 1 else sys.stdout
    nvp = lambda prior_rng, **kw: (lambda: RealNVP(n_epochs=1, batch_size=64, prior_rng=prior_rng, **kw))
    shapes = [("regression notebook: default RealNVP, d=1 c=1 n=1000 K=1000, prior_rng=host", nvp("host"), 1, 1, 1000, 1000),
              ("regression notebook: default RealNVP, d=1 c=1 n=1000 K=1000, prior_rng=device", nvp("device"), 1, 1, 1000, 1000),
              ("C2 net: 8 layers hidden=(128,), d=16 c=4 n=4096 K=256, prior_rng=host", nvp("host", hidden=(128,)), 16, 4, 4096, 256),
              ("C2 net: 8 layers hidden=(128,), d=16 c=4 n=4096 K=256, prior_rng=device", nvp("device", hidden=(128,)), 16, 4, 4096,
               256),
              ("ConditionalWGAN defaults (generator 100x100 relu, latent 1), d=1 c=1 n=1000 K=1000",
               lambda: ConditionalWGAN(n_epochs=1), 1, 1, 1000, 1000)]
    print("median [min .. max] ms per call; warm-up = as many calls as timed; %s" % torch.cuda.get_device_name(0), file=out)
    for title, make, d, c, n, K in shapes:
        rng = np.random.default_rng(0)
        torch.manual_seed(0)
        m = make()
        m.fit(rng.standard_normal((256, d)).astype(np.float32), rng.standard_normal((256, c)).astype(np.float32))
        C = rng.standard_normal((n, c)).astype(np.float32)
        Y = rng.standard_normal((n, d)).astype(np.float32)

        def many_numpy():
            return scores_of_draws(m.sample_many(C, K), Y, Q, False)

        def stats_q():
            return m.sample_stats(C, K, quantiles=Q)

        def scores():
            return m.sample_scores(C, Y, K, quantiles=Q)

        print("\n%s" % title, file=out)
        med = {}
        for label, fn, reps in [("(a) sample_many + numpy scores (sorted formula)", many_numpy, 3),
                                ("(b) sample_stats + quantiles", stats_q, 20),
                                ("(c) sample_scores", scores, 20)]:
            med[label[:3]] = timed(fn, reps)
            print("  %-50s %10.3f  [%9.3f .. %9.3f]" % ((label,) + med[label[:3]]), file=out)
            out.flush()
        print("  (c) - (b) = %.3f ms; (c) / (a) = %.4f" % (med["(c)"][0] - med["(b)"][0], med["(c)"][0] / med["(a)"][0]), file=out)
        out.flush()
    if out is not sys.stdout:
        out.close()


if __name__ == "__main__":
    main()
