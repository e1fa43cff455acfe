#!/usr/bin/env python3
"""Generate tests/golden/metrics1d_*.npz by running the REFERENCE's eight 1-D metrics (probaforms/metrics/ks1d.py,
div1d.py of hse-cs/probaforms).

Run it where a checkout of the reference and its CPU dependencies (sklearn, scipy) are at hand:

    PYTHONPATH=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_metrics1d.py

Per case the file holds the inputs X, Y, the numpy seed, n_iters, bins_hist (for kullback_leibler_1d /
jensen_shannon_1d) and bins_kde (for the _kde pair), and per metric <m>:
  <m>_raises   whether the reference's public call raises (then nothing else is stored for <m>)
  <m>_mean, <m>_std, <m>_next   the public call's (mean, std) and the next np.random.random() after it
  <m>_rep      [n_iters, d]: the per-replicate, per-feature statistics, replayed with the reference's own 1-D
               functions on sklearn.utils.resample draws under the same seed; the replay's feature average is
               checked to give the public call's (mean, std) exactly (NaN where the reference's is NaN).
The files are named metrics1d_* (the multivariate fixtures' tests glob metrics_*).
"""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

from probaforms.metrics import div1d, ks1d  # the reference  # noqa: E402
from sklearn.utils import resample  # noqa: E402

assert not getattr(sys.modules["probaforms"], "__probaforms_amd__", False), "must import the reference"
warnings.filterwarnings("ignore")

METRICS = {   # public name -> (module, 1-D function, takes bins, which bins)
    "kolmogorov_smirnov_1d": (ks1d, ks1d._ks1d, None),
    "cramer_von_mises_1d": (ks1d, ks1d._cvm1d, None),
    "roc_auc_score_1d": (ks1d, ks1d._roc1d, None),
    "anderson_darling_1d": (ks1d, ks1d._anderson1d, None),
    "kullback_leibler_1d": (div1d, div1d._kl1d, "bins_hist"),
    "jensen_shannon_1d": (div1d, div1d._js1d, "bins_hist"),
    "kullback_leibler_1d_kde": (div1d, div1d._kl1d_kde, "bins_kde"),
    "jensen_shannon_1d_kde": (div1d, div1d._js1d_kde, "bins_kde"),
}


def replay(fn1d, X, Y, seed, n_iters, extra):
    np.random.seed(seed)
    S = np.empty((n_iters, X.shape[1]))
    for r in range(n_iters):
        Xb, Yb = resample(X), resample(Y)
        for f in range(X.shape[1]):
            S[r, f] = fn1d(Xb[:, f], Yb[:, f], *extra)
    return S


def average(S):
    scores = []
    for r in range(S.shape[0]):
        s = 0
        for f in range(S.shape[1]):
            s += S[r, f] / S.shape[1]
        scores.append(s)
    scores = np.array(scores)
    return scores.mean(axis=0), scores.std(axis=0)


def case(name, X, Y, seed, n_iters, bins_hist=10, bins_kde=101, only=None):
    out = dict(X=X, Y=Y, seed=seed, n_iters=n_iters, bins_hist=bins_hist, bins_kde=bins_kde)
    for m, (mod, fn1d, bkey) in METRICS.items():
        if only is not None and m not in only:
            continue
        extra = () if bkey is None else (out[bkey],)
        np.random.seed(seed)
        try:
            mu, sd = getattr(mod, m)(X, Y, n_iters, *extra)
        except (ValueError, IndexError):
            out[m + "_raises"] = True
            print(name, m, "raises")
            continue
        nxt = np.random.random()
        S = replay(fn1d, X, Y, seed, n_iters, extra)
        rmu, rsd = average(S)
        assert (mu == rmu or (np.isnan(mu) and np.isnan(rmu))) and (sd == rsd or (np.isnan(sd) and np.isnan(rsd))), \
            (name, m, mu, rmu, sd, rsd)
        out.update({m + "_raises": False, m + "_mean": mu, m + "_std": sd, m + "_next": nxt, m + "_rep": S})
        print(name, m, X.shape, Y.shape, mu, sd, "nan reps %d" % np.isnan(S).sum())
    np.savez_compressed(os.path.join(HERE, "metrics1d_%s.npz" % name), **out)


def main():
    rng = np.random.default_rng(4242)
    sig = np.array([[1, 0.7], [0.7, 1]])
    case("diff_100_153", rng.multivariate_normal([0, 0], sig, 100),
         rng.multivariate_normal([0.3, 0], sig * 1.5, 153), seed=21, n_iters=100)
    case("same_1d", rng.normal(0, 1, 100).reshape(-1, 1), rng.normal(0, 1, 100).reshape(-1, 1), seed=22, n_iters=100)
    # heavy ties inside and across the samples: rounded normals and small integers
    X = np.column_stack([np.round(rng.normal(0, 1, 120), 1), rng.integers(0, 5, 120), np.round(rng.normal(0, 2, 120))])
    Y = np.column_stack([np.round(rng.normal(0.2, 1, 90), 1), rng.integers(1, 6, 90), np.round(rng.normal(0, 2, 90))])
    case("ties", X.astype(np.float64), Y.astype(np.float64), seed=23, n_iters=60)
    # values on histogram edges: integers on edges of 10 and 5 bins, tenths on the rounded edges k * 0.1 of 10 bins
    X = np.column_stack([rng.integers(0, 11, 80), rng.integers(0, 11, 80) / 10.0])
    Y = np.column_stack([rng.integers(0, 11, 70), rng.integers(0, 11, 70) / 10.0])
    X[:2] = [[0, 0.0], [10, 1.0]]
    case("edges", X.astype(np.float64), Y.astype(np.float64), seed=24, n_iters=40)
    case("edges_bins", X.astype(np.float64), Y.astype(np.float64), seed=25, n_iters=40, bins_hist=5, bins_kde=37)
    A = rng.normal(size=(16, 16)) / 4
    X = np.tanh(rng.normal(size=(300, 16)) @ A)
    Y = np.tanh(rng.normal(size=(250, 16)) @ A + 0.1) * 1.1
    case("d16", X, Y, seed=26, n_iters=10)
    # KDE underflow: a wide sample against a narrow one (most grid densities of either are exp() = 0) ...
    case("kde_wide", rng.normal(0, 1e4, 100).reshape(-1, 1), rng.normal(0, 1, 100).reshape(-1, 1), seed=27, n_iters=30)
    # ... and replicates where the narrow sample's densities are all 0 (both pooled extremes from the wide sample)
    X = rng.normal(5, 0.01, 60).reshape(-1, 1)
    Y = np.concatenate([rng.normal(0, 5000, 58), [-1.1e4, 1.37e4]]).reshape(-1, 1)
    case("kde_allzero", X, Y, seed=28, n_iters=30)
    # the raising cases: cramervonmises_2samp with a 1-row sample, anderson_ksamp with one distinct pooled value
    case("cvm_1row", np.array([[0.5]]), rng.normal(0, 1, 7).reshape(-1, 1), seed=29, n_iters=5)
    case("ad_one_value", np.array([[1.0], [1.0], [1.0], [2.0]]), np.array([[1.0], [1.0]]), seed=30, n_iters=20)


if __name__ == "__main__":
    main()
