#!/usr/bin/env python3
"""Generate tests/golden/wasserstein_*.npz: bootstrapped 1-D and sliced Wasserstein distances computed with scipy 1.15's
scipy.stats.wasserstein_distance (p = 1) and, for samples of one size, the sorted-pair formula
sqrt(mean((sort x - sort y)^2)) (p = 2).  Needs numpy and scipy only:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_wasserstein.py

The bootstrap is the one of the reference's metrics: per iteration sklearn.utils.resample(X), then resample(Y), which
on numpy's global legacy generator is randint(0, n, size=n).  The sliced cases draw their directions first,
np.random.normal(size=(n_projections, d)) with every row divided by its 2-norm, and project with the sum over the
features in order.

Per case the file holds kind ('1d' or 'sliced'), X, Y, seed, n_iters, p (the sliced ones n_projections too) and
  rep    [n_iters, d] per-replicate, per-feature W_p ('1d') or [n_iters] per-replicate sliced W_p
  mean, std   of the replicates (the '1d' ones averaged over the features first, `score += S[r, f] / d`)
  next   the next np.random.random() after the call's draws
"""
import os

import numpy as np
from scipy.stats import wasserstein_distance

HERE = os.path.dirname(os.path.abspath(__file__))


def dist(x, y, p):
    if p == 1:
        return wasserstein_distance(x, y)
    assert len(x) == len(y)
    return np.sqrt(np.mean((np.sort(x) - np.sort(y)) ** 2))


def resample(X):
    return X[np.random.randint(0, len(X), size=len(X))]


def save(name, **out):
    np.savez_compressed(os.path.join(HERE, "wasserstein_%s.npz" % name), **out)
    print(name, out["X"].shape, out["Y"].shape, "p", out["p"], out["mean"], out["std"])


def case_1d(name, X, Y, seed, n_iters, p):
    np.random.seed(seed)
    S = np.empty((n_iters, X.shape[1]))
    for r in range(n_iters):
        Xb, Yb = resample(X), resample(Y)
        for f in range(X.shape[1]):
            S[r, f] = dist(Xb[:, f], Yb[:, f], p)
    nxt = np.random.random()
    scores = []
    for r in range(n_iters):
        s = 0
        for f in range(X.shape[1]):
            s += S[r, f] / X.shape[1]
        scores.append(s)
    scores = np.array(scores)
    save(name, kind="1d", X=X, Y=Y, seed=seed, n_iters=n_iters, p=p, rep=S, mean=scores.mean(axis=0),
         std=scores.std(axis=0), next=nxt)


def case_sliced(name, X, Y, seed, n_iters, n_projections, p):
    np.random.seed(seed)
    th = np.random.normal(size=(n_projections, X.shape[1]))
    th = th / np.sqrt((th * th).sum(axis=1))[:, None]
    PX, PY = np.zeros((n_projections, len(X))), np.zeros((n_projections, len(Y)))
    for j in range(X.shape[1]):
        PX = PX + X[:, j][None, :] * th[:, j][:, None]
        PY = PY + Y[:, j][None, :] * th[:, j][:, None]
    S = np.empty(n_iters)
    for r in range(n_iters):
        Xb, Yb = resample(PX.T), resample(PY.T)
        w = np.array([dist(Xb[:, k], Yb[:, k], p) for k in range(n_projections)])
        S[r] = np.mean(w) if p == 1 else np.sqrt(np.mean(w * w))
    nxt = np.random.random()
    save(name, kind="sliced", X=X, Y=Y, seed=seed, n_iters=n_iters, n_projections=n_projections, p=p, rep=S,
         mean=S.mean(axis=0), std=S.std(axis=0), next=nxt)


def main():
    rng = np.random.default_rng(1515)
    sig = np.array([[1, 0.7], [0.7, 1]])
    case_1d("p1_diff_100_153", rng.multivariate_normal([0, 0], sig, 100), rng.multivariate_normal([0.3, 0], sig * 1.5, 153),
            seed=41, n_iters=40, p=1)
    # heavy ties inside and across the samples
    X = np.column_stack([np.round(rng.normal(0, 1, 120), 1), rng.integers(0, 5, 120), np.round(rng.normal(0, 2, 120))])
    Y = np.column_stack([np.round(rng.normal(0.2, 1, 90), 1), rng.integers(1, 6, 90), np.round(rng.normal(0, 2, 90))])
    case_1d("p1_ties", X.astype(np.float64), Y.astype(np.float64), seed=42, n_iters=30, p=1)
    case_1d("p1_1row", np.array([[0.5]]), rng.normal(0, 1, 7).reshape(-1, 1), seed=43, n_iters=5, p=1)
    case_1d("p2_equal_64", rng.normal(size=(64, 2)), rng.normal(0.4, 1.3, size=(64, 2)), seed=44, n_iters=30, p=2)
    case_1d("p2_equal_ties", np.round(rng.normal(size=(50, 3)), 1), np.round(rng.normal(0.1, 1, size=(50, 3)), 1), seed=45,
            n_iters=30, p=2)
    case_sliced("sliced_p1", rng.normal(size=(80, 3)), rng.standard_t(4, size=(60, 3)) * 0.8 + 0.1, seed=46, n_iters=12,
                n_projections=7, p=1)
    case_sliced("sliced_p2_equal", rng.normal(size=(64, 4)), rng.normal(0.2, 1.1, size=(64, 4)), seed=47, n_iters=12,
                n_projections=9, p=2)


if __name__ == "__main__":
    main()
