#!/usr/bin/env python3
"""Generate tests/golden/energy_*.npz: the bootstrapped and full-sample energy distance (Szekely & Rizzo, V-statistic) computed
with scipy.spatial.distance.cdist's Euclidean distances of the resampled rows.  The reference has no such metric, so nothing
here comes from it.  Needs numpy and scipy only:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_energy.py

The bootstrap is the one of the reference's metrics: per iteration sklearn.utils.resample(X), then resample(Y), which on
numpy's global legacy generator is randint(0, n, size=n).

Per case the file holds X, Y, seed, n_iters, standardize (whether the sums are those of the samples scaled by the real sample's
StandardScaler) and
  sums       [n_iters, 3]: the raw pair sums Srr, Sff, Srf of every replicate, all ordered pairs, zero diagonals included
  d2         [n_iters]: D^2 = (2 exy - exx) - eyy with exx = Srr / nr^2, eyy = Sff / nf^2, exy = Srf / (nr nf)
  mean, std  of D = sqrt(max(D^2, 0)) over the replicates
  full_sums  [3]: the same sums on the samples as given (no resampling)
  next       the next np.random.random() after the call's draws
The continuous samples are rounded to multiples of 1/64 so that the files stay small; their distances are irrational all the
same.
"""
import os

import numpy as np
from scipy.spatial.distance import cdist

HERE = os.path.dirname(os.path.abspath(__file__))


def pair_sums(R, F):
    return np.array([cdist(R, R).sum(), cdist(F, F).sum(), cdist(R, F).sum()])


def d2_of(S, nr, nf):
    E = S / np.array([nr * nr, nf * nf, nr * nf], dtype=np.float64)
    return (2.0 * E[..., 2] - E[..., 0]) - E[..., 1]


def scaled(X, Y):
    mu, sd = X.mean(axis=0), X.std(axis=0)
    sd = np.where(sd == 0, 1.0, sd)
    return (X - mu) / sd, (Y - mu) / sd


def case(X, Y, seed, n_iters, standardize=False):
    Xs, Ys = scaled(X, Y) if standardize else (X, Y)
    np.random.seed(seed)
    S = np.empty((n_iters, 3))
    for r in range(n_iters):
        ix = np.random.randint(0, len(X), size=len(X))
        iy = np.random.randint(0, len(Y), size=len(Y))
        S[r] = pair_sums(Xs[ix], Ys[iy])
    nxt = np.random.random()
    d2 = d2_of(S, len(X), len(Y))
    D = np.sqrt(np.maximum(d2, 0.0))
    return dict(X=X, Y=Y, seed=seed, n_iters=n_iters, standardize=standardize, sums=S, d2=d2, mean=D.mean(axis=0),
                std=D.std(axis=0), full_sums=pair_sums(Xs, Ys), next=nxt)


def grid(A):
    return np.round(A * 64) / 64


def cases():
    """-> {name: the file's arrays}"""
    rng = np.random.default_rng(1717)
    out = {}
    out["normal_100_153_d16"] = case(grid(rng.normal(size=(100, 16))), grid(rng.normal(0.2, 1.1, size=(153, 16))), seed=61,
                                     n_iters=10)
    X = grid(rng.normal(size=(64, 4)))
    out["self_64_d4"] = case(X, X.copy(), seed=62, n_iters=8)                # D^2 of the full samples is exactly 0
    out["integer_65_63_d1"] = case(rng.integers(-1000, 1001, size=(65, 1)).astype(np.float64),
                                   rng.integers(-900, 1101, size=(63, 1)).astype(np.float64), seed=63, n_iters=10)
    out["tiny_1_2_d1"] = case(np.array([[0.25]]), np.array([[-1.5], [2.0]]), seed=64, n_iters=6)
    real = np.concatenate([rng.normal(-4, 1, size=(60, 3)), rng.normal(4, 1, size=(60, 3))]) * [5.0, 0.1, 1.0] + [100.0, 0, -7]
    fake = np.concatenate([rng.normal(-3, 1, size=(50, 3)), rng.normal(5, 1, size=(50, 3))]) * [5.0, 0.1, 1.0] + [100.0, 0, -7]
    out["clusters_standardized"] = case(grid(real), grid(fake), seed=65, n_iters=8, standardize=True)
    return out


def main():
    for name, arrays in cases().items():
        path = os.path.join(HERE, "energy_%s.npz" % name)
        np.savez_compressed(path, **arrays)
        print(name, arrays["X"].shape, arrays["Y"].shape, "D", arrays["mean"], arrays["std"], os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
