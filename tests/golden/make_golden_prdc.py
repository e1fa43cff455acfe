#!/usr/bin/env python3
"""Generate tests/golden/prdc_*.npz: bootstrapped and full-sample k-nearest-neighbour precision, recall, density and coverage
computed with scipy.spatial.distance.cdist(..., 'sqeuclidean') and the four expressions the `prdc` package publishes
(prdc.compute_prdc; the package computes Euclidean distances, here both sides of every comparison are squared, which orders
the same).  Needs numpy and scipy only:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_prdc.py

The bootstrap is the one of the reference's metrics: per iteration sklearn.utils.resample(X), then resample(Y), which on
numpy's global legacy generator is randint(0, n, size=n).

Per case the file holds X, Y, seed, n_iters, k and
  counts  int64 [n_iters, 4]: P, Rc, Dn, Cv of every replicate, counted from the package's boolean matrices
  values  [n_iters, 4]: the package's precision, recall, density, coverage of every replicate
  mean, std   [4] of `values` over the replicates
  rr0, ss0    the squared radii of the first replicate
  full_counts, full_values   the same on the samples as given (no resampling)
  next    the next np.random.random() after the call's draws
"""
import os

import numpy as np
from scipy.spatial.distance import cdist

HERE = os.path.dirname(os.path.abspath(__file__))


def kth_value(unsorted, k):
    """prdc.get_kth_value"""
    indices = np.argpartition(unsorted, k, axis=-1)[..., :k]
    return np.take_along_axis(unsorted, indices, axis=-1).max(axis=-1)


def nn_radii(S, nearest_k):
    """prdc.compute_nearest_neighbour_distances, squared"""
    return kth_value(cdist(S, S, "sqeuclidean"), nearest_k + 1)


def compute_prdc(R, F, nearest_k):
    rr, ss = nn_radii(R, nearest_k), nn_radii(F, nearest_k)
    D = cdist(R, F, "sqeuclidean")
    inside = D < np.expand_dims(rr, axis=1)
    precision = inside.any(axis=0).mean()
    recall = (D < np.expand_dims(ss, axis=0)).any(axis=1).mean()
    density = (1. / float(nearest_k)) * inside.sum(axis=0).mean()
    coverage = (D.min(axis=1) < rr).mean()
    counts = [inside.any(axis=0).sum(), (D < np.expand_dims(ss, axis=0)).any(axis=1).sum(), inside.sum(),
              (D.min(axis=1) < rr).sum()]
    return np.array(counts, np.int64), np.array([precision, recall, density, coverage]), rr, ss


def resample(X):
    return X[np.random.randint(0, len(X), size=len(X))]


def case(name, X, Y, seed, n_iters, k):
    np.random.seed(seed)
    C, V = np.empty((n_iters, 4), np.int64), np.empty((n_iters, 4))
    for r in range(n_iters):
        Xb, Yb = resample(X), resample(Y)
        C[r], V[r], rr, ss = compute_prdc(Xb, Yb, k)
        if r == 0:
            rr0, ss0 = rr, ss
    nxt = np.random.random()
    fc, fv, _, _ = compute_prdc(X, Y, k)
    np.savez_compressed(os.path.join(HERE, "prdc_%s.npz" % name), X=X, Y=Y, seed=seed, n_iters=n_iters, k=k, counts=C,
                        values=V, mean=V.mean(axis=0), std=V.std(axis=0), rr0=rr0, ss0=ss0, full_counts=fc, full_values=fv,
                        next=nxt)
    print(name, X.shape, Y.shape, "k", k, V.mean(axis=0), "full", fv)


def main():
    rng = np.random.default_rng(1616)
    sig = np.array([[1, 0.7], [0.7, 1]])
    case("normal_100_153_k5", rng.multivariate_normal([0, 0], sig, 100), rng.multivariate_normal([0.3, 0], sig * 1.5, 153),
         seed=51, n_iters=12, k=5)
    # a generator collapsed onto one of two modes: high precision, recall near one half
    real = np.concatenate([rng.normal(-4, 1, size=(80, 3)), rng.normal(4, 1, size=(80, 3))])
    case("collapsed_k3", real, rng.normal(4, 1, size=(130, 3)), seed=52, n_iters=10, k=3)
    # an over-dispersed generator: low precision, high recall
    case("dispersed_k1", rng.normal(size=(70, 4)), rng.normal(0, 2.5, size=(90, 4)), seed=53, n_iters=10, k=1)
    # multiples of 1/8: every distance is exact, and exact ties between a cross distance and a radius occur
    X = np.clip(np.round(rng.normal(size=(120, 3)) * 8) / 8, -8, 8)
    Y = np.clip(np.round(rng.normal(0.3, 1.2, size=(90, 3)) * 8) / 8, -8, 8)
    case("dyadic_k5", X, Y, seed=54, n_iters=10, k=5)
    # (the package's argpartition needs nearest_k + 1 < rows, so nearest_k = rows - 2 is its smallest sample)
    case("tiny_k4", rng.normal(size=(6, 2)), rng.normal(0.2, 1, size=(7, 2)), seed=55, n_iters=8, k=4)


if __name__ == "__main__":
    main()
