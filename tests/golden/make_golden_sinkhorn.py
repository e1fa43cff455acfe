#!/usr/bin/env python3
"""Generate tests/golden/sinkhorn_*.npz: the debiased Sinkhorn divergence (Genevay et al. 2018; Feydy et al. 2019) of
resampled sets by the symmetrised Jacobi iteration that pf_metrics.h states for pfm_sinkhorn, computed with scipy's cdist and
logsumexp.  The reference has no such metric, so nothing here comes from it.  Needs numpy and scipy only:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_sinkhorn.py

Per case the file holds the inputs X, Y, the bootstrap indices ix [reps, nr] and iy [reps, nf] (randint(0, n, size=n) per
replicate from numpy's global legacy generator seeded with `seed`, X's first), p, eps, n_sinkhorn and
  value       [reps]: sum_i a_i (f_i - u_i) + sum_j b_j (g_j - v_j) after n_sinkhorn averaged steps and one plain step
  drift       [reps]: the largest |change| of a potential of a drawn row in the last averaged step
  potentials  [reps, 2, nr + nf]: (f, g) and (u, v) on the ORIGINAL pooled rows after the last step, rows that the replicate
              does not draw included
The columns of every softmin are the gathered rows with weights 1 / n.  The samples are rounded to multiples of 1/64 so that the
files stay small.
"""
import os

import numpy as np
from scipy.spatial.distance import cdist
from scipy.special import logsumexp

HERE = os.path.dirname(os.path.abspath(__file__))


def costs(A, B, p):
    return cdist(A, B) if p == 1 else cdist(A, B, "sqeuclidean")


def sm(h, C, eps):
    return -eps * logsumexp((h[None, :] - C) / eps, axis=1, b=np.full((1, C.shape[1]), 1.0 / C.shape[1]))


def one(X, Y, ix, iy, p, eps, n_sinkhorn):
    nr, nf = len(X), len(Y)
    C = dict(f=costs(X, Y[iy], p), g=costs(Y, X[ix], p), u=costs(X, X[ix], p), v=costs(Y, Y[iy], p))
    col = dict(f=("g", iy), g=("f", ix), u=("u", ix), v=("v", iy))       # whose potential the columns of a softmin carry
    drawn = dict(f=np.unique(ix), g=np.unique(iy), u=np.unique(ix), v=np.unique(iy))
    h = dict(f=np.zeros(nr), g=np.zeros(nf), u=np.zeros(nr), v=np.zeros(nf))
    drift = 0.0
    for _ in range(n_sinkhorn):
        new = {k: 0.5 * (h[k] + sm(h[col[k][0]][col[k][1]], C[k], eps)) for k in h}
        drift = max(np.abs(new[k] - h[k])[drawn[k]].max() for k in h)
        h = new
    h = {k: sm(h[col[k][0]][col[k][1]], C[k], eps) for k in h}
    value = (h["f"] - h["u"])[ix].mean() + (h["g"] - h["v"])[iy].mean()
    return value, drift, np.stack([np.concatenate([h["f"], h["g"]]), np.concatenate([h["u"], h["v"]])])


def case(X, Y, seed, reps, p, n_sinkhorn, eps=None, reg=0.1, same=False):
    np.random.seed(seed)
    ix = np.empty((reps, len(X)), np.int64)
    iy = np.empty((reps, len(Y)), np.int64)
    for r in range(reps):
        ix[r] = np.random.randint(0, len(X), size=len(X))
        iy[r] = np.random.randint(0, len(Y), size=len(Y))
    if same:
        iy = ix.copy()
    if eps is None:
        Z = np.concatenate([X, Y])
        eps = reg * np.median(cdist(Z, Z)) ** p
    outs = [one(X, Y, ix[r], iy[r], p, eps, n_sinkhorn) for r in range(reps)]
    return dict(X=X, Y=Y, seed=seed, ix=ix.astype(np.int32), iy=iy.astype(np.int32), p=p, eps=np.float64(eps),
                n_sinkhorn=n_sinkhorn, value=np.array([o[0] for o in outs]), drift=np.array([o[1] for o in outs]),
                potentials=np.stack([o[2] for o in outs]))


def grid(A):
    return np.round(A * 64) / 64


def cases():
    """-> {name: the file's arrays}"""
    rng = np.random.default_rng(2020)
    out = {}
    out["normal_40_35_d3_p2"] = case(grid(rng.normal(size=(40, 3))), grid(rng.normal(0.3, 1.2, size=(35, 3))), seed=71, reps=3,
                                     p=2, n_sinkhorn=100)
    out["normal_65_63_d16_p1"] = case(grid(rng.normal(size=(65, 16))), grid(rng.normal(0.2, 1.1, size=(63, 16))), seed=72,
                                      reps=2, p=1, n_sinkhorn=7)
    X = grid(rng.normal(size=(30, 2)))
    out["self_30_d2_p2"] = case(X, X.copy(), seed=73, reps=2, p=2, n_sinkhorn=20, same=True)     # the value is 0
    X, Y = grid(rng.normal(size=(20, 2))), grid(rng.normal(size=(20, 2)))
    X[7] = [1000.0, 0.0]                                        # a far outlier: an unshifted sum would underflow to log 0
    out["outlier_20_20_d2_p1"] = case(X, Y, seed=74, reps=2, p=1, n_sinkhorn=7, eps=1e-2)
    out["tiny_1_2_d1_p2"] = case(np.array([[0.25]]), np.array([[-1.5], [2.5]]), seed=75, reps=3, p=2, n_sinkhorn=5)
    return out


def main():
    for name, arrays in cases().items():
        path = os.path.join(HERE, "sinkhorn_%s.npz" % name)
        np.savez_compressed(path, **arrays)
        print(name, arrays["X"].shape, arrays["Y"].shape, "eps", arrays["eps"], "value", arrays["value"], "drift",
              arrays["drift"], os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
