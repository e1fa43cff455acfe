#!/usr/bin/env python3
"""Generate tests/golden/metrics_*.npz by running the REFERENCE's probaforms.metrics (hse-cs/probaforms).

Run it where a checkout of the reference and its CPU dependencies (sklearn, scipy) are at hand:

    PYTHONPATH=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_metrics.py

Per case and metric the file holds the inputs, the numpy seed, n_iters, standardize, the reference's
(mean, std), the per-replicate values (and for MMD the per-replicate median distance) from replaying the
reference's loop -- sklearn.utils.resample of X then Y, then the replicate's formula -- under the same
seed, and the next np.random.random() after the reference's call (where its generator stands).  The
replay is checked to reproduce the reference's (mean, std) exactly.  A case where the reference raises
records that (`mmd_raises`), and the replay's medians show which replicate has a median of 0.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))

from probaforms import metrics as ref  # the reference  # noqa: E402
from probaforms.models import RealNVP  # noqa: E402
from scipy.linalg import sqrtm  # noqa: E402
from sklearn.metrics import pairwise_distances  # noqa: E402
from sklearn.preprocessing import StandardScaler  # noqa: E402
from sklearn.utils import resample  # noqa: E402

assert not getattr(sys.modules["probaforms"], "__probaforms_amd__", False), "must import the reference"
torch.set_num_threads(1)


def replay_mmd(X, Y, seed, n_iters, standardize):
    if standardize:
        s = StandardScaler().fit(X)
        X, Y = s.transform(X), s.transform(Y)
    np.random.seed(seed)
    meds, vals = [], []
    for _ in range(n_iters):
        Xb, Yb = resample(X), resample(Y)
        meds.append(np.median(pairwise_distances(np.concatenate((Xb, Yb), axis=0))))
        vals.append(ref.mmd.mmd_calc(Xb, Yb) if meds[-1] > 0 else np.nan)
    return np.array(meds), np.array(vals)


def replay_fd(X, Y, seed, n_iters, standardize):
    if standardize:
        s = StandardScaler().fit(X)
        X, Y = s.transform(X), s.transform(Y)
    np.random.seed(seed)
    vals = []
    for _ in range(n_iters):
        Xb, Yb = resample(X), resample(Y)
        cr = np.atleast_2d(np.cov(Xb, rowvar=False))
        cf = np.atleast_2d(np.cov(Yb, rowvar=False))
        diff = np.sum((Xb.mean(axis=0) - Yb.mean(axis=0)) ** 2.0)
        tr = np.trace(sqrtm(cr.dot(cf), disp=False)[0].real)
        vals.append(diff + np.trace(cr) + np.trace(cf) - 2 * tr)
    return np.array(vals)


def case(name, X, Y, seed, n_iters, standardize=False, fd=True):
    out = dict(X=X, Y=Y, seed=seed, n_iters=n_iters, standardize=standardize)
    meds, vals = replay_mmd(X, Y, seed, n_iters, standardize)
    np.random.seed(seed)
    try:
        mu, sd = ref.maximum_mean_discrepancy(X, Y, n_iters=n_iters, standardize=standardize)
        out.update(mmd_raises=False, mmd_mean=mu, mmd_std=sd, mmd_next=np.random.random())
        assert mu == np.mean(vals) and sd == np.std(vals), (name, mu, np.mean(vals))
    except ValueError:
        assert (meds == 0).any(), name
        out.update(mmd_raises=True)
    out.update(mmd_med=meds, mmd_rep=vals)
    if fd:
        vals = replay_fd(X, Y, seed, n_iters, standardize)
        np.random.seed(seed)
        mu, sd = ref.frechet_distance(X, Y, n_iters=n_iters, standardize=standardize)
        out.update(fd_mean=mu, fd_std=sd, fd_next=np.random.random(), fd_rep=vals)
        assert np.isclose(mu, vals.mean(), rtol=1e-12, atol=0) and np.isclose(sd, vals.std(), rtol=1e-9, atol=0), (name,)
    np.savez_compressed(os.path.join(HERE, "metrics_%s.npz" % name), **out)
    print(name, X.shape, Y.shape, "mmd", out.get("mmd_mean", "raises"), "fd", out.get("fd_mean"))


def two_gaussians(dist, N, rng):
    """the notebook's gen_two_samples (docs/examples/metrics.ipynb), on a seeded generator"""
    sigma = np.array([[1, 0.7], [0.7, 1]])
    mu_x = np.array([0, 0])
    return rng.multivariate_normal(mu_x, sigma, N), rng.multivariate_normal(mu_x + dist / np.sqrt(2), sigma, N)


def c2_sample(n, rng):
    """a real d = 16 sample and the sample of a C2-shaped RealNVP (L = 8, hidden (128,), c = 4) trained on it"""
    A = rng.normal(size=(16, 16)) / 4
    C = rng.normal(size=(n, 4))
    X = np.tanh(rng.normal(size=(n, 16)) @ A) + C @ rng.normal(size=(4, 16)) * 0.3
    torch.manual_seed(0)
    m = RealNVP(n_layers=8, hidden=(128,), lr=0.001, n_epochs=3)
    m.fit(X, C)
    return X, np.asarray(m.sample(C), dtype=np.float64)


def main():
    rng = np.random.default_rng(2024)
    sig = np.array([[1, 0.7], [0.7, 1]])
    for dist in (0, 2, 10):
        X, Y = two_gaussians(float(dist), 1000, rng)
        case("nb_dist%d" % dist, X, Y, seed=dist + 1, n_iters=12)
    case("same_1d", rng.normal(0, 1, 100).reshape(-1, 1), rng.normal(1, 1, 100).reshape(-1, 1), seed=11, n_iters=100)
    case("diff_100_153", rng.multivariate_normal([0, 0], sig, 100), rng.multivariate_normal([0, 0], sig, 153),
         seed=12, n_iters=100)
    case("diff_342_100", rng.multivariate_normal([0, 0], sig, 342), rng.multivariate_normal([0, 0], sig, 100),
         seed=13, n_iters=100)
    X, Y = c2_sample(800, rng)
    case("c2_d16", X, Y, seed=14, n_iters=8)
    X = rng.multivariate_normal([3, -1], sig, 300) * np.array([5.0, 0.2])
    Y = rng.multivariate_normal([3.5, -1], sig, 260) * np.array([5.0, 0.2])
    X[:, 1] = np.round(X[:, 1], 1)
    case("standardize", X, Y, seed=15, n_iters=40, standardize=True)
    # tiny samples of mostly equal rows: some replicates' pooled distance matrices are more than half zeros
    X = np.array([[0.0], [0.0], [0.0], [1.0]])
    Y = np.array([[0.0], [0.0], [2.0]])
    case("median0", X, Y, seed=16, n_iters=20, fd=False)


if __name__ == "__main__":
    main()
