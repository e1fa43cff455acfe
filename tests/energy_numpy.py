"""Float64 numpy / scipy restatement of probaforms_amd.metrics.energy: every bootstrap resample is made explicitly with the
reference's stream (tests/wasserstein_numpy.draw), then
  sums      the three raw pair sums Srr, Sff, Srf of scipy.spatial.distance.cdist's Euclidean distances of the GATHERED rows;
  by_counts the same three as quadratic forms c D c over the ORIGINAL rows with the replicate's draw counts c (what the
            kernel computes, in another order);
  values    exx, eyy, exy = the sums over nr^2, nf^2, nr nf; D^2 = (2 exy - exx) - eyy; D = sqrt(max(D^2, 0)).
The yardstick the energy tests hold the GPU kernels and the committed fixtures against.  Test helper, not product code.
"""
import numpy as np
from scipy.spatial.distance import cdist

from probaforms_amd.metrics import _boot, _lib
from wasserstein_numpy import draw, standardize  # noqa: F401

TILE, REP_BLOCK = _lib.ENERGY_TILE, _lib.ENERGY_REP_BLOCK


def sums(X, Y, ix, iy):
    """-> [3] Srr, Sff, Srf of the resampled sets X[ix], Y[iy]: all ordered pairs, the zero diagonals included"""
    R, F = X[ix], Y[iy]
    return np.array([cdist(R, R).sum(), cdist(F, F).sum(), cdist(R, F).sum()])


def by_counts(X, Y, ix, iy):
    """the same three sums from the original rows' distances and the draw counts"""
    cx = np.bincount(ix, minlength=len(X)).astype(np.float64)
    cy = np.bincount(iy, minlength=len(Y)).astype(np.float64)
    return np.array([cx @ cdist(X, X) @ cx, cy @ cdist(Y, Y) @ cy, cx @ cdist(X, Y) @ cy])


def means(S, nr, nf):
    """[..., 3] raw sums -> exx, eyy, exy"""
    return np.asarray(S, np.float64) / np.array([nr * nr, nf * nf, nr * nf], dtype=np.float64)


def from_means(E, squared):
    E = np.asarray(E, np.float64).reshape(-1, 3)
    d2 = (2.0 * E[:, 2] - E[:, 0]) - E[:, 1]
    return d2 if squared else np.sqrt(np.maximum(d2, 0.0))


def values(S, nr, nf, squared):
    """[n, 3] raw sums -> [n] D^2 or D"""
    return from_means(means(np.asarray(S, np.float64).reshape(-1, 3), nr, nf), squared)


def replicates(X, Y, n_iters, counts=False):
    """-> dict: sums [n_iters, 3], the drawn indices ix / iy of every replicate and the generator's next random()"""
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    out = dict(sums=np.empty((n_iters, 3)), ix=[], iy=[])
    for r in range(n_iters):
        ix, iy = draw(len(X), len(Y))
        out["sums"][r] = (by_counts if counts else sums)(X, Y, ix, iy)
        out["ix"].append(ix)
        out["iy"].append(iy)
    out["next"] = np.random.random()
    return out


def full_sample(X, Y):
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    return sums(X, Y, np.arange(len(X)), np.arange(len(Y)))


def mean_std(S, nr, nf, squared=False):
    V = values(S, nr, nf, squared)
    return V.mean(axis=0), V.std(axis=0)


# ---- the shapes the host and GPU tests share: (rows real, rows fake, features, n_iters) -------------------------------

SEED = 77             # np.random.seed before every case's draws
N_ITERS = 3
ROW_CASES = [(1, 2, 3, N_ITERS), (2, 1, 3, N_ITERS), (TILE - 1, TILE + 1, 3, N_ITERS), (TILE, TILE, 3, N_ITERS),
             (TILE + 1, 2 * TILE + 1, 3, N_ITERS), (257, 256, 3, N_ITERS)]
FEATURE_CASES = [(100, 153, d, N_ITERS) for d in (1, 16, 17, 33)]
REP_CASES = [(65, 63, 2, n) for n in (1, REP_BLOCK - 1, REP_BLOCK, REP_BLOCK + 1)]
GROUPS_CASE = (40, 35, 3, _boot.MAX_GROUP + 2)          # two index groups: 128 + 2 replicates
MANY_TILES_CASE = (1200, 1000, 3, N_ITERS)              # 19 and 16 tiles per side: lists of several tiles, many workgroups
CASES = ROW_CASES + FEATURE_CASES + REP_CASES + [GROUPS_CASE, MANY_TILES_CASE]
INTEGER_CASE = (65, 63, 1, 5)
# the other shapes of tests/test_energy_gpu.py (independence, hygiene, inputs, standardize, a sample against itself)
OTHER_CASES = [(2 * TILE + 2, TILE + 36, 3, 4), (50, 51, 3, 4), (3, 2, 2, 4), (257, 130, 17, 4), (200, 150, 2, 4),
               (100, 153, 2, 4), (TILE + 37, TILE + 37, 4, 2), (1200, 1000, 3, 2)]


def data(nr, nf, d, n_iters=None):
    """continuous data: standard normal real rows, normal(0.3, 1.2) fake rows"""
    rng = np.random.default_rng(1000 * nr + nf + 7 * d)
    return rng.normal(size=(nr, d)), rng.normal(0.3, 1.2, size=(nf, d))


def integer_data(nr, nf, d=1, n_iters=None):
    """integers within +-1000: every distance at d = 1 is an integer and every sum of them is exact in float64"""
    rng = np.random.default_rng(31)
    return (rng.integers(-1000, 1001, size=(nr, d)).astype(np.float64),
            rng.integers(-900, 1101, size=(nf, d)).astype(np.float64))
