"""Float64 numpy / scipy restatement of probaforms_amd.metrics.sinkhorn (kernels: pf_sinkhorn.hip): the debiased Sinkhorn
divergence by the symmetrised Jacobi iteration of pf_metrics.h, with scipy.spatial.distance.cdist for the costs and
scipy.special.logsumexp (b= weights) for the softmin.

The COLUMNS of every softmin and the sums of the value are the GATHERED resampled rows X[ix], Y[iy] with uniform weights 1 / n
(the definition); the kernel works on the original rows with weights count / n, so a comparison also checks that formulation.
The ROWS of every softmin are all original rows, so that the potentials of rows that a resample leaves out (count 0), which the
kernel also iterates and writes, can be compared too; a gathered row's potential is that of its original row.
Test helper, not product code.
"""
import numpy as np
from scipy.spatial.distance import cdist
from scipy.special import logsumexp

from probaforms_amd.metrics import _boot, _lib
from wasserstein_numpy import draw, standardize  # noqa: F401

TILE, REP_BLOCK = _lib.ENERGY_TILE, _lib.ENERGY_REP_BLOCK


def cost(A, B, p):
    """|a - b|^p: the Euclidean distance, or its square summed directly (no root squared again)"""
    return cdist(A, B) if p == 1 else cdist(A, B, "sqeuclidean")


def cmax(X, Y, p):
    """the largest cost between two pooled rows: the scale of every tolerance"""
    Z = np.concatenate([X, Y])
    return float(cost(Z, Z, p).max())


def softmin(h, C, eps):
    """-eps log sum_j (1 / n) exp((h_j - C_ij) / eps) over the n columns"""
    n = C.shape[1]
    return -eps * logsumexp((h[None, :] - C) / eps, axis=1, b=np.full((1, n), 1.0 / n))


def solve(X, Y, ix, iy, p, eps, n_sinkhorn):
    """-> dict(value, drift, potentials [2, nr + nf]: (f, g) then (u, v) on the original pooled rows)"""
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    ix, iy = np.asarray(ix), np.asarray(iy)
    nr, nf = len(X), len(Y)
    R, F = X[ix], Y[iy]
    C_RF, C_FR, C_RR, C_FF = cost(X, F, p), cost(Y, R, p), cost(X, R, p), cost(Y, F, p)
    f, g, u, v = np.zeros(nr), np.zeros(nf), np.zeros(nr), np.zeros(nf)

    def softmins():
        return (softmin(g[iy], C_RF, eps), softmin(f[ix], C_FR, eps), softmin(u[ix], C_RR, eps), softmin(v[iy], C_FF, eps))

    drift = 0.0
    drawn_r, drawn_f = np.unique(ix), np.unique(iy)
    for _ in range(n_sinkhorn):
        old = (f, g, u, v)
        f, g, u, v = (0.5 * (h + s) for h, s in zip(old, softmins()))
        drift = max(np.abs(new - h)[rows].max() for new, h, rows in zip((f, g, u, v), old, (drawn_r, drawn_f, drawn_r, drawn_f)))
    f, g, u, v = softmins()
    value = (f - u)[ix].mean() + (g - v)[iy].mean()
    return dict(value=float(value), drift=float(drift), potentials=np.stack([np.concatenate([f, g]), np.concatenate([u, v])]))


def solve_many(X, Y, IX, IY, p, eps, n_sinkhorn):
    """-> dict(value [reps], drift [reps], potentials [reps, 2, nr + nf])"""
    outs = [solve(X, Y, ix, iy, p, eps, n_sinkhorn) for ix, iy in zip(IX, IY)]
    return {k: np.array([o[k] for o in outs]) for k in ("value", "drift", "potentials")}


def median(X, Y):
    """np.median of the pooled distance matrix, the diagonal zeros and both triangles included (pfm_mmd's median)"""
    Z = np.concatenate([np.asarray(X, np.float64), np.asarray(Y, np.float64)])
    return float(np.median(cdist(Z, Z)))


def replicates(X, Y, n_iters, p, eps, n_sinkhorn):
    """the reference's bootstrap stream -> dict: value / drift [n_iters], the indices ix / iy, the generator's next random()"""
    IX, IY = [], []
    for _ in range(n_iters):
        ix, iy = draw(len(X), len(Y))
        IX.append(ix)
        IY.append(iy)
    nxt = np.random.random()
    o = solve_many(X, Y, IX, IY, p, eps, n_sinkhorn)
    o.update(ix=IX, iy=IY, next=nxt)
    return o


def full_sample(X, Y, p, eps, n_sinkhorn):
    return solve(X, Y, np.arange(len(X)), np.arange(len(Y)), p, eps, n_sinkhorn)


def data(nr, nf, d):
    """continuous data: standard normal real rows, normal(0.3, 1.2) fake rows"""
    rng = np.random.default_rng(2000 * nr + nf + 11 * d)
    return rng.normal(size=(nr, d)), rng.normal(0.3, 1.2, size=(nf, d))


def bootstrap(nr, nf, reps, seed):
    """`reps` draws of the reference's stream from a seeded global generator -> int arrays [reps, nr], [reps, nf]"""
    np.random.seed(seed)
    host = np.empty(reps * (nr + nf), np.int32)
    _boot.draw_indices(host, reps, nr, nf)
    return host[:reps * nr].reshape(reps, nr).copy(), host[reps * nr:].reshape(reps, nf).copy()


# ---- the shapes of tests/test_sinkhorn_gpu.py: one sweep per axis around the middle case --------------------------------
# (rows real, rows fake, features, p, n_sinkhorn, replicates)
MIDDLE = (65, 130, 3, 2, 7, 3)
ROW_SHAPES = [(1, 1), (1, 5), (2, 3), (63, 65), (64, 64), (65, 130), (130, 70)]
ROW_CASES = [(nr, nf) + MIDDLE[2:] for nr, nf in ROW_SHAPES]
FEATURE_CASES = [MIDDLE[:2] + (d,) + MIDDLE[3:] for d in (1, 3, 16, 17, 33)]
P_CASES = [MIDDLE[:3] + (p,) + MIDDLE[4:] for p in (1, 2)]
STEP_CASES = [MIDDLE[:4] + (n,) + (2,) for n in (0, 1, 7, 100)]
REP_CASES = [MIDDLE[:5] + (r,) for r in (1, REP_BLOCK - 1, REP_BLOCK, REP_BLOCK + 1)]
CASES = sorted(set(ROW_CASES + FEATURE_CASES + P_CASES + STEP_CASES + REP_CASES))
REG = 0.1             # eps = REG * median^p of the case's data
SEED = 91
