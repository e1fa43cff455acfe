"""Float64 numpy restatement of one bootstrap replicate of each metric, written from the reference's
definitions (probaforms/metrics/mmd.py, fd.py) without sklearn or scipy: the yardstick the metrics tests
hold the GPU kernels and the committed fixtures against.  Test helper, not product code."""
import numpy as np


def pooled_upper_d2(Z, block=2048):
    """squared distances of every pair i < j of the rows of Z (row-major upper triangle), float64"""
    m = Z.shape[0]
    out = []
    for i0 in range(0, m, block):
        A = Z[i0:i0 + block]
        D = np.zeros((A.shape[0], m))
        for k in range(Z.shape[1]):
            df = A[:, k:k + 1] - Z[None, :, k]
            D += df * df
        for r in range(A.shape[0]):
            out.append(D[r, i0 + r + 1:])
    return np.concatenate(out) if out else np.zeros(0)


def median_distance(Z):
    """np.median of the full m x m Euclidean distance matrix: m diagonal zeros, every pair i < j twice"""
    m = Z.shape[0]
    u = pooled_upper_d2(Z)
    M = m * m
    ranks = sorted({(M - 1) // 2, M // 2})

    def at(k):                      # rank k of [0] * m + each u twice (u >= 0, so the zeros lead)
        if k < m:
            return 0.0
        j = (k - m) // 2
        return float(np.sqrt(np.partition(u, j)[j]))
    vals = [at(k) for k in ranks]
    return vals[0] if len(vals) == 1 else (vals[0] + vals[1]) / 2


def mmd_replicate(Xb, Yb, block=2048):
    """-> (median, mmd) of one replicate; mmd is NaN where the median is 0"""
    Z = np.concatenate((Xb, Yb), axis=0)
    med = median_distance(Z)
    if not med > 0:
        return med, np.nan
    gamma = 1.0 / (2 * med ** 2)

    def kmean(A, B):
        s = 0.0
        for i0 in range(0, A.shape[0], block):
            P = A[i0:i0 + block]
            D = np.zeros((P.shape[0], B.shape[0]))
            for k in range(A.shape[1]):
                df = P[:, k:k + 1] - B[None, :, k]
                D += df * df
            s += np.exp(-gamma * D).sum()
        return s / (A.shape[0] * B.shape[0])
    return med, kmean(Xb, Xb) + kmean(Yb, Yb) - 2 * kmean(Xb, Yb)


def boot_indices(nx, ny, n_iters):
    """the reference's draw order on numpy's global generator: per iteration X's indices, then Y's"""
    out = []
    for _ in range(n_iters):
        ix = np.random.randint(0, nx, size=nx)
        iy = np.random.randint(0, ny, size=ny)
        out.append((ix, iy))
    return out
