"""Float64 numpy restatement of probaforms_amd.metrics.wasserstein without scipy: every bootstrap resample is made
explicitly with the reference's stream and sorted, then
  W_1      by the cdf formula: sum |F_x - F_y| (z_{k+1} - z_k) over the sorted pooled resample z;
  W_p^p    on the integer grid of nx ny cells: sorted x_i covers [i ny, (i + 1) ny), sorted y_j covers [j nx, (j + 1) nx);
           over the sorted union of the breakpoints, sum (cell count) |x_i - y_j|^p / (nx ny);
  the projection by the feature-order loop acc = acc + X[:, j] * theta[j].
The yardstick the Wasserstein tests hold the GPU kernels and the committed fixtures against.  Test helper, not product code.
"""
import numpy as np


def w1(x, y):
    xs, ys = np.sort(x), np.sort(y)
    z = np.sort(np.concatenate([x, y]))
    fx = np.searchsorted(xs, z[:-1], side="right") / len(x)
    fy = np.searchsorted(ys, z[:-1], side="right") / len(y)
    return np.sum(np.abs(fx - fy) * np.diff(z))


def wp_pow(x, y, p):
    """W_p^p, p = 1 or 2 (identity or a square, never pow)"""
    xs, ys = np.sort(x), np.sort(y)
    nx, ny = len(x), len(y)
    right = np.union1d(np.arange(1, nx + 1, dtype=np.int64) * ny, np.arange(1, ny + 1, dtype=np.int64) * nx)
    left = np.concatenate([[0], right[:-1]])
    dv = np.abs(xs[left // ny] - ys[left // nx])
    return np.sum((right - left) * (dv if p == 1 else dv * dv)) / (float(nx) * float(ny))


def distance(x, y, p):
    """W_p of two 1-D samples"""
    return w1(x, y) if p == 1 else np.sqrt(wp_pow(x, y, p))


def sorted_pair_w2(x, y):
    """W_2 of two samples of one size: sqrt(mean((sort x - sort y)^2))"""
    assert len(x) == len(y)
    return np.sqrt(np.mean((np.sort(x) - np.sort(y)) ** 2))


def draw(nx, ny):
    """one iteration of the reference's stream: X's indices, then Y's"""
    return np.random.randint(0, nx, size=nx), np.random.randint(0, ny, size=ny)


def replicates_1d(X, Y, n_iters, p=1):
    """-> ([n_iters, d] W_p per replicate and feature, the generator's next random())"""
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    S = np.empty((n_iters, X.shape[1]))
    for r in range(n_iters):
        ix, iy = draw(len(X), len(Y))
        for f in range(X.shape[1]):
            S[r, f] = distance(X[ix, f], Y[iy, f], p)
    return S, np.random.random()


def directions(n_projections, d):
    th = np.random.normal(size=(n_projections, d))
    return th / np.sqrt((th * th).sum(axis=1))[:, None]


def project(X, th):
    """X @ th summed over the features in order, the product and the sum rounded separately"""
    acc = np.zeros(len(X))
    for j in range(X.shape[1]):
        acc = acc + X[:, j] * th[j]
    return acc


def standardize(X, Y):
    mu, sd = X.mean(axis=0), X.std(axis=0)
    sd = np.where(sd == 0, 1.0, sd)
    return (X - mu) / sd, (Y - mu) / sd


def replicates_sliced(X, Y, n_iters, n_projections=64, p=2, standardize_=False):
    """-> ([n_iters] sliced W_p per replicate, the generator's next random()); the directions are drawn first"""
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    th = directions(n_projections, X.shape[1])
    if standardize_:
        X, Y = standardize(X, Y)
    PX = np.stack([project(X, t) for t in th])
    PY = np.stack([project(Y, t) for t in th])
    S = np.empty((n_iters, n_projections))
    for r in range(n_iters):
        ix, iy = draw(len(X), len(Y))
        for k in range(n_projections):
            S[r, k] = wp_pow(PX[k, ix], PY[k, iy], p)
    S = S.mean(axis=1)
    return (S if p == 1 else np.sqrt(S)), np.random.random()


def feature_average(S):
    score = np.zeros(S.shape[0])
    for f in range(S.shape[1]):
        score = score + S[:, f] / S.shape[1]
    return score.mean(axis=0), score.std(axis=0)
