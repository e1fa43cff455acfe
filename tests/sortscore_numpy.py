"""Float64 numpy restatement of pfm_sort_score and pfm_pinball_grad (probaforms_amd/metrics/csrc/pf_sortscore.hip): per series the
CRPS of K draws against the series' target with its derivatives, and the pinball scores of the draws' empirical quantiles, from the
sorted series; written from the formulas and independent of the package; no GPU.

Per series s, with t_k = X[k, s] - Y[s] sorted by (value, draw index) (np.lexsort), t_(i) the i-th of them, and from np.searchsorted
on the sorted series lo_i = #{t < t_(i)} and hi_i = #{t <= t_(i)} - 1, the first and the last position of the run of t_(i):
    c_i            = lo_i + hi_i - K + 1                       (2 i - K + 1 without ties)
    crps           = (1/K) sum_i |t_(i)| - (1/(K D)) sum_i c_i t_(i),        D = K - 1 if fair else K
    d crps / d x_k = (sgn(t_k) D - c_k) / (K D),    d crps / d y = -(sum_k sgn(t_k)) / K,        sgn(0) = 0
    level p:  h = p (K - 1), i = floor(h) clipped to K - 2 (0 at K = 1), frac = h - i
              Q_p - y = lerp(t_(i), t_(i+1), frac) (numpy's),  side = p - [y < Q_p],  pinball = (y - Q_p) side
              idx = the draws that are t_(i) and t_(i+1)
A series whose sum of |t| is NaN has NaN for every float output; its idx are not defined here (the entries are -1).

value_grad returns beside the outputs the sums of the magnitudes of the value's terms: smag = (1/K) sum |t| + (1/(K D)) sum |c t| for
the CRPS, pmag = |t_(i)| + |t_(i+1)| for a pinball score.  A float64 sum of N correctly rounded terms, taken in any order, is within
N 2^-53 of those sums.  The gradients have no rounding to bound: an integer over an integer, one division.

The second half holds the series the host and the GPU tests feed the code under test."""
import numpy as np

LEVELS = (0.0, 0.05, 0.5, 0.95, 1.0)


def level_parts(levels, K):
    """-> (i [Q] int, frac [Q]): the lower order statistic and the weight of the upper one"""
    p = np.asarray(levels, np.float64).reshape(-1)
    h = p * np.float64(K - 1)
    i = np.clip(np.floor(h), 0, max(K - 2, 0))
    return i.astype(np.int64), h - i


def lerp(a, b, frac):
    """numpy's _lerp: a + (b - a) t; b - (b - a) (1 - t) where t >= 0.5; a where b == a"""
    diff = b - a
    out = a + diff * frac
    out = np.where(frac >= 0.5, b - diff * (1.0 - frac), out)
    return np.where(diff == 0.0, a, out)


def value_grad(X, Y, fair, levels=()):
    """X [K, M], Y [M] (any float dtype, widened) -> dict of arrays: crps, smag, grad_y [M]; grad_x [K, M]; pinball, side, pmag, qt
    (= Q_p - y) [Q, M]; idx [Q, M, 2] int32; c [K, M] (by draw) and order [K, M] (the draws in sorted order)"""
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    K, M = X.shape
    assert Y.shape == (M,) and (K > 1 or not fair)
    D = K - 1 if fair else K
    with np.errstate(all="ignore"):
        T = X - Y[None]
        order = np.lexsort((np.broadcast_to(np.arange(K)[:, None], (K, M)), T), axis=0)            # by (value, draw)
        Ts = np.take_along_axis(T, order, axis=0)
        C = np.empty((K, M), np.int64)
        for s in range(M):
            ts = Ts[:, s]
            C[:, s] = np.searchsorted(ts, ts, "left") + np.searchsorted(ts, ts, "right") - 1 - K + 1
        s1, s2 = np.abs(Ts).sum(axis=0), (C * Ts).sum(axis=0)
        bad = np.isnan(s1)
        crps = (1.0 / K) * s1 - (1.0 / (float(K) * D)) * s2
        smag = (1.0 / K) * s1 + (1.0 / (float(K) * D)) * np.abs(C * Ts).sum(axis=0)
        c_draw = np.empty_like(C)
        np.put_along_axis(c_draw, order, C, axis=0)
        sgn = np.where(np.isnan(T), 0.0, np.sign(T)).astype(np.int64)                           # (a NaN's series is NaN below)
        gx = (sgn * D - c_draw) / (float(K) * D)
        gy = -(sgn.sum(axis=0) / float(K))
        out = {"crps": np.where(bad, np.nan, crps), "smag": smag, "grad_x": np.where(bad[None], np.nan, gx),
               "grad_y": np.where(bad, np.nan, gy), "c": c_draw, "order": order, "bad": bad}
        i0, frac = level_parts(levels, K)
        i1 = np.minimum(i0 + 1, K - 1)
        ta, tb = Ts[i0], Ts[i1]                                                                 # [Q, M]
        qt = lerp(ta, tb, frac[:, None])                                                        # Q_p - y
        p = np.asarray(levels, np.float64).reshape(-1, 1)
        side = np.where(bad[None], np.nan, p - (0.0 < qt))
        out.update(pinball=np.where(bad[None], np.nan, -qt * side), side=side, pmag=np.abs(ta) + np.abs(tb), qt=qt,
                   idx=np.where(bad[None, :, None], -1, np.stack([order[i0], order[i1]], axis=-1)).astype(np.int32))
    return out


def pinball_grad(idx, side, g, levels, K):
    """pfm_pinball_grad: idx [Q, M, 2], side [Q, M], g [Q, M] -> (grad_x [K, M], grad_y [M]), q ascending"""
    Q, M = side.shape
    _, frac = level_parts(levels, K)
    gx, gy = np.zeros((K, M)), np.zeros(M)
    cols = np.arange(M)
    with np.errstate(all="ignore"):
        for q in range(Q):
            w = g[q] * side[q]
            gy = gy + w
            gx[idx[q, :, 0], cols] = gx[idx[q, :, 0], cols] + (-w) * (1.0 - frac[q])
            gx[idx[q, :, 1], cols] = gx[idx[q, :, 1], cols] + (-w) * frac[q]
    return gx, gy


def mean_score(X, Y, fair):
    """the mean CRPS alone, for central differences"""
    return float(value_grad(X, Y, fair)["crps"].mean())


# ---------------------------------------------------------------------------------------------------------------------------
# the series the tests feed
# ---------------------------------------------------------------------------------------------------------------------------

KINDS = ("generic", "all equal", "two values", "long run", "y on a draw", "y below", "y above", "signed zeros", "far centre")
LONG_RUN = 300                     # draws of the long tie run where K >= 1024: longer than a workgroup


def series(K, M, seed=0, first_kind=0):
    """X [K, M], Y [M]: series s is of kind KINDS[(first_kind + s) % len(KINDS)]"""
    rng = np.random.RandomState(100003 * K + 101 * M + seed)
    mu, sigma = rng.normal(size=M) * 2.0, 0.5 + rng.uniform(size=M)
    X = mu[None] + sigma[None] * rng.normal(size=(K, M))
    Y = mu + 0.3 + 0.8 * rng.normal(size=M)
    for s in range(M):
        kind = KINDS[(first_kind + s) % len(KINDS)]
        if kind == "all equal":
            X[:, s] = X[0, s]
        elif kind == "two values":
            X[:, s] = np.where(rng.randint(0, 2, size=K) == 1, mu[s] + 1.0, mu[s] - 0.5)
            Y[s] = mu[s] + (1.0 if s % 2 else 0.25)            # on the upper value, or between the two
        elif kind == "long run":
            run = LONG_RUN if K >= 1024 else K // 2
            X[rng.permutation(K)[:run], s] = mu[s] + 0.125
        elif kind == "y on a draw":
            Y[s] = X[K // 2, s]
        elif kind == "y below":
            Y[s] = X[:, s].min() - 1.0
        elif kind == "y above":
            Y[s] = X[:, s].max() + 1.0
        elif kind == "signed zeros":
            X[:, s] -= mu[s]
            at = rng.permutation(K)[:min(K, 4)]
            X[at, s] = np.where(np.arange(len(at)) % 2 == 0, 0.0, -0.0)
            Y[s] = 0.0 if s % 2 else 0.1
        elif kind == "far centre":
            X[:, s] = 1e6 + rng.normal(size=K)
            Y[s] = 1e6 + 0.3
    return X, Y


def integer_series(K, M, seed=0):
    """small integer draws and targets (ties everywhere): with fair=False and K a power of two every sum of the restatement and of
    any other order is an integer below 2^53 and every scale a power of two: exact"""
    rng = np.random.RandomState(7 * K + M + seed)
    return rng.randint(-3, 4, size=(K, M)).astype(np.float64), rng.randint(-3, 4, size=M).astype(np.float64)


def separated_series(K, M, seed=0, levels=()):
    """draws and targets of a series at least 0.1 apart from each other, and y at least 0.3 from every quantile asked for: central
    differences and gradcheck stay on one smooth piece"""
    rng = np.random.RandomState(31 * K + M + seed)
    X, Y = np.empty((K, M)), np.empty(M)
    for s in range(M):
        grid = rng.permutation(4 * K + 8)[:K + 1] * 0.25 + rng.uniform(0.0, 0.1, size=K + 1)    # cells of 0.25, jitter below 0.1
        X[:, s], y = grid[:K] - K / 2.0, grid[K] - K / 2.0
        if len(levels):
            q = np.quantile(X[:, s], levels)
            cand = np.concatenate([q - 0.45, q + 0.45, [X[:, s].min() - 1.0, X[:, s].max() + 1.0]])
            good = [c for c in cand if np.abs(c - q).min() >= 0.3 and np.abs(c - X[:, s]).min() >= 0.1]
            y = good[rng.randint(len(good))]
        Y[s] = y
    return X, Y
