"""Float64 numpy restatement of one bootstrap replicate's 1-D statistics (probaforms/metrics/ks1d.py, div1d.py) in the
tie-group form the kernels compute, without scipy or sklearn: the yardstick the 1-D metric tests hold the GPU
kernels and the committed fixtures against.  Test helper, not product code.

For resampled columns x (real) and y (fake), the pooled distinct values v_g in ascending order carry l_g pooled
rows, a_g real ones; C_g and Cr_g count the pooled and real rows below v_g.  Every rank statistic is a sum over g.
"""
import math

import numpy as np


def groups(x, y):
    """-> (v, l, a, C, Cr) over the distinct pooled values, int64 counts"""
    vals, inv = np.unique(np.concatenate([x, y]), return_inverse=True)
    l = np.bincount(inv, minlength=len(vals)).astype(np.int64)
    a = np.bincount(inv[:len(x)], minlength=len(vals)).astype(np.int64)
    return vals, l, a, np.cumsum(l) - l, np.cumsum(a) - a


def ks_raw(x, y):
    """the largest cdf difference at the pooled values, before ks_2samp's h / lcm step: what the kernel returns"""
    nx, ny = len(x), len(y)
    _, l, a, C, Cr = groups(x, y)
    diff = (Cr + a) / nx - ((C + l) - (Cr + a)) / ny
    minS = np.clip(-np.min(diff), 0, 1)
    maxS = np.max(diff)
    return minS if minS > maxS else maxS


def ks(x, y):
    """ks_2samp's statistic: ks_raw; scipy's exact method (both samples of at most 10 000 rows) then returns it as the
    fraction h / lcm(nx, ny), h = round(d * lcm)"""
    nx, ny = len(x), len(y)
    d = ks_raw(x, y)
    if max(nx, ny) > 10000:
        return d
    lcm = (nx // math.gcd(nx, ny)) * ny
    return int(np.round(d * lcm)) * 1.0 / lcm


def cvm_sums(x, y):
    """sum_i (2 R_i - 2 i)^2 over the sorted x (real) and the sorted y, R the pooled midrank: exact integers"""
    _, l, a, C, Cr = groups(x, y)
    out = []
    for cnt, below in ((a, Cr), (l - a, C - Cr)):
        s = 0
        for L, A, Cb, Bb in zip(l.tolist(), cnt.tolist(), C.tolist(), below.tolist()):
            B = 2 * Cb + L + 1 - 2 * Bb
            s += A * B * B - 2 * B * A * (A + 1) + 4 * (A * (A + 1) * (2 * A + 1) // 6)
        out.append(s)
    return out


def cvm(x, y):
    """cramervonmises_2samp's statistic (NaN, as scipy 1.15 returns it, for a sample of fewer than 2 rows)"""
    nx, ny = len(x), len(y)
    if nx < 2 or ny < 2:
        return np.nan
    sx, sy = cvm_sums(x, y)
    u = nx * np.float64(sx / 4)
    u += ny * np.float64(sy / 4)
    k, N = nx * ny, nx + ny
    return u / (k * N) - (4 * k - 1) / (6 * N)


def auc_u2(x, y):
    """2 U, U the Mann-Whitney statistic of the fake rows (a tie counts 1/2): an exact integer"""
    _, l, a, C, Cr = groups(x, y)
    return int(np.sum((l - a) * (2 * Cr + a)))


def auc(x, y):
    """|roc_auc_score([0] * nx + [1] * ny, [x; y]) - 0.5| + 0.5 = |U / (nx ny) - 0.5| + 0.5"""
    u2 = auc_u2(x, y)
    v = (u2 / 2.0) / (len(x) * len(y))
    return abs(v - 0.5) + 0.5


def ad_sums(x, y):
    """-> (sum_r, sum_f, distinct): scipy's _anderson_ksamp_midrank `inner` summed over the distinct pooled values for
    the real and for the fake sample, in scipy's per-value operation order, and the number of distinct values (with a
    single one `inner` is 0 / 0)"""
    _, l, a, C, Cr = groups(x, y)
    n = np.array([len(x), len(y)])
    N = int(n.sum())
    lj = l.astype(np.float64)
    Bj = C + lj / 2.
    sums = []
    for i, (cnt, below) in enumerate(((a, Cr), (l - a, C - Cr))):
        Mij = (below + cnt).astype(float)
        Mij -= cnt / 2.
        with np.errstate(invalid="ignore", divide="ignore"):
            inner = lj / float(N) * (N * Mij - Bj * n[i]) ** 2 / (Bj * (N - Bj) - N * l / 4.)
        sums.append(inner.sum())
    return sums[0], sums[1], len(l)


def ad(x, y):
    """anderson_ksamp([x, y]).statistic, midrank, in scipy's per-value operation order"""
    sr, sf, distinct = ad_sums(x, y)
    if distinct < 2:
        raise ValueError("one distinct value")
    n = np.array([len(x), len(y)])
    N = int(n.sum())
    A2akN = 0.
    A2akN += sr / n[0]
    A2akN += sf / n[1]
    A2akN *= (N - 1.) / N
    k = 2
    H = (1. / n).sum()
    hs_cs = (1. / np.arange(N - 1, 1, -1)).cumsum()
    h = hs_cs[-1] + 1
    g = (hs_cs / np.arange(2, N)).sum()
    a_ = (4 * g - 6) * (k - 1) + (10 - 6 * g) * H
    b_ = (2 * g - 4) * k ** 2 + 8 * h * k + (2 * g - 14 * h - 4) * H - 8 * h + 4 * g - 6
    c_ = (6 * h + 2 * g - 2) * k ** 2 + (4 * h - 4 * g + 6) * k + (2 * h - 6) * H + 4 * h
    d_ = (2 * h + 6) * k ** 2 - 4 * h * k
    sigmasq = (a_ * N ** 3 + b_ * N ** 2 + c_ * N + d_) / ((N - 1.) * (N - 2.) * (N - 3.))
    return (A2akN - (k - 1)) / math.sqrt(sigmasq)


def kl_divergence(p, q):
    return np.sum(p * np.log(p / q))


def js_divergence(p, q):
    m = 0.5 * (p + q)
    return 0.5 * kl_divergence(p, m) + 0.5 * kl_divergence(q, m)


def hist_counts(x, y, bins):
    """np.histogram counts of x and y in the bins of np.histogram([x; y], bins), from the groups: the edges are
    numpy's linspace, a value's bin the last edge <= it (the last bin closed)"""
    v, l, a, _, _ = groups(x, y)
    lo, hi = v[0], v[-1]
    if lo == hi:
        lo, hi = lo - 0.5, hi + 0.5
    e = np.linspace(lo, hi, bins + 1)
    k = np.minimum(np.searchsorted(e, v, side="right") - 1, bins - 1)
    return np.bincount(k, weights=a, minlength=bins).astype(np.int64), \
        np.bincount(k, weights=l - a, minlength=bins).astype(np.int64)


def hist_div(x, y, bins, js):
    hx, hy = hist_counts(x, y, bins)
    with np.errstate(divide="ignore", invalid="ignore"):
        p, q = hx / hx.sum(), hy / hy.sum()
        eps = 10 ** -5 / bins
        return (js_divergence if js else kl_divergence)(p + eps, q + eps)


def kde_logsum(s, grid, h):
    """log sum_i exp(-0.5 (grid_k - s_i)^2 / h^2) per grid point, shifted by its largest term: what the kernel returns"""
    t = -0.5 * (grid[:, None] - s[None, :]) ** 2 / (h * h)
    m = t.max(axis=1)
    return m + np.log(np.exp(t - m[:, None]).sum(axis=1))


def kde_probs(s, grid):
    """exp(KernelDensity(bandwidth='silverman').fit(s).score_samples(grid)) normalised: kde_logsum plus the Gaussian
    norm, minus log n"""
    n = len(s)
    h = (n * 3 / 4) ** (-1 / 5)
    lse = kde_logsum(s, grid, h)
    with np.errstate(divide="ignore", invalid="ignore", under="ignore"):
        p = np.exp(lse + (-0.5 * math.log(2 * math.pi) - math.log(h)) - np.log(n))
        return p / p.sum()


def kde_div(x, y, bins, js):
    z = np.concatenate([x, y])
    grid = np.linspace(z.min(), z.max(), bins)
    with np.errstate(divide="ignore", invalid="ignore"):
        p, q = kde_probs(x, grid), kde_probs(y, grid)
        eps = 10 ** -5 / bins
        return (js_divergence if js else kl_divergence)(p + eps, q + eps)


FUNCS = {   # public name -> (x, y, bins) -> statistic
    "kolmogorov_smirnov_1d": lambda x, y, b: ks(x, y),
    "cramer_von_mises_1d": lambda x, y, b: cvm(x, y),
    "roc_auc_score_1d": lambda x, y, b: auc(x, y),
    "anderson_darling_1d": lambda x, y, b: ad(x, y),
    "kullback_leibler_1d": lambda x, y, b: hist_div(x, y, b, False),
    "jensen_shannon_1d": lambda x, y, b: hist_div(x, y, b, True),
    "kullback_leibler_1d_kde": lambda x, y, b: kde_div(x, y, b, False),
    "jensen_shannon_1d_kde": lambda x, y, b: kde_div(x, y, b, True),
}
BINS = {"kullback_leibler_1d": "bins_hist", "jensen_shannon_1d": "bins_hist", "kullback_leibler_1d_kde": "bins_kde",
        "jensen_shannon_1d_kde": "bins_kde"}


def replicates(name, X, Y, n_iters, bins=None):
    """[n_iters, d] per-replicate, per-feature statistics on the reference's draws from numpy's global generator"""
    out = np.empty((n_iters, X.shape[1]))
    for r in range(n_iters):
        ix = np.random.randint(0, len(X), size=len(X))
        iy = np.random.randint(0, len(Y), size=len(Y))
        for f in range(X.shape[1]):
            out[r, f] = FUNCS[name](X[ix, f], Y[iy, f], bins)
    return out


def feature_average(S):
    score = np.zeros(S.shape[0])
    for f in range(S.shape[1]):
        score = score + S[:, f] / S.shape[1]
    return score.mean(axis=0), score.std(axis=0)
