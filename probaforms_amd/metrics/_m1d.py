"""Host side of the eight 1-D metrics (ks1d.py, div1d.py): argument checks, the per-call sorted order and tie
groups of each pooled feature, the replicate groups of pfm_metric1d, and the reference's finishing arithmetic.

The reference (probaforms/metrics/ks1d.py, _bootstrap_metric) resamples X_real, then X_fake, with
sklearn.utils.resample per iteration, scores every feature with a 1-D two-sample function and averages the
features as `score += mval / n_dim`.  The draws are _boot.replicates'; the kernels return the rank and density
sums of every (replicate, feature) and the scalar expressions of scipy / sklearn / the reference are applied here
in numpy, in the reference's order, so that KS, CvM and the histogram divergences are bitwise the reference's.
"""
import math

import numpy as np
import torch

from . import _boot, _lib


_NO_BINS = object()


# ---- the scalar checks of every metric's arguments (each caller's message names its parameter) ----------------

def is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))


def check_positive_int(v, name):
    if not is_int(v) or v < 1:
        raise ValueError("%s must be a positive integer, got %r" % (name, v))
    return int(v)


def check_bool(v, name):
    if not isinstance(v, (bool, np.bool_)):
        raise ValueError("%s must be a bool, got %r" % (name, v))


def check_positive(v, name, none_ok=False, reciprocal=False):
    """a positive finite int or float (no bool); reciprocal: 1 / v is finite as well; none_ok: or None"""
    if v is None and none_ok:
        return
    ok = isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, (bool, np.bool_))
    if not ok or not (math.isfinite(v) and v > 0 and (not reciprocal or math.isfinite(1.0 / float(v)))):
        raise ValueError("%s must be %sa positive finite number%s, got %r"
                         % (name, "None or " if none_ok else "", " with a finite reciprocal" if reciprocal else "", v))


def check_args(X_real, X_fake, n_iters, bins=_NO_BINS):
    """what is checked before any draw and without a device: shapes, dtypes, finiteness, n_iters, bins (if given)"""
    names = ("X_real", "X_fake")
    shapes = []
    for A, name in zip((X_real, X_fake), names):
        A, shape = _boot._check_2d(A, name)
        finite = bool(torch.isfinite(A).all()) if isinstance(A, torch.Tensor) else bool(np.isfinite(A).all())
        if not finite:
            raise ValueError("%s holds NaN or infinite values" % name)
        shapes.append(shape)
    if shapes[0][1] != shapes[1][1]:
        raise ValueError("X_real and X_fake have different numbers of features: %d and %d" % (shapes[0][1], shapes[1][1]))
    check_positive_int(n_iters, "n_iters")
    if bins is not _NO_BINS:
        check_positive_int(bins, "bins")


class Pooled:
    """the pooled columns of one call on the device: cols [d, N] float64, perm [d, N] (stable ascending order),
    the tie groups of that order as gstart [d, N + 1] and ngroups [d] (int32)"""

    def __init__(self, Xr, Xf):
        self._order(torch.cat([Xr, Xf], dim=0).t().contiguous(), Xr.shape[0])

    @classmethod
    def from_columns(cls, cols, nr):
        """of ready-made pooled columns [d, nr + nf] (the first nr entries of each are the real sample's)"""
        p = cls.__new__(cls)
        p._order(cols.contiguous(), nr)
        return p

    def _order(self, cols, nr):
        self.d, N = cols.shape
        self.nr, self.nf = nr, N - nr
        self.device = cols.device
        self.cols = cols
        vals, perm = torch.sort(self.cols, dim=1, stable=True)
        self.perm = perm.to(torch.int32).contiguous()
        new = torch.ones_like(vals, dtype=torch.bool)
        new[:, 1:] = vals[:, 1:] != vals[:, :-1]
        self.ngroups = new.sum(dim=1, dtype=torch.int32).contiguous()
        gid = new.to(torch.int64).cumsum(dim=1) - 1
        fi, ki = new.nonzero(as_tuple=True)
        self.gstart = torch.full((self.d, N + 1), N, dtype=torch.int32, device=self.device)
        self.gstart[fi, gid[fi, ki]] = ki.to(torch.int32)


OUT_SHAPE = {   # per replicate and feature, the layout of pf_metrics.h
    _lib.M1D_KS: ((), torch.float64), _lib.M1D_CVM: ((2,), torch.int64), _lib.M1D_AD: ((3,), torch.float64),
    _lib.M1D_AUC: ((), torch.int64), _lib.M1D_HIST: ((2, None), torch.int32), _lib.M1D_KDE: ((2, None), torch.float64),
}


def run(metric, X_real, X_fake, n_iters, bins=1, bandwidths=(1.0, 1.0)):
    """-> numpy [n_iters, d, ...]: pfm_metric1d's output for every bootstrap replicate of the public call, drawn
    from numpy's global generator as the reference draws them"""
    Xr, Xf = _boot.prepare(X_real, X_fake, ("X_real", "X_fake"), n_iters)
    with torch.cuda.device(Xr.device):
        p = Pooled(Xr, Xf)
        nr, nf, d = p.nr, p.nf, p.d
        tail, dtype = OUT_SHAPE[metric]
        out = torch.empty((n_iters, d) + tuple(bins if t is None else t for t in tail), dtype=dtype, device=p.device)

        def launch(start, reps, ir, jf, ws):
            _lib.metric1d(metric, p.cols, p.perm, p.gstart, p.ngroups, nr, nf, ir, jf, reps, bins, bandwidths[0],
                          bandwidths[1], out[start:start + reps], ws)

        _boot.replicates(nr, nf, p.device, n_iters, lambda r: _lib.metric1d_workspace_bytes(metric, nr, nf, d, r, bins), launch)
        return out.cpu().numpy()


def feature_average(S):
    """the reference's `score_boot += mval / n_dim` per replicate over the features of S [n_iters, d], in feature
    order (elementwise, so the same roundings as its scalar loop), then (mean, std) of the replicates"""
    n_dim = S.shape[1]
    score = np.zeros(S.shape[0])
    for f in range(n_dim):
        score = score + S[:, f] / n_dim
    return score.mean(axis=0), score.std(axis=0)


# ---- the statistics from the kernels' sums (scipy 1.15 / sklearn 1.7 expressions) -----------------------------

KS_EXACT_MAX_N = 10000    # ks_2samp's method='auto' is 'exact' while max(n1, n2) <= MAX_AUTO_N


def ks_statistic(D, n1, n2):
    """ks_2samp's returned statistic from the cdf difference D: with the exact method (max(n1, n2) <= 10000) scipy
    replaces d by h / lcm(n1, n2), h = int(np.round(d * lcm)) -- the exact fraction, rounded once"""
    if max(n1, n2) > KS_EXACT_MAX_N:
        return D
    g = math.gcd(n1, n2)
    lcm = (n1 // g) * n2
    h = np.round(D * lcm)
    return h * 1.0 / lcm


def cvm_statistic(sums, nx, ny):
    """cramervonmises_2samp's t from sum (2R - 2i)^2 per sample ([..., 2] int64): the reference's float sums of the
    quarter-integers (R - i)^2 are exact, so is sums / 4"""
    ux = sums[..., 0].astype(np.float64) / 4.0
    uy = sums[..., 1].astype(np.float64) / 4.0
    u = nx * ux
    u = u + ny * uy
    k, N = nx * ny, nx + ny
    return u / (k * N) - (4 * k - 1) / (6 * N)


def ad_sigmasq(nr, nf):
    """the normalisation of anderson_ksamp([x, y]): depends only on the sample sizes"""
    k = 2
    n = np.array([nr, nf])
    N = nr + nf
    H = (1. / n).sum()
    hs_cs = (1. / np.arange(N - 1, 1, -1)).cumsum()
    h = hs_cs[-1] + 1
    g = (hs_cs / np.arange(2, N)).sum()
    a = (4 * g - 6) * (k - 1) + (10 - 6 * g) * H
    b = (2 * g - 4) * k ** 2 + 8 * h * k + (2 * g - 14 * h - 4) * H - 8 * h + 4 * g - 6
    c = (6 * h + 2 * g - 2) * k ** 2 + (4 * h - 4 * g + 6) * k + (2 * h - 6) * H + 4 * h
    d = (2 * h + 6) * k ** 2 - 4 * h * k
    return (a * N ** 3 + b * N ** 2 + c * N + d) / ((N - 1.) * (N - 2.) * (N - 3.))


def ad_statistic(sums, nr, nf):
    """anderson_ksamp([x, y]).statistic (midrank) from the per-sample sums of `inner` ([..., 3] float64)"""
    n = np.array([nr, nf])
    N = nr + nf
    A2 = np.empty(sums.shape[:-1])
    sq = math.sqrt(ad_sigmasq(nr, nf))
    flat, sf = A2.reshape(-1), sums.reshape(-1, 3)
    for i in range(flat.size):
        A2akN = 0.
        A2akN += sf[i, 0] / n[0]
        A2akN += sf[i, 1] / n[1]
        A2akN *= (N - 1.) / N
        flat[i] = (A2akN - 1) / sq
    return A2


def auc_statistic(u2, nr, nf):
    """|roc_auc_score(labels, score) - 0.5| + 0.5 from 2U: the AUC is U / (nr nf) (the reference's trapezoids agree to
    rounding)"""
    auc = (u2.astype(np.float64) / 2.0) / (float(nr) * float(nf))
    return np.abs(auc - 0.5) + 0.5


def kl_divergence(p, q):
    return np.sum(p * np.log(p / q))


def js_divergence(p, q):
    m = 0.5 * (p + q)
    return 0.5 * kl_divergence(p, m) + 0.5 * kl_divergence(q, m)


def divergence(P, Q, bins, js):
    """the reference's _kl1d / _js1d tail per (replicate, feature) of the probabilities P, Q [n_iters, d, bins]: eps
    added, then the 1-D numpy calls themselves (a row-wise vectorisation could sum in another order)"""
    eps = 10 ** -5 / bins
    fn = js_divergence if js else kl_divergence
    S = np.empty(P.shape[:2])
    with np.errstate(divide="ignore", invalid="ignore"):
        for r in range(P.shape[0]):
            for f in range(P.shape[1]):
                S[r, f] = fn(P[r, f] + eps, Q[r, f] + eps)
    return S


def hist_probs(counts):
    """p = h / h.sum() per (replicate, feature, sample) of the counts [n_iters, d, 2, bins]"""
    h = counts.astype(np.int64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return h / h.sum(axis=-1, keepdims=True)


def silverman(n):
    """KernelDensity(bandwidth='silverman').bandwidth_ of an n-row 1-D sample (no data-scale factor)"""
    return (n * (1 + 2) / 4) ** (-1 / (1 + 4))


def kde_probs(logsum, nr, nf):
    """exp(score_samples(grid)) normalised, per (replicate, feature, sample), from the kernel's log-sum-exp [..., 2,
    bins]: score = logsum + log_knorm - log n, log_knorm = -0.5 log(2 pi) - log h (sklearn's Gaussian norm)"""
    P = np.empty_like(logsum)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        for s, n in ((0, nr), (1, nf)):
            knorm = -0.5 * 1 * math.log(2 * math.pi) - 1 * math.log(silverman(n))
            p = np.exp((logsum[:, :, s] + knorm) - np.log(n))
            P[:, :, s] = p / p.sum(axis=-1, keepdims=True)
    return P
