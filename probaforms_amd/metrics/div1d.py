"""kullback_leibler_1d, jensen_shannon_1d (histograms) and kullback_leibler_1d_kde, jensen_shannon_1d_kde (Gaussian
KDE, Silverman bandwidth): probaforms/metrics/div1d.py on the GPU (kernels: csrc/pf_metrics1d.hip, pfm_metric1d;
host side: _m1d.py).

Same signatures, defaults, bootstrap stream and (mean, std) return value as the reference (see ks1d.py).  The
histogram counts and the KDE log densities come from the kernels; p = h / h.sum() (or exp and normalise), the
eps = 1e-5 / bins and the divergence itself are the reference's numpy expressions.  Departures: NaN or infinite
input, and `bins` that is not a positive int, raise ValueError before any draw.  As in the reference, a KDE
replicate whose densities all underflow to 0 gives NaN.
"""
from . import _lib, _m1d


def _replicates_hist(X_real, X_fake, n_iters, bins, js):
    _m1d.check_args(X_real, X_fake, n_iters, bins)
    P = _m1d.hist_probs(_m1d.run(_lib.M1D_HIST, X_real, X_fake, n_iters, bins))
    return _m1d.divergence(P[:, :, 0], P[:, :, 1], bins, js)


def _replicates_kde(X_real, X_fake, n_iters, bins, js):
    _m1d.check_args(X_real, X_fake, n_iters, bins)
    nr, nf = len(X_real), len(X_fake)
    logsum = _m1d.run(_lib.M1D_KDE, X_real, X_fake, n_iters, bins, (_m1d.silverman(nr), _m1d.silverman(nf)))
    P = _m1d.kde_probs(logsum, nr, nf)
    return _m1d.divergence(P[:, :, 0], P[:, :, 1], bins, js)


# per-replicate, per-feature divergences [n_iters, d] of each public call, on the same draws
REPLICATES = {
    "kullback_leibler_1d": lambda X, Y, n_iters=100, bins=10: _replicates_hist(X, Y, n_iters, bins, False),
    "jensen_shannon_1d": lambda X, Y, n_iters=100, bins=10: _replicates_hist(X, Y, n_iters, bins, True),
    "kullback_leibler_1d_kde": lambda X, Y, n_iters=100, bins=101: _replicates_kde(X, Y, n_iters, bins, False),
    "jensen_shannon_1d_kde": lambda X, Y, n_iters=100, bins=101: _replicates_kde(X, Y, n_iters, bins, True),
}

_DOC = '''
    Calculates the {what} for real and fake samples, bootstrapped.
    The function calculates metric values for each input feature, and then averages them.

    Parameters:
    -----------
    X_real: array of shape [n_samples, n_features] (numpy, array-like or torch; a CUDA tensor stays on the device)
        Real sample.
    X_fake: array of shape [m_samples, n_features]
        Generated sample.
    n_iters: int
        The number of bootstrap iterations. Default = 100.
    bins: int
        {bins}

    Return:
    -------
    (mean, std) of the replicates' feature-averaged divergence (np.std, ddof 0), numpy float64.
    '''
_HIST = "Bins of the histograms (np.histogram of the pooled resample). Default = 10."
_KDE = "Points of the density grid (np.linspace over the pooled resample's range). Default = 101."


def kullback_leibler_1d(X_real, X_fake, n_iters=100, bins=10):
    return _m1d.feature_average(_replicates_hist(X_real, X_fake, n_iters, bins, False))


def jensen_shannon_1d(X_real, X_fake, n_iters=100, bins=10):
    return _m1d.feature_average(_replicates_hist(X_real, X_fake, n_iters, bins, True))


def kullback_leibler_1d_kde(X_real, X_fake, n_iters=100, bins=101):
    return _m1d.feature_average(_replicates_kde(X_real, X_fake, n_iters, bins, False))


def jensen_shannon_1d_kde(X_real, X_fake, n_iters=100, bins=101):
    return _m1d.feature_average(_replicates_kde(X_real, X_fake, n_iters, bins, True))


kullback_leibler_1d.__doc__ = _DOC.format(what="Kullback-Leibler divergence of the histograms", bins=_HIST)
jensen_shannon_1d.__doc__ = _DOC.format(what="Jensen-Shannon divergence of the histograms", bins=_HIST)
kullback_leibler_1d_kde.__doc__ = _DOC.format(what="Kullback-Leibler divergence of the 1-D KDEs", bins=_KDE)
jensen_shannon_1d_kde.__doc__ = _DOC.format(what="Jensen-Shannon divergence of the 1-D KDEs", bins=_KDE)
