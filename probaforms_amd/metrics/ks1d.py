"""kolmogorov_smirnov_1d, cramer_von_mises_1d, roc_auc_score_1d, anderson_darling_1d: probaforms/metrics/ks1d.py on
the GPU (kernels: csrc/pf_metrics1d.hip, pfm_metric1d; host side: _m1d.py).

Same signatures, defaults, bootstrap stream and (mean, std) return value as the reference: per iteration the rows of
X_real, then of X_fake, are resampled with replacement from numpy's global generator; each feature's statistic is
taken on the two resampled columns and the features are averaged.  Inputs may be numpy arrays, array-likes or torch
tensors; a CUDA tensor stays on its device.  All arithmetic is float64.  Importing this module needs no GPU.

Departures from the reference: NaN or infinite input raises ValueError before any draw; where the reference raises
(anderson_darling_1d on a replicate whose pooled resample holds a single distinct value, or with fewer than 3 pooled
rows) this raises ValueError.  cramer_von_mises_1d with a sample of fewer than 2 rows gives NaN, as the reference
does with scipy 1.15 (whose cramervonmises_2samp returns NaN there rather than raising).  Where the generator
stands after an error is unspecified.  cramer_von_mises_1d takes at most 2**20 pooled rows.
"""
import numpy as np

from . import _lib, _m1d


def _replicates_ks(X_real, X_fake, n_iters):
    _m1d.check_args(X_real, X_fake, n_iters)
    return _m1d.ks_statistic(_m1d.run(_lib.M1D_KS, X_real, X_fake, n_iters), len(X_real), len(X_fake))


def _replicates_cvm(X_real, X_fake, n_iters):
    _m1d.check_args(X_real, X_fake, n_iters)
    nr, nf = len(X_real), len(X_fake)
    if nr + nf > _lib.CVM_MAX_N:
        raise ValueError("cramer_von_mises_1d supports at most %d pooled rows, got %d" % (_lib.CVM_MAX_N, nr + nf))
    t = _m1d.cvm_statistic(_m1d.run(_lib.M1D_CVM, X_real, X_fake, n_iters), nr, nf)
    if nr < 2 or nf < 2:          # scipy 1.15's cramervonmises_2samp returns NaN for a sample of fewer than 2 rows
        t[...] = np.nan
    return t


def _replicates_auc(X_real, X_fake, n_iters):
    _m1d.check_args(X_real, X_fake, n_iters)
    return _m1d.auc_statistic(_m1d.run(_lib.M1D_AUC, X_real, X_fake, n_iters), len(X_real), len(X_fake))


def _replicates_ad(X_real, X_fake, n_iters):
    _m1d.check_args(X_real, X_fake, n_iters)
    nr, nf = len(X_real), len(X_fake)
    if nr + nf < 3:
        raise ValueError("anderson_darling_1d needs at least 3 pooled rows, got %d" % (nr + nf))
    sums = _m1d.run(_lib.M1D_AD, X_real, X_fake, n_iters)
    one = np.argwhere(sums[..., 2] < 2)
    if len(one):
        raise ValueError("bootstrap replicate %d, feature %d: the pooled resample holds a single distinct value "
                         "(anderson_ksamp needs more than one)" % tuple(one[0]))
    return _m1d.ad_statistic(sums, nr, nf)


# per-replicate, per-feature statistics [n_iters, d] of each public call, on the same draws
REPLICATES = {"kolmogorov_smirnov_1d": _replicates_ks, "cramer_von_mises_1d": _replicates_cvm,
              "roc_auc_score_1d": _replicates_auc, "anderson_darling_1d": _replicates_ad}

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

    Return:
    -------
    (mean, std) of the replicates' feature-averaged statistic (np.std, ddof 0), numpy float64.
    '''


def kolmogorov_smirnov_1d(X_real, X_fake, n_iters=100):
    return _m1d.feature_average(_replicates_ks(X_real, X_fake, n_iters))


def cramer_von_mises_1d(X_real, X_fake, n_iters=100):
    return _m1d.feature_average(_replicates_cvm(X_real, X_fake, n_iters))


def roc_auc_score_1d(X_real, X_fake, n_iters=100):
    return _m1d.feature_average(_replicates_auc(X_real, X_fake, n_iters))


def anderson_darling_1d(X_real, X_fake, n_iters=100):
    return _m1d.feature_average(_replicates_ad(X_real, X_fake, n_iters))


kolmogorov_smirnov_1d.__doc__ = _DOC.format(what="Kolmogorov-Smirnov statistic (scipy.stats.ks_2samp)")
cramer_von_mises_1d.__doc__ = _DOC.format(what="Cramer-von Mises statistic (scipy.stats.cramervonmises_2samp)")
roc_auc_score_1d.__doc__ = _DOC.format(what="ROC AUC of telling the samples apart, |AUC - 0.5| + 0.5")
anderson_darling_1d.__doc__ = _DOC.format(what="Anderson-Darling statistic (scipy.stats.anderson_ksamp, midrank)")
