"""probaforms_amd.metrics -- the two multivariate metrics of probaforms.metrics on the GPU.

    from probaforms_amd.metrics import maximum_mean_discrepancy, frechet_distance
    mu, sigma = maximum_mean_discrepancy(X, Y, n_iters=100, standardize=False)
    mu, sigma = frechet_distance(X_real, X_fake, n_iters=100, standardize=False)

Signatures, defaults, the bootstrap draws on numpy's global generator and the `(mean, std)` return value
are the reference's (probaforms/metrics/mmd.py, fd.py); all arithmetic is float64.  Inputs may be numpy
arrays, array-likes or torch tensors; a CUDA tensor is used on its device without a copy to the host.
The hot paths are HIP kernels in libpf_metrics.so (csrc/), loaded on the first call, so importing this
module needs no GPU.  There is no CPU fallback.

Only these two metrics exist here.  The eight 1-D metrics of the reference (kolmogorov_smirnov_1d,
cramer_von_mises_1d, anderson_darling_1d, roc_auc_score_1d, kullback_leibler_1d[_kde],
jensen_shannon_1d[_kde]) are not provided: `from probaforms.metrics import kolmogorov_smirnov_1d` after
`probaforms_amd.install_as_probaforms()` raises ImportError.
"""
from .fd import frechet_distance
from .mmd import maximum_mean_discrepancy

__all__ = ["frechet_distance", "maximum_mean_discrepancy"]
