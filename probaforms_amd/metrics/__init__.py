"""probaforms_amd.metrics -- the metrics of probaforms.metrics on the GPU.

    from probaforms_amd.metrics import maximum_mean_discrepancy, frechet_distance
    mu, sigma = maximum_mean_discrepancy(X, Y, n_iters=100, standardize=False)
    mu, sigma = frechet_distance(X_real, X_fake, n_iters=100, standardize=False)

Signatures, defaults, the bootstrap draws on numpy's global generator and the `(mean, std)` return value
are the reference's (probaforms/metrics/mmd.py, fd.py); all arithmetic is float64.  Inputs may be numpy
arrays, array-likes or torch tensors; a CUDA tensor is used on its device without a copy to the host.
The hot paths are HIP kernels in libpf_metrics.so (csrc/), loaded on the first call, so importing this
module needs no GPU.  There is no CPU fallback.

The eight 1-D metrics of the reference live in the reference's module paths, not in this package's export list:

    from probaforms_amd.metrics.ks1d import kolmogorov_smirnov_1d, cramer_von_mises_1d, roc_auc_score_1d, anderson_darling_1d
    from probaforms_amd.metrics.div1d import kullback_leibler_1d, jensen_shannon_1d           # histograms, bins=10
    from probaforms_amd.metrics.div1d import kullback_leibler_1d_kde, jensen_shannon_1d_kde   # Gaussian KDE, bins=101

The metrics the reference does not have are modules of their own, outside the export list as well: the Wasserstein distances
(wasserstein.py) and k-nearest-neighbour precision, recall, density and coverage, which say in which way a generated sample is
wrong (fidelity against diversity) where the distances only say how much, and the parameter-free energy distance:

    from probaforms_amd.metrics.wasserstein import wasserstein_1d, sliced_wasserstein_distance
    from probaforms_amd.metrics.prdc import prdc, prdc_full_sample     # bootstrapped (mean, std) pairs; the samples as given
    from probaforms_amd.metrics.energy import energy_distance, energy_distance_full_sample
    from probaforms_amd.metrics.twosample import energy_test, mmd_test, knn_test, nn_accuracy_full_sample   # permutation p-values

All of these return numpy floats.  The two statistics with a closed form can also be trained on: 0-d tensors whose backward
fills the gradient of the generated (or the real) rows, from one more sweep over the same pair tiles:

    from probaforms_amd.metrics.losses import energy_loss, mmd_loss       # differentiable D^2 and biased MMD^2

Those compare two pooled samples.  The loss a CONDITIONAL sampler is trained on scores every condition row's K draws against the
row's own observed target, the energy score and the CRPS that sample_joint_scores and sample_scores report as metrics:

    from probaforms_amd.metrics.losses import energy_score_loss, crps_loss    # X_draws [K, n, d] against Y [n, d], per row

The Frechet distance has both forms as well, wholly on the device for at most 64 features (a symmetric eigensolver in LDS gives the
trace of the matrix square root and, being a spectral function, its gradient): moment matching, O(n d^2) where the pair losses
walk n^2 pairs:

    from probaforms_amd.metrics.fd import frechet_distance_full_sample       # the samples as given, a numpy float
    from probaforms_amd.metrics.losses import frechet_loss                   # the same value with a backward()

`__all__` and the `probaforms.metrics` alias (`probaforms_amd.install_as_probaforms()`) name only the two
multivariate metrics, so `from probaforms.metrics import kolmogorov_smirnov_1d` raises ImportError there.
"""
from .fd import frechet_distance
from .mmd import maximum_mean_discrepancy

__all__ = ["frechet_distance", "maximum_mean_discrepancy"]
