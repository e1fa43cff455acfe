"""frechet_distance: probaforms/metrics/fd.py with the bootstrap moments on the GPU (csrc/pf_metrics.hip,
pfm_boot_moments) and the trace of the matrix square root on the host.

frechet_distance_full_sample: the distance of the samples as given, wholly on the device (csrc/pf_frechet.hip,
pfm_frechet_grad: the same moments, then the trace of the matrix square root from two symmetric eigen-decompositions by Jacobi
rotations in LDS), for at most 64 features; losses.frechet_loss is the same call with a backward()."""
import numpy as np
import torch

from . import _boot, _lib


def trace_sqrtm(A, B):
    """tr sqrtm(A @ B) for symmetric positive semi-definite A, B (numpy only).  With S = sqrt(A) (eigh), A B
    is similar to S B S, whose eigenvalues are real and >= 0: the trace is sum sqrt(clip(eigvalsh(S B S), 0)).
    Agrees with scipy.linalg.sqrtm(A @ B).real.trace() to rounding, also for singular A (n < d)."""
    w, V = np.linalg.eigh(A)
    S = (V * np.sqrt(np.clip(w, 0.0, None))) @ V.T
    M = S @ B @ S
    ev = np.linalg.eigvalsh((M + M.T) * 0.5)
    return float(np.sum(np.sqrt(np.clip(ev, 0.0, None))))


def frechet_distance(X_real, X_fake, n_iters=100, standardize=False):
    '''
    Calculates the Frechet Distance between real and fake samples, bootstrapped.

    Same signature, defaults, random stream and return value as the reference: per iteration the rows of
    X_real, then of X_fake, are resampled with replacement from numpy's global generator;
    FD = ||mu_r - mu_f||^2 + tr S_r + tr S_f - 2 tr sqrtm(S_r S_f), S the np.cov covariance (ddof 1).

    Parameters:
    -----------
    X_real: array of shape [n_samples, n_features] (numpy, array-like or torch; a CUDA tensor stays on the device)
        Real sample.
    X_fake: array of shape [m_samples, n_features]
        Generated sample.
    n_iters: int
        The number of bootstrap iterations. Default = 100.
    standardize: boolean
        If True, the mean and population std of X_real standardise both samples. Default = False.

    Return:
    -------
    (mean, std) of the replicates' distance (np.std, ddof 0), numpy float64.
    '''
    frd = replicates(X_real, X_fake, n_iters, standardize)
    return frd.mean(axis=0), frd.std(axis=0)


def frechet_distance_full_sample(X_real, X_fake, standardize=False):
    '''
    The Frechet Distance between real and fake samples as given: no resampling, nothing is drawn from any generator.
    FD = ||mu_r - mu_f||^2 + tr S_r + tr S_f - 2 tr sqrtm(S_r S_f), as frechet_distance forms it per replicate, computed wholly on
    the device (pfm_frechet_grad without a gradient).

    Parameters:
    -----------
    X_real, X_fake, standardize: as frechet_distance; at least 2 rows each and at most 64 features.

    Return:
    -------
    numpy float64.

    Raises ValueError for more than 64 features (there is no fallback) and fewer than 2 rows in a sample.
    '''
    from . import _m1d, losses                 # (losses imports this package's host helpers; the call is the loss's)
    _m1d.check_bool(standardize, "standardize")
    losses._frechet_shapes(X_real, X_fake)
    Xr, Xf = _boot.prepare(X_real, X_fake, ("X_real", "X_fake"), 1, standardize)
    with torch.cuda.device(Xr.device):
        Z = torch.cat([Xr, Xf], dim=0).contiguous()
        value = losses._frechet_call(0.0, 0, Z, Xr.shape[0], False)[0]
        return np.float64(value.item())


def replicates(X_real, X_fake, n_iters=100, standardize=False):
    """-> numpy float64 [n_iters]: each bootstrap replicate's Frechet distance, the draws of the public call"""
    mean, cov = moments(X_real, X_fake, n_iters, standardize)
    frd = np.empty(n_iters)
    for i in range(n_iters):
        diff = np.sum((mean[i, 0] - mean[i, 1]) ** 2.0)
        frd[i] = diff + np.trace(cov[i, 0]) + np.trace(cov[i, 1]) - 2 * trace_sqrtm(cov[i, 0], cov[i, 1])
    return frd


def moments(X_real, X_fake, n_iters=100, standardize=False):
    """-> (mean [n_iters, 2, d], cov [n_iters, 2, d, d]) of the resampled real (0) and fake (1) sets, numpy float64"""
    Xr, Xf = _boot.prepare(X_real, X_fake, ("X_real", "X_fake"), n_iters, standardize)
    nr, d = Xr.shape
    nf = Xf.shape[0]
    if d > _lib.MOMENTS_MAX_D:
        raise ValueError("frechet_distance supports at most %d features, got %d" % (_lib.MOMENTS_MAX_D, d))
    with torch.cuda.device(Xr.device):
        mean = torch.empty((n_iters, 2, d), dtype=torch.float64, device=Xr.device)
        cov = torch.empty((n_iters, 2, d, d), dtype=torch.float64, device=Xr.device)

        def launch(start, reps, ir, jf, ws):
            _lib.boot_moments(Xr, Xf, ir, jf, reps, mean[start:start + reps], cov[start:start + reps], ws)

        _boot.replicates(nr, nf, Xr.device, n_iters, lambda r: _lib.moments_workspace_bytes(nr, nf, d, r), launch)
        return mean.cpu().numpy(), cov.cpu().numpy()
