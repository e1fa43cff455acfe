"""maximum_mean_discrepancy: probaforms/metrics/mmd.py on the GPU (kernels: csrc/pf_metrics.hip, pfm_mmd)."""
import numpy as np
import torch

from . import _boot, _lib


def maximum_mean_discrepancy(X, Y, n_iters=100, standardize=False):
    '''
    Calculates the Maximum Mean Discrepancy between real and fake samples, bootstrapped.

    Same signature, defaults, random stream and return value as the reference: per iteration the rows of
    X, then of Y, are resampled with replacement from numpy's global generator; each replicate takes the
    RBF kernel with gamma = 1 / (2 median^2), median over the full pooled distance matrix.

    Parameters:
    -----------
    X: array of shape [n_samples, n_features] (numpy, array-like or torch; a CUDA tensor stays on the device)
        Real sample.
    Y: array of shape [m_samples, n_features]
        Generated sample.
    n_iters: int
        The number of bootstrap iterations. Default = 100.
    standardize: boolean
        If True, the mean and population std of X standardise X and Y. Default = False.

    Return:
    -------
    (mean, std) of the replicates' MMD (np.std, ddof 0), numpy float64.

    Raises ValueError if a replicate's median distance is 0 (as the reference's gamma = inf does).
    '''
    med, mmds = replicates(X, Y, n_iters, standardize)
    if not (med > 0).all():
        bad = int(np.flatnonzero(~(med > 0))[0])
        raise ValueError("bootstrap replicate %d: the median pairwise distance is 0, so gamma = 1 / (2 median^2) is "
                         "infinite (too few distinct rows)" % bad)
    return np.mean(mmds), np.std(mmds)


def replicates(X, Y, n_iters=100, standardize=False):
    """-> (medians, mmds): numpy float64 per replicate, the draws of the public call (a median of 0 gives a NaN mmd)"""
    X, Y = _boot.prepare(X, Y, ("X", "Y"), n_iters, standardize)
    with torch.cuda.device(X.device):
        nx, d = X.shape
        ny = Y.shape[0]
        med = torch.empty(n_iters, dtype=torch.float64, device=X.device)
        out = torch.empty(n_iters, dtype=torch.float64, device=X.device)

        def launch(start, reps, ix, iy, ws):
            _lib.mmd(X, Y, ix, iy, reps, med[start:start + reps], out[start:start + reps], ws)

        # (the groups are sized by the indices alone: ws_per_rep = 0)
        _boot.replicates(nx, ny, X.device, n_iters, lambda r: _lib.mmd_workspace_bytes(nx, ny, d, r), launch, 0)
        return med.cpu().numpy(), out.cpu().numpy()
