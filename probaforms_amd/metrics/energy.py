"""energy_distance, energy_distance_full_sample: the energy distance (Szekely & Rizzo) between a real and a generated
sample on the GPU (kernels: csrc/pf_energy.hip, pfm_energy; host side: _boot.py, _m1d.py).  The reference has no such metric;
arguments, bootstrap stream and the (mean, std) return value follow its other metrics.

With R and F the two (resampled) sets of nr and nf rows and |.| the Euclidean norm, the V-statistic: every ordered pair
counts, the zero diagonals of the within-sample sums included,
  exx = sum_ab |R_a - R_b| / nr^2     eyy = sum_ab |F_a - F_b| / nf^2     exy = sum_ab |R_a - F_b| / (nr nf)
  D^2 = 2 exy - exx - eyy             D = sqrt(max(D^2, 0))
D^2 is mathematically >= 0, and 0 only for equal distributions; the clamp absorbs rounding.  The distance has no bandwidth,
no directions and no neighbour count, and is defined for any number of features; at one feature it is
scipy.stats.energy_distance.  It is the whole-sample companion of the energy score of sample_joint_scores.

energy_distance resamples the rows of X_real, then of X_fake, with replacement from numpy's global generator per iteration,
as the other metrics do.  A replicate is the original sample with integer draw counts c, and its pair sums are quadratic
forms sum_ab c[a] c[b] |z_a - z_b|: the kernel forms every distance once for all replicates and spends one float64
multiply-add per replicate and pair.

Inputs may be numpy arrays, array-likes or torch tensors; a CUDA tensor stays on its device.  NaN or infinite input, a bad
n_iters and a non-bool standardize or squared raise ValueError before any draw.  Importing this module needs no GPU.
"""
import numpy as np
import torch

from . import _boot, _lib, _m1d


def _check(X_real, X_fake, n_iters, standardize, squared):
    _m1d.check_args(X_real, X_fake, n_iters)
    _m1d.check_bool(standardize, "standardize")
    _m1d.check_bool(squared, "squared")


def means_of(S, nr, nf):
    """[n, 3] raw pair sums Srr, Sff, Srf -> [n, 3] exx, eyy, exy: each divided once by its number of ordered pairs"""
    return np.asarray(S, np.float64).reshape(-1, 3) / np.array([nr * nr, nf * nf, nr * nf], dtype=np.float64)


def values_of(E, squared):
    """[n, 3] exx, eyy, exy -> [n] D^2 = (2 exy - exx) - eyy, or D = sqrt(max(D^2, 0))"""
    E = np.asarray(E, np.float64).reshape(-1, 3)
    d2 = (2.0 * E[:, 2] - E[:, 0]) - E[:, 1]
    return d2 if squared else np.sqrt(np.maximum(d2, 0.0))


def _means(X_real, X_fake, n_iters, standardize):
    """the checked arguments -> numpy float64 [n_iters, 3] exx, eyy, exy; n_iters = None: [1, 3] of the samples as given"""
    n = 1 if n_iters is None else n_iters
    Xr, Xf = _boot.prepare(X_real, X_fake, ("X_real", "X_fake"), n, standardize)
    (nr, d), nf = Xr.shape, Xf.shape[0]
    with torch.cuda.device(Xr.device):
        sums = torch.empty((n, 3), dtype=torch.float64, device=Xr.device)

        def launch(start, reps, ir, jf, ws):
            _lib.energy(Xr, Xf, ir, jf, reps, sums[start:start + reps], ws)

        _boot.replicates(nr, nf, Xr.device, n_iters, lambda r: _lib.energy_workspace_bytes(nr, nf, d, r), launch)
        return means_of(sums.cpu().numpy(), nr, nf)


def _replicates(X_real, X_fake, n_iters=100, standardize=False):
    """-> numpy float64 [n_iters, 3]: exx, eyy, exy of every bootstrap replicate, the draws made from numpy's global
    generator as the reference's metrics make them"""
    _check(X_real, X_fake, n_iters, standardize, False)
    return _means(X_real, X_fake, n_iters, standardize)


# per-replicate values of the public call, on the same draws: float64 [n_iters, 3] (exx, eyy, exy)
REPLICATES = {"energy_distance": _replicates}


def energy_distance(X_real, X_fake, n_iters=100, standardize=False, squared=False):
    '''
    Calculates the energy distance (Szekely & Rizzo) for real and fake samples, bootstrapped.
    D^2 = 2 E|X - Y| - E|X - X'| - E|Y - Y'| over all ordered pairs of rows (V-statistic), |.| the Euclidean norm.

    Parameters:
    -----------
    X_real: array of shape [n_samples, n_features] (numpy, array-like or torch; a CUDA tensor stays on the device)
        Real sample.
    X_fake: array of shape [m_samples, n_features]
        Generated sample.
    n_iters: int
        The number of bootstrap iterations. Default = 100.
    standardize: boolean
        If True, the StandardScaler fitted on the real sample is applied to both. Default = False.
    squared: boolean
        If True, D^2 (which rounding may leave slightly negative) instead of D = sqrt(max(D^2, 0)). Default = False.

    Return:
    -------
    (mean, std) of the replicates (np.std, ddof 0), numpy float64.
    '''
    _check(X_real, X_fake, n_iters, standardize, squared)
    V = values_of(_replicates(X_real, X_fake, n_iters, standardize), squared)
    return V.mean(axis=0), V.std(axis=0)


def energy_distance_full_sample(X_real, X_fake, standardize=False, squared=False):
    '''
    Calculates the energy distance of the samples as given, with no resampling.  Nothing is drawn; numpy's generator is
    untouched.

    Parameters:
    -----------
    X_real, X_fake, standardize, squared: as energy_distance.

    Return:
    -------
    The distance, numpy float64.
    '''
    _check(X_real, X_fake, 1, standardize, squared)
    return values_of(_means(X_real, X_fake, None, standardize), squared)[0]
