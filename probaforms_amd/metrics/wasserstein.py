"""wasserstein_1d, sliced_wasserstein_distance: the Wasserstein distance W_p (p = 1 or 2) between a real and a generated
sample, bootstrapped, on the GPU (kernels: csrc/pf_wasserstein.hip, pfm_wasserstein1d / pfm_project; host side: _m1d.py,
_boot.py).  The reference has no such metric; arguments, bootstrap stream and the (mean, std) return value follow its
other metrics.

Per iteration the rows of X_real, then of X_fake, are resampled with replacement from numpy's global generator.
  wasserstein_1d               per feature, W_p between the two resampled columns' empirical distributions,
                               W_p^p = int_0^1 |Q_real(u) - Q_fake(u)|^p du (p = 1: scipy.stats.wasserstein_distance);
                               the features are averaged.
  sliced_wasserstein_distance  (mean_k W_p^p(Xb theta_k, Yb theta_k))^(1/p) over n_projections unit directions theta_k,
                               drawn once per call before the first bootstrap draw: np.random.normal(size=(n_projections,
                               d)) on the same generator, each row divided by its 2-norm.
  sliced_wasserstein_full_sample  the same statistic of the samples as given, with no resampling: the directions are drawn
                               as above and nothing else is (kernels: csrc/pf_slicegrad.hip, the value of
                               losses.sliced_wasserstein_loss, p-th root taken).
Inputs may be numpy arrays, array-likes or torch tensors; a CUDA tensor stays on its device.  All arithmetic is
float64.  NaN or infinite input and a bad n_iters, p or n_projections raise ValueError before any draw.  Importing this
module needs no GPU.
"""
import numpy as np
import torch

from . import _boot, _lib, _m1d


def _order(p):
    """p as the int 1 or 2 (an int or float equal to one of them)"""
    if not isinstance(p, bool) and isinstance(p, (int, float, np.integer, np.floating)) and p in (1, 2):
        return int(p)
    raise ValueError("p must be 1 or 2, got %r" % (p,))


def directions(n_projections, d):
    """[n_projections, d] unit rows: normal draws from numpy's global generator, each row divided by its 2-norm"""
    th = np.random.normal(size=(n_projections, d))
    return th / np.sqrt((th * th).sum(axis=1))[:, None]


def index_groups(nr, nf, cols, n_iters, p):
    """the number of index groups (_boot.replicates) a call on `cols` pooled columns runs as"""
    G = _boot.group_size(n_iters, nr + nf, _lib.wasserstein1d_workspace_bytes(nr, nf, cols, 1, p))
    return -(-n_iters // G)


def _run(pooled, n_iters, p):
    """-> numpy [n_iters, pooled.d]: W_p^p of every bootstrap replicate of every pooled column, the draws made from
    numpy's global generator as the reference's metrics make them"""
    nr, nf, d = pooled.nr, pooled.nf, pooled.d
    out = torch.empty((n_iters, d), dtype=torch.float64, device=pooled.device)

    def launch(start, reps, ir, jf, ws):
        _lib.wasserstein1d(p, pooled.cols, pooled.perm, pooled.gstart, pooled.ngroups, nr, nf, ir, jf, reps,
                           out[start:start + reps], ws)

    _boot.replicates(nr, nf, pooled.device, n_iters, lambda r: _lib.wasserstein1d_workspace_bytes(nr, nf, d, r, p), launch)
    return out.cpu().numpy()


def _root(S, p):
    return S if p == 1 else np.sqrt(S)


def _replicates_1d(X_real, X_fake, n_iters=100, p=1):
    _m1d.check_args(X_real, X_fake, n_iters)
    p = _order(p)
    Xr, Xf = _boot.prepare(X_real, X_fake, ("X_real", "X_fake"), n_iters)
    with torch.cuda.device(Xr.device):
        return _root(_run(_m1d.Pooled(Xr, Xf), n_iters, p), p)


def _replicates_sliced(X_real, X_fake, n_iters=100, n_projections=64, p=2, standardize=False):
    _m1d.check_args(X_real, X_fake, n_iters)
    p = _order(p)
    n_projections = _m1d.check_positive_int(n_projections, "n_projections")
    Xr, Xf = _boot.prepare(X_real, X_fake, ("X_real", "X_fake"), n_iters, standardize)
    with torch.cuda.device(Xr.device):
        theta = torch.from_numpy(directions(n_projections, Xr.shape[1])).to(Xr.device)
        # a resample of projections is the projection of the resample: project the original rows once
        cols = torch.empty((n_projections, Xr.shape[0] + Xf.shape[0]), dtype=torch.float64, device=Xr.device)
        _lib.project(Xr, Xf, theta, cols)
        S = _run(_m1d.Pooled.from_columns(cols, Xr.shape[0]), n_iters, p)
    return _root(S.mean(axis=1), p)


# per-replicate values of each public call, on the same draws: [n_iters, d] (per feature) and [n_iters]
REPLICATES = {"wasserstein_1d": _replicates_1d, "sliced_wasserstein_distance": _replicates_sliced}


def wasserstein_1d(X_real, X_fake, n_iters=100, p=1):
    '''
    Calculates the 1-D Wasserstein distance W_p for real and fake samples, bootstrapped.
    The function calculates the distance for each input feature, and then averages them.

    Parameters:
    -----------
    X_real: array of shape [n_samples, n_features] (numpy, array-like or torch; a CUDA tensor stays on the device)
        Real sample.
    X_fake: array of shape [m_samples, n_features]
        Generated sample.
    n_iters: int
        The number of bootstrap iterations. Default = 100.
    p: 1 or 2
        The order of the distance. Default = 1 (scipy.stats.wasserstein_distance).

    Return:
    -------
    (mean, std) of the replicates' feature-averaged distance (np.std, ddof 0), numpy float64.
    '''
    return _m1d.feature_average(_replicates_1d(X_real, X_fake, n_iters, p))


def sliced_wasserstein_distance(X_real, X_fake, n_iters=100, n_projections=64, p=2, standardize=False):
    '''
    Calculates the sliced Wasserstein distance for real and fake samples, bootstrapped: the p-th root of the mean of
    W_p^p between the samples' projections on n_projections random unit directions (the same for every iteration).

    Parameters:
    -----------
    X_real: array of shape [n_samples, n_features] (numpy, array-like or torch; a CUDA tensor stays on the device)
        Real sample.
    X_fake: array of shape [m_samples, n_features]
        Generated sample.
    n_iters: int
        The number of bootstrap iterations. Default = 100.
    n_projections: int
        The number of directions. Default = 64.
    p: 1 or 2
        The order of the distance. Default = 2.
    standardize: boolean
        If True, the StandardScaler fitted on the real sample is applied to both before projecting. Default = False.

    Return:
    -------
    (mean, std) of the replicates (np.std, ddof 0), numpy float64.
    '''
    S = _replicates_sliced(X_real, X_fake, n_iters, n_projections, p, standardize)
    return S.mean(axis=0), S.std(axis=0)


def sliced_wasserstein_full_sample(X_real, X_fake, n_projections=64, p=2, standardize=False):
    '''
    Calculates the sliced Wasserstein distance of the samples as given, with no resampling: the p-th root of the mean of W_p^p
    between the samples' projections on n_projections random unit directions, drawn as sliced_wasserstein_distance draws them
    (one np.random.normal call on numpy's global generator); nothing else is drawn.

    Parameters:
    -----------
    X_real, X_fake, n_projections, p, standardize: as sliced_wasserstein_distance; n_projections at most 65535.

    Return:
    -------
    The distance, numpy float64: losses.sliced_wasserstein_loss of the same directions, p-th root taken.
    '''
    from . import losses                               # (the loss: its kernels, value only)
    _m1d.check_args(X_real, X_fake, 1)
    p = _order(p)
    n_projections = _m1d.check_positive_int(n_projections, "n_projections")
    if n_projections > losses.MAX_PROJECTIONS:
        raise ValueError("n_projections must be at most %d, got %d" % (losses.MAX_PROJECTIONS, n_projections))
    _m1d.check_bool(standardize, "standardize")
    Xr, Xf = _boot.prepare(X_real, X_fake, ("X_real", "X_fake"), 1, standardize)
    with torch.cuda.device(Xr.device):
        theta = torch.from_numpy(directions(n_projections, Xr.shape[1])).to(Xr.device)
        value, _ = losses._slice_call(p, torch.cat([Xr, Xf], dim=0).contiguous(), Xr.shape[0], theta, False)
        return _root(np.float64(value.cpu().numpy()), p)
