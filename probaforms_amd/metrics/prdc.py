"""prdc, prdc_full_sample: k-nearest-neighbour precision, recall, density and coverage between a real and a generated
sample on the GPU (kernels: csrc/pf_knn.hip, pfm_prdc; host side: _boot.py, _m1d.py).  The reference has no such metric;
arguments, bootstrap stream and the (mean, std) return values follow its other metrics.

Unlike the distances (MMD, Frechet, Wasserstein) the four values say in which way a generated sample is wrong: precision
and density fall when generated rows lie outside the real sample's support (low fidelity), recall and coverage fall when
parts of the real sample have no generated rows nearby (low diversity, mode collapse).  With k = nearest_k, every row's
radius is the distance to its k-th nearest neighbour inside its own sample (the row itself not counted), and
  precision  the share of fake rows inside at least one real row's ball      (Kynkaanniemi et al., NeurIPS 2019)
  recall     the share of real rows inside at least one fake row's ball
  density    the number of real balls a fake row lies in, averaged over the fake rows, over k   (Naeem et al., ICML 2020)
  coverage   the share of real rows whose ball holds at least one fake row
All comparisons are strict and between squared float64 distances (the `prdc` package's expressions, squared), so each
replicate is four integer counts and a call is exact and bitwise reproducible.

prdc resamples the rows of X_real, then of X_fake, with replacement from numpy's global generator per iteration, as the other
metrics do.  Resampling with replacement duplicates rows, a duplicate is a neighbour at distance 0, and so the bootstrapped
radii are smaller than the full samples': a row drawn more than nearest_k times has radius 0.  All four bootstrapped values
are therefore biased low against the published definitions; prdc_full_sample computes those, on the samples as given.

Inputs may be numpy arrays, array-likes or torch tensors; a CUDA tensor stays on its device.  NaN or infinite input and a
bad n_iters or nearest_k raise ValueError before any draw.  Importing this module needs no GPU.
"""
import collections

import numpy as np
import torch

from . import _boot, _lib, _m1d

PRDC = collections.namedtuple("PRDC", ["precision", "recall", "density", "coverage"])


def _check(X_real, X_fake, n_iters, nearest_k):
    """_m1d.check_args, then nearest_k: an int in 1 .. min(16, min(rows) - 1)"""
    _m1d.check_args(X_real, X_fake, n_iters)
    _m1d.check_positive_int(nearest_k, "nearest_k")
    if nearest_k > _lib.KNN_MAX_K:
        raise ValueError("nearest_k is at most %d, got %d" % (_lib.KNN_MAX_K, nearest_k))
    rows = min(_boot._check_2d(A, name)[1][0] for A, name in ((X_real, "X_real"), (X_fake, "X_fake")))
    if nearest_k >= rows:
        raise ValueError("nearest_k must be smaller than both samples' numbers of rows, got %d for %d rows"
                         % (nearest_k, rows))
    return int(nearest_k)


def _counts(X_real, X_fake, n_iters, k, standardize):
    """the checked arguments -> numpy int64 [n_iters, 4] P, Rc, Dn, Cv; n_iters = None: [1, 4] of the samples as given"""
    n = 1 if n_iters is None else n_iters
    Xr, Xf = _boot.prepare(X_real, X_fake, ("X_real", "X_fake"), n, standardize)
    (nr, d), nf = Xr.shape, Xf.shape[0]
    with torch.cuda.device(Xr.device):
        counts = torch.empty((n, 4), dtype=torch.int64, device=Xr.device)
        radii = []                  # a group's squared radii, real and fake

        def launch(start, reps, ir, jf, ws):
            if not radii:           # (the first group is the largest)
                radii.extend(torch.empty(reps * rows, dtype=torch.float64, device=Xr.device) for rows in (nr, nf))
            _lib.prdc(Xr, Xf, ir, jf, reps, k, radii[0][:reps * nr], radii[1][:reps * nf], counts[start:start + reps], ws)

        # a replicate's radii count among the bytes that bound a group
        _boot.replicates(nr, nf, Xr.device, n_iters, lambda r: _lib.prdc_workspace_bytes(nr, nf, d, r, k), launch,
                         _lib.prdc_workspace_bytes(nr, nf, d, 1, k) + 8 * (nr + nf))
        return counts.cpu().numpy()


def _replicates(X_real, X_fake, n_iters=100, nearest_k=5, standardize=False):
    """-> numpy int64 [n_iters, 4]: the counts P, Rc, Dn, Cv of every bootstrap replicate, the draws made from numpy's
    global generator as the reference's metrics make them"""
    return _counts(X_real, X_fake, n_iters, _check(X_real, X_fake, n_iters, nearest_k), standardize)


# per-replicate counts of the public call, on the same draws: int64 [n_iters, 4] (P, Rc, Dn, Cv)
REPLICATES = {"prdc": _replicates}


def metrics_of(counts, nr, nf, k):
    """[n, 4] int64 counts -> float64 [n, 4] precision, recall, density, coverage: Python ints divided, rounded once"""
    return np.array([[int(P) / nf, int(Rc) / nr, int(Dn) / (k * nf), int(Cv) / nr] for P, Rc, Dn, Cv in counts],
                    dtype=np.float64).reshape(-1, 4)


def prdc(X_real, X_fake, n_iters=100, nearest_k=5, standardize=False):
    '''
    Calculates k-nearest-neighbour precision, recall, density and coverage for real and fake samples, bootstrapped.
    Resampling with replacement shrinks the k-th-neighbour radii (duplicated rows are neighbours at distance 0), so the
    values are biased low against the published definitions: see prdc_full_sample.

    Parameters:
    -----------
    X_real: array of shape [n_samples, n_features] (numpy, array-like or torch; a CUDA tensor stays on the device)
        Real sample.
    X_fake: array of shape [m_samples, n_features]
        Generated sample.
    n_iters: int
        The number of bootstrap iterations. Default = 100.
    nearest_k: int
        The neighbour that sets a row's radius, 1 <= nearest_k <= 16 and below both samples' sizes. Default = 5.
    standardize: boolean
        If True, the StandardScaler fitted on the real sample is applied to both. Default = False.

    Return:
    -------
    PRDC(precision, recall, density, coverage), each the (mean, std) of the replicates (np.std, ddof 0), numpy float64.
    '''
    C = _replicates(X_real, X_fake, n_iters, nearest_k, standardize)
    nr, nf = len(X_real), len(X_fake)
    M = metrics_of(C, nr, nf, int(nearest_k))
    return PRDC(*[(M[:, q].mean(axis=0), M[:, q].std(axis=0)) for q in range(4)])


def prdc_full_sample(X_real, X_fake, nearest_k=5, standardize=False):
    '''
    Calculates k-nearest-neighbour precision, recall, density and coverage of the samples as given: the published
    definitions (the `prdc` package's values), with no resampling.  Nothing is drawn; numpy's generator is untouched.
    prdc's bootstrapped values are biased low against these, because a resample's duplicated rows shrink the radii.

    Parameters:
    -----------
    X_real, X_fake, nearest_k, standardize: as prdc.

    Return:
    -------
    PRDC(precision, recall, density, coverage), four numpy float64.
    '''
    k = _check(X_real, X_fake, 1, nearest_k)
    M = metrics_of(_counts(X_real, X_fake, None, k, standardize), len(X_real), len(X_fake), k)
    return PRDC(*[M[0, q] for q in range(4)])
