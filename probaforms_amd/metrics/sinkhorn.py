"""sinkhorn_divergence, sinkhorn_divergence_full_sample: the debiased Sinkhorn divergence (entropic optimal transport; Genevay
et al. 2018, Feydy et al. 2019) between a real and a generated sample on the GPU (kernels: csrc/pf_sinkhorn.hip, pfm_sinkhorn;
host side: _boot.py, _m1d.py).  The reference has no such metric; arguments, bootstrap stream and the (mean, std) return value
follow its other metrics.

With weights a on the nr real rows and b on the nf fake rows, cost C(x, y) = |x - y|^p (Euclidean norm, p = 1 or 2) and
  softmin(h, C, w)[i] = -eps log sum_j w_j exp((h_j - C_ij) / eps),
four potentials start at 0 and n_sinkhorn symmetrised Jacobi steps update them, each from the previous step's values:
  f <- (f + softmin(g, C_RF, b)) / 2     g <- (g + softmin(f, C_FR, a)) / 2
  u <- (u + softmin(u, C_RR, a)) / 2     v <- (v + softmin(v, C_FF, b)) / 2
One last step takes the four softmins without the averaging.  The divergence is
  S = sum_i a_i (f_i - u_i) + sum_j b_j (g_j - v_j) = OT_eps(a, b) - OT_eps(a, a) / 2 - OT_eps(b, b) / 2   (at convergence):
S >= 0, S = 0 for equal weighted samples; for large eps it tends to the energy distance (p = 1: D^2 / 2) or an MMD, for
eps -> 0 to the optimal-transport cost W_p^p.  `drift`, the largest change of a potential in the last averaged step, says how far
the iteration is from its fixed point: small eps needs many more steps than the default (README, Sinkhorn section).

sinkhorn_divergence resamples the rows of X_real, then of X_fake, with replacement from numpy's global generator per iteration,
as the other metrics do.  A replicate is the original sample with weights count / n, and the costs do not depend on it: the
kernel forms every cost once per group of replicates and iteration and spends one float64 exp per replicate, pair and
iteration.  Nothing of the size of the pair matrix is stored.

eps = reg * median^p by default, median being the median of the pooled distance matrix of the samples as given (after
standardize), as mmd_test takes it; one eps serves every replicate of a call.

Inputs may be numpy arrays, array-likes or torch tensors; a CUDA tensor stays on its device.  NaN or infinite input, a bad
n_iters, p, reg, epsilon or n_sinkhorn and a non-bool standardize raise ValueError before any draw.  Importing this module needs
no GPU.
"""
import collections
import math

import numpy as np
import torch

from . import _boot, _lib, _m1d
from .twosample import _median

Sinkhorn = collections.namedtuple("Sinkhorn", ("value", "epsilon", "drift"))

MAX_SINKHORN = 1000000      # pfm_sinkhorn's limit on n_sinkhorn


def _check(X_real, X_fake, n_iters, p, reg, epsilon, n_sinkhorn, standardize):
    _m1d.check_args(X_real, X_fake, n_iters)
    _m1d.check_bool(standardize, "standardize")
    if not _m1d.is_int(p) or p not in (1, 2):
        raise ValueError("p must be 1 or 2, got %r" % (p,))
    _m1d.check_positive(reg, "reg", reciprocal=True)
    _m1d.check_positive(epsilon, "epsilon", none_ok=True, reciprocal=True)
    if not _m1d.is_int(n_sinkhorn) or not 0 <= n_sinkhorn <= MAX_SINKHORN:
        raise ValueError("n_sinkhorn must be an integer in 0 .. %d, got %r" % (MAX_SINKHORN, n_sinkhorn))


def epsilon_of(median, p, reg):
    """eps = reg * median^p, numpy float64; a median of 0 raises"""
    if not median > 0:
        raise ValueError("the median pairwise distance is 0, so eps = reg * median^p is 0 (too few distinct rows); pass epsilon")
    eps = np.float64(reg) * np.float64(median) ** int(p)
    if not (np.isfinite(eps) and eps > 0 and math.isfinite(1.0 / float(eps))):
        raise ValueError("eps = reg * median^p = %r is not a positive finite number with a finite reciprocal" % (eps,))
    return eps


def _epsilon(Xr, Xf, p, reg, epsilon):
    if epsilon is not None:
        return np.float64(epsilon)
    with torch.cuda.device(Xr.device):
        return epsilon_of(_median(Xr, Xf), p, reg)


def _run(X_real, X_fake, n_iters, p, reg, epsilon, n_sinkhorn, standardize):
    """the checked arguments -> (numpy float64 [n_iters, 2]: value and drift of every replicate, eps); n_iters = None: [1, 2] of
    the samples as given"""
    n = 1 if n_iters is None else n_iters
    Xr, Xf = _boot.prepare(X_real, X_fake, ("X_real", "X_fake"), n, standardize)
    (nr, d), nf = Xr.shape, Xf.shape[0]
    eps = _epsilon(Xr, Xf, p, reg, epsilon)                    # before any draw: a median of 0 raises here
    with torch.cuda.device(Xr.device):
        out = torch.empty((2, n), dtype=torch.float64, device=Xr.device)

        def launch(start, reps, ir, jf, ws):
            _lib.sinkhorn(Xr, Xf, ir, jf, reps, p, eps, n_sinkhorn, out[0, start:start + reps], out[1, start:start + reps],
                          None, ws)

        _boot.replicates(nr, nf, Xr.device, n_iters, lambda r: _lib.sinkhorn_workspace_bytes(nr, nf, d, r), launch)
        return np.ascontiguousarray(out.cpu().numpy().T), eps


def _replicates(X_real, X_fake, n_iters=100, p=2, reg=0.1, epsilon=None, n_sinkhorn=100, standardize=False):
    """-> numpy float64 [n_iters, 2]: value and drift of every bootstrap replicate, the draws made from numpy's global
    generator as the reference's metrics make them"""
    _check(X_real, X_fake, n_iters, p, reg, epsilon, n_sinkhorn, standardize)
    return _run(X_real, X_fake, n_iters, p, reg, epsilon, n_sinkhorn, standardize)[0]


# per-replicate values of the public call, on the same draws: float64 [n_iters, 2] (value, drift)
REPLICATES = {"sinkhorn_divergence": _replicates}


def sinkhorn_divergence(X_real, X_fake, n_iters=100, p=2, reg=0.1, epsilon=None, n_sinkhorn=100, standardize=False):
    '''
    Calculates the debiased Sinkhorn divergence (entropic optimal transport) for real and fake samples, bootstrapped.

    Parameters:
    -----------
    X_real: array of shape [n_samples, n_features] (numpy, array-like or torch; a CUDA tensor stays on the device)
        Real sample.
    X_fake: array of shape [m_samples, n_features]
        Generated sample.
    n_iters: int
        The number of bootstrap iterations. Default = 100.
    p: int
        The cost is the Euclidean distance to the power p, 1 or 2. Default = 2.
    reg: float
        eps = reg * median^p, median being the median pairwise distance of the pooled samples as given. Default = 0.1.
    epsilon: None or float
        The entropic regularisation eps itself, in units of the cost; reg is then not used. Default = None.
    n_sinkhorn: int
        The number of averaged iterations before the final one. Default = 100.
    standardize: boolean
        If True, the StandardScaler fitted on the real sample is applied to both. Default = False.

    Return:
    -------
    (mean, std) of the replicates (np.std, ddof 0), numpy float64.

    Raises ValueError if epsilon is None and the median pairwise distance is 0.
    '''
    V = _replicates(X_real, X_fake, n_iters, p, reg, epsilon, n_sinkhorn, standardize)[:, 0]
    return V.mean(axis=0), V.std(axis=0)


def sinkhorn_divergence_full_sample(X_real, X_fake, p=2, reg=0.1, epsilon=None, n_sinkhorn=100, standardize=False):
    '''
    Calculates the debiased Sinkhorn divergence of the samples as given, with no resampling.  Nothing is drawn; numpy's
    generator is untouched.

    Parameters:
    -----------
    X_real, X_fake, p, reg, epsilon, n_sinkhorn, standardize: as sinkhorn_divergence.

    Return:
    -------
    Sinkhorn(value, epsilon, drift): the divergence, the eps it was computed with, and the largest change of a potential in the
    last averaged iteration (the convergence diagnostic, in units of the cost); numpy float64.
    '''
    _check(X_real, X_fake, 1, p, reg, epsilon, n_sinkhorn, standardize)
    ((value, drift),), eps = _run(X_real, X_fake, None, p, reg, epsilon, n_sinkhorn, standardize)
    return Sinkhorn(value, eps, drift)
