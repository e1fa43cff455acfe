"""energy_loss, mmd_loss: the two closed-form two-sample statistics as differentiable losses on the GPU (kernel:
csrc/pf_pairgrad.hip, pfm_pair_grad; host side: _boot.py, _m1d.py, twosample.py).  The reference has no such loss; the
arguments follow energy_distance and mmd_test, real sample first.

Pool Z = [X_real; X_fake] (N = nr + nf rows), w[a] = +1 / nr on a real row and -1 / nf on a fake one, d2(a, b) the squared
distance every kernel of the library forms.  Then
  L       = sum_ab w[a] w[b] g(d2(a, b))
  dL/dz_a = 2 w[a] sum_b w[b] c(d2(a, b)) (z_a - z_b)
  energy_loss   g = -sqrt(d2), c = -1 / sqrt(d2) and exactly 0 where d2 = 0: L is energy_distance_full_sample(squared=True),
                the V-statistic D^2 (not D: sqrt has no finite derivative at 0)
  mmd_loss      g = sum_m exp(-gamma_m d2), c = -2 sum_m gamma_m exp(-gamma_m d2), gamma_m = 1 / (2 sigma_m^2): L is the biased
                MMD^2 of mmd_test (diagonals included); with several bandwidths the kernel is the sum of the Gaussians
The kernel forms the value and the [N, d] row gradients in ONE sweep over the pair tiles; nothing of the size of the pair
matrix is stored, for the forward or for the backward.  The difference z_a - z_b is taken on the rows themselves: a generated
row that copies a real row gets a finite gradient, duplicated rows add exactly 0 to each other, and samples centred far from the
origin lose nothing.

The result is a 0-d float64 tensor on the device.  backward() fills .grad of whichever inputs require one: the node is a
torch.autograd.Function (once differentiable) whose forward keeps the row gradients and whose backward scales and splits them.
With no input requiring a gradient only the value is formed and the result has no grad_fn.

Inputs may be numpy arrays, array-likes or torch tensors; a CUDA tensor stays on its device, slices and other views are taken
as they are, and float32 is upcast with a torch op, so its gradient comes back as float32.  NO finiteness check of the contents
is made (it would be a host synchronisation in every training step): NaN and infinity propagate into the value and the
gradient.  Shape and dtype errors, a bad bandwidth and a non-bool standardize raise ValueError before anything is launched.
With tensors on the device and a given bandwidth, forward and backward only enqueue work: nothing waits for the device.
Importing this module needs no GPU.

sinkhorn_loss is the member of the family in between, the debiased Sinkhorn divergence of sinkhorn.py with a backward()
(kernels: csrc/pf_sinkgrad.hip, pfm_sinkhorn_grad): its gradient is the envelope-theorem gradient, exact at the fixed point of
the iteration and NOT the derivative of the unrolled steps; see its docstring and `drift`.

sliced_wasserstein_loss and wasserstein_1d_loss are the sort-based members (kernels: csrc/pf_slicegrad.hip, pfm_slice_grad): per
direction each sample's projections are sorted by (value, row) in LDS and coupled by quantiles, O(P n log n) where the three above
walk n^2 pairs.  The value is mean_k W_p^p without the p-th root, for the reason energy_loss returns D^2.

energy_score_loss and crps_loss are the CONDITIONAL members (kernel: csrc/pf_scoregrad.hip, pfm_score_grad): per condition row the
energy score (Gneiting & Raftery 2007) of the row's K draws against the row's observed target, the strictly proper scoring rule
sample_joint_scores and sample_scores report as metrics, with a backward().  The four above compare two pooled samples; these give
every row its own signal and cost K^2 pairs per row, not n^2.  Value and gradients come from one sweep over each row's pairs in LDS;
nothing of size K^2 is stored, for the forward or for the backward.

variogram_score_loss is the third conditional member (kernel: csrc/pf_variogram.hip, pfm_variogram_grad): per condition row the
variogram score (Scheuerer & Hamill 2015) of the row's K draws against the row's target, the `variogram` of sample_joint_scores
with a backward().  The energy score hardly separates predictive laws that differ only in the dependence between the features and
the CRPS is blind to it; the variogram score reacts to it, and is trained as energy_score_loss + lambda * variogram_score_loss.  A
row's d (d - 1) / 2 pair terms stay in LDS beside its draws: nothing of size K d^2 or n d^2 is stored, for the forward or for the
backward.

crps_loss(method="sorted") and pinball_loss are the sort-based conditional members (kernels: csrc/pf_sortscore.hip, pfm_sort_score
and pfm_pinball_grad): every (row, feature) series of draws is sorted by (value, draw) in LDS and scored in one pass, O(K log^2 K)
per series where the pair walk costs K^2 / 2, for up to 8192 draws.  Once the series is sorted the derivative of the CRPS by a draw is
a ratio of integers taken from the draw's rank, and the derivative of an empirical quantile touches two order statistics.

frechet_loss is the moment-matching member (kernels: csrc/pf_frechet.hip, pfm_frechet_grad): the Frechet distance of fd.py between the
two samples' Gaussians, O(n d^2) where energy_loss and mmd_loss walk n^2 pairs, for at most 64 features.  The trace of the matrix
square root is a spectral function of M = sym(S C_f S), S = C_r^(1/2): its derivative is tr(f'(M) dM), so the backward needs two
symmetric eigen-decompositions per route (Jacobi, one workgroup, in LDS) and NO eigenvector derivative, whose 1 / (lambda_i - lambda_j)
terms blow up for close eigenvalues.  With device tensors forward and backward only enqueue work.
"""
import math

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import _boot, _lib, _m1d

NAMES = ("X_real", "X_fake")
MAX_PROJECTIONS = 65535                  # pfm_slice_grad's n_proj: the directions are a grid dimension
_MAX_LDS_ROWS = _lib.SLICE_LDS_ROWS      # rows per sample up to which pfm_slice_grad sorts itself; above, torch.sort and perm_in


class PooledLossFunction(torch.autograd.Function):
    """A scalar loss of the pooled rows Z = [Xr; Xf] as one autograd node: the node of energy_loss / mmd_loss (pfm_pair_grad),
    sinkhorn_loss (pfm_sinkhorn_grad) and sliced_wasserstein_loss / wasserstein_1d_loss (pfm_slice_grad).

    call(Z, nr, want_rows) runs the loss's entry point once and returns (value 0-d, rows = dL/dZ [N, d] or None, further 0-d
    outputs ...): _pair_call, _sinkhorn_call, _slice_call or _frechet_call with the loss's constants bound.
    forward : the call; rows is kept if an input requires a gradient; -> (value, further outputs ...), the further ones (the
              Sinkhorn drift) marked non-differentiable
    backward: dL/dZ times the incoming scalar, split into the real and the fake rows"""

    @staticmethod
    def forward(ctx, call, Xr, Xf):
        ctx.nr = Xr.shape[0]
        want = ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        Z = torch.cat([Xr.detach(), Xf.detach()], dim=0).contiguous()
        value, rows, *more = call(Z, ctx.nr, want)
        ctx.mark_non_differentiable(*more)
        if want:
            ctx.save_for_backward(rows)
        return (value, *more)

    @staticmethod
    @once_differentiable
    def backward(ctx, gL, *_):
        (rows,) = ctx.saved_tensors
        G = rows * gL
        return None, G[:ctx.nr] if ctx.needs_input_grad[1] else None, G[ctx.nr:] if ctx.needs_input_grad[2] else None


def _outputs(Z, want_rows, workspace_bytes):
    """what every pooled entry point fills: (value 0-d, rows [N, d] or None, the workspace)"""
    return (torch.empty((), dtype=torch.float64, device=Z.device), torch.empty_like(Z) if want_rows else None,
            torch.empty(workspace_bytes, dtype=torch.uint8, device=Z.device))


def _pair_call(kind, gammas, Z, nr, want_rows):
    """pfm_pair_grad once on the pooled rows Z [N, d] (float64, contiguous, on the device): -> (value 0-d, rows [N, d] or None)"""
    value, rows, ws = _outputs(Z, want_rows, _lib.pair_grad_workspace_bytes(Z.shape[0], Z.shape[1], nr))
    _lib.pair_grad(kind, gammas, Z, nr, value, rows, ws)
    return value, rows


def _sinkhorn_call(p, eps, n_sinkhorn, Z, nr, want_rows):
    """pfm_sinkhorn_grad once, as _pair_call: -> (value 0-d, the envelope-theorem rows [N, d] or None, drift 0-d)"""
    value, rows, ws = _outputs(Z, want_rows, _lib.sinkhorn_grad_workspace_bytes(Z.shape[0], Z.shape[1], nr))
    drift = torch.empty_like(value)
    _lib.sinkhorn_grad(Z, nr, p, eps, n_sinkhorn, value, drift, rows, None, ws)
    return value, rows, drift


def _given_order(Z, nr, theta):
    """int32 [P, N]: per direction the real rows in stable ascending order of their projections, then the fake rows, as pooled
    row indices (pfm_slice_grad's perm_in).  pfm_project forms the projections the kernel forms: the same order, the same bytes"""
    if theta is None:
        cols = Z.t().contiguous()
    else:
        cols = torch.empty((theta.shape[0], Z.shape[0]), dtype=torch.float64, device=Z.device)
        _lib.project(Z[:nr], Z[nr:], theta, cols)
    first = torch.sort(cols[:, :nr], dim=1, stable=True)[1]
    second = torch.sort(cols[:, nr:], dim=1, stable=True)[1] + nr
    return torch.cat([first, second], dim=1).to(torch.int32).contiguous()


def _slice_call(p, Z, nr, theta, want_rows, cols_out=None, perm_out=None):
    """pfm_slice_grad once, as _pair_call: -> (value 0-d, rows [N, d] or None).  theta [P, d] on the device or None (the
    coordinate axes), a constant.  A sample above _MAX_LDS_ROWS is ordered by torch.sort"""
    N, d = Z.shape
    P = d if theta is None else theta.shape[0]
    perm_in = _given_order(Z, nr, theta) if max(nr, N - nr) > _MAX_LDS_ROWS else None
    value, rows, ws = _outputs(Z, want_rows, _lib.slice_grad_workspace_bytes(N, d, nr, P))
    _lib.slice_grad(p, Z, nr, theta, P, perm_in, value, rows, cols_out, perm_out, ws)
    return value, rows


class ScoreFunction(torch.autograd.Function):
    """The per-row energy scores [n] of the draws X [K, n, d] against the targets Y [n, d] as one autograd node.

    forward : pfm_score_grad once: the scores and, for whichever of X and Y requires a gradient, the unscaled per-row derivatives
              d scores[i] / d X[:, i, :] and d scores[i] / d Y[i, :], which are kept
    backward: those times the incoming [n] vector"""

    @staticmethod
    def forward(ctx, fair, X, Y):
        X, Y = X.detach(), Y.detach()
        scores = torch.empty(X.shape[1], dtype=torch.float64, device=X.device)
        gx = torch.empty_like(X) if ctx.needs_input_grad[1] else None
        gy = torch.empty_like(Y) if ctx.needs_input_grad[2] else None
        ws = torch.empty(_lib.score_grad_workspace_bytes(X.shape[1], X.shape[0], X.shape[2]), dtype=torch.uint8, device=X.device)
        _lib.score_grad(X, Y, fair, scores, None, gx, gy, ws)
        ctx.save_for_backward(gx, gy)
        return scores

    @staticmethod
    @once_differentiable
    def backward(ctx, gS):
        gx, gy = ctx.saved_tensors
        return (None, gx * gS[None, :, None] if ctx.needs_input_grad[1] else None,
                gy * gS[:, None] if ctx.needs_input_grad[2] else None)


class VariogramFunction(torch.autograd.Function):
    """The per-row variogram scores [n] of the draws X [K, n, d] against the targets Y [n, d] as one autograd node.

    forward : pfm_variogram_grad once: the scores and, for whichever of X and Y requires a gradient, the unscaled per-row derivatives
              d scores[i] / d X[:, i, :] and d scores[i] / d Y[i, :], which are kept; order and the weights W [d, d] (or None)
              are constants
    backward: those times the incoming [n] vector"""

    @staticmethod
    def forward(ctx, order, W, X, Y):
        X, Y = X.detach(), Y.detach()
        scores = torch.empty(X.shape[1], dtype=torch.float64, device=X.device)
        gx = torch.empty_like(X) if ctx.needs_input_grad[2] else None
        gy = torch.empty_like(Y) if ctx.needs_input_grad[3] else None
        ws = torch.empty(_lib.variogram_grad_workspace_bytes(X.shape[1], X.shape[0], X.shape[2]), dtype=torch.uint8,
                         device=X.device)
        _lib.variogram_grad(X, Y, W, order, scores, gx, gy, ws)
        ctx.save_for_backward(gx, gy)
        return scores

    @staticmethod
    @once_differentiable
    def backward(ctx, gS):
        gx, gy = ctx.saved_tensors
        return (None, None, gx * gS[None, :, None] if ctx.needs_input_grad[2] else None,
                gy * gS[:, None] if ctx.needs_input_grad[3] else None)


class SortedCrpsFunction(torch.autograd.Function):
    """The CRPS [M] of the draws X [K, M] against the targets Y [M] from the sorted series, as one autograd node.

    forward : pfm_sort_score once: the scores and, for whichever of X and Y requires a gradient, the unscaled derivatives
              d crps[s] / d X[:, s] and d crps[s] / d Y[s], which are kept
    backward: those times the incoming [M] vector"""

    @staticmethod
    def forward(ctx, fair, X, Y):
        X, Y = X.detach(), Y.detach()
        scores = torch.empty(X.shape[1], dtype=torch.float64, device=X.device)
        gx = torch.empty_like(X) if ctx.needs_input_grad[1] else None
        gy = torch.empty_like(Y) if ctx.needs_input_grad[2] else None
        ws = torch.empty(_lib.sort_score_workspace_bytes(X.shape[1], X.shape[0]), dtype=torch.uint8, device=X.device)
        _lib.sort_score(X, Y, fair, (), scores, gx, gy, None, None, None, ws)
        ctx.save_for_backward(gx, gy)
        return scores

    @staticmethod
    @once_differentiable
    def backward(ctx, gS):
        gx, gy = ctx.saved_tensors
        return None, gx * gS[None, :] if ctx.needs_input_grad[1] else None, gy * gS if ctx.needs_input_grad[2] else None


class PinballFunction(torch.autograd.Function):
    """The pinball scores [Q, M] of the empirical quantiles of the draws X [K, M] at the levels (a tuple of Q floats, constants)
    against the targets Y [M], as one autograd node.

    forward : pfm_sort_score once: the scores and, if X or Y requires a gradient, per level and series the two draws the quantile
              lies between (idx) and side = p - [y < Q_p], which are kept: 2 Q M numbers, not K M
    backward: pfm_pinball_grad once: the incoming [Q, M] weights go to those two draws and to the target"""

    @staticmethod
    def forward(ctx, levels, X, Y):
        X, Y = X.detach(), Y.detach()
        K, M = X.shape
        Q = len(levels)
        want = ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        pin = torch.empty((Q, M), dtype=torch.float64, device=X.device)
        side = torch.empty_like(pin) if want else None
        idx = torch.empty((Q, M, 2), dtype=torch.int32, device=X.device) if want else None
        ws = torch.empty(_lib.sort_score_workspace_bytes(M, K, Q), dtype=torch.uint8, device=X.device)
        _lib.sort_score(X, Y, False, levels, None, None, None, pin, side, idx, ws)
        ctx.levels, ctx.K = levels, K
        ctx.save_for_backward(idx, side)
        return pin

    @staticmethod
    @once_differentiable
    def backward(ctx, gP):
        idx, side = ctx.saved_tensors
        Q, M = side.shape
        gx = torch.empty((ctx.K, M), dtype=torch.float64, device=side.device) if ctx.needs_input_grad[1] else None
        gy = torch.empty(M, dtype=torch.float64, device=side.device) if ctx.needs_input_grad[2] else None
        ws = torch.empty(_lib.sort_score_workspace_bytes(M, ctx.K, Q), dtype=torch.uint8, device=side.device)
        with torch.cuda.device(side.device):
            _lib.pinball_grad(idx, side, gP.contiguous(), ctx.levels, ctx.K, gx, gy, ws)
        return None, gx, gy


def _frechet_call(rcond, sides, Z, nr, want_rows, outputs=None):
    """pfm_frechet_grad once, as _pair_call: -> (value 0-d, rows [N, d] or None, rank 0-d int32).  sides: bit 0 the real rows'
    gradient, bit 1 the fake rows' (only what is asked for is formed: with a constant real sample one route runs).  outputs: None or
    a dict that receives parts [5], eig [d], rank [2] and the workspace"""
    N, d = Z.shape
    value, rows, ws = _outputs(Z, want_rows, _lib.frechet_grad_workspace_bytes(N, d, nr))
    rank = torch.empty(2, dtype=torch.int32, device=Z.device)
    parts = eig = None
    if outputs is not None:
        parts, eig = torch.empty(5, dtype=torch.float64, device=Z.device), torch.empty(d, dtype=torch.float64, device=Z.device)
        outputs.update(parts=parts, eig=eig, rank=rank, workspace=ws)
    _lib.frechet_grad(Z, nr, rcond, sides if want_rows else 0, value, rows, parts, eig, rank, ws)
    return value, rows, rank[0]


def _frechet_shapes(X_real, X_fake):
    """(nr, nf, d) after the shape and dtype checks and the limits of pfm_frechet_grad, before anything touches a device"""
    d = _features(X_real, X_fake)
    nr, nf = _boot._check_2d(X_real, NAMES[0])[1][0], _boot._check_2d(X_fake, NAMES[1])[1][0]
    if d > _lib.FRECHET_MAX_D:
        raise ValueError("at most %d features, got %d (there is no fallback)" % (_lib.FRECHET_MAX_D, d))
    if nr < 2 or nf < 2:
        raise ValueError("both samples need at least 2 rows (the covariance divides by n - 1), got %d and %d" % (nr, nf))
    return nr, nf, d


def _rcond(rcond, d):
    """None -> d 2^-52 (numpy's matrix_rank / Hermitian pinv: max(M, N) eps); else a float in [0, 1)"""
    if rcond is None:
        return d * 2.0 ** -52
    number = isinstance(rcond, (int, float, np.integer, np.floating)) and not isinstance(rcond, (bool, np.bool_))
    if not number or not 0.0 <= float(rcond) < 1.0:
        raise ValueError("rcond must be None or a number in [0, 1), got %r" % (rcond,))
    return float(rcond)


def frechet_loss(X_real, X_fake, standardize=False, rcond=None, return_rank=False):
    '''
    The Frechet distance between real and fake samples as a differentiable loss: the value of frechet_distance_full_sample,
    FD = |mu_r - mu_f|^2 + tr C_r + tr C_f - 2 tr (C_r C_f)^(1/2) with the np.cov covariances (ddof 1). Moment matching is the
    cheapest two-sample training signal: O(n d^2), where energy_loss and mmd_loss walk n^2 pairs.

    The trace term is sum_i sqrt(max(lambda_i, 0)) over the eigenvalues of M = sym(S C_f S), S = C_r^(1/2) (fd.trace_sqrtm). It is a
    spectral function of M, so its derivative is tr(f'(M) dM): with M^(-1/2)_cut = V diag(c_i) V^T, c_i = lambda_i^(-1/2) where
    lambda_i > rcond * lambda_max and exactly 0 otherwise,
      dFD/dC_f = I - S M^(-1/2)_cut S,   dFD/dC_r the same with the samples swapped,
      dFD/dz_a = (2 / n_s) (mu_s - mu_o) + (2 / (n_s - 1)) dFD/dC_s (z_a - mu_s)      for row a of sample s, o the other sample.
    No eigenvector derivative appears: repeated or close eigenvalues are no special case. A cut eigenvalue adds the subgradient 0.

    **An eigenvalue of rounding noise just above the cut gives gradient elements of order 1 / sqrt(rcond * lambda_max).** With
    n <= d or collinear features the covariance is singular and its zero eigenvalues come out as +-1e-16 lambda_max: pass a larger
    rcond (1e-10, say) and look at rank (return_rank=True).

    Parameters:
    -----------
    X_real, X_fake, standardize: as energy_loss; at least 2 rows each and at most 64 features.
    rcond: None or float in [0, 1)
        The relative cut of the eigenvalues in the gradient. Default = None: n_features * 2^-52, numpy's convention for
        matrix_rank and the Hermitian pinv. It is a constant, and it does not enter the value.
    return_rank: boolean
        If True, (loss, rank) is returned, rank a 0-d int32 tensor on the device without a grad_fn: the eigenvalues of M the cut
        kept (n_features for non-singular data; reading it waits for the device, the call does not). Default = False.

    Return:
    -------
    0-d float64 tensor on the device, as energy_loss; only the gradients of the inputs that require one are formed (with a
    constant real sample one of the two routes runs), and with none only the value. The contents are not checked: a NaN anywhere
    makes the value and every gradient element NaN. With device tensors forward and backward only enqueue work.

    Raises ValueError for more than 64 features (there is no fallback), fewer than 2 rows in a sample, a bad rcond and non-bool flags.
    '''
    _m1d.check_bool(standardize, "standardize")
    _m1d.check_bool(return_rank, "return_rank")
    d = _frechet_shapes(X_real, X_fake)[2]
    rc = _rcond(rcond, d)
    Xr, Xf = _pooled_inputs(X_real, X_fake, standardize)
    with torch.cuda.device(Xr.device):
        sides = (1 if Xr.requires_grad else 0) | (2 if Xf.requires_grad else 0)
        value, rank = PooledLossFunction.apply(lambda Z, nr, want: _frechet_call(rc, sides, Z, nr, want), Xr, Xf)
    return (value, rank) if return_rank else value


def _gammas(bandwidth):
    """a positive float or a sequence of 1 .. 8 of them -> the list of gamma = 1 / (2 sigma^2)"""
    if not isinstance(bandwidth, (list, tuple)) and not (isinstance(bandwidth, np.ndarray) and bandwidth.ndim == 1):
        sigmas = [bandwidth]
    else:
        sigmas = list(bandwidth)
        if not 1 <= len(sigmas) <= _lib.PAIR_MAX_GAMMAS:
            raise ValueError("bandwidth must be a positive finite number or a sequence of 1 to %d of them, got %d values"
                             % (_lib.PAIR_MAX_GAMMAS, len(sigmas)))
    out = []
    for s in sigmas:
        _m1d.check_positive(s, "bandwidth")
        sq = 2 * float(s) ** 2
        gamma = 1.0 / sq if sq > 0 else math.inf
        if not (math.isfinite(gamma) and gamma > 0):
            raise ValueError("gamma = 1 / (2 sigma^2) is not a positive finite number for sigma = %r" % (s,))
        out.append(gamma)
    return out


def _pooled_inputs(X_real, X_fake, standardize):
    """the two samples as float64 tensors on one HIP device, in their autograd graph: the scaler runs as plain torch ops, so
    autograd carries its derivative, and the upcast's"""
    Xr, Xf = _boot.prepare(X_real, X_fake, NAMES, 1, standardize, graph=True)
    if Xr.shape[0] + Xf.shape[0] >= 2 ** 31:
        raise ValueError("at most 2**31 - 1 pooled samples, got %d" % (Xr.shape[0] + Xf.shape[0]))
    return Xr, Xf


def _order_p(p):
    if not _m1d.is_int(p) or p not in (1, 2):
        raise ValueError("p must be 1 or 2, got %r" % (p,))
    return int(p)


def _loss(kind, X_real, X_fake, bandwidth, standardize):
    _m1d.check_bool(standardize, "standardize")
    gammas = [] if kind == _lib.PERM_ENERGY or bandwidth is None else _gammas(bandwidth)
    Xr, Xf = _pooled_inputs(X_real, X_fake, standardize)
    with torch.cuda.device(Xr.device):
        if kind == _lib.PERM_GAUSS and bandwidth is None:
            from . import twosample                    # (the permutation tests; imported where the median is asked for)
            sigma = twosample._median(Xr.detach(), Xf.detach())          # one host read-back
            if not sigma > 0:
                raise ValueError("the median pairwise distance is 0, so gamma = 1 / (2 median^2) is infinite (too few "
                                 "distinct rows)")
            gammas = _gammas(sigma)
        return PooledLossFunction.apply(lambda Z, nr, want: _pair_call(kind, gammas, Z, nr, want), Xr, Xf)[0]


def energy_loss(X_real, X_fake, standardize=False):
    '''
    The squared energy distance (Szekely & Rizzo) between real and fake samples as a differentiable loss.
    D^2 = 2 E|X - Y| - E|X - X'| - E|Y - Y'| over all ordered pairs of rows (V-statistic), |.| the Euclidean norm: the value
    of energy_distance_full_sample(squared=True).

    Parameters:
    -----------
    X_real: array of shape [n_samples, n_features] (numpy, array-like or torch; a CUDA tensor stays on the device)
        Real sample.
    X_fake: array of shape [m_samples, n_features]
        Generated sample; for training, a tensor that requires a gradient (model.nf.sample(C), a generator's output).
    standardize: boolean
        If True, the StandardScaler fitted on the real sample is applied to both, as torch ops (the gradient passes through
        it). Default = False.

    Return:
    -------
    0-d float64 tensor on the device. backward() fills the gradients of the tensor inputs that require one; a coincident
    pair of rows adds the subgradient 0. The contents are not checked: NaN and infinity propagate.
    '''
    return _loss(_lib.PERM_ENERGY, X_real, X_fake, None, standardize)


def mmd_loss(X_real, X_fake, bandwidth=None, standardize=False):
    '''
    The biased squared Maximum Mean Discrepancy (RBF kernel) between real and fake samples as a differentiable loss:
    mean K_XX + mean K_YY - 2 mean K_XY, diagonals included, the statistic of mmd_test.

    Parameters:
    -----------
    X_real, X_fake, standardize: as energy_loss.
    bandwidth: None, float, or a sequence of 1 to 8 floats
        sigma of the kernel exp(-d^2 / (2 sigma^2)); with a sequence the kernel is the sum of the Gaussians (the multi-scale
        MMD loss), and the value the sum of the single-bandwidth values. Default = None: the median of the pooled distance
        matrix of the samples as given, as mmd_test takes it. That costs one read-back to the host per call; a training
        loop passes a number. The bandwidth is a constant: no gradient flows through it.

    Return:
    -------
    0-d float64 tensor on the device, as energy_loss.

    Raises ValueError if bandwidth is None and the median pairwise distance is 0.
    '''
    return _loss(_lib.PERM_GAUSS, X_real, X_fake, bandwidth, standardize)


def sinkhorn_loss(X_real, X_fake, p=2, reg=0.1, epsilon=None, n_sinkhorn=100, standardize=False, return_drift=False):
    '''
    The debiased Sinkhorn divergence (entropic optimal transport; Genevay et al. 2018, Feydy et al. 2019) between real and fake
    samples as a differentiable loss: the value of sinkhorn_divergence_full_sample (the same iteration with uniform weights; not
    bitwise, the sums run in another order), the member of the family between energy_loss / mmd_loss (large eps) and W_p^p
    (eps -> 0).

    The gradient is the envelope-theorem gradient (as GeomLoss takes it): every row's final softmin is differentiated by that
    row's own coordinates, the other rows and the incoming potentials held fixed.  That is the exact derivative of the value AT
    THE FIXED POINT of the iteration; it is NOT the derivative of the n_sinkhorn unrolled steps.  Far from convergence the two
    differ (by 10 - 30 % of the largest element at drift = 0.1 in units of the cost): ask for return_drift=True and watch drift,
    the largest change of a potential in the last averaged step.  Nothing of the size of the pair matrix is stored, for the
    forward or for the backward, and no graph of the steps is kept.

    Parameters:
    -----------
    X_real, X_fake, standardize: as energy_loss.
    p: int
        The cost is the Euclidean distance to the power p, 1 or 2. Default = 2. For p = 1 a coincident pair of rows adds the
        subgradient 0.
    reg: float
        eps = reg * median^p, median being the median pairwise distance of the pooled samples as given (after standardize).
        Default = 0.1.
    epsilon: None or float
        The entropic regularisation eps itself, in units of the cost; reg is then not used. Default = None: eps from the median,
        which costs one read-back to the host per call; a training loop passes a number. eps is a constant: no gradient flows
        through it.
    n_sinkhorn: int
        The number of averaged iterations before the final one, 0 .. 1000000. Default = 100.
    return_drift: boolean
        If True, (loss, drift) is returned, drift a 0-d float64 tensor on the device without a grad_fn (reading it waits for
        the device; the call does not). Default = False.

    Return:
    -------
    0-d float64 tensor on the device, as energy_loss; with no input requiring a gradient only the value is formed. The contents
    are not checked: NaN and infinity propagate.

    Raises ValueError if epsilon is None and the median pairwise distance is 0.
    '''
    from . import sinkhorn as _sk                      # (the metric: its limits and eps = reg * median^p; imports twosample)
    _m1d.check_bool(standardize, "standardize")
    _m1d.check_bool(return_drift, "return_drift")
    p = _order_p(p)
    _m1d.check_positive(reg, "reg", reciprocal=True)
    _m1d.check_positive(epsilon, "epsilon", none_ok=True, reciprocal=True)
    if not _m1d.is_int(n_sinkhorn) or not 0 <= n_sinkhorn <= _sk.MAX_SINKHORN:
        raise ValueError("n_sinkhorn must be an integer in 0 .. %d, got %r" % (_sk.MAX_SINKHORN, n_sinkhorn))
    Xr, Xf = _pooled_inputs(X_real, X_fake, standardize)
    with torch.cuda.device(Xr.device):
        if epsilon is None:
            eps = float(_sk.epsilon_of(_sk._median(Xr.detach(), Xf.detach()), p, reg))     # one host read-back
        else:
            eps = float(epsilon)
        n_sinkhorn = int(n_sinkhorn)
        value, drift = PooledLossFunction.apply(lambda Z, nr, want: _sinkhorn_call(p, eps, n_sinkhorn, Z, nr, want), Xr, Xf)
    return (value, drift) if return_drift else value


def _check_directions(directions, d):
    """shape and dtype checks on the caller's directions, before anything touches a device"""
    T, shape = _boot._check_2d(directions, "directions")
    if shape[1] != d or shape[0] > MAX_PROJECTIONS:
        raise ValueError("directions: expected shape (P, %d) with 1 <= P <= %d, got %s" % (d, MAX_PROJECTIONS, tuple(shape)))
    return T


def _features(X_real, X_fake):
    """the number of features, after the shape and dtype checks _boot.prepare makes first"""
    sa, sb = _boot._check_2d(X_real, NAMES[0])[1], _boot._check_2d(X_fake, NAMES[1])[1]
    if sa[1] != sb[1]:
        raise ValueError("%s and %s have different numbers of features: %d and %d" % (NAMES[0], NAMES[1], sa[1], sb[1]))
    return sa[1]


def sliced_wasserstein_loss(X_real, X_fake, n_projections=64, p=2, directions=None, standardize=False):
    '''
    The sliced Wasserstein distance between real and fake samples as a differentiable loss: the mean over the directions of
    W_p^p between the two samples' projections, WITHOUT the p-th root (sliced_wasserstein_full_sample takes it), for the reason
    energy_loss returns D^2. Per direction each sample's projections are sorted by (value, row) and coupled by quantiles: it
    costs O(P n log n) where energy_loss, mmd_loss and sinkhorn_loss walk n^2 pairs.

    Parameters:
    -----------
    X_real, X_fake, standardize: as energy_loss.
    n_projections: int
        The number of random unit directions, 1 .. 65535. Default = 64. They are ONE draw from numpy's global generator per
        call, np.random.normal(size=(n_projections, d)) with each row divided by its 2-norm: the draw
        sliced_wasserstein_distance makes first, so after the same np.random.seed both use the same directions.
    p: int
        The order, 1 or 2. Default = 2.
    directions: None, or an array or tensor of shape [P, d], 1 <= P <= 65535
        The directions themselves, used as given and not normalised; n_projections is then not used and nothing is drawn. A
        training loop that wants fresh directions every step without touching the host draws them on the device. The directions
        are constants: no gradient flows to them.

    Return:
    -------
    0-d float64 tensor on the device, as energy_loss; with no input requiring a gradient only the value is formed. Among tied
    projections the (value, row index) order decides which rows are matched: a valid subgradient, and deterministic; for
    p = 1 a coincident pair adds the subgradient 0. The contents are not checked: NaN propagates into the value. A sample of
    more than 13312 rows is ordered by torch.sort instead of the library's own sort; the result is the same bytes.
    '''
    _m1d.check_bool(standardize, "standardize")
    p = _order_p(p)
    if directions is None and (not _m1d.is_int(n_projections) or not 1 <= n_projections <= MAX_PROJECTIONS):
        raise ValueError("n_projections must be an integer in 1 .. %d, got %r" % (MAX_PROJECTIONS, n_projections))
    d = _features(X_real, X_fake)
    if directions is not None:
        directions = _check_directions(directions, d)
    Xr, Xf = _pooled_inputs(X_real, X_fake, standardize)
    with torch.cuda.device(Xr.device):
        if directions is None:
            from . import wasserstein                  # (the metric: its draw of the directions)
            directions = wasserstein.directions(int(n_projections), d)
        if not isinstance(directions, torch.Tensor):
            directions = torch.from_numpy(np.array(directions, dtype=np.float64))        # (a copy: the caller's may be read-only)
        theta = directions.detach().to(device=Xr.device, dtype=torch.float64).contiguous()
        return PooledLossFunction.apply(lambda Z, nr, want: _slice_call(p, Z, nr, theta, want), Xr, Xf)[0]


def wasserstein_1d_loss(X_real, X_fake, p=1):
    '''
    The 1-D Wasserstein distance of every feature as a differentiable loss: the mean over the features of W_p^p between the two
    samples' columns, without the p-th root (wasserstein_1d's statistic of the samples as given, for p = 1). Nothing is drawn.
    A column is the feature itself, copied: an infinity in one feature does not reach the other features' terms.

    Parameters:
    -----------
    X_real, X_fake: as energy_loss; at most 65535 features.
    p: int
        The order, 1 or 2. Default = 1.

    Return:
    -------
    0-d float64 tensor on the device, as sliced_wasserstein_loss.
    '''
    p = _order_p(p)
    d = _features(X_real, X_fake)
    if d > MAX_PROJECTIONS:
        raise ValueError("at most %d features, got %d" % (MAX_PROJECTIONS, d))
    Xr, Xf = _pooled_inputs(X_real, X_fake, False)
    with torch.cuda.device(Xr.device):
        return PooledLossFunction.apply(lambda Z, nr, want: _slice_call(p, Z, nr, None, want), Xr, Xf)[0]


def _check_nd(A, name, rank, what):
    """shape and dtype checks on the caller's object, before anything touches a device"""
    if isinstance(A, torch.Tensor):
        if A.is_complex() or A.dtype == torch.bool:
            raise ValueError("%s: expected a real numeric tensor, got %s" % (name, A.dtype))
        shape = tuple(A.shape)
    else:
        A = np.asarray(A)
        if A.dtype.kind not in "fiu":
            raise ValueError("%s: expected a real numeric array, got dtype %s" % (name, A.dtype))
        shape = A.shape
    if len(shape) != rank:
        raise ValueError("%s: expected a %d-D array %s, got shape %s" % (name, rank, what, tuple(shape)))
    if min(shape) < 1:
        raise ValueError("%s: expected at least one draw, one row and one feature, got shape %s" % (name, tuple(shape)))
    return A, tuple(shape)


def _score_inputs(X_draws, Y, fair, reduction, per_feature, weights=None, max_d=None, sort_route=False):
    """the checks, all before a device is touched -> (X [K, n, d], Y [n, d], Y's shape as given, weights): contiguous float64
    tensors on one HIP device, in their autograd graph; per_feature: every (row, feature) series becomes a row of one feature;
    weights: None or a real [d, d] constant, which comes back detached on the device; max_d: the most features taken; sort_route:
    the limits are pfm_sort_score's, not pfm_score_grad's"""
    _m1d.check_bool(fair, "fair")
    if reduction not in ("mean", "none"):
        raise ValueError("reduction must be 'mean' or 'none', got %r" % (reduction,))
    X, sx = _check_nd(X_draws, "X_draws", 3, "[n_draws, n_samples, n_features]")
    Yt, sy = _check_nd(Y, "Y", 2, "[n_samples, n_features]")
    K, n, d = sx
    if sy != (n, d):
        raise ValueError("X_draws and Y have different numbers of samples or features: %s and %s" % (sx, sy))
    if per_feature:
        n, d = n * d, 1
    if fair and K == 1:
        raise ValueError("fair=True needs at least 2 draws per row (the spread is divided by K - 1), got 1")
    if sort_route:
        if K > _lib.SORT_MAX_K:
            raise ValueError("at most %d draws per series, got %d" % (_lib.SORT_MAX_K, K))
    elif K > _lib.SCORE_MAX_K or K * d > _lib.SCORE_MAX_KD:
        raise ValueError("at most %d draws per row and %d draws times features, got K = %d, d = %d"
                         % (_lib.SCORE_MAX_K, _lib.SCORE_MAX_KD, K, d))
    if max_d is not None and d > max_d:
        raise ValueError("at most %d features, got %d" % (max_d, d))
    if n >= 2 ** 31:
        raise ValueError("at most 2**31 - 1 rows, got %d" % n)
    if weights is not None:
        try:
            weights, sw = _check_nd(weights, "weights", 2, "[n_features, n_features]")
        except (TypeError, ValueError) as e:
            raise ValueError("weights: expected None or a real numeric array of shape (%d, %d): %s" % (d, d, e)) from None
        if sw != (d, d):
            raise ValueError("weights: expected shape (%d, %d), got %s" % (d, d, sw))
    if not torch.cuda.is_available():
        raise RuntimeError("probaforms_amd.metrics runs on a HIP device and none is visible (there is no CPU fallback)")
    dev = next((t.device for t in (X, Yt) if isinstance(t, torch.Tensor) and t.is_cuda),
               torch.device("cuda", torch.cuda.current_device()))

    def dev64(t, shape):
        if not isinstance(t, torch.Tensor):
            t = torch.from_numpy(np.array(t, dtype=np.float64))                      # (a copy: the caller's may be read-only)
        return t.to(device=dev, dtype=torch.float64).contiguous().reshape(shape)        # torch ops: the graph carries them
    return dev64(X, (K, n, d)), dev64(Yt, (n, d)), sy, None if weights is None else dev64(weights, (d, d)).detach()


def _score_loss(X_draws, Y, fair, reduction, per_feature):
    X, Yt, shape, _ = _score_inputs(X_draws, Y, fair, reduction, per_feature)
    with torch.cuda.device(X.device):
        scores = ScoreFunction.apply(bool(fair), X, Yt)
        if reduction == "mean":
            return scores.mean()
        return scores.reshape(shape) if per_feature else scores


def energy_score_loss(X_draws, Y, fair=True, reduction="mean"):
    '''
    The energy score (Gneiting & Raftery 2007) of K draws per condition row against the row's observed target, as a
    differentiable loss: per row ES = (1/K) sum_k |x_k - y| - 1/(2 K D) sum_k sum_l |x_k - x_l|, |.| the Euclidean norm, the
    `energy` of sample_joint_scores. Minimising its mean over a batch is a strictly proper objective for any conditional sampler
    (scoring-rule minimisation, "engression"): X_draws = model.nf.sample(C.repeat(K, 1)).view(K, n, d).

    Parameters:
    -----------
    X_draws: array of shape [n_draws, n_samples, n_features] (numpy, array-like or torch; a CUDA tensor stays on the device)
        Draw k of row i is X_draws[k, i], as sample_many returns them; for training, a tensor that requires a gradient. At most
        1024 draws and 16384 draws times features.
    Y: array of shape [n_samples, n_features]
        The observed targets.
    fair: boolean
        If True, D = K - 1 (the unbiased spread; needs K >= 2), else D = K. Default = True, which DIFFERS from
        sample_joint_scores, a metric: used as a loss, the biased D = K form halves the spread at K = 2 and trains
        under-dispersed samplers. fair=False with K = 1 is the mean Euclidean error.
    reduction: "mean" or "none"
        "mean": the mean over the rows, a 0-d tensor. "none": the [n_samples] per-row scores, for a weighted sum. Default =
        "mean".

    Return:
    -------
    float64 tensor on the device. backward() fills the gradients of whichever of X_draws and Y require one (float32 inputs get
    float32 gradients); with none only the scores are formed and the result has no grad_fn. A coincident pair of draws, or a
    draw equal to its target, adds the subgradient 0. The contents are not checked: a NaN in a row's draws or target makes
    that row's score and gradients NaN and touches no other row. With device tensors nothing waits for the device.
    '''
    return _score_loss(X_draws, Y, fair, reduction, False)


def _sorted_inputs(X_draws, Y, fair, reduction):
    """_score_inputs for the sorted route -> (X [K, M], Y [M], Y's shape as given): every (row, feature) series is a column"""
    X, Yt, shape, _ = _score_inputs(X_draws, Y, fair, reduction, True, sort_route=True)
    return X.reshape(X.shape[0], X.shape[1]), Yt.reshape(-1), shape


def crps_loss(X_draws, Y, fair=True, reduction="mean", method="pairs"):
    '''
    The continuous ranked probability score of K draws per condition row and feature against the observed value, as a
    differentiable loss: the energy score of every (row, feature) series on its own, at n_features = 1 the `crps` of
    sample_scores.

    method="pairs" is the same kernel call as energy_score_loss on X_draws.reshape(K, n d, 1) and Y.reshape(n d, 1): it walks the
    K (K - 1) / 2 pairs of every series, O(K^2), for at most 1024 draws.

    method="sorted" sorts every series by (value, draw) and takes the score and both derivatives from one pass over the sorted
    series, O(K log^2 K), for at most 8192 draws: with t = x - y sorted, crps = (1/K) sum_i |t_(i)| - 1/(K D) sum_i c_i t_(i) and
    d crps / d x_k = (sgn(t_k) D - c_k) / (K D), c_i being the number of draws strictly below t_(i) minus the number strictly above
    (2 i - K + 1 without ties). Tied draws and a draw on its target get the subgradient of the pair route (sgn(0) = 0). The two
    routes agree to rounding, not bitwise: their sums run in different orders. Nothing switches between them automatically.

    Parameters:
    -----------
    X_draws, Y, fair: as energy_score_loss; at most 1024 draws for method="pairs" and 8192 for method="sorted".
    reduction: "mean" or "none"
        "mean": the mean over rows and features, a 0-d tensor. "none": the [n_samples, n_features] scores. Default = "mean".
    method: "pairs" or "sorted"
        Default = "pairs".

    Return:
    -------
    float64 tensor on the device, as energy_score_loss. With method="sorted" a NaN in a series' draws or target makes that
    series' score and all its gradient elements NaN and touches no other series.

    Raises ValueError for another method and beyond the limits of the method asked for (there is no fallback).
    '''
    if method == "pairs":
        return _score_loss(X_draws, Y, fair, reduction, True)
    if method != "sorted":
        raise ValueError("method must be 'pairs' or 'sorted', got %r" % (method,))
    X, Yt, shape = _sorted_inputs(X_draws, Y, fair, reduction)
    with torch.cuda.device(X.device):
        scores = SortedCrpsFunction.apply(bool(fair), X, Yt)
        return scores.mean() if reduction == "mean" else scores.reshape(shape)


def _quantile_levels(quantiles):
    """a number or a sequence of 1 .. 16 of them in [0, 1] -> the tuple of floats"""
    seq = isinstance(quantiles, (list, tuple)) or (isinstance(quantiles, np.ndarray) and quantiles.ndim == 1)
    levels = list(quantiles) if seq else [quantiles]
    if not 1 <= len(levels) <= _lib.SORT_MAX_Q:
        raise ValueError("quantiles must be a number in [0, 1] or a sequence of 1 to %d of them, got %d values"
                         % (_lib.SORT_MAX_Q, len(levels)))
    for p in levels:
        number = isinstance(p, (int, float, np.integer, np.floating)) and not isinstance(p, (bool, np.bool_))
        if not number or not 0.0 <= float(p) <= 1.0:
            raise ValueError("quantiles must be numbers in [0, 1], got %r" % (p,))
    return tuple(float(p) for p in levels)


def pinball_loss(X_draws, Y, quantiles=(0.05, 0.95), reduction="mean"):
    '''
    The pinball (quantile) loss of the empirical quantiles of K draws per condition row and feature against the observed value, as a
    differentiable loss: per level p, (y - Q_p) (p - [y < Q_p]) with Q_p numpy's linear quantile of the series' draws, the `pinball`
    of sample_scores. It is the quantile-regression loss, and the CRPS is twice its integral over p: training on a few levels
    fits those quantiles of the sampler, e.g. the 5 % / 95 % band.

    Every series is sorted by (value, draw) as for crps_loss(method="sorted"). Q_p lies between two order statistics, h = p (K - 1),
    i = floor(h), frac = h - i: the derivative goes to those two draws, -(p - [y < Q_p]) (1 - frac) and -(p - [y < Q_p]) frac, and
    p - [y < Q_p] to the target. Among tied draws the (value, draw index) order names the two; y on Q_p counts as y >= Q_p.

    Parameters:
    -----------
    X_draws, Y: as energy_score_loss; at most 8192 draws, one draw is valid.
    quantiles: float, or a sequence of 1 to 16 floats in [0, 1]
        The levels p. Default = (0.05, 0.95). They are constants.
    reduction: "mean" or "none"
        "mean": the mean over levels, rows and features, a 0-d tensor. "none": the [n_levels, n_samples, n_features] scores.
        Default = "mean".

    Return:
    -------
    float64 tensor on the device. backward() fills the gradients of whichever of X_draws and Y require one (float32 inputs get
    float32 gradients); with none only the scores are formed and the result has no grad_fn. The contents are not checked: a NaN
    in a series' draws or target makes that series' scores NaN and touches no other series. With device tensors nothing waits for
    the device.

    Raises ValueError for no level, more than 16, a level outside [0, 1], and more than 8192 draws (there is no fallback).
    '''
    levels = _quantile_levels(quantiles)
    X, Yt, shape = _sorted_inputs(X_draws, Y, False, reduction)
    with torch.cuda.device(X.device):
        pin = PinballFunction.apply(levels, X, Yt)
        return pin.mean() if reduction == "mean" else pin.reshape((len(levels),) + shape)


def _variogram_order(order):
    number = isinstance(order, (int, float, np.integer, np.floating)) and not isinstance(order, (bool, np.bool_))
    if not number or float(order) not in (0.5, 1.0, 2.0):
        raise ValueError("order must be 0.5, 1 or 2, got %r" % (order,))
    return float(order)


def variogram_score_loss(X_draws, Y, order=0.5, weights=None, reduction="mean"):
    '''
    The variogram score (Scheuerer & Hamill 2015) of K draws per condition row against the row's observed target, as a
    differentiable loss: per row VS = sum_i sum_j w_ij (|y_i - y_j|^p - (1/K) sum_k |x_ki - x_kj|^p)^2, with unit weights the
    `variogram` of sample_joint_scores. It reacts to the dependence between the features, which the energy score hardly sees and
    the CRPS not at all; it does not see a shift of all features by one constant, so it is trained together with a proper score:
    energy_score_loss(X_draws, Y) + lam * variogram_score_loss(X_draws, Y).

    Parameters:
    -----------
    X_draws: array of shape [n_draws, n_samples, n_features] (numpy, array-like or torch; a CUDA tensor stays on the device)
        Draw k of row i is X_draws[k, i], as for energy_score_loss. At most 1024 draws, 16384 draws times features and 64 features;
        one draw is valid.
    Y: array of shape [n_samples, n_features]
        The observed targets.
    order: 0.5, 1 or 2 (int or float)
        The order p of the variogram. Default = 0.5, as sample_joint_scores. For p = 0.5 the derivative by a coordinate of a
        draw is sgn(t) / (2 sqrt|t|) of its differences t to the draw's other coordinates: it GROWS WITHOUT BOUND as two
        coordinates of a draw approach each other (and is taken as 0 where they are equal).
    weights: None, or an array or tensor of shape [n_features, n_features]
        w_ij, used as given: it need not be symmetric and may hold negative values. Default = None: all 1. The weights are
        constants: no gradient flows to them.
    reduction: "mean" or "none"
        "mean": the mean over the rows, a 0-d tensor. "none": the [n_samples] per-row scores, for a weighted sum. Default =
        "mean".

    Return:
    -------
    float64 tensor on the device. backward() fills the gradients of whichever of X_draws and Y require one (float32 inputs get
    float32 gradients); with none only the scores are formed and the result has no grad_fn. A tied pair of coordinates adds the
    subgradient 0; with one feature the score and both gradients are 0. The contents are not checked: a NaN in a row's draws or
    target makes that row's score and gradients NaN and touches no other row. With device tensors nothing waits for the device.

    Raises ValueError for an order other than 0.5, 1 or 2, for weights of another shape or dtype, and beyond the limits (there is
    no fallback).
    '''
    order = _variogram_order(order)
    X, Yt, _, W = _score_inputs(X_draws, Y, False, reduction, False, weights=weights, max_d=_lib.VARIO_MAX_D)
    with torch.cuda.device(X.device):
        scores = VariogramFunction.apply(order, W, X, Yt)
        return scores.mean() if reduction == "mean" else scores
