"""probaforms_amd.metrics.losses without a GPU: the float64 restatement (tests/pairgrad_numpy.py) against torch-CPU float64
autograd of the same formula at every shape the GPU test uses, the C header against the binding, the workspace query and the
argument statuses of pfm_pair_grad, and the argument checks of the public calls that need no device.

The autograd yardstick writes the energy distance as where(d2 > 0, sqrt(.), 0) (the square root is taken of 1 where d2 = 0, so
that the masked branch has a finite derivative and the pair adds the subgradient 0) and builds the weights in float64.  Both
sides sum the same terms in other orders, so they are compared within 1e-12 of the sum of the magnitudes of the terms, M for the
gradient's elements: the project's tolerance for float64 sums taken in another order.
"""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import pairgrad_numpy as pg  # noqa: E402
import native_libs  # noqa: E402
from probaforms_amd.metrics import _lib, losses  # noqa: E402

CSRC = os.path.join(ROOT, "probaforms_amd", "metrics", "csrc")
NEW = ("pfm_pair_grad_workspace_bytes", "pfm_pair_grad")


def autograd_loss_and_grad(Xr, Xf, sigmas, block=128):
    """torch-CPU float64 autograd of L = sum_ab w_a w_b g(d2_ab), a block of rows a at a time (the blocks' backward passes
    accumulate into Z.grad) -> (L, dL/dZ)"""
    Z = torch.from_numpy(np.concatenate([Xr, Xf], axis=0)).clone().requires_grad_(True)
    w = torch.from_numpy(pg.weights(len(Xr), len(Xf)))
    total = 0.0
    for a0 in range(0, Z.shape[0], block):
        diff = Z[a0:a0 + block, None, :] - Z[None, :, :]
        d2 = (diff * diff).sum(dim=2)
        if sigmas is None:
            pos = d2 > 0
            g = -torch.where(pos, torch.where(pos, d2, torch.ones_like(d2)).sqrt(), torch.zeros_like(d2))
        else:
            g = sum(torch.exp(-(1.0 / (2.0 * float(s) ** 2)) * d2) for s in sigmas)
        Lb = (w[a0:a0 + block, None] * w[None, :] * g).sum()
        Lb.backward()
        total += float(Lb.detach())
    return total, Z.grad.numpy()


@pytest.mark.parametrize("kind", pg.KINDS)
@pytest.mark.parametrize("case", pg.CASES + pg.HOST_ONLY_CASES, ids=pg.case_id)
def test_restatement_equals_torch_autograd(case, kind):
    Xr, Xf = pg.make(case)
    sigmas = pg.bandwidths(kind, case[2])
    L, Lmag, grad, M = pg.loss_and_grad(Xr, Xf, sigmas)
    L_t, grad_t = autograd_loss_and_grad(Xr, Xf, sigmas)
    assert np.isfinite(grad).all() and np.isfinite(grad_t).all() and np.isfinite(L)
    err = np.abs(grad - grad_t)
    print("value off by %.3g of its terms; gradient off by at most %.3g of M"
          % (abs(L - L_t) / Lmag, float((err / np.where(M > 0, M, 1.0)).max())))
    assert abs(L - L_t) <= pg.TOL * Lmag
    assert (err <= pg.TOL * M).all()


def test_restatement_on_hand_made_data():
    # one real row at 0, one fake row at (3, 4): D^2 = 2 * 5, dL/dz = 2 w_a w_b c (z_a - z_b) = +-2 (3, 4) / 5
    L, Lmag, grad, M = pg.loss_and_grad(np.zeros((1, 2)), np.array([[3.0, 4.0]]), None)
    assert L == 10.0 == Lmag and (M == np.abs(grad)).all()
    assert np.allclose(grad, [[-1.2, -1.6], [1.2, 1.6]], rtol=1e-15, atol=0)
    # a fake row on top of the real row: the subgradient 0, and a value of 0
    L, Lmag, grad, M = pg.loss_and_grad(np.ones((1, 3)), np.ones((1, 3)), None)
    assert L == 0.0 and (grad == 0.0).all() and (M == 0.0).all()
    # several bandwidths: the value and the gradient are the sums of the single-bandwidth ones
    Xr, Xf = pg.make((5, 4, 3, "plain"))
    one = [pg.loss_and_grad(Xr, Xf, [s]) for s in (0.7, 1.9)]
    both = pg.loss_and_grad(Xr, Xf, [0.7, 1.9])
    assert abs(both[0] - one[0][0] - one[1][0]) <= 1e-15 * both[1]
    assert (np.abs(both[2] - one[0][2] - one[1][2]) <= 1e-15 * both[3]).all()
    # duplicated fake rows add exactly 0 to each other: their gradients are the same bits
    Xr, Xf = pg.make((65, 63, 17, "copies"))
    grad = pg.loss_and_grad(Xr, Xf, None)[2]
    assert (grad[65 + 1] == grad[65 + 2]).all() and np.isfinite(grad).all()


# ---- header, binding, statuses ------------------------------------------------------------------------------

def test_header_declarations_equal_the_binding():
    raw = open(os.path.join(CSRC, "pf_metrics.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = re.findall(r"\b(pfm_[a-z0-9_]+)\s*\(", text)
    assert sorted(declared) == sorted(_lib.EXPORTS) and set(NEW) <= set(_lib.EXPORTS)
    assert "#define PFM_VERSION %d " % _lib.ABI_VERSION in raw and _lib.ABI_VERSION == 101       # no argument list changed
    assert re.search(r"#define PFM_PAIR_MAX_GAMMAS %d\s" % _lib.PAIR_MAX_GAMMAS, raw) and _lib.PAIR_MAX_GAMMAS == 8
    assert "pf_pairgrad.o" in open(os.path.join(CSRC, "Makefile")).read()
    assert "atomic" not in re.sub(r"//.*", "", open(os.path.join(CSRC, "pf_pairgrad.hip")).read())


def test_workspace_query_and_argument_statuses_without_a_device():
    native_libs.ensure_built(_lib)
    q = _lib.pair_grad_workspace_bytes
    assert q(2, 1, 1) > 0 and q(20000, 16, 10000) > 0 and q(2200, 33, 1200) > 0
    for bad in ((1, 1, 1), (0, 1, 0), (10, 0, 5), (10, 2, 0), (10, 2, 10), (10, 2, -1), (2 ** 31, 2, 1), (2 ** 30, 2 ** 40, 1)):
        assert q(*bad) == 0, bad
    # the slices' partials [slices, n, d] and a value per workgroup: nothing of the size of the pair matrix
    assert q(20000, 16, 10000) <= 8 * 20000 * 16 * 8 and q(20000, 2, 10000) <= 8 * 20000 * 2 * 8
    assert q(2200, 2, 1200) == q(2200, 2, 7)                      # a function of (n, d) only
    L, fake = _lib.lib(), ctypes.c_void_p(256)
    one = (ctypes.c_double * 8)(*([0.5] * 8))

    def call(kind=_lib.PERM_GAUSS, gammas=one, ng=1, Z=fake, n=10, d=2, nfirst=4, value=fake, grad=fake, ws=fake,
             nbytes=1 << 20):
        return L.pfm_pair_grad(None, kind, ctypes.cast(gammas, ctypes.c_void_p) if gammas is not None else None, ng, Z, n, d,
                               nfirst, value, grad, ws, nbytes)

    # refused before anything is read or launched (the device pointers are never dereferenced)
    assert call(Z=None) == _lib.PFM_EINVAL and call(value=None) == _lib.PFM_EINVAL
    assert call(n=1, nfirst=1) == _lib.PFM_EINVAL and call(d=0) == _lib.PFM_EINVAL
    assert call(nfirst=0) == _lib.PFM_EINVAL and call(nfirst=10) == _lib.PFM_EINVAL and call(n=2 ** 31) == _lib.PFM_EINVAL
    assert call(kind=2) == _lib.PFM_EUNSUPPORTED and call(kind=-1) == _lib.PFM_EUNSUPPORTED
    assert call(ng=0) == _lib.PFM_EINVAL and call(ng=9) == _lib.PFM_EINVAL and call(gammas=None) == _lib.PFM_EINVAL
    for g in (0.0, -1.0, float("inf"), float("nan")):
        assert call(gammas=(ctypes.c_double * 2)(0.5, g), ng=2) == _lib.PFM_EINVAL, g
    assert call(ws=None) == _lib.PFM_EWORKSPACE and call(nbytes=q(10, 2, 4) - 1) == _lib.PFM_EWORKSPACE
    assert call(kind=_lib.PERM_ENERGY, gammas=None, ng=0, nbytes=q(10, 2, 4) - 1) == _lib.PFM_EWORKSPACE


# ---- the public calls' argument checks ---------------------------------------------------------------------

def test_argument_errors_need_no_device():
    X, Y = np.zeros((5, 3)), np.ones((4, 3))
    for fn in (losses.energy_loss, losses.mmd_loss):
        with pytest.raises(ValueError, match="different numbers of features"):
            fn(X, np.ones((4, 2)))
        with pytest.raises(ValueError, match="2-D"):
            fn(X[:, 0], Y)
        with pytest.raises(ValueError, match="2-D"):
            fn(torch.zeros(5, 3), torch.zeros(4))
        with pytest.raises(ValueError, match="real numeric"):
            fn(X.astype(complex), Y)
        for bad in (1, 0, None, "yes", np.array([True])):
            with pytest.raises(ValueError, match="standardize must be a bool"):
                fn(X, Y, standardize=bad)
    for bad in (0, 0.0, -1.0, float("inf"), float("nan"), True, "1", [], (), [1.0] * 9, [1.0, 0.0], [1.0, -2.0], [[1.0]],
                np.zeros(0), torch.ones(1), 1e-200):
        with pytest.raises(ValueError, match="bandwidth|gamma"):
            losses.mmd_loss(X, Y, bandwidth=bad)
    assert losses._gammas(2.0) == [0.125] and losses._gammas([1.0, 2]) == [0.5, 0.125]
    assert losses._gammas(np.array([1.0] * 8)) == [0.5] * 8 and losses._gammas(np.float32(1)) == [0.5]


def test_module_stays_out_of_the_export_list():
    import probaforms_amd.metrics as m
    assert m.__all__ == ["frechet_distance", "maximum_mean_discrepancy"]
    assert not hasattr(m, "energy_loss") and not hasattr(m, "mmd_loss")
