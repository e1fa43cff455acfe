"""probaforms_amd.metrics.losses.sinkhorn_loss without a GPU: the float64 restatement's gradient (tests/sinkhorn_grad_numpy.py)
against central differences of the restatement's own ITERATED value at converged configurations and against torch-CPU autograd of
the last step at the shapes where the GPU test crosses the sweep's axes, the C header against the binding, the workspace query and
the argument statuses of pfm_sinkhorn_grad, and the public call's argument checks.

The autograd yardstick reads the potentials of the restatement's own iteration and differentiates the last step alone, so both
sides sum the same terms in other orders: the value is held within 1e-12 cmax and a gradient element within 1e-12 M.

At drift <= 1e-13 the envelope-theorem gradient is the derivative of the whole iterated value: central differences with
h = 1e-5 carry a truncation error of about h^2 |S'''| / 6 ~ 1e-11 and a rounding error of about 1e-16 cmax / h ~ 1e-10, so
the two are held within 1e-8.  The variant that also differentiates the last step through its columns is twice the right
answer there, and is held to twice the central differences within the same bound: that is what the kernel must NOT compute.
"""
import ctypes
import functools
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import native_libs  # noqa: E402
import pairgrad_numpy as pg  # noqa: E402
import sinkhorn_grad_numpy as sg  # noqa: E402
import sinkhorn_numpy as sn  # noqa: E402
from probaforms_amd.metrics import _lib, losses  # noqa: E402

CSRC = os.path.join(ROOT, "probaforms_amd", "metrics", "csrc")
NEW = ("pfm_sinkhorn_grad_workspace_bytes", "pfm_sinkhorn_grad")
H, FD_TOL, DRIFT = 1e-5, 1e-8, 1e-13


@functools.lru_cache(maxsize=None)
def central_differences(case):
    nr, nf, d, eps, p, n = case
    Xr, Xf = sg.converged_data(nr, nf, d)
    Z = np.concatenate([Xr, Xf])
    N = len(Z)
    batch = np.repeat(Z[None], 2 * N * d + 1, axis=0)            # +h then -h on every coordinate, and Z itself
    for e in range(N * d):
        batch[2 * e, e // d, e % d] += H
        batch[2 * e + 1, e // d, e % d] -= H
    vals = sg.iterated_values(batch, nr, p, eps, n)
    assert abs(vals[-1] - sg.iterate(Xr, Xf, p, eps, n)[0]) <= 1e-13 * sn.cmax(Xr, Xf, p)     # the same function
    fd = ((vals[0:-1:2] - vals[1:-1:2]) / (2 * H)).reshape(N, d)
    fd.setflags(write=False)
    return fd


@pytest.mark.parametrize("case", sg.CONVERGED, ids=str)
def test_gradient_equals_central_differences_of_the_iterated_value(case):
    nr, nf, d, eps, p, n = case
    Xr, Xf = sg.converged_data(nr, nf, d)
    o = sg.value_drift_grad(Xr, Xf, p, eps, n)
    print("drift %.3g" % o["drift"])
    assert o["drift"] <= DRIFT
    fd = central_differences(case)
    err = float(np.abs(o["grad"] - fd).max())
    print("%s: gradient off central differences by at most %.3g; columns sum to %s" % (case, err, o["grad"].sum(axis=0)))
    assert err <= FD_TOL
    assert (np.abs(o["grad"].sum(axis=0)) <= FD_TOL).all()                  # translation invariance
    # the same function as the metric's restatement
    want = sn.full_sample(Xr, Xf, p, eps, n)
    assert abs(o["value"] - want["value"]) <= 1e-13 * sn.cmax(Xr, Xf, p) and o["drift"] == want["drift"]
    assert np.array_equal(o["fin"], want["potentials"])


@pytest.mark.parametrize("case", sg.CONVERGED, ids=str)
def test_differentiating_through_the_columns_too_doubles_the_gradient(case):
    nr, nf, d, eps, p, n = case
    Xr, Xf = sg.converged_data(nr, nf, d)
    fd = central_differences(case)
    twice = sg.value_drift_grad(Xr, Xf, p, eps, n, doubled=True)["grad"]
    err = float(np.abs(twice - 2.0 * fd).max())
    print("%s: doubled variant off 2 x central differences by at most %.3g, largest element %.3g" % (case, err, np.abs(fd).max()))
    assert err <= 2 * FD_TOL
    assert float(np.abs(twice - fd).max()) >= 0.5 * float(np.abs(fd).max())


def autograd_last_step(Xr, Xf, p, eps, old, block=128):
    """torch-CPU float64 autograd of S = sum_a w_a (fin[0][a] - fin[1][a]), every fin a softmin over the columns of the potentials
    `old` the last step read, with the columns' coordinates and `old` held fixed: the envelope-theorem gradient the kernel forms.
    A block of rows at a time, the blocks' backward passes accumulating -> (S, dS/dZ)"""
    Z = torch.from_numpy(np.concatenate([Xr, Xf])).clone().requires_grad_(True)
    cols, h = Z.detach(), torch.from_numpy(np.asarray(old))
    nr, N = len(Xr), Z.shape[0]
    first = torch.arange(N) < nr
    w = torch.from_numpy(np.where(np.arange(N) < nr, 1.0 / nr, 1.0 / (N - nr)))          # built in float64
    total = 0.0
    for a0 in range(0, N, block):
        diff = Z[a0:a0 + block, None, :] - cols[None, :, :]
        d2 = (diff * diff).sum(dim=2)
        pos = d2 > 0
        C = torch.where(pos, torch.where(pos, d2, torch.ones_like(d2)).sqrt(), torch.zeros_like(d2)) if p == 1 else d2
        same = first[a0:a0 + block, None] == first[None, :]
        minus_inf = torch.full_like(C, -float("inf"))
        part = 0.0
        for slot, mask, sign in ((0, ~same, 1.0), (1, same, -1.0)):
            z = torch.where(mask, (h[slot][None, :] - C) / eps + torch.log(w)[None, :], minus_inf)
            part = part + sign * (w[a0:a0 + block] * (-eps * torch.logsumexp(z, dim=1))).sum()
        part.backward()
        total += float(part.detach())
    return total, Z.grad.numpy()


@pytest.mark.parametrize("p", (1, 2))
@pytest.mark.parametrize("case", [(65, 63, 17, "plain"), (130, 70, 2, "copies")] + pg.CROSSED, ids=pg.case_id)
def test_restatement_equals_torch_autograd_of_the_last_step(case, p):
    Xr, Xf = pg.make(case)
    eps = float(0.1 * sn.median(Xr, Xf) ** p)
    cm = sn.cmax(Xr, Xf, p)
    o = sg.value_drift_grad(Xr, Xf, p, eps, 2)
    S, grad = autograd_last_step(Xr, Xf, p, eps, o["old"])
    err = np.abs(grad - o["grad"])
    print("%s p=%d: cmax / eps %.3g, value off by %.3g cmax, gradient by at most %.3g of M"
          % (pg.case_id(case), p, cm / eps, abs(S - o["value"]) / cm, float((err / np.where(o["M"] > 0, o["M"], 1.0)).max())))
    assert np.isfinite(grad).all() and abs(S - o["value"]) <= pg.TOL * cm
    assert (err <= pg.TOL * o["M"]).all()


def test_restatement_on_hand_made_data():
    # one real row at 0, one fake row at (3, 4), p = 1: every softmin has one column, f = g = 5 / 2, S = 5, P = 1 on every pair; the self
    # pairs are at d2 = 0 and add nothing
    o = sg.value_drift_grad(np.zeros((1, 2)), np.array([[3.0, 4.0]]), 1, 0.7, 3)
    assert abs(o["value"] - 5.0) <= 1e-14 and np.allclose(o["grad"], [[-0.6, -0.8], [0.6, 0.8]], rtol=1e-14, atol=0)
    # p = 2, no averaged step: f = g = 25, S = 50, P = 1, dS/dz_a = 2 (z_a - z_b)
    o = sg.value_drift_grad(np.zeros((1, 2)), np.array([[3.0, 4.0]]), 2, 0.7, 0)
    assert abs(o["value"] - 50.0) <= 1e-13 and np.allclose(o["grad"], [[-6.0, -8.0], [6.0, 8.0]], rtol=1e-14, atol=0)
    assert o["drift"] == 0.0 and not o["old"].any()
    # equal samples: S = 0 and the cross and self terms of every row cancel
    X = sg.converged_data(7, 7, 2)[0]
    o = sg.value_drift_grad(X, X, 2, 0.5, 5)
    assert abs(o["value"]) <= 1e-14 and (np.abs(o["grad"]) <= 1e-14 * o["M"]).all()


# ---- header, binding, statuses ------------------------------------------------------------------------------

def test_header_declarations_equal_the_binding():
    raw = open(os.path.join(CSRC, "pf_metrics.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = re.findall(r"\b(pfm_[a-z0-9_]+)\s*\(", text)
    assert sorted(declared) == sorted(_lib.EXPORTS) and set(NEW) <= set(_lib.EXPORTS)
    assert "#define PFM_VERSION %d " % _lib.ABI_VERSION in raw
    assert "pf_sinkgrad.o" in open(os.path.join(CSRC, "Makefile")).read()
    assert "atomic" not in re.sub(r"//.*", "", open(os.path.join(CSRC, "pf_sinkgrad.hip")).read())


def test_workspace_query_and_argument_statuses_without_a_device():
    native_libs.ensure_built(_lib)
    L = _lib.lib()
    assert L.pfm_version() == _lib.ABI_VERSION and all(hasattr(L, name) for name in NEW)
    q = _lib.sinkhorn_grad_workspace_bytes
    assert q(2, 1, 1) > 0 and q(20000, 16, 10000) > 0 and q(2200, 33, 1200) > 0
    for bad in ((1, 1, 1), (0, 1, 0), (10, 0, 5), (10, 2, 0), (10, 2, 10), (10, 2, -1), (2 ** 31, 2, 1), (2 ** 30, 2 ** 40, 1)):
        assert q(*bad) == 0, bad
    # three potential buffers [2, n] and the slices' partials [slices, n, d]: nothing of the size of the pair matrix
    assert q(20000, 16, 10000) <= 8 * 20000 * 16 * 8 + 3 * (16 * 20000 + 256)
    assert q(2200, 2, 1200) == q(2200, 2, 7)                      # a function of (n, d) only
    fake = ctypes.c_void_p(256)

    def call(Z=fake, n=10, d=2, nfirst=4, p=2, eps=0.5, steps=3, value=fake, drift=fake, grad=fake, pots=fake, ws=fake,
             nbytes=1 << 20):
        return L.pfm_sinkhorn_grad(None, Z, n, d, nfirst, p, eps, steps, value, drift, grad, pots, ws, nbytes)

    # refused before anything is read or launched (the device pointers are never dereferenced)
    assert call(Z=None) == _lib.PFM_EINVAL and call(value=None) == _lib.PFM_EINVAL and call(drift=None) == _lib.PFM_EINVAL
    assert call(n=1, nfirst=1) == _lib.PFM_EINVAL and call(d=0) == _lib.PFM_EINVAL
    assert call(nfirst=0) == _lib.PFM_EINVAL and call(nfirst=10) == _lib.PFM_EINVAL and call(n=2 ** 31) == _lib.PFM_EINVAL
    for eps in (0.0, -1.0, float("inf"), float("nan"), 1e-320):
        assert call(eps=eps) == _lib.PFM_EINVAL, eps
    assert call(steps=-1) == _lib.PFM_EINVAL and call(steps=1000001) == _lib.PFM_EINVAL
    assert call(p=0) == _lib.PFM_EUNSUPPORTED and call(p=3) == _lib.PFM_EUNSUPPORTED
    assert call(ws=None) == _lib.PFM_EWORKSPACE and call(nbytes=q(10, 2, 4) - 1) == _lib.PFM_EWORKSPACE
    assert call(grad=None, pots=None, nbytes=q(10, 2, 4) - 1) == _lib.PFM_EWORKSPACE


# ---- the public call's argument checks ----------------------------------------------------------------------

def test_sinkhorn_loss_is_importable_and_checks_its_arguments_without_a_device(monkeypatch):
    def launched(*a, **k):
        raise AssertionError("an argument error must be raised before anything is launched")
    monkeypatch.setattr(_lib, "sinkhorn_grad", launched)
    monkeypatch.setattr(_lib, "mmd", launched)
    X, Y = np.zeros((5, 3)), np.ones((4, 3))
    fn = losses.sinkhorn_loss
    with pytest.raises(ValueError, match="different numbers of features"):
        fn(X, np.ones((4, 2)), epsilon=1.0)
    with pytest.raises(ValueError, match="2-D"):
        fn(X[:, 0], Y)
    with pytest.raises(ValueError, match="2-D"):
        fn(torch.zeros(5, 3), torch.zeros(4))
    with pytest.raises(ValueError, match="real numeric"):
        fn(X.astype(complex), Y)
    for bad in (1, 0, None, "yes", np.array([True])):
        with pytest.raises(ValueError, match="standardize must be a bool"):
            fn(X, Y, standardize=bad)
        with pytest.raises(ValueError, match="return_drift must be a bool"):
            fn(X, Y, return_drift=bad)
    for bad in (0, 3, 1.0, True, "2", None):
        with pytest.raises(ValueError, match="p must be 1 or 2"):
            fn(X, Y, p=bad)
    for bad in (0, -1.0, float("inf"), float("nan"), True, "1", None, 1e-320, [0.1]):
        with pytest.raises(ValueError, match="reg must be a positive finite number with a finite reciprocal"):
            fn(X, Y, reg=bad)
    for bad in (0, -1.0, float("inf"), float("nan"), True, "1", 1e-320, torch.ones(1)):
        with pytest.raises(ValueError, match="epsilon must be None or a positive finite number with a finite reciprocal"):
            fn(X, Y, epsilon=bad)
    for bad in (-1, 1000001, 1.0, True, None, "3"):
        with pytest.raises(ValueError, match="n_sinkhorn must be an integer in 0 .. 1000000"):
            fn(X, Y, n_sinkhorn=bad)


def test_module_stays_out_of_the_export_list():
    import probaforms_amd.metrics as m
    assert m.__all__ == ["frechet_distance", "maximum_mean_discrepancy"] and not hasattr(m, "sinkhorn_loss")
