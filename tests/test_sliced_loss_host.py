"""probaforms_amd.metrics.losses.sliced_wasserstein_loss / wasserstein_1d_loss without a GPU: the float64 restatement
(tests/slicegrad_numpy.py) against scipy's 1-Wasserstein distance, central differences and a torch-CPU autograd version, the C
header against the binding, the workspace query and the argument statuses of pfm_slice_grad, and the public calls' argument
checks.

Central differences, step h = 1e-6: between two changes of the sort order the value is a polynomial of degree p <= 2 in every
coordinate, so central differences have no truncation error and carry the rounding error of the two values, about
1e-16 |L| / h = 1e-10 for |L| of order 1.  The bound is 1e-8.
"""
import ctypes
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import native_libs  # noqa: E402
import slicegrad_numpy as sl  # noqa: E402
from probaforms_amd.metrics import _lib, losses, wasserstein  # noqa: E402

CSRC = os.path.join(ROOT, "probaforms_amd", "metrics", "csrc")
NEW = ("pfm_slice_grad_workspace_bytes", "pfm_slice_grad")
SIZES = [(1, 1), (2, 3), (7, 7), (64, 65), (100, 37), (5, 1)]
H, FD_TOL = 1e-6, 1e-8


@pytest.mark.parametrize("size", SIZES, ids=str)
def test_restatement_equals_scipy_per_projection(size):
    stats = pytest.importorskip("scipy.stats")
    nr, nf = size
    Xr, Xf = sl.make(nr, nf, 3)
    theta = sl.unit_directions(4, 3)
    o = sl.value_grad(Xr, Xf, theta, 1)
    for k in range(4):
        want = stats.wasserstein_distance(o["cols"][k, :nr], o["cols"][k, nr:])
        assert abs(o["W"][k] - want) <= 1e-14 * max(1.0, want), (k, o["W"][k], want)
    assert abs(o["value"] - o["W"].mean()) <= 1e-15 * o["Lmag"]


@pytest.mark.parametrize("p", (1, 2))
@pytest.mark.parametrize("size", SIZES, ids=str)
def test_restatement_gradient_equals_central_differences(size, p):
    nr, nf = size
    Xr, Xf = sl.make(nr, nf, 2)
    theta = sl.unit_directions(3, 2)
    o = sl.value_grad(Xr, Xf, theta, p)
    Z = np.concatenate([Xr, Xf])
    fd = np.empty_like(Z)
    for a in range(len(Z)):
        for j in range(2):
            v = []
            for s in (H, -H):
                Zs = Z.copy()
                Zs[a, j] += s
                v.append(sl.value_grad(Zs[:nr], Zs[nr:], theta, p, vectorised=True)["value"])
            fd[a, j] = (v[0] - v[1]) / (2 * H)
    err = float(np.abs(o["grad"] - fd).max())
    print("%s p=%d: gradient off central differences by at most %.3g" % (size, p, err))
    assert err <= FD_TOL
    assert (np.abs(o["grad"].sum(axis=0)) <= 1e-12 * o["M"].sum(axis=0)).all()        # translation invariance


@pytest.mark.parametrize("p", (1, 2))
@pytest.mark.parametrize("size", [(2, 3), (7, 7), (64, 65), (100, 37), (1025, 1023)], ids=str)
def test_vectorised_coupling_equals_the_loops(size, p):
    nr, nf = size
    Xr, Xf = sl.make(nr, nf, 2)
    theta = sl.unit_directions(2, 2)
    a, b = sl.value_grad(Xr, Xf, theta, p), sl.value_grad(Xr, Xf, theta, p, vectorised=True)
    assert abs(a["value"] - b["value"]) <= 1e-14 * a["Lmag"] and abs(a["Lmag"] - b["Lmag"]) <= 1e-14 * a["Lmag"]
    assert (np.abs(a["grad"] - b["grad"]) <= 1e-14 * a["M"]).all() and (np.abs(a["M"] - b["M"]) <= 1e-14 * a["M"]).all()
    assert np.array_equal(a["perm"], b["perm"])
    i, j, ov = sl.segments(nr, nf)
    assert len(i) == nr + nf - math.gcd(nr, nf) and ov.min() > 0 and int(ov.sum()) == nr * nf


@pytest.mark.parametrize("p", (1, 2))
@pytest.mark.parametrize("n", (1, 7, 64, 100))
def test_restatement_equals_torch_autograd_for_equal_sizes(n, p):
    Xr, Xf = sl.make(n, n, 3)
    theta = sl.unit_directions(5, 3)
    o = sl.value_grad(Xr, Xf, theta, p)
    A, B = torch.from_numpy(Xr).requires_grad_(True), torch.from_numpy(Xf).requires_grad_(True)
    L = sl.torch_value(A, B, torch.from_numpy(theta), p)
    L.backward()
    grad = torch.cat([A.grad, B.grad]).numpy()
    assert abs(float(L.detach()) - o["value"]) <= 1e-12 * o["Lmag"]
    assert (np.abs(grad - o["grad"]) <= 1e-12 * o["M"]).all()


@pytest.mark.parametrize("p", (1, 2))
@pytest.mark.parametrize("case", [(100, 37, 3, 5), (5, 1, 2, 3)] + sl.CROSSED + [s + (None,) for s in sl.CROSSED_AXES], ids=str)
def test_restatement_equals_torch_autograd_at_the_crossed_shapes(case, p):
    nr, nf, d, P = case                                           # P None: the coordinate axes
    Xr, Xf = sl.make(nr, nf, d)
    theta = None if P is None else sl.unit_directions(P, d)
    o = sl.value_grad(Xr, Xf, theta, p)
    A, B = torch.from_numpy(Xr).requires_grad_(True), torch.from_numpy(Xf).requires_grad_(True)
    L = sl.torch_value(A, B, None if theta is None else torch.from_numpy(theta), p)
    L.backward()
    grad = torch.cat([A.grad, B.grad]).numpy()
    err = np.abs(grad - o["grad"])
    print("%s p=%d: value off by %.3g Lmag, gradient by at most %.3g M"
          % (case, p, abs(float(L.detach()) - o["value"]) / o["Lmag"], float((err / np.where(o["M"] > 0, o["M"], 1.0)).max())))
    assert abs(float(L.detach()) - o["value"]) <= 1e-12 * o["Lmag"]
    assert (err <= 1e-12 * o["M"]).all()


def test_restatement_on_hand_made_data():
    # one real row at 0, one fake row at (3, 4), theta = the axes: W = (3, 4) for p = 1, (9, 16) for p = 2
    o = sl.value_grad(np.zeros((1, 2)), np.array([[3.0, 4.0]]), None, 1)
    assert o["value"] == 3.5 and np.array_equal(o["grad"], [[-0.5, -0.5], [0.5, 0.5]])
    o = sl.value_grad(np.zeros((1, 2)), np.array([[3.0, 4.0]]), np.eye(2), 2)
    assert o["value"] == 12.5 and np.array_equal(o["grad"], [[-3.0, -4.0], [3.0, 4.0]])
    # ties: the (value, index) order; every row equal on a projection adds exactly nothing
    X = np.array([[1.0, 5.0], [0.0, 5.0], [1.0, 5.0]])
    o = sl.value_grad(X, X[::-1].copy(), np.eye(2), 1)
    assert np.array_equal(o["perm"], [[1, 0, 2, 4, 3, 5], [0, 1, 2, 3, 4, 5]]) and o["value"] == 0.0 and not o["grad"].any()


# ---- header, binding, statuses ------------------------------------------------------------------------------

def test_header_declarations_equal_the_binding():
    raw = open(os.path.join(CSRC, "pf_metrics.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = re.findall(r"\b(pfm_[a-z0-9_]+)\s*\(", text)
    assert sorted(declared) == sorted(_lib.EXPORTS) and set(NEW) <= set(_lib.EXPORTS)
    assert _lib.ABI_VERSION == 101 and "#define PFM_VERSION 101 " in raw
    assert "#define PFM_SLICE_LDS_ROWS %d " % _lib.SLICE_LDS_ROWS in raw and _lib.SLICE_LDS_ROWS >= 10000
    assert 12 * _lib.SLICE_LDS_ROWS <= 160 * 1024
    assert "pf_slicegrad.o" in open(os.path.join(CSRC, "Makefile")).read()
    assert "atomic" not in re.sub(r"//.*|std::atomic|<atomic>", "", open(os.path.join(CSRC, "pf_slicegrad.hip")).read()).lower()
    # the header's argument lists are the binding's: count the parameters
    for name in NEW:
        args = re.search(r"\b%s\s*\(([^)]*)\)" % name, text).group(1)
        assert len(args.split(",")) == len(_lib._SIGNATURES[name][1]), name
    assert losses._MAX_LDS_ROWS == _lib.SLICE_LDS_ROWS


def test_workspace_query_and_argument_statuses_without_a_device():
    native_libs.ensure_built(_lib)
    L = _lib.lib()
    assert L.pfm_version() == _lib.ABI_VERSION == 101 and all(hasattr(L, name) for name in NEW)
    q = _lib.slice_grad_workspace_bytes
    assert q(2, 1, 1, 1) > 0 and q(20000, 16, 10000, 64) > 0 and q(2 ** 31 - 1, 1, 5, 65535) > 0
    bad_sizes = ((1, 1, 1, 1), (0, 1, 0, 1), (10, 0, 5, 1), (10, 2, 0, 1), (10, 2, 10, 1), (10, 2, -1, 1), (2 ** 31, 2, 1, 1),
                 (10, 2, 5, 0), (10, 2, 5, 65536), (2 ** 30, 2 ** 40, 1, 1))
    for bad in bad_sizes:
        assert q(*bad) == 0, bad
    # 20 bytes per direction and pooled row and the value partials: O(P n), nothing of the size of a pair matrix
    assert q(20000, 16, 10000, 64) <= 20 * 64 * 20000 + 8 * 64 * 80 + 4 * 256
    assert q(2200, 2, 1200, 7) == q(2200, 33, 7, 7)                # a function of (n, n_proj) only
    fake = ctypes.c_void_p(256)

    def call(p=2, Z=fake, n=10, d=2, nfirst=4, theta=fake, nproj=3, perm_in=None, value=fake, rows=fake, cols=fake, perm=fake,
             ws=fake, nbytes=1 << 20):
        return L.pfm_slice_grad(None, p, Z, n, d, nfirst, theta, nproj, perm_in, value, rows, cols, perm, ws, nbytes)

    # refused before anything is read or launched (the device pointers are never dereferenced)
    assert call(Z=None) == _lib.PFM_EINVAL and call(value=None) == _lib.PFM_EINVAL
    for n, d, nfirst, nproj in bad_sizes:
        assert call(n=n, d=d, nfirst=nfirst, nproj=nproj) == _lib.PFM_EINVAL, (n, d, nfirst, nproj)
    assert call(theta=None, nproj=3) == _lib.PFM_EINVAL                         # the axes: n_proj must be d
    assert call(p=0) == _lib.PFM_EUNSUPPORTED and call(p=3) == _lib.PFM_EUNSUPPORTED
    big = 2 * _lib.SLICE_LDS_ROWS + 2
    assert call(n=big, nfirst=_lib.SLICE_LDS_ROWS + 1, nbytes=1 << 40) == _lib.PFM_EUNSUPPORTED     # no perm_in: the call sorts
    assert call(n=big, nfirst=1, nbytes=1 << 40) == _lib.PFM_EUNSUPPORTED
    assert call(ws=None) == _lib.PFM_EWORKSPACE and call(nbytes=q(10, 2, 4, 3) - 1) == _lib.PFM_EWORKSPACE
    assert call(rows=None, cols=None, perm=None, nbytes=q(10, 2, 4, 3) - 1) == _lib.PFM_EWORKSPACE
    assert call(n=big, nfirst=1, perm_in=fake, nbytes=q(big, 2, 1, 3) - 1) == _lib.PFM_EWORKSPACE    # perm_in: any size


# ---- the public calls' argument checks ----------------------------------------------------------------------

def test_argument_errors_are_raised_before_any_draw_or_launch(monkeypatch):
    def launched(*a, **k):
        raise AssertionError("an argument error must be raised before anything is launched")
    monkeypatch.setattr(_lib, "slice_grad", launched)
    monkeypatch.setattr(_lib, "project", launched)
    np.random.seed(11)
    state = np.random.get_state()
    X, Y = np.zeros((5, 3)), np.ones((4, 3))
    for fn in (losses.sliced_wasserstein_loss, losses.wasserstein_1d_loss, wasserstein.sliced_wasserstein_full_sample):
        with pytest.raises(ValueError, match="different numbers of features"):
            fn(X, np.ones((4, 2)))
        with pytest.raises(ValueError, match="2-D"):
            fn(X[:, 0], Y)
        with pytest.raises(ValueError, match="2-D"):
            fn(torch.zeros(5, 3), torch.zeros(4))
        with pytest.raises(ValueError, match="real numeric"):
            fn(X.astype(complex), Y)
        for bad in (0, 3, True, "2", None):
            with pytest.raises(ValueError, match="p must be 1 or 2"):
                fn(X, Y, p=bad)
    with pytest.raises(ValueError, match="p must be 1 or 2"):
        losses.sliced_wasserstein_loss(X, Y, p=1.0)
    for fn in (losses.sliced_wasserstein_loss, wasserstein.sliced_wasserstein_full_sample):
        for bad in (1, 0, None, "yes", np.array([True])):
            with pytest.raises(ValueError, match="standardize must be a bool"):
                fn(X, Y, standardize=bad)
        for bad in (0, -1, 65536, 1.0, True, None, "3"):
            with pytest.raises(ValueError, match="n_projections must be"):
                fn(X, Y, n_projections=bad)
    for bad in (np.zeros(3), np.zeros((2, 2)), np.zeros((0, 3)), np.zeros((2, 3, 1)), torch.zeros(2, 4), np.zeros((65536, 3))):
        with pytest.raises(ValueError, match="directions"):
            losses.sliced_wasserstein_loss(X, Y, directions=bad)
    with pytest.raises(ValueError, match="directions"):
        losses.sliced_wasserstein_loss(X, Y, directions=np.zeros((2, 3), dtype=complex))
    with pytest.raises(ValueError, match="NaN or infinite"):
        wasserstein.sliced_wasserstein_full_sample(X, np.full((4, 3), np.nan))
    with pytest.raises(ValueError, match="at most 65535 features"):
        losses.wasserstein_1d_loss(np.zeros((1, 65536)), np.zeros((1, 65536)))
    after = np.random.get_state()
    assert state[0] == after[0] and np.array_equal(state[1], after[1]) and state[2:] == after[2:]


def test_new_names_stay_out_of_the_export_list():
    import probaforms_amd.metrics as m
    assert m.__all__ == ["frechet_distance", "maximum_mean_discrepancy"]
    assert not hasattr(m, "sliced_wasserstein_loss") and not hasattr(m, "sliced_wasserstein_full_sample")
