"""probaforms_amd.metrics.losses.variogram_score_loss without a GPU: the float64 restatement (tests/variogram_grad_numpy.py) against
the variogram of the existing restatement (tests/joint_scores_numpy.py) and central differences, the C header against the binding,
the workspace query, pfm_variogram_plan and the argument statuses of pfm_variogram_grad, and the public call's argument checks.

Central differences, step h = 1e-6, by the coordinates that lie apart from the point's other coordinates by 0.05 and more: the
truncation error h^2 / 6 |f'''| of sqrt|t| is h^2 / 16 |t|^-2.5 < 1.2e-10 there (the other orders have none), and the rounding
error of the two values is about 2^-52 |score| / h = 2e-8 for scores of order 100.  The bound is 1e-6 of 1 + |gradient|.
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

import joint_scores_numpy as js  # noqa: E402
import native_libs  # noqa: E402
import variogram_grad_numpy as vg  # noqa: E402
from probaforms_amd.metrics import _lib, losses  # noqa: E402

CSRC = os.path.join(ROOT, "probaforms_amd", "metrics", "csrc")
NEW = ("pfm_variogram_grad_workspace_bytes", "pfm_variogram_plan", "pfm_variogram_grad")
ORDERS = (0.5, 1, 2)
H, FD_TOL = 1e-6, 1e-6
LDS_CU = 160 * 1024


# ---- the restatement ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("shape", [(1, 2), (2, 1), (3, 2), (33, 17), (257, 3)], ids=str)
def test_restatement_equals_the_joint_scores_restatement(shape, order):
    K, d = shape
    for X, Y in (vg.finite_rows(K, d), tuple(a.astype(np.float32) for a in vg.rows(K, 4, d))):
        o = vg.value_grad(X, Y, order)
        ref = js.scores_of_stacked(X, Y, False, float(order))
        tol = js.bound_variogram(ref.variogram, ref, K, d) - js._ulp32(ref.variogram)        # bound_variogram without its ulp32 term
        err = np.abs(o["scores"] - ref.variogram)
        assert (err <= tol).all(), (err, tol)
        assert (np.abs(o["smag"] - ref.v) <= 1e-12 * ref.v).all()                            # smag with unit weights is the metric's V
        assert all(np.isfinite(v).all() for v in o.values())


@pytest.mark.parametrize("weighted", (False, True))
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("shape", [(1, 2, 2), (2, 3, 3), (5, 2, 4)], ids=str)
def test_restatement_gradient_equals_central_differences(shape, order, weighted):
    K, n, d = shape
    X, Y = vg.rows(K, n, d)
    W = vg.weights(d) if weighted else None
    o = vg.value_grad(X, Y, order, W)
    worst = 0.0
    for name, A, G in (("x", X, o["grad_x"]), ("y", Y, o["grad_y"])):
        apart = np.abs(A[..., :, None] - A[..., None, :]) + np.eye(d)
        for idx in np.ndindex(A.shape):
            if apart[idx].min() < 0.05:                              # (see the module's docstring)
                continue
            v = []
            for step in (H, -H):
                B = A.copy()
                B[idx] += step
                v.append(vg.score_of(B, Y, order, W) if name == "x" else vg.score_of(X, B, order, W))
            fd = (v[0] - v[1]) / (2 * H)
            worst = max(worst, abs(fd - G[idx]) / (1.0 + abs(G[idx])))
    print("%s order=%s weighted=%s: gradient off central differences by at most %.3g" % (shape, order, weighted, worst))
    assert 0.0 < worst <= FD_TOL
    # a shift of all coordinates of a draw, or of the target, changes nothing: every point's derivatives sum to 0 over the features
    assert (np.abs(o["grad_x"].sum(axis=2)) <= 1e-13 * o["mx"].sum(axis=2)).all()
    assert (np.abs(o["grad_y"].sum(axis=1)) <= 1e-13 * o["my"].sum(axis=1)).all()


def test_restatement_on_hand_made_data():
    # one row, d = 2, K = 2: draws (0, 1) and (0, 3), target (0, 4).  p = 1: m = 2, v = 4, r = 2, VS = 2 r^2 = 8
    X, Y = np.array([[[0.0, 1.0]], [[0.0, 3.0]]]), np.array([[0.0, 4.0]])
    o = vg.value_grad(X, Y, 1)
    assert o["scores"][0] == 8.0 and o["smag"][0] == 72.0
    assert np.array_equal(o["grad_x"][:, 0], [[4.0, -4.0], [4.0, -4.0]])     # -(2/2) 2 r sgn(x_i - x_j)
    assert np.array_equal(o["grad_y"][0], [-8.0, 8.0])                       # 2 2 r sgn(y_i - y_j)
    # p = 2: m = (1 + 9) / 2 = 5, v = 16, r = 11, VS = 242;  p = 0.5: m = (1 + sqrt 3) / 2, v = 2
    assert vg.value_grad(X, Y, 2)["scores"][0] == 242.0
    assert abs(vg.value_grad(X, Y, 0.5)["scores"][0] - 2 * (2 - (1 + np.sqrt(3.0)) / 2) ** 2) < 1e-15
    # weights: only w_01 and w_10 meet a non-zero r
    assert vg.value_grad(X, Y, 1, np.array([[5.0, 0.25], [-1.0, 7.0]]))["scores"][0] == (0.25 - 1.0) * 4.0
    # d = 1, and all coordinates equal: everything is exactly 0, for every order
    for order in ORDERS:
        o = vg.value_grad(np.full((3, 2, 1), 1.5), np.full((2, 1), -2.0), order)
        assert not any(v.any() for v in o.values())
        o = vg.value_grad(np.full((3, 2, 4), 1.5), np.full((2, 4), -2.0), order)
        assert not any(v.any() for v in o.values()) and all(np.isfinite(v).all() for v in o.values())
    # a NaN stays in its row and fills it
    X, Y = vg.rows(3, 4, 3)
    X, Y = X.copy(), Y.copy()
    X[1, 0, 1], Y[2, 0] = np.nan, np.nan
    for order in ORDERS:
        o = vg.value_grad(X, Y, order)
        assert np.isnan(o["scores"]).tolist() == [True, False, True, False]
        gx, gy = np.isnan(o["grad_x"]), np.isnan(o["grad_y"])
        assert gx[:, [0, 2]].all() and not gx[:, [1, 3]].any() and gy[[0, 2]].all() and not gy[[1, 3]].any()


# ---- header, binding, statuses ------------------------------------------------------------------------------

def test_header_declarations_equal_the_binding():
    raw = open(os.path.join(CSRC, "pf_metrics.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = re.findall(r"\b(pfm_[a-z0-9_]+)\s*\(", text)
    assert sorted(declared) == sorted(_lib.EXPORTS) and set(NEW) <= set(_lib.EXPORTS)
    assert _lib.ABI_VERSION == 101 and "#define PFM_VERSION 101 " in raw
    assert "#define PFM_VARIO_MAX_D %d " % _lib.VARIO_MAX_D in raw and _lib.VARIO_MAX_D == 64
    assert "pf_variogram.o" in open(os.path.join(CSRC, "Makefile")).read()
    source = re.sub(r"//.*", "", open(os.path.join(CSRC, "pf_variogram.hip")).read())
    assert "atomic" not in source.lower() and not re.search(r"\bpow[fl]?\s*\(", source)
    for name in NEW:
        args = re.search(r"\b%s\s*\(([^)]*)\)" % name, text).group(1)
        assert len(args.split(",")) == len(_lib._SIGNATURES[name][1]), name
    assert _lib._SIGNATURES["pfm_variogram_grad"][1][7] is ctypes.c_double           # the order travels as a double


BAD_SIZES = ((0, 2, 2), (-1, 2, 2), (5, 0, 2), (5, -3, 2), (5, 2, 0), (5, 2, -1), (2 ** 31, 2, 2))
ABOVE = ((5, 2, _lib.VARIO_MAX_D + 1), (5, 1, _lib.VARIO_MAX_D + 1), (5, _lib.SCORE_MAX_K + 1, 1), (5, _lib.SCORE_MAX_K + 1, 2),
         (5, 257, 64), (5, _lib.SCORE_MAX_K, 17), (5, 16385, 1), (5, 2 ** 40, 2 ** 40), (5, 1, 2 ** 40))
AT = ((5, 1, 64), (5, 256, 64), (5, 1024, 16), (5, 1024, 1), (2 ** 31 - 1, 4, 16), (1, 1, 1), (65536, 32, 16), (5, 963, 17))


def test_workspace_query_and_argument_statuses_without_a_device():
    native_libs.ensure_built(_lib)
    L = _lib.lib()
    assert L.pfm_version() == _lib.ABI_VERSION == 101 and all(hasattr(L, name) for name in NEW)
    q = _lib.variogram_grad_workspace_bytes
    for ok in AT:
        assert 0 < q(*ok) <= 4096, ok                                # a constant: nothing of size n, K d^2 or n d^2
    assert len({q(*ok) for ok in AT}) == 1
    for bad in BAD_SIZES + ABOVE:
        assert q(*bad) == 0, bad
    fake = ctypes.c_void_p(256)

    def call(X=fake, Y=fake, W=fake, n=10, K=4, d=3, order=0.5, scores=fake, gx=fake, gy=fake, ws=fake, nbytes=1 << 20):
        return L.pfm_variogram_grad(None, X, Y, W, n, K, d, order, scores, gx, gy, ws, nbytes)

    # refused before anything is read or launched (the device pointers are never dereferenced)
    assert call(X=None) == call(Y=None) == call(scores=None) == _lib.PFM_EINVAL
    for n, K, d in BAD_SIZES:
        assert call(n=n, K=K, d=d) == _lib.PFM_EINVAL, (n, K, d)
    for order in (0.0, 0.25, 1.5, 3.0, -1.0, -0.5, float("nan"), float("inf"), 0.5 + 2.0 ** -53, 1e-300):
        assert call(order=order) == _lib.PFM_EINVAL, order
        assert call(order=order, d=_lib.VARIO_MAX_D + 1) == _lib.PFM_EINVAL, order
    for n, K, d in ABOVE:
        for order in ORDERS:
            assert call(n=n, K=K, d=d, order=order) == _lib.PFM_EUNSUPPORTED, (n, K, d)
    assert call(ws=None) == _lib.PFM_EWORKSPACE and call(nbytes=q(10, 4, 3) - 1) == _lib.PFM_EWORKSPACE
    assert call(W=None, gx=None, gy=None, nbytes=0) == _lib.PFM_EWORKSPACE and call(d=1, K=1, ws=None) == _lib.PFM_EWORKSPACE


def test_plan_needs_no_device_and_is_consistent():
    native_libs.ensure_built(_lib)
    assert _lib.lib().pfm_variogram_plan(10, 4, 2, None) == _lib.PFM_EINVAL
    for bad in BAD_SIZES:
        assert _lib.variogram_plan_status(*bad)[0] == _lib.PFM_EINVAL, bad
    for bad in ABOVE:
        assert _lib.variogram_plan_status(*bad)[0] == _lib.PFM_EUNSUPPORTED, bad
    for n, K, d in AT + ((1000, 33, 5), (4096, 256, 16), (7, 3, 64)):
        st, (R, S, lds, wgs, G, T) = _lib.variogram_plan_status(n, K, d)
        assert st == 0 and _lib.variogram_grad_workspace_bytes(n, K, d) > 0, (n, K, d)   # a plan exactly where the query has a size
        assert R >= 1 and R % G == 0 and wgs == -(-n // R) and 1 <= T <= K, (n, K, d, R, G, T, wgs)
        if d > 1:
            assert S == min(256, 1 << (K - 1).bit_length()) and S * G <= 256, (K, S, G)
            pairs = d * (d - 1) // 2
            assert 8 * (R * K * d + R * d + G * pairs) <= lds <= LDS_CU, (n, K, d, lds)   # the rows' draws whole, a table per row in flight
        else:
            assert (R, S, lds, G, T) == (256, 1, 0, 256, 1)
    # the two regimes: a few draws pack rows into a workgroup, many draws take it alone
    assert _lib.variogram_plan(65536, 4, 16)[1] == 4 and _lib.variogram_plan(65536, 4, 16)[0] >= 64
    assert _lib.variogram_plan(4096, 256, 16)[1] == 256 and _lib.variogram_plan(4096, 256, 16)[4] == 1
    # many draws of few features: the draws are cut into slices so that all lanes of the row sum pairs
    assert _lib.variogram_plan(1000, 1000, 5)[5] == 25


# ---- the public call's argument checks ----------------------------------------------------------------------

def test_argument_errors_are_raised_before_any_device_is_touched(monkeypatch):
    def touched(*a, **k):
        raise AssertionError("an argument error must be raised before anything touches a device")
    monkeypatch.setattr(_lib, "variogram_grad", touched)
    monkeypatch.setattr(_lib, "variogram_grad_workspace_bytes", touched)
    monkeypatch.setattr(torch.cuda, "is_available", touched)
    fn = losses.variogram_score_loss
    X, Y = np.zeros((4, 5, 3)), np.ones((5, 3))
    for bad in (0, 3, 0.25, 1.5, -1, "1", None, True, np.float64("nan"), [0.5], np.array([1.0])):
        with pytest.raises(ValueError, match="order must be 0.5, 1 or 2"):
            fn(X, Y, order=bad)
    for bad in (np.ones((3, 2)), np.ones((2, 3)), np.ones(3), np.ones((3, 3, 1)), torch.ones(4, 4), np.ones((0, 0)), 1.0):
        with pytest.raises(ValueError, match="weights"):
            fn(X, Y, weights=bad)
    for bad in (np.ones((3, 3), complex), torch.ones(3, 3, dtype=torch.bool), np.array([["a"] * 3] * 3), [[1, 2, 3], [1, 2], [1]]):
        with pytest.raises(ValueError, match="weights"):
            fn(X, Y, weights=bad)
    for bad in (X[0], X[None], np.zeros(5)):
        with pytest.raises(ValueError, match="3-D"):
            fn(bad, Y)
    for bad in (Y[0], Y[None], torch.zeros(5, 3, 1)):
        with pytest.raises(ValueError, match="2-D"):
            fn(X, bad)
    for bad in (np.ones((6, 3)), np.ones((5, 2)), torch.ones(3, 5)):
        with pytest.raises(ValueError, match="different numbers"):
            fn(X, bad)
    for a, b in ((np.zeros((0, 5, 3)), Y), (np.zeros((4, 0, 3)), np.zeros((0, 3))), (np.zeros((4, 5, 0)), np.zeros((5, 0)))):
        with pytest.raises(ValueError, match="at least one"):
            fn(a, b)
    with pytest.raises(ValueError, match="real numeric"):
        fn(X.astype(complex), Y)
    with pytest.raises(ValueError, match="real numeric"):
        fn(X, torch.zeros(5, 3, dtype=torch.bool))
    for bad in ("sum", None, 1, "Mean"):
        with pytest.raises(ValueError, match="reduction must be"):
            fn(X, Y, reduction=bad)
    with pytest.raises(ValueError, match="at most 64 features, got 65"):
        fn(np.zeros((2, 1, 65)), np.zeros((1, 65)))
    with pytest.raises(ValueError, match="at most 1024 draws"):
        fn(np.zeros((1025, 2, 1)), np.zeros((2, 1)))
    with pytest.raises(ValueError, match="16384 draws times features"):
        fn(np.zeros((16385 // 5 + 1, 1, 5)), np.zeros((1, 5)))


def test_valid_arguments_reach_the_device_check(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    X, Y = np.zeros((4, 5, 3)), np.ones((5, 3))
    calls = [dict(), dict(order=1), dict(order=2.0), dict(order=np.float32(0.5)), dict(order=np.int64(2)), dict(reduction="none"),
             dict(weights=np.ones((3, 3))), dict(weights=torch.ones(3, 3, dtype=torch.float32)), dict(weights=[[1, 2, 3]] * 3),
             dict(weights=-np.ones((3, 3), np.int32))]
    for kw in calls:
        with pytest.raises(RuntimeError, match="HIP device"):
            losses.variogram_score_loss(X, Y, **kw)
    for K, d in ((1, 64), (256, 64), (1024, 16), (1, 1)):                        # the limits themselves are taken
        with pytest.raises(RuntimeError, match="HIP device"):
            losses.variogram_score_loss(torch.zeros(K, 2, d), torch.zeros(2, d))


def test_new_name_stays_out_of_the_export_list():
    import probaforms_amd.metrics as m
    assert m.__all__ == ["frechet_distance", "maximum_mean_discrepancy"]
    assert not hasattr(m, "variogram_score_loss") and callable(losses.variogram_score_loss)
    assert issubclass(losses.VariogramFunction, torch.autograd.Function)
    assert "variogram_score_loss" in losses.__doc__ and "pfm_variogram_grad" in losses.__doc__
