"""probaforms_amd.metrics.losses.energy_score_loss / crps_loss without a GPU: the float64 restatement (tests/scoregrad_numpy.py)
against the energy score's existing restatement (tests/joint_scores_numpy.py), central differences and torch-CPU float64 autograd of
the same formula at the shapes where the GPU test crosses the kernel's axes, the C header against the binding, the workspace query,
pfm_score_plan and the argument statuses of pfm_score_grad, and the public calls' argument checks.

The autograd yardstick sums the same terms in another order: it is held within scoregrad_numpy.rtol_of(d) of the sum of the
magnitudes of an output's terms, the bound the GPU test holds the kernel to.

Central differences, step h = 1e-6, on rows whose points lie apart by 0.1 and more: the truncation error h^2 / 6 |f'''| is below
1e-10 there, and the rounding error of the two values is about 2^-52 |score| / h = 1e-9 for scores of order 1.  The bound is 1e-7.
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
import scoregrad_numpy as sg  # noqa: E402
from probaforms_amd.metrics import _lib, losses  # noqa: E402

CSRC = os.path.join(ROOT, "probaforms_amd", "metrics", "csrc")
NEW = ("pfm_score_grad_workspace_bytes", "pfm_score_plan", "pfm_score_grad")
H, FD_TOL = 1e-6, 1e-7
LDS_CU = 160 * 1024


@pytest.mark.parametrize("fair", (False, True))
@pytest.mark.parametrize("shape", [(2, 1), (3, 2), (33, 17), (257, 3)], ids=str)
def test_restatement_equals_the_joint_scores_restatement(shape, fair):
    K, d = shape
    X, Y = sg.finite_rows(K, d)
    o = sg.value_grad(X, Y, fair)
    ref = js.scores_of_stacked(X, Y, fair, None)
    tol = js.bound_pairs(ref.energy, ref, K, d) - js._ulp32(ref.energy)             # bound_pairs without its ulp32 term
    for name, got, want in (("energy", o["scores"], ref.energy), ("spread", o["spread"], ref.spread)):
        err = np.abs(got - want)
        print("K=%d d=%d fair=%s %s: off by at most %.3g of the bound" % (K, d, fair, name, float((err / tol).max())))
        assert (err <= tol).all(), (name, err, tol)
    generic = sg.rows(K, 4, d)
    X32, Y32 = generic[0].astype(np.float32), generic[1].astype(np.float32)
    o, ref = sg.value_grad(X32, Y32, fair), js.scores_of_stacked(X32, Y32, fair, None)
    tol = js.bound_pairs(ref.energy, ref, K, d) - js._ulp32(ref.energy)
    assert (np.abs(o["scores"] - ref.energy) <= tol).all() and (np.abs(o["spread"] - ref.spread) <= tol).all()


@pytest.mark.parametrize("fair", (False, True))
@pytest.mark.parametrize("shape", [(2, 3, 1), (3, 2, 2), (5, 2, 3)], ids=str)
def test_restatement_gradient_equals_central_differences(shape, fair):
    K, n, d = shape
    X, Y = sg.rows(K, n, d)
    o = sg.value_grad(X, Y, fair)
    worst = 0.0
    for name, A, G in (("x", X, o["grad_x"]), ("y", Y, o["grad_y"])):
        for idx in np.ndindex(A.shape):
            v = []
            for step in (H, -H):
                B = A.copy()
                B[idx] += step
                v.append(sg.score_of(B, Y, fair) if name == "x" else sg.score_of(X, B, fair))
            fd = (v[0] - v[1]) / (2 * H) * n                         # the mean over n rows; G is the row's own derivative
            worst = max(worst, abs(fd - G[idx]))
    print("%s fair=%s: gradient off central differences by at most %.3g" % (shape, fair, worst))
    assert worst <= FD_TOL
    # translation invariance: a row's derivatives by its points sum to 0
    total = o["grad_x"].sum(axis=0) + o["grad_y"]
    assert (np.abs(total) <= 1e-13 * (o["mx"].sum(axis=0) + o["my"])).all()


def autograd_value_grad(X, Y, fair, budget=1 << 22):
    """torch-CPU float64 autograd of the rows' scores (a row's outputs depend on that row alone, so the gradient of the sum of the
    scores is every row's own); the distance is where(d2 > 0, sqrt(.), 0) with the root taken of 1 where d2 = 0, so that a
    coincident pair adds the subgradient 0; the pairs a block of draws at a time, the blocks' backward passes accumulating
    -> (scores, spread, grad_x, grad_y)"""
    A, B = torch.from_numpy(np.array(X, np.float64)).requires_grad_(True), torch.from_numpy(np.array(Y, np.float64)).requires_grad_(True)
    K, n, d = A.shape
    D = K - 1 if fair else K

    def dist(diff):
        d2 = (diff * diff).sum(dim=-1)
        pos = d2 > 0
        return torch.where(pos, torch.where(pos, d2, torch.ones_like(d2)).sqrt(), torch.zeros_like(d2))

    t1 = dist(A - B[None]).sum(dim=0) / K
    t1.sum().backward()
    spread = torch.zeros(n, dtype=torch.float64)
    step = max(1, budget // (K * n * d))
    for k0 in range(0, K, step):
        part = dist(A[k0:k0 + step, None] - A[None]).sum(dim=(0, 1)) / (2.0 * K * D)
        (-part.sum()).backward()
        spread = spread + part.detach()
    return (t1.detach() - spread).numpy(), spread.numpy(), A.grad.numpy(), B.grad.numpy()


AUTOGRAD_CASES = [(1, 3, 2), (2, 3, 1), (33, 7, 17), (257, 3, 2)] + sg.CROSSED + sg.CROSSED_NAN + sg.CROSSED_LAYOUT


@pytest.mark.parametrize("fair", (False, True))
@pytest.mark.parametrize("case", AUTOGRAD_CASES, ids=str)
def test_restatement_equals_torch_autograd(case, fair):
    K, n, d = case
    if K == 1 and fair:
        return
    X, Y = sg.rows(K, n, d)
    o = sg.value_grad(X, Y, fair)
    scores, spread, gx, gy = autograd_value_grad(X, Y, fair)
    rtol = sg.rtol_of(d)
    for name, got, mag in (("scores", scores, "smag"), ("spread", spread, "spread"), ("grad_x", gx, "mx"), ("grad_y", gy, "my")):
        err, m = np.abs(got - o[name]), np.abs(o[mag])
        print("%s fair=%s: %s off by at most %.3g of its terms' magnitudes (bound %.3g)"
              % (case, fair, name, float((err / np.where(m > 0, m, 1.0)).max()), rtol))
        assert np.isfinite(got).all() and (err <= rtol * m).all(), name


def test_restatement_on_hand_made_data():
    # one row, d = 2: draws (0, 0) and (6, 8), target (3, 4): T1 = 5, pair distance 10
    X, Y = np.array([[[0.0, 0.0]], [[6.0, 8.0]]]), np.array([[3.0, 4.0]])
    o = sg.value_grad(X, Y, True)
    assert o["scores"][0] == 0.0 and o["spread"][0] == 5.0
    o = sg.value_grad(X, Y, False)
    assert o["scores"][0] == 2.5 and o["spread"][0] == 2.5 and not o["grad_y"].any()
    assert np.allclose(o["grad_x"][0, 0], [-0.3 + 0.15, -0.4 + 0.2], rtol=0, atol=1e-15)
    # K = 1, fair=False: the Euclidean error; a draw on its target adds the subgradient 0
    o = sg.value_grad(np.array([[[3.0, 4.0], [1.0, 1.0]]]), np.array([[0.0, 0.0], [1.0, 1.0]]), False)
    assert np.array_equal(o["scores"], [5.0, 0.0]) and not o["spread"].any()
    assert np.allclose(o["grad_x"][0], [[0.6, 0.8], [0.0, 0.0]], rtol=0, atol=1e-15) and not o["grad_x"][0, 1].any()
    # a NaN stays in its row
    X, Y = sg.rows(3, 4, 2)
    X, Y = X.copy(), Y.copy()
    X[1, 0, 1], Y[2, 0] = np.nan, np.nan
    o = sg.value_grad(X, Y, True)
    assert np.isnan(o["scores"]).tolist() == [True, False, True, False]
    assert np.isnan(o["spread"]).tolist() == [True, False, False, False]            # the spread does not meet y
    gx, gy = np.isnan(o["grad_x"]), np.isnan(o["grad_y"])
    assert gx[:, [0, 2]].all() and not gx[:, [1, 3]].any() and gy[[0, 2]].all() and not gy[[1, 3]].any()


# ---- header, binding, statuses ------------------------------------------------------------------------------

def test_header_declarations_equal_the_binding():
    raw = open(os.path.join(CSRC, "pf_metrics.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = re.findall(r"\b(pfm_[a-z0-9_]+)\s*\(", text)
    assert sorted(declared) == sorted(_lib.EXPORTS) and set(NEW) <= set(_lib.EXPORTS)
    assert _lib.ABI_VERSION == 101 and "#define PFM_VERSION 101 " in raw
    assert "#define PFM_SCORE_MAX_K %d " % _lib.SCORE_MAX_K in raw and _lib.SCORE_MAX_K >= 1024
    assert "#define PFM_SCORE_MAX_KD %d " % _lib.SCORE_MAX_KD in raw and _lib.SCORE_MAX_KD >= 16384
    assert "pf_scoregrad.o" in open(os.path.join(CSRC, "Makefile")).read()
    assert "atomic" not in re.sub(r"//.*", "", open(os.path.join(CSRC, "pf_scoregrad.hip")).read()).lower()
    for name in NEW:
        args = re.search(r"\b%s\s*\(([^)]*)\)" % name, text).group(1)
        assert len(args.split(",")) == len(_lib._SIGNATURES[name][1]), name


BAD_SIZES = ((0, 2, 2), (-1, 2, 2), (5, 0, 2), (5, -3, 2), (5, 2, 0), (5, 2, -1), (2 ** 31, 2, 2))
ABOVE = ((5, _lib.SCORE_MAX_K + 1, 1), (5, 2, _lib.SCORE_MAX_KD // 2 + 1), (5, 1, _lib.SCORE_MAX_KD + 1),
         (5, _lib.SCORE_MAX_K, _lib.SCORE_MAX_KD // _lib.SCORE_MAX_K + 1), (5, 2 ** 40, 2 ** 40))
PLAN_SHAPES = [(n, K, d) for n in (1, 1000, 65536) for K in (1, 2, 3, 8, 32, 33, 64, 255, 256, 257, 512, 1024) for d in (1, 2, 16)]
PLAN_SHAPES += [(4096, 256, 64), (7, 1, 16384), (7, 2, 8192), (100000, 963, 17), (2 ** 31 - 1, 4, 16)]


def test_workspace_query_and_argument_statuses_without_a_device():
    native_libs.ensure_built(_lib)
    L = _lib.lib()
    assert L.pfm_version() == _lib.ABI_VERSION == 101 and all(hasattr(L, name) for name in NEW)
    q = _lib.score_grad_workspace_bytes
    assert 0 < q(1, 1, 1) and 0 < q(65536, 32, 16) and 0 < q(2 ** 31 - 1, 1024, 16) and 0 < q(3, 256, 64)
    # O(n d) at the most: here a constant, and nothing of size K^2
    assert q(1, 1, 1) == q(65536, 32, 16) == q(4096, 1024, 16) <= 4096
    for bad in BAD_SIZES + ABOVE:
        assert q(*bad) == 0, bad
    fake = ctypes.c_void_p(256)

    def call(X=fake, Y=fake, n=10, K=4, d=2, fair=1, scores=fake, spread=fake, gx=fake, gy=fake, ws=fake, nbytes=1 << 20):
        return L.pfm_score_grad(None, X, Y, n, K, d, fair, scores, spread, gx, gy, ws, nbytes)

    # refused before anything is read or launched (the device pointers are never dereferenced)
    assert call(X=None) == call(Y=None) == call(scores=None) == _lib.PFM_EINVAL
    for n, K, d in BAD_SIZES:
        assert call(n=n, K=K, d=d) == _lib.PFM_EINVAL and call(n=n, K=K, d=d, fair=0) == _lib.PFM_EINVAL, (n, K, d)
    assert call(K=1, fair=1) == _lib.PFM_EINVAL and call(K=1, fair=7) == _lib.PFM_EINVAL
    for n, K, d in ABOVE:
        assert call(n=n, K=K, d=d, fair=int(K > 1)) == _lib.PFM_EUNSUPPORTED, (n, K, d)
    assert call(ws=None) == _lib.PFM_EWORKSPACE and call(nbytes=q(10, 4, 2) - 1) == _lib.PFM_EWORKSPACE
    assert call(K=1, fair=0, nbytes=0) == _lib.PFM_EWORKSPACE
    assert call(spread=None, gx=None, gy=None, nbytes=q(10, 4, 2) - 1) == _lib.PFM_EWORKSPACE


def test_plan_needs_no_device_and_is_consistent():
    native_libs.ensure_built(_lib)
    assert _lib.lib().pfm_score_plan(10, 4, 2, None) == _lib.PFM_EINVAL
    for bad in BAD_SIZES:
        assert _lib.score_plan_status(*bad)[0] == _lib.PFM_EINVAL, bad
    for bad in ABOVE:
        assert _lib.score_plan_status(*bad)[0] == _lib.PFM_EUNSUPPORTED, bad
    for n, K, d in PLAN_SHAPES:
        st, (R, S, lds, wgs) = _lib.score_plan_status(n, K, d)
        assert st == 0 and _lib.score_grad_workspace_bytes(n, K, d) > 0, (n, K, d)     # a plan exactly where the query has a size
        assert R >= 1 and wgs == -(-n // R), (n, K, d, R, wgs)
        assert S in (1, 2, 4, 8, 16, 32, 64, 128, 256) and S == min(256, 1 << (K - 1).bit_length()), (K, S)
        assert 8 * K * d <= lds <= LDS_CU, (n, K, d, lds)
        assert lds >= 8 * R * (K * d), (n, K, d, R, lds)                                # the rows' draws are staged whole
    # the two regimes: a few draws pack rows into a workgroup, many draws take it alone
    assert _lib.score_plan(65536, 4, 16)[1] == 4 and _lib.score_plan(65536, 4, 16)[0] >= 64
    assert _lib.score_plan(4096, 256, 16)[1] == 256
    # rows per workgroup fall while the workgroups are few, down to one group of rows in flight
    assert _lib.score_plan(1, 4, 16)[0] == 64 and _lib.score_plan(1, 1000, 1)[0] == 1


# ---- the public calls' argument checks ----------------------------------------------------------------------

def test_argument_errors_are_raised_before_any_device_is_touched(monkeypatch):
    def touched(*a, **k):
        raise AssertionError("an argument error must be raised before anything touches a device")
    monkeypatch.setattr(_lib, "score_grad", touched)
    monkeypatch.setattr(_lib, "score_grad_workspace_bytes", touched)
    monkeypatch.setattr(torch.cuda, "is_available", touched)
    X, Y = np.zeros((4, 5, 3)), np.ones((5, 3))
    for fn in (losses.energy_score_loss, losses.crps_loss):
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
        for bad in (1, 0, None, "yes", np.array([True])):
            with pytest.raises(ValueError, match="fair must be a bool"):
                fn(X, Y, fair=bad)
        for bad in ("sum", None, 1, "Mean"):
            with pytest.raises(ValueError, match="reduction must be"):
                fn(X, Y, reduction=bad)
        with pytest.raises(ValueError, match="at least 2 draws"):
            fn(X[:1], Y)
        with pytest.raises(ValueError, match="at least 2 draws"):
            fn(torch.zeros(1, 5, 3), torch.zeros(5, 3), fair=True)
        with pytest.raises(ValueError, match="at most 1024 draws"):
            fn(np.zeros((_lib.SCORE_MAX_K + 1, 2, 1)), np.zeros((2, 1)))
    with pytest.raises(ValueError, match="16384 draws times features"):
        losses.energy_score_loss(np.zeros((2, 1, _lib.SCORE_MAX_KD // 2 + 1)), np.zeros((1, _lib.SCORE_MAX_KD // 2 + 1)))


def test_new_names_stay_out_of_the_export_list():
    import probaforms_amd.metrics as m
    assert m.__all__ == ["frechet_distance", "maximum_mean_discrepancy"]
    assert not hasattr(m, "energy_score_loss") and not hasattr(m, "crps_loss")
    assert callable(losses.energy_score_loss) and callable(losses.crps_loss)
