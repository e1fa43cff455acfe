"""probaforms_amd.metrics.losses.crps_loss(method="sorted") / pinball_loss without a GPU: the float64 restatement
(tests/sortscore_numpy.py) against the pair route's restatement at d = 1 (tests/scoregrad_numpy.py) and against the restatement of
sample_scores (tests/scores_numpy.py), central differences, the C header against the binding, pfm_sort_score_plan against its
restatement here, the argument statuses of pfm_sort_score and pfm_pinball_grad, and the public calls' argument checks.

Values: the two restatements sum the same terms in another order; they are held within scoregrad_numpy.RTOL = 1e-12 of the sum of the
magnitudes of the terms, the project's bound.  Gradients: on small integers every c (x_k - x_l) of the pair route is exactly +-1 or 0
and its sums are exact integers, so what is compared with == is what both routes claim to be exact: the integer numerator
sgn(t_k) D - c_k, read back from the pair route's gradient as rint(K D grad), and the quotient itself wherever the pair route's own
expression sgn / K - c / (K D) rounds once (K and K D powers of two); elsewhere that expression rounds three times and is held to
4 2^-53 of its terms' magnitudes.

Central differences, step h = 1e-6, on series whose points lie apart by 0.1 and more (for the pinball score, y at least 0.3 from every
quantile): both scores are piecewise linear there, so the truncation error is 0 and the rounding error of the two values is about
2^-52 |score| / h = 1e-9 for scores of order 1 to 10, as in tests/test_score_loss_host.py.  The bound is 1e-7.
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

import native_libs  # noqa: E402
import scoregrad_numpy as sg  # noqa: E402
import scores_numpy as sn  # noqa: E402
import sortscore_numpy as ss  # noqa: E402
from probaforms_amd.metrics import _lib, losses  # noqa: E402

CSRC = os.path.join(ROOT, "probaforms_amd", "metrics", "csrc")
NEW = ("pfm_sort_score_workspace_bytes", "pfm_sort_score_plan", "pfm_sort_score", "pfm_pinball_grad")
H, FD_TOL = 1e-6, 1e-7
LDS_CU = 160 * 1024
U53 = 2.0 ** -53
KS = (1, 2, 3, 33, 257)


def fairs(K):
    return (False,) if K == 1 else (False, True)


# ---- the restatement against the pair route's and against sample_scores' --------------------------------------------------

@pytest.mark.parametrize("K", KS)
def test_restatement_equals_the_pair_routes_restatement(K):
    M = 2 * len(ss.KINDS)
    X, Y = ss.series(K, M)                                       # generic, tie runs, y on a draw, y outside, draws at 1e6
    assert len({ss.KINDS[s % len(ss.KINDS)] for s in range(M)}) == len(ss.KINDS)
    for fair in fairs(K):
        o, ref = ss.value_grad(X, Y, fair), sg.value_grad(X[:, :, None], Y[:, None], fair)
        err, tol = np.abs(o["crps"] - ref["scores"]), sg.RTOL * ref["smag"]
        print("K=%d fair=%s: crps off the pair route by at most %.3g of the bound" % (K, fair, float((err / np.where(tol > 0, tol, 1)).max())))
        assert (err <= tol).all(), (K, fair, err, tol)
        assert (o["smag"] >= ref["smag"] * (1 - sg.RTOL)).all()      # |c_i t_(i)| bounds the run of pair terms it stands for
        # the gradients agree to the rounding of the pair route's three-step expression on any data
        assert (np.abs(o["grad_x"] - ref["grad_x"][:, :, 0]) <= sg.RTOL * ref["mx"][:, :, 0]).all()
        assert (np.abs(o["grad_y"] - ref["grad_y"][:, 0]) <= sg.RTOL * ref["my"][:, 0]).all()


@pytest.mark.parametrize("K", KS)
def test_gradients_equal_the_pair_routes_on_exact_data(K):
    for d in range(1, 7):                                        # the data's differences: c (x_k - x_l) is exactly 1
        assert (1.0 / d) * d == 1.0
    X, Y = ss.integer_series(K, 40)
    for fair in fairs(K):
        D = K - 1 if fair else K
        o, ref = ss.value_grad(X, Y, fair), sg.value_grad(X[:, :, None], Y[:, None], fair)
        gx, gy = ref["grad_x"][:, :, 0], ref["grad_y"][:, 0]
        sgn = np.sign(X - Y[None]).astype(np.int64)
        # the integer numerators, formed exactly by both routes
        assert np.array_equal(np.rint(gx * (K * D)).astype(np.int64), sgn * D - o["c"])
        assert np.array_equal(np.rint(gy * K).astype(np.int64), -sgn.sum(axis=0))
        # grad_y = -(sum sgn) / K is one division in both routes
        assert np.array_equal(o["grad_y"], gy)
        once = K & (K - 1) == 0 and D & (D - 1) == 0             # 1 / K and 1 / (K D) are powers of two: the pair route rounds once
        if once:
            assert np.array_equal(o["grad_x"], gx)
        else:
            mag = 1.0 / K + np.abs(o["c"]) / float(K * D)
            assert (np.abs(o["grad_x"] - gx) <= 4 * U53 * mag).all()
    # a tie and a draw on its target: the subgradient 0 of the pair route
    o = ss.value_grad(np.array([[1.0], [1.0], [2.0]]), np.array([1.0]), False)
    assert o["c"][:, 0].tolist() == [-1, -1, 2] and np.array_equal(o["grad_x"][:, 0], np.array([1, 1, 1]) / 9.0)
    assert o["grad_y"][0] == -(1 / 3.0)


@pytest.mark.parametrize("fair", (False, True))
@pytest.mark.parametrize("K", (2, 3, 33, 257))
def test_restatement_equals_the_restatement_of_sample_scores(K, fair):
    M = 2 * len(ss.KINDS)
    X, Y = ss.series(K, M)
    X, Y = X.astype(np.float32), Y.astype(np.float32)
    o = ss.value_grad(X, Y, fair, ss.LEVELS)
    ref = sn.scores(np.ascontiguousarray(X.T[None]), Y[None], ss.LEVELS, fair)                   # xt [1, M, K]
    scale = sn.scale_of(np.ascontiguousarray(X.T[None]), Y[None])[0]
    tol = 2.0 * K * U53 * scale + sg.RTOL * o["smag"] + K * K * U53 * o["smag"]                     # sn.bound without its float32 ulp; the pair sum's K^2 terms
    assert (np.abs(o["crps"] - ref.crps[0]) <= tol).all(), (np.abs(o["crps"] - ref.crps[0]) / tol).max()
    tol = 16.0 * U53 * scale                                     # the quantile is lerped on x there, on x - y here: seven roundings
                                                                 # in the two routes together, each below 2^-53 of 2 max(|x|, |y|)
    assert (np.abs(o["pinball"] - ref.pinball[:, 0]) <= tol[None]).all()
    # the quantile itself: Q_p = y + lerp(t) against numpy's on the draws
    i0, frac = ss.level_parts(ss.LEVELS, K)
    ts = np.sort(X.astype(np.float64) - Y[None].astype(np.float64), axis=0)
    qt = ss.lerp(ts[i0], ts[np.minimum(i0 + 1, K - 1)], frac[:, None])
    assert (np.abs(qt + Y[None].astype(np.float64) - ref.quantiles[:, 0]) <= tol[None]).all()


def test_restatement_on_hand_made_data():
    # draws 0, 1, 2, 3 against y = 1.5: sum |t| = 4, pairs sum |x_k - x_l| over k < l = 10
    X, Y = np.array([[0.0], [3.0], [1.0], [2.0]]), np.array([1.5])
    o = ss.value_grad(X, Y, False, (0.0, 0.5, 1.0, 0.25))
    assert o["crps"][0] == 4 / 4 - 10 / 16 and o["order"][:, 0].tolist() == [0, 2, 3, 1] and o["c"][:, 0].tolist() == [-3, 3, -1, 1]
    assert abs(ss.value_grad(X, Y, True)["crps"][0] - (4 / 4 - 10 / 12)) <= 2 * U53
    assert np.array_equal(o["grad_x"][:, 0], np.array([-4 + 3, 4 - 3, -4 + 1, 4 - 1]) / 16.0) and o["grad_y"][0] == 0.0
    # quantiles 0, 1.5, 3, 0.75 -> Q - y = -1.5, 0, 1.5, -0.75
    assert np.array_equal(o["side"][:, 0], [0.0, 0.5, 0.0, 0.25]) and np.array_equal(o["pinball"][:, 0], [0.0, 0.0, 0.0, 0.75 * 0.25])
    assert o["idx"][:, 0].tolist() == [[0, 2], [2, 3], [3, 1], [0, 2]]
    gx, gy = ss.pinball_grad(o["idx"], o["side"], np.ones((4, 1)), (0.0, 0.5, 1.0, 0.25), 4)
    assert gy[0] == 0.75 and np.array_equal(gx[:, 0], [-0.25 * 0.25, 0.0, -0.25 - 0.25 * 0.75, -0.25])
    # K = 1, fair=False: the absolute error; every level is the draw
    o = ss.value_grad(np.array([[3.0, 1.0]]), np.array([1.0, 1.0]), False, (0.3,))
    assert np.array_equal(o["crps"], [2.0, 0.0]) and np.array_equal(o["grad_x"], [[1.0, 0.0]]) and np.array_equal(o["grad_y"], [-1.0, 0.0])
    assert o["idx"].tolist() == [[[0, 0], [0, 0]]] and np.array_equal(o["pinball"][0], [2.0 * 0.7, 0.0])
    # a NaN stays in its series
    X, Y = ss.series(5, 4)
    X[2, 1], Y[3] = np.nan, np.nan
    o = ss.value_grad(X, Y, True, (0.5,))
    bad = [False, True, False, True]
    for name in ("crps", "grad_y"):
        assert np.isnan(o[name]).tolist() == bad, name
    assert np.isnan(o["grad_x"]).all(axis=0).tolist() == bad and np.isnan(o["grad_x"]).any(axis=0).tolist() == bad
    assert np.isnan(o["pinball"][0]).tolist() == bad and np.isnan(o["side"][0]).tolist() == bad


# ---- central differences ---------------------------------------------------------------------------------------------------

def central(fn, X, Y):
    """d fn / d X and d fn / d Y of the MEAN score by central differences, times the number of series"""
    out = []
    for name, A in (("x", X), ("y", Y)):
        G = np.empty_like(A)
        for at in np.ndindex(A.shape):
            v = []
            for step in (H, -H):
                B = A.copy()
                B[at] += step
                v.append(fn(B, Y) if name == "x" else fn(X, B))
            G[at] = (v[0] - v[1]) / (2 * H)
        out.append(G)
    return out


@pytest.mark.parametrize("K", (1, 2, 3, 5))
def test_restatement_gradient_equals_central_differences(K):
    M = 3
    for fair in fairs(K):
        X, Y = ss.separated_series(K, M)
        o = ss.value_grad(X, Y, fair)
        fx, fy = central(lambda A, B: ss.mean_score(A, B, fair) * M, X, Y)
        worst = max(np.abs(fx - o["grad_x"]).max(), np.abs(fy - o["grad_y"]).max())
        print("crps K=%d fair=%s: gradient off central differences by at most %.3g" % (K, fair, worst))
        assert worst <= FD_TOL
        assert (np.abs(o["grad_x"].sum(axis=0) + o["grad_y"]) <= 1e-15 * K).all()                 # translation invariance
    levels = (0.0, 0.05, 0.5, 0.95, 1.0, 0.5)
    Q = len(levels)
    X, Y = ss.separated_series(K, M, levels=levels)
    o = ss.value_grad(X, Y, False, levels)
    assert np.abs(o["qt"]).min() >= 0.3                           # |Q_p - y| of every level
    rng = np.random.RandomState(K)
    g = rng.uniform(0.5, 1.5, size=(Q, M))                        # a weighted sum of the scores: the node's incoming gradient
    gx, gy = ss.pinball_grad(o["idx"], o["side"], g, levels, K)
    fx, fy = central(lambda A, B: float((g * ss.value_grad(A, B, False, levels)["pinball"]).sum()), X, Y)
    worst = max(np.abs(fx - gx).max(), np.abs(fy - gy).max())
    print("pinball K=%d: gradient off central differences by at most %.3g" % (K, worst))
    assert worst <= FD_TOL


# ---- header, binding, plan, statuses -------------------------------------------------------------------------------------

def test_header_declarations_equal_the_binding():
    raw = open(os.path.join(CSRC, "pf_metrics.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = re.findall(r"\b(pfm_[a-z0-9_]+)\s*\(", text)
    assert sorted(declared) == sorted(_lib.EXPORTS) and set(NEW) <= set(_lib.EXPORTS)
    assert _lib.ABI_VERSION == 101 and "#define PFM_VERSION 101 " in raw
    assert "#define PFM_SORT_MAX_K %d " % _lib.SORT_MAX_K in raw and _lib.SORT_MAX_K == 8192
    assert "#define PFM_SORT_MAX_Q %d " % _lib.SORT_MAX_Q in raw and _lib.SORT_MAX_Q == 16
    assert "pf_sortscore.o" in open(os.path.join(CSRC, "Makefile")).read()
    source = re.sub(r"//.*", "", open(os.path.join(CSRC, "pf_sortscore.hip")).read())
    assert "atomic" not in source.lower() and '#include "pf_segsort.h"' in source
    for name in NEW:
        args = re.search(r"\b%s\s*\(([^)]*)\)" % name, text).group(1)
        assert len(args.split(",")) == len(_lib._SIGNATURES[name][1]), name


def plan_restated(M, K):
    """pf_metrics.h, pfm_sort_score_plan: an odd pitch; 64 KiB of 16-byte entries and the sums' scratch, or one series"""
    scratch = 256 * (8 + 8 + 4)
    pitch = K | 1
    G = max(1, ((64 * 1024 - scratch) // 16) // pitch)
    return G, pitch, 16 * G * pitch + scratch, -(-M // G)


BAD_SIZES = ((0, 2), (-1, 2), (5, 0), (5, -3), (2 ** 31, 2))
ABOVE = ((5, _lib.SORT_MAX_K + 1), (5, 2 ** 40))


def test_plan_needs_no_device_and_equals_its_restatement():
    native_libs.ensure_built(_lib)
    assert _lib.lib().pfm_sort_score_plan(10, 4, None) == _lib.PFM_EINVAL
    for bad in BAD_SIZES:
        assert _lib.sort_score_plan_status(*bad)[0] == _lib.PFM_EINVAL, bad
    for bad in ABOVE:
        assert _lib.sort_score_plan_status(*bad)[0] == _lib.PFM_EUNSUPPORTED, bad
    seen = set()
    for K in (1, 2, 31, 32, 33, 1024, 8192):
        for M in (1, 7, 4096, 10 ** 6):
            st, plan = _lib.sort_score_plan_status(M, K)
            G, pitch, lds, wgs = plan
            assert st == 0 and plan == plan_restated(M, K), (M, K, plan)
            assert G >= 1 and pitch >= K and wgs == -(-M // G) and 16 * G * K <= lds <= LDS_CU, (M, K, plan)
            if K >= 32:
                assert (pitch * 8) % 256 != 0, (K, pitch)
            assert plan[:3] == _lib.sort_score_plan(1, K)[:3]            # only the workgroups depend on M
            seen.add(G > 1)
    assert seen == {False, True} and _lib.sort_score_plan(1, 8192)[0] == 1 and _lib.sort_score_plan(1, 2)[0] > 256


def test_workspace_query_and_argument_statuses_without_a_device():
    native_libs.ensure_built(_lib)
    L = _lib.lib()
    assert L.pfm_version() == _lib.ABI_VERSION == 101 and all(hasattr(L, name) for name in NEW)
    q = _lib.sort_score_workspace_bytes
    assert 0 < q(1, 1) == q(65536 * 16, 32, 2) == q(2 ** 31 - 1, 8192, 16) <= 4096            # a constant: nothing of size K or M
    for M, K in BAD_SIZES + ABOVE:
        assert q(M, K) == 0 and q(M, K, 2) == 0, (M, K)
    assert q(5, 4, -1) == 0 and q(5, 4, 17) == 0
    fake = ctypes.c_void_p(256)
    E, U, W = _lib.PFM_EINVAL, _lib.PFM_EUNSUPPORTED, _lib.PFM_EWORKSPACE

    def levels(*p):
        return ctypes.cast((ctypes.c_double * max(1, len(p)))(*p), ctypes.c_void_p)

    def score(X=fake, Y=fake, M=10, K=4, fair=1, lv=levels(0.05, 0.95), Q=2, crps=fake, gx=fake, gy=fake, pin=fake, side=fake,
              idx=fake, ws=fake, nbytes=1 << 20):
        return L.pfm_sort_score(None, X, Y, M, K, fair, lv, Q, crps, gx, gy, pin, side, idx, ws, nbytes)

    # refused before anything is read or launched (the device pointers are never dereferenced)
    assert score(X=None) == score(Y=None) == E
    for M, K in BAD_SIZES:
        assert score(M=M, K=K) == E and score(M=M, K=K, fair=0) == E, (M, K)
    assert score(K=1, fair=1) == E and score(K=1, fair=7) == E
    for bad in (-0.001, 1.001, float("nan"), float("inf"), -float("inf")):
        assert score(lv=levels(0.5, bad)) == E and score(lv=levels(bad), Q=1, nbytes=0) == E, bad
    assert score(Q=-1) == E and score(lv=None) == E
    assert score(Q=0, lv=None) == E                                  # pinball, side and idx given without a level
    assert score(crps=None, gx=None, gy=None, pin=None, side=None, idx=None) == E            # no output at all
    assert score(crps=None, gx=None, gy=None, pin=None, side=None, idx=None, Q=0, lv=None) == E
    for M, K in ABOVE:
        assert score(M=M, K=K) == U, (M, K)
    assert score(Q=17, lv=levels(*([0.5] * 17))) == U
    assert score(ws=None) == W and score(nbytes=q(10, 4, 2) - 1) == W
    assert score(Q=0, lv=None, pin=None, side=None, idx=None, gx=None, gy=None, nbytes=0) == W
    assert score(K=1, fair=0, crps=None, gx=None, gy=None, nbytes=0) == W

    def grad(idx=fake, side=fake, g=fake, lv=levels(0.05, 0.95), Q=2, M=10, K=4, gx=fake, gy=fake, ws=fake, nbytes=1 << 20):
        return L.pfm_pinball_grad(None, idx, side, g, lv, Q, M, K, gx, gy, ws, nbytes)

    assert grad(idx=None) == grad(side=None) == grad(g=None) == grad(lv=None) == E
    assert grad(gx=None, gy=None) == E and grad(Q=0) == E and grad(Q=-1) == E
    for M, K in BAD_SIZES:
        assert grad(M=M, K=K) == E, (M, K)
    for bad in (-0.001, 1.001, float("nan")):
        assert grad(lv=levels(0.5, bad)) == E
    for M, K in ABOVE:
        assert grad(M=M, K=K) == U, (M, K)
    assert grad(Q=17, lv=levels(*([0.5] * 17))) == U
    assert grad(ws=None) == W and grad(nbytes=255) == W and grad(gx=None, nbytes=0) == W


# ---- the public calls' argument checks ----------------------------------------------------------------------------------

def test_argument_errors_are_raised_before_any_device_is_touched(monkeypatch):
    def touched(*a, **k):
        raise AssertionError("an argument error must be raised before anything touches a device")
    for name in ("sort_score", "pinball_grad", "sort_score_workspace_bytes", "score_grad", "score_grad_workspace_bytes"):
        monkeypatch.setattr(_lib, name, touched)
    monkeypatch.setattr(torch.cuda, "is_available", touched)
    X, Y = np.zeros((4, 5, 3)), np.ones((5, 3))
    sorted_crps = lambda a, b, **kw: losses.crps_loss(a, b, method="sorted", **kw)  # noqa: E731
    for fn in (sorted_crps, losses.pinball_loss):
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
        for bad in ("sum", None, 1, "Mean"):
            with pytest.raises(ValueError, match="reduction must be"):
                fn(X, Y, reduction=bad)
        with pytest.raises(ValueError, match="at most 8192 draws"):
            fn(np.zeros((_lib.SORT_MAX_K + 1, 2, 1)), np.zeros((2, 1)))
    for bad in (1, 0, None, "yes"):
        with pytest.raises(ValueError, match="fair must be a bool"):
            sorted_crps(X, Y, fair=bad)
    with pytest.raises(ValueError, match="at least 2 draws"):
        sorted_crps(X[:1], Y)
    for bad in ("sort", "Sorted", None, 1, True):
        with pytest.raises(ValueError, match="method must be 'pairs' or 'sorted'"):
            losses.crps_loss(X, Y, method=bad)
    for bad in ((), [], [0.5] * 17, np.zeros(0)):
        with pytest.raises(ValueError, match="1 to 16"):
            losses.pinball_loss(X, Y, quantiles=bad)
    for bad in (-0.1, 1.5, float("nan"), [0.5, 1.0001], (0.5, None), "0.5", [True], float("inf"), np.zeros((2, 2))):
        with pytest.raises(ValueError, match=r"in \[0, 1\]"):
            losses.pinball_loss(X, Y, quantiles=bad)


def test_the_default_method_is_the_pair_route_as_before(monkeypatch):
    calls = []
    monkeypatch.setattr(losses, "_score_loss", lambda *a: calls.append(a) or "pairs")
    X, Y = np.zeros((4, 5, 3)), np.ones((5, 3))
    assert losses.crps_loss(X, Y) == "pairs" and losses.crps_loss(X, Y, method="pairs") == "pairs"
    assert losses.crps_loss(X, Y, False, "none") == "pairs" and losses.crps_loss(X, Y, fair=False, reduction="none", method="pairs") == "pairs"
    assert all(c[0] is X and c[1] is Y for c in calls)
    assert [c[2:] for c in calls] == [(True, "mean", True)] * 2 + [(False, "none", True)] * 2
    # the pair route keeps its limit: the sorted route's does not leak into it
    monkeypatch.undo()
    with pytest.raises(ValueError, match="at most 1024 draws"):
        losses.crps_loss(np.zeros((_lib.SCORE_MAX_K + 1, 2, 1)), np.zeros((2, 1)))
    with pytest.raises(ValueError, match="at most 1024 draws"):
        losses.crps_loss(np.zeros((_lib.SCORE_MAX_K + 1, 2, 1)), np.zeros((2, 1)), method="pairs")


def test_new_names_stay_out_of_the_export_list():
    import probaforms_amd.metrics as m
    assert m.__all__ == ["frechet_distance", "maximum_mean_discrepancy"]
    assert not hasattr(m, "pinball_loss") and callable(losses.pinball_loss)
    assert "not provided" not in losses.crps_loss.__doc__ and "sorted" in losses.crps_loss.__doc__
