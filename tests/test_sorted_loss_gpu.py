"""probaforms_amd.metrics.losses.crps_loss(method="sorted") / pinball_loss on the GPU (pfm_sort_score and pfm_pinball_grad in
libpf_metrics.so) against the float64 restatement (tests/sortscore_numpy.py), the pair route, the restatement of sample_scores,
torch's gradcheck, and the write-bounds, workspace and stream drivers.

Tolerances.  The CRPS is two sums of K terms each and two products: it is held within RTOL = 1e-12 (scoregrad_numpy.RTOL, the
project's bound) of the sum of the magnitudes of its terms, from the restatement; a float64 sum of at most 2 x 8192 correctly rounded
terms in any order stays within 16384 2^-53 = 1.8e-12 of that sum in the worst case and within its square root's share, 1e-14, for
roundings of either sign; the largest ratio seen is printed by test_zz_largest_deviation (on an MI355X: 0.19 of the bound for a
CRPS, and the pinball scores equal the restatement's bitwise).  A pinball score is a lerp of two values
and one product, a few 2^-53 of |t_(i)| + |t_(i+1)|: the same bound.  grad_x, grad_y, side and idx have nothing to bound: integers
formed exactly and at most one division, compared with ==.  On integer draws with fair=False and K a power of two every sum is an
integer and every scale a power of two, so the values are compared with == too.

Shapes: every K of KS (K = 1 with fair=False only) at M in 1, G - 1, G, G + 1, 2 G + 3, G the series a workgroup takes
(pfm_sort_score_plan: 3776 at K = 1, 1258 at K = 2, 1 from K = 1888 on), and at M = 18, where every kind of series of sortscore_numpy.KINDS comes
twice: generic, all draws equal, two distinct values, a long tie run (300 draws at K >= 1024), y on a draw, y outside the range on
either side, signed zeros among the draws, draws at 1e6.
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bounds  # noqa: E402
import hygiene  # noqa: E402
import native_libs  # noqa: E402
import scoregrad_numpy as sg  # noqa: E402
import scores_numpy as sn  # noqa: E402
import sortscore_numpy as ss  # noqa: E402
import streams  # noqa: E402
from probaforms_amd.metrics import _lib, losses  # noqa: E402

pytestmark = pytest.mark.gpu

native_libs.ensure_built(_lib)

RTOL = sg.RTOL
F64, I32 = torch.float64, torch.int32
KS = (1, 2, 3, 5, 31, 32, 33, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097, 8191, 8192)
LEVELS = ss.LEVELS + (0.5,)                                   # the last meets the third on one order statistic
Q = len(LEVELS)
ALL_KINDS = 2 * len(ss.KINDS)
WORST = {"crps": 0.0, "pinball": 0.0}


def G_of(K):
    return _lib.sort_score_plan(1, K)[0]


def sizes(K):
    G = G_of(K)
    return sorted({M for M in (1, G - 1, G, G + 1, 2 * G + 3, ALL_KINDS) if M >= 1})


CASES = [(K, M) for K in KS for M in sizes(K)]
assert max(M for _, M in CASES) <= 7600 and max(M for K, M in CASES if K >= 1024) <= ALL_KINDS      # 2 x 3776 + 3 at K = 1


def case_id(case):
    return "K%d_M%d" % case


def fairs(K):
    return (False,) if K == 1 else (False, True)


def dev(A, grad=False, dtype=F64):
    return torch.from_numpy(np.array(A)).to(device="cuda", dtype=dtype).requires_grad_(grad)


@functools.lru_cache(maxsize=None)
def reference(case, fair):
    """(X, Y, restatement dict) of a case: computed once, shared, never written to"""
    K, M = case
    X, Y = ss.series(K, M)
    o = ss.value_grad(X, Y, fair, LEVELS)
    for a in (X, Y) + tuple(o.values()):
        a.setflags(write=False)
    return X, Y, o


NAMES = ("crps", "grad_x", "grad_y", "pinball", "side", "idx")


def raw(X, Y, fair, levels=LEVELS, want=NAMES):
    """pfm_sort_score once -> dict of numpy arrays (the outputs asked for)"""
    Xd, Yd = dev(X), dev(Y)
    K, M = Xd.shape
    nq = len(levels)
    shapes = dict(crps=(M,), grad_x=(K, M), grad_y=(M,), pinball=(nq, M), side=(nq, M), idx=(nq, M, 2))
    out = {k: torch.empty(shapes[k], dtype=I32 if k == "idx" else F64, device="cuda") for k in want}
    hygiene.poison_outputs(*out.values())
    ws = torch.empty(_lib.sort_score_workspace_bytes(M, K, nq), dtype=torch.uint8, device="cuda")
    _lib.sort_score(Xd, Yd, fair, levels, *[out.get(k) for k in NAMES], ws)
    return {k: v.cpu().numpy() for k, v in out.items()}


def raw_grad(idx, side, g, levels, K, gx=True, gy=True):
    """pfm_pinball_grad once -> (grad_x or None, grad_y or None) as numpy arrays"""
    nq, M = side.shape
    ox = torch.empty((K, M), dtype=F64, device="cuda") if gx else None
    oy = torch.empty(M, dtype=F64, device="cuda") if gy else None
    hygiene.poison_outputs(ox, oy)
    ws = torch.empty(_lib.sort_score_workspace_bytes(M, K, nq), dtype=torch.uint8, device="cuda")
    _lib.pinball_grad(dev(idx, dtype=I32), dev(side), dev(g), levels, K, ox, oy, ws)
    return (None if ox is None else ox.cpu().numpy()), (None if oy is None else oy.cpu().numpy())


def assert_equals_restatement(got, want, what, exact_values=False):
    for name, mag in (("crps", "smag"), ("pinball", "pmag")):
        if name not in got:
            continue
        err, m = np.abs(got[name] - want[name]), want[mag]
        rel = float((err / np.where(m > 0, m, 1.0)).max())
        WORST[name] = max(WORST[name], rel / RTOL)
        print("%s: %s off by at most %.3g of its terms' magnitudes (bound %.3g)" % (what, name, rel, RTOL))
        assert np.isfinite(got[name]).all() and (err <= RTOL * m).all(), (what, name, rel)
        if exact_values:
            assert np.array_equal(got[name], want[name]), (what, name)
    for name in ("grad_x", "grad_y", "side", "idx"):
        if name in got:
            assert got[name].dtype == want[name].dtype and np.array_equal(got[name], want[name]), (what, name)


def same(a, b):
    return a.tobytes() == b.tobytes()


# ---- the kernels against the restatement ----------------------------------------------------------------------------------

def test_the_cases_reach_one_and_many_series_per_workgroup_and_many_workgroups():
    plans = [_lib.sort_score_plan(M, K) for K, M in CASES]
    assert any(p[0] == 1 for p in plans) and any(p[0] > 256 for p in plans) and any(1 < p[0] < 256 for p in plans)
    assert any(p[3] > 1 and p[0] > 1 for p in plans) and any(p[3] > 1 and p[0] == 1 for p in plans)
    assert all(p[2] <= 160 * 1024 for p in plans) and any(p[2] > 64 * 1024 for p in plans)
    for K, M in CASES:                                           # whole workgroups, a ragged last one, one series short of one
        G = G_of(K)
        assert {1, G, G + 1, 2 * G + 3} <= set(sizes(K))


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_scores_gradients_and_quantiles_equal_the_restatement(case):
    K, M = case
    rng = np.random.RandomState(K + M)
    for fair in fairs(K):
        X, Y, want = reference(case, fair)
        got = raw(X, Y, fair)
        assert_equals_restatement(got, want, "%s fair=%s" % (case_id(case), fair))
        # the values alone, and the quantile outputs alone, are formed alike
        assert same(raw(X, Y, fair, (), ("crps",))["crps"], got["crps"])
        alone = raw(X, Y, False, LEVELS, ("pinball",))
        assert same(alone["pinball"], got["pinball"])
    # the pinball scores' derivative from what the call left
    g = rng.uniform(0.5, 1.5, size=(Q, M)) * rng.choice([-1.0, 1.0], size=(Q, M))
    gx, gy = raw_grad(got["idx"], got["side"], g, LEVELS, K)
    wx, wy = ss.pinball_grad(want["idx"], want["side"], g, LEVELS, K)
    assert np.array_equal(gx, wx) and np.array_equal(gy, wy)
    assert same(raw_grad(got["idx"], got["side"], g, LEVELS, K, gy=False)[0], gx)
    assert same(raw_grad(got["idx"], got["side"], g, LEVELS, K, gx=False)[1], gy)


@pytest.mark.parametrize("K", (2, 32, 64, 256, 1024, 8192))
def test_integer_draws_agree_bit_for_bit(K):
    M = 2 * G_of(K) + 3 if K >= 256 else 40
    X, Y = ss.integer_series(K, M)
    want = ss.value_grad(X, Y, False, LEVELS)
    assert_equals_restatement(raw(X, Y, False), want, "integers K=%d" % K, exact_values=True)
    if K > 2:                                                    # fair: K D is no power of two; the bound
        assert_equals_restatement(raw(X, Y, True), ss.value_grad(X, Y, True, LEVELS), "integers K=%d fair" % K)


def test_every_draw_on_the_target_gives_exact_zeros():
    for K in (1, 3, 64, 1025):
        Y = np.array([1.5, -2.0, 1e6])
        X = np.broadcast_to(Y[None], (K, 3)).copy()
        got = raw(X, Y, False)
        assert not got["crps"].any() and not got["grad_x"].any() and not got["grad_y"].any() and not got["pinball"].any()
        assert np.array_equal(got["side"], np.broadcast_to(np.array(LEVELS)[:, None], (Q, 3)))        # y < Q_p nowhere


# ---- reproducibility -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", (3, 33, 257, 1025, 8192))
def test_a_series_outputs_do_not_depend_on_m_position_or_the_outputs_asked_for(K):
    G = G_of(K)
    M = 2 * G + 3 if G > 1 else 7
    X, Y = ss.series(K, M)
    full = raw(X, Y, True)
    again = raw(X, Y, True)
    assert all(same(full[k], again[k]) for k in full)            # two calls give identical bytes
    cut = M // 2 + 1
    for a, b in ((0, 1), (1, 2), (0, cut), (cut, M), (M - 1, M), (G - 1 if G > 1 else 2, min(M, G + 2))):
        part = raw(X[:, a:b], Y[a:b], True)
        for k in NAMES:
            axis = 0 if full[k].ndim == 1 else 1
            assert same(part[k], np.ascontiguousarray(np.take(full[k], np.arange(a, b), axis=axis))), (k, a, b)
    for want in (("crps",), ("grad_x",), ("grad_y",), ("crps", "grad_y"), ("pinball",), ("side", "idx"), ("grad_x", "idx")):
        part = raw(X, Y, True, LEVELS if set(want) & {"pinball", "side", "idx"} else (), want)
        assert all(same(part[k], full[k]) for k in want), want
    # the levels do not meet each other either
    one = raw(X, Y, True, (LEVELS[1],), ("pinball", "side", "idx"))
    assert same(one["pinball"][0], full["pinball"][1]) and same(one["idx"][0], full["idx"][1])


@pytest.mark.parametrize("K", (3, 33, 1025))
def test_a_nan_stays_in_its_series(K):
    M = G_of(K) + 4
    X, Y = ss.series(K, M)
    clean = raw(X, Y, True)
    X, Y = X.copy(), Y.copy()
    X[K // 2, 1] = np.nan
    Y[4] = np.nan
    X[K - 1, 6] = np.inf                                         # not part of the contract, except that it stays in its series
    got = raw(X, Y, True)
    bad = np.zeros(M, bool)
    bad[[1, 4]] = True
    finite = np.arange(M) != 6                                   # (the series with the infinity: whatever the formulas give)
    for k in ("crps", "grad_y"):
        assert np.array_equal(np.isnan(got[k])[finite], bad[finite]), k
    assert np.isnan(got["grad_x"][:, bad]).all() and np.isnan(got["pinball"][:, bad]).all() and np.isnan(got["side"][:, bad]).all()
    assert (got["idx"] >= 0).all() and (got["idx"] < K).all()
    keep = ~bad
    keep[6] = False
    for k in NAMES:
        axis = 0 if got[k].ndim == 1 else 1
        assert same(np.compress(keep, got[k], axis=axis), np.compress(keep, clean[k], axis=axis)), k
    # the derivative of the pinball scores: NaN for the series' target and for the draws named, nothing else
    g = np.ones((Q, M))
    gx, gy = raw_grad(got["idx"], got["side"], g, LEVELS, K)
    assert np.array_equal(np.isnan(gy)[finite], bad[finite]) and not np.isnan(gx[:, keep]).any() and np.isnan(gx[:, bad]).any(axis=0).all()


@pytest.mark.parametrize("case", [(5, 7), (33, 2 * (3776 // 33) + 3), (8192, 3)], ids=case_id)
def test_outputs_do_not_depend_on_the_workspace_and_are_all_written(case):
    K, M = case
    X, Y = ss.series(K, M)
    Xd, Yd = dev(X), dev(Y)
    nbytes = _lib.sort_score_workspace_bytes(M, K, Q)
    g = dev(np.random.RandomState(1).normal(size=(Q, M)))
    outs = {}
    for pattern in ("zeros", "ones", "huge"):
        o = dict(crps=torch.empty(M, dtype=F64, device="cuda"), grad_x=torch.empty_like(Xd), grad_y=torch.empty_like(Yd),
                 pinball=torch.empty((Q, M), dtype=F64, device="cuda"), side=torch.empty((Q, M), dtype=F64, device="cuda"),
                 idx=torch.empty((Q, M, 2), dtype=I32, device="cuda"), pin_gx=torch.empty_like(Xd), pin_gy=torch.empty_like(Yd))
        hygiene.poison_outputs(*o.values())
        _lib.sort_score(Xd, Yd, True, LEVELS, *[o[k] for k in NAMES], hygiene.workspace(nbytes, pattern))
        _lib.pinball_grad(o["idx"], o["side"], g, LEVELS, K, o["pin_gx"], o["pin_gy"], hygiene.workspace(nbytes, pattern))
        torch.cuda.synchronize()
        hygiene.assert_all_written(o, "pfm_sort_score / pfm_pinball_grad %s %s" % (case_id(case), pattern))
        outs[pattern] = o
    hygiene.assert_pattern_independent(outs, "pfm_sort_score / pfm_pinball_grad %s" % case_id(case))


# ---- write bounds and streams ---------------------------------------------------------------------------------------------

GUARDED = [(5, 7), (33, 2 * (3776 // 33) + 3), (8192, 2)]       # one small, one of several workgroups, one that takes a CU's LDS


def guarded_calls(case):
    K, M = case
    X, Y = ss.series(K, M)
    Xd, Yd = dev(X), dev(Y)
    need = _lib.sort_score_workspace_bytes(M, K, Q)
    Out = bounds.Out
    tag = "%d draws, %d series" % (K, M)
    yield ("pfm_sort_score[%s]" % tag, need,
           lambda ws, o: _lib.sort_score_status(Xd, Yd, True, LEVELS, *[o[k] for k in NAMES], ws),
           dict(crps=Out(F64, (M,)), grad_x=Out(F64, (K, M)), grad_y=Out(F64, (M,)), pinball=Out(F64, (Q, M)), side=Out(F64, (Q, M)),
                idx=Out(I32, (Q, M, 2))), dict(X=Xd, Y=Yd))
    yield ("pfm_sort_score[%s, values alone]" % tag, need,
           lambda ws, o: _lib.sort_score_status(Xd, Yd, False, LEVELS[:2], o["crps"], None, None, o["pinball"], None, None, ws),
           dict(crps=Out(F64, (M,)), pinball=Out(F64, (2, M))), dict(X=Xd, Y=Yd))
    left = raw(X, Y, False, LEVELS, ("side", "idx"))
    idx, side = dev(left["idx"], dtype=I32), dev(left["side"])
    g = dev(np.random.RandomState(K).normal(size=(Q, M)))
    yield ("pfm_pinball_grad[%s]" % tag, need,
           lambda ws, o: _lib.pinball_grad_status(idx, side, g, LEVELS, K, o["grad_x"], o["grad_y"], ws),
           dict(grad_x=Out(F64, (K, M)), grad_y=Out(F64, (M,))), dict(idx=idx, side=side, g=g))


@pytest.mark.parametrize("case", GUARDED, ids=case_id)
def test_no_write_outside_the_workspace_and_the_outputs(case):
    assert _lib.sort_score_plan(*case[::-1])[3] > 1 or case == GUARDED[0]
    for what, need, call, outs, inputs in guarded_calls(case):
        bounds.run(what, need, call, outs, inputs, keeps_nothing=True)


@pytest.mark.parametrize("case", GUARDED, ids=case_id)
def test_everything_is_enqueued_on_the_callers_stream(case):
    for what, need, call, outs, inputs in guarded_calls(case):
        res = streams.run(what, need, call, outs, inputs)
        assert res["pending"] and res["captured"], what


# ---- the public layer -----------------------------------------------------------------------------------------------------

def stacked(K, n, d, seed=0):
    """X [K, n, d], Y [n, d] from sortscore_numpy.series"""
    X, Y = ss.series(K, n * d, seed)
    return X.reshape(K, n, d), Y.reshape(n, d)


@pytest.mark.parametrize("fair", (False, True))
@pytest.mark.parametrize("K", (2, 33, 257, 1024))
def test_the_sorted_route_agrees_with_the_pair_route(K, fair):
    n, d = 6, 3
    X, Y = stacked(K, n, d)
    want = ss.value_grad(X.reshape(K, n * d), Y.reshape(-1), fair)
    res = {}
    for method in ("pairs", "sorted"):
        A, B = dev(X, True), dev(Y, True)
        L = losses.crps_loss(A, B, fair=fair, reduction="none", method=method)
        assert L.shape == (n, d) and L.dtype == F64 and L.is_cuda and L.grad_fn is not None
        L.sum().backward()
        res[method] = [t.cpu().numpy() for t in (L.detach(), A.grad, B.grad)]
    (ps, px, py), (ss_, sx, sy) = res["pairs"], res["sorted"]
    smag = want["smag"].reshape(n, d)
    assert (np.abs(ps - ss_) <= RTOL * smag).all(), float((np.abs(ps - ss_) / smag).max())
    D = K - 1 if fair else K
    mx = (1.0 / K + np.abs(want["c"]) / float(K * D)).reshape(K, n, d)      # the magnitudes of a gradient's two terms
    assert (np.abs(px - sx) <= RTOL * mx).all() and (np.abs(py - sy) <= RTOL).all()
    # the sorted route is the kernel's output, element for element; the mean is torch's
    assert np.array_equal(sx, want["grad_x"].reshape(K, n, d)) and np.array_equal(sy, want["grad_y"].reshape(n, d))
    V = losses.crps_loss(dev(X), dev(Y), fair=fair, method="sorted")
    assert V.shape == () and V.grad_fn is None and abs(float(V) - want["crps"].mean()) <= RTOL * want["smag"].mean()


def test_the_sorted_route_takes_what_the_pair_route_refuses():
    X, Y = stacked(8192, 2, 1)
    with pytest.raises(ValueError, match="at most 1024 draws"):
        losses.crps_loss(dev(X), dev(Y))
    A = dev(X, True)
    L = losses.crps_loss(A, dev(Y), method="sorted", reduction="none")
    L.sum().backward()
    want = ss.value_grad(X.reshape(8192, 2), Y.reshape(-1), True)
    assert (np.abs(L.detach().cpu().numpy().reshape(-1) - want["crps"]) <= RTOL * want["smag"]).all()
    assert np.array_equal(A.grad.cpu().numpy().reshape(8192, 2), want["grad_x"])


@pytest.mark.parametrize("K", (1, 2, 33, 257))
def test_pinball_loss_is_the_pinball_score_of_sample_scores(K):
    n, d = 6, 3
    X, Y = stacked(K, n, d)
    X, Y = X.astype(np.float32), Y.astype(np.float32)
    ref = sn.scores_of_stacked(X, Y, ss.LEVELS, False)
    P = losses.pinball_loss(X, Y, quantiles=ss.LEVELS, reduction="none")
    assert P.shape == (len(ss.LEVELS), n, d) and P.dtype == F64 and P.is_cuda and P.grad_fn is None
    scale = sn.scale_of(np.ascontiguousarray(np.moveaxis(X, 0, -1)), Y)
    tol = 16.0 * 2.0 ** -53 * scale                              # the quantile is lerped on x there, on x - y here: seven roundings
                                                                 # in the two routes together, each below 2^-53 of 2 max(|x|, |y|)
    assert (np.abs(P.cpu().numpy() - ref.pinball) <= tol[None]).all()
    V = losses.pinball_loss(X, Y, quantiles=ss.LEVELS)
    assert V.shape == () and abs(float(V) - float(P.mean())) <= 1e-15 * float(P.abs().max() + 1)
    band = losses.pinball_loss(X, Y, reduction="none")           # the default levels: the 5 % / 95 % band
    assert hygiene.same_bits(band, P[[1, 3]].contiguous())
    one = losses.pinball_loss(X, Y, quantiles=0.5, reduction="none")
    assert one.shape == (1, n, d) and hygiene.same_bits(one[0], P[2])


@pytest.mark.parametrize("fair", (False, True))
@pytest.mark.parametrize("reduction", ("mean", "none"))
def test_gradcheck_on_the_public_functions(fair, reduction):
    levels = (0.05, 0.5, 0.95, 1.0)
    for K in (2, 5):
        X, Y = ss.separated_series(K, 6, levels=levels)
        X, Y = X.reshape(K, 3, 2), Y.reshape(3, 2)
        assert torch.autograd.gradcheck(lambda a, b: losses.crps_loss(a, b, fair=fair, reduction=reduction, method="sorted"),
                                        (dev(X, True), dev(Y, True)))
        if not fair:
            assert torch.autograd.gradcheck(lambda a, b: losses.pinball_loss(a, b, quantiles=levels, reduction=reduction),
                                            (dev(X, True), dev(Y, True)))
    if not fair:
        X, Y = ss.separated_series(1, 6, levels=(0.3,))
        for fn in (lambda a, b: losses.crps_loss(a, b, fair=False, reduction=reduction, method="sorted"),
                   lambda a, b: losses.pinball_loss(a, b, quantiles=0.3, reduction=reduction)):
            assert torch.autograd.gradcheck(fn, (dev(X.reshape(1, 3, 2), True), dev(Y.reshape(3, 2), True)))


def test_two_levels_on_one_order_statistic_add_up():
    X, Y = np.array([[[0.0]], [[3.0]], [[1.0]]]), np.array([[2.5]])                               # K = 3: the median is draw 2
    A, B = dev(X, True), dev(Y, True)
    P = losses.pinball_loss(A, B, quantiles=(0.5, 0.5), reduction="none")
    (P * dev(np.array([1.0, 0.25]).reshape(2, 1, 1))).sum().backward()
    want = ss.value_grad(X.reshape(3, 1), Y.reshape(1), False, (0.5, 0.5))
    gx, gy = ss.pinball_grad(want["idx"], want["side"], np.array([[1.0], [0.25]]), (0.5, 0.5), 3)
    assert want["idx"].tolist() == [[[2, 1]], [[2, 1]]] and np.array_equal(P.detach().cpu().numpy().reshape(2, 1), want["pinball"])
    assert np.array_equal(A.grad.cpu().numpy().reshape(3, 1), gx) and np.array_equal(B.grad.cpu().numpy().reshape(1), gy)
    assert gx[:, 0].tolist() == [0.0, 0.0, -0.625] and gy[0] == 0.625


def test_gradient_goes_to_the_inputs_that_ask(monkeypatch):
    X, Y = stacked(33, 4, 2)
    seen = []
    score, grad = _lib.sort_score_status, _lib.pinball_grad_status

    def spy_score(X_, Y_, fair, levels, crps, gx, gy, pin, side, idx, ws):
        seen.append(("score", gx is not None, gy is not None, side is not None, idx is not None))
        return score(X_, Y_, fair, levels, crps, gx, gy, pin, side, idx, ws)

    def spy_grad(idx, side, g, levels, K, gx, gy, ws):
        seen.append(("grad", gx is not None, gy is not None))
        return grad(idx, side, g, levels, K, gx, gy, ws)
    monkeypatch.setattr(_lib, "sort_score_status", spy_score)
    monkeypatch.setattr(_lib, "pinball_grad_status", spy_grad)
    for fn in (lambda a, b: losses.crps_loss(a, b, method="sorted"), losses.pinball_loss):
        both = [dev(X, True), dev(Y, True)]
        fn(*both).backward()
        A, B = dev(X), dev(Y, True)
        fn(A, B).backward()
        assert A.grad is None and hygiene.same_bits(B.grad, both[1].grad)
        A, B = dev(X, True), dev(Y)
        (4 * fn(A, B)).backward()                                # (a power of two: the scaling commutes with the mean's 1 / n)
        assert B.grad is None and torch.equal(A.grad, 4 * both[0].grad)
        for a, b in ((dev(X), dev(Y)), (X, Y), (X.tolist(), dev(Y))):
            V = fn(a, b)
            assert V.grad_fn is None and not V.requires_grad and V.is_cuda and V.dtype == F64 and V.shape == ()
    assert seen[:6] == [("score", True, True, False, False), ("score", False, True, False, False), ("score", True, False, False, False)] \
        + [("score", False, False, False, False)] * 3
    assert seen[6:] == [("score", False, False, True, True), ("grad", True, True), ("score", False, False, True, True),
                        ("grad", False, True), ("score", False, False, True, True), ("grad", True, False)] \
        + [("score", False, False, False, False)] * 3


def test_float32_inputs_get_float32_gradients():
    X, Y = stacked(33, 4, 2)
    for fn in (lambda a, b: losses.crps_loss(a, b, method="sorted"), losses.pinball_loss):
        A, B = dev(X, True, torch.float32), dev(Y, True, torch.float32)
        L = fn(A, B)
        assert L.dtype == F64
        L.backward()
        assert A.grad.dtype == torch.float32 == B.grad.dtype and A.grad.shape == A.shape and B.grad.shape == B.shape
        A64, B64 = A.detach().double().requires_grad_(True), B.detach().double().requires_grad_(True)
        L64 = fn(A64, B64)
        L64.backward()
        assert hygiene.same_bits(L.reshape(1), L64.reshape(1))
        assert torch.equal(A.grad, A64.grad.float()) and torch.equal(B.grad, B64.grad.float())


def test_slices_and_permuted_views_give_the_result_of_their_contiguous_copies():
    X, Y = stacked(33, 7, 2)
    for fn in (lambda a, b: losses.crps_loss(a, b, method="sorted"), losses.pinball_loss):
        A, B = dev(X, True), dev(Y)
        L = fn(A, B)
        L.backward()
        T = A.detach().permute(1, 0, 2).contiguous().requires_grad_(True)      # [n, K, d]: the draws are its permuted view
        LT = fn(T.permute(1, 0, 2), B)
        LT.backward()
        assert hygiene.same_bits(L.reshape(1), LT.reshape(1)) and hygiene.same_bits(T.grad.permute(1, 0, 2), A.grad)
        W = dev(np.concatenate([X, X[:, :, ::-1]], axis=2), True)              # a slice of a wider tensor, every other row
        LS = fn(W[:, ::2, :2], B[::2])
        LS.backward()
        C = A.detach()[:, ::2].contiguous().requires_grad_(True)
        LC = fn(C, B[::2].contiguous())
        LC.backward()
        assert hygiene.same_bits(LS.reshape(1), LC.reshape(1)) and hygiene.same_bits(W.grad[:, ::2, :2].contiguous(), C.grad)
        assert not W.grad[:, 1::2].any() and not W.grad[:, :, 2:].any()


def test_forward_and_backward_never_wait_for_the_device():
    X, Y = stacked(33, 7, 2)
    A, B = dev(X, True), dev(Y, True)
    losses.crps_loss(A, B, method="sorted").backward()          # warm-up: library, code objects, allocator
    losses.pinball_loss(A, B, reduction="none").sum().backward()
    losses.crps_loss(A.detach(), B.detach(), method="sorted")
    A.grad = B.grad = None
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        L = losses.crps_loss(A, B, method="sorted")
        (2 * L).backward()
        P = losses.pinball_loss(A, B, quantiles=(0.1, 0.5, 0.9), reduction="none")
        P.sum().backward()
        losses.pinball_loss(A, B).backward()
        V = losses.crps_loss(A.detach(), B.detach(), fair=False, reduction="none", method="sorted")
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    want = ss.value_grad(X.reshape(33, 14), Y.reshape(-1), False)
    assert bool(torch.isfinite(A.grad).all()) and bool(A.grad.ne(0).any()) and bool(torch.isfinite(B.grad).all())
    assert (np.abs(V.cpu().numpy().reshape(-1) - want["crps"]) <= RTOL * want["smag"]).all() and bool(torch.isfinite(P).all())


def test_a_toy_sampler_learns_the_band_from_the_pinball_loss():
    gen = torch.Generator(device="cuda").manual_seed(3)
    n, K = 256, 64
    Y = 2.0 + 0.5 * torch.randn(n, 1, generator=gen, device="cuda", dtype=F64)
    mu = torch.zeros(1, device="cuda", dtype=F64, requires_grad=True)
    sigma = torch.ones(1, device="cuda", dtype=F64, requires_grad=True)
    opt = torch.optim.Adam([mu, sigma], lr=0.05)
    first = None
    for _ in range(100):
        eps = torch.randn(K, n, 1, generator=gen, device="cuda", dtype=F64)
        L = losses.pinball_loss(mu + sigma * eps, Y, quantiles=(0.05, 0.5, 0.95))
        first = float(L.detach()) if first is None else first
        opt.zero_grad()
        L.backward()
        opt.step()
    print("toy descent: pinball loss %.4f -> %.4f, mu 0 -> %.4f, sigma 1 -> %.4f" % (first, float(L.detach()), float(mu.detach()), float(sigma.detach())))
    assert float(L.detach()) < first and abs(float(mu.detach()) - 2.0) < 2.0


def test_zz_largest_deviation():
    print("largest deviation seen, in units of the bound %.3g of the terms' magnitudes: %s" % (RTOL, ", ".join("%s %.3g" % kv for kv in WORST.items())))
