"""probaforms_amd.metrics.losses.variogram_score_loss on the GPU (pfm_variogram_grad in libpf_metrics.so) against the float64
restatement (tests/variogram_grad_numpy.py), the variogram of sample_joint_scores' restatement, torch's gradcheck, and through the
flow's differentiable sampling.

Tolerance (derived, not measured): every output is a float64 sum of at most K + d <= 1088 terms, each off by a few 2^-53 of its
(v_ij + m_ij) |h|; that is at most about 1.3e-13 of the sum of those magnitudes, which the restatement returns beside every output
(smag, mx, my), so every output is held within RTOL = 1e-12 of its magnitude, the RTOL of the other loss tests.  Where the magnitude
is 0 the output must be exactly 0.  The largest ratios seen are printed by test_zz_largest_deviation.

Shapes (K, n, d): K in 1, 2, 3, 31, 32, 33, 63, 64, 65, 257, 1024 at (7, 3); d in 1, 2, 3, 4, 5, 15, 16, 17, 33, 63, 64 at K = 33;
n in 1, 2, R - 1, R, R + 1, 3 R + 1 at K = 3, d = 3; every K (at d = 3) and every d (at K = 3) at which pfm_variogram_plan changes
the lanes per row or the rows in flight, with the value one above; the limit shapes (1024, 3, 16) and (256, 3, 64); three shapes
whose n makes a workgroup take its rows in several passes, and (4, 49152, 14), whose workgroups take all 163 840 bytes of a CU's LDS,
against small calls on its rows.  tests/test_variogram_plans_host.py proves that the list reaches every
k_vario instantiation and every branch of the host's plan.
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
import joint_scores_numpy as js  # noqa: E402
import native_libs  # noqa: E402
import streams  # noqa: E402
import variogram_grad_numpy as vg  # noqa: E402
import variogram_plans as vp  # noqa: E402
from probaforms_amd.metrics import _lib, losses  # noqa: E402

pytestmark = pytest.mark.gpu

native_libs.ensure_built(_lib)

RTOL = vg.RTOL
ORDERS = (0.5, 1, 2)
OUTPUTS = (("scores", "smag"), ("grad_x", "mx"), ("grad_y", "my"))
WORST = {name: 0.0 for name, _ in OUTPUTS}
F64 = torch.float64

R3 = _lib.variogram_plan(1, 3, 3)[0]
# (K, n, d)
CASES = [(K, 7, 3) for K in sorted({1, 2, 3, 31, 32, 33, 63, 64, 65, 257, 1024} | set(vp.changes_in_k(3)))]
CASES += [(33, 7, d) for d in (1, 2, 3, 4, 5, 15, 16, 17, 33, 63, 64)]
CASES += [(3, 7, d) for d in sorted(set(vp.changes_in_d(3)) | {64})]
CASES += [(3, n, 3) for n in (1, 2, R3 - 1, R3, R3 + 1, 3 * R3 + 1)]
PASSES = [(33, 2051, 3), (129, 769, 3), (33, 2051, 17)]      # n so large that a workgroup takes its rows in several passes
LIMITS = [(1024, 3, 16), (256, 3, 64)]
CASES = sorted(set(CASES)) + PASSES + LIMITS
assert len(set(CASES)) == len(CASES)
WEIGHT_CASES = [(33, 7, 5), (33, 7, 17)]
PACKED, ALONE = (16, 65, 16), (300, 5, 17)                   # rows packed into a workgroup; a workgroup per row at a time
EDGE_SHAPES = [(1, 2), (2, 3), (3, 2), (33, 17), (65, 16), (257, 3)]          # (K, d)
NAN_CASES = [(3, R3 + 6, 3), (33, 7, 17), (257, 7, 3), (33, 7, 16), (300, 7, 2)]
POSITION_CASES = [(3, 3 * R3 + 1, 3), (33, 2051, 3), (257, 7, 3), (33, 7, 17), (300, 5, 16)]
WORKSPACE_CASES = [(3, R3 + 1, 3), (33, 5, 17), (257, 3, 16), (2, 1, 1), (5, 3, 64)]


def case_id(case):
    return "K%d_n%d_d%d" % case


def dev(A, grad=False, dtype=F64):
    return torch.from_numpy(np.array(A, order="C")).to(device="cuda", dtype=dtype).requires_grad_(grad)


@functools.lru_cache(maxsize=None)
def reference(case, order, weighted=False):
    """(X, Y, W, restatement dict) of a case: computed once, shared, never written to"""
    K, n, d = case
    X, Y = vg.rows(K, n, d)
    W = vg.weights(d) if weighted else None
    o = vg.value_grad(X, Y, order, W)
    for a in (X, Y) + tuple(o.values()) + (() if W is None else (W,)):
        a.setflags(write=False)
    return X, Y, W, o


def raw(X, Y, order, W=None, gx=True, gy=True):
    """pfm_variogram_grad once -> dict of numpy arrays (the outputs asked for)"""
    Xd, Yd = dev(X), dev(Y)
    K, n, d = Xd.shape
    out = {"scores": torch.empty(n, dtype=F64, device="cuda")}
    if gx:
        out["grad_x"] = torch.empty_like(Xd)
    if gy:
        out["grad_y"] = torch.empty_like(Yd)
    hygiene.poison_outputs(*out.values())
    ws = torch.empty(_lib.variogram_grad_workspace_bytes(n, K, d), dtype=torch.uint8, device="cuda")
    _lib.variogram_grad(Xd, Yd, None if W is None else dev(W), order, out["scores"], out.get("grad_x"), out.get("grad_y"), ws)
    return {k: v.cpu().numpy() for k, v in out.items()}


def assert_close(got, want, what):
    for name, mag in OUTPUTS:
        if name not in got:
            continue
        err, m = np.abs(got[name] - want[name]), np.abs(want[mag])
        rel = float((err / np.where(m > 0, m, 1.0)).max())
        WORST[name] = max(WORST[name], rel)
        print("%s: %s off by at most %.3g of its terms' magnitudes (bound %.3g)" % (what, name, rel, RTOL))
        assert np.isfinite(got[name]).all(), (what, name)
        assert (err <= RTOL * m).all(), (what, name, rel)


def same(a, b):
    return a.tobytes() == b.tobytes()


# ---- accuracy ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_scores_and_gradients_equal_the_restatement(case, order):
    K, n, d = case
    st, (R, S, lds, wgs, G, T) = _lib.variogram_plan_status(n, K, d)
    assert st == 0 and R >= 1 and lds <= 160 * 1024 and wgs == -(-n // R)
    if case in PASSES:
        assert R > G                                             # several passes over the rows in flight
    X, Y, _, want = reference(case, order)
    got = raw(X, Y, order)
    assert_close(got, want, "%s order=%s" % (case_id(case), order))
    if d == 1:
        assert not any(v.any() for v in got.values())            # no pair: exact zeros
    # the value alone is formed alike
    assert same(raw(X, Y, order, gx=False, gy=False)["scores"], got["scores"])
    # the public function: the same kernel call behind an autograd node
    A, B = dev(X, True), dev(Y, True)
    L = losses.variogram_score_loss(A, B, order=order, reduction="none")
    assert L.shape == (n,) and L.dtype == F64 and L.is_cuda and L.grad_fn is not None
    L.sum().backward()
    assert same(L.detach().cpu().numpy(), got["scores"])
    assert np.array_equal(A.grad.cpu().numpy(), got["grad_x"]) and np.array_equal(B.grad.cpu().numpy(), got["grad_y"])
    V = losses.variogram_score_loss(dev(X), dev(Y), order=order, reduction="none")
    assert V.grad_fn is None and same(V.cpu().numpy(), got["scores"])


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("case", WEIGHT_CASES, ids=case_id)
def test_weights_are_used_as_given(case, order):
    K, n, d = case
    X, Y, W, want = reference(case, order, True)
    assert (W[d // 2] == 0).all() and (W < 0).any() and not np.array_equal(W, W.T)
    got = raw(X, Y, order, W)
    assert_close(got, want, "%s order=%s weighted" % (case_id(case), order))
    A, B = dev(X, True), dev(Y, True)
    Wd = dev(W, True)                                            # a constant: no gradient flows to it
    L = losses.variogram_score_loss(A, B, order=order, weights=Wd, reduction="none")
    L.sum().backward()
    assert Wd.grad is None and same(L.detach().cpu().numpy(), got["scores"])
    assert np.array_equal(A.grad.cpu().numpy(), got["grad_x"]) and np.array_equal(B.grad.cpu().numpy(), got["grad_y"])
    assert same(losses.variogram_score_loss(X, Y, order=order, weights=W.tolist(), reduction="none").cpu().numpy(), got["scores"])
    # W = NULL is a W of ones
    plain, ones = raw(X, Y, order), raw(X, Y, order, np.ones((d, d)))
    assert all(same(plain[k], ones[k]) for k in plain)
    assert not same(plain["scores"], got["scores"])


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("shape", EDGE_SHAPES, ids=str)
def test_equal_coordinates_ties_last_bits_and_far_centres(shape, order):
    K, d = shape
    # all coordinates of a row equal: every |t|^p and every h is 0; p = 0.5 must not form 0 times infinity
    X = np.broadcast_to(np.array([1.5, -3.0, 0.0, 1e6, 1e-300])[None, :, None], (K, 5, d)).copy()
    Y = np.broadcast_to(np.array([-2.0, -3.0, 0.0, 7.0, 1e300])[:, None], (5, d)).copy()
    got = raw(X, Y, order)
    assert all(np.isfinite(v).all() and not v.any() for v in got.values()), got
    # a tied pair, y on a draw, last-bit differences, centre 1e6, a far y
    X, Y = vg.finite_rows(K, d)
    want = vg.value_grad(X, Y, order)
    got = raw(X, Y, order)
    assert all(np.isfinite(v).all() for v in got.values())
    assert_close(got, want, "finite rows K=%d d=%d order=%s" % (K, d, order))


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("K", (1, 33, 300))
def test_one_feature_gives_exact_zeros(K, order):
    X, Y = vg.rows(K, 300, 1)
    got = raw(X, Y, order)
    assert got["scores"].shape == (300,) and got["grad_x"].shape == (K, 300, 1) and not any(v.any() for v in got.values())
    L = losses.variogram_score_loss(dev(X, True), dev(Y, True), order=order)
    L.backward()
    assert float(L) == 0.0


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("shape", [(4, 70, 3), (64, 70, 16), (512, 9, 5), (16, 9, 33), (1024, 3, 2)], ids=str)
def test_lattice_rows_agree_exactly(shape, order):
    # rows in {0, 1}, K a power of two, unit weights: every |t|^p, h, r, r^2 and sum is exact, in the restatement's order and in any
    K, n, d = shape
    X, Y = vg.lattice_rows(K, n, d)
    want = vg.value_grad(X, Y, order)
    got = raw(X, Y, order)
    assert want["scores"].any() and want["grad_x"].any() and want["grad_y"].any()
    for name, _ in OUTPUTS:
        assert np.array_equal(got[name], want[name]), name


# ---- reproducibility and layout -------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", POSITION_CASES, ids=case_id)
def test_a_rows_outputs_do_not_depend_on_n_position_or_split(case):
    K, n, d = case
    X, Y, _, _ = reference(case, 0.5)
    full = raw(X, Y, 0.5)
    again = raw(X, Y, 0.5)
    assert all(same(full[k], again[k]) for k in full)             # two calls give identical bytes
    lo, hi = (2, 5) if n < 10 else (5, min(n, 70))
    cut = n // 2 + 1
    for a, b in ((lo, hi), (0, cut), (cut, n), (n - 1, n)):
        part = raw(X[:, a:b], Y[a:b], 0.5)
        assert same(part["scores"], full["scores"][a:b]), (a, b)
        assert same(part["grad_x"], np.ascontiguousarray(full["grad_x"][:, a:b])) and same(part["grad_y"], full["grad_y"][a:b])
    # the row at another position among other rows
    perm = np.random.RandomState(3).permutation(n)
    moved = raw(X[:, perm], Y[perm], 0.5)
    assert same(moved["scores"], full["scores"][perm]) and same(moved["grad_y"], full["grad_y"][perm])
    assert same(moved["grad_x"], np.ascontiguousarray(full["grad_x"][:, perm]))


def test_a_workgroup_that_takes_all_of_a_cus_lds_gives_the_rows_of_a_small_call():
    # K = 4, d = 14: 64 rows in flight need more than 64 KiB, so a workgroup of a long call takes three passes and all 163 840 bytes
    K, n, d = 4, 49152, 14
    R, S, lds, wgs, G, T = _lib.variogram_plan(n, K, d)
    assert lds == 160 * 1024 and R == 3 * G and _lib.variogram_plan(70, K, d)[0] == G
    X, Y = vg.rows(K, n, d)
    full = raw(X, Y, 0.5)
    for a, b in ((0, 70), (n // 2 - 35, n // 2 + 35), (n - 70, n)):
        part = raw(X[:, a:b], Y[a:b], 0.5)
        assert same(part["scores"], full["scores"][a:b]) and same(part["grad_y"], full["grad_y"][a:b]), (a, b)
        assert same(part["grad_x"], np.ascontiguousarray(full["grad_x"][:, a:b])), (a, b)
    assert_close(part, vg.value_grad(X[:, n - 70:], Y[n - 70:], 0.5), "the last 70 rows of %d" % n)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("case", NAN_CASES, ids=case_id)
def test_a_nan_stays_in_its_row(case, order):
    K, n, d = case
    X, Y = vg.rows(K, n, d)
    X, Y = X.copy(), Y.copy()
    X[K // 2, 1, d - 1] = np.nan
    Y[4, 0] = np.nan
    got = raw(X, Y, order)
    rows = np.zeros(n, bool)
    rows[[1, 4]] = True
    assert np.array_equal(np.isnan(got["scores"]), rows)
    gx, gy = np.isnan(got["grad_x"]), np.isnan(got["grad_y"])
    assert gx[:, rows].all() and not gx[:, ~rows].any() and gy[rows].all() and not gy[~rows].any()
    clean = vg.value_grad(np.delete(X, [1, 4], axis=1), np.delete(Y, [1, 4], axis=0), order)
    assert_close({k: np.delete(v, [1, 4], axis=1 if k == "grad_x" else 0) for k, v in got.items()}, clean, "beside NaN rows")


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("case", WORKSPACE_CASES, ids=case_id)
def test_outputs_do_not_depend_on_the_workspace_and_are_all_written(case, order):
    K, n, d = case
    X, Y = vg.rows(K, n, d)
    Xd, Yd = dev(X), dev(Y)
    nbytes = _lib.variogram_grad_workspace_bytes(n, K, d)
    outs = {}
    for pattern in ("zeros", "ones"):
        got = {}
        for tag, (gx, gy) in (("", (1, 1)), ("value_", (0, 0)), ("x_", (1, 0)), ("y_", (0, 1))):
            o = {"scores": torch.empty(n, dtype=F64, device="cuda")}
            if gx:
                o["grad_x"] = torch.empty_like(Xd)
            if gy:
                o["grad_y"] = torch.empty_like(Yd)
            hygiene.poison_outputs(*o.values())
            _lib.variogram_grad(Xd, Yd, None, order, o["scores"], o.get("grad_x"), o.get("grad_y"), hygiene.workspace(nbytes, pattern))
            torch.cuda.synchronize()
            got.update({tag + k: t for k, t in o.items()})
        for tag in ("value_", "x_", "y_"):                       # an output is the same bits whichever others are asked for
            for k in ("scores", "grad_x", "grad_y"):
                if tag + k in got:
                    assert hygiene.same_bits(got[tag + k], got[k]), (tag, k)
        hygiene.assert_all_written(got, "pfm_variogram_grad %s %s" % (case_id(case), pattern))
        outs[pattern] = got
    hygiene.assert_pattern_independent(outs, "pfm_variogram_grad %s" % case_id(case))


def _guarded_call(case):
    K, n, d = case
    gen = torch.Generator(device="cuda").manual_seed(67)
    X = torch.randn(K, n, d, dtype=F64, device="cuda", generator=gen)
    Y = torch.randn(n, d, dtype=F64, device="cuda", generator=gen)
    W = torch.rand(d, d, dtype=F64, device="cuda", generator=gen)
    what = "pfm_variogram_grad[%d draws, %d rows, d %d%%s]" % (K, n, d)
    full = (what % "", lambda ws, o: _lib.variogram_grad_status(X, Y, W, 0.5, o["scores"], o["grad_x"], o["grad_y"], ws),
            dict(scores=bounds.Out(F64, (n,)), grad_x=bounds.Out(F64, (K, n, d)), grad_y=bounds.Out(F64, (n, d))), dict(X=X, Y=Y, W=W))
    value = (what % ", values alone", lambda ws, o: _lib.variogram_grad_status(X, Y, None, 2, o["scores"], None, None, ws),
             dict(scores=bounds.Out(F64, (n,))), dict(X=X, Y=Y))
    return _lib.variogram_grad_workspace_bytes(n, K, d), (full, value)


@pytest.mark.parametrize("case", [PACKED, ALONE], ids=case_id)
def test_no_write_outside_the_workspace_and_the_outputs(case):
    need, forms = _guarded_call(case)
    for what, call, outs, inputs in forms:
        bounds.run(what, need, call, outs, inputs, keeps_nothing=True)


@pytest.mark.parametrize("case", [PACKED, ALONE], ids=case_id)
def test_everything_is_enqueued_on_the_callers_stream(case):
    need, forms = _guarded_call(case)
    for what, call, outs, inputs in forms:
        res = streams.run(what, need, call, outs, inputs)
        assert res["pending"] and res["captured"]


# ---- consistency with the metric ------------------------------------------------------------------------------------

@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("shape", [(2, 3), (33, 17), (257, 3)], ids=str)
def test_value_agrees_with_the_restatement_of_the_metric(shape, order):
    K, d = shape
    X, Y = vg.finite_rows(K, d)
    assert X.dtype == np.float32
    ref = js.scores_of_stacked(X, Y, False, float(order))
    got = losses.variogram_score_loss(X, Y, order=order, reduction="none").cpu().numpy()
    tol = js.bound_variogram(ref.variogram, ref, K, d) - js._ulp32(ref.variogram) + RTOL * ref.v
    assert got.shape == (5,) and (np.abs(got - ref.variogram) <= tol).all(), (got, ref.variogram)


def test_the_loss_sees_the_dependence_that_crps_does_not():
    xt, sh, y = js.comonotone(64)                                # [1, 2, K]: the same marginals, the second column's draws permuted
    A, B = np.ascontiguousarray(np.transpose(xt, (2, 0, 1))), np.ascontiguousarray(np.transpose(sh, (2, 0, 1)))
    # the CRPS takes every feature's draws as a set: equal up to the order of its sums, (K^2 / 2 + 9) 2^-53 of T1 + spread < 8
    ca, cb = losses.crps_loss(A, y, reduction="none"), losses.crps_loss(B, y, reduction="none")
    assert float((ca - cb).abs().max()) <= (64 * 64 / 2.0 + 9.0) * 2.0 ** -53 * 8.0 and float(ca.max()) < 4.0
    for order in ORDERS:
        va, vb = float(losses.variogram_score_loss(A, y, order=order)), float(losses.variogram_score_loss(B, y, order=order))
        print("order %s: variogram score %.6g comonotone, %.6g with the dependence broken" % (order, va, vb))
        assert va == 0.0 and vb > 1e-3                           # x = (t, t) and y on the diagonal: every difference is 0


# ---- autograd -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("weighted", (False, True))
@pytest.mark.parametrize("reduction", ("mean", "none"))
@pytest.mark.parametrize("order", ORDERS)
def test_gradcheck_on_the_public_function(order, reduction, weighted):
    X, Y = vg.rows(3, 4, 3)                                      # tie-free: coordinates apart by far more than gradcheck's step
    W = dev(vg.weights(3)) if weighted else None
    fn = lambda a, b: losses.variogram_score_loss(a, b, order=order, weights=W, reduction=reduction)
    assert torch.autograd.gradcheck(fn, (dev(X, True), dev(Y, True)))


def test_gradient_goes_to_the_inputs_that_ask(monkeypatch):
    X, Y, _, want = reference((33, 7, 3), 0.5)
    both = [dev(X, True), dev(Y, True)]
    losses.variogram_score_loss(both[0], both[1]).backward()
    assert (np.abs(both[0].grad.cpu().numpy() * 7 - want["grad_x"]) <= RTOL * want["mx"]).all()      # the mean's 1 / n
    seen = []
    status = _lib.variogram_grad_status

    def spy(X_, Y_, W_, order, scores, gx, gy, ws):
        seen.append((gx is not None, gy is not None))
        return status(X_, Y_, W_, order, scores, gx, gy, ws)
    monkeypatch.setattr(_lib, "variogram_grad_status", spy)
    A, B = dev(X), dev(Y, True)
    losses.variogram_score_loss(A, B).backward()
    assert A.grad is None and hygiene.same_bits(B.grad, both[1].grad)
    A, B = dev(X, True), dev(Y)
    (4 * losses.variogram_score_loss(A, B)).backward()           # (a power of two: the scaling commutes with the mean's 1 / n)
    assert B.grad is None and torch.equal(A.grad, 4 * both[0].grad)
    for a, b in ((dev(X), dev(Y)), (X, Y), (X.tolist(), dev(Y))):
        V = losses.variogram_score_loss(a, b)
        assert V.grad_fn is None and not V.requires_grad and V.is_cuda and V.dtype == F64 and V.shape == ()
        assert abs(float(V) - want["scores"].mean()) <= RTOL * want["smag"].mean()
    assert seen == [(False, True), (True, False)] + [(False, False)] * 3


def test_float32_inputs_get_float32_gradients():
    X, Y, _, _ = reference((33, 7, 3), 0.5)
    A, B = dev(X, True, torch.float32), dev(Y, True, torch.float32)
    L = losses.variogram_score_loss(A, B)
    assert L.dtype == F64
    L.backward()
    assert A.grad.dtype == torch.float32 == B.grad.dtype and A.grad.shape == A.shape and B.grad.shape == B.shape
    A64, B64 = A.detach().double().requires_grad_(True), B.detach().double().requires_grad_(True)
    L64 = losses.variogram_score_loss(A64, B64)
    L64.backward()
    assert hygiene.same_bits(L.reshape(1), L64.reshape(1))
    assert torch.equal(A.grad, A64.grad.float()) and torch.equal(B.grad, B64.grad.float())


def test_a_permuted_view_gives_the_result_of_its_contiguous_copy():
    X, Y, _, _ = reference((33, 7, 3), 0.5)
    A, B = dev(X, True), dev(Y)
    L = losses.variogram_score_loss(A, B)
    L.backward()
    T = A.detach().permute(1, 0, 2).contiguous().requires_grad_(True)          # [n, K, d]: the draws are its permuted view
    LT = losses.variogram_score_loss(T.permute(1, 0, 2), B)
    LT.backward()
    assert hygiene.same_bits(L.reshape(1), LT.reshape(1)) and hygiene.same_bits(T.grad.permute(1, 0, 2), A.grad)


def test_a_weighted_sum_of_the_rows_backpropagates_the_weights():
    X, Y, _, want = reference((33, 7, 3), 0.5)
    w = np.arange(1.0, 8.0)
    A, B = dev(X, True), dev(Y, True)
    S = losses.variogram_score_loss(A, B, reduction="none")
    (S * dev(w)).sum().backward()
    got = raw(X, Y, 0.5)
    assert np.array_equal(A.grad.cpu().numpy(), got["grad_x"] * w[None, :, None])
    assert np.array_equal(B.grad.cpu().numpy(), got["grad_y"] * w[:, None])
    assert (np.abs(got["grad_x"] - want["grad_x"]) <= RTOL * want["mx"]).all()


def test_forward_and_backward_never_wait_for_the_device():
    X, Y, _, want = reference((33, 7, 3), 0.5)
    A, B, W = dev(X, True), dev(Y, True), dev(np.ones((3, 3)))
    losses.variogram_score_loss(A, B).backward()                 # warm-up: library, code objects, allocator
    losses.variogram_score_loss(A, B, order=2, weights=W, reduction="none").sum().backward()
    losses.variogram_score_loss(A.detach(), B.detach())
    A.grad = B.grad = None
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        L = losses.variogram_score_loss(A, B)
        (2 * L).backward()
        C = losses.variogram_score_loss(A, B, order=2, weights=W, reduction="none")
        C.sum().backward()
        V = losses.variogram_score_loss(A.detach(), B.detach(), reduction="none")
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert bool(torch.isfinite(A.grad).all()) and bool(A.grad.ne(0).any()) and bool(torch.isfinite(B.grad).all())
    assert (np.abs(V.cpu().numpy() - want["scores"]) <= RTOL * want["smag"]).all() and bool(torch.isfinite(C).all())
    assert abs(float(L.detach()) - want["scores"].mean()) <= RTOL * want["smag"].mean()


# ---- end to end -------------------------------------------------------------------------------------------------------

def test_energy_plus_variogram_reaches_a_flows_parameters_through_its_sampler():
    from probaforms_amd.models import RealNVP
    rng = np.random.RandomState(5)
    n = 300
    C0 = rng.uniform(-1, 1, size=(n, 1)).astype(np.float32)
    X0 = (np.concatenate([np.sin(3 * C0), np.cos(3 * C0)], axis=1) + 0.1 * rng.normal(size=(n, 2))).astype(np.float32)
    torch.manual_seed(7)
    model = RealNVP(n_layers=3, hidden=(8,), n_epochs=1, batch_size=100)
    model.fit(X0, C0)
    for q in model.nf.parameters():
        q.grad = None
    C = torch.from_numpy(C0).cuda()
    Y = torch.from_numpy(X0).cuda()
    X = model.nf.sample(C.repeat(4, 1)).view(4, n, 2)
    L = losses.energy_score_loss(X, Y) + 0.5 * losses.variogram_score_loss(X, Y)
    assert L.grad_fn is not None and bool(torch.isfinite(L))
    L.backward()
    grads = [q.grad for q in model.nf.parameters()]
    assert all(g is not None and bool(torch.isfinite(g).all()) for g in grads)
    assert any(bool(g.ne(0).any()) for g in grads)
    for q in model.nf.parameters():
        q.grad = None
    losses.variogram_score_loss(model.nf.sample(C.repeat(4, 1)).view(4, n, 2), Y).backward()          # and the new term alone
    assert any(bool(q.grad.ne(0).any()) for q in model.nf.parameters())


# ---- memory ---------------------------------------------------------------------------------------------------------

def test_forward_and_backward_keep_nothing_of_the_size_of_the_feature_pairs():
    # by design: the kept gradient and the returned one (and a contiguous copy, had the input needed one), never [K, n, d, d]
    n, K, d = 512, 256, 16
    gen = torch.Generator(device="cuda").manual_seed(1)
    X = torch.randn(K, n, d, generator=gen, device="cuda", dtype=F64).requires_grad_(True)
    Y = torch.randn(n, d, generator=gen, device="cuda", dtype=F64)
    losses.variogram_score_loss(X[:, :4].detach(), Y[:4])        # warm-up
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    losses.variogram_score_loss(X, Y).backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    bytes_x = X.numel() * 8
    print("allocator peak of forward + backward: %.2f times the bytes of X_draws" % (peak / bytes_x))
    assert peak <= 4 * bytes_x + (1 << 20)
    assert 8 * K * n * d * d == 16 * bytes_x                     # what the torch route's [K, n, d, d] temporary alone would take
    assert bool(torch.isfinite(X.grad).all())


def test_zz_largest_deviation():
    print("largest deviation seen, in units of the terms' magnitudes (bound %.3g): %s"
          % (RTOL, ", ".join("%s %.3g" % kv for kv in WORST.items())))
