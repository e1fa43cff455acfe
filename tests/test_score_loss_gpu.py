"""probaforms_amd.metrics.losses.energy_score_loss / crps_loss on the GPU (pfm_score_grad in libpf_metrics.so) against the float64
restatement (tests/scoregrad_numpy.py), the existing restatements of sample_scores and sample_joint_scores, torch's gradcheck, and
through the flow's differentiable sampling.

Tolerance: every output within RTOL = 1e-12 (the RTOL of tests/test_sliced_loss_gpu.py) of the sum of the magnitudes of its own
terms, from the restatement: a float64 sum of at most 1024 + 64 correctly rounded terms, in any order, stays within
1088 2^-53 = 1.2e-13 of that sum, and a term (a square root, a reciprocal, a product) carries a few 2^-53 of its own: two orders
below the bound.  Where the magnitudes are 0 (every term coincident) the output must be exactly 0.  The largest ratios seen are
printed by test_zz_largest_deviation.
"A term carries a few 2^-53" does not hold where a distance sums thousands of squares, so for d > 128 the bound per output is
(1e-12 + d 2^-53) of the magnitudes: a sum of d non-negative squares taken in any order (the kernel's is an fma chain, the
restatement's numpy's pairwise sum) is within d 2^-53 of itself relatively; the square root halves that and the reciprocal keeps
it, and every term of every output is a distance or a difference over a distance.  rtol_of states it.  Seen on an MI355X for the
crossed-axes cases (scoregrad_numpy.CROSSED and its NaN and layout shapes): at most 0.0031 of their bound for grad_x, 0.0019 for
grad_y, 0.0014 for the spread and 0.0009 for the scores, that is 4e-15 of the magnitudes at the most.

Shapes: K in 1, 2, 3, 31, 32, 33, 63, 64, 65, 257 and every K at which pfm_score_plan changes the lanes per row or the draws per
lane, with K + 1, at d = 2; d in 1, 2, 16, 17, 33 (one chunk of 16 features, its edge, three chunks) at K = 33; n in 1, 2, R - 1, R,
R + 1, 3 R + 1 at K = 3, d = 2, and two shapes whose n is large enough for several passes per workgroup; the limit shapes
K = 1024, d = 16 and K = 256, d = 64.  scoregrad_numpy.CROSSED crosses the axes: every k_score instantiation (draws per lane 1, 2, 4 by
1, 4, 16 features in registers or chunks) and every branch of the host's plan (the target left in global memory, even pitches,
rows in flight halved for the LDS, idle lanes, several chunked passes), as tests/test_loss_plans_host.py proves.
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import hygiene  # noqa: E402
import joint_scores_numpy as js  # noqa: E402
import native_libs  # noqa: E402
import scoregrad_numpy as sg  # noqa: E402
import scores_numpy as sn  # noqa: E402
from probaforms_amd.metrics import _lib, losses  # noqa: E402

pytestmark = pytest.mark.gpu

native_libs.ensure_built(_lib)

RTOL = 1e-12
U53 = 2.0 ** -53
OUTPUTS = (("scores", "smag"), ("spread", "spread"), ("grad_x", "mx"), ("grad_y", "my"))
WORST = {name: 0.0 for name, _ in OUTPUTS}


def packing(K):
    """(lanes that share a row, draws per lane) of pfm_score_plan"""
    S = _lib.score_plan(1, K, 1)[1]
    return S, -(-K // S)


BASE_K = (1, 2, 3, 31, 32, 33, 63, 64, 65, 257)
CHANGES = [K for K in range(2, _lib.SCORE_MAX_K + 1) if packing(K) != packing(K - 1)]
KS = sorted(set(BASE_K) | set(CHANGES) | {K + 1 for K in CHANGES})
R3 = _lib.score_plan(1, 3, 2)[0]
# (K, n, d)
CASES = [(K, 7, 2) for K in KS] + [(33, 7, d) for d in (1, 2, 16, 17, 33)]
CASES += [(3, n, 2) for n in (1, 2, R3 - 1, R3, R3 + 1, 3 * R3 + 1)]
PASSES = [(33, 2051, 2), (129, 769, 2), (33, 2051, 17)]     # n so large that a workgroup takes its rows in several passes
LIMITS = [(1024, 3, 16), (256, 3, 64)]
CASES = sorted(set(CASES)) + PASSES[:2] + LIMITS + sg.CROSSED
assert PASSES[2] in sg.CROSSED and len(set(CASES)) == len(CASES)
NAN_CASES = [(3, R3 + 6, 2), (33, 7, 17), (257, 7, 2)] + sg.CROSSED_NAN
POSITION_CASES = [(3, 3 * R3 + 1, 2), (33, 2051, 2), (257, 7, 2), (33, 7, 17)] + sg.CROSSED_LAYOUT
WORKSPACE_CASES = [(3, R3 + 1, 2), (33, 5, 17), (257, 3, 2), (2, 1, 1)] + sg.CROSSED_LAYOUT
NEW = set(sg.CROSSED + sg.CROSSED_NAN + sg.CROSSED_LAYOUT)
WORST_NEW = {name: 0.0 for name, _ in OUTPUTS}              # of the bound, over the cases of NEW


def case_id(case):
    return "K%d_n%d_d%d" % case


rtol_of = sg.rtol_of             # RTOL, and d 2^-53 more where a distance sums more than 128 squares (derived beside it)
assert rtol_of(128) == RTOL and rtol_of(4096) == RTOL + 4096 * U53


def dev(A, grad=False, dtype=torch.float64):
    return torch.from_numpy(np.array(A)).to(device="cuda", dtype=dtype).requires_grad_(grad)


@functools.lru_cache(maxsize=None)
def reference(case, fair):
    """(X, Y, restatement dict) of a case: computed once, shared, never written to"""
    K, n, d = case
    X, Y = sg.rows(K, n, d)
    o = sg.value_grad(X, Y, fair)
    for a in (X, Y) + tuple(o.values()):
        a.setflags(write=False)
    return X, Y, o


def raw(X, Y, fair, spread=True, gx=True, gy=True):
    """pfm_score_grad once -> dict of numpy arrays (the outputs asked for)"""
    Xd, Yd = dev(X), dev(Y)
    K, n, d = Xd.shape
    out = {"scores": torch.empty(n, dtype=torch.float64, device="cuda")}
    if spread:
        out["spread"] = torch.empty(n, dtype=torch.float64, device="cuda")
    if gx:
        out["grad_x"] = torch.empty_like(Xd)
    if gy:
        out["grad_y"] = torch.empty_like(Yd)
    hygiene.poison_outputs(*out.values())
    ws = torch.empty(_lib.score_grad_workspace_bytes(n, K, d), dtype=torch.uint8, device="cuda")
    _lib.score_grad(Xd, Yd, fair, out["scores"], out.get("spread"), out.get("grad_x"), out.get("grad_y"), ws)
    return {k: v.cpu().numpy() for k, v in out.items()}


def assert_close(got, want, what, case=None):
    rtol = RTOL if case is None else rtol_of(case[2])
    for name, mag in OUTPUTS:
        if name not in got:
            continue
        err, m = np.abs(got[name] - want[name]), np.abs(want[mag])
        rel = float((err / np.where(m > 0, m, 1.0)).max())
        WORST[name] = max(WORST[name], rel)
        if case in NEW:
            WORST_NEW[name] = max(WORST_NEW[name], rel / rtol)
        print("%s: %s off by at most %.3g of its terms' magnitudes (bound %.3g)" % (what, name, rel, rtol))
        assert np.isfinite(got[name]).all(), (what, name)
        assert (err <= rtol * m).all(), (what, name, rel)


# ---- accuracy ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fair", (False, True))
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_scores_spread_and_gradients_equal_the_restatement(case, fair):
    K, n, d = case
    if K == 1 and fair:
        with pytest.raises(ValueError, match="at least 2 draws"):
            losses.energy_score_loss(dev(np.zeros((1, n, d))), dev(np.zeros((n, d))), fair=True)
        return
    st, (R, S, lds, wgs) = _lib.score_plan_status(n, K, d)
    assert st == 0 and R >= 1 and lds <= 160 * 1024 and wgs == -(-n // R)
    if case in PASSES:
        assert R > _lib.score_plan(1, K, d)[0]                   # several passes over the rows in flight
    X, Y, want = reference(case, fair)
    got = raw(X, Y, fair)
    assert_close(got, want, "%s fair=%s" % (case_id(case), fair), case)
    # the value alone is formed alike
    assert raw(X, Y, fair, gx=False, gy=False)["scores"].tobytes() == got["scores"].tobytes()
    # the public function: the same kernel call behind an autograd node
    A, B = dev(X, True), dev(Y, True)
    L = losses.energy_score_loss(A, B, fair=fair, reduction="none")
    assert L.shape == (n,) and L.dtype == torch.float64 and L.is_cuda and L.grad_fn is not None
    L.sum().backward()
    assert L.detach().cpu().numpy().tobytes() == got["scores"].tobytes()
    assert np.array_equal(A.grad.cpu().numpy(), got["grad_x"]) and np.array_equal(B.grad.cpu().numpy(), got["grad_y"])


@pytest.mark.parametrize("fair", (False, True))
@pytest.mark.parametrize("shape", [(2, 1), (3, 2), (33, 17), (65, 2), (257, 3)], ids=str)
def test_tied_draws_targets_on_draws_last_bits_and_far_centres(shape, fair):
    K, d = shape
    X, Y = sg.finite_rows(K, d)
    want = sg.value_grad(X, Y, fair)
    got = raw(X, Y, fair)
    assert all(np.isfinite(v).all() for v in got.values())
    assert_close(got, want, "finite rows K=%d d=%d fair=%s" % (K, d, fair))
    if K == 2:                                                   # row 0: the two draws are tied, their pair adds exactly 0
        assert got["spread"][0] == 0.0 and np.array_equal(got["grad_x"][0, 0], got["grad_x"][1, 0])
    # every draw on the target: all terms are coincident, every output exactly 0
    Z = np.broadcast_to(Y[None], X.shape).copy()
    zero = raw(Z, Y, fair)
    assert all(not v.any() for v in zero.values())


@pytest.mark.parametrize("shape", [(4, 70, 1), (64, 70, 1), (512, 9, 1)], ids=str)
def test_integer_valued_rows_agree_bit_for_bit(shape):
    # d = 1, values in {0, 1}, K a power of two, fair=False: every distance is 0 or 1, every c (x - y) is 0 or +-1, every sum an
    # integer below 2^53 and every scale a power of two: the restatement's sums and any other order's are exact
    K, n, d = shape
    X, Y = sg.lattice_rows(K, n, d)
    want = sg.value_grad(X, Y, False)
    got = raw(X, Y, False)
    for name, _ in OUTPUTS:
        assert np.array_equal(got[name], want[name]), name
    # d = 2 on the same lattice: distances are 0, 1 or sqrt(2); held to the tolerance
    X, Y = sg.lattice_rows(K, n, 2)
    assert_close(raw(X, Y, True), sg.value_grad(X, Y, True), "lattice %s d=2" % (shape,))


# ---- reproducibility and layout -------------------------------------------------------------------------------------

def same(a, b):
    return a.tobytes() == b.tobytes()


@pytest.mark.parametrize("case", POSITION_CASES, ids=case_id)
def test_a_rows_outputs_do_not_depend_on_n_position_or_split(case):
    K, n, d = case
    X, Y, _ = reference(case, True)
    full = raw(X, Y, True)
    again = raw(X, Y, True)
    assert all(same(full[k], again[k]) for k in full)             # two calls give identical bytes
    lo, hi = (2, 5) if n < 10 else (5, min(n, 70))
    cut = n // 2 + 1
    for a, b in ((lo, hi), (0, cut), (cut, n), (n - 1, n)):
        part = raw(X[:, a:b], Y[a:b], True)
        assert same(part["scores"], full["scores"][a:b]) and same(part["spread"], full["spread"][a:b]), (a, b)
        assert same(part["grad_x"], np.ascontiguousarray(full["grad_x"][:, a:b])) and same(part["grad_y"], full["grad_y"][a:b])


@pytest.mark.parametrize("fair", (False, True))
@pytest.mark.parametrize("case", WORKSPACE_CASES, ids=case_id)
def test_outputs_do_not_depend_on_the_workspace_and_are_all_written(case, fair):
    K, n, d = case
    X, Y = sg.rows(K, n, d)
    Xd, Yd = dev(X), dev(Y)
    nbytes = _lib.score_grad_workspace_bytes(n, K, d)
    outs = {}
    for pattern in ("zeros", "ones"):
        got = {}
        for tag, (sp, gx, gy) in (("", (1, 1, 1)), ("value_", (0, 0, 0)), ("x_", (0, 1, 0)), ("y_", (1, 0, 1))):
            o = {"scores": torch.empty(n, dtype=torch.float64, device="cuda")}
            if sp:
                o["spread"] = torch.empty(n, dtype=torch.float64, device="cuda")
            if gx:
                o["grad_x"] = torch.empty_like(Xd)
            if gy:
                o["grad_y"] = torch.empty_like(Yd)
            hygiene.poison_outputs(*o.values())
            _lib.score_grad(Xd, Yd, fair, o["scores"], o.get("spread"), o.get("grad_x"), o.get("grad_y"),
                            hygiene.workspace(nbytes, pattern))
            torch.cuda.synchronize()
            got.update({tag + k: t for k, t in o.items()})
        for tag in ("value_", "x_", "y_"):                       # an output is the same bits whichever others are asked for
            for k in ("scores", "spread", "grad_x", "grad_y"):
                if tag + k in got:
                    assert hygiene.same_bits(got[tag + k], got[k]), (tag, k)
        hygiene.assert_all_written(got, "pfm_score_grad %s %s" % (case_id(case), pattern))
        outs[pattern] = got
    hygiene.assert_pattern_independent(outs, "pfm_score_grad %s" % case_id(case))


# ---- consistency with the existing scores -------------------------------------------------------------------------

@pytest.mark.parametrize("fair", (False, True))
def test_crps_loss_is_the_energy_score_of_every_series(fair):
    X, Y = sg.rows(9, 6, 5)
    C = losses.crps_loss(dev(X), dev(Y), fair=fair, reduction="none")
    E = losses.energy_score_loss(dev(X.reshape(9, 30, 1)), dev(Y.reshape(30, 1)), fair=fair, reduction="none")
    assert C.shape == (6, 5) and C.grad_fn is None and hygiene.same_bits(C.reshape(30), E)
    assert hygiene.same_bits(losses.crps_loss(dev(X), dev(Y), fair=fair).reshape(1), E.mean().reshape(1))
    A, B = dev(X, True), dev(Y, True)
    losses.crps_loss(A, B, fair=fair).backward()
    A1, B1 = dev(X.reshape(9, 30, 1), True), dev(Y.reshape(30, 1), True)
    losses.energy_score_loss(A1, B1, fair=fair).backward()
    assert hygiene.same_bits(A.grad.reshape(9, 30, 1), A1.grad) and hygiene.same_bits(B.grad.reshape(30, 1), B1.grad)


@pytest.mark.parametrize("fair", (False, True))
@pytest.mark.parametrize("K", (2, 33, 257))
def test_values_agree_with_the_restatements_of_the_metrics(K, fair):
    # d = 1: the crps of sample_scores
    X, Y = sg.finite_rows(K, 1)
    ref = sn.scores_of_stacked(X, Y, (), fair).crps
    own = sg.value_grad(X, Y, fair)
    got = losses.crps_loss(X, Y, fair=fair, reduction="none").cpu().numpy()
    tol = RTOL * own["smag"][:, None] + (K * K / 2.0 + 9.0) * U53 * own["smag"][:, None]
    assert got.shape == (5, 1) and (np.abs(got - ref) <= tol).all(), (got, ref)
    # float32 draws at d = 17: the energy of sample_joint_scores
    X, Y = sg.finite_rows(K, 17)
    ref = js.scores_of_stacked(X, Y, fair, None)
    got = losses.energy_score_loss(X, Y, fair=fair, reduction="none").cpu().numpy()
    tol = js.bound_pairs(ref.energy, ref, K, 17) - js._ulp32(ref.energy) + RTOL * (ref.t1 + np.abs(ref.spread))
    assert (np.abs(got - ref.energy) <= tol).all(), (got, ref.energy)


# ---- autograd -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fair", (False, True))
@pytest.mark.parametrize("reduction", ("mean", "none"))
def test_gradcheck_on_the_public_functions(fair, reduction):
    X, Y = sg.rows(3, 4, 2)
    for fn in (losses.energy_score_loss, losses.crps_loss):
        assert torch.autograd.gradcheck(lambda a, b: fn(a, b, fair=fair, reduction=reduction), (dev(X, True), dev(Y, True)))


def test_gradient_goes_to_the_inputs_that_ask(monkeypatch):
    X, Y, want = reference((33, 7, 2), True)
    both = [dev(X, True), dev(Y, True)]
    losses.energy_score_loss(both[0], both[1]).backward()
    assert (np.abs(both[0].grad.cpu().numpy() * 7 - want["grad_x"]) <= RTOL * want["mx"]).all()      # the mean's 1 / n
    seen = []
    status = _lib.score_grad_status

    def spy(X_, Y_, fair, scores, spread, gx, gy, ws):
        seen.append((gx is not None, gy is not None))
        return status(X_, Y_, fair, scores, spread, gx, gy, ws)
    monkeypatch.setattr(_lib, "score_grad_status", spy)
    A, B = dev(X), dev(Y, True)
    losses.energy_score_loss(A, B).backward()
    assert A.grad is None and hygiene.same_bits(B.grad, both[1].grad)
    A, B = dev(X, True), dev(Y)
    (4 * losses.energy_score_loss(A, B)).backward()              # (a power of two: the scaling commutes with the mean's 1 / n)
    assert B.grad is None and torch.equal(A.grad, 4 * both[0].grad)
    for a, b in ((dev(X), dev(Y)), (X, Y), (X.tolist(), dev(Y))):
        V = losses.energy_score_loss(a, b)
        assert V.grad_fn is None and not V.requires_grad and V.is_cuda and V.dtype == torch.float64 and V.shape == ()
        assert abs(float(V) - want["scores"].mean()) <= RTOL * want["smag"].mean()
    assert seen == [(False, True), (True, False)] + [(False, False)] * 3


def test_float32_inputs_get_float32_gradients():
    X, Y, _ = reference((33, 7, 2), True)
    A, B = dev(X, True, torch.float32), dev(Y, True, torch.float32)
    L = losses.energy_score_loss(A, B)
    assert L.dtype == torch.float64
    L.backward()
    assert A.grad.dtype == torch.float32 == B.grad.dtype and A.grad.shape == A.shape and B.grad.shape == B.shape
    A64, B64 = A.detach().double().requires_grad_(True), B.detach().double().requires_grad_(True)
    L64 = losses.energy_score_loss(A64, B64)
    L64.backward()
    assert hygiene.same_bits(L.reshape(1), L64.reshape(1))
    assert torch.equal(A.grad, A64.grad.float()) and torch.equal(B.grad, B64.grad.float())


def test_a_permuted_view_gives_the_result_of_its_contiguous_copy():
    X, Y, _ = reference((33, 7, 2), True)
    A, B = dev(X, True), dev(Y)
    L = losses.energy_score_loss(A, B)
    L.backward()
    T = A.detach().permute(1, 0, 2).contiguous().requires_grad_(True)          # [n, K, d]: the draws are its permuted view
    LT = losses.energy_score_loss(T.permute(1, 0, 2), B)
    LT.backward()
    assert hygiene.same_bits(L.reshape(1), LT.reshape(1)) and hygiene.same_bits(T.grad.permute(1, 0, 2), A.grad)


def test_a_weighted_sum_of_the_rows_backpropagates_the_weights():
    X, Y, want = reference((33, 7, 2), True)
    w = np.arange(1.0, 8.0)
    A, B = dev(X, True), dev(Y, True)
    S = losses.energy_score_loss(A, B, reduction="none")
    (S * dev(w)).sum().backward()
    got = raw(X, Y, True)
    assert np.array_equal(A.grad.cpu().numpy(), got["grad_x"] * w[None, :, None])
    assert np.array_equal(B.grad.cpu().numpy(), got["grad_y"] * w[:, None])
    assert (np.abs(got["grad_x"] - want["grad_x"]) <= RTOL * want["mx"]).all()


# ---- device behaviour -----------------------------------------------------------------------------------------------

def test_forward_and_backward_never_wait_for_the_device():
    X, Y, want = reference((33, 7, 2), True)
    A, B = dev(X, True), dev(Y, True)
    losses.energy_score_loss(A, B).backward()                    # warm-up: library, code objects, allocator
    losses.crps_loss(A, B, reduction="none").sum().backward()
    losses.energy_score_loss(A.detach(), B.detach())
    A.grad = B.grad = None
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        L = losses.energy_score_loss(A, B)
        (2 * L).backward()
        C = losses.crps_loss(A, B, fair=False, reduction="none")
        C.sum().backward()
        V = losses.energy_score_loss(A.detach(), B.detach(), reduction="none")
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert bool(torch.isfinite(A.grad).all()) and bool(A.grad.ne(0).any()) and bool(torch.isfinite(B.grad).all())
    assert (np.abs(V.cpu().numpy() - want["scores"]) <= RTOL * want["smag"]).all() and bool(torch.isfinite(C).all())
    assert abs(float(L.detach()) - want["scores"].mean()) <= RTOL * want["smag"].mean()


@pytest.mark.parametrize("case", NAN_CASES, ids=case_id)
def test_a_nan_stays_in_its_row(case):
    K, n, d = case
    X, Y = sg.rows(K, n, d)
    X, Y = X.copy(), Y.copy()
    X[K // 2, 1, d - 1] = np.nan
    Y[4, 0] = np.nan
    got = raw(X, Y, True)
    rows = np.zeros(n, bool)
    rows[[1, 4]] = True
    assert np.array_equal(np.isnan(got["scores"]), rows)
    assert np.isnan(got["spread"][1]) and np.isfinite(np.delete(got["spread"], 1)).all()          # the spread does not meet y
    gx, gy = np.isnan(got["grad_x"]), np.isnan(got["grad_y"])
    assert gx[:, rows].all() and not gx[:, ~rows].any() and gy[rows].all() and not gy[~rows].any()
    clean = sg.value_grad(np.delete(X, [1, 4], axis=1), np.delete(Y, [1, 4], axis=0), True)
    assert_close({k: np.delete(v, [1, 4], axis=1 if k == "grad_x" else 0) for k, v in got.items()}, clean, "beside NaN rows",
                 case)


# ---- end to end -------------------------------------------------------------------------------------------------------

def test_energy_score_loss_reaches_a_flows_parameters_through_its_sampler():
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
    L = losses.energy_score_loss(X, Y)
    assert L.grad_fn is not None and bool(torch.isfinite(L))
    L.backward()
    grads = [q.grad for q in model.nf.parameters()]
    assert all(g is not None and bool(torch.isfinite(g).all()) for g in grads)
    assert any(bool(g.ne(0).any()) for g in grads)


def test_a_toy_sampler_descends_towards_the_targets():
    gen = torch.Generator(device="cuda").manual_seed(3)
    n, K = 256, 8
    Y = 2.0 + 0.5 * torch.randn(n, 1, generator=gen, device="cuda", dtype=torch.float64)
    mu = torch.zeros(1, device="cuda", dtype=torch.float64, requires_grad=True)
    sigma = torch.ones(1, device="cuda", dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([mu, sigma], lr=0.05)
    first = None
    for _ in range(100):
        eps = torch.randn(K, n, 1, generator=gen, device="cuda", dtype=torch.float64)
        L = losses.energy_score_loss(mu + sigma * eps, Y)
        first = float(L.detach()) if first is None else first
        opt.zero_grad()
        L.backward()
        opt.step()
    eps = torch.randn(K, n, 1, generator=gen, device="cuda", dtype=torch.float64)
    last = float(losses.energy_score_loss((mu + sigma * eps).detach(), Y))
    print("toy descent: loss %.4f -> %.4f, mu 0 -> %.4f, sigma 1 -> %.4f" % (first, last, float(mu.detach()), float(sigma.detach())))
    assert last < first and abs(float(mu.detach()) - 2.0) < 2.0


# ---- memory ---------------------------------------------------------------------------------------------------------

def test_forward_and_backward_keep_nothing_of_the_size_of_the_pairs():
    # by design: the kept gradient and the returned one (and a contiguous copy, had the input needed one), never [n, K, K]
    n, K, d = 512, 256, 16
    gen = torch.Generator(device="cuda").manual_seed(1)
    X = torch.randn(K, n, d, generator=gen, device="cuda", dtype=torch.float64).requires_grad_(True)
    Y = torch.randn(n, d, generator=gen, device="cuda", dtype=torch.float64)
    losses.energy_score_loss(X[:, :4].detach(), Y[:4])           # warm-up
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    losses.energy_score_loss(X, Y).backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    bytes_x = X.numel() * 8
    print("allocator peak of forward + backward: %.2f times the bytes of X_draws" % (peak / bytes_x))
    assert peak <= 4 * bytes_x + (1 << 20)
    assert 8 * n * K * K == 16 * bytes_x                         # what the cdist yardstick's distances alone would take
    assert bool(torch.isfinite(X.grad).all())


def test_zz_largest_deviation():
    print("largest deviation seen, in units of the terms' magnitudes (bound %.3g): %s"
          % (RTOL, ", ".join("%s %.3g" % kv for kv in WORST.items())))
    print("largest deviation of the crossed-axes cases, in units of their own bound: %s"
          % ", ".join("%s %.3g" % kv for kv in WORST_NEW.items()))
