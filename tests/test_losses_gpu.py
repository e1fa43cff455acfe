"""probaforms_amd.metrics.losses on the GPU (pfm_pair_grad in libpf_metrics.so) against the float64 restatement
(tests/pairgrad_numpy.py), the existing metrics, torch's gradcheck, and through the flow's differentiable sampling.

Tolerances.  The value is compared within 1e-12 of the sum of the magnitudes of its terms, a gradient element within 1e-12 M,
M[a, k] = 2 sum_b |w_a w_b c (z_a - z_b)[k]| from the restatement: the project's tolerance for float64 sums taken in another
order, applied to the magnitudes because the sums cancel (tests/test_losses_host.py holds the restatement itself to torch-CPU
autograd within the same bound at every shape used here).  Agreement with energy_distance_full_sample and mmd_test is held
within 4e-12 of the largest of the three means the statistic is made of.

The shapes (tests/pairgrad_numpy.py CASES): two and three pooled rows, the 64-row tile exactly and one row either side, one
feature chunk exactly (d = 16), one and two chunks spilling over (17, 33), 1200 + 1000 rows (35 tiles per side: several column
slices, many workgroups) at d = 2 (the four-feature kernel) and d = 17, copied and duplicated rows, and data centred at 1e6.
pairgrad_numpy.CROSSED crosses the axes: several column tiles per workgroup in every form of the sweep (four features, one resident
chunk, re-staged chunks with and without a full middle chunk), a ragged last slice, and one row of a sample against several tiles
of the other, where first_left's clamp and the weight 1 / 1 live.  test_zz_largest_deviation prints the largest ratios seen; on an
MI355X the crossed-axes cases were off by at most 3.1e-16 of the value's terms and 3.1e-15 M.
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import pairgrad_numpy as pg  # noqa: E402
import hygiene  # noqa: E402
import native_libs  # noqa: E402
from probaforms_amd.metrics import _boot, _lib, energy as energy_mod, losses, twosample  # noqa: E402

pytestmark = pytest.mark.gpu

native_libs.ensure_built(_lib)

AGREE = 4e-12
WORST = {"value": 0.0, "grad": 0.0}
WORST_NEW = {"value": 0.0, "grad": 0.0}                    # over pairgrad_numpy.CROSSED


def dev(A, grad=False, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(A)).to(device="cuda", dtype=dtype).requires_grad_(grad)


@functools.lru_cache(maxsize=None)
def reference(case, kind):
    """(Xr, Xf, sigmas, L, Lmag, grad, M) of a case: computed once, shared, never written to"""
    Xr, Xf = pg.make(case)
    sigmas = pg.bandwidths(kind, case[2])
    out = (Xr, Xf, sigmas) + pg.loss_and_grad(Xr, Xf, sigmas)
    for a in out:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def public(kind, Xr, Xf, sigmas, **kw):
    if kind == pg.ENERGY:
        return losses.energy_loss(Xr, Xf, **kw)
    return losses.mmd_loss(Xr, Xf, bandwidth=sigmas[0] if kind == pg.GAUSS1 else list(sigmas), **kw)


def assert_close(L, grad, want_L, Lmag, want_grad, M, what, new=False):
    verr = abs(float(L) - want_L) / Lmag
    gerr = np.abs(grad - want_grad)
    rel = float((gerr / np.where(M > 0, M, 1.0)).max())
    for worst in (WORST, WORST_NEW) if new else (WORST,):
        worst["value"], worst["grad"] = max(worst["value"], verr), max(worst["grad"], rel)
    print("%s: value off by %.3g of its terms, gradient by at most %.3g of M" % (what, verr, rel))
    assert verr <= pg.TOL, what
    assert (gerr <= pg.TOL * M).all(), what


# ---- value and gradient against the restatement -----------------------------------------------------------

@pytest.mark.parametrize("kind", pg.KINDS)
@pytest.mark.parametrize("case", pg.CASES, ids=pg.case_id)
def test_value_and_gradient_equal_the_restatement(case, kind):
    Xr, Xf, sigmas, want_L, Lmag, want_grad, M = reference(case, kind)
    A, B = dev(Xr, True), dev(Xf, True)
    L = public(kind, A, B, sigmas)
    assert L.shape == () and L.dtype == torch.float64 and L.is_cuda and L.grad_fn is not None
    L.backward()
    grad = torch.cat([A.grad, B.grad]).cpu().numpy()
    assert np.isfinite(grad).all()
    assert_close(L, grad, want_L, Lmag, want_grad, M, pg.case_id(case) + " " + kind, case in pg.CROSSED)
    if case[3] == "copies":           # duplicated fake rows add exactly 0 to each other and see the others alike
        assert hygiene.same_bits(B.grad[1], B.grad[2])


def test_several_bandwidths_sum_the_single_ones():
    Xr, Xf, sigmas, _, Lmag, _, M = reference((65, 63, 17, "plain"), pg.GAUSS3)
    A, B = dev(Xr), dev(Xf, True)
    both = losses.mmd_loss(A, B, bandwidth=tuple(sigmas))
    both.backward()
    g_both, B.grad = B.grad, None
    total = 0.0
    for s in sigmas:
        one = losses.mmd_loss(A, B, bandwidth=s)
        one.backward()
        total += float(one)
    assert abs(float(both) - total) <= pg.TOL * Lmag
    assert ((g_both - B.grad).abs().cpu().numpy() <= pg.TOL * M[65:]).all()


# ---- agreement with the existing metrics -------------------------------------------------------------------

@pytest.mark.parametrize("case", [(65, 63, 17, "plain"), (1200, 1000, 2, "plain"), (40, 50, 5, "far"), (130, 70, 2, "copies")],
                         ids=pg.case_id)
def test_energy_loss_equals_energy_distance_full_sample(case):
    Xr, Xf = pg.make(case)
    exx, eyy, exy = energy_mod._means(Xr, Xf, None, False)[0]
    want = energy_mod.energy_distance_full_sample(Xr, Xf, squared=True)
    got = float(losses.energy_loss(Xr, Xf))
    print("D^2 %.17g against %.17g: off by %.3g of max(exx, eyy, exy)" % (got, want, abs(got - want) / max(exx, eyy, exy)))
    assert abs(got - want) <= AGREE * max(exx, eyy, exy)


def kernel_means(Xr, Xf, sigma):
    """mean K_XX, mean K_YY, mean K_XY in numpy"""
    def mean(A, B):
        d2 = ((A[:, None, :] - B[None, :, :]) ** 2).sum(axis=2)
        return float(np.exp(-d2 / (2.0 * sigma ** 2)).mean())
    return mean(Xr, Xr), mean(Xf, Xf), mean(Xr, Xf)


@pytest.mark.parametrize("bandwidth", [None, 1.7])
@pytest.mark.parametrize("case", [(65, 63, 17, "plain"), (130, 70, 2, "copies"), (40, 50, 5, "far")], ids=pg.case_id)
def test_mmd_loss_equals_mmd_test_statistic(case, bandwidth):
    Xr, Xf = pg.make(case)
    state = np.random.get_state()
    try:
        want = twosample.mmd_test(Xr, Xf, n_permutations=1, bandwidth=bandwidth).statistic
    finally:
        np.random.set_state(state)
    got = float(losses.mmd_loss(Xr, Xf, bandwidth=bandwidth))
    sigma = bandwidth if bandwidth is not None else twosample._median(dev(Xr), dev(Xf))
    scale = max(kernel_means(Xr, Xf, sigma))
    print("MMD^2 %.17g against %.17g: off by %.3g of the largest kernel mean" % (got, want, abs(got - want) / scale))
    assert abs(got - want) <= AGREE * scale


# ---- gradcheck -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", pg.KINDS)
def test_gradcheck_on_the_public_functions(kind):
    Xr, Xf = pg.make((5, 4, 3, "plain"))                       # distinct rows
    sigmas = pg.bandwidths(kind, 3)
    assert torch.autograd.gradcheck(lambda a, b: public(kind, a, b, sigmas), (dev(Xr, True), dev(Xf, True)))


# ---- plumbing -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", (pg.ENERGY, pg.GAUSS1))
def test_gradient_goes_to_the_inputs_that_ask(kind):
    case = (65, 63, 17, "plain")
    Xr, Xf, sigmas, want_L, Lmag, want_grad, M = reference(case, kind)
    both = [dev(Xr, True), dev(Xf, True)]
    public(kind, both[0], both[1], sigmas).backward()
    # fake only (what training a generator does), real only
    A, B = dev(Xr), dev(Xf, True)
    L = public(kind, A, B, sigmas)
    L.backward()
    assert A.grad is None and hygiene.same_bits(B.grad, both[1].grad)
    A, B = dev(Xr, True), dev(Xf)
    public(kind, A, B, sigmas).backward()
    assert B.grad is None and hygiene.same_bits(A.grad, both[0].grad)
    # neither: the value alone, no node; numpy inputs as well
    for a, b in ((dev(Xr), dev(Xf)), (Xr, Xf), (Xr.tolist(), dev(Xf))):
        V = public(kind, a, b, sigmas)
        assert V.grad_fn is None and not V.requires_grad and V.is_cuda and V.dtype == torch.float64
        assert abs(float(V) - want_L) <= pg.TOL * Lmag
    # the incoming scalar
    A, B = dev(Xr, True), dev(Xf, True)
    (3 * public(kind, A, B, sigmas)).backward()
    assert torch.equal(A.grad, 3 * both[0].grad) and torch.equal(B.grad, 3 * both[1].grad)


def test_float32_inputs_get_float32_gradients():
    Xr, Xf = pg.make((65, 63, 17, "plain"))
    A, B = dev(Xr, True, torch.float32), dev(Xf, True, torch.float32)
    L = losses.energy_loss(A, B)
    assert L.dtype == torch.float64
    L.backward()
    assert A.grad.dtype == torch.float32 == B.grad.dtype and A.grad.shape == A.shape and B.grad.shape == B.shape
    A64, B64 = A.detach().double().requires_grad_(True), B.detach().double().requires_grad_(True)
    L64 = losses.energy_loss(A64, B64)
    L64.backward()
    assert hygiene.same_bits(L.reshape(1), L64.reshape(1))                                    # the upcast is exact
    assert torch.equal(A.grad, A64.grad.float()) and torch.equal(B.grad, B64.grad.float())     # one rounding, at the end


@pytest.mark.parametrize("kind", (pg.ENERGY, pg.GAUSS3))
def test_views_give_the_gradient_of_the_contiguous_copy(kind):
    Xr, Xf, sigmas = reference((65, 63, 17, "plain"), kind)[:3]
    A = dev(Xr)
    B = dev(Xf, True)
    public(kind, A, B, sigmas).backward()
    wide = torch.full((63, 17 + 5), 7.0, dtype=torch.float64, device="cuda")
    wide[:, 2:19] = B.detach()
    wide.requires_grad_(True)
    public(kind, A, wide[:, 2:19], sigmas).backward()
    assert hygiene.same_bits(wide.grad[:, 2:19], B.grad)
    assert not wide.grad[:, :2].any() and not wide.grad[:, 19:].any()
    T = B.detach().t().contiguous().requires_grad_(True)               # [d, nf]: the sample is its transposed view
    public(kind, A, T.t(), sigmas).backward()
    assert hygiene.same_bits(T.grad.t(), B.grad)
    every = B.detach().repeat_interleave(2, dim=0).requires_grad_(True)       # every second row
    public(kind, A[::1], every[::2], sigmas).backward()
    assert hygiene.same_bits(every.grad[::2], B.grad) and not every.grad[1::2].any()


def scaler_bound(Z, nr, M):
    """M pushed through the backward of _boot.standardize with every coefficient's magnitude.  With mu, sd of the real rows and
    G the gradient by the standardized rows, dL/dB = G_B / sd and
      dL/dA_i = G_i / sd - (sum_all G / sd) / nr - (sum_all G (Z - mu) / sd^2) (A_i - mu) / (nr sd)
    are linear in G, so an elementwise error of at most 1e-12 M in G is at most 1e-12 times this in the result."""
    A = Z[:nr]
    mu, sd = A.mean(axis=0), A.std(axis=0)
    sd = np.where(sd == 0, 1.0, sd)
    out = M / sd
    out[:nr] += (M / sd).sum(axis=0) / nr + (M * np.abs(Z - mu) / sd ** 2).sum(axis=0) * np.abs(A - mu) / (nr * sd)
    return out


def torch_loss(Zs, nr, sigmas):
    """the restatement's formula in float64 torch ops on the device of Zs"""
    N = Zs.shape[0]
    w = torch.from_numpy(pg.weights(nr, N - nr)).to(Zs.device)                    # built in float64
    diff = Zs[:, None, :] - Zs[None, :, :]
    d2 = (diff * diff).sum(dim=2)
    if sigmas is None:
        pos = d2 > 0
        g = -torch.where(pos, torch.where(pos, d2, torch.ones_like(d2)).sqrt(), torch.zeros_like(d2))
    else:
        g = sum(torch.exp(-(1.0 / (2.0 * float(s) ** 2)) * d2) for s in sigmas)
    return (w[:, None] * w[None, :] * g).sum()


@pytest.mark.parametrize("kind", (pg.ENERGY, pg.GAUSS1))
def test_standardize_carries_the_scalers_derivative(kind):
    Xr, Xf = pg.make((40, 50, 5, "plain"))
    Xr = Xr * np.array([1.0, 10.0, 0.1, 3.0, 1.0]) + np.array([0.0, 5.0, -2.0, 100.0, 1.0])
    Xf = Xf * np.array([1.0, 10.0, 0.1, 3.0, 1.0]) + np.array([0.0, 5.0, -2.0, 100.0, 1.0])
    sigmas = pg.bandwidths(kind, 5)
    A, B = dev(Xr, True), dev(Xf, True)
    L = public(kind, A, B, sigmas, standardize=True)
    L.backward()
    A2, B2 = dev(Xr, True), dev(Xf, True)
    As, Bs = _boot.standardize(A2, B2)
    L2 = torch_loss(torch.cat([As, Bs]), 40, sigmas)
    L2.backward()
    Zs = torch.cat([As, Bs]).detach().cpu().numpy()
    _, Lmag, _, M = pg.loss_and_grad(Zs[:40], Zs[40:], sigmas)
    bound = pg.TOL * scaler_bound(np.concatenate([Xr, Xf]), 40, M)
    # twice: the yardstick's own sums are float64 sums in yet another order
    err = (torch.cat([A.grad, B.grad]) - torch.cat([A2.grad, B2.grad])).abs().cpu().numpy()
    print("standardize, %s: value off by %.3g of its terms, gradient by at most %.3g of the bound"
          % (kind, abs(float(L) - float(L2)) / Lmag, float((err / bound).max())))
    assert abs(float(L) - float(L2)) <= 2 * pg.TOL * Lmag
    assert (err <= 2 * bound).all()


# ---- reproducibility and workspace hygiene -----------------------------------------------------------------

@pytest.mark.parametrize("kind", pg.KINDS)
def test_two_calls_give_identical_bytes(kind):
    Xr, Xf, sigmas = reference((1200, 1000, 17, "plain"), kind)[:3]
    outs = []
    for _ in range(2):
        A, B = dev(Xr, True), dev(Xf, True)
        L = public(kind, A, B, sigmas)
        L.backward()
        outs.append((L.detach().reshape(1), A.grad, B.grad))
        torch.empty(1 << 22, device="cuda").fill_(float("nan"))          # the allocator hands other memory to the next call
    for a, b in zip(*outs):
        assert hygiene.same_bits(a, b)


@pytest.mark.parametrize("kind", (pg.ENERGY, pg.GAUSS3))
@pytest.mark.parametrize("case", [(65, 63, 17, "plain"), (1200, 1000, 2, "plain"), (2, 1, 33, "plain")], ids=pg.case_id)
def test_outputs_do_not_depend_on_the_workspace(case, kind):
    Xr, Xf, sigmas = reference(case, kind)[:3]
    Z = dev(np.concatenate([Xr, Xf]))
    nr, (N, d) = len(Xr), Z.shape
    k = _lib.PERM_ENERGY if sigmas is None else _lib.PERM_GAUSS
    gammas = [] if sigmas is None else [1.0 / (2.0 * s * s) for s in sigmas]
    nbytes = _lib.pair_grad_workspace_bytes(N, d, nr)
    outs = {}
    for pattern in hygiene.PATTERNS:
        ws = hygiene.workspace(nbytes, pattern)
        if pattern == "replay":                                           # as another call left it: other data, other split
            other = torch.empty_like(Z)
            scrap = torch.empty(1, dtype=torch.float64, device="cuda")
            assert _lib.pair_grad_status(k, gammas, (Z * 3.0 + 1.0).contiguous(), max(1, nr // 2), scrap, other, ws) == 0
        value = torch.empty(1, dtype=torch.float64, device="cuda")
        grad = torch.empty_like(Z)
        hygiene.poison_outputs(value, grad)
        assert _lib.pair_grad_status(k, gammas, Z, nr, value, grad, ws) == 0
        value_only = torch.empty(1, dtype=torch.float64, device="cuda")
        hygiene.poison_outputs(value_only)
        assert _lib.pair_grad_status(k, gammas, Z, nr, value_only, None, hygiene.workspace(nbytes, pattern)) == 0
        torch.cuda.synchronize()
        outs[pattern] = {"value": value, "grad": grad, "value_only": value_only}
        hygiene.assert_all_written(outs[pattern], "pfm_pair_grad %s %s" % (pg.case_id(case), pattern))
        assert hygiene.same_bits(value, value_only)                       # the sweep without the gradient sums alike
    hygiene.assert_pattern_independent(outs, "pfm_pair_grad %s" % pg.case_id(case))


# ---- through the flow seam ---------------------------------------------------------------------------------

def test_energy_loss_trains_a_flow_through_its_sampler():
    """X = model.nf.sample(C) is float32; X.double() is the input, so that its float64 gradient can be held to the
    restatement's bound, and X.grad is that gradient rounded once to float32."""
    from probaforms_amd.models import RealNVP
    rng = np.random.RandomState(5)
    n = 300
    C0 = rng.uniform(-1, 1, size=(n, 1)).astype(np.float32)
    X0 = (np.concatenate([np.sin(3 * C0), np.cos(3 * C0)], axis=1) + 0.1 * rng.normal(size=(n, 2))).astype(np.float32)
    torch.manual_seed(7)
    model = RealNVP(n_layers=3, hidden=(8,), n_epochs=1, batch_size=100)
    model.fit(X0, C0)
    for p in model.nf.parameters():
        p.grad = None
    C = torch.from_numpy(C0).cuda()
    X = model.nf.sample(C)
    assert X.requires_grad and X.shape == (n, 2)
    X.retain_grad()
    Xd = X.double()
    Xd.retain_grad()
    L = losses.energy_loss(X0, Xd)
    L.backward()
    want_L, Lmag, want_grad, M = pg.loss_and_grad(X0.astype(np.float64), X.detach().double().cpu().numpy(), None)
    assert_close(L, Xd.grad.cpu().numpy(), want_L, Lmag, want_grad[n:], M[n:], "flow seam")
    assert torch.equal(X.grad, Xd.grad.float())
    grads = [p.grad for p in model.nf.parameters()]
    assert all(g is not None and bool(torch.isfinite(g).all()) for g in grads)
    assert any(bool(g.ne(0).any()) for g in grads)


# ---- no host synchronisation -------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", pg.KINDS)
def test_forward_and_backward_never_wait_for_the_device(kind):
    Xr, Xf, sigmas = reference((65, 63, 17, "plain"), kind)[:3]
    A = dev(Xr)
    W = dev(np.concatenate([Xf, Xf], axis=1), True)
    public(kind, A, W[:, :17], sigmas).backward()                           # warm-up: library, code objects, allocator
    W.grad = None
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        L = public(kind, A, W[:, :17], sigmas)
        (2 * L).backward()
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert bool(torch.isfinite(W.grad).all()) and bool(W.grad[:, :17].ne(0).any())


# ---- argument errors ---------------------------------------------------------------------------------------

def test_argument_errors():
    X, Y = dev(np.zeros((5, 3))), dev(np.ones((4, 3)))
    for fn in (losses.energy_loss, losses.mmd_loss):
        with pytest.raises(ValueError, match="different numbers of features"):
            fn(X, Y[:, :2])
        with pytest.raises(ValueError, match="2-D"):
            fn(X[:, 0], Y)
        with pytest.raises(ValueError, match="standardize must be a bool"):
            fn(X, Y, standardize=1)
    for bad in (0, -1.0, [], [1.0] * 9, [1.0, 0.0]):
        with pytest.raises(ValueError, match="bandwidth"):
            losses.mmd_loss(X, Y, bandwidth=bad)
    with pytest.raises(ValueError, match="median pairwise distance is 0"):
        losses.mmd_loss(np.ones((6, 2)), np.ones((5, 2)))
    with pytest.raises(ValueError, match="median pairwise distance is 0"):
        twosample.mmd_test(np.ones((6, 2)), np.ones((5, 2)), n_permutations=1)


def test_nan_propagates_and_is_not_checked():
    Xr, Xf = pg.make((65, 63, 17, "plain"))
    Xf = Xf.copy()
    Xf[3, 2] = np.nan
    for kind in (pg.ENERGY, pg.GAUSS1):
        B = dev(Xf, True)
        L = public(kind, dev(Xr), B, pg.bandwidths(kind, 17))
        L.backward()
        assert bool(torch.isnan(L)) and bool(torch.isnan(B.grad[3]).all())


def test_zz_largest_deviation():
    print("largest deviation seen: value %.3g of its terms, gradient %.3g M (bound %.3g for both); of the crossed-axes cases: "
          "value %.3g, gradient %.3g" % (WORST["value"], WORST["grad"], pg.TOL, WORST_NEW["value"], WORST_NEW["grad"]))
