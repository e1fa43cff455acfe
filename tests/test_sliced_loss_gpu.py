"""probaforms_amd.metrics.losses.sliced_wasserstein_loss / wasserstein_1d_loss and wasserstein.sliced_wasserstein_full_sample on
the GPU (pfm_slice_grad in libpf_metrics.so) against the float64 restatement (tests/slicegrad_numpy.py), the existing
pfm_wasserstein1d, torch's gradcheck, and through the flow's differentiable sampling.

Tolerances, the project's for float64 sums taken in another order: the value within 1e-12 Lmag (the sum of the magnitudes of its
terms), every gradient element within 1e-12 M (the sum of the magnitudes of the element's own terms), both from the restatement.
The projections are bitwise the restatement's and the order is byte for byte np.lexsort's by (value, row): that pins the sort.  The
largest ratios seen are printed by test_zz_largest_deviation; on an MI355X the crossed-axes cases (slicegrad_numpy.CROSSED and
CROSSED_AXES) were off by at most 4.1e-16 Lmag and 9.9e-16 M.

Shapes: slicegrad_numpy.ROWS (one and two rows, the 64-entry and 1024-entry edges of the sort network and one row either side, so
the virtual padding; (100, 37) and (37, 100) for long partner ranges on one side) at d = 2, P = 3; around (65, 63) d in 1, 2, 16, 17
and P in 1, 3, 64, 65, one axis at a time; the LDS cap and one row above it (the torch.sort route).  slicegrad_numpy.CROSSED
crosses them: (300, 250, 17, 9) is three blocks of 256 rows by two chunks of 16 features by two groups of 8 directions in
k_slice_project, (1, 1025) and (1025, 1) couple one element with a whole sample; CROSSED_AXES takes the coordinate-axes route over
several row blocks and direction groups.  All with p = 1 and 2.
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
import native_libs  # noqa: E402
import slicegrad_numpy as sl  # noqa: E402
from probaforms_amd.metrics import _lib, _m1d, losses, wasserstein  # noqa: E402

pytestmark = pytest.mark.gpu

native_libs.ensure_built(_lib)

RTOL = 1e-12
CAP = _lib.SLICE_LDS_ROWS
# (nr, nf, d, P)
CASES = [(nr, nf, 2, 3) for nr, nf in sl.ROWS]
CASES += [sl.MIDDLE + (d, 3) for d in sl.FEATURES] + [sl.MIDDLE + (2, P) for P in sl.PROJECTIONS]
CASES = sorted(set(CASES)) + sl.CROSSED
AXES_SIZES = [(65, 63, 3), (100, 37, 1), (2, 3, 17)] + sl.CROSSED_AXES
CAP_CASES = [(CAP, CAP, 2, 2), (CAP + 1, 50, 2, 2)]
WORST = {"value": 0.0, "grad": 0.0}
WORST_NEW = {"value": 0.0, "grad": 0.0}                    # over slicegrad_numpy.CROSSED and CROSSED_AXES


def case_id(case):
    return "%dx%d_d%d_P%d" % case


def dev(A, grad=False, dtype=torch.float64):
    return torch.from_numpy(np.array(A)).to(device="cuda", dtype=dtype).requires_grad_(grad)


@functools.lru_cache(maxsize=None)
def reference(case, p):
    """(Xr, Xf, theta, restatement dict) of a case: computed once, shared, never written to"""
    nr, nf, d, P = case
    Xr, Xf = sl.make(nr, nf, d)
    theta = sl.unit_directions(P, d)
    o = sl.value_grad(Xr, Xf, theta, p, vectorised=max(nr, nf) > 2048)
    for a in (Xr, Xf, theta) + tuple(v for v in o.values() if isinstance(v, np.ndarray)):
        a.setflags(write=False)
    return Xr, Xf, theta, o


def raw(Xr, Xf, theta, p, want_rows=True):
    """losses._slice_call with the projections and the order asked for -> (value, rows, cols, perm) as numpy"""
    Z = dev(np.concatenate([Xr, Xf]))
    N, d = Z.shape
    P = d if theta is None else len(theta)
    cols = torch.full((P, N), float("nan"), dtype=torch.float64, device="cuda")
    perm = torch.full((P, N), -7, dtype=torch.int32, device="cuda")
    value, rows = losses._slice_call(p, Z, len(Xr), None if theta is None else dev(theta), want_rows, cols, perm)
    return float(value), None if rows is None else rows.cpu().numpy(), cols.cpu().numpy(), perm.cpu().numpy()


def assert_close(value, grad, want, what, new=False):
    verr = abs(value - want["value"]) / want["Lmag"] if want["Lmag"] > 0 else abs(value - want["value"])
    gerr = np.abs(grad - want["grad"])
    rel = float((gerr / np.where(want["M"] > 0, want["M"], 1.0)).max())
    for worst in (WORST, WORST_NEW) if new else (WORST,):
        worst["value"], worst["grad"] = max(worst["value"], verr), max(worst["grad"], rel)
    print("%s: value off by %.3g Lmag, gradient by at most %.3g M" % (what, verr, rel))
    assert np.isfinite(grad).all(), what
    assert abs(value - want["value"]) <= RTOL * want["Lmag"], what
    assert (gerr <= RTOL * want["M"]).all(), what


# ---- value, gradient, projections and order against the restatement ---------------------------------------------

@pytest.mark.parametrize("p", (1, 2))
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_value_gradient_projections_and_order_equal_the_restatement(case, p):
    Xr, Xf, theta, want = reference(case, p)
    value, rows, cols, perm = raw(Xr, Xf, theta, p)
    assert np.array_equal(cols.view(np.int64), want["cols"].view(np.int64))           # bitwise
    assert perm.dtype == np.int32 and perm.tobytes() == want["perm"].tobytes()        # np.lexsort's order
    assert_close(value, rows, want, "%s p=%d" % (case_id(case), p), case in sl.CROSSED)
    # the public function: the same kernel call behind an autograd node
    A, B = dev(Xr, True), dev(Xf, True)
    L = losses.sliced_wasserstein_loss(A, B, p=p, directions=dev(theta))
    assert L.shape == () and L.dtype == torch.float64 and L.is_cuda and L.grad_fn is not None
    L.backward()
    assert float(L.detach()) == value and np.array_equal(torch.cat([A.grad, B.grad]).cpu().numpy(), rows)
    # the value alone is formed alike
    assert raw(Xr, Xf, theta, p, want_rows=False)[0] == value


@pytest.mark.parametrize("p", (1, 2))
@pytest.mark.parametrize("case", CAP_CASES, ids=case_id)
def test_lds_cap_and_one_row_above_it(case, p, monkeypatch):
    Xr, Xf, theta, want = reference(case, p)
    seen = []
    status = _lib.slice_grad_status

    def spy(p_, Z, n_first, th, n_proj, perm_in, *rest):
        seen.append(perm_in)
        return status(p_, Z, n_first, th, n_proj, perm_in, *rest)
    monkeypatch.setattr(_lib, "slice_grad_status", spy)
    value, rows, cols, perm = raw(Xr, Xf, theta, p)
    assert len(seen) == 1 and (seen[0] is None) == (max(case[:2]) <= CAP)             # one row above the cap: torch.sort's order
    assert perm.tobytes() == want["perm"].tobytes()
    assert np.array_equal(cols.view(np.int64), want["cols"].view(np.int64))
    assert_close(value, rows, want, "%s p=%d" % (case_id(case), p))


# ---- ties ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("p", (1, 2))
@pytest.mark.parametrize("size", [(65, 63), (100, 37), (1025, 1023)], ids=str)
def test_integer_data_with_many_duplicates(size, p):
    nr, nf = size
    rng = np.random.RandomState(nr)
    Xr, Xf = rng.randint(0, 4, size=(nr, 2)).astype(np.float64), rng.randint(0, 5, size=(nf, 2)).astype(np.float64)
    theta = np.array([[1.0, 0.0], [0.0, 1.0], [1.0, 1.0], [1.0, -1.0]])
    want = sl.value_grad(Xr, Xf, theta, p)
    value, rows, cols, perm = raw(Xr, Xf, theta, p)
    assert perm.tobytes() == want["perm"].tobytes() and np.array_equal(cols, want["cols"])
    assert_close(value, rows, want, "integers %s p=%d" % (size, p))


@pytest.mark.parametrize("p", (1, 2))
def test_a_projection_on_which_every_row_is_equal_adds_exactly_nothing(p):
    Xr, Xf = sl.make(65, 63, 2)
    Xr, Xf = Xr.copy(), Xf.copy()
    Xr[:, 1] = Xf[:, 1] = 0.0                                  # data along x
    value, rows, cols, perm = raw(Xr, Xf, np.array([[0.0, 1.0]]), p)
    assert value == 0.0 and not rows.any() and not cols.any()
    assert np.array_equal(perm[0], np.arange(128))             # all tied: the index decides


@pytest.mark.parametrize("p", (1, 2))
def test_fake_rows_that_copy_real_rows(p):
    Xr, Xf = sl.make(65, 63, 3)
    theta = sl.unit_directions(5, 3)
    Xf = Xf.copy()
    Xf[:20] = Xr[10:30]
    want = sl.value_grad(Xr, Xf, theta, p)
    value, rows, cols, perm = raw(Xr, Xf, theta, p)
    assert np.isfinite(rows).all() and perm.tobytes() == want["perm"].tobytes()
    assert_close(value, rows, want, "copies p=%d" % p)
    # every row copied, nr = nf: the samples are equal
    A, B = dev(Xr, True), dev(Xr.copy(), True)
    L = losses.sliced_wasserstein_loss(A, B, p=p, directions=theta)
    L.backward()
    assert float(L.detach()) == 0.0 and not bool(A.grad.any()) and not bool(B.grad.any())


# ---- the two sort routes ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("p", (1, 2))
@pytest.mark.parametrize("case", [(65, 63, 2, 3), (1025, 1023, 2, 3)], ids=case_id)
def test_both_sort_routes_give_the_same_bytes(case, p, monkeypatch):
    Xr, Xf, theta, want = reference(case, p)
    own = raw(Xr, Xf, theta, p)
    seen = []
    status = _lib.slice_grad_status

    def spy(p_, Z, n_first, th, n_proj, perm_in, *rest):
        seen.append(perm_in)
        return status(p_, Z, n_first, th, n_proj, perm_in, *rest)
    monkeypatch.setattr(_lib, "slice_grad_status", spy)
    monkeypatch.setattr(losses, "_MAX_LDS_ROWS", 0)
    given = raw(Xr, Xf, theta, p)
    assert len(seen) == 1 and seen[0] is not None
    assert own[0] == given[0]
    for a, b in zip(own[1:], given[1:]):
        assert a.tobytes() == b.tobytes()
    # and the coordinate axes
    a, b = sl.make(case[0], case[1], 3)
    monkeypatch.setattr(losses, "_MAX_LDS_ROWS", CAP)
    own = raw(a, b, None, p)
    monkeypatch.setattr(losses, "_MAX_LDS_ROWS", 0)
    given = raw(a, b, None, p)
    assert own[0] == given[0] and all(x.tobytes() == y.tobytes() for x, y in zip(own[1:], given[1:]))


# ---- reproducibility and workspace hygiene -------------------------------------------------------------------------

def test_two_calls_give_identical_bytes():
    Xr, Xf, theta, want = reference((1025, 1023, 2, 3), 2)
    outs = []
    for _ in range(2):
        A, B = dev(Xr, True), dev(Xf, True)
        L = losses.sliced_wasserstein_loss(A, B, p=2, directions=dev(theta))
        L.backward()
        outs.append((L.detach().reshape(1), A.grad, B.grad))
        torch.empty(1 << 22, device="cuda").fill_(float("nan"))          # the allocator hands other memory to the next call
    for a, b in zip(*outs):
        assert hygiene.same_bits(a, b)


@pytest.mark.parametrize("p", (1, 2))
@pytest.mark.parametrize("case", [(65, 63, 17, 3), (1025, 1023, 2, 3), (2, 1, 2, 64)], ids=case_id)
def test_outputs_do_not_depend_on_the_workspace(case, p):
    nr, nf, d, P = case
    Xr, Xf = sl.make(nr, nf, d)
    Z, theta = dev(np.concatenate([Xr, Xf])), dev(sl.unit_directions(P, d))
    N = nr + nf
    nbytes = _lib.slice_grad_workspace_bytes(N, d, nr, P)
    given = losses._given_order(Z, nr, theta)

    def outputs(rows=True):
        o = {"value": torch.empty(1, dtype=torch.float64, device="cuda"),
             "cols": torch.empty((P, N), dtype=torch.float64, device="cuda"),
             "perm": torch.empty((P, N), dtype=torch.int32, device="cuda")}
        if rows:
            o["rows"] = torch.empty_like(Z)
        hygiene.poison_outputs(*o.values())
        return o

    outs = {}
    for pattern in ("zeros", "ones"):
        got = {}
        for perm_in, tag in ((None, ""), (given, "_given")):
            o = outputs()
            _lib.slice_grad(p, Z, nr, theta, P, perm_in, o["value"], o["rows"], o["cols"], o["perm"],
                            hygiene.workspace(nbytes, pattern))
            v = outputs(rows=False)
            _lib.slice_grad(p, Z, nr, theta, P, perm_in, v["value"], None, v["cols"], v["perm"], hygiene.workspace(nbytes, pattern))
            torch.cuda.synchronize()
            got.update({k + tag: t for k, t in o.items()})
            got.update({"only_" + k + tag: t for k, t in v.items()})
            for k in ("value", "cols", "perm"):
                assert hygiene.same_bits(o[k], v[k])
        for k in ("value", "rows", "cols", "perm"):                      # the two routes
            assert hygiene.same_bits(got[k], got[k + "_given"])
        hygiene.assert_all_written(got, "pfm_slice_grad %s %s" % (case_id(case), pattern))
        outs[pattern] = got
    hygiene.assert_pattern_independent(outs, "pfm_slice_grad %s" % case_id(case))


# ---- wasserstein_1d_loss ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("p", (1, 2))
@pytest.mark.parametrize("size", AXES_SIZES, ids=str)
def test_wasserstein_1d_loss_is_the_restatement_on_the_coordinate_axes(size, p):
    Xr, Xf = sl.make(*size)
    want = sl.value_grad(Xr, Xf, None, p)
    A, B = dev(Xr, True), dev(Xf, True)
    L = losses.wasserstein_1d_loss(A, B, p=p)
    assert L.shape == () and L.dtype == torch.float64 and L.grad_fn is not None
    L.backward()
    assert_close(float(L.detach()), torch.cat([A.grad, B.grad]).cpu().numpy(), want, "axes %s p=%d" % (size, p),
                 size in sl.CROSSED_AXES)
    value, rows, cols, perm = raw(Xr, Xf, None, p)
    assert np.array_equal(cols, want["cols"]) and perm.tobytes() == want["perm"].tobytes()
    ident = sl.value_grad(Xr, Xf, np.eye(size[2]), p)
    assert abs(want["value"] - ident["value"]) <= RTOL * want["Lmag"] and (np.abs(want["grad"] - ident["grad"]) <= RTOL * want["M"]).all()
    assert losses.wasserstein_1d_loss(Xr, Xf).grad_fn is None             # default p = 1, numpy inputs, the value alone


@pytest.mark.parametrize("p", (1, 2))
def test_an_infinity_stays_in_its_own_feature(p):
    Xr, Xf = sl.make(65, 63, 3)
    want = sl.value_grad(Xr, Xf, None, p)
    Xf = Xf.copy()
    Xf[5, 1] = np.inf
    value, rows, cols, perm = raw(Xr, Xf, None, p)
    assert not np.isfinite(value)
    for j in (0, 2):                                            # the clean features' terms are what they were
        assert np.isfinite(rows[:, j]).all()
        assert (np.abs(rows[:, j] - want["grad"][:, j]) <= RTOL * want["M"][:, j]).all()
        assert perm[j].tobytes() == want["perm"][j].tobytes()


# ---- the existing kernel computes the same number --------------------------------------------------------------

@pytest.mark.parametrize("p", (1, 2))
@pytest.mark.parametrize("case", [(65, 63, 2, 3), (100, 37, 2, 3), (1025, 1023, 2, 3)], ids=case_id)
def test_per_projection_value_equals_pfm_wasserstein1d(case, p):
    Xr, Xf, theta, want = reference(case, p)
    nr, nf, d, P = case
    cols = dev(want["cols"])
    pooled = _m1d.Pooled.from_columns(cols, nr)
    out = torch.empty((1, P), dtype=torch.float64, device="cuda")
    ws = torch.empty(max(16, _lib.wasserstein1d_workspace_bytes(nr, nf, P, 1, p)), dtype=torch.uint8, device="cuda")
    ir, jf = (torch.arange(n, dtype=torch.int32, device="cuda") for n in (nr, nf))
    _lib.wasserstein1d(p, pooled.cols, pooled.perm, pooled.gstart, pooled.ngroups, nr, nf, ir, jf, 1, out, ws)
    other = out.cpu().numpy()[0]
    for k in range(P):
        mine = raw(Xr, Xf, theta[k:k + 1], p, want_rows=False)[0]
        print("direction %d: pfm_slice_grad %.17g, pfm_wasserstein1d %.17g, restatement %.17g" % (k, mine, other[k], want["W"][k]))
        assert abs(mine - other[k]) <= RTOL * want["W"][k]


# ---- sliced_wasserstein_full_sample and the drawn directions ------------------------------------------------------

@pytest.mark.parametrize("p", (1, 2))
def test_full_sample_is_the_root_of_the_loss_on_the_same_draw(p):
    Xr, Xf = sl.make(100, 37, 3)
    np.random.seed(123)
    metric = wasserstein.sliced_wasserstein_full_sample(Xr, Xf, n_projections=7, p=p)
    after = np.random.get_state()
    np.random.seed(123)
    L = losses.sliced_wasserstein_loss(Xr, Xf, n_projections=7, p=p)
    after_loss = np.random.get_state()
    np.random.seed(123)
    theta = wasserstein.directions(7, 3)
    alone = np.random.get_state()
    for st in (after, after_loss):
        assert st[0] == alone[0] and np.array_equal(st[1], alone[1]) and st[2:] == alone[2:]
    want = sl.value_grad(Xr, Xf, theta, p)
    assert isinstance(metric, np.float64) and L.grad_fn is None
    assert abs(float(L) - want["value"]) <= RTOL * want["Lmag"]
    root = float(L) ** (1.0 / p)
    # d root / d L = root / (p L): the value's tolerance carried through the root
    assert abs(metric - root) <= RTOL * want["Lmag"] * root / (p * float(L)) + 2e-16 * root
    # the bootstrap metric draws the same directions first, then its resamples
    np.random.seed(123)
    wasserstein.sliced_wasserstein_distance(Xr, Xf, n_iters=1, n_projections=7, p=p)
    metric_state = np.random.get_state()
    np.random.seed(123)
    wasserstein.directions(7, 3)
    np.random.randint(0, 100, size=100), np.random.randint(0, 37, size=37)
    assert np.array_equal(metric_state[1], np.random.get_state()[1]) and metric_state[2] == np.random.get_state()[2]


# ---- inputs and routing ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("p", (1, 2))
def test_gradcheck_on_the_public_function(p):
    Xr, Xf = sl.make(5, 4, 3)
    theta = dev(sl.unit_directions(4, 3))
    assert torch.autograd.gradcheck(lambda a, b: losses.sliced_wasserstein_loss(a, b, p=p, directions=theta),
                                    (dev(Xr, True), dev(Xf, True)))
    assert torch.autograd.gradcheck(lambda a, b: losses.wasserstein_1d_loss(a, b, p=p), (dev(Xr, True), dev(Xf, True)))


def test_gradient_goes_to_the_inputs_that_ask(monkeypatch):
    Xr, Xf, theta, want = reference((65, 63, 2, 3), 2)
    th = dev(theta, True)                                       # a constant, even if it asks
    both = [dev(Xr, True), dev(Xf, True)]
    losses.sliced_wasserstein_loss(both[0], both[1], directions=th).backward()
    assert th.grad is None
    A, B = dev(Xr), dev(Xf, True)
    losses.sliced_wasserstein_loss(A, B, directions=th).backward()
    assert A.grad is None and hygiene.same_bits(B.grad, both[1].grad)
    A, B = dev(Xr, True), dev(Xf)
    (3 * losses.sliced_wasserstein_loss(A, B, directions=th)).backward()
    assert B.grad is None and torch.equal(A.grad, 3 * both[0].grad)
    seen = []
    status = _lib.slice_grad_status

    def spy(p_, Z, n_first, th_, n_proj, perm_in, value, rows, *rest):
        seen.append(rows)
        return status(p_, Z, n_first, th_, n_proj, perm_in, value, rows, *rest)
    monkeypatch.setattr(_lib, "slice_grad_status", spy)
    for a, b in ((dev(Xr), dev(Xf)), (Xr, Xf), (Xr.tolist(), dev(Xf))):
        V = losses.sliced_wasserstein_loss(a, b, directions=theta)
        assert V.grad_fn is None and not V.requires_grad and V.is_cuda and V.dtype == torch.float64
        assert abs(float(V) - want["value"]) <= RTOL * want["Lmag"]
    assert len(seen) == 3 and all(r is None for r in seen)


def test_float32_inputs_get_float32_gradients():
    Xr, Xf, theta, want = reference((65, 63, 2, 3), 2)
    A, B = dev(Xr, True, torch.float32), dev(Xf, True, torch.float32)
    L = losses.sliced_wasserstein_loss(A, B, directions=theta)
    assert L.dtype == torch.float64
    L.backward()
    assert A.grad.dtype == torch.float32 == B.grad.dtype and A.grad.shape == A.shape and B.grad.shape == B.shape
    A64, B64 = A.detach().double().requires_grad_(True), B.detach().double().requires_grad_(True)
    L64 = losses.sliced_wasserstein_loss(A64, B64, directions=theta)
    L64.backward()
    assert hygiene.same_bits(L.reshape(1), L64.reshape(1))
    assert torch.equal(A.grad, A64.grad.float()) and torch.equal(B.grad, B64.grad.float())


def test_a_transposed_view_gives_the_result_of_its_contiguous_copy():
    Xr, Xf, theta, want = reference((65, 63, 2, 3), 2)
    A, B = dev(Xr), dev(Xf, True)
    L = losses.sliced_wasserstein_loss(A, B, directions=theta)
    L.backward()
    T = B.detach().t().contiguous().requires_grad_(True)               # [d, nf]: the sample is its transposed view
    LT = losses.sliced_wasserstein_loss(A, T.t(), directions=theta)
    LT.backward()
    assert hygiene.same_bits(L.reshape(1), LT.reshape(1)) and hygiene.same_bits(T.grad.t(), B.grad)


def test_standardize_runs_as_torch_ops():
    Xr, Xf, theta, want = reference((65, 63, 2, 3), 2)
    from probaforms_amd.metrics import _boot
    A, B = dev(Xr * 3 + 1, True), dev(Xf * 3 + 1, True)
    L = losses.sliced_wasserstein_loss(A, B, directions=theta, standardize=True)
    L.backward()
    A2, B2 = dev(Xr * 3 + 1, True), dev(Xf * 3 + 1, True)
    L2 = losses.sliced_wasserstein_loss(*_boot.standardize(A2, B2), directions=theta)
    L2.backward()
    assert hygiene.same_bits(L.reshape(1), L2.reshape(1))
    assert bool(torch.isfinite(A.grad).all()) and bool(A.grad.ne(0).any())
    assert float((A.grad - A2.grad).abs().max()) <= 1e-13 * float(A2.grad.abs().max())


def test_forward_and_backward_never_wait_for_the_device(monkeypatch):
    Xr, Xf, theta, want = reference((65, 63, 2, 3), 2)
    A, th = dev(Xr), dev(theta)
    W = dev(np.concatenate([Xf, Xf], axis=1), True)
    for rows in (CAP, 0):                                            # both sort routes
        monkeypatch.setattr(losses, "_MAX_LDS_ROWS", rows)
        losses.sliced_wasserstein_loss(A, W[:, :2], directions=th).backward()       # warm-up: library, code objects, allocator
        losses.wasserstein_1d_loss(A, W[:, :2].detach())
        W.grad = None
        torch.cuda.synchronize()
        mode = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("error")
        try:
            L = losses.sliced_wasserstein_loss(A, W[:, :2], directions=th)
            (2 * L).backward()
            V = losses.sliced_wasserstein_loss(A, W[:, :2].detach(), directions=th, standardize=True, p=1)
            U = losses.wasserstein_1d_loss(A, W[:, :2].detach())
        finally:
            torch.cuda.set_sync_debug_mode(mode)
        assert bool(torch.isfinite(W.grad).all()) and bool(W.grad[:, :2].ne(0).any()) and not bool(W.grad[:, 2:].any())
        assert abs(float(L.detach()) - want["value"]) <= RTOL * want["Lmag"] and bool(torch.isfinite(V)) and bool(torch.isfinite(U))


def test_nan_propagates_into_the_value_and_the_call_returns():
    Xr, Xf = sl.make(65, 63, 3)
    Xf = Xf.copy()
    Xf[3, 2] = np.nan
    for p in (1, 2):
        B = dev(Xf, True)
        L = losses.sliced_wasserstein_loss(dev(Xr), B, p=p, directions=sl.unit_directions(4, 3))
        L.backward()
        assert bool(torch.isnan(L))


# ---- through the flow seam ---------------------------------------------------------------------------------

def test_sliced_loss_reaches_a_flows_parameters_through_its_sampler():
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
    X = torch.from_numpy(X0).cuda()
    np.random.seed(3)
    L = losses.sliced_wasserstein_loss(torch.cat([X, C], 1), torch.cat([model.nf.sample(C), C], 1))
    assert L.grad_fn is not None and bool(torch.isfinite(L))
    L.backward()
    grads = [q.grad for q in model.nf.parameters()]
    assert all(g is not None and bool(torch.isfinite(g).all()) for g in grads)
    assert any(bool(g.ne(0).any()) for g in grads)


def test_zz_largest_deviation():
    print("largest deviation seen: value %.3g Lmag, gradient %.3g M (bound %.3g for both)" % (WORST["value"], WORST["grad"], RTOL))
    print("of the crossed-axes cases: value %.3g Lmag, gradient %.3g M" % (WORST_NEW["value"], WORST_NEW["grad"]))
