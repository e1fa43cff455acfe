"""pfm_sym_eig, pfm_frechet_grad, losses.frechet_loss and fd.frechet_distance_full_sample on the GPU against the float64 numpy
restatement (tests/frechet_numpy.py), np.linalg.eigh, the reference's own replicates (tests/golden/metrics_*.npz), pfm_boot_moments
(bitwise) and torch.autograd.gradcheck.  The write-bounds and stream drivers run in tests/test_streams_frechet_gpu.py.

pfm_sym_eig.  max|w - eigvalsh|, max|A V - V diag(w)| <= C d 2^-53 |A|_2 and max|V^T V - I| <= C d 2^-53.  C is not chosen: it is
8 times the largest of numpy's own residual and orthogonality defect, in the same units, over the same matrices on the CPU (floor 1),
computed at import.  With the LAPACK of the numpy this was written against the largest of numpy's figures is 1.72, C = 13.8;
MEASURED_EIG below holds the GPU's worst figures in those units.

pfm_frechet_grad.  Values and parts within 1e-12 of |dmu|^2 + tr C_r + tr C_f, every gradient element within 1e-12 of the largest
gradient element of its sample: the project's convention for the losses, about 100 times the deviation of the restatement's two CPU
routes from each other (tests/test_frechet_host.py).  MEASURED_GRAD below holds the GPU's worst figures.
Singular inputs (rcond = 1e-10): the restatement's eigenvalues are asserted to lie above 1e-6 lambda_max or below 1e-13 lambda_max,
so both implementations cut the same ones and rank is compared with ==; the kept spectrum then has lambda_max / lambda <= 1e6 and
the gradient is held within 1e-9 of its largest element; the value within 4 d sqrt(d 2^-53 lambda_max) of the restatement's (Weyl's
bound on the eigenvalues of rounding noise, d 2^-53 lambda_max each, through the square root, on both sides, twice in FD).

MEASURED_EIG:  eigenvalues 1.00, residual 0.87, orthogonality 3.25 (in units of d 2^-53 |A|_2 and d 2^-53), at most 9 sweeps
               (8 at d = 64; 9 for the rank-3 matrix at d = 16)
MEASURED_GRAD: values and parts 6.3e-15 of the scale, gradients 3.8e-14 of their largest element (both at 300 + 260 rows, d = 64);
               singular inputs: gradients 2.6e-15, values 2.3e-8 under a bound of 3.0e-6 (n <= d) and 1.4e-8 under 6.1e-7
"""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import frechet_numpy as fr  # noqa: E402
import hygiene  # noqa: E402
import native_libs  # noqa: E402
from test_frechet_host import FD_FIXTURES, fixture_rows  # noqa: E402
from probaforms_amd.metrics import _lib, fd, losses  # noqa: E402

pytestmark = pytest.mark.gpu

native_libs.ensure_built(_lib)

F64, I32 = torch.float64, torch.int32
U53 = 2.0 ** -53
EIG_DS = (1, 2, 3, 7, 16, 17, 32, 33, 63, 64)
SHAPES = ((2, 2, 1), (2, 3, 1), (5, 4, 2), (37, 53, 3), (40, 33, 5), (64, 40, 16), (90, 70, 17), (150, 131, 33), (300, 260, 64),
          (5000, 4100, 16))
TOL = 1e-12


def dev(a, dtype=F64):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


# ---- pfm_sym_eig ---------------------------------------------------------------------------------------------------------

def eig_matrices(d):
    """{name: symmetric [d, d]}: a covariance, a diagonal matrix, c I, an indefinite matrix, the zero matrix, and at d = 16 a
    rank-3 positive semi-definite one; at d = 2 the indefinite matrix is [[0, 1], [1, 0]]"""
    rng = np.random.RandomState(100 + d)
    X = rng.normal(size=(3 * d + 5, d)) @ (np.eye(d) + 0.3 * rng.normal(size=(d, d)) / np.sqrt(d))
    B = rng.normal(size=(d, d))
    m = dict(cov=np.cov(X, rowvar=False).reshape(d, d), diag=np.diag(rng.normal(size=d)), cI=2.5 * np.eye(d),
             indef=np.array([[0.0, 1.0], [1.0, 0.0]]) if d == 2 else (B + B.T) * 0.5, zero=np.zeros((d, d)))
    if d == 16:
        R = rng.normal(size=(d, 3))
        m["rank3"] = R @ R.T
    return m


def defects(A, w, V, ref):
    """(eigenvalue error, residual, orthogonality defect) in units of d 2^-53 |A|_2 (the last: d 2^-53); 0 for a zero quantity"""
    d = A.shape[0]
    unit, nrm = d * U53, np.linalg.norm(A, 2)
    e = [np.abs(w - ref).max(), np.abs(A @ V - V * w[None, :]).max()]
    return [0.0 if x == 0 else x / (unit * nrm) for x in e] + [np.abs(V.T @ V - np.eye(d)).max() / unit]


def numpy_constant():
    worst = 1.0 / 8
    for d in EIG_DS:
        for A in eig_matrices(d).values():
            w, V = np.linalg.eigh(A)
            worst = max([worst] + defects(A, w, V, w)[1:])
    return 8.0 * worst


C_EIG = numpy_constant()


def run_eig(As, with_v=True):
    A = dev(np.stack(As))
    b, d = A.shape[0], A.shape[1]
    w, V = torch.empty(b, d, dtype=F64, device="cuda"), torch.empty(b, d, d, dtype=F64, device="cuda") if with_v else None
    sweeps = torch.empty(b, dtype=I32, device="cuda")
    hygiene.poison_outputs(w, V, sweeps)
    _lib.sym_eig(A, w, V, sweeps, hygiene.workspace(_lib.sym_eig_workspace_bytes(b, d), "ones"))
    return w, V, sweeps


@pytest.mark.parametrize("d", EIG_DS)
def test_sym_eig_against_numpy(d):
    mats = eig_matrices(d)
    names = list(mats)
    w, V, sweeps = run_eig([mats[k] for k in names[:5]])
    assert w.shape[0] == 5
    extra = run_eig([mats["rank3"]]) if "rank3" in mats else None
    worst = [0.0, 0.0, 0.0]
    for i, name in enumerate(names):
        if i < 5:
            wi, Vi, si = w[i], V[i], int(sweeps[i])
        else:
            wi, Vi, si = extra[0][0], extra[1][0], int(extra[2][0])
        A = mats[name]
        wn, Vn = wi.cpu().numpy(), Vi.cpu().numpy()
        assert np.isfinite(wn).all() and np.isfinite(Vn).all() and (np.diff(wn) >= 0).all(), name
        got = defects(A, wn, Vn, np.linalg.eigvalsh(A))
        worst = [max(a, b) for a, b in zip(worst, got)]
        print("sym_eig d=%d %-6s sweeps %2d  eigenvalues %.2f residual %.2f orthogonality %.2f (C = %.1f)" % ((d, name, si) + tuple(got) + (C_EIG,)))
        assert max(got) <= C_EIG, (name, got, C_EIG)
        assert 0 <= si < _lib.EIG_MAX_SWEEPS and (si <= 1 if name in ("diag", "cI", "zero") else True), (name, si)
        # alone: the same bits as in the batch
        w1, V1, s1 = run_eig([A])
        assert hygiene.same_bits(w1[0], wi) and hygiene.same_bits(V1[0], Vi) and int(s1[0]) == si, name
    if d == 2:
        assert np.allclose(w[names.index("indef")].cpu().numpy(), [-1.0, 1.0], rtol=0, atol=4 * U53)
    if d == 16:
        assert (np.abs(extra[0][0].cpu().numpy()[:13]) <= C_EIG * d * U53 * np.linalg.norm(mats["rank3"], 2)).all()


@pytest.mark.parametrize("d", (2, 17, 64))
def test_sym_eig_reads_the_lower_triangle_contains_a_nan_and_repeats(d):
    mats = eig_matrices(d)
    A, B = mats["cov"], mats["indef"]
    w, V, s = run_eig([A, B])
    up = np.triu(np.ones((d, d), dtype=bool), 1)
    An, Bn = A.copy(), B.copy()
    An[up], Bn[up] = np.nan, np.nan
    w2, V2, s2 = run_eig([An, Bn])
    assert hygiene.same_bits(w, w2) and hygiene.same_bits(V, V2) and torch.equal(s, s2)
    # a matrix of NaN between two others: NaN for it alone, the loop ends at its bound, the others keep their bits
    w3, V3, s3 = run_eig([A, np.full((d, d), np.nan), B])
    assert bool(torch.isnan(w3[1]).all()) and bool(torch.isnan(V3[1]).all()) and int(s3[1]) == _lib.EIG_MAX_SWEEPS
    for i, j in ((0, 0), (2, 1)):
        assert hygiene.same_bits(w3[i], w[j]) and hygiene.same_bits(V3[i], V[j]) and int(s3[i]) == int(s[j])
    # a second call gives the same bytes; the eigenvalues alone are the same eigenvalues
    w4, V4, s4 = run_eig([A, B])
    assert hygiene.same_bits(w, w4) and hygiene.same_bits(V, V4) and torch.equal(s, s4)
    assert hygiene.same_bits(run_eig([A, B], with_v=False)[0], w)


# ---- pfm_frechet_grad ----------------------------------------------------------------------------------------------------

def run_grad(Xr, Xf, rcond=None, sides=3, want_grad=True, fill="ones"):
    """-> dict(value, grad, parts, eig, rank, mean, cov) of one direct call, numpy"""
    Z = dev(np.concatenate([Xr, Xf], axis=0))
    n, d = Z.shape
    nr = Xr.shape[0]
    value, parts = torch.empty(1, dtype=F64, device="cuda"), torch.empty(5, dtype=F64, device="cuda")
    grad = torch.empty(n, d, dtype=F64, device="cuda") if want_grad else None
    eig, rank = torch.empty(d, dtype=F64, device="cuda"), torch.empty(2, dtype=I32, device="cuda")
    hygiene.poison_outputs(value, parts, grad, eig, rank)
    ws = hygiene.workspace(_lib.frechet_grad_workspace_bytes(n, d, nr), fill)
    _lib.frechet_grad(Z, nr, d * 2.0 ** -52 if rcond is None else rcond, sides, value, grad, parts, eig, rank, ws)
    mean, cov = _lib.frechet_moments(ws, d)
    out = dict(value=value, grad=grad, parts=parts, eig=eig, rank=rank, mean=mean, cov=cov)
    return {k: None if v is None else v.cpu().numpy().copy() for k, v in out.items()}


_restated = {}


def restated(shape):
    if shape not in _restated:
        Xr, Xf = fr.data(*shape)
        _restated[shape] = (Xr, Xf, fr.value_grad(Xr, Xf))
    return _restated[shape]


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_frechet_grad_against_the_restatement(shape):
    nr, nf, d = shape
    Xr, Xf, ref = restated(shape)
    assert ref["eig"][-1] / ref["eig"][0] <= 100 and ref["eig_swapped"][-1] / ref["eig_swapped"][0] <= 100
    got = run_grad(Xr, Xf)
    ev = np.abs(got["parts"] - ref["parts"]).max() / ref["scale"]
    eg = max(np.abs(got["grad"][:nr] - ref["grad_r"]).max() / np.abs(ref["grad_r"]).max(),
             np.abs(got["grad"][nr:] - ref["grad_f"]).max() / np.abs(ref["grad_f"]).max())
    print("frechet_grad %s: value and parts off by %.3g of the scale, gradients by %.3g of their largest element" % (shape, ev, eg))
    assert got["value"][0] == got["parts"][0] and ev <= TOL and eg <= TOL
    assert np.abs(got["eig"] - ref["eig"]).max() <= TOL * ref["eig"][-1] and got["rank"].tolist() == [d, d]
    if d == 1:
        want = (Xr.mean() - Xf.mean()) ** 2 + (Xr.std(ddof=1) - Xf.std(ddof=1)) ** 2
        assert abs(got["value"][0] - want) <= TOL * ref["scale"]
    # the moments are pfm_boot_moments' for identity indices, bitwise
    A, B = dev(Xr), dev(Xf)
    mean, cov = torch.empty(1, 2, d, dtype=F64, device="cuda"), torch.empty(1, 2, d, d, dtype=F64, device="cuda")
    ia, ib = torch.arange(nr, dtype=I32, device="cuda"), torch.arange(nf, dtype=I32, device="cuda")
    _lib.boot_moments(A, B, ia, ib, 1, mean, cov, hygiene.workspace(_lib.moments_workspace_bytes(nr, nf, d, 1), "zeros"))
    assert np.array_equal(mean[0].cpu().numpy(), got["mean"]) and np.array_equal(cov[0].cpu().numpy(), got["cov"])
    assert got["parts"][2] == sum(got["cov"][0, k, k] for k in range(d)) and got["parts"][3] == sum(got["cov"][1, k, k] for k in range(d))
    # two calls, two workspaces: the same bytes; the value alone is the same value
    again = run_grad(Xr, Xf, fill="huge")
    for k in ("value", "grad", "parts", "eig", "rank"):
        assert got[k].tobytes() == again[k].tobytes(), k
    alone = run_grad(Xr, Xf, want_grad=False, sides=0)
    assert alone["parts"].tobytes() == got["parts"].tobytes() and alone["rank"].tolist() == [d, -1]


def test_sides_choose_the_routes_and_the_rows():
    nr, nf, d = 40, 33, 5
    Xr, Xf, _ = restated((nr, nf, d))
    both, fake, real = (run_grad(Xr, Xf, sides=s) for s in (3, 2, 1))
    assert fake["rank"].tolist() == [d, -1] and real["rank"].tolist() == [d, d]
    assert np.array_equal(fake["grad"][nr:], both["grad"][nr:]) and not fake["grad"][:nr].any()
    assert np.array_equal(real["grad"][:nr], both["grad"][:nr]) and not real["grad"][nr:].any()
    assert fake["parts"].tobytes() == both["parts"].tobytes() == real["parts"].tobytes()


def test_equal_samples():
    Xr, _ = fr.data(150, 150, 33)
    got = run_grad(Xr, Xr.copy())
    tr = got["parts"][2]
    assert abs(got["value"][0]) <= TOL * tr and np.abs(got["grad"]).max() <= TOL
    v = fd.frechet_distance_full_sample(Xr, Xr.copy())
    assert isinstance(v, np.float64) and abs(v) <= TOL * tr


def singular_cases():
    Xr, Xf = fr.data(4, 6, 8)
    yield "n <= d", Xr, Xf
    Xr, Xf = fr.data(40, 33, 5)
    Xr = Xr.copy()
    Xr[:, 2] = 1.5
    yield "constant column", Xr, Xf
    Xr, _ = fr.data(9, 4, 3)
    yield "equal rows", Xr, np.tile(np.array([[0.5, -1.25, 3.0]]), (4, 1))


@pytest.mark.parametrize("case", list(singular_cases()), ids=lambda c: c[0])
def test_singular_inputs(case):
    name, Xr, Xf = case
    nr, d = Xr.shape
    rcond = 1e-10
    ref = fr.value_grad(Xr, Xf, rcond=rcond)
    for lam in (ref["eig"], ref["eig_swapped"]):                 # a gap: both implementations cut the same eigenvalues
        assert ((lam > 1e-6 * lam[-1]) | (lam <= 1e-13 * abs(lam[-1]))).all(), lam
    got = run_grad(Xr, Xf, rcond=rcond)
    assert got["rank"].tolist() == ref["rank"].tolist() and max(ref["rank"]) < d
    assert np.isfinite(got["grad"]).all()
    eg = max(np.abs(got["grad"][:nr] - ref["grad_r"]).max() / np.abs(ref["grad_r"]).max(),
             np.abs(got["grad"][nr:] - ref["grad_f"]).max() / np.abs(ref["grad_f"]).max())
    lmax = max(ref["eig"][-1], 0.0)
    bound = 4 * d * np.sqrt(d * U53 * lmax)
    print("singular %s: ranks %s, gradient off by %.3g of its largest element, value off by %.3g (bound %.3g)"
          % (name, got["rank"].tolist(), eg, abs(got["value"][0] - ref["value"]), bound))
    assert eg <= 1e-9
    # the bound is the trace term's (it enters FD twice); the other parts are sums of the moments and keep the bound of the values
    assert 2 * abs(got["parts"][4] - ref["parts"][4]) <= bound and np.abs(got["parts"][1:4] - ref["parts"][1:4]).max() <= TOL * ref["scale"]
    assert abs(got["value"][0] - ref["value"]) <= bound + TOL * ref["scale"]
    if name == "equal rows":
        assert got["rank"].tolist() == [0, 0]
        # G = I: the gradient is the mean term plus 2 / (n - 1) (z - mu)
        want = fr.row_gradient(Xr, ref["mean"][0], ref["mean"][1], np.eye(d))
        assert np.abs(got["grad"][:nr] - want).max() <= TOL * np.abs(want).max()


@pytest.mark.parametrize("path", FD_FIXTURES, ids=lambda p: os.path.basename(p)[8:-4])
def test_full_sample_reproduces_the_references_replicates(path):
    f, rows = fixture_rows(path, 5)
    got = np.array([fd.frechet_distance_full_sample(a, b) for a, b in rows])
    np.testing.assert_allclose(got, f["fd_rep"][:len(rows)], rtol=1e-9, atol=1e-13)
    lam = np.concatenate([fr.value_grad(a, b)["eig"] / fr.value_grad(a, b)["eig"][-1] for a, b in rows[:2]])
    assert lam.min() > 1e-5


# ---- the public calls ----------------------------------------------------------------------------------------------------

def test_frechet_loss_gradcheck_and_dtypes():
    Xr, Xf = fr.data(7, 6, 3)
    a, b = dev(Xr).requires_grad_(), dev(Xf).requires_grad_()
    assert torch.autograd.gradcheck(lambda x, y: losses.frechet_loss(x, y), (a, b))
    L = losses.frechet_loss(a, b)
    assert L.dtype == F64 and L.dim() == 0 and L.is_cuda and L.grad_fn is not None
    ref = fr.value_grad(Xr, Xf)
    assert abs(float(L.detach()) - ref["value"]) <= TOL * ref["scale"]
    assert float(L.detach()) == fd.frechet_distance_full_sample(Xr, Xf)
    # float32 inputs get float32 gradients; numpy inputs give a value without a grad_fn
    a32, b32 = dev(Xr, torch.float32).requires_grad_(), dev(Xf, torch.float32).requires_grad_()
    losses.frechet_loss(a32, b32).backward()
    assert a32.grad.dtype == torch.float32 and b32.grad.dtype == torch.float32 and a32.grad.shape == a32.shape
    ref32 = fr.value_grad(Xr.astype(np.float32).astype(np.float64), Xf.astype(np.float32).astype(np.float64))
    assert np.abs(b32.grad.cpu().numpy() - ref32["grad_f"]).max() <= 2.0 ** -22 * np.abs(ref32["grad_f"]).max()
    plain = losses.frechet_loss(Xr, Xf)
    assert plain.grad_fn is None and float(plain) == float(L.detach())


def test_one_side_runs_one_route(monkeypatch):
    Xr, Xf, ref = restated((40, 33, 5))
    seen = []
    original = _lib.frechet_grad
    monkeypatch.setattr(_lib, "frechet_grad", lambda *a: seen.append((a[3], a[8])) or original(*a))
    a, b = dev(Xr), dev(Xf).requires_grad_()
    L, rank = losses.frechet_loss(a, b, return_rank=True)
    L.backward()
    assert a.grad is None and [s for s, _ in seen] == [2]
    torch.cuda.synchronize()
    assert seen[0][1].tolist() == [5, -1]                        # the swapped route was not run
    assert np.abs(b.grad.cpu().numpy() - ref["grad_f"]).max() <= TOL * np.abs(ref["grad_f"]).max()
    assert rank.dtype == I32 and rank.dim() == 0 and rank.grad_fn is None and not rank.requires_grad and int(rank) == 5
    a2 = dev(Xr).requires_grad_()
    losses.frechet_loss(a2, dev(Xf)).backward()
    assert [s for s, _ in seen] == [2, 1]
    assert np.abs(a2.grad.cpu().numpy() - ref["grad_r"]).max() <= TOL * np.abs(ref["grad_r"]).max()


def test_standardize_and_scaling_of_the_incoming_gradient():
    Xr, Xf = fr.data(64, 40, 16)
    Sr, Sf = fr.standardized(Xr, Xf)
    ref = fr.value_grad(Sr, Sf)
    got = losses.frechet_loss(Xr, Xf, standardize=True)
    hand = losses.frechet_loss(Sr, Sf)
    assert abs(float(got) - float(hand)) <= TOL * ref["scale"] and abs(float(got) - ref["value"]) <= TOL * ref["scale"]
    assert abs(fd.frechet_distance_full_sample(Xr, Xf, standardize=True) - ref["value"]) <= TOL * ref["scale"]
    b = dev(Sf).requires_grad_()
    (3.0 * losses.frechet_loss(dev(Sr), b)).backward()
    assert np.abs(b.grad.cpu().numpy() - 3.0 * ref["grad_f"]).max() <= 3.0 * TOL * np.abs(ref["grad_f"]).max()


def test_forward_and_backward_only_enqueue():
    Xr, Xf = fr.data(90, 70, 17)
    a, b = dev(Xr).requires_grad_(), dev(Xf).requires_grad_()
    losses.frechet_loss(a, b).backward()                          # the one-time setup of the kernels
    a.grad = b.grad = None
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        L, rank = losses.frechet_loss(a, b, return_rank=True)
        L.backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    ref = fr.value_grad(Xr, Xf)
    assert int(rank) == 17 and np.abs(a.grad.cpu().numpy() - ref["grad_r"]).max() <= TOL * np.abs(ref["grad_r"]).max()


def test_a_nan_reaches_the_value_and_every_gradient_element():
    Xr, Xf = fr.data(40, 33, 5)
    for side in (0, 1):
        A, B = Xr.copy(), Xf.copy()
        (A if side == 0 else B)[3, 2] = np.nan
        a, b = dev(A).requires_grad_(), dev(B).requires_grad_()
        L = losses.frechet_loss(a, b)
        L.backward()
        assert bool(torch.isnan(L)) and bool(torch.isnan(a.grad).all()) and bool(torch.isnan(b.grad).all()), side
    # no fault left behind: the next call on the device runs
    assert np.isfinite(fd.frechet_distance_full_sample(Xr, Xf))
