"""probaforms_amd.metrics.wasserstein on the GPU (pfm_wasserstein1d / pfm_project in libpf_metrics.so) against the committed
fixtures (tests/golden/wasserstein_*.npz, made with scipy) and the float64 restatement (tests/wasserstein_numpy.py), the global
RNG state, bitwise reproducibility, CUDA-tensor inputs, the workspace check and workspace hygiene.

Tolerance: rtol 1e-12 plus atol 1e-12 (pooled max - pooled min).  A replicate is a sum of at most N float64 terms of one
sign; its worst-case rounding N 2^-53 is under 4e-13 for the largest shapes here (N = 2 500 pooled rows, 3 002 with the
two-row sample), and 1e-12 is the bar roc_auc_score_1d and anderson_darling_1d have.  The atol covers replicates near 0.
The table of a column's non-empty groups is held in LDS up to 2 048 entries: 1000 x 1500 and 3000 x 2 keep theirs in the
workspace, every other shape in LDS.
"""
import functools
import glob
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, ROOT)

import hygiene  # noqa: E402
import native_libs  # noqa: E402
import wasserstein_numpy as wn  # noqa: E402
from probaforms_amd.metrics import _boot, _lib, _m1d, wasserstein  # noqa: E402

pytestmark = pytest.mark.gpu

native_libs.ensure_built(_lib)

FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "wasserstein_*.npz")))
RTOL = 1e-12
REP_1D = wasserstein.REPLICATES["wasserstein_1d"]
REP_SLICED = wasserstein.REPLICATES["sliced_wasserstein_distance"]


def fid(p):
    return os.path.basename(p)[12:-4]


def spread(X, Y):
    return float(max(np.max(X), np.max(Y)) - min(np.min(X), np.min(Y)))


def assert_close(got, want, X, Y):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape
    err = np.abs(got - want)
    print("max |diff| %.3g, max relative %.3g" % (err.max(), (err / np.maximum(np.abs(want), 1e-300)).max()))
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=RTOL * spread(X, Y))


@pytest.mark.parametrize("path", FIXTURES, ids=fid)
def test_fixtures(path):
    f = np.load(path)
    X, Y, n_iters, p = f["X"], f["Y"], int(f["n_iters"]), int(f["p"])
    sliced = str(f["kind"]) == "sliced"
    args = (n_iters, int(f["n_projections"]), p) if sliced else (n_iters, p)
    np.random.seed(int(f["seed"]))
    S = (REP_SLICED if sliced else REP_1D)(X, Y, *args)
    assert np.random.random() == float(f["next"])
    assert_close(S, f["rep"], X, Y)
    np.random.seed(int(f["seed"]))
    mu, sd = (wasserstein.sliced_wasserstein_distance if sliced else wasserstein.wasserstein_1d)(X, Y, *args)
    assert np.random.random() == float(f["next"])                 # the public call makes the same draws
    assert isinstance(mu, np.float64) and isinstance(sd, np.float64)
    assert_close([mu, sd], [f["mean"], f["std"]], X, Y)


def _data(case):
    rng = np.random.default_rng(sum(map(ord, case)))
    if case == "ties":                    # three index groups (n_iters = 300), ties inside and across the samples
        return np.round(rng.normal(size=(40, 3)), 1), np.round(rng.normal(0.3, 1.2, size=(35, 3)), 1), 300
    if case == "chunks":                  # more tie groups than one scan chunk (1 024), nr != nf, tables in the workspace
        return rng.normal(size=(1000, 4)), rng.standard_t(4, size=(1500, 4)) * 0.8 + 0.1, 4
    if case == "coprime":
        return rng.normal(size=(257, 2)), rng.normal(0.5, 2, size=(256, 2)), 5
    if case == "equal":
        return rng.normal(size=(64, 2)), rng.normal(0.4, 1.3, size=(64, 2)), 5
    if case == "disjoint":                # every X below every Y: the merge's worst case for balance
        return rng.uniform(-3, 0, size=(600, 1)), rng.uniform(0.5, 9, size=(700, 1)), 4
    if case == "two_rows":                # interleaved supports, one sample of two rows
        return rng.normal(size=(3000, 1)), np.array([[-3.0], [4.0]]), 4
    if case == "one_row":
        return np.array([[0.5, -1.0]]), rng.normal(size=(7, 2)), 6
    if case == "constant":                # a column constant over both samples, next to an ordinary one
        X, Y = rng.normal(size=(50, 2)), rng.normal(size=(45, 2))
        X[:, 0] = 2.0
        Y[:, 0] = 2.0
        return X, Y, 5
    if case == "same":                    # X_fake = X_real: small positive replicates
        X = rng.normal(size=(100, 2))
        return X, X.copy(), 5
    raise KeyError(case)


CASES = ("ties", "chunks", "coprime", "equal", "disjoint", "two_rows", "one_row", "constant", "same")
SEED = 99


@functools.lru_cache(maxsize=None)
def restated_1d(case, p):
    X, Y, n_iters = _data(case)
    np.random.seed(SEED)
    S, nxt = wn.replicates_1d(X, Y, n_iters, p)
    S.setflags(write=False)
    return S, nxt


@pytest.mark.parametrize("p", [1, 2])
@pytest.mark.parametrize("case", CASES)
def test_wasserstein_1d_against_the_restatement(case, p):
    X, Y, n_iters = _data(case)
    want, nxt = restated_1d(case, p)
    np.random.seed(SEED)
    S = REP_1D(X, Y, n_iters, p)
    assert np.random.random() == nxt
    assert S.shape == (n_iters, X.shape[1]) and (S >= 0).all()
    assert_close(S, want, X, Y)
    if case == "constant":
        assert (S[:, 0] == 0).all()
    if case == "same":
        assert (S > 0).all()
    np.random.seed(SEED)
    mu, sd = wasserstein.wasserstein_1d(X, Y, n_iters, p=float(p))
    assert np.random.random() == nxt
    assert_close([mu, sd], wn.feature_average(want), X, Y)


def test_equal_sizes_p2_is_the_sorted_pair_formula():
    X, Y, n_iters = _data("equal")
    np.random.seed(SEED)
    S = REP_1D(X, Y, n_iters, 2)
    np.random.seed(SEED)
    want = np.empty_like(S)
    for r in range(n_iters):
        ix, iy = wn.draw(len(X), len(Y))
        for f in range(X.shape[1]):
            want[r, f] = wn.sorted_pair_w2(X[ix, f], Y[iy, f])
    assert_close(S, want, X, Y)


def test_disjoint_supports_w1_is_the_difference_of_the_means():
    X, Y, n_iters = _data("disjoint")
    np.random.seed(SEED)
    S = REP_1D(X, Y, n_iters, 1)
    np.random.seed(SEED)
    want = np.empty_like(S)
    for r in range(n_iters):
        ix, iy = wn.draw(len(X), len(Y))
        want[r, 0] = Y[iy, 0].mean() - X[ix, 0].mean()
    assert_close(S, want, X, Y)


def _sliced_data(case):
    rng = np.random.default_rng(len(case))
    if case == "d3_P130":                 # more columns than features, a multiple of nothing
        return rng.normal(size=(200, 3)), rng.normal(0.3, 1.2, size=(150, 3)), 3, 130, False
    if case == "d1_P2":
        return rng.normal(size=(90, 1)), rng.normal(0.5, 1, size=(70, 1)), 5, 2, False
    if case == "standardize":             # a feature that is constant over the real sample (its std of 0 becomes 1)
        X, Y = rng.normal(1.0, 3.0, size=(120, 3)), rng.normal(1.5, 2.0, size=(100, 3))
        X[:, 1] = 2.0
        return X, Y, 4, 17, True
    raise KeyError(case)


SLICED = ("d3_P130", "d1_P2", "standardize")


@functools.lru_cache(maxsize=None)
def restated_sliced(case, p):
    X, Y, n_iters, P, std = _sliced_data(case)
    np.random.seed(SEED)
    S, nxt = wn.replicates_sliced(X, Y, n_iters, P, p, std)
    S.setflags(write=False)
    return S, nxt


@pytest.mark.parametrize("p", [1, 2])
@pytest.mark.parametrize("case", SLICED)
def test_sliced_against_the_restatement(case, p):
    X, Y, n_iters, P, std = _sliced_data(case)
    want, nxt = restated_sliced(case, p)
    np.random.seed(SEED)
    S = REP_SLICED(X, Y, n_iters, P, p, std)
    assert np.random.random() == nxt
    assert S.shape == (n_iters,)
    Xs, Ys = wn.standardize(X, Y) if std else (X, Y)
    assert_close(S, want, Xs, Ys)
    np.random.seed(SEED)
    mu, sd = wasserstein.sliced_wasserstein_distance(X, Y, n_iters, n_projections=P, p=p, standardize=std)
    assert np.random.random() == nxt
    assert_close([mu, sd], [want.mean(), want.std()], Xs, Ys)


def test_sliced_defaults():
    X, Y, _, _, _ = _sliced_data("d3_P130")
    X, Y = X[:50], Y[:40]
    np.random.seed(SEED)
    want, nxt = wn.replicates_sliced(X, Y, 100, 64, 2, False)
    np.random.seed(SEED)
    mu, sd = wasserstein.sliced_wasserstein_distance(X, Y)
    assert np.random.random() == nxt
    assert_close([mu, sd], [want.mean(), want.std()], X, Y)


@pytest.mark.parametrize("nr,nf,d,P", [(200, 150, 3, 130), (90, 70, 1, 2), (1, 2, 5, 1), (700, 900, 16, 7)])
def test_projection_is_bitwise_the_feature_order_loop(nr, nf, d, P):
    rng = np.random.default_rng(P)
    X, Y, th = rng.normal(size=(nr, d)), rng.normal(size=(nf, d)), rng.normal(size=(P, d))
    cols = torch.full((P, nr + nf), float("nan"), dtype=torch.float64, device="cuda")
    _lib.project(torch.from_numpy(X).cuda(), torch.from_numpy(Y).cuda(), torch.from_numpy(th).cuda(), cols)
    want = np.stack([np.concatenate([wn.project(X, t), wn.project(Y, t)]) for t in th])
    assert np.array_equal(cols.cpu().numpy(), want)
    p = _m1d.Pooled.from_columns(cols, nr)
    assert (p.nr, p.nf, p.d) == (nr, nf, P) and p.cols.data_ptr() == cols.data_ptr()


def test_pooled_from_columns_equals_pooled_of_the_samples():
    rng = np.random.default_rng(8)
    Xr, Xf = torch.from_numpy(np.round(rng.normal(size=(30, 3)), 1)).cuda(), torch.from_numpy(np.round(rng.normal(size=(20, 3)), 1)).cuda()
    a = _m1d.Pooled(Xr, Xf)
    b = _m1d.Pooled.from_columns(torch.cat([Xr, Xf]).t().contiguous(), 30)
    assert (a.nr, a.nf, a.d, a.device) == (b.nr, b.nf, b.d, b.device)
    for name in ("cols", "perm", "gstart", "ngroups"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name


CALLS = {
    "wasserstein_1d-p1": lambda X, Y: wasserstein.wasserstein_1d(X, Y, 20, p=1),
    "wasserstein_1d-p2": lambda X, Y: wasserstein.wasserstein_1d(X, Y, 20, p=2),
    "sliced-p1": lambda X, Y: wasserstein.sliced_wasserstein_distance(X, Y, 20, n_projections=9, p=1),
    "sliced-p2-std": lambda X, Y: wasserstein.sliced_wasserstein_distance(X, Y, 20, n_projections=9, standardize=True),
}


@pytest.mark.parametrize("name", list(CALLS))
def test_same_seed_is_bitwise_identical(name):
    rng = np.random.default_rng(3)
    X, Y = rng.normal(size=(1200, 3)), rng.normal(0.2, 1, size=(1000, 3))        # (the 1-D p = 2 tables are in the workspace)
    outs = []
    for _ in range(2):
        np.random.seed(17)
        outs.append(CALLS[name](X, Y))
    assert outs[0][0].tobytes() == outs[1][0].tobytes() and outs[0][1].tobytes() == outs[1][1].tobytes()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("name", list(CALLS))
def test_cuda_tensor_inputs(name, dtype):
    rng = np.random.default_rng(11)
    X = torch.from_numpy(rng.normal(size=(200, 2))).to(dtype)
    Y = torch.from_numpy(rng.normal(0.5, 1, size=(150, 2))).to(dtype)
    np.random.seed(4)
    want = CALLS[name](X.double().numpy(), Y.double().numpy())
    np.random.seed(4)
    got = CALLS[name](X.cuda(), Y.cuda())
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()


def test_nonfinite_cuda_tensor_raises():
    X = torch.zeros(5, 2, device="cuda")
    X[2, 0] = float("inf")
    with pytest.raises(ValueError):
        wasserstein.wasserstein_1d(X, torch.zeros(4, 2, device="cuda"))
    with pytest.raises(ValueError):
        wasserstein.sliced_wasserstein_distance(X, torch.zeros(4, 2, device="cuda"))


def _boot_case(nr, nf, d, reps, seed):
    """data and the reference's bootstrap draws for `reps` replicates, on the host and on the device"""
    rng = np.random.default_rng(seed)
    X = np.round(rng.normal(size=(nr, d)), 2)
    Y = np.round(rng.normal(0.3, 1.2, size=(nf, d)), 2)
    np.random.seed(seed)
    host = np.empty(reps * (nr + nf), np.int32)
    _boot.draw_indices(host, reps, nr, nf)
    ix, iy = host[:reps * nr].reshape(reps, nr), host[reps * nr:].reshape(reps, nf)
    return X, Y, ix, iy, torch.from_numpy(ix.reshape(-1).copy()).cuda(), torch.from_numpy(iy.reshape(-1).copy()).cuda()


def _raw(p, X, Y, ixd, iyd, reps, ws):
    """pfm_wasserstein1d through the raw binding on a poisoned output -> (status, out [reps, d])"""
    pooled = _m1d.Pooled(torch.from_numpy(X).cuda(), torch.from_numpy(Y).cuda())
    out = torch.empty((reps, pooled.d), dtype=torch.float64, device="cuda")
    hygiene.poison_outputs(out)
    st = _lib.wasserstein1d_status(p, pooled.cols, pooled.perm, pooled.gstart, pooled.ngroups, pooled.nr, pooled.nf, ixd, iyd, reps,
                                   out, ws)
    torch.cuda.synchronize()
    return st, out


@pytest.mark.parametrize("nr,nf", [(30, 20), (1000, 1500)], ids=["lds", "workspace"])
@pytest.mark.parametrize("p", [1, 2])
def test_too_small_workspace_is_refused(p, nr, nf):
    reps, d = 2, 2
    X, Y, _, _, ixd, iyd = _boot_case(nr, nf, d, reps, 1)
    need = _lib.wasserstein1d_workspace_bytes(nr, nf, d, reps, p)
    assert need > 0
    st, out = _raw(p, X, Y, ixd, iyd, reps, torch.empty(need - 1, dtype=torch.uint8, device="cuda"))
    assert st == _lib.PFM_EWORKSPACE and hygiene.poisoned(out) == out.numel()
    st, out = _raw(p, X, Y, ixd, iyd, reps, torch.empty(need, dtype=torch.uint8, device="cuda"))
    assert st == 0 and hygiene.poisoned(out) == 0


# (rows real, rows fake, features, replicates): the last one keeps its p = 2 tables in the workspace
HYGIENE_SIZES = [(50, 51, 3, 5), (1, 2, 2, 4), (1000, 1500, 4, 3)]


@pytest.mark.parametrize("nr,nf,d,reps", HYGIENE_SIZES)
@pytest.mark.parametrize("p", [1, 2])
def test_results_do_not_depend_on_the_workspace(p, nr, nf, d, reps):
    X, Y, ix, iy, ixd, iyd = _boot_case(nr, nf, d, reps, 11)
    pr = (nr + 20, nf + 30, d, reps + 2)                          # the `replay` primer: more replicates and more rows
    PX, PY, _, _, pixd, piyd = _boot_case(*pr, 12)
    nbytes, pbytes = _lib.wasserstein1d_workspace_bytes(nr, nf, d, reps, p), _lib.wasserstein1d_workspace_bytes(*pr, p)
    outs = {}
    for pat in hygiene.PATTERNS:
        ws = hygiene.workspace(pbytes if pat == "replay" else nbytes, pat)
        if pat == "replay":
            assert _raw(p, PX, PY, pixd, piyd, pr[3], ws)[0] == 0
        st, out = _raw(p, X, Y, ixd, iyd, reps, ws)
        assert st == 0
        outs[pat] = dict(out=out)
    hygiene.assert_all_written(outs["zeros"], "pfm_wasserstein1d[p=%d]" % p)
    hygiene.assert_pattern_independent(outs, "pfm_wasserstein1d[p=%d]" % p)
    want = np.empty((reps, d))
    for r in range(reps):
        for f in range(d):
            want[r, f] = wn.wp_pow(X[ix[r], f], Y[iy[r], f], p)
    got = outs["zeros"]["out"].cpu().numpy()                      # W_p^p: the bar scales with the spread to the p
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=RTOL * spread(X, Y) ** p)
