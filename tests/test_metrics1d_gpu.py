"""The eight 1-D metrics on the GPU (pfm_metric1d in libpf_metrics.so) against the reference's committed fixtures
(tests/golden/metrics1d_*.npz), the float64 restatement (tests/metrics1d_numpy.py) on shapes the fixtures do not
cover, the global RNG state, bitwise reproducibility, CUDA-tensor inputs, the raising cases and the workspace check."""
import glob
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, ROOT)

import metrics1d_numpy as m1  # noqa: E402
import native_libs  # noqa: E402
from probaforms_amd.metrics import _lib, _m1d, div1d, ks1d  # noqa: E402

pytestmark = pytest.mark.gpu

native_libs.ensure_built(_lib)

FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "metrics1d_*.npz")))
NAMES = tuple(m1.FUNCS)
BITWISE = ("kolmogorov_smirnov_1d", "cramer_von_mises_1d", "kullback_leibler_1d", "jensen_shannon_1d")
RTOL = {"roc_auc_score_1d": 1e-12, "anderson_darling_1d": 1e-12, "kullback_leibler_1d_kde": 1e-9,
        "jensen_shannon_1d_kde": 1e-9}


def module(name):
    return ks1d if name in ks1d.REPLICATES else div1d


def public(name):
    return getattr(module(name), name)


def fid(p):
    return os.path.basename(p)[10:-4]


def cases(raising):
    out = []
    for p in FIXTURES:
        f = np.load(p)
        for m in NAMES:
            if (m + "_raises") in f.files and bool(f[m + "_raises"]) == raising:
                out.append(pytest.param(p, m, id="%s-%s" % (fid(p), m)))
    return out


def extra(f, name):
    return (int(f[m1.BINS[name]]),) if name in m1.BINS else ()


def assert_close(got, want, name):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    if name in BITWISE:
        assert np.array_equal(got[ok], want[ok]), np.abs(got[ok] - want[ok]).max()
    else:
        np.testing.assert_allclose(got[ok], want[ok], rtol=RTOL[name], atol=0)


@pytest.mark.parametrize("path,name", cases(False))
def test_replicates_match_the_reference(path, name):
    f = np.load(path)
    np.random.seed(int(f["seed"]))
    S = module(name).REPLICATES[name](f["X"], f["Y"], int(f["n_iters"]), *extra(f, name))
    assert_close(S, f[name + "_rep"], name)


@pytest.mark.parametrize("path,name", cases(False))
def test_public_call_matches_the_reference(path, name):
    f = np.load(path)
    np.random.seed(int(f["seed"]))
    mu, sd = public(name)(f["X"], f["Y"], int(f["n_iters"]), *extra(f, name))
    assert np.random.random() == float(f[name + "_next"])        # the generator stands where the reference left it
    assert isinstance(mu, np.float64) and isinstance(sd, np.float64)
    assert_close([mu, sd], [f[name + "_mean"], f[name + "_std"]], name)


@pytest.mark.parametrize("path,name", cases(True))
def test_raising_cases_raise_and_the_device_stays_usable(path, name):
    f = np.load(path)
    np.random.seed(int(f["seed"]))
    with pytest.raises(ValueError):
        public(name)(f["X"], f["Y"], int(f["n_iters"]), *extra(f, name))
    np.random.seed(0)
    mu, _ = public(name)(np.arange(12.0).reshape(6, 2), np.arange(12.0).reshape(6, 2) + 0.5, n_iters=3)
    assert np.isfinite(mu)


def restated(name, X, Y, seed, n_iters, bins):
    np.random.seed(seed)
    with np.errstate(all="ignore"):
        return m1.replicates(name, X, Y, n_iters, bins)


def replicates(name, X, Y, n_iters, bins):
    return module(name).REPLICATES[name](X, Y, n_iters, *(() if bins is None else (bins,)))


@pytest.mark.parametrize("name", NAMES)
def test_more_replicates_than_one_group_against_the_restatement(name):
    """n_iters = 300 runs as three index groups (at most 128 replicates each)"""
    rng = np.random.default_rng(7)
    X = np.round(rng.normal(size=(40, 3)), 1)
    Y = np.round(rng.normal(0.3, 1.2, size=(35, 3)), 1)
    bins = 7 if name in m1.BINS else None
    np.random.seed(99)
    S = replicates(name, X, Y, 300, bins)
    after = np.random.random()
    want = restated(name, X, Y, 99, 300, bins)
    assert np.random.random() == after
    assert_close(S, want, name)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("shape", [(1000, 1500, 4), (3000, 2, 1)], ids=["1000x1500x4", "3000x2x1"])
def test_larger_shapes_against_the_restatement(name, shape):
    nr, nf, d = shape
    rng = np.random.default_rng(nr + d)
    X = rng.normal(size=(nr, d))
    Y = rng.standard_t(4, size=(nf, d)) * 0.8 + 0.1 if nf > 2 else np.array([[-3.0], [4.0]])
    # 3000 histogram bins count in global memory rather than LDS
    bins = {"kullback_leibler_1d": 10, "jensen_shannon_1d": 3000, "kullback_leibler_1d_kde": 101,
            "jensen_shannon_1d_kde": 64}.get(name)
    np.random.seed(5)
    S = replicates(name, X, Y, 4, bins)
    assert_close(S, restated(name, X, Y, 5, 4, bins), name)


@pytest.mark.parametrize("name", NAMES)
def test_same_seed_is_bitwise_identical(name):
    rng = np.random.default_rng(3)
    X, Y = rng.normal(size=(500, 3)), rng.normal(0.2, 1, size=(400, 3))
    outs = []
    for _ in range(2):
        np.random.seed(17)
        outs.append(public(name)(X, Y, 20))
    assert outs[0][0].tobytes() == outs[1][0].tobytes() and outs[0][1].tobytes() == outs[1][1].tobytes()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("name", NAMES)
def test_cuda_tensor_inputs(name, dtype):
    rng = np.random.default_rng(11)
    X = torch.from_numpy(rng.normal(size=(200, 2))).to(dtype)
    Y = torch.from_numpy(rng.normal(0.5, 1, size=(150, 2))).to(dtype)
    np.random.seed(4)
    want = public(name)(X.double().numpy(), Y.double().numpy(), 10)
    np.random.seed(4)
    got = public(name)(X.cuda(), Y.cuda(), 10)
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()


def test_nonfinite_cuda_tensor_raises():
    X = torch.zeros(5, 2, device="cuda")
    X[2, 0] = float("inf")
    with pytest.raises(ValueError):
        ks1d.kolmogorov_smirnov_1d(X, torch.zeros(4, 2, device="cuda"))


def test_default_call_is_bitwise_the_reference():
    f = np.load(os.path.join(GOLDEN, "metrics1d_diff_100_153.npz"))
    np.random.seed(int(f["seed"]))
    mu, sd = ks1d.kolmogorov_smirnov_1d(f["X"], f["Y"])
    assert mu == f["kolmogorov_smirnov_1d_mean"] and sd == f["kolmogorov_smirnov_1d_std"]


@pytest.mark.parametrize("metric", range(6))
def test_too_small_workspace_is_refused(metric):
    rng = np.random.default_rng(1)
    Xr = torch.from_numpy(rng.normal(size=(30, 2))).cuda()
    Xf = torch.from_numpy(rng.normal(size=(20, 2))).cuda()
    p = _m1d.Pooled(Xr, Xf)
    reps, bins = 2, 8
    idx = torch.zeros(reps * 50, dtype=torch.int32, device="cuda")
    need = _lib.metric1d_workspace_bytes(metric, 30, 20, 2, reps, bins)
    assert need > 0
    tail, dtype = _m1d.OUT_SHAPE[metric]
    out = torch.zeros((reps, 2) + tuple(bins if t is None else t for t in tail), dtype=dtype, device="cuda")
    ws = torch.empty(need - 1, dtype=torch.uint8, device="cuda")
    st = _lib.metric1d_status(metric, p.cols, p.perm, p.gstart, p.ngroups, 30, 20, idx[:reps * 30], idx[reps * 30:],
                              reps, bins, 1.0, 1.0, out, ws)
    assert st == _lib.PFM_EWORKSPACE
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    st = _lib.metric1d_status(metric, p.cols, p.perm, p.gstart, p.ngroups, 30, 20, idx[:reps * 30], idx[reps * 30:],
                              reps, bins, 1.0, 1.0, out, ws)
    assert st == 0
    torch.cuda.synchronize()
