"""probaforms_amd.metrics on the GPU: the HIP kernels of libpf_metrics.so against the reference's committed
fixtures (tests/golden/metrics_*.npz), an independent float64 numpy restatement (tests/metrics_numpy.py)
on shapes the fixtures do not cover, the global RNG state, bitwise reproducibility and CUDA-tensor inputs.

The shapes here (nx, ny, d): MMD (50, 51, 3), (60, 70, 100), (129, 65, 5), (1, 2, 2), (4000, 4000, 16); moments (50, 51, 3),
(40, 70, 100), (3000, 2500, 1), (5000, 4100, 16), all continuous Gaussian data through the public path.  The edges of the kernels are
in tests/test_metrics_edges_gpu.py, through the raw entry points: the median select where the two middle keys part in each of its
six digits, tie exactly, or straddle the diagonal zeros; dyadic data with bitwise medians; replicates of different kinds in one call;
MMD seam and feature-chunk shapes (64, 64, 16), (63, 66, 17), (1, 130, 32), (130, 1, 33), (65, 1, 1); moments with unequal and
saturated row parts (2048 | 2049, 4097 | 100, 133122 rows), d = 2, 3, 22, 23, 65, 257, 2049, one- and two-row samples, samples
centred at +-1e6; the status codes on poisoned outputs."""
import glob
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, ROOT)

import metrics_numpy as mn  # noqa: E402
import native_libs  # noqa: E402
from probaforms_amd.metrics import _lib, fd, frechet_distance, maximum_mean_discrepancy, mmd  # noqa: E402

pytestmark = pytest.mark.gpu

native_libs.ensure_built(_lib)

FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "metrics_*.npz")))


def fid(p):
    return os.path.basename(p)[8:-4]


def load(path):
    f = np.load(path)
    return f, f["X"], f["Y"], int(f["seed"]), int(f["n_iters"]), bool(f["standardize"])


@pytest.mark.parametrize("path", FIXTURES, ids=fid)
def test_mmd_replicates_match_the_reference(path):
    f, X, Y, seed, n_iters, std = load(path)
    np.random.seed(seed)
    med, val = mmd.replicates(X, Y, n_iters, std)
    np.testing.assert_allclose(med, f["mmd_med"], rtol=1e-12, atol=0)
    ok = f["mmd_med"] > 0
    assert np.array_equal(med > 0, ok)
    ref = f["mmd_rep"][ok]
    assert (np.abs(val[ok] - ref) <= 1e-11 + 1e-9 * np.abs(ref)).all(), np.abs(val[ok] - ref).max()
    assert np.isnan(val[~ok]).all()


@pytest.mark.parametrize("path", FIXTURES, ids=fid)
def test_mmd_public_call_matches_the_reference(path):
    f, X, Y, seed, n_iters, std = load(path)
    np.random.seed(seed)
    if bool(f["mmd_raises"]):
        with pytest.raises(ValueError):
            maximum_mean_discrepancy(X, Y, n_iters=n_iters, standardize=std)
        # no fault left behind: the next call on the device runs
        np.random.seed(0)
        mu, _ = maximum_mean_discrepancy(np.arange(12.0).reshape(6, 2), np.arange(12.0).reshape(6, 2) + 0.5, n_iters=3)
        assert np.isfinite(mu)
        return
    mu, sd = maximum_mean_discrepancy(X, Y, n_iters=n_iters, standardize=std)
    assert np.random.random() == float(f["mmd_next"])            # the generator stands where the reference left it
    assert isinstance(mu, np.float64) and isinstance(sd, np.float64)
    np.testing.assert_allclose([mu, sd], [f["mmd_mean"], f["mmd_std"]], rtol=1e-9, atol=0)


FD_FIXTURES = [p for p in FIXTURES if "fd_rep" in np.load(p).files]


@pytest.mark.parametrize("path", FD_FIXTURES, ids=fid)
def test_fd_matches_the_reference(path):
    f, X, Y, seed, n_iters, std = load(path)
    np.random.seed(seed)
    rep = fd.replicates(X, Y, n_iters, std)
    np.testing.assert_allclose(rep, f["fd_rep"], rtol=1e-9, atol=1e-13)
    np.random.seed(seed)
    mu, sd = frechet_distance(X, Y, n_iters=n_iters, standardize=std)
    assert np.random.random() == float(f["fd_next"])
    np.testing.assert_allclose([mu, sd], [f["fd_mean"], f["fd_std"]], rtol=1e-9, atol=0)


def numpy_replicates(X, Y, seed, n_iters):
    np.random.seed(seed)
    out = [mn.mmd_replicate(X[ix], Y[iy]) for ix, iy in mn.boot_indices(len(X), len(Y), n_iters)]
    return np.array([o[0] for o in out]), np.array([o[1] for o in out])


@pytest.mark.parametrize("nx,ny,d,n_iters", [
    (50, 51, 3, 5),        # m odd: one middle value
    (60, 70, 100, 3),      # d = 100: seven feature chunks
    (129, 65, 5, 4),       # nx != ny, ragged tiles across the X / Y seam
    (1, 2, 2, 6),          # smallest samples
    (4000, 4000, 16, 1),   # one large replicate: 8000 pooled rows
])
def test_mmd_against_numpy_restatement(nx, ny, d, n_iters):
    rng = np.random.default_rng(nx * 7 + d)
    X = rng.normal(size=(nx, d))
    Y = rng.normal(size=(ny, d)) * 1.3 + 0.2
    med_ref, val_ref = numpy_replicates(X, Y, 99, n_iters)
    np.random.seed(99)
    med, val = mmd.replicates(X, Y, n_iters)
    np.testing.assert_allclose(med, med_ref, rtol=1e-12, atol=0)
    ok = med_ref > 0
    assert (np.abs(val[ok] - val_ref[ok]) <= 1e-11 + 1e-9 * np.abs(val_ref[ok])).all()


@pytest.mark.parametrize("nr,nf,d", [(50, 51, 3), (40, 70, 100), (3000, 2500, 1), (5000, 4100, 16)])
def test_fd_moments_against_numpy(nr, nf, d):
    rng = np.random.default_rng(nr + d)
    X = rng.normal(size=(nr, d)) + 3.0
    Y = rng.normal(size=(nf, d)) * 0.7
    np.random.seed(5)
    mean, cov = fd.moments(X, Y, 3)
    np.random.seed(5)
    for i, (ix, iy) in enumerate(mn.boot_indices(nr, nf, 3)):
        for s, B in enumerate((X[ix], Y[iy])):
            np.testing.assert_allclose(mean[i, s], B.mean(axis=0), rtol=1e-12, atol=1e-14)
            np.testing.assert_allclose(cov[i, s], np.atleast_2d(np.cov(B, rowvar=False)), rtol=1e-11, atol=1e-13)


def test_same_seed_is_bitwise_reproducible():
    rng = np.random.default_rng(1)
    X, Y = rng.normal(size=(700, 4)), rng.normal(size=(650, 4)) + 0.1
    runs = []
    for _ in range(2):
        np.random.seed(3)
        runs.append(mmd.replicates(X, Y, 20) + (fd.replicates(X, Y, 20),) + fd.moments(X, Y, 4))
    for a, b in zip(*runs):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_cuda_tensors_match_the_numpy_path(dtype):
    rng = np.random.default_rng(2)
    Xt = torch.from_numpy(rng.normal(size=(300, 3))).to("cuda", dtype)
    Yt = torch.from_numpy(rng.normal(size=(280, 3)) + 0.2).to("cuda", dtype)
    Xn, Yn = Xt.double().cpu().numpy(), Yt.double().cpu().numpy()
    for fn in (mmd.replicates, fd.replicates):
        np.random.seed(8)
        a = fn(Xt, Yt, 6)
        np.random.seed(8)
        b = fn(Xn, Yn, 6)
        for u, v in zip(a if isinstance(a, tuple) else (a,), b if isinstance(b, tuple) else (b,)):
            assert np.array_equal(u, v)
    np.random.seed(8)
    r1 = maximum_mean_discrepancy(Xt, Yt, n_iters=4, standardize=True) + frechet_distance(Xt, Yt, n_iters=4, standardize=True)
    np.random.seed(8)
    r2 = maximum_mean_discrepancy(Xn, Yn, n_iters=4, standardize=True) + frechet_distance(Xn, Yn, n_iters=4, standardize=True)
    assert r1 == r2


def test_groups_of_replicates_keep_the_stream():
    """a call split into several groups of replicates (index buffers alternating) draws what one group does"""
    from probaforms_amd.metrics import _boot
    rng = np.random.default_rng(4)
    X, Y = rng.normal(size=(90, 2)), rng.normal(size=(80, 2))
    np.random.seed(6)
    one = mmd.replicates(X, Y, 9)
    nxt = np.random.random()
    keep = _boot.MAX_GROUP
    try:
        _boot.MAX_GROUP = 2
        np.random.seed(6)
        many = mmd.replicates(X, Y, 9)
        assert np.random.random() == nxt
    finally:
        _boot.MAX_GROUP = keep
    np.testing.assert_allclose(many[0], one[0], rtol=0, atol=0)
    np.testing.assert_allclose(many[1], one[1], rtol=1e-12, atol=1e-15)
