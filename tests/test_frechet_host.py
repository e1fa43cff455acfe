"""probaforms_amd.metrics.losses.frechet_loss / fd.frechet_distance_full_sample without a GPU: the float64 restatement
(tests/frechet_numpy.py) against its independent route (scipy.linalg.sqrtm and np.linalg.solve), against central differences and
against the reference's own replicates in tests/golden/metrics_*.npz; the C header against the binding; the workspace queries and the
argument statuses of pfm_sym_eig and pfm_frechet_grad; the public calls' argument checks.

Bounds.  The two routes compute the same quantities by different factorisations of float64 matrices of condition number at most
100 (asserted): they are held within 1e-12 of |dmu|^2 + tr C_r + tr C_f (values) and of the largest gradient element of the sample
(gradients), the bound of the GPU tests; measured here 1.3e-15 and 1.2e-14.  Central differences, step h = 1e-6: FD is smooth on
non-singular data, the truncation error is O(h^2 |FD'''|) = 1e-12 and the rounding error of the two values about 2^-52 |FD| / h =
1e-8 for |FD| up to 50: the bound is 1e-6.
"""
import ctypes
import glob
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import frechet_numpy as fr  # noqa: E402
import metrics_numpy as mn  # noqa: E402
import native_libs  # noqa: E402
from probaforms_amd.metrics import _lib, fd, losses  # noqa: E402
from probaforms_amd.metrics.fd import frechet_distance_full_sample  # noqa: E402
from probaforms_amd.metrics.losses import frechet_loss  # noqa: E402

CSRC = os.path.join(ROOT, "probaforms_amd", "metrics", "csrc")
NEW = ("pfm_sym_eig_workspace_bytes", "pfm_sym_eig", "pfm_frechet_grad_workspace_bytes", "pfm_frechet_grad")
SHAPES = ((2, 2, 1), (2, 3, 1), (5, 4, 2), (37, 53, 3), (40, 33, 5), (64, 40, 16), (90, 70, 17), (150, 131, 33), (300, 260, 64))
FD_FIXTURES = [p for p in sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "metrics_*.npz"))) if "fd_rep" in np.load(p).files]
H, FD_TOL = 1e-6, 1e-6


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_the_two_routes_agree(shape):
    Xr, Xf = fr.data(*shape)
    a, b = fr.value_grad(Xr, Xf), fr.independent(Xr, Xf)
    assert a["eig"][-1] / a["eig"][0] <= 100 and a["eig_swapped"][-1] / a["eig_swapped"][0] <= 100
    assert a["rank"].tolist() == [shape[2]] * 2
    ev = abs(a["value"] - b["value"]) / a["scale"]
    eg = max(np.abs(a[k] - b[k]).max() / np.abs(a[k]).max() for k in ("grad_r", "grad_f"))
    print("%s: value off by %.3g of the scale, gradients by %.3g of their largest element" % (shape, ev, eg))
    assert ev <= 1e-12 and eg <= 1e-12
    assert np.array_equal(a["parts"][0], a["value"]) and abs(a["parts"][1:4].sum() - a["scale"]) <= 1e-15 * a["scale"]


@pytest.mark.parametrize("shape", ((5, 4, 2), (7, 6, 3), (12, 9, 5)), ids=str)
def test_restatement_gradient_equals_central_differences(shape):
    Xr, Xf = fr.data(*shape)
    o = fr.value_grad(Xr, Xf)
    worst = 0.0
    for name, A in (("grad_r", Xr), ("grad_f", Xf)):
        for at in np.ndindex(A.shape):
            v = []
            for step in (H, -H):
                B = A.copy()
                B[at] += step
                v.append(fr.value_of(B, Xf) if name == "grad_r" else fr.value_of(Xr, B))
            worst = max(worst, abs((v[0] - v[1]) / (2 * H) - o[name][at]))
    print("%s: gradient off central differences by at most %.3g" % (shape, worst))
    assert worst <= FD_TOL


def test_equal_samples_and_one_feature():
    Xr, _ = fr.data(40, 40, 5)
    o = fr.value_grad(Xr, Xr.copy())
    assert abs(o["value"]) <= 1e-12 * o["scale"] and np.abs(o["Gr"]).max() <= 1e-12 and np.abs(o["grad_f"]).max() <= 1e-12
    Xr, Xf = fr.data(9, 7, 1)
    o = fr.value_grad(Xr, Xf)
    want = (Xr.mean() - Xf.mean()) ** 2 + (Xr.std(ddof=1) - Xf.std(ddof=1)) ** 2
    assert abs(o["value"] - want) <= 1e-14 * o["scale"]
    # rows all equal (four of them, dyadic: their mean is exact): C_f = 0, M = 0, nothing is kept and G = I
    Xr, _ = fr.data(9, 5, 3)
    o = fr.value_grad(Xr, np.tile(np.array([[0.5, -1.25, 3.0]]), (4, 1)), rcond=1e-10)
    assert o["rank"].tolist() == [0, 0] and np.array_equal(o["Gf"], np.eye(3)) and np.array_equal(o["Gr"], np.eye(3))


def fixture_rows(path, count=None):
    """-> (the fixture, [(resampled real rows, resampled fake rows)] of its first `count` replicates, on the reference's own
    index stream, the scaler applied in numpy)"""
    f = np.load(path)
    X, Y = f["X"].astype(np.float64), f["Y"].astype(np.float64)
    if bool(f["standardize"]):
        X, Y = fr.standardized(X, Y)
    state = np.random.get_state()
    np.random.seed(int(f["seed"]))
    idx = mn.boot_indices(len(X), len(Y), int(f["n_iters"]))
    np.random.set_state(state)
    return f, [(X[ix], Y[iy]) for ix, iy in idx[:count]]


@pytest.mark.parametrize("path", FD_FIXTURES, ids=lambda p: os.path.basename(p)[8:-4])
def test_restatement_reproduces_the_references_replicates(path):
    f, rows = fixture_rows(path)
    got = np.array([fr.value_of(a, b) for a, b in rows])
    print("%s: off the reference by at most %.3g (relative)" % (os.path.basename(path), np.abs(got / f["fd_rep"] - 1).max()))
    np.testing.assert_allclose(got, f["fd_rep"], rtol=1e-9, atol=1e-13)
    assert rows[0][0].shape[1] <= 16 and any(bool(np.load(p)["standardize"]) for p in FD_FIXTURES)


# ---- header, binding, statuses -------------------------------------------------------------------------------------------

def test_header_declarations_equal_the_binding():
    raw = open(os.path.join(CSRC, "pf_metrics.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = re.findall(r"\b(pfm_[a-z0-9_]+)\s*\(", text)
    assert sorted(declared) == sorted(_lib.EXPORTS) and set(NEW) <= set(_lib.EXPORTS)
    assert _lib.ABI_VERSION == 101 and "#define PFM_VERSION 101 " in raw
    assert "#define PFM_FRECHET_MAX_D %d " % _lib.FRECHET_MAX_D in raw and _lib.FRECHET_MAX_D == 64
    assert "#define PFM_EIG_MAX_SWEEPS %d " % _lib.EIG_MAX_SWEEPS in raw and _lib.EIG_MAX_SWEEPS == 30
    assert "pf_frechet.o" in open(os.path.join(CSRC, "Makefile")).read()
    source = re.sub(r"//.*", "", open(os.path.join(CSRC, "pf_frechet.hip")).read())
    assert "atomic" not in source.lower() and '#include "pf_moments.h"' in source
    for name in NEW:
        args = re.search(r"\b%s\s*\(([^)]*)\)" % name, text).group(1)
        assert len(args.split(",")) == len(_lib._SIGNATURES[name][1]), name
    assert _lib._SIGNATURES["pfm_frechet_grad"][1][5] is ctypes.c_double                   # rcond travels as a double
    # four d x d matrices at the odd pitch and the scratch fit the LDS of one CU
    assert 8 * 4 * 64 * 65 + 4096 <= 160 * 1024


def test_workspace_queries_and_argument_statuses_without_a_device():
    native_libs.ensure_built(_lib)
    L, fake = _lib.lib(), ctypes.c_void_p(256)
    E, U, W = _lib.PFM_EINVAL, _lib.PFM_EUNSUPPORTED, _lib.PFM_EWORKSPACE
    assert L.pfm_version() == _lib.ABI_VERSION == 101 and all(hasattr(L, name) for name in NEW)

    qe = _lib.sym_eig_workspace_bytes
    assert 0 < qe(1, 1) == qe(65535, 64) <= 4096                                            # a constant: nothing is kept
    for bad in ((0, 4), (-1, 4), (65536, 4), (3, 0), (3, -2), (3, 65), (3, 2 ** 40)):
        assert qe(*bad) == 0, bad

    def eig(A=fake, batch=3, d=5, w=fake, V=fake, sweeps=fake, ws=fake, nbytes=1 << 20):
        return L.pfm_sym_eig(None, A, batch, d, w, V, sweeps, ws, nbytes)

    # refused before anything is read or launched (the device pointers are never dereferenced)
    assert eig(A=None) == eig(w=None) == E
    assert eig(batch=0) == eig(batch=-1) == eig(batch=65536) == eig(d=0) == eig(d=-3) == E
    assert eig(d=65) == eig(d=2 ** 40) == U and eig(d=65, batch=0) == E
    assert eig(ws=None) == eig(nbytes=qe(3, 5) - 1) == eig(V=None, sweeps=None, nbytes=0) == W

    qf = _lib.frechet_grad_workspace_bytes
    assert qf(4, 1, 2) > 0 and qf(2 ** 31 - 1, 64, 2 ** 30) > 0
    for bad in ((3, 2, 1), (3, 2, 2), (4, 2, 1), (4, 2, 3), (4, 0, 2), (4, -1, 2), (2 ** 31, 2, 5), (10, 65, 5), (10, 2, -2), (10, 2, 11)):
        assert qf(*bad) == 0, bad
    # the moments, two d x d factors and the moments' partial sums (at most 64 row parts): nothing of size n d^2
    assert qf(2 ** 31 - 1, 64, 2 ** 30) <= 8 * (2 * 64 + 4 * 64 * 64 + 2 * 64 * (64 + 64 * 65 // 2)) + 8 * 256
    assert qf(2 ** 20, 16, 2 ** 19) == qf(2 ** 24, 16, 2 ** 23)                               # the row parts are saturated

    def grad(Z=fake, n=10, d=3, nfirst=4, rcond=1e-10, sides=3, value=fake, g=fake, parts=fake, ev=fake, rank=fake, ws=fake,
             nbytes=1 << 20):
        return L.pfm_frechet_grad(None, Z, n, d, nfirst, rcond, sides, value, g, parts, ev, rank, ws, nbytes)

    assert grad(Z=None) == grad(value=None) == E
    assert grad(nfirst=1) == grad(nfirst=0) == grad(nfirst=-1) == grad(nfirst=9) == grad(nfirst=10) == grad(n=3, nfirst=2) == E
    assert grad(d=0) == grad(d=-1) == grad(n=2 ** 31, nfirst=5) == E
    for bad in (-1e-300, -1.0, 1.0, 1.5, float("inf"), -float("inf"), float("nan")):
        assert grad(rcond=bad) == E, bad
    assert grad(sides=-1) == grad(sides=4) == grad(sides=0) == E
    assert grad(sides=0, g=None, nbytes=0) == W                                             # no gradient: sides may be 0
    assert grad(d=65) == grad(d=2 ** 40) == U and grad(d=65, nfirst=1) == E
    assert grad(ws=None) == grad(nbytes=qf(10, 3, 4) - 1) == W
    assert grad(g=None, parts=None, ev=None, rank=None, nbytes=0) == W
    for ok in (0.0, 0.5, 1.0 - 2.0 ** -53):
        assert grad(rcond=ok, nbytes=0) == W, ok


# ---- the public calls' argument checks ----------------------------------------------------------------------------------

def test_argument_errors_are_raised_before_any_device_is_touched(monkeypatch):
    def touched(*a, **k):
        raise AssertionError("an argument error must be raised before anything touches a device")
    for name in ("frechet_grad", "frechet_grad_workspace_bytes", "sym_eig", "lib"):
        monkeypatch.setattr(_lib, name, touched)
    monkeypatch.setattr(torch.cuda, "is_available", touched)
    X, Y = np.zeros((5, 3)), np.ones((4, 3))
    for fn in (frechet_loss, frechet_distance_full_sample):
        with pytest.raises(ValueError, match="different numbers of features"):
            fn(X, np.ones((4, 2)))
        with pytest.raises(ValueError, match="2-D"):
            fn(X[:, 0], Y)
        with pytest.raises(ValueError, match="2-D"):
            fn(torch.zeros(5, 3), torch.zeros(4))
        with pytest.raises(ValueError, match="real numeric"):
            fn(X.astype(complex), Y)
        for bad in (1, 0, None, "yes", np.array([True])):
            with pytest.raises(ValueError, match="standardize must be a bool"):
                fn(X, Y, standardize=bad)
        with pytest.raises(ValueError, match="at most 64 features, got 65"):
            fn(np.zeros((5, 65)), np.zeros((4, 65)))
        with pytest.raises(ValueError, match="at most 64 features"):
            fn(torch.zeros(5, 100), torch.zeros(4, 100))
        for a, b in ((X[:1], Y), (X, Y[:1]), (torch.zeros(1, 3), torch.zeros(1, 3))):
            with pytest.raises(ValueError, match="at least 2 rows"):
                fn(a, b)
    for bad in (-1e-12, 1.0, 2, float("nan"), float("inf"), True, "1e-10", [1e-10], np.array([1e-10])):
        with pytest.raises(ValueError, match=r"rcond must be None or a number in \[0, 1\)"):
            losses.frechet_loss(X, Y, rcond=bad)
    for bad in (1, 0, None, "yes"):
        with pytest.raises(ValueError, match="return_rank must be a bool"):
            losses.frechet_loss(X, Y, return_rank=bad)
    assert losses._rcond(None, 16) == 16 * 2.0 ** -52 and losses._rcond(0, 3) == 0.0 and losses._rcond(np.float32(0.5), 3) == 0.5


def test_new_names_stay_out_of_the_export_list():
    import probaforms_amd.metrics as m
    assert m.__all__ == ["frechet_distance", "maximum_mean_discrepancy"]
    assert not hasattr(m, "frechet_loss") and not hasattr(m, "frechet_distance_full_sample")
    assert callable(losses.frechet_loss) and callable(fd.frechet_distance_full_sample)
    assert "**An eigenvalue of rounding noise" in losses.frechet_loss.__doc__
