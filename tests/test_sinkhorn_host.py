"""probaforms_amd.metrics.sinkhorn without a GPU: the float64 restatement (tests/sinkhorn_numpy.py) against the committed
fixtures (tests/golden/sinkhorn_*.npz), its summation-order floor, its two limits (a sample against itself; the energy distance
at large eps), argument checks before any draw, importing without a GPU, the C header against the binding, and the status codes
and workspace query of pfm_sinkhorn without a device.

Why the GPU tests' tolerance (1e-11 cmax, cmax the largest pooled cost) is safe.  Each softmin carries a few ulps of the
potentials' magnitude, which cmax bounds, and the averaged map is non-expansive, so 101 steps add at most about 1e-13 cmax:
test_summation_order_floor measures the restatement against itself with the rows and the draws of both samples in another
order and requires 1e-13 cmax.  The GPU bound leaves 100 x for the device's exp and log.
"""
import ctypes
import glob
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, ROOT)
sys.path.insert(0, GOLDEN)

import energy_numpy as en  # noqa: E402
import make_golden_sinkhorn  # noqa: E402
import native_libs  # noqa: E402
import sinkhorn_numpy as sn  # noqa: E402
from probaforms_amd.metrics import _lib, sinkhorn as sk  # noqa: E402

FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "sinkhorn_*.npz")))
NAMES = {"normal_40_35_d3_p2", "normal_65_63_d16_p1", "self_30_d2_p2", "outlier_20_20_d2_p1", "tiny_1_2_d1_p2"}


def fid(p):
    return os.path.basename(p)[9:-4]


def test_fixtures_exist_and_are_small():
    assert {fid(p) for p in FIXTURES} == NAMES == set(make_golden_sinkhorn.cases())
    assert sum(os.path.getsize(p) for p in FIXTURES) <= 64 << 10


@pytest.mark.parametrize("path", FIXTURES, ids=fid)
def test_restatement_reproduces_the_fixture(path):
    f = np.load(path)
    X, Y, p, eps, n = f["X"], f["Y"], int(f["p"]), float(f["eps"]), int(f["n_sinkhorn"])
    reps, N = len(f["ix"]), len(X) + len(Y)
    assert f["value"].shape == f["drift"].shape == (reps,) and f["potentials"].shape == (reps, 2, N)
    np.random.seed(int(f["seed"]))
    if not fid(path).startswith("self"):                                # the indices are the reference's stream
        for r in range(reps):
            ix, iy = sn.draw(len(X), len(Y))
            assert np.array_equal(ix, f["ix"][r]) and np.array_equal(iy, f["iy"][r])
    o = sn.solve_many(X, Y, f["ix"], f["iy"], p, eps, n)
    tol = 1e-13 * sn.cmax(X, Y, p)
    for key in ("value", "drift", "potentials"):
        print("%s: largest difference %.3g (bound %.3g)" % (key, np.abs(o[key] - f[key]).max(), tol))
        assert np.abs(o[key] - f[key]).max() <= tol
    assert np.isfinite(f["potentials"]).all() and (f["value"] >= -tol).all() and (f["drift"] >= 0).all()
    if fid(path).startswith("self"):
        assert np.abs(f["value"]).max() <= tol and np.array_equal(f["ix"], f["iy"])
    if fid(path).startswith("outlier"):
        assert sn.cmax(X, Y, p) / eps > 745.0 * 100                      # exp of an unshifted term underflows by far


@pytest.mark.parametrize("p", (1, 2))
def test_summation_order_floor(p):
    """the same weighted samples with the rows AND the draws of both samples in another order: every sum of the restatement
    runs in another order, the result is the same up to rounding"""
    nr, nf, d = 65, 130, 3
    X, Y = sn.data(nr, nf, d)
    IX, IY = sn.bootstrap(nr, nf, 2, sn.SEED)
    cm, eps = sn.cmax(X, Y, p), sn.REG * sn.median(X, Y) ** p
    rng = np.random.default_rng(5)
    worst = 0.0
    for ix, iy in zip(IX, IY):
        a = sn.solve(X, Y, ix, iy, p, eps, 100)
        pr, pf = rng.permutation(nr), rng.permutation(nf)                # new row r is old row pr[r]
        inv_r, inv_f = np.argsort(pr), np.argsort(pf)
        b = sn.solve(X[pr], Y[pf], inv_r[ix][rng.permutation(nr)], inv_f[iy][rng.permutation(nf)], p, eps, 100)
        back = np.stack([np.concatenate([b["potentials"][s, :nr][inv_r], b["potentials"][s, nr:][inv_f]]) for s in (0, 1)])
        worst = max(worst, abs(a["value"] - b["value"]), abs(a["drift"] - b["drift"]), np.abs(a["potentials"] - back).max())
    print("p = %d: largest difference between the two orders %.3g cmax" % (p, worst / cm))
    assert 0 < worst <= 1e-13 * cm


@pytest.mark.parametrize("p", (1, 2))
def test_a_sample_against_itself_is_zero(p):
    X, _ = sn.data(70, 3, 4)
    IX, _ = sn.bootstrap(70, 70, 2, sn.SEED)
    cm, eps = sn.cmax(X, X, p), sn.REG * sn.median(X, X) ** p
    for ix in (IX[0], np.arange(70)):
        o = sn.solve(X, X.copy(), ix, ix, p, eps, 30)
        assert abs(o["value"]) <= 1e-13 * cm
        assert np.abs(o["potentials"][0] - o["potentials"][1]).max() <= 1e-13 * cm


def test_large_eps_is_half_the_squared_energy_distance():
    """softmin(h, C, w) = sum_j w_j (C_ij - h_j) - O(cmax^2 / eps): at p = 1 the fixed point has S = exy - exx / 2 - eyy / 2"""
    nr, nf, d = 65, 130, 3
    X, Y = sn.data(nr, nf, d)
    IX, IY = sn.bootstrap(nr, nf, 2, sn.SEED)
    cm = sn.cmax(X, Y, 1)
    for ix, iy in list(zip(IX, IY)) + [(np.arange(nr), np.arange(nf))]:
        o = sn.solve(X, Y, ix, iy, 1, 1e6 * cm, 100)
        d2 = en.values(en.sums(X, Y, ix, iy), nr, nf, True)[0]
        print("S %.12g, D^2 / 2 %.12g, difference %.3g cmax" % (o["value"], d2 / 2, abs(o["value"] - d2 / 2) / cm))
        assert abs(o["value"] - d2 / 2) <= 1e-5 * cm and o["value"] > 0


OK = (np.arange(40.0).reshape(20, 2), np.arange(36.0).reshape(18, 2) + 0.5)
BAD = {
    "NaN": ((np.array([[0.0, np.nan]] * 8), np.zeros((8, 2))), {}),
    "inf": ((np.zeros((8, 2)), np.array([[np.inf, 0.0]] * 8)), {}),
    "features": ((np.zeros((10, 2)), np.zeros((12, 3))), {}),
    "1-D": ((np.zeros(10), np.zeros((10, 1))), {}),
    "empty": ((np.zeros((0, 2)), np.zeros((10, 2))), {}),
    "standardize=1": (OK, dict(standardize=1)),
    "p=3": (OK, dict(p=3)),
    "p=0": (OK, dict(p=0)),
    "p=2.0": (OK, dict(p=2.0)),
    "p=True": (OK, dict(p=True)),
    "reg=0": (OK, dict(reg=0.0)),
    "reg=-1": (OK, dict(reg=-1.0)),
    "reg=nan": (OK, dict(reg=float("nan"))),
    "reg=None": (OK, dict(reg=None)),
    "epsilon=0": (OK, dict(epsilon=0.0)),
    "epsilon=-2": (OK, dict(epsilon=-2.0)),
    "epsilon=inf": (OK, dict(epsilon=float("inf"))),
    "epsilon='a'": (OK, dict(epsilon="a")),
    "epsilon=1e-320": (OK, dict(epsilon=1e-320)),
    "n_sinkhorn=-1": (OK, dict(n_sinkhorn=-1)),
    "n_sinkhorn=2.5": (OK, dict(n_sinkhorn=2.5)),
    "n_sinkhorn=True": (OK, dict(n_sinkhorn=True)),
    "n_sinkhorn=None": (OK, dict(n_sinkhorn=None)),
}
BAD_BOOT = {
    "n_iters=0": (OK, dict(n_iters=0)),
    "n_iters=True": (OK, dict(n_iters=True)),
    "n_iters=2.5": (OK, dict(n_iters=2.5)),
}


@pytest.mark.parametrize("bad", list(BAD) + list(BAD_BOOT))
def test_argument_errors_raise_value_error_before_any_draw(bad):
    (X, Y), kw = {**BAD, **BAD_BOOT}[bad]
    fns = [sk.sinkhorn_divergence, sk.REPLICATES["sinkhorn_divergence"]]
    if bad in BAD:
        fns.append(sk.sinkhorn_divergence_full_sample)
    np.random.seed(3)
    want = np.random.random()
    for fn in fns:
        np.random.seed(3)
        with pytest.raises(ValueError):
            fn(X, Y, **kw)
        assert np.random.random() == want


def test_epsilon_of():
    assert sk.epsilon_of(2.0, 2, 0.1) == np.float64(0.1) * np.float64(2.0) ** 2
    assert sk.epsilon_of(3.0, 1, 0.5) == 1.5 and isinstance(sk.epsilon_of(3.0, 1, 0.5), np.float64)
    for median in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            sk.epsilon_of(median, 2, 0.1)
    with pytest.raises(ValueError):
        sk.epsilon_of(1e-170, 2, 0.1)                                    # eps underflows: no finite reciprocal


def test_signatures():
    assert str(inspect.signature(sk.sinkhorn_divergence)) == \
        "(X_real, X_fake, n_iters=100, p=2, reg=0.1, epsilon=None, n_sinkhorn=100, standardize=False)"
    assert str(inspect.signature(sk.sinkhorn_divergence_full_sample)) == \
        "(X_real, X_fake, p=2, reg=0.1, epsilon=None, n_sinkhorn=100, standardize=False)"
    assert list(sk.REPLICATES) == ["sinkhorn_divergence"] and sk.Sinkhorn._fields == ("value", "epsilon", "drift")


def test_import_needs_no_gpu_loads_nothing_and_widens_no_export_list():
    code = ("from probaforms_amd.metrics.sinkhorn import sinkhorn_divergence, sinkhorn_divergence_full_sample, Sinkhorn\n"
            "from probaforms_amd.metrics import _lib\n"
            "import probaforms_amd.metrics as m\n"
            "assert _lib.LIBRARY.loaded is False\n"
            "assert m.__all__ == ['frechet_distance', 'maximum_mean_discrepancy']\n"
            "print('ok')")
    env = dict(os.environ, PYTHONPATH=ROOT, HIP_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr


def test_header_declarations_equal_the_binding_exports():
    header = os.path.join(ROOT, "probaforms_amd", "metrics", "csrc", "pf_metrics.h")
    raw = open(header).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = re.findall(r"\b(pfm_[a-z0-9_]+)\s*\(", text)
    assert sorted(set(declared)) == sorted(_lib.EXPORTS) and len(declared) == len(_lib.EXPORTS)
    assert {"pfm_sinkhorn", "pfm_sinkhorn_workspace_bytes"} <= set(_lib.EXPORTS)
    assert "#define PFM_VERSION %d " % _lib.ABI_VERSION in raw and _lib.ABI_VERSION == 101
    makefile = open(os.path.join(os.path.dirname(header), "Makefile")).read()
    assert "pf_sinkhorn.o" in makefile


def test_workspace_query_and_argument_statuses_without_a_device():
    native_libs.ensure_built(_lib)
    assert _lib.lib().pfm_version() == 101
    q = _lib.sinkhorn_workspace_bytes
    assert q(30, 20, 2, 3) > 0 and q(1, 1, 1, 1) > 0 and q(30, 20, 2, 65535) > 0
    for bad in ((0, 20, 2, 3), (30, 0, 2, 3), (30, 20, 0, 3), (30, 20, 2, 0), (30, 20, 2, 65536), (-1, 20, 2, 3),
                (30, 20, 2, -1), (2 ** 31, 20, 2, 3), (30, 2 ** 31, 2, 3), (2 ** 30, 2 ** 30, 2 ** 40, 3)):
        assert q(*bad) == 0, bad
    # counts, log-weights and three potential buffers: 60 bytes per replicate and pooled row, nothing of the pair matrix's size
    n = 10000
    assert 60 * 100 * 2 * n <= q(n, n, 16, 100) <= 60 * 100 * 2 * n + (5 << 8) and q(n, n, 16, 100) < 8 * (2 * n) ** 2 // 20
    for nr, nf, d in ((30, 20, 2), (3000, 2500, 5)):
        assert q(nr, nf, d, 7) <= 7 * q(nr, nf, d, 1)
        assert q(nr, nf, d, 7) == q(nr, nf, d + 9, 7)
    # refused before anything is read or launched (the pointers are never dereferenced)
    L, fake = _lib.lib(), ctypes.c_void_p(256)

    def call(nr=30, nf=20, d=2, reps=3, p=2, eps=0.5, n=5, Xr=fake, Xf=fake, ir=fake, jf=fake, value=fake, drift=fake,
             pot=fake, ws=fake, nbytes=1 << 30):
        return L.pfm_sinkhorn(None, Xr, nr, Xf, nf, d, ir, jf, reps, p, eps, n, value, drift, pot, ws, nbytes)

    for kw in (dict(Xr=None), dict(Xf=None), dict(ir=None), dict(jf=None), dict(value=None), dict(drift=None), dict(nr=0),
               dict(nf=0), dict(d=0), dict(reps=0), dict(reps=65536), dict(nr=2 ** 31), dict(eps=0.0), dict(eps=-1.0),
               dict(eps=float("inf")), dict(eps=float("nan")), dict(eps=1e-320), dict(n=-1)):
        assert call(**kw) == _lib.PFM_EINVAL, kw
    for p in (0, 3, -1):
        assert call(p=p) == _lib.PFM_EUNSUPPORTED
    assert call(p=3, eps=0.0) == _lib.PFM_EINVAL
    assert call(nbytes=q(30, 20, 2, 3) - 1) == _lib.PFM_EWORKSPACE and call(ws=None) == _lib.PFM_EWORKSPACE
    assert call(pot=None, nbytes=q(30, 20, 2, 3) - 1) == _lib.PFM_EWORKSPACE
