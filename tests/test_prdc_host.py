"""probaforms_amd.metrics.prdc without a GPU: the float64 restatement (tests/prdc_numpy.py) against the committed fixtures
(tests/golden/prdc_*.npz, made with scipy's cdist and the `prdc` package's published expressions), the margin condition that
makes the GPU tests' exact comparison legitimate, argument checks before any draw, importing without a GPU, the C header against
the binding and the workspace query.

Exactness argument.  A replicate's output is four integer counts of comparisons `D^2 < radius^2`.  The kernel accumulates
fma(df, df, acc); the restatement rounds the product and the sum separately; scipy may do either.  Per feature the two differ by
one rounding of a non-negative term, so a squared distance moves by at most d 2^-52 relative, and the counts agree exactly unless
a compared pair is closer than that.
  dyadic data      multiples of 1/8 within +-8: every df, df^2 and sum is exact in float64 under any convention, so radii and
                   counts are bitwise equal, and exact ties between a cross distance and a radius occur (they test the strict <);
  continuous data  every compared pair (D^2, radius^2) of every replicate of every case must have a relative gap above 1e-9
                   (d 2^-52 is below 4e-15 for d <= 17) and no gap of exactly 0.  This is a condition on the inputs, asserted
                   here on the restatement alone; it is not a tolerance of the comparison.
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

import native_libs  # noqa: E402
import prdc_numpy as pn  # noqa: E402
from probaforms_amd.metrics import _lib, prdc as prdc_mod  # noqa: E402

FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "prdc_*.npz")))
MARGIN = 1e-9
# the package's density is (1 / k) * mean(counts): three roundings where Dn / (k nf) has one; means and stds of at most 12
# values of magnitude <= 1.1 add a few more.  1e-15 relative, and 1e-15 absolute for the stds near 0.
VALUE_TOL = 1e-15


def fid(p):
    return os.path.basename(p)[5:-4]


def test_fixtures_exist():
    assert {"normal_100_153_k5", "collapsed_k3", "dispersed_k1", "dyadic_k5", "tiny_k4"} <= {fid(p) for p in FIXTURES}
    assert sum(os.path.getsize(p) for p in FIXTURES) < (1 << 18)


@pytest.mark.parametrize("path", FIXTURES, ids=fid)
def test_restatement_reproduces_the_fixture(path):
    f = np.load(path)
    X, Y, n_iters, k = f["X"], f["Y"], int(f["n_iters"]), int(f["k"])
    np.random.seed(int(f["seed"]))
    o = pn.replicates(X, Y, n_iters, k, keep=True)
    assert o["next"] == float(f["next"])
    if fid(path).startswith("dyadic"):
        assert o["ties"] > 0
        assert np.array_equal(o["rr"][0], f["rr0"]) and np.array_equal(o["ss"][0], f["ss0"])
    else:
        assert o["margin"] > MARGIN
        rtol = (X.shape[1] + 1) * 2.0 ** -52
        np.testing.assert_allclose(o["rr"][0], f["rr0"], rtol=rtol, atol=0)
        np.testing.assert_allclose(o["ss"][0], f["ss0"], rtol=rtol, atol=0)
    assert np.array_equal(o["counts"], f["counts"])
    V = np.array([pn.metrics(c, len(X), len(Y), k) for c in o["counts"]])
    np.testing.assert_allclose(V, f["values"], rtol=VALUE_TOL, atol=0)
    ms = pn.mean_std(o["counts"], len(X), len(Y), k)
    np.testing.assert_allclose([m for m, _ in ms], f["mean"], rtol=VALUE_TOL, atol=VALUE_TOL)
    np.testing.assert_allclose([s for _, s in ms], f["std"], rtol=VALUE_TOL, atol=VALUE_TOL)
    C, vals, rr, ss, D = pn.full_sample(X, Y, k)
    assert list(C) == list(f["full_counts"])
    np.testing.assert_allclose(vals, f["full_values"], rtol=VALUE_TOL, atol=0)
    if not fid(path).startswith("dyadic"):
        assert pn.margin(D, rr, ss) > MARGIN


def test_the_collapsed_fixture_reads_as_high_precision_and_half_recall():
    f = np.load(os.path.join(GOLDEN, "prdc_collapsed_k3.npz"))
    precision, recall, _, _ = f["full_values"]
    assert precision > 0.9 and 0.4 < recall < 0.6


@pytest.mark.parametrize("case", pn.CASES + [pn.GROUPS_CASE, pn.MANY_TILES_CASE], ids=str)
def test_every_gpu_case_keeps_its_margin(case):
    """the condition on the inputs under which tests/test_prdc_gpu.py compares counts exactly"""
    X, Y = pn.data(*case)
    np.random.seed(pn.SEED)
    n_iters = {pn.GROUPS_CASE: pn.GROUPS_ITERS, pn.MANY_TILES_CASE: pn.MANY_TILES_ITERS}.get(case, pn.N_ITERS)
    o = pn.replicates(X, Y, n_iters, case[3])
    print("smallest relative gap %.3g" % o["margin"])
    assert o["ties"] == 0 and o["margin"] > MARGIN


def test_the_dyadic_case_has_exact_ties():
    X, Y = pn.dyadic(*pn.DYADIC_CASE)
    assert np.array_equal(X * 8, np.round(X * 8)) and np.abs(X).max() <= 8 and np.abs(Y).max() <= 8
    np.random.seed(pn.SEED)
    o = pn.replicates(X, Y, pn.N_ITERS, pn.DYADIC_CASE[3])
    assert o["ties"] > 0


def test_radius_of_a_row_drawn_more_than_k_times_is_zero():
    X = np.arange(12.0).reshape(6, 2)
    S = X[[0, 0, 0, 1, 2, 5]]
    assert list(pn.radii(S, 2)[:3]) == [0.0, 0.0, 0.0] and pn.radii(S, 3)[0] > 0
    assert pn.radii(X, 5)[0] == pn.d2(X[:1], X).max()           # k = rows - 1: the row's largest value


OK = (np.arange(40.0).reshape(20, 2), np.arange(36.0).reshape(18, 2) + 0.5)
BAD = {
    "nearest_k=0": (OK, dict(nearest_k=0)),
    "nearest_k=-1": (OK, dict(nearest_k=-1)),
    "nearest_k=True": (OK, dict(nearest_k=True)),
    "nearest_k=2.0": (OK, dict(nearest_k=2.0)),
    "nearest_k='5'": (OK, dict(nearest_k="5")),
    "nearest_k=17": (OK, dict(nearest_k=17)),
    "nearest_k=rows": (OK, dict(nearest_k=18)),
    "nearest_k=min(rows)": ((np.zeros((9, 2)), np.zeros((5, 2))), dict(nearest_k=5)),
    "k=62 at 65x63x33": (pn.data(*pn.TOO_LARGE_K), dict(nearest_k=pn.TOO_LARGE_K[3])),
    "NaN": ((np.array([[0.0, np.nan]] * 8), np.zeros((8, 2))), {}),
    "inf": ((np.zeros((8, 2)), np.array([[np.inf, 0.0]] * 8)), {}),
    "features": ((np.zeros((10, 2)), np.zeros((12, 3))), {}),
    "1-D": ((np.zeros(10), np.zeros((10, 1))), {}),
    "strings": ((np.array([["a", "b"]] * 8), np.zeros((8, 2))), {}),
}
BAD_BOOT = {
    "n_iters=0": (OK, dict(n_iters=0)),
    "n_iters=True": (OK, dict(n_iters=True)),
    "n_iters=2.5": (OK, dict(n_iters=2.5)),
}


@pytest.mark.parametrize("bad", list(BAD) + list(BAD_BOOT))
def test_argument_errors_raise_value_error_before_any_draw(bad):
    (X, Y), kw = {**BAD, **BAD_BOOT}[bad]
    fns = [prdc_mod.prdc, prdc_mod.REPLICATES["prdc"]] + ([prdc_mod.prdc_full_sample] if bad in BAD else [])
    np.random.seed(3)
    want = np.random.random()
    for fn in fns:
        np.random.seed(3)
        with pytest.raises(ValueError):
            fn(X, Y, **kw)
        assert np.random.random() == want


def test_signatures():
    assert str(inspect.signature(prdc_mod.prdc)) == "(X_real, X_fake, n_iters=100, nearest_k=5, standardize=False)"
    assert str(inspect.signature(prdc_mod.prdc_full_sample)) == "(X_real, X_fake, nearest_k=5, standardize=False)"
    assert list(prdc_mod.REPLICATES) == ["prdc"]
    assert prdc_mod.PRDC._fields == ("precision", "recall", "density", "coverage")
    for fn in (prdc_mod.prdc, prdc_mod.prdc_full_sample):
        assert "biased low" in fn.__doc__


def test_metrics_of_divides_python_ints_once():
    C = np.array([[7, 5, 29, 6], [2 ** 40 + 1, 3, 2 ** 53 + 2, 1]], dtype=np.int64)
    M = prdc_mod.metrics_of(C, 6, 7, 4)
    assert M.dtype == np.float64 and M.shape == (2, 4)
    assert M[0].tolist() == [7 / 7, 5 / 6, 29 / 28, 6 / 6] and M[1, 2] == (2 ** 53 + 2) / 28
    assert [tuple(r) for r in M] == [pn.metrics(c, 6, 7, 4) for c in C]


def _run(code):
    env = dict(os.environ, PYTHONPATH=ROOT, HIP_VISIBLE_DEVICES="")
    return subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)


def test_import_needs_no_gpu_loads_nothing_and_widens_no_export_list():
    r = _run("from probaforms_amd.metrics.prdc import prdc, prdc_full_sample, PRDC\n"
             "from probaforms_amd.metrics import _lib\n"
             "import probaforms_amd, probaforms_amd.metrics as m\n"
             "assert _lib.LIBRARY.loaded is False\n"
             "assert m.__all__ == ['frechet_distance', 'maximum_mean_discrepancy']\n"
             "probaforms_amd.install_as_probaforms()\n"
             "import inspect\n"
             "from probaforms import metrics\n"
             "names = sorted(n for n, _ in inspect.getmembers(metrics, inspect.isfunction))\n"
             "assert names == ['frechet_distance', 'maximum_mean_discrepancy'], names\n"
             "print('ok')")
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr


def test_header_declarations_equal_the_binding_exports():
    header = os.path.join(ROOT, "probaforms_amd", "metrics", "csrc", "pf_metrics.h")
    raw = open(header).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = re.findall(r"\b(pfm_[a-z0-9_]+)\s*\(", text)
    assert sorted(set(declared)) == sorted(_lib.EXPORTS) and len(declared) == len(_lib.EXPORTS)
    assert {"pfm_prdc", "pfm_prdc_workspace_bytes"} <= set(_lib.EXPORTS)
    assert "#define PFM_VERSION %d " % _lib.ABI_VERSION in raw and _lib.ABI_VERSION == 101
    assert "#define PFM_KNN_MAX_K %d " % _lib.KNN_MAX_K in raw and _lib.KNN_MAX_K == 16


def test_workspace_query_and_argument_statuses_without_a_device():
    native_libs.ensure_built(_lib)
    q = _lib.prdc_workspace_bytes
    assert q(30, 20, 2, 3, 5) > 0 and q(2, 2, 1, 1, 1) > 0 and q(30, 20, 2, 65535, 16) > 0
    for bad in ((0, 20, 2, 3, 5), (30, 0, 2, 3, 5), (30, 20, 0, 3, 5), (30, 20, 2, 0, 5), (30, 20, 2, 65536, 5),
                (30, 20, 2, 3, 0), (30, 20, 2, 3, -1), (30, 20, 2, 3, 20), (20, 30, 2, 3, 20), (30, 20, 2, 3, 25),
                (30, 20, 2, 3, 17), (65, 63, 33, 1, 62), (-1, 20, 2, 3, 5), (2 ** 31, 20, 2, 3, 5), (30, 2 ** 31, 2, 3, 5),
                (2 ** 30, 2 ** 30, 2 ** 40, 3, 5)):
        assert q(*bad) == 0, bad
    # counted per replicate, so that _boot.group_size can split a call
    for nr, nf, d, k in ((30, 20, 2, 5), (3000, 2500, 5, 16)):
        assert q(nr, nf, d, 7, k) <= 7 * q(nr, nf, d, 1, k)
    # refused before anything is read or launched (the pointers are never dereferenced)
    L, fake = _lib.lib(), ctypes.c_void_p(256)

    def call(nr=30, nf=20, d=2, reps=3, k=5, Xr=fake, counts=fake, ws=fake, nbytes=1 << 30):
        return L.pfm_prdc(None, Xr, nr, fake, nf, d, fake, fake, reps, k, fake, fake, counts, ws, nbytes)

    EINVAL = -1
    assert call(Xr=None) == EINVAL and call(counts=None) == EINVAL
    assert call(nr=0) == EINVAL and call(nf=0) == EINVAL and call(d=0) == EINVAL and call(reps=0) == EINVAL
    assert call(reps=65536) == EINVAL and call(k=0) == EINVAL and call(k=20) == EINVAL and call(k=25) == EINVAL
    assert call(k=17) == _lib.PFM_EUNSUPPORTED and call(nr=65, nf=63, d=33, k=62) == _lib.PFM_EUNSUPPORTED
    assert call(nbytes=q(30, 20, 2, 3, 5) - 1) == _lib.PFM_EWORKSPACE and call(ws=None) == _lib.PFM_EWORKSPACE
