"""probaforms_amd.metrics without a GPU: the bootstrap index stream, the host trace-sqrtm, the committed
reference fixtures against the float64 restatement, argument checks, the probaforms.metrics alias, and the proof that every
constructed input of tests/metrics_cases.py has the property tests/test_metrics_edges_gpu.py relies on."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, ROOT)

import metrics_cases as mc  # noqa: E402
import metrics_numpy as mn  # noqa: E402
from probaforms_amd.metrics import _boot  # noqa: E402
from probaforms_amd.metrics.fd import trace_sqrtm  # noqa: E402


def fixtures():
    return sorted(glob.glob(os.path.join(GOLDEN, "metrics_*.npz")))


def test_fixtures_exist():
    names = {os.path.basename(f)[8:-4] for f in fixtures()}
    assert {"nb_dist0", "nb_dist2", "nb_dist10", "same_1d", "diff_100_153", "diff_342_100", "c2_d16", "standardize",
            "median0"} <= names
    assert sum(os.path.getsize(f) for f in fixtures()) < (1 << 20)


def test_index_draw_matches_sklearn_resample():
    utils = pytest.importorskip("sklearn.utils")
    nx, ny, reps = 37, 53, 6
    np.random.seed(123)
    buf = np.empty(reps * (nx + ny), np.int32)
    _boot.draw_indices(buf, reps, nx, ny)
    after = np.random.random()
    np.random.seed(123)
    ix, iy = np.arange(nx), np.arange(ny)
    want_x, want_y = [], []
    for _ in range(reps):
        want_x.append(utils.resample(ix))
        want_y.append(utils.resample(iy))
    assert np.random.random() == after
    np.testing.assert_array_equal(buf[:reps * nx].reshape(reps, nx), np.array(want_x))
    np.testing.assert_array_equal(buf[reps * nx:].reshape(reps, ny), np.array(want_y))


def test_index_draw_is_the_legacy_randint_stream():
    np.random.seed(7)
    buf = np.empty(3 * (5 + 9), np.int32)
    _boot.draw_indices(buf, 3, 5, 9)
    np.random.seed(7)
    want = mn.boot_indices(5, 9, 3)
    np.testing.assert_array_equal(buf[:15].reshape(3, 5), np.array([w[0] for w in want]))
    np.testing.assert_array_equal(buf[15:].reshape(3, 9), np.array([w[1] for w in want]))


def test_group_sizes_cover_the_call():
    assert _boot.group_sizes(100, 10000) == [100]
    G = _boot.group_size(100, 2_000_000)
    assert G == 8 and _boot.group_sizes(100, 2_000_000) == [4, 8]
    assert _boot.group_size(5, 10, ws_per_rep=1 << 40) == 1


@pytest.mark.parametrize("d", [1, 2, 3, 7, 16, 32])
@pytest.mark.parametrize("n", [3, 50])
def test_trace_sqrtm_matches_scipy(d, n):
    linalg = pytest.importorskip("scipy.linalg")
    rng = np.random.default_rng(d * 100 + n)
    A = np.atleast_2d(np.cov(rng.normal(size=(n, d)) * rng.uniform(0.1, 3, d), rowvar=False))
    B = np.atleast_2d(np.cov(rng.normal(size=(n, d)) + 0.3, rowvar=False))
    want = np.trace(linalg.sqrtm(A.dot(B), disp=False)[0].real)
    # n <= d: A is singular and its zero eigenvalues come out of either method as rounding noise of ~1e-17, whose
    # square roots (~sqrt(eps) of the scale) enter the trace; with n > d both agree to rounding
    tol = (2e-7 if n <= d else 1e-12) * abs(want) + 1e-14
    assert abs(trace_sqrtm(A, B) - want) <= tol


@pytest.mark.parametrize("path", [p for p in fixtures() if "fd_rep" in np.load(p).files],
                         ids=lambda p: os.path.basename(p)[8:-4])
def test_fd_fixture_by_host_moments(path):
    """the reference's per-replicate FD from the index stream, np.mean / np.cov and trace_sqrtm"""
    f = np.load(path)
    X, Y = f["X"], f["Y"]
    if bool(f["standardize"]):
        mu, sd = X.mean(axis=0), X.std(axis=0)
        sd[sd == 0] = 1
        X, Y = (X - mu) / sd, (Y - mu) / sd
    np.random.seed(int(f["seed"]))
    got = []
    for ix, iy in mn.boot_indices(len(X), len(Y), int(f["n_iters"])):
        Xb, Yb = X[ix], Y[iy]
        cr, cf = np.atleast_2d(np.cov(Xb, rowvar=False)), np.atleast_2d(np.cov(Yb, rowvar=False))
        got.append(np.sum((Xb.mean(0) - Yb.mean(0)) ** 2.0) + np.trace(cr) + np.trace(cf) - 2 * trace_sqrtm(cr, cf))
    assert np.random.random() == float(f["fd_next"])
    np.testing.assert_allclose(got, f["fd_rep"], rtol=1e-9, atol=1e-13)
    np.testing.assert_allclose([np.mean(got), np.std(got)], [f["fd_mean"], f["fd_std"]], rtol=1e-9)


@pytest.mark.parametrize("name", ["same_1d", "diff_100_153", "diff_342_100", "standardize", "median0"])
def test_mmd_fixture_by_numpy_restatement(name):
    """the semantics the kernels implement (full-matrix median incl. the diagonal, RBF means incl. the
    diagonals) against the reference's own per-replicate values"""
    f = np.load(os.path.join(GOLDEN, "metrics_%s.npz" % name))
    X, Y = f["X"], f["Y"]
    if bool(f["standardize"]):
        mu, sd = X.mean(axis=0), X.std(axis=0)
        sd[sd == 0] = 1
        X, Y = (X - mu) / sd, (Y - mu) / sd
    np.random.seed(int(f["seed"]))
    meds, vals = [], []
    for ix, iy in mn.boot_indices(len(X), len(Y), int(f["n_iters"])):
        med, v = mn.mmd_replicate(X[ix], Y[iy])
        meds.append(med)
        vals.append(v)
    meds, vals = np.array(meds), np.array(vals)
    np.testing.assert_allclose(meds, f["mmd_med"], rtol=1e-12, atol=0)
    ok = f["mmd_med"] > 0
    np.testing.assert_allclose(vals[ok], f["mmd_rep"][ok], rtol=1e-9, atol=1e-11)
    assert bool(f["mmd_raises"]) == (not ok.all())


@pytest.mark.parametrize("bad", [
    lambda: (np.zeros(10), np.zeros((10, 1))),                 # 1-D
    lambda: (np.zeros((10, 2, 1)), np.zeros((10, 2))),         # 3-D
    lambda: (np.zeros((10, 2)), np.zeros((12, 3))),            # feature counts differ
    lambda: (np.zeros((0, 2)), np.zeros((12, 2))),             # no rows
    lambda: (np.zeros((10, 2), complex), np.zeros((10, 2))),   # complex
    lambda: (np.array([["a", "b"]]), np.zeros((1, 2))),        # strings
    lambda: (np.zeros((4, 2), bool), np.zeros((4, 2))),        # booleans
])
@pytest.mark.parametrize("metric", ["maximum_mean_discrepancy", "frechet_distance"])
def test_argument_errors_raise_value_error(bad, metric):
    import probaforms_amd.metrics as M
    X, Y = bad()
    with pytest.raises(ValueError):
        getattr(M, metric)(X, Y, n_iters=2)


@pytest.mark.parametrize("n_iters", [0, -1, 2.5, True])
def test_n_iters_must_be_a_positive_integer(n_iters):
    from probaforms_amd.metrics import maximum_mean_discrepancy
    with pytest.raises(ValueError):
        maximum_mean_discrepancy(np.zeros((4, 2)), np.zeros((4, 2)), n_iters=n_iters)


def _run(code):
    env = dict(os.environ, PYTHONPATH=ROOT, HIP_VISIBLE_DEVICES="")
    return subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)


def test_import_needs_no_gpu_and_loads_nothing():
    r = _run("import probaforms_amd.metrics as m, sys\n"
             "from probaforms_amd.metrics import _lib\n"
             "assert _lib.LIBRARY.loaded is False\n"
             "assert m.__all__ == ['frechet_distance', 'maximum_mean_discrepancy']\n"
             "print('ok')")
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr


def test_install_as_probaforms_exposes_exactly_the_two_metrics():
    r = _run("import inspect, probaforms_amd\n"
             "probaforms_amd.install_as_probaforms()\n"
             "from probaforms import metrics\n"
             "import probaforms.metrics as pm\n"
             "from probaforms.metrics import maximum_mean_discrepancy, frechet_distance\n"
             "import probaforms_amd.metrics as am\n"
             "assert pm is metrics and maximum_mean_discrepancy is am.maximum_mean_discrepancy\n"
             "assert frechet_distance is am.frechet_distance\n"
             "names = sorted(n for n, _ in inspect.getmembers(metrics, inspect.isfunction))\n"
             "assert names == ['frechet_distance', 'maximum_mean_discrepancy'], names\n"
             "assert sorted(metrics.__all__) == names\n"
             "try:\n"
             "    from probaforms.metrics import kolmogorov_smirnov_1d\n"
             "except ImportError:\n"
             "    print('ok')\n"
             "from probaforms.models import RealNVP\n")
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr


# ---- tests/metrics_cases.py: every constructed input has its named property, from the numpy restatement alone -------------------

def test_key_digits_are_the_kernels_layout():
    assert mc.SHIFT[0] + mc.WIDTH[0] == 64 and mc.SHIFT[-1] == 0
    assert all(mc.SHIFT[i] == mc.SHIFT[i + 1] + mc.WIDTH[i + 1] for i in range(5))
    assert mc.key(0.0) == 0 and mc.key(5e-324) == 1 and mc.key(1.0) == 0x3FF << 52
    assert mc.parting_digit(1.0, 1.0) is None and mc.parting_digit(1.0, 2.0) == 0
    assert [mc.parting_digit(0.0, np.float64(2.0 ** (s - 1074))) for s in mc.SHIFT[1:]] == [1, 2, 3, 4, 5]


@pytest.mark.parametrize("digit", sorted(mc.PARTING))
def test_four_points_part_the_middle_keys_in_the_named_digit(digit):
    X, Y = mc.four_points(*mc.PARTING[digit])
    Z = np.concatenate((X, Y))
    lo, hi = mc.middle_values(Z)
    assert 0 < lo < hi and mc.parting_digit(lo, hi) == digit
    # both middle values are exact (so the kernel's fma chain and the restatement's products and sums give the same bits), and
    # they are the 2nd and 3rd smallest pair (in the digit-0 case two pairs share the upper one)
    u = np.sort(mn.pooled_upper_d2(Z))
    Zl = Z.astype(np.longdouble)
    ul = np.sort(np.array([((Zl[i] - Zl[j]) ** 2).sum() for i in range(4) for j in range(i + 1, 4)]))
    assert u[1] == lo and u[2] == hi and u[0] < lo and hi <= u[3]
    assert np.longdouble(lo) == ul[1] and np.longdouble(hi) == ul[2]
    assert mn.median_distance(Z) == (np.sqrt(lo) + np.sqrt(hi)) / 2


def test_four_points_tie_has_equal_middle_keys():
    X, Y = mc.four_points(*mc.TIE)
    Z = np.concatenate((X, Y))
    lo, hi = mc.middle_values(Z)
    assert (len(Z) ** 2) % 2 == 0 and lo > 0
    assert mc.key(lo) == mc.key(hi) and mc.parting_digit(lo, hi) is None
    u = np.sort(mn.pooled_upper_d2(Z))
    assert u[0] < u[1] == u[2] == lo < u[3]                       # two different pairs share the bits: ranks 6 to 9
    Zl = Z.astype(np.longdouble)
    assert ((Zl[1] - Zl[3]) ** 2).sum() == np.longdouble(lo) == ((Zl[2] - Zl[3]) ** 2).sum()       # and they are exact


@pytest.mark.parametrize("digit", sorted(mc.LADDER))
def test_ladder_parts_a_diagonal_zero_from_the_pair_in_the_named_digit(digit):
    X, Y = mc.ladder(mc.LADDER[digit])
    Z = np.concatenate((X, Y))
    lo, hi = mc.middle_values(Z)
    assert lo == 0.0 and hi > 0 and mc.parting_digit(lo, hi) == digit
    assert all(g == 0 for g in mc.digits(hi)[:digit])             # the pair shares the all-zero prefix up to that digit
    if digit == 0:
        assert hi == 2.25
    else:                                                     # d^2 is the denormal with the integer key k^2: exact
        k = mc.LADDER[digit] / 2.0 ** -537
        assert mc.key(hi) == int(k) ** 2 and np.sqrt(hi) == mc.LADDER[digit]
    assert mn.median_distance(Z) == mc.LADDER[digit] / 2


def test_dyadic_case_is_exact_and_tied_at_the_middle():
    X, Y, idx = mc.dyadic()
    assert (X.shape[0], Y.shape[0], X.shape[1]) == mc.DYADIC_SHAPE and len(idx) == mc.DYADIC_REPS
    assert ((X.shape[0] + Y.shape[0]) ** 2) % 2 == 0
    for ix, iy in idx:
        Z = np.concatenate((X[ix], Y[iy]))
        u = mn.pooled_upper_d2(Z)
        Zl = Z.astype(np.longdouble)
        m = len(Z)
        ul = np.concatenate([((Zl[i + 1:] - Zl[i]) ** 2).sum(axis=1) for i in range(m - 1)])
        assert ul.dtype == np.longdouble and np.array_equal(u.astype(np.longdouble), ul)       # every d^2 is exact
        for v in mc.middle_values(Z):
            shared = int((u == v).sum())
            print("middle d^2 %r: %d pairs, %d entries of the full matrix" % (v, shared, 2 * shared))
            assert v > 0 and shared >= 2                          # at least two different pairs: a tie the select must hold


def test_moments_longdouble_agrees_with_numpy():
    rng = np.random.default_rng(0)
    B = rng.normal(size=(40, 5)) * rng.uniform(0.5, 2, 5) + 3.0
    mean, cov = mc.moments_longdouble(B)
    assert mean.dtype == np.longdouble and cov.dtype == np.longdouble
    np.testing.assert_allclose(mean.astype(np.float64), B.mean(axis=0), rtol=1e-13, atol=0)
    np.testing.assert_allclose(cov.astype(np.float64), np.cov(B, rowvar=False), rtol=1e-13, atol=1e-13)
    assert np.array_equal(cov, cov.T)
    one = mc.moments_longdouble(B[:1])
    assert np.array_equal(one[0].astype(np.float64), B[0]) and np.isnan(one[1]).all()
