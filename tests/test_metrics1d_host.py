"""The eight 1-D metrics without a GPU: the committed reference fixtures (tests/golden/metrics1d_*.npz) against the
float64 tie-group restatement (tests/metrics1d_numpy.py), argument checks before any device is touched, importing
without a GPU, and the probaforms.metrics alias left at its two names."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, ROOT)

import metrics1d_numpy as m1  # noqa: E402

FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "metrics1d_*.npz")))
BITWISE = ("kolmogorov_smirnov_1d", "cramer_von_mises_1d", "kullback_leibler_1d", "jensen_shannon_1d")
RTOL = {"roc_auc_score_1d": 1e-12, "anderson_darling_1d": 1e-12, "kullback_leibler_1d_kde": 1e-9,
        "jensen_shannon_1d_kde": 1e-9}


def fid(p):
    return os.path.basename(p)[10:-4]


def cases():
    out = []
    for p in FIXTURES:
        f = np.load(p)
        for m in m1.FUNCS:
            if (m + "_raises") in f.files and not bool(f[m + "_raises"]):
                out.append(pytest.param(p, m, id="%s-%s" % (fid(p), m)))
    return out


def test_fixtures_exist():
    names = {fid(p) for p in FIXTURES}
    assert {"diff_100_153", "same_1d", "ties", "edges", "edges_bins", "d16", "kde_wide", "kde_allzero", "cvm_1row",
            "ad_one_value"} <= names
    assert sum(os.path.getsize(p) for p in FIXTURES) < (1 << 20)
    f = np.load(os.path.join(GOLDEN, "metrics1d_ad_one_value.npz"))
    assert bool(f["anderson_darling_1d_raises"])
    for name in ("kde_wide", "kde_allzero"):          # replicates whose KDE probabilities all underflow
        assert np.isnan(np.load(os.path.join(GOLDEN, "metrics1d_%s.npz" % name))["kullback_leibler_1d_kde_rep"]).any()


def assert_close(got, want, metric):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    if metric in BITWISE:
        assert np.array_equal(got[ok], want[ok]), np.abs(got[ok] - want[ok]).max()
    else:
        np.testing.assert_allclose(got[ok], want[ok], rtol=RTOL[metric], atol=0)


@pytest.mark.parametrize("path,metric", cases())
def test_restatement_reproduces_the_reference(path, metric):
    f = np.load(path)
    bins = int(f[m1.BINS[metric]]) if metric in m1.BINS else None
    np.random.seed(int(f["seed"]))
    with np.errstate(all="ignore"):
        S = m1.replicates(metric, f["X"], f["Y"], int(f["n_iters"]), bins)
    assert np.random.random() == float(f[metric + "_next"])
    assert_close(S, f[metric + "_rep"], metric)
    with np.errstate(all="ignore"):
        mu, sd = m1.feature_average(S)
    assert_close([mu, sd], [f[metric + "_mean"], f[metric + "_std"]], metric)


def test_cvm_group_sums_are_the_rank_sums():
    """the closed form per tie group against sum (2R - 2i)^2 from average ranks computed directly"""
    rng = np.random.default_rng(5)
    for _ in range(20):
        x = rng.integers(0, 6, rng.integers(1, 30)).astype(float)
        y = rng.integers(0, 6, rng.integers(1, 30)).astype(float)
        z = np.concatenate([np.sort(x), np.sort(y)])
        rank = np.array([np.sum(z < v) + (np.sum(z == v) + 1) / 2 for v in z])
        want = [int(np.sum((2 * rank[:len(x)] - 2 * np.arange(1, len(x) + 1)) ** 2)),
                int(np.sum((2 * rank[len(x):] - 2 * np.arange(1, len(y) + 1)) ** 2))]
        assert m1.cvm_sums(x, y) == want


NAMES_KS = ("kolmogorov_smirnov_1d", "cramer_von_mises_1d", "roc_auc_score_1d", "anderson_darling_1d")
NAMES_DIV = ("kullback_leibler_1d", "jensen_shannon_1d", "kullback_leibler_1d_kde", "jensen_shannon_1d_kde")


def public(name):
    from probaforms_amd.metrics import div1d, ks1d
    return getattr(ks1d if name in NAMES_KS else div1d, name)


@pytest.mark.parametrize("bad", [
    lambda: (np.zeros(10), np.zeros((10, 1))),                 # 1-D
    lambda: (np.zeros((10, 2)), np.zeros((12, 3))),            # feature counts differ
    lambda: (np.zeros((0, 2)), np.zeros((12, 2))),             # no rows
    lambda: (np.zeros((10, 2), complex), np.zeros((10, 2))),   # complex
    lambda: (np.array([["a", "b"]]), np.zeros((1, 2))),        # strings
    lambda: (np.array([[0.0, np.nan]]), np.zeros((3, 2))),     # NaN
    lambda: (np.zeros((3, 2)), np.array([[np.inf, 0.0]])),     # infinite
])
@pytest.mark.parametrize("name", NAMES_KS + NAMES_DIV)
def test_argument_errors_raise_value_error_before_any_draw(bad, name):
    X, Y = bad()
    np.random.seed(3)
    with pytest.raises(ValueError):
        public(name)(X, Y, n_iters=2)
    np.random.seed(3)
    want = np.random.random()
    np.random.seed(3)
    with pytest.raises(ValueError):
        public(name)(X, Y, n_iters=2)
    assert np.random.random() == want


def test_nonfinite_torch_input_raises_value_error():
    import torch
    X = torch.zeros(4, 2, dtype=torch.float64)
    X[1, 1] = float("nan")
    with pytest.raises(ValueError):
        public("kolmogorov_smirnov_1d")(X, torch.zeros(3, 2))


@pytest.mark.parametrize("bins", [0, -3, 2.0, True, "10", None])
@pytest.mark.parametrize("name", NAMES_DIV)
def test_bins_must_be_a_positive_int(bins, name):
    with pytest.raises(ValueError):
        public(name)(np.zeros((4, 2)), np.zeros((4, 2)), n_iters=2, bins=bins)


@pytest.mark.parametrize("n_iters", [0, -1, 2.5, True])
@pytest.mark.parametrize("name", NAMES_KS + NAMES_DIV)
def test_n_iters_must_be_a_positive_integer(n_iters, name):
    with pytest.raises(ValueError):
        public(name)(np.zeros((4, 2)), np.zeros((4, 2)), n_iters=n_iters)


def test_anderson_darling_needs_three_pooled_rows():
    with pytest.raises(ValueError):
        public("anderson_darling_1d")(np.zeros((1, 1)), np.ones((1, 1)), n_iters=2)


def test_signatures_are_the_reference_ones():
    import inspect
    for name in NAMES_KS:
        assert str(inspect.signature(public(name))) == "(X_real, X_fake, n_iters=100)"
    for name in NAMES_DIV:
        b = 101 if name.endswith("_kde") else 10
        assert str(inspect.signature(public(name))) == "(X_real, X_fake, n_iters=100, bins=%d)" % b


def _run(code):
    env = dict(os.environ, PYTHONPATH=ROOT, HIP_VISIBLE_DEVICES="")
    return subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)


def test_import_of_the_1d_modules_needs_no_gpu_and_loads_nothing():
    r = _run("import probaforms_amd.metrics.ks1d as k, probaforms_amd.metrics.div1d as v\n"
             "from probaforms_amd.metrics import _lib\n"
             "import probaforms_amd.metrics as m\n"
             "assert _lib.LIBRARY.loaded is False\n"
             "assert callable(k.kolmogorov_smirnov_1d) and callable(v.jensen_shannon_1d_kde)\n"
             "assert m.__all__ == ['frechet_distance', 'maximum_mean_discrepancy']\n"
             "print('ok')")
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr


def test_probaforms_alias_still_has_exactly_two_metrics():
    r = _run("import inspect, probaforms_amd\n"
             "import probaforms_amd.metrics.ks1d, probaforms_amd.metrics.div1d\n"
             "probaforms_amd.install_as_probaforms()\n"
             "from probaforms import metrics\n"
             "names = sorted(n for n, _ in inspect.getmembers(metrics, inspect.isfunction))\n"
             "assert names == ['frechet_distance', 'maximum_mean_discrepancy'], names\n"
             "try:\n"
             "    from probaforms.metrics import kolmogorov_smirnov_1d\n"
             "except ImportError:\n"
             "    print('ok')\n")
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr
