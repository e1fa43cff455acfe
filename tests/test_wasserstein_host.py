"""probaforms_amd.metrics.wasserstein without a GPU: the committed fixtures (tests/golden/wasserstein_*.npz, made with scipy)
against the float64 restatement (tests/wasserstein_numpy.py), the restatement's two formulas against each other, argument
checks before any draw, importing without a GPU, and the C header against the binding."""
import ctypes
import glob
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
import wasserstein_numpy as wn  # noqa: E402
from probaforms_amd.metrics import _lib, wasserstein  # noqa: E402

FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "wasserstein_*.npz")))
RTOL = 1e-12          # tests/test_wasserstein_gpu.py says why


def fid(p):
    return os.path.basename(p)[12:-4]


def test_fixtures_exist():
    assert {"p1_diff_100_153", "p1_ties", "p1_1row", "p2_equal_64", "p2_equal_ties", "sliced_p1", "sliced_p2_equal"} \
        <= {fid(p) for p in FIXTURES}
    assert sum(os.path.getsize(p) for p in FIXTURES) < (1 << 18)


def spread(f):
    Z = np.concatenate([f["X"], f["Y"]])
    return float(Z.max() - Z.min())


@pytest.mark.parametrize("path", FIXTURES, ids=fid)
def test_restatement_reproduces_the_fixture(path):
    f = np.load(path)
    np.random.seed(int(f["seed"]))
    if str(f["kind"]) == "1d":
        S, nxt = wn.replicates_1d(f["X"], f["Y"], int(f["n_iters"]), int(f["p"]))
        mu, sd = wn.feature_average(S)
    else:
        S, nxt = wn.replicates_sliced(f["X"], f["Y"], int(f["n_iters"]), int(f["n_projections"]), int(f["p"]))
        mu, sd = S.mean(axis=0), S.std(axis=0)
    assert nxt == float(f["next"])
    atol = RTOL * spread(f)
    np.testing.assert_allclose(S, f["rep"], rtol=RTOL, atol=atol)
    np.testing.assert_allclose([mu, sd], [f["mean"], f["std"]], rtol=RTOL, atol=atol)


@pytest.mark.parametrize("nx,ny", [(40, 35), (64, 64), (1, 7), (257, 256), (3000, 2)])
def test_the_two_formulas_agree(nx, ny):
    """W_1 by the cdf formula equals the grid formula at p = 1; at one size the grid formula at p = 2 is the sorted pairs'"""
    rng = np.random.default_rng(nx + ny)
    x, y = np.round(rng.normal(size=nx), 1 if nx == 40 else 12), rng.normal(0.3, 2, size=ny)
    np.testing.assert_allclose(wn.wp_pow(x, y, 1), wn.w1(x, y), rtol=RTOL)
    if nx == ny:
        np.testing.assert_allclose(np.sqrt(wn.wp_pow(x, y, 2)), wn.sorted_pair_w2(x, y), rtol=RTOL)
    assert wn.wp_pow(x, x, 2) == 0.0 and wn.w1(x, x) == 0.0


PUBLIC = {"wasserstein_1d": wasserstein.wasserstein_1d, "sliced_wasserstein_distance": wasserstein.sliced_wasserstein_distance}
OK = (np.zeros((4, 2)), np.ones((5, 2)))
BAD = {
    "p=3": (OK, dict(p=3)),
    "p=0.5": (OK, dict(p=0.5)),
    "p=True": (OK, dict(p=True)),
    "p='1'": (OK, dict(p="1")),
    "NaN": ((np.array([[0.0, np.nan]]), np.zeros((3, 2))), {}),
    "inf": ((np.zeros((3, 2)), np.array([[np.inf, 0.0]])), {}),
    "features": ((np.zeros((10, 2)), np.zeros((12, 3))), {}),
    "1-D": ((np.zeros(10), np.zeros((10, 1))), {}),
    "n_iters=0": (OK, dict(n_iters=0)),
    "n_iters=True": (OK, dict(n_iters=True)),
}
BAD_SLICED = {
    "n_projections=0": (OK, dict(n_projections=0)),
    "n_projections=True": (OK, dict(n_projections=True)),
    "n_projections=2.0": (OK, dict(n_projections=2.0)),
}


def _bad_cases():
    out = [(n, k) for n in PUBLIC for k in BAD]
    return out + [("sliced_wasserstein_distance", k) for k in BAD_SLICED]


@pytest.mark.parametrize("name,bad", _bad_cases())
def test_argument_errors_raise_value_error_before_any_draw(name, bad):
    (X, Y), kw = {**BAD, **BAD_SLICED}[bad]
    np.random.seed(3)
    want = np.random.random()
    for fn in (PUBLIC[name], wasserstein.REPLICATES[name]):
        np.random.seed(3)
        with pytest.raises(ValueError):
            fn(X, Y, **kw)
        assert np.random.random() == want


def test_p_may_be_a_float_equal_to_1_or_2():
    assert [wasserstein._order(p) for p in (1, 2, 1.0, 2.0, np.int64(2), np.float64(1.0))] == [1, 2, 1, 2, 2, 1]


def test_signatures():
    import inspect
    assert str(inspect.signature(wasserstein.wasserstein_1d)) == "(X_real, X_fake, n_iters=100, p=1)"
    assert str(inspect.signature(wasserstein.sliced_wasserstein_distance)) == \
        "(X_real, X_fake, n_iters=100, n_projections=64, p=2, standardize=False)"
    assert sorted(wasserstein.REPLICATES) == ["sliced_wasserstein_distance", "wasserstein_1d"]


def _run(code):
    env = dict(os.environ, PYTHONPATH=ROOT, HIP_VISIBLE_DEVICES="")
    return subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)


def test_import_needs_no_gpu_loads_nothing_and_widens_no_export_list():
    r = _run("from probaforms_amd.metrics.wasserstein import wasserstein_1d, sliced_wasserstein_distance\n"
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
    text = re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)
    declared = re.findall(r"\b(pfm_[a-z0-9_]+)\s*\(", text)
    assert sorted(set(declared)) == sorted(_lib.EXPORTS) and len(declared) == len(_lib.EXPORTS)
    assert {"pfm_project", "pfm_wasserstein1d", "pfm_wasserstein1d_workspace_bytes"} <= set(_lib.EXPORTS)
    assert "#define PFM_VERSION %d " % _lib.ABI_VERSION in open(header).read() and _lib.ABI_VERSION == 101


def test_workspace_query_and_argument_statuses_without_a_device():
    native_libs.ensure_built(_lib)
    q = _lib.wasserstein1d_workspace_bytes
    assert q(30, 20, 2, 3, 1) > 0 and q(30, 20, 2, 3, 2) > 0
    for bad in ((0, 20, 2, 3, 1), (30, 0, 2, 3, 1), (30, 20, 0, 3, 1), (30, 20, 2, 0, 1), (30, 20, 2, 65536, 1),
                (2 ** 30, 2 ** 30, 2, 3, 1), (30, 20, 2, 3, 0), (30, 20, 2, 3, 3), (-1, 20, 2, 3, 2)):
        assert q(*bad) == 0, bad
    # counted per replicate: r replicates need at most r times what one needs, so _boot.group_size can split a call
    for nr, nf, d, p in ((30, 20, 2, 1), (30, 20, 2, 2), (3000, 2500, 5, 2)):
        assert q(nr, nf, d, 7, p) <= 7 * q(nr, nf, d, 1, p)
    assert q(3000, 2500, 5, 1, 2) > q(3000, 2500, 5, 1, 1)         # the compacted tables beyond LDS
    # refused before anything is read or launched (the pointers are never dereferenced)
    L, fake = _lib.lib(), ctypes.c_void_p(256)
    call = lambda p, cols, reps, nbytes: L.pfm_wasserstein1d(None, p, cols, fake, fake, fake, 30, 20, 2, fake, fake, reps, fake,
                                                              fake, nbytes)
    assert call(1, None, 3, 1 << 30) == -1 and call(1, fake, 0, 1 << 30) == -1          # PFM_EINVAL
    assert call(3, fake, 3, 1 << 30) == _lib.PFM_EUNSUPPORTED and call(0, fake, 3, 1 << 30) == _lib.PFM_EUNSUPPORTED
    assert call(2, fake, 3, q(30, 20, 2, 3, 2) - 1) == _lib.PFM_EWORKSPACE
    assert L.pfm_project(None, None, 30, fake, 20, 2, fake, 4, fake) == -1
    assert L.pfm_project(None, fake, 30, fake, 20, 2, fake, 0, fake) == -1
