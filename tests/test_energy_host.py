"""probaforms_amd.metrics.energy without a GPU: the float64 restatement (tests/energy_numpy.py) against scipy.stats.energy_distance
at one feature, the two summation orders (gathered rows against draw counts) at every shape the GPU tests use, the committed
fixtures (tests/golden/energy_*.npz, regenerated bit for bit), argument checks before any draw, importing without a GPU, the C
header against the binding and the workspace query.

Why the GPU tests' tolerance is safe.  The kernel computes a replicate's pair sums as c D c over the original rows, tile by
tile; the restatement sums scipy's cdist of the gathered rows with numpy's pairwise sum.  Both add the same non-negative terms in
float64, so each is within (number of additions in a chain) 2^-53 relative of the exact sum; test_the_two_summation_orders_agree
measures the two restatements against each other at every shape and stays below 1e-13, two orders of magnitude inside the
GPU tests' rtol of 1e-12.
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
import scipy.stats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, ROOT)
sys.path.insert(0, GOLDEN)

import energy_numpy as en  # noqa: E402
import make_golden_energy  # noqa: E402
import native_libs  # noqa: E402
from probaforms_amd.metrics import _lib, energy as energy_mod  # noqa: E402

FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "energy_*.npz")))
NAMES = {"normal_100_153_d16", "self_64_d4", "integer_65_63_d1", "tiny_1_2_d1", "clusters_standardized"}


def fid(p):
    return os.path.basename(p)[7:-4]


def test_fixtures_exist_and_are_small():
    assert {fid(p) for p in FIXTURES} == NAMES
    largest_prdc = max(os.path.getsize(p) for p in glob.glob(os.path.join(GOLDEN, "prdc_*.npz")))
    assert all(os.path.getsize(p) <= largest_prdc for p in FIXTURES)


def test_fixtures_regenerate_bit_for_bit():
    made = make_golden_energy.cases()
    assert set(made) == NAMES
    for name, arrays in made.items():
        f = np.load(os.path.join(GOLDEN, "energy_%s.npz" % name))
        assert sorted(f.files) == sorted(arrays)
        for key, want in arrays.items():
            want = np.asarray(want)
            assert f[key].dtype == want.dtype and f[key].shape == want.shape and f[key].tobytes() == want.tobytes(), (name, key)


@pytest.mark.parametrize("path", FIXTURES, ids=fid)
def test_restatement_reproduces_the_fixture(path):
    f = np.load(path)
    X, Y, n_iters = f["X"], f["Y"], int(f["n_iters"])
    Xs, Ys = en.standardize(X, Y) if bool(f["standardize"]) else (X, Y)
    np.random.seed(int(f["seed"]))
    o = en.replicates(Xs, Ys, n_iters)
    assert o["next"] == float(f["next"])
    np.testing.assert_allclose(o["sums"], f["sums"], rtol=1e-13, atol=0)
    E = en.means(f["sums"], len(X), len(Y))
    assert np.abs(en.values(o["sums"], len(X), len(Y), True) - f["d2"]).max() <= 4e-13 * E.max()
    assert np.array_equal(en.values(f["sums"], len(X), len(Y), True), f["d2"])
    m, s = en.mean_std(f["sums"], len(X), len(Y))
    assert m == f["mean"] and s == f["std"]
    np.testing.assert_allclose(en.full_sample(Xs, Ys), f["full_sums"], rtol=1e-13, atol=0)
    if fid(path).startswith("self"):
        assert f["full_sums"][0] == f["full_sums"][1] and en.values(f["full_sums"], 64, 64, False)[0] <= 1e-7
    if fid(path).startswith("integer"):
        assert np.array_equal(f["sums"], np.round(f["sums"])) and f["sums"].max() < 2 ** 53
        assert np.array_equal(o["sums"], f["sums"])


def test_one_feature_is_scipys_energy_distance():
    """within 1e-14 absolute on unit-scale samples, whose distances are of order 1 (scipy integrates the squared difference of
    the two distribution functions, another formula altogether)"""
    worst = 0.0
    for nr, nf, d, n_iters in ((100, 153, 1, 3), (65, 63, 1, 4), (257, 256, 1, 3), (1, 2, 1, 3)):
        X, Y = en.data(nr, nf, 1)
        np.random.seed(en.SEED)
        o = en.replicates(X, Y, n_iters)
        D = en.values(o["sums"], nr, nf, False)
        for r in range(n_iters):
            want = scipy.stats.energy_distance(X[o["ix"][r], 0], Y[o["iy"][r], 0])
            worst = max(worst, abs(D[r] - want))
    print("largest |restatement - scipy.stats.energy_distance| = %.3g" % worst)
    assert worst <= 1e-14


@pytest.mark.parametrize("case", en.CASES + en.OTHER_CASES + [en.INTEGER_CASE], ids=str)
def test_the_two_summation_orders_agree(case):
    """gathered rows (the definition) against draw counts on the original rows (what the kernel does)"""
    nr, nf, d, n_iters = case
    X, Y = (en.integer_data if case == en.INTEGER_CASE else en.data)(nr, nf, d)
    n_iters = min(n_iters, 4)               # the draws do not change the orders compared
    np.random.seed(en.SEED)
    a = en.replicates(X, Y, n_iters)
    np.random.seed(en.SEED)
    b = en.replicates(X, Y, n_iters, counts=True)
    assert a["next"] == b["next"]
    rel = np.abs(a["sums"] - b["sums"]) / np.where(a["sums"] > 0, a["sums"], 1.0)
    print("largest relative difference %.3g" % rel.max())
    np.testing.assert_allclose(b["sums"], a["sums"], rtol=1e-13, atol=0)
    if case == en.INTEGER_CASE:
        assert np.array_equal(a["sums"], b["sums"])


def test_values():
    S = np.array([[8.0, 18.0, 15.0], [0.0, 0.0, 0.0], [4.0, 9.0, 5.0]])
    E = en.means(S, 2, 3)
    assert E.tolist() == [[2.0, 2.0, 2.5], [0.0, 0.0, 0.0], [1.0, 1.0, 5.0 / 6.0]]
    assert en.from_means(E, True).tolist() == [1.0, 0.0, (2.0 * (5.0 / 6.0) - 1.0) - 1.0]
    assert en.from_means(E, False).tolist() == [1.0, 0.0, 0.0]                # a negative D^2 is clamped before the root
    assert np.array_equal(energy_mod.means_of(S, 2, 3), E)
    for sq in (True, False):
        assert np.array_equal(energy_mod.values_of(E, sq), en.from_means(E, sq))
        assert np.array_equal(en.values(S, 2, 3, sq), en.from_means(E, sq))


OK = (np.arange(40.0).reshape(20, 2), np.arange(36.0).reshape(18, 2) + 0.5)
BAD = {
    "NaN": ((np.array([[0.0, np.nan]] * 8), np.zeros((8, 2))), {}),
    "inf": ((np.zeros((8, 2)), np.array([[np.inf, 0.0]] * 8)), {}),
    "features": ((np.zeros((10, 2)), np.zeros((12, 3))), {}),
    "1-D": ((np.zeros(10), np.zeros((10, 1))), {}),
    "empty": ((np.zeros((0, 2)), np.zeros((10, 2))), {}),
    "strings": ((np.array([["a", "b"]] * 8), np.zeros((8, 2))), {}),
    "standardize=1": (OK, dict(standardize=1)),
    "standardize=None": (OK, dict(standardize=None)),
    "squared=0": (OK, dict(squared=0)),
    "squared='yes'": (OK, dict(squared="yes")),
}
BAD_BOOT = {
    "n_iters=0": (OK, dict(n_iters=0)),
    "n_iters=True": (OK, dict(n_iters=True)),
    "n_iters=2.5": (OK, dict(n_iters=2.5)),
}


@pytest.mark.parametrize("bad", list(BAD) + list(BAD_BOOT))
def test_argument_errors_raise_value_error_before_any_draw(bad):
    (X, Y), kw = {**BAD, **BAD_BOOT}[bad]
    fns = [energy_mod.energy_distance] + ([energy_mod.energy_distance_full_sample] if bad in BAD else [])
    if "squared" not in kw:
        fns.append(energy_mod.REPLICATES["energy_distance"])
    np.random.seed(3)
    want = np.random.random()
    for fn in fns:
        np.random.seed(3)
        with pytest.raises(ValueError):
            fn(X, Y, **kw)
        assert np.random.random() == want


def test_signatures():
    assert str(inspect.signature(energy_mod.energy_distance)) == "(X_real, X_fake, n_iters=100, standardize=False, squared=False)"
    assert str(inspect.signature(energy_mod.energy_distance_full_sample)) == "(X_real, X_fake, standardize=False, squared=False)"
    assert list(energy_mod.REPLICATES) == ["energy_distance"]


def _run(code):
    env = dict(os.environ, PYTHONPATH=ROOT, HIP_VISIBLE_DEVICES="")
    return subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)


def test_import_needs_no_gpu_loads_nothing_and_widens_no_export_list():
    r = _run("from probaforms_amd.metrics.energy import energy_distance, energy_distance_full_sample, REPLICATES\n"
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
    assert {"pfm_energy", "pfm_energy_workspace_bytes"} <= set(_lib.EXPORTS)
    assert "#define PFM_VERSION %d " % _lib.ABI_VERSION in raw and _lib.ABI_VERSION == 101
    assert re.search(r"#define PFM_ENERGY_TILE %d\s" % _lib.ENERGY_TILE, raw)
    assert re.search(r"#define PFM_ENERGY_REP_BLOCK %d\s" % _lib.ENERGY_REP_BLOCK, raw)
    assert _lib.ENERGY_TILE >= 2 and _lib.ENERGY_REP_BLOCK >= 2


def test_workspace_query_and_argument_statuses_without_a_device():
    native_libs.ensure_built(_lib)
    q = _lib.energy_workspace_bytes
    assert q(30, 20, 2, 3) > 0 and q(1, 1, 1, 1) > 0 and q(30, 20, 2, 65535) > 0
    for bad in ((0, 20, 2, 3), (30, 0, 2, 3), (30, 20, 0, 3), (30, 20, 2, 0), (30, 20, 2, 65536), (-1, 20, 2, 3),
                (30, 20, 2, -1), (2 ** 31, 20, 2, 3), (30, 2 ** 31, 2, 3), (2 ** 30, 2 ** 30, 2 ** 40, 3)):
        assert q(*bad) == 0, bad
    # the draw counts and the partials: nothing of the size of the pair matrix, and counted per replicate
    n = 10000
    assert q(n, n, 16, 100) < 100 * (4 * 2 * n) + (8 << 20) and q(n, n, 16, 100) < 8 * (2 * n) ** 2 // 100
    for nr, nf, d in ((30, 20, 2), (3000, 2500, 5)):
        assert q(nr, nf, d, 7) <= 7 * q(nr, nf, d, 1)
        assert q(nr, nf, d, 7) == q(nr, nf, d + 9, 7)                   # the decomposition does not depend on d
    # refused before anything is read or launched (the pointers are never dereferenced)
    L, fake = _lib.lib(), ctypes.c_void_p(256)

    def call(nr=30, nf=20, d=2, reps=3, Xr=fake, Xf=fake, ir=fake, jf=fake, sums=fake, ws=fake, nbytes=1 << 30):
        return L.pfm_energy(None, Xr, nr, Xf, nf, d, ir, jf, reps, sums, ws, nbytes)

    assert call(Xr=None) == _lib.PFM_EINVAL and call(Xf=None) == _lib.PFM_EINVAL and call(sums=None) == _lib.PFM_EINVAL
    assert call(ir=None) == _lib.PFM_EINVAL and call(jf=None) == _lib.PFM_EINVAL
    assert call(nr=0) == _lib.PFM_EINVAL and call(nf=0) == _lib.PFM_EINVAL and call(d=0) == _lib.PFM_EINVAL
    assert call(reps=0) == _lib.PFM_EINVAL and call(reps=65536) == _lib.PFM_EINVAL
    assert call(nbytes=q(30, 20, 2, 3) - 1) == _lib.PFM_EWORKSPACE and call(ws=None) == _lib.PFM_EWORKSPACE
