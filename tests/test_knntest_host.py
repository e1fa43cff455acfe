"""probaforms_amd.metrics.twosample.knn_test without a GPU: the C header against the binding, the workspace queries and the
argument statuses of pfm_nn_index / pfm_nn_count, the restatement (tests/knntest_numpy.py: cdist and a stable argsort) against
scipy's cKDTree, the condition under which a continuous data set's neighbours are the same for any way of accumulating d^2, the
committed fixtures (tests/golden/knntest_*.npz, regenerated bit for bit), the null distribution's mean, and the argument checks
of the public calls before any draw and before any device is asked for.

The gap condition.  The kernel accumulates d^2 with fused multiply-adds and cdist without, so each is within d 2^-53 relative of
the exact value.  Where consecutive squared distances among a row's first k + 1 neighbours differ by 1e-9 relative at least, six
orders of magnitude above that, both order the neighbours alike and the GPU tests may compare row indices byte for byte.  On
integer data both are exact, ties are real ties and the (d^2, index) order is fully determined.
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
from scipy.spatial import cKDTree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, ROOT)
sys.path.insert(0, GOLDEN)

import knntest_numpy as kn  # noqa: E402
import twosample_numpy as tn  # noqa: E402
import make_golden_knntest  # noqa: E402
import native_libs  # noqa: E402
from probaforms_amd.metrics import _lib, twosample  # noqa: E402

FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "knntest_*.npz")))
NAMES = {"shift_130_93_d3_k1", "equal_130_93_d3_k5", "copy_70_70_d3_k1", "tiny_2_3_d2_k4", "clusters_standardized_k3"}
NEW = ("pfm_nn_index_workspace_bytes", "pfm_nn_index", "pfm_nn_count_workspace_bytes", "pfm_nn_count")


def fid(p):
    return os.path.basename(p)[8:-4]


# ---- header, binding, statuses ------------------------------------------------------------------------------

def test_header_constants_and_declarations_equal_the_binding():
    raw = open(os.path.join(ROOT, "probaforms_amd", "metrics", "csrc", "pf_metrics.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = re.findall(r"\b(pfm_[a-z0-9_]+)\s*\(", text)
    assert sorted(declared) == sorted(_lib.EXPORTS) and set(NEW) <= set(_lib.EXPORTS)
    assert "#define PFM_VERSION %d " % _lib.ABI_VERSION in raw and _lib.ABI_VERSION == 101
    assert re.search(r"#define PFM_NN_MAX_K %d\s" % _lib.NN_MAX_K, raw) and 8 <= _lib.NN_MAX_K <= 16
    assert re.search(r"#define PFM_NN_STAGE_MAX_N %d\s" % _lib.NN_STAGE_MAX_N, raw) and _lib.NN_STAGE_MAX_N % 64 == 0
    assert re.search(r"#define PFM_KNN_MAX_K 16\s", raw) and _lib.KNN_MAX_K == 16
    assert "pf_nn.o" in open(os.path.join(ROOT, "probaforms_amd", "metrics", "csrc", "Makefile")).read()
    assert max(kn.LIST_EDGES) == _lib.NN_MAX_K


def test_workspace_queries_and_argument_statuses_without_a_device():
    native_libs.ensure_built(_lib)
    qi, qc = _lib.nn_index_workspace_bytes, _lib.nn_count_workspace_bytes
    assert qi(2, 1, 1) > 0 and qi(20000, 16, _lib.NN_MAX_K) > 0
    for bad in ((1, 1, 1), (0, 1, 1), (10, 0, 1), (10, 2, 0), (10, 2, -1), (10, 2, 10), (2 ** 31, 2, 1), (100, 2, _lib.NN_MAX_K + 1),
                (2 ** 30, 2 ** 40, 1)):
        assert qi(*bad) == 0, bad
    assert qc(2, 1, 1) > 0 and qc(1, 1, 1) > 0 and qc(20000, 16, 65536) > 0
    for bad in ((0, 1, 1), (10, 0, 1), (10, 1, 0), (-1, 1, 1), (10, -1, 1), (10, 1, -1), (2 ** 31, 1, 1), (10, 1, 2 ** 31),
                (2 ** 30, 2 ** 40, 1)):
        assert qc(*bad) == 0, bad
    # the slices' counts only: a function of the labellings and of n k / 65536, nothing of the size of the table
    assert qc(2000, 5, 1000) <= 1000 * 16 + 256 and qc(20000, 16, 1000) <= 1000 * 16 * 5 + 256
    assert qc(5000, 5, 7) <= 7 * qc(5000, 5, 1)
    # refused before anything is read or launched (the pointers are never dereferenced)
    L, fake = _lib.lib(), ctypes.c_void_p(256)

    def index(Z=fake, n=10, d=2, k=3, nbr=fake, d2=fake, ws=fake, nbytes=1 << 20):
        return L.pfm_nn_index(None, Z, n, d, k, nbr, d2, ws, nbytes)

    assert index(Z=None) == _lib.PFM_EINVAL and index(nbr=None) == _lib.PFM_EINVAL and index(d2=None) == _lib.PFM_EINVAL
    assert index(n=1, k=1) == _lib.PFM_EINVAL and index(d=0) == _lib.PFM_EINVAL and index(k=0) == _lib.PFM_EINVAL
    assert index(k=10) == _lib.PFM_EINVAL and index(n=2 ** 31) == _lib.PFM_EINVAL
    assert index(n=100, k=_lib.NN_MAX_K + 1) == _lib.PFM_EUNSUPPORTED
    assert index(n=_lib.NN_MAX_K + 1, k=_lib.NN_MAX_K + 1) == _lib.PFM_EINVAL          # k > n - 1 comes first
    assert index(ws=None) == _lib.PFM_EWORKSPACE and index(nbytes=qi(10, 2, 3) - 1) == _lib.PFM_EWORKSPACE

    def count(nbr=fake, n=10, k=3, lab=fake, reps=4, out=fake, ws=fake, nbytes=1 << 20):
        return L.pfm_nn_count(None, nbr, n, k, lab, reps, out, ws, nbytes)

    assert count(nbr=None) == _lib.PFM_EINVAL and count(lab=None) == _lib.PFM_EINVAL and count(out=None) == _lib.PFM_EINVAL
    assert count(n=0) == _lib.PFM_EINVAL and count(k=0) == _lib.PFM_EINVAL and count(reps=0) == _lib.PFM_EINVAL
    assert count(n=-5) == _lib.PFM_EINVAL and count(n=2 ** 31) == _lib.PFM_EINVAL
    assert count(ws=None) == _lib.PFM_EWORKSPACE and count(nbytes=qc(10, 3, 4) - 1) == _lib.PFM_EWORKSPACE


# ---- the restatement ------------------------------------------------------------------------------------------

def test_restatement_on_hand_made_data():
    Z = np.array([[0.0], [1.0], [1.0], [3.0], [0.0]])
    nbr, d2 = kn.neighbours(Z, 2)
    assert nbr.dtype == np.int32 and nbr.tolist() == [[4, 1], [2, 0], [1, 0], [1, 2], [0, 1]]      # ties by row index
    assert d2.tolist() == [[0.0, 1.0], [0.0, 1.0], [0.0, 1.0], [4.0, 4.0], [0.0, 1.0]]
    assert kn.min_gap(Z, 2) == 0.0
    L = np.array([[1, 1, 0, 0, 1], [0, 0, 0, 0, 0], [1, 1, 1, 1, 1]], np.uint8)
    assert kn.counts(nbr, L).tolist() == [[5, 1], [0, 10], [10, 0]]
    assert kn.shares(kn.counts(nbr, L[:1]), 3, 2, 2).tolist() == [[6 / 10, 5 / 6, 1 / 4]]
    assert kn.expected_null(3, 2) == (6 + 2) / 20 and kn.expected_null(50, 50) == 49 / 99


@pytest.mark.parametrize("nr,nf,d,k", kn.INDEX_CASES + [kn.CKDTREE_CASE])
def test_continuous_data_meets_the_gap_condition_and_ckdtree_agrees(nr, nf, d, k):
    Z = tn.data(nr, nf, d)
    gap = kn.min_gap(Z, k)
    print("smallest relative gap %.3g" % gap)
    assert gap >= kn.GAP
    nbr, d2 = kn.neighbours(Z, k)
    assert ((nbr != np.arange(len(Z))[:, None]).all()) and (np.diff(d2, axis=1) > 0).all()
    dist, idx = cKDTree(Z).query(Z, k=k + 1)
    assert (idx[:, 0] == np.arange(len(Z))).all()                          # no duplicates: the row itself comes first
    assert np.array_equal(idx[:, 1:], nbr)
    assert np.allclose(dist[:, 1:] ** 2, d2, rtol=1e-12, atol=0)


def test_the_other_data_sets():
    for desc in (True, False):
        Z = kn.line(desc)
        assert kn.min_gap(Z, 16) >= kn.GAP
        nbr, _ = kn.neighbours(Z, 3)
        assert nbr[0].tolist() == ([299, 298, 297] if desc else [1, 2, 3])
    n, ks = kn.MOD7
    nbr, d2 = kn.neighbours(kn.mod7(n), max(ks))
    assert (d2 == 0.0).all() and nbr[0].tolist()[:3] == [7, 14, 21] and nbr[8].tolist()[:3] == [1, 15, 22]
    Z = tn.integer_data(*kn.INTEGER)
    D = np.abs(Z - Z.T) ** 2
    assert np.array_equal(D, np.round(D)) and D.max() < 2 ** 53                 # exact: ties are real ties
    assert kn.min_gap(tn.data(*tn.OTHER[0]), max(kn.LIST_EDGES)) >= kn.GAP      # the shape every list length is run at
    X = tn.data(70, 1, 3)[:70]
    assert kn.min_gap(X, 2) >= kn.GAP                                          # the copied sample of the public tests
    nbr, d2 = kn.neighbours(np.concatenate([X, X]), 1)
    assert (nbr[:, 0] == (np.arange(140) + 70) % 140).all() and (d2 == 0.0).all()


# ---- the fixtures ---------------------------------------------------------------------------------------------

def test_fixtures_exist_and_are_small():
    assert {fid(p) for p in FIXTURES} == NAMES
    assert all(os.path.getsize(p) <= 10000 for p in FIXTURES)


def test_fixtures_regenerate_bit_for_bit():
    made = make_golden_knntest.cases()
    assert set(made) == NAMES
    for name, arrays in made.items():
        f = np.load(os.path.join(GOLDEN, "knntest_%s.npz" % name))
        assert sorted(f.files) == sorted(arrays)
        for key, want in arrays.items():
            want = np.asarray(want)
            assert f[key].dtype == want.dtype and f[key].shape == want.shape and f[key].tobytes() == want.tobytes(), (name, key)


@pytest.mark.parametrize("path", FIXTURES, ids=fid)
def test_restatement_reproduces_the_fixture(path):
    f = np.load(path)
    X, Y, P, k = f["X"], f["Y"], int(f["n_permutations"]), int(f["nearest_k"])
    Xs, Ys = tn.standardize(X, Y) if bool(f["standardize"]) else (X, Y)
    if not fid(path).startswith("copy"):
        assert kn.min_gap(np.concatenate([Xs, Ys]), k) >= kn.GAP
    np.random.seed(int(f["seed"]))
    o = kn.test(Xs, Ys, P, k)
    assert o["next"] == float(f["next"])
    for key in ("statistic", "real", "fake", "pvalue"):
        assert o[key] == f[key] and f[key].dtype == np.float64 and f[key].shape == (), key
    assert np.array_equal(o["null"], f["null"]) and f["null"].shape == (P,)
    nr, nf = len(X), len(Y)
    if fid(path).startswith("copy"):
        assert f["statistic"] == 0.0 and f["pvalue"] == 1.0 and (f["null"] > 0).all()
    if fid(path).startswith("shift"):
        assert f["pvalue"] == 1 / 200 and f["statistic"] > f["null"].max()
    if fid(path).startswith("tiny"):             # k = N - 1: every other row is a neighbour, whatever the labelling
        assert f["statistic"] == kn.expected_null(nr, nf) and (f["null"] == f["statistic"]).all() and f["pvalue"] == 1.0


def test_the_nulls_mean_is_the_expected_statistic():
    nr, nf, d = tn.OTHER[0]
    assert (nr, nf, d) == (130, 93, 3)
    for k in (1, 5):
        nbr, _ = kn.neighbours(tn.data(nr, nf, d), k)
        V = kn.shares(kn.counts(nbr, tn.labels(kn.SEED, 0, 2000, nr + nf, nr)), nr, nf, k)[:, 0]
        se = V.std(ddof=1) / np.sqrt(len(V))
        print("k %d: null mean %.5f, expected %.5f, standard error %.2g" % (k, V.mean(), kn.expected_null(nr, nf), se))
        assert abs(V.mean() - kn.expected_null(nr, nf)) <= 3 * se


# ---- the public calls, as far as they go without a device -----------------------------------------------------------

def test_shares_of_and_signatures():
    C = np.array([[5, 1], [0, 0], [6, 4]], np.int64)
    assert twosample.shares_of(C, 3, 2, 2).tobytes() == kn.shares(C, 3, 2, 2).tobytes()
    assert twosample.shares_of(C, 3, 2, 2)[2].tolist() == [1.0, 1.0, 1.0]
    assert str(inspect.signature(twosample.knn_test)) == "(X_real, X_fake, n_permutations=999, nearest_k=1, standardize=False)"
    assert str(inspect.signature(twosample.nn_accuracy_full_sample)) == "(X_real, X_fake, nearest_k=1, standardize=False)"
    assert twosample.KnnTest._fields == ("statistic", "pvalue", "null", "real", "fake")
    assert twosample.NnAccuracy._fields == ("total", "real", "fake")


OK = (np.arange(40.0).reshape(20, 2), np.arange(36.0).reshape(18, 2) + 0.5)
BAD = {
    "NaN": ((np.array([[0.0, np.nan]] * 8), np.zeros((8, 2))), {}),
    "inf": ((np.zeros((8, 2)), np.array([[np.inf, 0.0]] * 8)), {}),
    "features": ((np.zeros((10, 2)), np.zeros((12, 3))), {}),
    "1-D": ((np.zeros(10), np.zeros((10, 1))), {}),
    "empty": ((np.zeros((0, 2)), np.zeros((10, 2))), {}),
    "strings": ((np.array([["a", "b"]] * 8), np.zeros((8, 2))), {}),
    "standardize=1": (OK, dict(standardize=1)),
    "nearest_k=0": (OK, dict(nearest_k=0)),
    "nearest_k=-1": (OK, dict(nearest_k=-1)),
    "nearest_k=True": (OK, dict(nearest_k=True)),
    "nearest_k=2.0": (OK, dict(nearest_k=2.0)),
    "nearest_k=None": (OK, dict(nearest_k=None)),
    "nearest_k=nr+nf": ((OK[0][:4], OK[1][:3]), dict(nearest_k=7)),
    "nearest_k=NN_MAX_K+1": (OK, dict(nearest_k=_lib.NN_MAX_K + 1)),
}
BAD_PERMUTATIONS = {
    "n_permutations=0": (OK, dict(n_permutations=0)),
    "n_permutations=True": (OK, dict(n_permutations=True)),
    "n_permutations=2.5": (OK, dict(n_permutations=2.5)),
    "n_permutations=None": (OK, dict(n_permutations=None)),
}


@pytest.mark.parametrize("bad", list(BAD) + list(BAD_PERMUTATIONS))
def test_argument_errors_raise_value_error_before_any_draw(bad, monkeypatch):
    import torch
    (X, Y), kw = {**BAD, **BAD_PERMUTATIONS}[bad]
    fns = [twosample.knn_test] + ([twosample.nn_accuracy_full_sample] if bad in BAD else [])

    def no_device(*a, **k):
        raise AssertionError("a device was asked for")

    monkeypatch.setattr(torch.cuda, "is_available", no_device)
    monkeypatch.setattr(torch.cuda, "current_device", no_device)
    np.random.seed(3)
    want = np.random.random()
    for fn in fns:
        np.random.seed(3)
        with pytest.raises(ValueError):
            fn(X, Y, **kw)
        assert np.random.random() == want


def test_import_needs_no_gpu_loads_nothing_and_widens_no_export_list():
    env = dict(os.environ, PYTHONPATH=ROOT, HIP_VISIBLE_DEVICES="")
    code = ("from probaforms_amd.metrics.twosample import knn_test, nn_accuracy_full_sample, KnnTest, NnAccuracy\n"
            "from probaforms_amd.metrics import _lib\n"
            "import probaforms_amd.metrics as m\n"
            "assert _lib.LIBRARY.loaded is False\n"
            "assert m.__all__ == ['frechet_distance', 'maximum_mean_discrepancy']\n"
            "print('ok')")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr
