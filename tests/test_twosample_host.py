"""probaforms_amd.metrics.twosample without a GPU: the Philox restatement (tests/twosample_numpy.py) against the Random123 known
answers, the labellings' counts under every key mask, the kernel's order of summation against the einsum order at every shape the
GPU tests use, the committed fixtures (tests/golden/twosample_*.npz, regenerated bit for bit), argument checks before any draw,
importing without a GPU, the C header against the binding and the workspace queries.

Why the GPU tests' bound is safe.  S = sum_ab s[a] s[b] G(a, b) cancels (it is -(nr nf)^2 D^2, while its terms are of the size of
(nr nf)^2 times a distance), so a relative bound on S would not hold for any order of summation.  The kernel and the restatement
add the same terms in float64 in different orders, so each is within (additions in a chain) 2^-53 of the exact sum RELATIVE TO THE
SUM OF THE TERMS' MAGNITUDES A = sum_ab |s[a] s[b]| G(a, b); test_the_two_summation_orders_agree measures the two orders against
each other at every shape and stays below 1e-14 A, two orders of magnitude inside the GPU tests' bound of 1e-12 A.
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

import twosample_numpy as tn  # noqa: E402
import make_golden_twosample  # noqa: E402
import native_libs  # noqa: E402
from probaforms_amd.metrics import _lib, twosample  # noqa: E402

FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "twosample_*.npz")))
MADE_HERE = {"shift_130_93_d3", "equal_130_93_d3", "integer_65_63_d1", "tiny_1_2_d1", "clusters_standardized"}
NAMES = MADE_HERE | {"mmd_reference"}


def fid(p):
    return os.path.basename(p)[10:-4]


def test_philox_known_answers():
    for counter, key, want in tn.KNOWN_ANSWERS:
        assert tuple(int(v) for v in tn.philox4x32_10(counter, key)) == want
    # vectorised over the counter's first word, as keys() uses it
    many = tn.philox4x32_10((np.array([0, 0xffffffff, 0x243f6a88], np.uint64), 0, 0, 0), (0, 0))
    assert int(many[0][0]) == 0x6627e8d5 and many[0].shape == (3,)


@pytest.mark.parametrize("N,nr", tn.LABEL_CASES)
def test_every_labelling_has_nr_ones(N, nr):
    for mask in tn.MASKS:
        L = tn.labels(tn.SEED, 3, 6, N, nr, mask)
        assert L.dtype == np.uint8 and L.shape == (6, N) and set(np.unique(L)) <= {0, 1}
        assert (L.sum(axis=1) == nr).all(), mask
        if mask == 0:
            assert (L == tn.observed(N, nr)[None]).all()
        if mask == 3 and N >= 64:
            k = tn.keys(tn.SEED, 3, N, mask)
            assert k.max() <= 3 and np.bincount(k.astype(np.int64)).max() >= N // 8       # ties, many-fold
    if N >= 255:                                       # labellings differ from one another and from the observed one
        L = tn.labels(tn.SEED, 0, 3, N, nr)
        assert not (L[0] == L[1]).all() and not (L[0] == tn.observed(N, nr)).all()
        assert (tn.labels(tn.SEED, 2, 1, N, nr)[0] == L[2]).all()


def test_fixtures_exist_and_are_small():
    assert {fid(p) for p in FIXTURES} == NAMES
    largest_energy = max(os.path.getsize(p) for p in glob.glob(os.path.join(GOLDEN, "energy_*.npz")))
    assert all(os.path.getsize(p) <= largest_energy for p in FIXTURES)


def test_fixtures_regenerate_bit_for_bit():
    made = make_golden_twosample.cases()
    assert set(made) == MADE_HERE
    for name, arrays in made.items():
        f = np.load(os.path.join(GOLDEN, "twosample_%s.npz" % name))
        assert sorted(f.files) == sorted(arrays)
        for key, want in arrays.items():
            want = np.asarray(want)
            assert f[key].dtype == want.dtype and f[key].shape == want.shape and f[key].tobytes() == want.tobytes(), (name, key)


@pytest.mark.parametrize("path", FIXTURES, ids=fid)
def test_restatement_reproduces_the_fixture(path):
    f = np.load(path)
    X, Y, P = f["X"], f["Y"], int(f["n_permutations"])
    Xs, Ys = tn.standardize(X, Y) if bool(f["standardize"]) else (X, Y)
    med = tn.median(Xs, Ys)
    assert abs(med - float(f["median"])) <= 1e-14 * med
    for name, kind, gamma in (("energy", tn.ENERGY, 0.0), ("mmd", tn.GAUSS, 1.0 / (2 * float(f["median"]) ** 2))):
        np.random.seed(int(f["seed"]))
        o = tn.test(Xs, Ys, P, kind, gamma)
        assert o["next"] == float(f["next"])
        assert abs(o["statistic"] - f[name + "_statistic"]) <= o["bound"][0]
        assert np.array_equal(o["null"], f[name + "_null"]) and f[name + "_null"].shape == (P,)
        assert float(f[name + "_pvalue"]) == tn.pvalue(f[name + "_statistic"], f[name + "_null"]) == o["pvalue"]
    if fid(path).startswith("shift"):
        assert float(f["energy_pvalue"]) == float(f["mmd_pvalue"]) == 1 / 200
        assert f["energy_statistic"] > 2 * f["energy_null"].max()
    if fid(path).startswith("integer"):
        S = f["energy_null"] * np.float64((65 * 63) ** 2)
        assert np.array_equal(S, np.round(S))


@pytest.mark.parametrize("kind", [tn.ENERGY, tn.GAUSS], ids=["energy", "gauss"])
def test_the_two_summation_orders_agree(kind):
    """the kernel's tile order against the einsum order, relative to the sum of magnitudes A"""
    shapes = [(nr, nf, d) for nr, nf in tn.FORM_SHAPES for d in tn.FORM_DS] + [tn.LARGE[:3], tn.INTEGER] + tn.OTHER
    shapes += [(65, 63, 3), (120, 100, 3), (70, 58, 4)]          # and the fixtures'
    worst = 0.0
    for nr, nf, d in shapes:
        Z = tn.integer_data(nr, nf, d) if (nr, nf, d) == tn.INTEGER else tn.data(nr, nf, d)
        L = np.concatenate([tn.observed(nr + nf, nr)[None], tn.labels(tn.SEED, 0, 2, nr + nf, nr)])
        S, A = tn.form(Z, L, nr, kind, tn.gamma_of(d))
        St = tn.form_tiles(Z, L, nr, kind, tn.gamma_of(d))
        rel = np.abs(St - S) / A
        worst = max(worst, rel.max())
        assert (rel <= 1e-14).all(), (nr, nf, d)
        if (nr, nf, d) == tn.INTEGER and kind == tn.ENERGY:
            assert np.array_equal(S, St) and np.array_equal(S, np.round(S)) and A.max() < 2 ** 53
    print("largest |tile order - einsum order| / A = %.3g" % worst)


def test_values_and_pvalue():
    S = np.array([-8.0, 0.0, -0.0, 4.0])
    for kind, sign in ((tn.ENERGY, -1.0), (tn.GAUSS, 1.0)):
        V = twosample.values_of(S, 2, 1, kind)
        assert np.array_equal(V, sign * S / 4.0) and not np.signbit(V[1]) and not np.signbit(V[2])
        assert V.tobytes() == tn.values(S, 2, 1, kind).tobytes()
    null = np.array([0.5, 1.0, 2.0, 1.0])
    assert twosample.pvalue_of(1.0, null) == 4 / 5 == tn.pvalue(1.0, null)
    assert twosample.pvalue_of(3.0, null) == 1 / 5 and twosample.pvalue_of(0.0, null) == 1.0
    assert isinstance(twosample.pvalue_of(1.0, null), np.float64)
    assert twosample.group_size(1000, 200, 64) == 1000 and twosample.group_size(1000, 1 << 40, 64) == 1


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
    "n_permutations=0": (OK, dict(n_permutations=0)),
    "n_permutations=True": (OK, dict(n_permutations=True)),
    "n_permutations=2.5": (OK, dict(n_permutations=2.5)),
    "n_permutations=-3": (OK, dict(n_permutations=-3)),
}
BAD_BANDWIDTH = {
    "bandwidth=0": (OK, dict(bandwidth=0.0)),
    "bandwidth=-1": (OK, dict(bandwidth=-1.0)),
    "bandwidth=inf": (OK, dict(bandwidth=float("inf"))),
    "bandwidth=nan": (OK, dict(bandwidth=float("nan"))),
    "bandwidth='1'": (OK, dict(bandwidth="1")),
    "bandwidth=True": (OK, dict(bandwidth=True)),
}


@pytest.mark.parametrize("bad", list(BAD) + list(BAD_BANDWIDTH))
def test_argument_errors_raise_value_error_before_any_draw(bad, monkeypatch):
    import torch
    (X, Y), kw = {**BAD, **BAD_BANDWIDTH}[bad]
    fns = [twosample.mmd_test] + ([twosample.energy_test] if bad in BAD else [])

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


def test_signatures():
    assert str(inspect.signature(twosample.energy_test)) == "(X_real, X_fake, n_permutations=999, standardize=False)"
    assert str(inspect.signature(twosample.mmd_test)) == "(X_real, X_fake, n_permutations=999, standardize=False, bandwidth=None)"
    assert twosample.TwoSampleTest._fields == ("statistic", "pvalue", "null")


def _run(code):
    env = dict(os.environ, PYTHONPATH=ROOT, HIP_VISIBLE_DEVICES="")
    return subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)


def test_import_needs_no_gpu_loads_nothing_and_widens_no_export_list():
    r = _run("from probaforms_amd.metrics.twosample import energy_test, mmd_test, TwoSampleTest\n"
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


def test_header_constants_and_declarations_equal_the_binding():
    header = os.path.join(ROOT, "probaforms_amd", "metrics", "csrc", "pf_metrics.h")
    raw = open(header).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = re.findall(r"\b(pfm_[a-z0-9_]+)\s*\(", text)
    assert sorted(set(declared)) == sorted(_lib.EXPORTS) and len(declared) == len(_lib.EXPORTS)
    assert {"pfm_perm_labels", "pfm_perm_labels_workspace_bytes", "pfm_perm_form", "pfm_perm_form_workspace_bytes"} <= set(_lib.EXPORTS)
    assert "#define PFM_VERSION %d " % _lib.ABI_VERSION in raw and _lib.ABI_VERSION == 101
    assert re.search(r"#define PFM_PERM_ENERGY %d\s" % _lib.PERM_ENERGY, raw)
    assert re.search(r"#define PFM_PERM_GAUSS\s+%d\s" % _lib.PERM_GAUSS, raw)
    assert (_lib.PERM_ENERGY, _lib.PERM_GAUSS) == (tn.ENERGY, tn.GAUSS) and _lib.KEY_MASK_ALL == tn.ALL == 2 ** 64 - 1
    assert tn.TILE == _lib.ENERGY_TILE
    src = open(os.path.join(ROOT, "probaforms_amd", "metrics", "csrc", "pf_quadform.h")).read()
    assert re.search(r"MIN_LIST = %d;" % tn.MIN_LIST, src) and re.search(r"TARGET_WGS = %d;" % tn.TARGET_WGS, src)
    assert "pf_perm.o" in open(os.path.join(ROOT, "probaforms_amd", "metrics", "csrc", "Makefile")).read()


def test_workspace_queries_and_argument_statuses_without_a_device():
    native_libs.ensure_built(_lib)
    ql, qf = _lib.perm_labels_workspace_bytes, _lib.perm_form_workspace_bytes
    assert ql(1, 2, 1) > 0 and ql(1000, 20000, 10000) > 0
    for bad in ((0, 10, 5), (-1, 10, 5), (3, 1, 1), (3, 10, 0), (3, 10, 10), (3, 10, 11), (3, 2 ** 31, 5), (2 ** 31, 10, 5)):
        assert ql(*bad) == 0, bad
    assert qf(2, 1, 1, 1) > 0 and qf(20000, 16, 10000, 1000) > 0
    for bad in ((1, 2, 1, 3), (10, 0, 5, 3), (10, 2, 0, 3), (10, 2, 10, 3), (10, 2, 5, 0), (10, 2, 5, -1), (2 ** 31, 2, 5, 3),
                (10, 2, 5, 65535 * 128 + 1), (2 ** 30, 2 ** 40, 5, 3)):
        assert qf(*bad) == 0, bad
    # the partials only: nothing of the size of the pair matrix, counted per labelling, and no function of d
    n = 20000
    assert qf(n, 16, n // 2, 1000) <= 1000 * 8 * 2048 + 256 and qf(n, 16, n // 2, 1000) < 8 * n * n // 100
    assert qf(5500, 5, 3000, 7) <= 7 * qf(5500, 5, 3000, 1) and qf(5500, 5, 3000, 7) == qf(5500, 14, 2000, 7)
    # refused before anything is read or launched (the pointers are never dereferenced)
    L, fake = _lib.lib(), ctypes.c_void_p(256)

    def labels(first=0, reps=3, n=10, nr=5, out=fake, ws=fake, nbytes=1 << 20):
        return L.pfm_perm_labels(None, 1, tn.ALL, first, reps, n, nr, out, ws, nbytes)

    assert labels(out=None) == _lib.PFM_EINVAL and labels(reps=0) == _lib.PFM_EINVAL and labels(n=1, nr=1) == _lib.PFM_EINVAL
    assert labels(nr=0) == _lib.PFM_EINVAL and labels(nr=10) == _lib.PFM_EINVAL and labels(first=-1) == _lib.PFM_EINVAL
    assert labels(first=2 ** 32 - 2) == _lib.PFM_EINVAL
    assert labels(ws=None) == _lib.PFM_EWORKSPACE and labels(nbytes=ql(3, 10, 5) - 1) == _lib.PFM_EWORKSPACE

    def form(kind=tn.ENERGY, gamma=0.0, Z=fake, n=10, d=2, nr=5, lab=fake, reps=3, S=fake, ws=fake, nbytes=1 << 20):
        return L.pfm_perm_form(None, kind, gamma, Z, n, d, nr, lab, reps, S, ws, nbytes)

    assert form(Z=None) == _lib.PFM_EINVAL and form(lab=None) == _lib.PFM_EINVAL and form(S=None) == _lib.PFM_EINVAL
    assert form(n=1, nr=1) == _lib.PFM_EINVAL and form(d=0) == _lib.PFM_EINVAL and form(reps=0) == _lib.PFM_EINVAL
    assert form(nr=0) == _lib.PFM_EINVAL and form(nr=10) == _lib.PFM_EINVAL
    assert form(kind=2) == _lib.PFM_EUNSUPPORTED and form(kind=-1) == _lib.PFM_EUNSUPPORTED
    for g in (0.0, -1.0, float("inf"), float("nan")):
        assert form(kind=tn.GAUSS, gamma=g) == _lib.PFM_EINVAL, g
    assert form(ws=None) == _lib.PFM_EWORKSPACE and form(nbytes=qf(10, 2, 5, 3) - 1) == _lib.PFM_EWORKSPACE
