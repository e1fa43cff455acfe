"""sample_joint_scores: everything that needs no GPU -- the binding against the header's text, pfp_joint_tiling, argument
validation, the numpy host route (joint_scores_of_draws) against the yardstick of tests/joint_scores_numpy.py, the non-finite
rules, and pfp_joint_scores' argument errors."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import joint_scores_numpy as JN
import native_libs
import scores_numpy as SN
from probaforms_amd.models import _predict_lib

native_libs.ensure_built(_predict_lib)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "probaforms_amd", "models", "predict_csrc", "pf_predict.h")
ORDERS = (0.5, 1.0, 2.0)


# ---- the header, the binding, the library -------------------------------------------------------------------------
def test_header_declares_what_the_binding_exports():
    from probaforms_amd.models import _predict_lib as pl
    with open(HEADER) as f:
        raw = f.read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(pfp_[a-z_]+)\s*\(", text))
    assert declared == set(pl.EXPORTS)
    assert {"pfp_joint_scores", "pfp_joint_tiling"} <= declared
    for name, count in (("pfp_joint_scores", 11), ("pfp_joint_tiling", 3)):
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, text)
        assert len([p for p in m.group(1).split(",") if p.strip()]) == count == len(pl._SIGNATURES[name][1]), name
    assert pl._SIGNATURES["pfp_joint_scores"][1][7] is C.c_double                    # the order travels as a double
    consts = dict(re.findall(r"#define\s+(PFP_[A-Z_]+)\s+\(?(-?\d+)\)?", raw))
    assert int(consts["PFP_VERSION"]) == pl.ABI_VERSION == 101
    fields = re.search(r"typedef struct \{(.*?)\} pfp_joint_tile;", text, flags=re.S).group(1)
    assert re.findall(r"\b([a-z_]+)\s*[,;]", fields) == [n for n, _ in pl.JointTile._fields_]


def test_library_exports_both_entry_points():
    from probaforms_amd.models import _predict_lib as pl
    L = pl.lib()
    assert L.pfp_version() == 101
    assert hasattr(L, "pfp_joint_scores") and hasattr(L, "pfp_joint_tiling")


def test_joint_tiling():
    from probaforms_amd.models import _predict_lib as pl
    t = pl.joint_tiling(1, 8192)
    assert (t.n_tiles, t.tile_draws, t.n_chunks, t.chunk_cols) == (1, 8192, 1, 1)
    assert t.threads == 256 and t.max_grid >= 1 and 0 < t.budget_bytes < t.lds_bytes + t.budget_bytes <= 160 * 1024
    for d, K in ((1, 1), (1, 19), (2, 257), (16, 256), (5, 1000), (16, 300), (33, 64), (33, 309), (33, 310), (48, 1024), (2, 8192),
                 (17, 8192), (79, 8192), (80, 5), (80, 8192), (200, 70), (5000, 3), (100000, 1)):
        t = pl.joint_tiling(d, K)
        what = (d, K, t.tile_draws, t.n_tiles, t.chunk_cols, t.n_chunks)
        assert (t.n_tiles - 1) * t.tile_draws < K <= t.n_tiles * t.tile_draws, what                     # the tiles cover K
        assert (t.n_chunks - 1) * t.chunk_cols < d <= t.n_chunks * t.chunk_cols, what                   # the chunks cover d
        images = 1 if t.n_tiles == 1 and t.n_chunks == 1 else 2
        claimed = 4 * t.chunk_cols * (images * t.tile_draws + 1)                                        # the images and y
        assert claimed <= t.budget_bytes and claimed < t.lds_bytes <= 64 * 1024, what
        if t.n_tiles > 1 or t.n_chunks > 1:
            assert 4 * d * (K + 1) > t.budget_bytes and t.tile_draws % 64 == 0, what
        if t.n_chunks > 1:
            assert t.tile_draws == 64, what
        if K > 64 and 4 * d * K > t.budget_bytes:
            assert t.n_tiles >= 2, what
    assert pl.joint_tiling(48, 1024).n_tiles >= 2
    assert pl.joint_tiling(200, 70).n_chunks >= 2
    out = pl.JointTile()
    L = pl.lib()
    assert L.pfp_joint_tiling(0, 5, C.byref(out)) == -1 and L.pfp_joint_tiling(3, 0, C.byref(out)) == -1
    assert L.pfp_joint_tiling(3, 5, None) == -1
    assert L.pfp_joint_tiling(3, 8193, C.byref(out)) == pl.EUNSUPPORTED


def test_pfp_joint_scores_argument_errors_need_no_launch():
    from probaforms_amd.models import _predict_lib as pl
    fake = 4096                                   # never dereferenced: no call below reaches a launch

    def call(xt=fake, y=fake, n_rows=4, d=3, k=19, fair=0, order=0.5, e=fake, s=fake, v=fake):
        return pl.lib().pfp_joint_scores(None, xt, y, n_rows, d, k, fair, order, e, s, v)
    assert call(xt=None) == -1 and call(y=None) == -1
    assert call(n_rows=-1) == -1 and call(d=0) == -1 and call(d=-2) == -1 and call(k=0) == -1 and call(k=-5) == -1
    for order in (0.0, 0.25, 1.5, 3.0, -1.0, float("nan"), float("inf")):
        assert call(order=order) == -1
        assert call(order=order, n_rows=0, v=None) == 0                               # ignored when variogram is NULL
    assert call(k=8193) == pl.EUNSUPPORTED and call(k=1 << 40) == pl.EUNSUPPORTED
    assert call(n_rows=0) == 0 and call(n_rows=0, d=100000) == 0                      # zero rows: ok without a launch
    assert call(n_rows=0, k=8193) == pl.EUNSUPPORTED                                  # the checks come before the early return
    assert call(e=None, s=None, v=None) == 0                                          # nothing asked for: nothing launched


def test_binding_refuses_tensors_off_the_device():
    from probaforms_amd.models import _predict_lib as pl
    xt = torch.zeros(2, 3, 5)
    for y in (torch.zeros(2, 3), torch.zeros(2, 3, dtype=torch.float64), np.zeros((2, 3), np.float32), None):
        with pytest.raises(RuntimeError, match="y "):
            pl.joint_scores(xt, y, 2, 3, 5, False, 0.5, None, None, None)


# ---- validation ---------------------------------------------------------------------------------------------------
def test_validate_joint():
    from probaforms_amd.models import _predict as P
    assert P.validate_joint(19) == (19, 0.5)
    assert P.validate_joint(1, None) == (1, None)
    assert P.validate_joint(8192, 1) == (8192, 1.0) and isinstance(P.validate_joint(5, 1)[1], float)
    assert P.validate_joint(5, 2.0) == (5, 2.0) and P.validate_joint(5, np.float32(0.5)) == (5, 0.5)
    for bad in (0, -3, 2.5, 8193, True):
        with pytest.raises(ValueError):
            P.validate_joint(bad)
        with pytest.raises(ValueError):
            P.validate_joint(bad, None)
    for order in (0, 0.25, 1.5, 3, -1, float("nan"), "half", True, (0.5,)):
        with pytest.raises(ValueError):
            P.validate_joint(10, order)
    assert P.JointScores._fields == ("energy", "spread", "variogram")


# ---- the host route against the yardstick -------------------------------------------------------------------------
def _host(xt, y, fair, order):
    from probaforms_amd.models import _predict as P
    s = P.joint_scores_of_draws(np.moveaxis(xt, (1, 2), (2, 0)), y, fair, order)
    assert isinstance(s, P.JointScores)
    for a in s:
        assert a is None or (a.dtype == np.float32 and a.shape == (xt.shape[0],))
    return s


@pytest.mark.parametrize("fair", [False, True])
@pytest.mark.parametrize("d", [1, 2, 5])
@pytest.mark.parametrize("K", [1, 2, 3, 19, 257])
def test_joint_scores_of_draws_on_finite_rows(K, d, fair):
    xt, y = JN.finite(K, d)
    for order in ORDERS:
        got, ref = _host(xt, y, fair, order), JN.scores(xt, y, fair, order)
        JN.check_all(got, ref, K, d, (K, d, fair, order))
        if K == 1 and fair:
            assert np.isnan(got.energy).all() and np.isnan(got.spread).all()           # 0 / 0, as the formula gives
        else:
            assert (got.spread >= 0).all()
            if not fair:
                assert (got.energy >= 0).all()
        assert (got.variogram >= 0).all() and ((got.variogram == 0).all() if d == 1 else (got.variogram > 0).any())
    none = _host(xt, y, fair, None)
    assert none.variogram is None
    np.testing.assert_array_equal(none.energy, got.energy)
    np.testing.assert_array_equal(none.spread, got.spread)


@pytest.mark.parametrize("fair", [False, True])
@pytest.mark.parametrize("K", [1, 2, 3, 19, 257])
def test_one_column_is_the_crps(K, fair):
    """d = 1: energy is sample_scores' crps (within the sum of both bounds), spread its second term, variogram 0; and the
    yardsticks agree exactly"""
    from probaforms_amd.models import _predict as P
    xt, y = JN.finite(K, 1)
    ref, sref = JN.scores(xt, y, fair, 0.5), SN.scores(xt, y, (), fair)
    np.testing.assert_array_equal(ref.energy, sref.crps[:, 0])
    got = _host(xt, y, fair, 0.5)
    crps = P.scores_of_draws(np.moveaxis(xt, -1, 0), y, None, fair).crps[:, 0]
    tol = JN.bound_pairs(ref.energy, ref, K, 1) + SN.bound(sref.crps[:, 0], K, SN.scale_of(xt, y)[:, 0])
    assert np.array_equal(np.isnan(got.energy), np.isnan(crps))
    ok = ~np.isnan(crps)
    assert (np.abs(got.energy.astype(np.float64) - crps)[ok] <= tol[ok]).all()
    assert (got.variogram == 0).all()


@pytest.mark.parametrize("fair", [False, True])
@pytest.mark.parametrize("K", [1, 2, 3, 19, 257])
def test_nonfinite_table_through_the_host_route(K, fair):
    xt, y = JN.nonfinite(K)
    d = xt.shape[1]
    for order in ORDERS + (None,):
        got, ref = _host(xt, y, fair, order), JN.scores(xt, y, fair, order)
        JN.check_all(got, ref, K, d, (K, fair, order))
        JN.table(K, fair, *got)
        if order is not None:
            JN.table(K, fair, ref.energy, ref.spread, ref.variogram)
        alone = _host(xt[-1:], y[-1:], fair, order)                                    # nothing leaves its row
        for a, b in zip(got, alone):
            assert (a is None) == (b is None)
            if a is not None:
                np.testing.assert_array_equal(a[-1:], b)


@pytest.mark.parametrize("K", [19, 257])
def test_comonotone_against_shuffled(K):
    """the same marginals, another dependence: the per-column scores cannot tell, the joint scores can"""
    from probaforms_amd.models import _predict as P
    xt, sh, y = JN.comonotone(K)
    a, b = _host(xt, y, False, 0.5), _host(sh, y, False, 0.5)
    ca = P.scores_of_draws(np.moveaxis(xt, -1, 0), y, None, False).crps
    cb = P.scores_of_draws(np.moveaxis(sh, -1, 0), y, None, False).crps
    np.testing.assert_array_equal(ca.view(np.uint32), cb.view(np.uint32))
    assert a.variogram[0] == 0 and b.variogram[0] > 0
    assert b.energy[0] > a.energy[0]


def test_joint_scores_of_draws_refuses_a_wrong_target_shape():
    from probaforms_amd.models import _predict as P
    X = np.zeros((7, 4, 3), np.float32)
    for shape in ((4,), (3, 4), (4, 2), (1, 4, 3), (5, 3)):
        with pytest.raises(ValueError):
            P.joint_scores_of_draws(X, np.zeros(shape, np.float32), False, 0.5)
    s = P.joint_scores_of_draws(np.zeros((7, 0, 3), np.float32), np.zeros((0, 3), np.float32), False, 0.5)
    assert s.energy.shape == s.spread.shape == s.variogram.shape == (0,) and s.energy.dtype == np.float32
    t = P.joint_scores_of_draws(X, torch.zeros(4, 3).numpy().tolist(), False, None)   # array-like targets
    assert (t.energy == 0).all() and (t.spread == 0).all() and t.variogram is None


def test_blocked_pair_sum_holds_no_k_by_k_by_d_array(monkeypatch):
    """a small block budget walks the same pairs: the result moves by rounding only"""
    from probaforms_amd.models import _predict as P
    K, d = 300, 4
    xt, y = JN.finite(K, d)
    one = _host(xt, y, False, 1.0)
    monkeypatch.setattr(P, "PAIR_BLOCK_ELEMS", 1000)
    two = _host(xt, y, False, 1.0)
    JN.check_all(two, JN.scores(xt, y, False, 1.0), K, d, "small blocks")
    np.testing.assert_allclose(two.energy, one.energy, rtol=1e-6)


# ---- the public call without a GPU: the host route of a layer-wise flow -------------------------------------------
def test_public_call_falls_back_to_the_notebook_loop():
    from probaforms_amd.models import RealNVP
    from probaforms_amd.models import _predict as P
    from test_predict_host import _flow
    m = RealNVP()
    m.nf = _flow([(8,), (12,)])
    rng = np.random.default_rng(3)
    calls = []

    def fake_sample(Cn):
        calls.append(len(Cn))
        return rng.standard_normal((len(Cn), 3)).astype(np.float32)

    m.sample = fake_sample
    Cn = np.zeros((4, 2), np.float32)
    Y = np.random.default_rng(4).standard_normal((4, 3)).astype(np.float32)
    js = m.sample_joint_scores(Cn, Y, 7, fair=True, variogram_order=1)
    assert calls == [4] * 7 and isinstance(js, P.JointScores)
    rng = np.random.default_rng(3)
    X = np.array([rng.standard_normal((4, 3)).astype(np.float32) for _ in range(7)])
    JN.check_all(js, JN.scores_of_stacked(X, Y, True, 1.0), 7, 3, "fallback")
    assert m.sample_joint_scores(Cn, Y, 7, variogram_order=None).variogram is None
    for kw in (dict(n_draws=0), dict(n_draws=8193), dict(n_draws=5, variogram_order=0.3)):
        with pytest.raises(ValueError):
            m.sample_joint_scores(Cn, Y, **kw)
    with pytest.raises(ValueError):
        m.sample_joint_scores(Cn, Y[:, :2], 5)
