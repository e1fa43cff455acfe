"""pfp_joint_scores (models/predict_csrc/pf_predict.h) and sample_joint_scores of the four models on the GPU, against the
O(K^2 d) numpy yardstick of tests/joint_scores_numpy.py.  Runs on the GPU box: `pytest -m gpu`.

Tolerances (joint_scores_numpy.bound_pairs / bound_variogram; derived, u = 2^-53): energy and spread lie within
ulp32(ref) + (K^2 / 2 + d + 8) u (T1 + spread) of the float64 value, variogram within ulp32(ref) + (K + d^2 + 16) u 4 V: at
most one float32 ulp and a float64 term 10^-2 of it, which float32 differences or sums do not meet."""
import itertools

import numpy as np
import pytest
import torch

import joint_scores_numpy as JN
import native_libs
import scores_numpy as SN
from probaforms_amd.models import _cnormal_lib, _gendraw_lib, _predict_lib, _wgan_lib
from test_predict_edges_gpu import SENTINEL, _bits, _guarded, _guards_intact
from test_predict_gpu import _dev
from test_scores_gpu import MODELS, N, _public_model, _realnvp, _scores

pytestmark = pytest.mark.gpu

native_libs.ensure_built(_cnormal_lib, _gendraw_lib, _predict_lib, _wgan_lib)

ORDERS = (0.5, 1.0, 2.0)
ALL = ("energy", "spread", "variogram")


def _joint(xt, y, fair=False, order=0.5, want=ALL, bitwise_upload=False):
    """one pfp_joint_scores call -> [energy, spread, variogram] as numpy, None where not asked for"""
    from probaforms_amd.models import _predict_lib as pl
    n, d, k = xt.shape
    xd, yd = _dev(xt), _dev(y)
    if bitwise_upload:                                               # NaN signs and payloads reached the device
        np.testing.assert_array_equal(_bits(xd.cpu().numpy()), _bits(xt))
        np.testing.assert_array_equal(_bits(yd.cpu().numpy()), _bits(y))
    outs = [torch.empty(n, device="cuda") if name in want else None for name in ALL]
    pl.joint_scores(xd, yd, n, d, k, fair, order, *outs)
    torch.cuda.synchronize()
    return [None if t is None else t.cpu().numpy() for t in outs]


def _same_bits(a, b, what=None):
    for i, (u, v) in enumerate(zip(a, b)):
        assert (u is None) == (v is None), (what, i)
        if u is not None:
            np.testing.assert_array_equal(_bits(u), _bits(v), err_msg=str((what, i)))


def _tiles(d, K):
    from probaforms_amd.models import _predict_lib as pl
    t = pl.joint_tiling(d, K)
    return t.n_tiles, t.tile_draws, t.n_chunks


def _against_the_yardstick(xt, y, what, fairs=(False, True), orders=ORDERS):
    n, d, K = xt.shape
    refs = JN.scores_grid(xt, y, fairs, orders)
    for (fair, order), ref in refs.items():
        JN.check_all(_joint(xt, y, fair, order), ref, K, d, (what, K, d, fair, order))
    return refs


# ---- 1. synthetic rows against the yardstick ----------------------------------------------------------------------
# the cross product, trimmed where the yardstick is slowest: K = 1000 with d = 1, 3, 17, 33
SHAPES = [(K, d) for K in (1, 2, 3, 16, 19, 255, 256, 257, 1000) for d in (1, 2, 3, 16, 17, 33) if not (K == 1000 and d in (2, 16))]


@pytest.mark.parametrize("K,d", SHAPES)
def test_joint_scores_vs_numpy(K, d):
    xt, y = JN.finite(K, d)                                          # a tied pair of draws, a y equal to a draw, near-ties, 1e6
    refs = _against_the_yardstick(xt, y, "finite")
    if d == 1:
        assert (_joint(xt, y)[2] == 0).all()
    if K == 1:
        got = _joint(xt, y, True)
        assert np.isnan(got[0]).all() and np.isnan(got[1]).all()     # fair and one draw: 0 / 0
    assert refs


def test_joint_scores_of_the_longest_series():
    """K = 8192: one row near 0, one near 1e6 with unit spread (cancellation); d = 2 walks the row in tiles"""
    K, d = 8192, 2
    rng = np.random.default_rng(K)
    xt = np.stack([rng.standard_normal((d, K)) * 3 + 1, 1e6 + rng.standard_normal((d, K))]).astype(np.float32)
    xt[0, :, 100:200] = xt[0, :, 100:101]                            # ties
    y = np.array([xt[0, :, 100], [1e6 + 0.25] * d], np.float32)
    assert _tiles(d, K)[0] >= 2
    _against_the_yardstick(xt, y, "longest", orders=(0.5,))
    one = np.ascontiguousarray(xt[:, :1])                            # d = 1: the same K in ONE tile
    assert _tiles(1, K) == (1, K, 1)
    _against_the_yardstick(one, np.ascontiguousarray(y[:, :1]), "longest, one column", orders=(0.5,))


# ---- 3. the tiled paths -------------------------------------------------------------------------------------------
def _tile_cases():
    d = 33
    t = 128                                                          # the tile of d = 33 once a row does not fit one image
    return [(d, K) for K in (t - 1, t + 1, 2 * t + 1, 309, 310, 3 * t - 1, 3 * t, 3 * t + 1, 5 * t + 7)] + [(48, 1024)]


@pytest.mark.parametrize("d,K", _tile_cases())
def test_multi_tile_path(d, K):
    from probaforms_amd.models import _predict_lib as pl
    t = pl.joint_tiling(d, K)
    budget = t.budget_bytes
    fits = 4 * d * (K + 1) <= budget
    assert (t.n_tiles == 1) == fits and t.n_chunks == 1
    if not fits:
        tile = (budget // 4 // d - 1) // 2 // 64 * 64
        assert tile >= 64 and t.tile_draws == tile and t.n_tiles == -(-K // tile) >= 2
    if (d, K) in ((33, 310), (33, 383), (33, 385), (33, 647), (48, 1024)):
        assert t.n_tiles >= 2                                        # the multi-tile path is reached
    if (d, K) in ((33, 310), (33, 383), (33, 385), (33, 647)):
        assert K % t.tile_draws != 0                                 # with a last tile that is not full
    xt, y = JN.finite(K, d)
    if d == 48:
        xt, y = xt[:2], y[:2]
    _against_the_yardstick(xt, y, "tiles", fairs=(False,), orders=(0.5, 2.0))


@pytest.mark.parametrize("d,K", [(200, 70), (80, 129), (2000, 5)])
def test_column_chunk_path(d, K):
    """d too wide for two 64-draw images of all columns: the columns pass through in chunks"""
    from probaforms_amd.models import _predict_lib as pl
    t = pl.joint_tiling(d, K)
    assert t.n_chunks >= 2 and t.tile_draws == 64 and t.n_tiles == -(-K // 64) and d % t.chunk_cols != 0
    xt, y = JN.finite(K, d)
    _against_the_yardstick(xt[:3], y[:3], "chunks", fairs=(True,), orders=(1.0,))


# ---- 4. one column: the CRPS --------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 2, 19, 256, 1000])
def test_one_column_is_pfp_scores_crps(K):
    xt, y = JN.finite(K, 1)
    for fair in (False, True):
        ref, sref = JN.scores(xt, y, fair, 0.5), SN.scores(xt, y, (), fair)
        got = _joint(xt, y, fair, 0.5)
        crps = _scores(xt, y, None, fair, want=("crps",))[0][:, 0]
        tol = JN.bound_pairs(ref.energy, ref, K, 1) + SN.bound(sref.crps[:, 0], K, SN.scale_of(xt, y)[:, 0])
        assert np.array_equal(np.isnan(got[0]), np.isnan(crps))
        ok = ~np.isnan(crps)
        assert (np.abs(got[0].astype(np.float64) - crps)[ok] <= tol[ok]).all(), (K, fair)
        assert (got[2] == 0).all()


# ---- 5. non-finite values -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 2, 19, 256, 400])
def test_nonfinite_table(K):
    d = 3 if K < 400 else 33                                         # K = 400, d = 33: the rules on the multi-tile path
    xt, y = JN.nonfinite(K, d)
    if d == 33:
        assert _tiles(d, K)[0] >= 2
    for fair in (False, True):
        for order in (0.5, 2.0):
            got, ref = _joint(xt, y, fair, order, bitwise_upload=True), JN.scores(xt, y, fair, order)
            JN.check_all(got, ref, K, d, (K, fair, order))
            JN.table(K, fair, *got)
            alone = _joint(xt[-1:], y[-1:], fair, order)
            _same_bits([a[-1:] for a in got], alone, "a clean row beside dirty ones")


# ---- 6. grid stride -----------------------------------------------------------------------------------------------
def test_joint_scores_grid_stride():
    """five rows more than the largest grid: five workgroups score a second row"""
    from probaforms_amd.models import _predict_lib as pl
    K, d = 5, 2
    grid = pl.joint_tiling(d, K).max_grid
    n = grid + 5
    rng = np.random.default_rng(8)
    xt = (rng.standard_normal((n, d, K)) * 3 + 1).astype(np.float32)
    y = (rng.standard_normal((n, d)) * 3 + 1).astype(np.float32)
    y[::7] = xt[::7, :, 2]
    got = _joint(xt, y)
    JN.check_all(got, JN.scores(xt, y), K, d, "grid stride")
    tail = _joint(xt[grid:], y[grid:])
    _same_bits([a[grid:] for a in got], tail, "the rows of the second round alone")


# ---- 7. reruns, row splits, permutations --------------------------------------------------------------------------
@pytest.mark.parametrize("d,K", [(3, 19), (3, 1000), (33, 400)])
def test_rerun_and_row_split_are_bitwise(d, K):
    xt, y = JN.finite(K, d)
    rng = np.random.default_rng(K)
    pk, pd = rng.permutation(K), rng.permutation(d)
    for fair in (False, True):
        one = _joint(xt, y, fair)
        _same_bits(_joint(xt, y, fair), one, "rerun")
        a, b = _joint(xt[:2], y[:2], fair), _joint(xt[2:], y[2:], fair)
        _same_bits([np.concatenate([u, v]) for u, v in zip(a, b)], one, "rows split over two calls")
        ref = JN.scores(xt, y, fair, 0.5)
        tols = [JN.bound_pairs(ref.energy, ref, K, d), JN.bound_pairs(ref.spread, ref, K, d),
                JN.bound_variogram(ref.variogram, ref, K, d)]
        for what, x2, y2 in (("draws permuted", xt[:, :, pk], y), ("columns permuted", xt[:, pd], y[:, pd])):
            got = _joint(np.ascontiguousarray(x2), np.ascontiguousarray(y2), fair)
            JN.check_all(got, ref, K, d, what)
            for g, o, tol in zip(got, one, tols):
                assert (np.abs(g.astype(np.float64) - o) <= 2 * tol).all(), what


# ---- 8. output bounds ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,K", [(2, 19), (3, 257), (33, 400)])
def test_outputs_are_fully_written_and_stay_inside_their_arrays(d, K):
    from probaforms_amd.models import _predict_lib as pl
    xf, yf = JN.finite(K, d)
    xn, yn = JN.nonfinite(K, d)
    xt, y = np.concatenate([xf, xn]), np.concatenate([yf, yn])
    n = xt.shape[0]
    outs = [_guarded((n,)) for _ in range(3)]
    xd, xb = _guarded((n, d, K))
    yd, yb = _guarded((n, d))
    xd.copy_(_dev(xt))
    yd.copy_(_dev(y))
    pl.joint_scores(xd, yd, n, d, K, False, 0.5, *[o[0] for o in outs])
    torch.cuda.synchronize()
    for arr, buf in outs:
        assert (_guards_intact(arr, buf) != SENTINEL).all()          # every word written: no NaN the kernel forms is the sentinel
    np.testing.assert_array_equal(_guards_intact(xd, xb), _bits(xt).ravel())          # the inputs are not modified
    np.testing.assert_array_equal(_guards_intact(yd, yb), _bits(y).ravel())
    _same_bits([o[0].cpu().numpy() for o in outs], _joint(xt, y), "guarded arrays")


# ---- 9. nullable outputs ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,K", [(3, 40), (33, 400)])
def test_every_subset_of_outputs(d, K):
    xt, y = JN.finite(K, d)
    full = _joint(xt, y, True, 1.0)
    for r in range(4):
        for want in itertools.combinations(ALL, r):
            got = _joint(xt, y, True, 1.0, want=want)
            _same_bits(got, [f if name in want else None for name, f in zip(ALL, full)], want)
    for order in (None, 7.0, float("nan")):                          # no variogram: any order is accepted
        _same_bits(_joint(xt, y, True, order, want=("energy", "spread")), [full[0], full[1], None], order)


def test_binding_refuses_a_wrong_dtype_and_a_wrong_order():
    from probaforms_amd.models import _predict_lib as pl
    xt, y = torch.zeros(2, 3, 5, device="cuda"), torch.zeros(2, 3, device="cuda")
    out = torch.empty(2, device="cuda")
    with pytest.raises(RuntimeError, match="y must be contiguous"):
        pl.joint_scores(xt, y.double(), 2, 3, 5, False, 0.5, out, None, None)
    with pytest.raises(RuntimeError, match="y must be contiguous"):
        pl.joint_scores(xt, torch.zeros(3, 2, device="cuda").t(), 2, 3, 5, False, 0.5, out, None, None)
    with pytest.raises(RuntimeError, match="y must be a tensor on a HIP device"):
        pl.joint_scores(xt, y.cpu(), 2, 3, 5, False, 0.5, out, None, None)
    with pytest.raises(RuntimeError, match="xt must be contiguous"):
        pl.joint_scores(xt.double(), y, 2, 3, 5, False, 0.5, out, None, None)
    with pytest.raises(RuntimeError, match="energy must be contiguous"):
        pl.joint_scores(xt, y, 2, 3, 5, False, 0.5, out.double(), None, None)
    with pytest.raises(RuntimeError, match="invalid argument"):
        pl.joint_scores(xt, y, 2, 3, 5, False, 0.75, out, None, torch.empty(2, device="cuda"))


# ---- 11. the public call, per model -------------------------------------------------------------------------------
def _xt(many):
    return np.ascontiguousarray(np.transpose(many, (1, 2, 0)))


@pytest.mark.parametrize("K", [19, 40])
@pytest.mark.parametrize("kind", MODELS)
def test_public_call_scores_the_seeded_draws(kind, K):
    from probaforms_amd.models._predict import JointScores
    m, d, c = _public_model(kind)
    C = np.random.default_rng(43).standard_normal((N, c)).astype(np.float32)
    torch.manual_seed(5)
    many = m.sample_many(C, K)
    end = torch.get_rng_state()
    assert many.shape == (K, N, d)
    Y = (np.random.default_rng(44).standard_normal((N, d)) * 2).astype(np.float32)
    Y[1] = many[K // 2, 1]                                           # a target equal to a draw
    Y[2] = 1e3                                                       # and one far outside
    refs = JN.scores_grid(_xt(many), Y, (False, True), (0.5, 2.0))
    for (fair, order), ref in refs.items():
        torch.manual_seed(5)
        js = m.sample_joint_scores(C, Y, K, fair=fair, variogram_order=order)
        assert torch.equal(torch.get_rng_state(), end)
        assert isinstance(js, JointScores) and all(a.dtype == np.float32 and a.shape == (N,) for a in js)
        JN.check_all(js, ref, K, d, (kind, K, fair, order))
    torch.manual_seed(5)
    j0 = m.sample_joint_scores(C, torch.from_numpy(Y).cuda(), K, fair=True, variogram_order=None)   # targets already on the device
    assert j0.variogram is None
    np.testing.assert_array_equal(_bits(j0.energy), _bits(js.energy))
    np.testing.assert_array_equal(_bits(j0.spread), _bits(js.spread))
    torch.manual_seed(5)
    _same_bits(m.sample_joint_scores(C, Y, K), _joint(_xt(many), Y), "the default call is the kernel on sample_many's draws")


def test_flow_call_takes_and_returns_device_tensors():
    m, d, c = _realnvp("host")
    C = torch.from_numpy(np.random.default_rng(43).standard_normal((N, c)).astype(np.float32)).cuda()
    Y = torch.from_numpy(np.random.default_rng(44).standard_normal((N, d)).astype(np.float32)).cuda()
    torch.manual_seed(5)
    js = m.nf.sample_joint_scores(C, Y, 19, variogram_order=1)
    assert all(isinstance(a, torch.Tensor) and a.is_cuda and a.dtype == torch.float32 and a.shape == (N,) for a in js)
    torch.manual_seed(5)
    pub = m.sample_joint_scores(C.cpu().numpy(), Y.cpu().numpy(), 19, variogram_order=1)
    _same_bits([a.cpu().numpy() for a in js], pub, "nf.sample_joint_scores")


@pytest.mark.parametrize("kind", ["realnvp_host", "realnvp_device", "cvae", "cnormal"])
def test_generator_ends_where_the_loop_ends(kind):
    m, d, c = _public_model(kind)
    K = 19
    C = np.random.default_rng(43).standard_normal((N, c)).astype(np.float32)
    Y = np.zeros((N, d), np.float32)
    torch.manual_seed(5)
    for _ in range(K):
        m.sample(C)
    end = torch.get_rng_state()
    torch.manual_seed(5)
    m.sample_joint_scores(C, Y, K)
    assert torch.equal(torch.get_rng_state(), end)


def test_row_chunks_give_the_one_chunk_result(monkeypatch):
    from probaforms_amd.models import _predict as P
    K = 19
    for kind in ("realnvp_host", "realnvp_device", "wgan"):
        m, d, c = _public_model(kind)
        C = np.random.default_rng(43).standard_normal((N, c)).astype(np.float32)
        Y = np.random.default_rng(44).standard_normal((N, d)).astype(np.float32)
        torch.manual_seed(5)
        one = m.sample_joint_scores(C, Y, K)
        end = torch.get_rng_state()
        with monkeypatch.context() as mp:
            mp.setattr(P, "XT_CHUNK_BYTES", 4 * d * K * 10)           # chunks of 10 rows
            mp.setattr(P, "Z_WINDOW_BYTES", 4 * N * 2 * 7)            # a few draws per window
            assert len(P.quantile_row_chunks(N, d, K, P.XT_CHUNK_BYTES)) == 4
            torch.manual_seed(5)
            two = m.sample_joint_scores(C, Y, K)
            assert torch.equal(torch.get_rng_state(), end)
        _same_bits(two, one, kind)


def _host_and_kernel_agree(js, loop, Y, K, d, fair, order, what):
    """the host route's scores of the loop's draws and pfp_joint_scores of the same draws: each within the bound of the float64
    value, so at most twice the bound apart"""
    ref = JN.scores_of_stacked(loop, Y, fair, order)
    kern = _joint(_xt(loop), Y, fair, order)
    JN.check_all(js, ref, K, d, (what, "host"))
    JN.check_all(kern, ref, K, d, (what, "kernel"))
    JN.check_all(js, JN.Joint(ref.t1, kern[1].astype(np.float64), kern[0].astype(np.float64), kern[2].astype(np.float64), ref.v),
                 K, d, (what, "host against kernel"), times=2.0)


def test_layerwise_flow_is_scored_on_the_host():
    from probaforms_amd.models.nflow import DEVICE, NormalizingFlow, StandardNormalPrior
    from probaforms_amd.models.realnvp import RealNVPLayer
    d, c, n, K = 4, 2, 9, 19
    torch.manual_seed(1)
    nf = NormalizingFlow([RealNVPLayer(d, c, (torch.arange(d) + i) % 2, hidden=h) for i, h in enumerate([(8,), (12,)])],
                         StandardNormalPrior(d, DEVICE))
    assert nf._predict_route() == "layerwise"
    C = torch.randn(n, c, device=DEVICE)
    Y = torch.randn(n, d, device=DEVICE)
    with torch.no_grad():
        torch.manual_seed(2)
        loop = torch.stack([nf.sample(C) for _ in range(K)]).cpu().numpy()
    end = torch.get_rng_state()
    Yn = Y.cpu().numpy()
    for fair in (False, True):
        torch.manual_seed(2)
        js = [a.cpu().numpy() for a in nf.sample_joint_scores(C, Y, K, fair=fair, variogram_order=0.5)]
        assert torch.equal(torch.get_rng_state(), end)
        _host_and_kernel_agree(js, loop, Yn, K, d, fair, 0.5, ("layerwise", fair))


def test_user_assigned_prior_is_scored_on_the_host():
    m, d, c = _realnvp("host")
    m.nf.prior = torch.distributions.MultivariateNormal(torch.zeros(d), torch.eye(d))
    assert m.nf._predict_route() == "prior"
    K = 19
    C = np.random.default_rng(43).standard_normal((N, c)).astype(np.float32)
    Y = np.random.default_rng(44).standard_normal((N, d)).astype(np.float32)
    torch.manual_seed(5)
    loop = np.array([m.sample(C) for _ in range(K)])
    end = torch.get_rng_state()
    torch.manual_seed(5)
    js = m.sample_joint_scores(C, Y, K, variogram_order=2)
    assert torch.equal(torch.get_rng_state(), end)
    _host_and_kernel_agree(js, loop, Y, K, d, False, 2.0, "user prior")


@pytest.mark.parametrize("kind", MODELS)
def test_empty_input_and_refusals(kind):
    m, d, c = _public_model(kind)
    before = torch.get_rng_state()
    s = m.sample_joint_scores(np.zeros((0, c), np.float32), np.zeros((0, d), np.float32), 5)
    assert s.energy.shape == s.spread.shape == s.variogram.shape == (0,) and s.energy.dtype == np.float32
    if kind != "realnvp_device":                                     # (its seeds are drawn whatever the row count, as the loop's)
        assert torch.equal(torch.get_rng_state(), before)
    C = np.zeros((4, c), np.float32)
    for shape in ((4,), (d, 4), (4, d + 1), (5, d), (1, 4, d)):
        with pytest.raises(ValueError):
            m.sample_joint_scores(C, np.zeros(shape, np.float32), 5)
    Y = np.zeros((4, d), np.float32)
    for bad in (0, -1, 8193):
        with pytest.raises(ValueError):
            m.sample_joint_scores(C, Y, bad)
    for order in (0.25, 3, "half"):
        with pytest.raises(ValueError):
            m.sample_joint_scores(C, Y, 10, variogram_order=order)


@pytest.mark.parametrize("kind", ["realnvp", "cvae", "wgan", "cnormal"])
def test_row_count_instead_of_conditions(kind):
    """a model fitted without conditions takes C as a python int, as sample does"""
    from probaforms_amd.models import RealNVP
    from test_gendraw_gpu import _fitted
    K, n = 19, 21
    if kind == "realnvp":
        torch.manual_seed(3)
        m = RealNVP(n_layers=4, hidden=(10,), batch_size=32, n_epochs=1, lr=1e-3)
        m.fit(np.random.default_rng(7).standard_normal((64, 3)).astype(np.float32))
    else:
        m = _fitted(kind, False)
    Y = np.random.default_rng(44).standard_normal((n, 3)).astype(np.float32)
    torch.manual_seed(5)
    many = m.sample_many(n, K)
    end = torch.get_rng_state()
    torch.manual_seed(5)
    js = m.sample_joint_scores(n, Y, K)
    assert torch.equal(torch.get_rng_state(), end)
    JN.check_all(js, JN.scores_of_stacked(many, Y, False, 0.5), K, 3, kind)


# ---- 12. the same marginals, another dependence -------------------------------------------------------------------
@pytest.mark.parametrize("K", [19, 257])
def test_comonotone_against_shuffled(K):
    xt, sh, y = JN.comonotone(K)
    a, b = _joint(xt, y), _joint(sh, y)
    _same_bits(_scores(xt, y, None, False, want=("crps",)), _scores(sh, y, None, False, want=("crps",)), "the per-column scores")
    assert a[2][0] == 0 and b[2][0] > 0
    assert b[0][0] > a[0][0]
