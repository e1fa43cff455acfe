"""pfp_scores (models/predict_csrc/pf_predict.h) and sample_scores of the four models on the GPU, against the O(K^2) numpy
yardstick of tests/scores_numpy.py.  Runs on the GPU box: `pytest -m gpu`.

Tolerances: pit is exact; quantiles are bitwise those of pfp_quantiles / sample_stats; crps and pinball lie within
ulp32(ref) + 2 K 2^-53 max(|x|, |y|) of the float64 value -- the float64 rounding of at most K-term sums of terms bounded by
max |x|, plus the one final rounding to float32 (scores_numpy.bound)."""
import itertools

import numpy as np
import pytest
import torch

import native_libs
import scores_numpy as SN
import scores_series as S
from probaforms_amd.models import _cnormal_lib, _gendraw_lib, _predict_lib, _wgan_lib
from test_gendraw_gpu import _fitted
from test_predict_edges_gpu import SENTINEL, _bits, _guarded, _guards_intact
from test_predict_gpu import _dev
from test_scores_host import PROBS, _table

pytestmark = pytest.mark.gpu

native_libs.ensure_built(_cnormal_lib, _gendraw_lib, _predict_lib, _wgan_lib)


def _scores(xt, y, probs=PROBS, fair=False, want=("crps", "pit", "q"), bitwise_upload=False):
    """one pfp_scores call -> (crps, pit, quantiles, pinball) as numpy, None where not asked for"""
    from probaforms_amd.models import _predict_lib as pl
    n, d, k = xt.shape
    xd, yd = _dev(xt), _dev(y)
    if bitwise_upload:                                               # NaN signs and payloads reached the device
        np.testing.assert_array_equal(_bits(xd.cpu().numpy()), _bits(xt))
    nq = 0 if probs is None else len(probs)
    new = lambda *shape: torch.empty(*shape, device="cuda")
    crps = new(n, d) if "crps" in want else None
    pit = new(n, d) if "pit" in want else None
    q, pin = (new(nq, n, d), new(nq, n, d)) if ("q" in want and nq) else (None, None)
    pd = torch.tensor(probs, dtype=torch.float64, device="cuda") if nq else None
    pl.scores(xd, yd, n, d, k, fair, pd, crps, pit, q, pin)
    torch.cuda.synchronize()
    return [None if t is None else t.cpu().numpy() for t in (crps, pit, q, pin)]


def _quantiles(xt, probs=PROBS):
    from probaforms_amd.models import _predict_lib as pl
    n, d, k = xt.shape
    q = torch.empty(len(probs), n, d, device="cuda")
    pl.quantiles(_dev(xt), n, d, k, torch.tensor(probs, dtype=torch.float64, device="cuda"), q)
    return q.cpu().numpy()


def _same_bits(a, b, what=None):
    for i, (u, v) in enumerate(zip(a, b)):
        assert (u is None) == (v is None), (what, i)
        if u is not None:
            np.testing.assert_array_equal(_bits(u), _bits(v), err_msg=str((what, i)))


# ---- 1. synthetic series against the yardstick --------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 3])
@pytest.mark.parametrize("K", [1, 2, 3, 16, 19, 255, 256, 257, 1000])
def test_scores_vs_numpy_pair_sum(K, d):
    xt, y = S.finite(K, d)
    scale = SN.scale_of(xt, y)
    qs = _quantiles(xt)
    for fair in (False, True):
        got, ref = _scores(xt, y, PROBS, fair), SN.scores(xt, y, PROBS, fair)
        SN.check_all(got, ref, K, scale, (K, d, fair))
        np.testing.assert_array_equal(_bits(got[2]), _bits(qs))
        np.testing.assert_array_equal(got[1][2, 0], np.float32(0.5))                 # y tied with all K draws
        assert (got[1][4, 0::2] == 1).all() and (got[1][4, 1::2] == 0).all()         # y above / below every draw


def test_scores_of_the_longest_series():
    K = 8192
    rng = np.random.default_rng(K)
    xt = np.stack([rng.standard_normal((1, K)) * 3 + 1, 1e6 + rng.standard_normal((1, K))]).astype(np.float32)
    xt[0, 0, 100:200] = xt[0, 0, 100]                                # ties
    y = np.array([[xt[0, 0, 100]], [1e6 + 0.25]], np.float32)
    scale = SN.scale_of(xt, y)
    qs = _quantiles(xt)
    for fair in (False, True):
        got, ref = _scores(xt, y, PROBS, fair), SN.scores(xt, y, PROBS, fair)
        SN.check_all(got, ref, K, scale, (K, fair))
        np.testing.assert_array_equal(_bits(got[2]), _bits(qs))


# ---- 2. non-finite values -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 2, 19, 256])
def test_nonfinite_table(K):
    xt, y = S.nonfinite(K)
    scale = SN.scale_of(xt, y)
    qs = _quantiles(xt)
    for fair in (False, True):
        got, ref = _scores(xt, y, PROBS, fair, bitwise_upload=True), SN.scores(xt, y, PROBS, fair)
        SN.check_all(got, ref, K, scale, (K, fair))
        _table(K, fair, got[0][:, 0], got[1][:, 0], got[2][:, :, 0], got[3][:, :, 0])
        np.testing.assert_array_equal(_bits(got[2]), _bits(qs))
        for a in got:
            assert np.isfinite(a[..., 1]).all() or (K == 1 and fair)                 # nothing leaves its (row, column)
        alone = _scores(np.ascontiguousarray(xt[:, 1:]), np.ascontiguousarray(y[:, 1:]), PROBS, fair)
        _same_bits([a[..., 1:] for a in got], alone, "a clean series beside dirty ones")


# ---- 3. grid stride -----------------------------------------------------------------------------------------------
def test_scores_grid_stride():
    """65536 + 5 series: five workgroups score a second series"""
    n, K = 65536 + 5, 5
    rng = np.random.default_rng(8)
    xt = (rng.standard_normal((n, 1, K)) * 3 + 1).astype(np.float32)
    y = (rng.standard_normal((n, 1)) * 3 + 1).astype(np.float32)
    y[::7, 0] = xt[::7, 0, 2]
    got, ref = _scores(xt, y, PROBS, False), SN.scores(xt, y, PROBS, False)
    SN.check_all(got, ref, K, SN.scale_of(xt, y), "grid stride")
    tail = _scores(xt[65536:], y[65536:], PROBS, False)
    _same_bits([a[..., 65536:, :] for a in got], tail, "the series of the second round alone")


# ---- 4., 5. row splits and reruns ---------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [19, 1000])
def test_row_split_and_rerun_are_bitwise(K):
    xt, y = S.finite(K, 3)
    for fair in (False, True):
        one = _scores(xt, y, PROBS, fair)
        _same_bits(_scores(xt, y, PROBS, fair), one, "rerun")
        a, b = _scores(xt[:2], y[:2], PROBS, fair), _scores(xt[2:], y[2:], PROBS, fair)
        _same_bits([np.concatenate([u, v], axis=-2) for u, v in zip(a, b)], one, "rows split over two calls")


# ---- 6. output bounds ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [19, 257])
def test_outputs_are_fully_written_and_stay_inside_their_arrays(K):
    from probaforms_amd.models import _predict_lib as pl
    xf, yf = S.finite(K, 2)
    xn, yn = S.nonfinite(K)
    xt, y = np.concatenate([xf, xn]), np.concatenate([yf, yn])
    n, d, nq = xt.shape[0], 2, len(PROBS)
    outs = [_guarded((n, d)), _guarded((n, d)), _guarded((nq, n, d)), _guarded((nq, n, d))]
    xd, xb = _guarded((n, d, K))
    yd, yb = _guarded((n, d))
    xd.copy_(_dev(xt))
    yd.copy_(_dev(y))
    pl.scores(xd, yd, n, d, K, False, torch.tensor(PROBS, dtype=torch.float64, device="cuda"), *[o[0] for o in outs])
    torch.cuda.synchronize()
    for arr, buf in outs:
        assert (_guards_intact(arr, buf) != SENTINEL).all()          # every word written: no NaN the kernel forms is the sentinel
    np.testing.assert_array_equal(_guards_intact(xd, xb), _bits(xt).ravel())          # the inputs are not modified
    np.testing.assert_array_equal(_guards_intact(yd, yb), _bits(y).ravel())
    _same_bits([o[0].cpu().numpy() for o in outs], _scores(xt, y, PROBS, False), "guarded arrays")


# ---- 7. nullable outputs ------------------------------------------------------------------------------------------
def test_every_subset_of_outputs():
    K = 40
    xt, y = S.finite(K, 3)
    full = _scores(xt, y, PROBS, True)
    for r in range(4):
        for want in itertools.combinations(("crps", "pit", "q"), r):
            got = _scores(xt, y, PROBS, True, want=want)
            expect = [full[0] if "crps" in want else None, full[1] if "pit" in want else None] + \
                     ([full[2], full[3]] if "q" in want else [None, None])
            _same_bits(got, expect, want)
    none = _scores(xt, y, None, True)                                # no probabilities: probs NULL, n_probs 0
    _same_bits(none, [full[0], full[1], None, None], "no quantiles")


def test_binding_refuses_a_wrong_dtype():
    from probaforms_amd.models import _predict_lib as pl
    xt, y = torch.zeros(2, 3, 5, device="cuda"), torch.zeros(2, 3, device="cuda")
    out = torch.empty(2, 3, device="cuda")
    with pytest.raises(RuntimeError, match="y must be contiguous"):
        pl.scores(xt, y.double(), 2, 3, 5, False, None, out, None, None, None)
    with pytest.raises(RuntimeError, match="y must be contiguous"):
        pl.scores(xt, torch.zeros(3, 2, device="cuda").t(), 2, 3, 5, False, None, out, None, None, None)
    with pytest.raises(RuntimeError, match="y must be a tensor on a HIP device"):
        pl.scores(xt, y.cpu(), 2, 3, 5, False, None, out, None, None, None)


# ---- 8. the public call, per model --------------------------------------------------------------------------------
N = 37
QS = (0.05, 0.5, 0.95)


def _realnvp(which):
    from probaforms_amd.models import RealNVP
    L, d, c, hidden, prior_rng = {"host": (4, 3, 2, (10,), "host"), "device": (4, 3, 2, (10,), "device"),
                                  "wide": (4, 16, 4, (64,), "host")}[which]
    rng = np.random.default_rng(7)
    torch.manual_seed(3)
    m = RealNVP(n_layers=L, hidden=hidden, batch_size=32, n_epochs=1, lr=1e-3, prior_rng=prior_rng)
    m.fit(rng.standard_normal((64, d)).astype(np.float32), rng.standard_normal((64, c)).astype(np.float32))
    return m, d, c


def _public_model(kind):
    if kind.startswith("realnvp_"):
        return _realnvp(kind[len("realnvp_"):])
    return _fitted(kind, True), 3, 2


MODELS = ("realnvp_host", "realnvp_device", "realnvp_wide", "cvae", "wgan", "cnormal", "cnormal_independent")


@pytest.mark.parametrize("K", [19, 40])
@pytest.mark.parametrize("kind", MODELS)
def test_public_call_scores_the_seeded_draws(kind, K):
    from probaforms_amd.models._predict import SampleScores
    m, d, c = _public_model(kind)
    C = np.random.default_rng(43).standard_normal((N, c)).astype(np.float32)
    torch.manual_seed(5)
    many = m.sample_many(C, K)
    end = torch.get_rng_state()
    assert many.shape == (K, N, d)
    Y = (np.random.default_rng(44).standard_normal((N, d)) * 2).astype(np.float32)
    Y[1] = many[K // 2, 1]                                           # targets equal to a draw
    Y[2] = 1e3                                                       # and far outside
    scale = SN.scale_of(np.moveaxis(many, 0, -1), Y)
    torch.manual_seed(5)
    st = m.sample_stats(C, K, quantiles=QS)
    for fair in (False, True):
        torch.manual_seed(5)
        sc = m.sample_scores(C, Y, K, quantiles=QS, fair=fair)
        assert torch.equal(torch.get_rng_state(), end)
        assert isinstance(sc, SampleScores)
        assert sc.crps.shape == sc.pit.shape == (N, d) and sc.quantiles.shape == sc.pinball.shape == (len(QS), N, d)
        assert all(a.dtype == np.float32 for a in sc)
        SN.check_all(sc, SN.scores_of_stacked(many, Y, QS, fair), K, scale, (kind, K, fair))
        np.testing.assert_array_equal(_bits(sc.quantiles), _bits(st.quantiles))
        assert (sc.pit[2] == 1).all() and ((sc.pit[1] > 0) & (sc.pit[1] < 1)).all()
    torch.manual_seed(5)
    s0 = m.sample_scores(C, torch.from_numpy(Y).cuda(), K, quantiles=None, fair=True)       # targets already on the device
    assert s0.quantiles is None and s0.pinball is None
    np.testing.assert_array_equal(_bits(s0.crps), _bits(sc.crps))
    np.testing.assert_array_equal(_bits(s0.pit), _bits(sc.pit))


def test_flow_call_takes_and_returns_device_tensors():
    m, d, c = _realnvp("host")
    C = torch.from_numpy(np.random.default_rng(43).standard_normal((N, c)).astype(np.float32)).cuda()
    Y = torch.from_numpy(np.random.default_rng(44).standard_normal((N, d)).astype(np.float32)).cuda()
    torch.manual_seed(5)
    sc = m.nf.sample_scores(C, Y, 19, quantiles=QS)
    assert all(isinstance(a, torch.Tensor) and a.is_cuda and a.dtype == torch.float32 for a in sc)
    torch.manual_seed(5)
    pub = m.sample_scores(C.cpu().numpy(), Y.cpu().numpy(), 19, quantiles=QS)
    _same_bits([a.cpu().numpy() for a in sc], pub, "nf.sample_scores")


# ---- 9. the public call, edge cases -------------------------------------------------------------------------------
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
    m.sample_scores(C, Y, K)
    assert torch.equal(torch.get_rng_state(), end)


def test_row_chunks_give_the_one_chunk_result(monkeypatch):
    from probaforms_amd.models import _predict as P
    K = 19
    for kind in ("realnvp_host", "realnvp_device", "wgan"):
        m, d, c = _public_model(kind)
        C = np.random.default_rng(43).standard_normal((N, c)).astype(np.float32)
        Y = np.random.default_rng(44).standard_normal((N, d)).astype(np.float32)
        torch.manual_seed(5)
        one = m.sample_scores(C, Y, K, quantiles=QS)
        end = torch.get_rng_state()
        with monkeypatch.context() as mp:
            mp.setattr(P, "XT_CHUNK_BYTES", 4 * d * K * 10)           # chunks of 10 rows
            mp.setattr(P, "Z_WINDOW_BYTES", 4 * N * 2 * 7)            # a few draws per window
            assert len(P.quantile_row_chunks(N, d, K, P.XT_CHUNK_BYTES)) == 4
            torch.manual_seed(5)
            two = m.sample_scores(C, Y, K, quantiles=QS)
            assert torch.equal(torch.get_rng_state(), end)
        _same_bits(two, one, kind)


def _host_and_kernel_agree(sc, loop, Y, K, fair, scale, what):
    """the host route's scores of the loop's draws and pfp_scores of the same draws: each within the bound of the float64
    value, so at most twice the bound apart; pit equal"""
    ref = SN.scores_of_stacked(loop, Y, QS, fair)
    kern = _scores(np.ascontiguousarray(np.moveaxis(loop, 0, -1)), Y, QS, fair)
    SN.check_all(sc, ref, K, scale, (what, "host"))
    SN.check_all(kern, ref, K, scale, (what, "kernel"))
    np.testing.assert_array_equal(sc[1], kern[1])
    for got, k, r in zip(sc, kern, ref):
        assert (np.abs(got.astype(np.float64) - k) <= 2 * SN.bound(r, K, scale)).all(), what


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
    scale = SN.scale_of(np.moveaxis(loop, 0, -1), Yn)
    for fair in (False, True):
        torch.manual_seed(2)
        sc = [a.cpu().numpy() for a in nf.sample_scores(C, Y, K, quantiles=QS, fair=fair)]
        assert torch.equal(torch.get_rng_state(), end)
        _host_and_kernel_agree(sc, loop, Yn, K, fair, scale, ("layerwise", fair))


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
    scale = SN.scale_of(np.moveaxis(loop, 0, -1), Y)
    torch.manual_seed(5)
    sc = m.sample_scores(C, Y, K, quantiles=QS)
    assert torch.equal(torch.get_rng_state(), end)
    _host_and_kernel_agree(sc, loop, Y, K, False, scale, "user prior")


@pytest.mark.parametrize("kind", MODELS)
def test_empty_input_and_refusals(kind):
    m, d, c = _public_model(kind)
    before = torch.get_rng_state()
    s = m.sample_scores(np.zeros((0, c), np.float32), np.zeros((0, d), np.float32), 5, quantiles=(0.5,))
    assert s.crps.shape == s.pit.shape == (0, d) and s.quantiles.shape == s.pinball.shape == (1, 0, d)
    assert s.crps.dtype == np.float32
    if kind != "realnvp_device":                                     # (its seeds are drawn whatever the row count, as the loop's)
        assert torch.equal(torch.get_rng_state(), before)
    C = np.zeros((4, c), np.float32)
    for shape in ((4,), (d, 4), (4, d + 1), (5, d), (1, 4, d)):
        with pytest.raises(ValueError):
            m.sample_scores(C, np.zeros(shape, np.float32), 5)
    Y = np.zeros((4, d), np.float32)
    for bad in (0, -1, 8193):
        with pytest.raises(ValueError):
            m.sample_scores(C, Y, bad, quantiles=None)
    for q in (-0.1, 1.5):
        with pytest.raises(ValueError):
            m.sample_scores(C, Y, 10, quantiles=(q,))


@pytest.mark.parametrize("kind", ["realnvp", "cvae", "wgan", "cnormal"])
def test_row_count_instead_of_conditions(kind):
    """a model fitted without conditions takes C as a python int, as sample does"""
    from probaforms_amd.models import RealNVP
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
    sc = m.sample_scores(n, Y, K, quantiles=QS)
    assert torch.equal(torch.get_rng_state(), end)
    SN.check_all(sc, SN.scores_of_stacked(many, Y, QS, False), K, SN.scale_of(np.moveaxis(many, 0, -1), Y), kind)
