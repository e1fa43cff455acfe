"""libpf_predict.so (models/predict_csrc/pf_predict.h) and RealNVP.sample_stats / sample_many on the GPU: the draws against
the CPU oracle, the moments and quantiles against numpy in float64, split invariance, determinism, and the public calls
against the notebook loop they replace.  Runs on the GPU box: `pytest -m gpu`.

Shapes: n = 37 rows (not a multiple of 16) and K = 19 draws (crosses one 16-draw tile, not a multiple of 16).
Tolerances: the draws meet the bar tests/test_hip_kernels.py sets for the product sampling kernels (mean |err| < 5e-6 *
max(1, mean |want|)); mean / std / quantiles are float64 arithmetic rounded once to float32, compared at 2 float32 ulps
(rtol 2.4e-7); min / max are exact."""
import functools

import numpy as np
import pytest
import torch

import native_libs
from conftest import load_case
from probaforms_amd.models import _predict_lib

pytestmark = pytest.mark.gpu

native_libs.ensure_built(_predict_lib)

NAMES = ["c2", "c3", "c4", "tm", "tm_nocond", "reg1d", "relu_mh"]
N, K, ROW0 = 37, 19, 11
ULP2 = 2.4e-7


def _dev(a, dtype=torch.float32):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a)).to(dtype).cuda().contiguous()


def _close(got, want, what):
    """within 2 float32 ulps of the float64 value"""
    err = np.abs(np.asarray(got, np.float64) - want)
    assert (err <= ULP2 * np.abs(want)).all(), (what, float(err.max()))


@functools.lru_cache(maxsize=None)
def _setup(name):
    from probaforms_amd import _hip
    cs = load_case(name)
    shape = _hip.RnvpShape.make(cs["L"], cs["d"], cs["c"], cs["hidden"], cs["act"], alt_masks=0)
    rng = np.random.default_rng(17)
    Cn = rng.standard_normal((N, cs["c"])).astype(np.float32) if cs["c"] else None
    seeds = [int(v) for v in rng.integers(0, 2 ** 64, size=K, dtype=np.uint64)]
    return cs, shape, _dev(cs["params"]), _dev(cs["masks"], torch.uint8), Cn, seeds


def _ws(shape, k):
    from probaforms_amd.models import _predict_lib as pl
    return torch.empty(pl.workspace_bytes(shape, k), dtype=torch.uint8, device="cuda")


def _draw(name, rows=(0, N), ks=(0, K), state=None, want_x=True, want_xt=False, z=None, n_total=None, row0=ROW0):
    """one pfp_draw_accumulate call over rows [lo, hi) of the test's N rows and draws [k_lo, k_hi) of its K"""
    from probaforms_amd.models import _predict_lib as pl
    cs, shape, params, masks, Cn, seeds = _setup(name)
    (lo, hi), (k_lo, k_hi), d = rows, ks, cs["d"]
    m, kc = hi - lo, k_hi - k_lo
    c = None if Cn is None else _dev(Cn[lo:hi])
    x = torch.empty(kc, m, d, device="cuda") if want_x else None
    xt = torch.zeros(m, d, K, device="cuda") if want_xt else None
    keep = pl.draw_accumulate(shape, params, masks, c, m, row0 + lo, None if z is not None else seeds[k_lo:k_hi],
                              None if z is None else z[k_lo:k_hi].contiguous(), n_total if z is not None else ROW0 + N,
                              k_lo, kc, K, state, x, xt, _ws(shape, kc))
    torch.cuda.synchronize()
    del keep
    return x, xt


def _finalize(state, n, d, ddof):
    from probaforms_amd.models import _predict_lib as pl
    out = [torch.empty(n, d, device="cuda") for _ in range(4)]
    pl.finalize(state, n, d, ddof, *out)
    return [t.cpu().numpy() for t in out]


@functools.lru_cache(maxsize=None)
def _one_call(name):
    """the whole job in one launch: draws, transposed draws and state; shared by the tests below (read only)"""
    from probaforms_amd.models import _predict_lib as pl
    d = _setup(name)[0]["d"]
    state = pl.new_state(N, d, "cuda")
    x, xt = _draw(name, state=state, want_xt=True)
    return x.cpu().numpy(), xt.cpu().numpy(), state


def _bar(got, want):
    err = np.abs(got - want)
    assert err.mean() < 5e-6 * max(1.0, np.abs(want).mean()), err.mean()


@pytest.mark.parametrize("name", NAMES)
def test_draws_seed_path_vs_oracle(name, oracle32):
    from oracle import Shape
    cs, _, _, _, Cn, seeds = _setup(name)
    x, xt, _ = _one_call(name)
    so = Shape.make(cs["L"], cs["d"], cs["c"], cs["hidden"], cs["act"])
    want = np.stack([oracle32.sample(so, cs["params"], oracle32.prior_normal(s, ROW0, N, cs["d"]), Cn, cs["masks"]) for s in seeds])
    assert np.isfinite(x).all()
    _bar(x, want)
    np.testing.assert_array_equal(xt, np.transpose(x, (1, 2, 0)))


@pytest.mark.parametrize("name", NAMES)
def test_draws_z_path_vs_oracle(name, oracle32):
    from oracle import Shape
    cs, _, _, _, Cn, _ = _setup(name)
    n_total, row0, d = N + 20, 9, cs["d"]
    z = np.random.default_rng(23).standard_normal((K, n_total, d)).astype(np.float32)
    x, _ = _draw(name, z=_dev(z), n_total=n_total, row0=row0)
    so = Shape.make(cs["L"], cs["d"], cs["c"], cs["hidden"], cs["act"])
    want = np.stack([oracle32.sample(so, cs["params"], z[k, row0:row0 + N], Cn, cs["masks"]) for k in range(K)])
    _bar(x.cpu().numpy(), want)


@pytest.mark.parametrize("name", NAMES)
def test_moments_vs_numpy_float64(name):
    x, _, state = _one_call(name)
    d = x.shape[2]
    x64 = x.astype(np.float64)
    for ddof in (0, 1):
        mean, std, mn, mx = _finalize(state, N, d, ddof)
        _close(mean, x64.mean(0), "mean")
        _close(std, x64.std(0, ddof=ddof), "std")
        np.testing.assert_array_equal(mn, x.min(0))
        np.testing.assert_array_equal(mx, x.max(0))


def test_single_draw_has_zero_std():
    from probaforms_amd.models import _predict_lib as pl
    d = _setup("tm")[0]["d"]
    state = pl.new_state(N, d, "cuda")
    x, _ = _draw("tm", ks=(0, 1), state=state)
    mean, std, mn, mx = _finalize(state, N, d, 0)
    x = x.cpu().numpy()[0]
    for got in (mean, mn, mx):
        np.testing.assert_array_equal(got, x)
    np.testing.assert_array_equal(std, np.zeros_like(x))
    assert np.isnan(_finalize(state, N, d, 1)[1]).all()              # numpy: std of one value with ddof = 1


@pytest.mark.parametrize("name", ["c2", "tm", "relu_mh"])
def test_row_split_and_rerun_are_bitwise(name):
    from probaforms_amd.models import _predict_lib as pl
    x, xt, state = _one_call(name)
    d = x.shape[2]
    st2 = pl.new_state(N, d, "cuda")
    xa, xta = _draw(name, rows=(0, 20), state=st2[:20], want_xt=True)
    xb, xtb = _draw(name, rows=(20, N), state=st2[20:], want_xt=True)
    np.testing.assert_array_equal(np.concatenate([xa.cpu().numpy(), xb.cpu().numpy()], axis=1), x)
    np.testing.assert_array_equal(np.concatenate([xta.cpu().numpy(), xtb.cpu().numpy()], axis=0), xt)
    assert torch.equal(st2, state)
    st3 = pl.new_state(N, d, "cuda")
    xc, _ = _draw(name, state=st3)
    np.testing.assert_array_equal(xc.cpu().numpy(), x)
    assert torch.equal(st3, state)


@pytest.mark.parametrize("name", ["c2", "tm"])
def test_draw_windows_agree_within_rounding(name):
    from probaforms_amd.models import _predict_lib as pl
    x, xt, state = _one_call(name)
    d = x.shape[2]
    st = pl.new_state(N, d, "cuda")
    xa, xta = _draw(name, ks=(0, 8), state=st, want_xt=True)
    xb, _ = _draw(name, ks=(8, K), state=st, want_xt=False)
    np.testing.assert_array_equal(np.concatenate([xa.cpu().numpy(), xb.cpu().numpy()]), x)     # the draws themselves: bitwise
    np.testing.assert_array_equal(xta.cpu().numpy()[:, :, :8], xt[:, :, :8])
    for ddof in (0, 1):
        one, two = _finalize(state, N, d, ddof), _finalize(st, N, d, ddof)
        _close(two[0], one[0].astype(np.float64), "mean")
        _close(two[1], one[1].astype(np.float64), "std")
        np.testing.assert_array_equal(two[2], one[2])
        np.testing.assert_array_equal(two[3], one[3])


@pytest.mark.parametrize("k", [1, 2, 19, 1000, 8192])
def test_quantiles_vs_numpy(k):
    from probaforms_amd.models import _predict_lib as pl
    rng = np.random.default_rng(k)
    n, d = 3, 2
    xt = (rng.standard_normal((n, d, k)) * 3 + 1).astype(np.float32)
    xt[1, 1, :] = np.float32(0.7)                                    # a constant series: ties everywhere
    xt[2, 0, : k // 2] = xt[2, 0, 0]                                 # half of a series tied
    probs = [0.0, 0.05, 0.5, 0.95, 1.0]
    q = torch.empty(len(probs), n, d, device="cuda")
    pl.quantiles(_dev(xt), n, d, k, torch.tensor(probs, dtype=torch.float64, device="cuda"), q)
    want = np.quantile(xt.astype(np.float64), probs, axis=-1)
    got = q.cpu().numpy()
    _close(got, want, "quantiles")
    np.testing.assert_array_equal(got[:, 1, 1], np.full(len(probs), np.float32(0.7)))
    np.testing.assert_array_equal(got[0], xt.min(-1))
    np.testing.assert_array_equal(got[-1], xt.max(-1))


def _model(name, prior_rng):
    from cases import CASES
    from probaforms_amd.models import RealNVP
    L, d, c, hidden, act, _ = CASES[name]
    rng = np.random.default_rng(7)
    torch.manual_seed(3)
    m = RealNVP(n_layers=L, hidden=hidden, activation=act, batch_size=32, n_epochs=1, lr=1e-3, prior_rng=prior_rng)
    m.fit(rng.standard_normal((64, d)).astype(np.float32), rng.standard_normal((64, c)).astype(np.float32))
    return m, d, c


@pytest.mark.parametrize("prior_rng", ["host", "device"])
@pytest.mark.parametrize("name,n", [("tm", N), ("tm", 32), ("reg1d", 5)])
def test_api_vs_notebook_loop(name, n, prior_rng):
    """n d = 185: one device draw of the host stream per sample; 160: whole 16-blocks, one draw per window; 5: host randn"""
    m, d, c = _model(name, prior_rng)
    C = np.random.default_rng(11).standard_normal((n, c)).astype(np.float32)
    probs = (0.05, 0.95)
    torch.manual_seed(5)
    s = m.sample_stats(C, K, quantiles=probs)
    after_stats = torch.get_rng_state()
    torch.manual_seed(5)
    loop = np.array([m.sample(C) for _ in range(K)])
    after_loop = torch.get_rng_state()
    assert torch.equal(after_stats, after_loop)
    torch.manual_seed(5)
    many = m.sample_many(C, K)
    assert torch.equal(torch.get_rng_state(), after_loop)
    assert many.shape == loop.shape == (K, n, d) and many.dtype == np.float32
    delta = many.astype(np.float64) - loop.astype(np.float64)
    _bar(many, loop)
    l64 = loop.astype(np.float64)
    for a in (s.mean, s.std, s.min, s.max):
        assert a.shape == (n, d) and a.dtype == np.float32
    assert s.quantiles.shape == (2, n, d) and s.quantiles.dtype == np.float32
    assert (np.abs(s.mean - l64.mean(0)) <= np.abs(delta).mean(0) + ULP2 * np.abs(l64.mean(0))).all()
    assert (np.abs(s.std - l64.std(0)) <= np.sqrt((delta ** 2).mean(0)) + ULP2 * l64.std(0)).all()
    # against the call's own draws: float64 arithmetic, one rounding
    m64 = many.astype(np.float64)
    _close(s.mean, m64.mean(0), "mean")
    _close(s.std, m64.std(0), "std")
    np.testing.assert_array_equal(s.min, many.min(0))
    np.testing.assert_array_equal(s.max, many.max(0))
    _close(s.quantiles, np.quantile(m64, probs, axis=0), "quantiles")
    assert m.sample_stats(C, 3).quantiles is None                    # no quantiles asked for


def test_validation_and_empty_input():
    m, d, c = _model("tm", "host")
    C = np.zeros((4, c), np.float32)
    for bad in (0, -1):
        with pytest.raises(ValueError):
            m.sample_stats(C, bad)
        with pytest.raises(ValueError):
            m.sample_many(C, bad)
    for q in (-0.1, 1.5):
        with pytest.raises(ValueError):
            m.sample_stats(C, 10, quantiles=(q,))
    with pytest.raises(ValueError):
        m.sample_stats(C, 8193, quantiles=(0.5,))
    s = m.sample_stats(np.zeros((0, c), np.float32), 5, quantiles=(0.5,))
    assert s.mean.shape == s.std.shape == s.min.shape == s.max.shape == (0, d) and s.quantiles.shape == (1, 0, d)
    assert m.sample_many(np.zeros((0, c), np.float32), 5).shape == (5, 0, d)


def test_layerwise_flow_falls_back_to_the_loop_bitwise():
    from probaforms_amd.models import _predict as P
    from probaforms_amd.models.nflow import DEVICE, NormalizingFlow, StandardNormalPrior
    from probaforms_amd.models.realnvp import RealNVPLayer
    d, c, n = 4, 2, 9
    torch.manual_seed(1)
    nf = NormalizingFlow([RealNVPLayer(d, c, (torch.arange(d) + i) % 2, hidden=h) for i, h in enumerate([(8,), (12,)])],
                         StandardNormalPrior(d, DEVICE))
    assert nf._predict_route() == "layerwise"
    C = torch.randn(n, c, device=DEVICE)
    with torch.no_grad():
        torch.manual_seed(2)
        loop = torch.stack([nf.sample(C) for _ in range(5)]).cpu().numpy()
    torch.manual_seed(2)
    many = nf.sample_many(C, 5)
    np.testing.assert_array_equal(many.cpu().numpy(), loop)
    torch.manual_seed(2)
    s = nf.sample_stats(C, 5, quantiles=(0.05, 0.95), ddof=1)
    want = P.stats_of_draws(loop, (0.05, 0.95), 1)
    for got, w in zip(s, want):
        np.testing.assert_array_equal(got.cpu().numpy(), w)


@pytest.mark.parametrize("name", ["tm", "relu_mh", "c2"])
def test_draws_do_not_depend_on_the_pass_width(name):
    """40 draws in one call run 64 (or, for a large image, 32) draws per pass; the same draws fed as windows of 16 and 24 run
    16 and 32 per pass: every draw is bitwise the same, and the moments of the one call match numpy"""
    from probaforms_amd.models import _predict_lib as pl
    cs, shape, params, masks, Cn, _ = _setup(name)
    k, d = 40, cs["d"]
    seeds = [int(v) for v in np.random.default_rng(41).integers(0, 2 ** 64, size=k, dtype=np.uint64)]
    c = _dev(Cn)

    def call(k_lo, k_hi, state):
        x = torch.empty(k_hi - k_lo, N, d, device="cuda")
        keep = pl.draw_accumulate(shape, params, masks, c, N, ROW0, seeds[k_lo:k_hi], None, ROW0 + N, k_lo, k_hi - k_lo, k,
                                  state, x, None, _ws(shape, k_hi - k_lo))
        torch.cuda.synchronize()
        del keep
        return x.cpu().numpy()

    state = pl.new_state(N, d, "cuda")
    x = call(0, k, state)
    np.testing.assert_array_equal(np.concatenate([call(0, 16, None), call(16, k, None)]), x)
    x64 = x.astype(np.float64)
    mean, std, mn, mx = _finalize(state, N, d, 1)
    _close(mean, x64.mean(0), "mean")
    _close(std, x64.std(0, ddof=1), "std")
    np.testing.assert_array_equal(mn, x.min(0))
    np.testing.assert_array_equal(mx, x.max(0))


@pytest.mark.parametrize("prior_rng", ["host", "device"])
def test_api_with_a_row_count_instead_of_conditions(prior_rng):
    """a flow fitted without conditions takes C as a python int, as sample does"""
    from probaforms_amd.models import RealNVP
    rng = np.random.default_rng(7)
    torch.manual_seed(3)
    m = RealNVP(n_layers=8, hidden=(10,), batch_size=32, n_epochs=1, lr=1e-3, prior_rng=prior_rng)
    m.fit(rng.standard_normal((64, 5)).astype(np.float32))
    n = 21
    torch.manual_seed(5)
    s = m.sample_stats(n, K, quantiles=(0.5,))
    after = torch.get_rng_state()
    torch.manual_seed(5)
    loop = np.array([m.sample(n) for _ in range(K)])
    assert torch.equal(after, torch.get_rng_state())
    torch.manual_seed(5)
    many = m.sample_many(n, K)
    assert many.shape == loop.shape == (K, n, 5)
    _bar(many, loop)
    m64 = many.astype(np.float64)
    _close(s.mean, m64.mean(0), "mean")
    _close(s.std, m64.std(0), "std")
    _close(s.quantiles, np.quantile(m64, [0.5], axis=0), "quantiles")


@pytest.mark.parametrize("prior_rng", ["host", "device"])
@pytest.mark.parametrize("n", [N, 32])
def test_row_chunks_and_draw_windows_give_the_one_chunk_result(n, prior_rng, monkeypatch):
    """budgets small enough for three row chunks (quantiles) and three windows of draws (host prior): the generator ends where
    the one-chunk call leaves it, the draws' order statistics are bitwise the same, the moments agree to rounding"""
    from probaforms_amd.models import _predict as P
    m, d, c = _model("tm", prior_rng)
    C = np.random.default_rng(11).standard_normal((n, c)).astype(np.float32)
    probs = (0.0, 0.05, 0.5, 0.95, 1.0)
    torch.manual_seed(5)
    one = m.sample_stats(C, K, quantiles=probs, ddof=1)
    after = torch.get_rng_state()
    rows = (n + 2) // 3
    monkeypatch.setattr(P, "XT_CHUNK_BYTES", rows * d * K * 4)
    monkeypatch.setattr(P, "Z_WINDOW_BYTES", 8 * n * d * 4)
    assert len(P.quantile_row_chunks(n, d, K, P.XT_CHUNK_BYTES)) == 3 and len(P.draw_windows(K, n, d, P.Z_WINDOW_BYTES)) == 3
    torch.manual_seed(5)
    two = m.sample_stats(C, K, quantiles=probs, ddof=1)
    assert torch.equal(torch.get_rng_state(), after)
    np.testing.assert_array_equal(two.quantiles, one.quantiles)
    np.testing.assert_array_equal(two.min, one.min)
    np.testing.assert_array_equal(two.max, one.max)
    _close(two.mean, one.mean.astype(np.float64), "mean")
    _close(two.std, one.std.astype(np.float64), "std")
    torch.manual_seed(5)
    many = m.sample_many(C, K)                                        # (windows of draws, no row chunks)
    assert torch.equal(torch.get_rng_state(), after)
    np.testing.assert_array_equal(np.quantile(many.astype(np.float64), probs, axis=0).astype(np.float32), one.quantiles)
