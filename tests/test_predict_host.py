"""Multi-draw predictive statistics (RealNVP.sample_stats / sample_many): everything that needs no GPU -- the binding against
the header's text, argument validation, the draw-window and row-chunk arithmetic, and the routing to the host loop."""
import os
import re

import numpy as np
import pytest
import torch

import native_libs
from probaforms_amd.models import _predict_lib

native_libs.ensure_built(_predict_lib)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "probaforms_amd", "models", "predict_csrc", "pf_predict.h")


def _header():
    with open(HEADER) as f:
        return f.read()


def test_exports_and_version_match_the_header_text():
    from probaforms_amd.models import _predict_lib as pl
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    declared = set(re.findall(r"\b(pfp_[a-z_]+)\s*\(", text))
    assert declared == set(pl.EXPORTS)
    for name, (_, args) in pl._SIGNATURES.items():
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, text)
        params = [p for p in m.group(1).split(",") if p.strip() and p.strip() != "void"]
        assert len(params) == len(args), name
    consts = dict(re.findall(r"#define\s+(PFP_[A-Z_]+)\s+\(?(-?\d+)\)?", _header()))
    assert int(consts["PFP_VERSION"]) == pl.ABI_VERSION == 101
    assert int(consts["PFP_STATE_BYTES"]) == pl.STATE_BYTES
    assert int(consts["PFP_MAX_QUANTILE_DRAWS"]) == pl.MAX_QUANTILE_DRAWS
    assert int(consts["PFP_EUNSUPPORTED"]) == pl.EUNSUPPORTED


def test_library_reports_the_version_and_has_every_export():
    from probaforms_amd.models import _predict_lib as pl
    L = pl.lib()
    assert L.pfp_version() == pl.ABI_VERSION
    for name in pl.EXPORTS:
        assert hasattr(L, name)
    assert L.pfp_status_string(0) == b"ok"


def test_supported_shapes_are_decided_on_the_host():
    from cases import CASES
    from probaforms_amd import _hip
    from probaforms_amd.models import _predict_lib as pl
    for name in ["c2", "c3", "c4", "tm", "tm_nocond", "reg1d", "relu_mh"]:
        L, d, c, hidden, act, _ = CASES[name]
        s = _hip.RnvpShape.make(L, d, c, hidden, act)
        assert pl.supported(s), name
        assert pl.workspace_bytes(s, 1000) >= 8000
    big = _hip.RnvpShape.make(8, 16, 4, (2048, 2048), "tanh")
    assert not pl.supported(big) and pl.workspace_bytes(big, 10) == 0


def test_validate():
    from probaforms_amd.models import _predict as P
    assert P.validate(19, (0.05, 0.95)) == (19, (0.05, 0.95))
    assert P.validate(1) == (1, None)
    assert P.validate(8192, [0.5]) == (8192, (0.5,))
    assert P.validate(100000, None) == (100000, None)
    assert P.validate(5, 0.5) == (5, (0.5,))
    for bad in (0, -3):
        with pytest.raises(ValueError):
            P.validate(bad)
    for q in (-0.01, 1.01, float("nan")):
        with pytest.raises(ValueError):
            P.validate(10, (0.5, q))
    with pytest.raises(ValueError):
        P.validate(8193, (0.5,))
    with pytest.raises(ValueError):
        P.validate(10, None, ddof=-1)
    with pytest.raises(ValueError):
        P.validate(2.5)


def test_draw_windows_cover_the_draws_within_the_budget():
    from probaforms_amd.models import _predict as P
    assert P.draw_windows(1000, 1000, 1) == [(0, 1000)]
    w = P.draw_windows(19, 37, 5, budget=37 * 5 * 4 * 8)
    assert w == [(0, 8), (8, 8), (16, 3)]
    assert P.draw_windows(3, 100, 4, budget=10) == [(0, 1), (1, 1), (2, 1)]          # one draw never splits
    n, d, K = 1 << 20, 16, 1000
    w = P.draw_windows(K, n, d)
    assert all(cnt * n * d * 4 <= P.Z_WINDOW_BYTES for _, cnt in w)
    assert [lo for lo, _ in w] == list(np.cumsum([0] + [cnt for _, cnt in w[:-1]])) and sum(cnt for _, cnt in w) == K


def test_quantile_row_chunks():
    from probaforms_amd.models import _predict as P
    assert P.quantile_row_chunks(0, 4, 100) == []
    assert P.quantile_row_chunks(1000, 1, 1000) == [(0, 1000)]
    c = P.quantile_row_chunks(10, 4, 100, budget=4 * 100 * 4 * 3)
    assert c == [(0, 3), (3, 3), (6, 3), (9, 1)]
    assert P.quantile_row_chunks(3, 4, 100, budget=1) == [(0, 1), (1, 1), (2, 1)]
    n, d, K = 100000, 16, 8192
    c = P.quantile_row_chunks(n, d, K)
    assert len(c) > 1 and all(m * d * K * 4 <= P.XT_CHUNK_BYTES for _, m in c) and sum(m for _, m in c) == n


def _flow(hiddens, prior="std"):
    from probaforms_amd.models.nflow import NormalizingFlow, StandardNormalPrior
    from probaforms_amd.models.realnvp import RealNVPLayer
    d = 3
    layers = [RealNVPLayer(d, 2, (torch.arange(d) + i) % 2, hidden=h) for i, h in enumerate(hiddens)]
    pr = StandardNormalPrior(d, "cpu") if prior == "std" else torch.distributions.MultivariateNormal(torch.zeros(d), torch.eye(d))
    return NormalizingFlow(layers, pr)


def test_route():
    from probaforms_amd.models import _predict as P
    assert P.route(_flow([(8,), (8,)])) == "kernel"
    assert P.route(_flow([(8,), (8,)]), lambda: True) == "kernel"
    assert P.route(_flow([(8,), (8,)]), lambda: False) == "shape"
    assert P.route(_flow([(8,), (12,)])) == "layerwise"
    assert P.route(_flow([(8,), (8,)], prior="user")) == "prior"


def test_fallback_is_the_notebook_loop():
    """a flow the kernels do not serve: sample_stats / sample_many are self.sample n_draws times plus numpy"""
    from probaforms_amd.models import RealNVP
    from probaforms_amd.models import _predict as P
    m = RealNVP()
    m.nf = _flow([(8,), (12,)])
    rng = np.random.default_rng(3)
    calls = []

    def fake_sample(C):
        calls.append(len(C))
        return rng.standard_normal((len(C), 3)).astype(np.float32)

    m.sample = fake_sample
    C = np.zeros((4, 2), np.float32)
    s = m.sample_stats(C, 7, quantiles=(0.05, 0.95), ddof=1)
    assert calls == [4] * 7
    rng = np.random.default_rng(3)
    X = np.array([rng.standard_normal((4, 3)).astype(np.float32) for _ in range(7)])
    np.testing.assert_array_equal(s.mean, X.astype(np.float64).mean(0).astype(np.float32))
    np.testing.assert_array_equal(s.std, X.astype(np.float64).std(0, ddof=1).astype(np.float32))
    np.testing.assert_array_equal(s.min, X.min(0))
    np.testing.assert_array_equal(s.max, X.max(0))
    np.testing.assert_array_equal(s.quantiles, np.quantile(X.astype(np.float64), [0.05, 0.95], axis=0).astype(np.float32))
    assert s.mean.dtype == np.float32 and s.quantiles.shape == (2, 4, 3)
    rng = np.random.default_rng(3)
    np.testing.assert_array_equal(m.sample_many(C, 7), X)
    with pytest.raises(ValueError):
        m.sample_stats(C, 0)
    with pytest.raises(ValueError):
        m.sample_stats(C, 9000, quantiles=(0.5,))


def test_draw_accumulate_checks_rows_and_draws_before_any_launch():
    """row_offset + n_rows <= n_total and k_lo + k_cnt <= k_total on every call, whichever outputs are asked for"""
    import ctypes as C
    from probaforms_amd import _hip
    from probaforms_amd.models import _predict_lib as pl
    s = _hip.RnvpShape.make(2, 3, 0, (8,), "tanh", alt_masks=1)
    seeds = (C.c_uint64 * 4)(1, 2, 3, 4)
    fake = 4096                                   # never dereferenced: the calls below fail their argument checks

    def call(n_rows, row_offset, n_total, k_lo, k_cnt, k_total):
        return pl.lib().pfp_draw_accumulate(None, C.byref(s), fake, None, None, n_rows, row_offset,
                                            C.cast(seeds, C.c_void_p), None, n_total, k_lo, k_cnt, k_total, None, None, None,
                                            fake, 4096)
    assert call(5, 3, 7, 0, 4, 4) == -1           # rows 3 .. 8 of 7
    assert call(5, 3, 8, 2, 4, 5) == -1           # draws 2 .. 6 of 5
    assert call(5, 3, 8, 0, 0, 4) == -1
    assert call(-1, 0, 8, 0, 4, 4) == -1


# ---------------------------------------------------------------------------------------------------------------------------
# The comparison rules of tests/test_predict_edges_gpu.py can fail: numpy stand-ins for wrong kernels are rejected by them on
# the series that file feeds the kernels, and the host route (stats_of_draws) passes.
# ---------------------------------------------------------------------------------------------------------------------------
def _standin_moments(x, windows, ddof, shift, nan_minmax):
    """pf_predict.hip's k_draw / k_finalize arithmetic over x [K, ...] in numpy: float64 sums of (x - shift) and its square,
    16-draw tile by tile.  shift: 'first' (the first draw, whatever it is), 'finite' (0 when that draw is not finite) or
    'none' (plain sums).  nan_minmax: numpy's min / max, else fmin / fmax (which drop NaN)."""
    x = np.asarray(x, np.float32)
    x64 = x.astype(np.float64)
    with np.errstate(all="ignore"):
        sh = {"first": x64[0], "finite": np.where(np.isfinite(x64[0]), x64[0], 0.0), "none": np.zeros_like(x64[0])}[shift]
        s, ss, cnt = np.zeros_like(sh), np.zeros_like(sh), 0
        for lo, hi in windows:
            for t0 in range(lo, hi, 16):
                dv = x64[t0:min(hi, t0 + 16)] - sh
                s, ss, cnt = s + dv.sum(0), ss + (dv * dv).sum(0), cnt + len(dv)
        q = ss - s * s / cnt
        q = np.where(q < 0.0, 0.0, q)
        std = np.sqrt(q / (cnt - ddof)) if cnt > ddof else np.full_like(q, np.nan)
        if nan_minmax:
            mn, mx = x.min(0), x.max(0)
        else:                                             # folded into a state that starts at +inf / -inf
            mn, mx = np.fmin(np.float32(np.inf), np.fmin.reduce(x, axis=0)), np.fmax(np.float32(-np.inf), np.fmax.reduce(x, axis=0))
        return [a.astype(np.float32) for a in (sh + s / cnt, std, mn, mx)]


def _standin_quantiles(xt, probs, nan_check):
    """k_quantiles in numpy: sort by the kernel's uint32 key (negative NaNs first, positive NaNs last), numpy's lerp in float64"""
    xt = np.asarray(xt, np.float32)
    K = xt.shape[-1]
    b = xt.view(np.uint32)
    keys = np.where(b & 0x80000000, ~b, b | 0x80000000).astype(np.uint32)
    srt = np.take_along_axis(xt, np.argsort(keys, axis=-1, kind="stable"), axis=-1).astype(np.float64)
    out = np.empty((len(probs),) + xt.shape[:-1], np.float32)
    with np.errstate(all="ignore"):
        for i, p in enumerate(probs):
            pos = p * (K - 1)
            fl = min(max(np.floor(pos), 0.0), K - 1.0)
            lo, t = int(fl), pos - fl
            a, bb = srt[..., lo], srt[..., min(lo + 1, K - 1)]
            diff = bb - a
            res = bb - diff * (1.0 - t) if t >= 0.5 else a + diff * t
            res = np.where(diff == 0.0, a, res)
            if nan_check:
                res = np.where(np.isnan(srt[..., 0]) | np.isnan(srt[..., K - 1]), np.nan, res)
            out[i] = res
    return out


def _rejected(check, *args):
    try:
        check(*args)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("K", [19, 40])
def test_edge_rules_reject_fmin_fmax_and_a_non_finite_shift(K):
    import predict_edge_series as E
    from probaforms_amd.models import _predict as P
    x = E.nonfinite(K)
    for ddof in (0, 1):
        for w in E.windows_of(K):
            today = _standin_moments(x, w, ddof, "first", False)
            fixed = _standin_moments(x, w, ddof, "finite", True)
            E.check_moments(fixed, x, ddof, "fixed")
            assert _rejected(E.check_moments, today, x, ddof, "today")
            for j, kind in enumerate(E.NONFINITE_KINDS):
                bad = _rejected(E.check_moments, [a[:, j] for a in today], x[:, :, j], ddof, kind)
                # fmin / fmax lose every NaN; an infinite first draw turns the shifted sums into NaN; an infinity met later,
                # and the two zeros, are right either way
                assert bad == (j <= 6), (kind, bad)
            np.testing.assert_array_equal(fixed[0][:, 9], np.zeros(3, np.float32))
        s = P.stats_of_draws(x, None, ddof)
        E.check_moments([s.mean, s.std, s.min, s.max], x, ddof, "stats_of_draws")


@pytest.mark.parametrize("K", [3, 4, 5, 17, 4097, 8191])
def test_edge_rules_reject_quantiles_that_overlook_a_nan(K):
    import predict_edge_series as E
    from probaforms_amd.models import _predict as P
    xt, probs = E.quantile_series(K)
    want = E.quantile_reference(xt, probs)
    assert np.isnan(want[:, 0, 1]).all() and np.isnan(want[:, 1, 0]).all()      # a NaN of either sign: every quantile
    E.same(_standin_quantiles(xt, probs, True), want, "fixed")
    today = _standin_quantiles(xt, probs, False)
    for r in range(3):
        for j in range(2):
            kind = E.QUANTILE_KINDS[2 * r + j]
            assert _rejected(E.same, today[:, r, j], want[:, r, j], kind) == (kind in ("+nan", "-nan")), kind
    s = P.stats_of_draws(np.moveaxis(xt, -1, 0), probs, 0)
    E.same(s.quantiles, want, "stats_of_draws")


@pytest.mark.parametrize("K", [1, 2, 15, 16, 17, 19, 40, 65, 1000])
def test_edge_rules_reject_unshifted_sums(K):
    import predict_edge_series as E
    from probaforms_amd.models import _predict as P
    x = E.conditioned(K)
    assert np.isfinite(x).all() and (np.abs(x) > 1e-30).all()
    for ddof in (0, 1):
        for w in E.windows_of(K):
            E.check_moments(_standin_moments(x, w, ddof, "finite", True), x, ddof, "shifted")
            plain = _standin_moments(x, w, ddof, "none", True)
            # the float64 sums of x and x^2 lose the variance of a series whose mean is 10^6 .. 10^7 standard deviations; with
            # few draws, or the two-valued series at an even count, those sums can still come out exact
            for j in ((0, 1, 4) if K in (19, 65, 1000) else ((0,) if K >= 15 else ())):
                assert _rejected(E.check_moments, [a[:, j] for a in plain], x[:, :, j], ddof, E.CONDITIONED_KINDS[j])
        s = P.stats_of_draws(x, None, ddof)
        E.check_moments([s.mean, s.std, s.min, s.max], x, ddof, "stats_of_draws")
