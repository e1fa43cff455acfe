"""sample_scores: everything that needs no GPU -- argument validation, the numpy host route (scores_of_draws) against the
O(K^2) yardstick of tests/scores_numpy.py, the comparison rules themselves (numpy stand-ins for wrong kernels are rejected by
them on the series tests/test_scores_gpu.py feeds the kernel), the binding's refusals and pfp_scores' argument errors."""
import ctypes as C

import numpy as np
import pytest
import torch

import native_libs
import scores_numpy as SN
import scores_series as S
from probaforms_amd.models import _predict_lib

native_libs.ensure_built(_predict_lib)

KS = (1, 2, 3, 19, 256)
PROBS = (0.0, 0.05, 0.5, 0.95, 1.0)


def test_validate_scores():
    from probaforms_amd.models import _predict as P
    assert P.validate_scores(19, (0.05, 0.95)) == (19, (0.05, 0.95))
    assert P.validate_scores(1, None) == (1, None)
    assert P.validate_scores(8192, None) == (8192, None)
    assert P.validate_scores(5, 0.5) == (5, (0.5,))
    assert P.validate_scores(5, ()) == (5, None)
    for bad in (0, -3, 2.5):
        with pytest.raises(ValueError):
            P.validate_scores(bad)
    for quantiles in (None, (0.5,)):                                 # the series is always sorted
        with pytest.raises(ValueError):
            P.validate_scores(8193, quantiles)
    for q in (-0.01, 1.01, float("nan")):
        with pytest.raises(ValueError):
            P.validate_scores(10, (0.5, q))
    assert P.SampleScores._fields == ("crps", "pit", "quantiles", "pinball")


def _host(xt, y, probs, fair):
    from probaforms_amd.models import _predict as P
    s = P.scores_of_draws(np.moveaxis(xt, -1, 0), y, probs, fair)
    assert isinstance(s, P.SampleScores)
    for a in s:
        assert a is None or a.dtype == np.float32
    return s


@pytest.mark.parametrize("fair", [False, True])
@pytest.mark.parametrize("K", KS)
def test_scores_of_draws_on_finite_series(K, fair):
    for d in (1, 3):
        xt, y = S.finite(K, d)
        got, ref = _host(xt, y, PROBS, fair), SN.scores(xt, y, PROBS, fair)
        SN.check_all(got, ref, K, SN.scale_of(xt, y), (K, d, fair), quantiles_exact=True)
        assert got.crps.shape == got.pit.shape == (5, d) and got.quantiles.shape == got.pinball.shape == (len(PROBS), 5, d)
        if K == 1 and fair:
            assert np.isnan(got.crps).all()                          # 0 / 0, as the formula gives
        elif not fair:
            assert (got.crps >= 0).all()                             # (the fair estimate may fall below zero)
        assert ((got.pit >= 0) & (got.pit <= 1)).all()
        np.testing.assert_array_equal(got.pit[2, 0], np.float32(0.5))                # y tied with all K draws
        assert (got.pit[4, 0::2] == 1).all() and (got.pit[4, 1::2] == 0).all()       # y above / below every draw
    none = _host(xt, y, None, fair)
    assert none.quantiles is None and none.pinball is None
    np.testing.assert_array_equal(none.crps, got.crps)
    np.testing.assert_array_equal(none.pit, got.pit)


def _table(K, fair, crps, pit, q, pin):
    """the non-finite rules, spelled out for column 0 of scores_series.nonfinite(K)"""
    kind = {k: i for i, k in enumerate(S.NONFINITE_KINDS)}
    for k in ("+nan", "-nan", "nan and inf"):
        r = kind[k]
        assert np.isnan(crps[r]) and np.isnan(pit[r]) and np.isnan(q[:, r]).all() and np.isnan(pin[:, r]).all(), k
    r = kind["y nan"]
    assert np.isnan(crps[r]) and np.isnan(pit[r]) and np.isnan(pin[:, r]).all() and np.isfinite(q[:, r]).all()
    for k in ("+inf", "-inf", "both inf", "+inf and y +inf", "all +inf"):
        assert np.isnan(crps[kind[k]]) and np.isfinite(pit[kind[k]]), k
    undefined = K == 1 and fair
    assert np.isnan(crps[kind["y +inf"]]) if undefined else crps[kind["y +inf"]] == np.inf
    assert np.isnan(crps[kind["y -inf"]]) if undefined else crps[kind["y -inf"]] == np.inf
    assert pit[kind["y +inf"]] == 1 and pit[kind["y -inf"]] == 0
    assert pit[kind["all +inf"]] == 0
    assert pit[kind["-0 among +0, y +0"]] == 0.5 and pit[kind["-0 among +0, y -0"]] == 0.5
    if not undefined:
        assert crps[kind["-0 among +0, y +0"]] == 0 and np.isfinite(crps[kind["clean"]])


@pytest.mark.parametrize("fair", [False, True])
@pytest.mark.parametrize("K", KS)
def test_scores_of_draws_on_nonfinite_series(K, fair):
    xt, y = S.nonfinite(K)
    got, ref = _host(xt, y, PROBS, fair), SN.scores(xt, y, PROBS, fair)
    SN.check_all(got, ref, K, SN.scale_of(xt, y), (K, fair), quantiles_exact=True)
    _table(K, fair, got.crps[:, 0], got.pit[:, 0], got.quantiles[:, :, 0], got.pinball[:, :, 0])
    _table(K, fair, ref.crps[:, 0], ref.pit[:, 0], ref.quantiles[:, :, 0], ref.pinball[:, :, 0])
    for a in got:
        assert np.isfinite(a[..., 1]).all() or (K == 1 and fair)     # nothing leaves its (row, column)
    alone = _host(xt[:, 1:], y[:, 1:], PROBS, fair)
    for a, b in zip(got, alone):
        np.testing.assert_array_equal(a[..., 1:], b)


def test_scores_of_draws_refuses_a_wrong_target_shape():
    from probaforms_amd.models import _predict as P
    X = np.zeros((7, 4, 3), np.float32)
    for shape in ((4,), (3, 4), (4, 2), (1, 4, 3), (5, 3)):
        with pytest.raises(ValueError):
            P.scores_of_draws(X, np.zeros(shape, np.float32), None, False)
    s = P.scores_of_draws(np.zeros((7, 0, 3), np.float32), np.zeros((0, 3), np.float32), (0.5,), False)
    assert s.crps.shape == s.pit.shape == (0, 3) and s.quantiles.shape == s.pinball.shape == (1, 0, 3)
    t = P.scores_of_draws(X, torch.zeros(4, 3).numpy().tolist(), None, False)         # array-like targets
    assert (t.crps == 0).all() and (t.pit == 0.5).all()


# ---------------------------------------------------------------------------------------------------------------------------
# The comparison rules can fail: numpy stand-ins for wrong kernels are rejected by them, the right one passes.
# ---------------------------------------------------------------------------------------------------------------------------
WRONG = ("pit counts ties whole", "pit by sort key", "y nan overlooked", "fair ignored", "float32 sums", "pair sum not halved",
         "inf series not nan")


def _standin(xt, y, probs, fair, wrong=None):
    """k_scores' arithmetic in numpy: sort by the uint32 key, one pass over the sorted series, float64 sums, one rounding"""
    xt, y = np.asarray(xt, np.float32), np.asarray(y, np.float32)
    K = xt.shape[-1]
    b = xt.view(np.uint32)
    keys = np.where(b & 0x80000000, ~b, b | 0x80000000).astype(np.uint32)
    s32 = np.take_along_axis(xt, np.argsort(keys, axis=-1, kind="stable"), axis=-1)
    acc = np.float32 if wrong == "float32 sums" else np.float64
    s, yy = s32.astype(acc), y.astype(acc)[..., None]
    with np.errstate(all="ignore"):
        mid = s[..., K // 2:K // 2 + 1]
        mid = np.where(np.isfinite(mid), mid, 0).astype(acc)
        w = (2 * np.arange(K) - K + 1).astype(acc)
        s1 = np.abs(s - yy).sum(-1, dtype=acc).astype(np.float64)
        s2 = (w * ((s - mid) if wrong != "float32 sums" else s)).sum(-1, dtype=acc).astype(np.float64)
        D = K if (not fair or wrong == "fair ignored") else K - 1
        crps = s1 / K - (2.0 if wrong == "pair sum not halved" else 1.0) * s2 / (np.float64(K) * np.float64(D))
        nan = np.isnan(s32[..., 0]) | np.isnan(s32[..., K - 1])
        bad = nan if wrong == "y nan overlooked" else nan | np.isnan(y)
        if wrong != "inf series not nan":
            crps = np.where(np.isinf(s32[..., 0]) | np.isinf(s32[..., K - 1]), np.nan, crps)
        if wrong == "pit by sort key":
            yb = y.view(np.uint32)
            yk = np.where(yb & 0x80000000, ~yb, yb | 0x80000000).astype(np.uint32)[..., None]
            lt, eq = (np.sort(keys, -1) < yk).sum(-1), (np.sort(keys, -1) == yk).sum(-1)
        else:
            lt, eq = (s32 < y[..., None]).sum(-1), (s32 == y[..., None]).sum(-1)
        pit = (lt + (1.0 if wrong == "pit counts ties whole" else 0.5) * eq) / K
        crps, pit = np.where(bad, np.nan, crps), np.where(bad, np.nan, pit)
        q = np.quantile(s32.astype(np.float64), list(probs), axis=-1)
        q = np.where(nan, np.nan, q)
        p = np.asarray(probs, np.float64).reshape((-1,) + (1,) * y.ndim)
        pin = np.where(bad, np.nan, (y.astype(np.float64) - q) * (p - (y.astype(np.float64) < q)))
    return [a.astype(np.float32) for a in (crps, pit, q, pin)]


def _rejected(*args, **kw):
    try:
        SN.check_all(*args, **kw)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("fair", [False, True])
@pytest.mark.parametrize("K", [19, 256])
def test_rules_reject_wrong_stand_ins(K, fair):
    data = [S.finite(K, 3), S.nonfinite(K)]
    refs = [SN.scores(xt, y, PROBS, fair) for xt, y in data]
    for (xt, y), ref in zip(data, refs):
        SN.check_all(_standin(xt, y, PROBS, fair), ref, K, SN.scale_of(xt, y), "right")
    # where each wrong stand-in shows: (finite series, non-finite series)
    expect = {"pit counts ties whole": (True, True), "pit by sort key": (False, True), "y nan overlooked": (False, True),
              "fair ignored": (fair, fair), "float32 sums": (True, None), "pair sum not halved": (True, True),
              "inf series not nan": (False, None)}
    for wrong in WRONG:
        for i, ((xt, y), ref) in enumerate(zip(data, refs)):
            bad = _rejected(_standin(xt, y, PROBS, fair, wrong), ref, K, SN.scale_of(xt, y), wrong)
            if expect[wrong][i] is not None:
                assert bad == expect[wrong][i], (wrong, i, bad)


def test_rules_reject_an_infinite_series_that_is_not_nan():
    """a lone +inf above a finite y: S1 = inf and S2 = +inf give NaN by themselves; K = 1 and an all-infinite series with the
    middle shift do not, and the rule 'a series holding an infinity has crps NaN' has to be applied"""
    xt = np.full((1, 1, 4), np.inf, np.float32)
    y = np.zeros((1, 1), np.float32)
    ref = SN.scores(xt, y, PROBS, False)
    assert np.isnan(ref.crps).all()
    SN.check_all(_standin(xt, y, PROBS, False), ref, 4, SN.scale_of(xt, y), "right")
    got = _standin(xt, y, PROBS, False, "inf series not nan")
    assert _rejected(got, ref, 4, SN.scale_of(xt, y), "wrong") == (not np.isnan(got[0]).all())


# ---------------------------------------------------------------------------------------------------------------------------
# the binding and the C entry point, as far as no launch is needed
# ---------------------------------------------------------------------------------------------------------------------------
def test_binding_refuses_targets_off_the_device():
    from probaforms_amd.models import _predict_lib as pl
    xt = torch.zeros(2, 3, 5)
    for y in (torch.zeros(2, 3), torch.zeros(2, 3, dtype=torch.float64), np.zeros((2, 3), np.float32), None):
        with pytest.raises(RuntimeError, match="y "):
            pl.scores(xt, y, 2, 3, 5, False, None, None, None, None, None)


def test_pfp_scores_argument_errors_need_no_launch():
    from probaforms_amd.models import _predict_lib as pl
    fake = 4096                                   # never dereferenced: no call below reaches a launch
    probs = (C.c_double * 2)(0.05, 0.95)
    pp = C.cast(probs, C.c_void_p)

    def call(xt=fake, y=fake, n_rows=4, d=3, k=19, fair=0, p=pp, nq=2):
        return pl.lib().pfp_scores(None, xt, y, n_rows, d, k, fair, p, nq, fake, fake, fake, fake)
    assert call(xt=None) == -1 and call(y=None) == -1
    assert call(n_rows=-1) == -1 and call(d=0) == -1 and call(d=-2) == -1 and call(k=0) == -1 and call(k=-5) == -1
    assert call(p=None, nq=2) == -1 and call(nq=-1) == -1
    assert call(k=8193) == pl.EUNSUPPORTED and call(k=1 << 40) == pl.EUNSUPPORTED
    assert call(n_rows=0) == 0 and call(n_rows=0, p=None, nq=0) == 0          # zero series: ok without a launch
    assert call(n_rows=0, k=8193) == pl.EUNSUPPORTED                          # the checks come before the early return


def test_a_library_without_the_entry_point_is_reported_as_missing(monkeypatch):
    """a libpf_predict.so built before pfp_scores existed reports the same pfp_version(): lib() says rebuild, not AttributeError"""
    from probaforms_amd.models import _predict_lib as pl
    pl.LIBRARY.forget()
    monkeypatch.setitem(pl._SIGNATURES, "pfp_not_there", (C.c_int, []))
    with pytest.raises(pl.PredictLibraryMissing, match="rebuild"):
        pl.lib()
    assert pl.LIBRARY.loaded is False
