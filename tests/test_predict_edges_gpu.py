"""libpf_predict.so (models/predict_csrc/pf_predict.h) at its edges: non-finite and badly conditioned series against numpy in
float64, Linear geometries off the fixtures against the float64 oracle, the NULL mask table, the second iteration of both
grid-stride loops, and the bounds of every output.  Runs on the GPU box: `pytest -m gpu`.

Identity flow.  With a mask table of all ones every feature passes through every layer, so on the z path k_draw writes
x == z bit for bit whatever the parameters are: pfp_draw_accumulate + pfp_finalize can be fed any float32 series.  Every test
that relies on it first asserts x_out == z on the uint32 view; numpy is then taken over exactly what the kernel accumulated.

Rules (tests/predict_edge_series.py, shown able to fail by tests/test_predict_host.py): NaN in the same places, infinities
equal, elsewhere mean / std / quantiles within 2 float32 ulps of the float64 value (test_predict_gpu._close), min / max exact.

Geometry cases: n rows, K = 19 draws (and 40 where noted) on the seed path from global row 11, alternating table unless
`user`.  e32 = mean |oracle32 - oracle64| / max(1, mean |oracle64|) is the float32 restatement's own error on the same draws,
`kernel` the same figure for k_draw; the bar is max(5e-6, 4 e32), which is 5e-6 for every case below.  Measured on an
MI355X:

    (L, d, c, hidden, act)            n   K   table   e32        kernel
    (1, 2, 0, (4,), tanh)             37  19  alt     3.17e-08   4.76e-08
    (2, 3, 1, (15,), tanh)            37  19  alt     3.56e-08   4.81e-08
    (2, 4, 1, (16,), relu)            37  19  alt     3.56e-08   4.46e-08
    (2, 5, 5, (17,), tanh)            37  19  alt     4.83e-08   6.37e-08
    (2, 5, 5, (17,), tanh)            37  19  user    5.82e-08   7.54e-08
    (3, 17, 2, (33,), tanh)           37  19  alt     6.15e-08   7.72e-08
    (2, 6, 2, (7, 20, 5), relu)       37  19  alt     3.46e-08   4.19e-08
    (2, 6, 2, (7, 20, 5), relu)       37  19  user    3.14e-08   3.87e-08
    (2, 4, 0, (8, 8, 8), tanh)        37  19  alt     3.49e-08   5.42e-08
    (4, 16, 4, (64,), tanh)           37  19  alt     9.22e-08   1.08e-07
    (4, 16, 4, (64,), tanh)           37  40  alt     8.68e-08   1.00e-07
    (2, 4, 1, (8,) x 8, relu)         21  19  alt     3.41e-08   4.70e-08
"""
import functools

import numpy as np
import pytest
import torch

import native_libs
import predict_edge_series as E
from probaforms_amd.models import _predict_lib
from test_predict_gpu import K, N, ROW0, _close, _dev, _finalize, _model, _setup, _ws

pytestmark = pytest.mark.gpu

native_libs.ensure_built(_predict_lib)

SENTINEL = 0xFFC0DEAD                                                # a NaN payload no arithmetic here produces


def _shape(L, d, c, hidden, act, alt_masks=0):
    from probaforms_amd import _hip
    return _hip.RnvpShape.make(L, d, c, hidden, act, alt_masks=alt_masks)


def _params(L, d, c, hidden, seed):
    """as cases.numpy_params: U(-1/sqrt(fan_in), 1/sqrt(fan_in)) in nf.parameters() order, seeded PCG64"""
    from cases import linear_shapes
    rng = np.random.default_rng(seed)
    parts = []
    for _ in range(2 * L):
        for o, i in linear_shapes(d, c, hidden):
            b = 1.0 / np.sqrt(i)
            parts += [rng.uniform(-b, b, size=o * i), rng.uniform(-b, b, size=o)]
    return np.concatenate(parts).astype(np.float32)


def _call(shape, params, masks, c, n, row0, seeds, z, n_total, k_lo, k_cnt, k_total, state=None, x=None, xt=None):
    from probaforms_amd.models import _predict_lib as pl
    keep = pl.draw_accumulate(shape, params, masks, c, n, row0, seeds, z, n_total, k_lo, k_cnt, k_total, state, x, xt,
                              _ws(shape, k_cnt))
    torch.cuda.synchronize()
    del keep


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------------------
# the identity flow: moments of any series
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _identity(d):
    L, hidden = 2, (4,)
    return _shape(L, d, 0, hidden, "tanh"), _dev(_params(L, d, 0, hidden, 5)), _dev(np.ones((L, d)), torch.uint8)


def _identity_moments(z, windows):
    """z [K, n, d] float32 through the identity flow in the given draw windows -> (state, {ddof: (mean, std, min, max)})"""
    from probaforms_amd.models import _predict_lib as pl
    k, n, d = z.shape
    shape, params, ones = _identity(d)
    zd = _dev(z)
    state = pl.new_state(n, d, "cuda")
    x = torch.empty(k, n, d, device="cuda")
    for lo, hi in windows:
        _call(shape, params, ones, None, n, 0, None, zd[lo:hi].contiguous(), n, lo, hi - lo, k, state, x[lo:hi])
    np.testing.assert_array_equal(_bits(x.cpu().numpy()), _bits(z))                  # what was accumulated is z itself
    return state, {ddof: _finalize(state, n, d, ddof) for ddof in (0, 1)}


@pytest.mark.parametrize("k", E.CONDITIONED_K)
def test_conditioned_moments_vs_numpy_float64(k):
    z = E.conditioned(k)
    assert np.isfinite(z).all() and (np.abs(z) >= 2.0 ** -126).all()
    for w in E.windows_of(k):
        got = _identity_moments(z, w)[1]
        for ddof in (0, 1):
            E.check_moments(got[ddof], z, ddof, (k, len(w), ddof))


@pytest.mark.parametrize("k", [19, 40])
def test_nonfinite_moments_vs_numpy_float64(k):
    z = E.nonfinite(k)
    zc = E.clean_like(z)
    assert np.isfinite(zc).all() and np.isfinite(z[:, :, 10]).all()
    for w in E.windows_of(k):
        state, got = _identity_moments(z, w)
        state_c, got_c = _identity_moments(zc, w)
        for ddof in (0, 1):
            for j, kind in enumerate(E.NONFINITE_KINDS + ("clean",)):
                E.check_moments([a[:, j] for a in got[ddof]], z[:, :, j], ddof, (k, len(w), ddof, kind))
            for a in got[ddof]:
                np.testing.assert_array_equal(a[:, 9], np.zeros(z.shape[1], np.float32))       # -0 among +0: either zero
            # the clean series is untouched by its neighbours' NaNs and infinities
            for a, b in zip(got[ddof], got_c[ddof]):
                np.testing.assert_array_equal(_bits(a[:, 10]), _bits(b[:, 10]))
        assert torch.equal(state[:, 10], state_c[:, 10])


# ---------------------------------------------------------------------------------------------------------------------------
# quantiles
# ---------------------------------------------------------------------------------------------------------------------------
def _quantiles(xt, probs):
    from probaforms_amd.models import _predict_lib as pl
    n, d, k = xt.shape
    q = torch.empty(len(probs), n, d, device="cuda")
    xd = _dev(xt)
    np.testing.assert_array_equal(_bits(xd.cpu().numpy()), _bits(xt))                 # NaN signs and payloads reached the device
    pl.quantiles(xd, n, d, k, torch.tensor(probs, dtype=torch.float64, device="cuda"), q)
    return q.cpu().numpy()


@pytest.mark.parametrize("k", E.QUANTILE_K)
def test_nonfinite_and_awkward_quantiles_vs_numpy(k):
    xt, probs = E.quantile_series(k)
    got, want = _quantiles(xt, probs), E.quantile_reference(xt, probs)
    for r in range(3):
        for j in range(2):
            E.same(got[:, r, j], want[:, r, j], (k, E.QUANTILE_KINDS[2 * r + j]))


def test_quantiles_grid_stride():
    """65536 + 5 series: five workgroups sort a second series"""
    n, k = 65536 + 5, 5
    xt = (np.random.default_rng(8).standard_normal((n, 1, k)) * 3 + 1).astype(np.float32)
    probs = [0.0, 0.05, 0.5, 0.95, 1.0]
    got, want = _quantiles(xt, probs), E.quantile_reference(xt, probs)
    _close(got, want, "quantiles")
    np.testing.assert_array_equal(got[0], xt.min(-1))
    np.testing.assert_array_equal(got[-1], xt.max(-1))


# ---------------------------------------------------------------------------------------------------------------------------
# the public call with a NaN condition row: the kernel route and the host route agree
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prior_rng", ["host", "device"])
def test_api_nan_condition_row_matches_the_host_route(prior_rng):
    from probaforms_amd.models import _predict as P
    m, d, c = _model("tm", prior_rng)
    C = np.random.default_rng(11).standard_normal((N, c)).astype(np.float32)
    bad = 5
    C[bad, 1] = np.nan
    clean = np.arange(N) != bad
    probs = (0.05, 0.95)
    torch.manual_seed(5)
    s = m.sample_stats(C, K, quantiles=probs)
    torch.manual_seed(5)
    many = m.sample_many(C, K)
    host = P.stats_of_draws(many, probs, 0)
    assert np.isnan(many[:, bad]).all() and np.isfinite(many[:, clean]).all()
    for name in ("mean", "std", "min", "max", "quantiles"):
        got, want = getattr(s, name), getattr(host, name)
        assert np.array_equal(np.isnan(got), np.isnan(want)), name
        assert np.isnan(got[..., bad, :]).all() and np.isfinite(got[..., clean, :]).all(), name
    m64 = many[:, clean].astype(np.float64)
    _close(s.mean[clean], m64.mean(0), "mean")
    _close(s.std[clean], m64.std(0), "std")
    np.testing.assert_array_equal(s.min[clean], many[:, clean].min(0))
    np.testing.assert_array_equal(s.max[clean], many[:, clean].max(0))
    _close(s.quantiles[:, clean], np.quantile(m64, probs, axis=0), "quantiles")


# ---------------------------------------------------------------------------------------------------------------------------
# Linear geometries off the fixtures, against the float64 oracle
# ---------------------------------------------------------------------------------------------------------------------------
GEOMETRY = [
    # L, d, c, hidden, act, n, K, table
    (1, 2, 0, (4,), "tanh", 37, 19, "alt"),
    (2, 3, 1, (15,), "tanh", 37, 19, "alt"),
    (2, 4, 1, (16,), "relu", 37, 19, "alt"),
    (2, 5, 5, (17,), "tanh", 37, 19, "alt"),
    (2, 5, 5, (17,), "tanh", 37, 19, "user"),
    (3, 17, 2, (33,), "tanh", 37, 19, "alt"),            # d > 16: two output tiles in the last Linear
    (2, 6, 2, (7, 20, 5), "relu", 37, 19, "alt"),        # three hidden layers: the ping-pong returns to H0
    (2, 6, 2, (7, 20, 5), "relu", 37, 19, "user"),
    (2, 4, 0, (8, 8, 8), "tanh", 37, 19, "alt"),
    (4, 16, 4, (64,), "tanh", 37, 19, "alt"),
    (4, 16, 4, (64,), "tanh", 37, 40, "alt"),
    (2, 4, 1, (8,) * 8, "relu", 21, 19, "alt"),          # RNVP_MAX_HIDDEN levels
]


def _table(L, d, kind):
    if kind == "alt":
        return ((np.arange(d)[None, :] + np.arange(L)[:, None]) % 2).astype(np.uint8)
    first = np.arange(d) < (d + 1) // 2                   # the first ceil(d / 2) features pass in even layers, the rest in odd ones
    return np.stack([first if l % 2 == 0 else ~first for l in range(L)]).astype(np.uint8)


@pytest.mark.parametrize("L,d,c,hidden,act,n,k,table", GEOMETRY)
def test_geometry_vs_float64_oracle(L, d, c, hidden, act, n, k, table, oracle32, oracle64):
    from oracle import Shape
    from probaforms_amd.models import _predict_lib as pl
    idx = GEOMETRY.index((L, d, c, hidden, act, n, k, table))
    params, masks = _params(L, d, c, hidden, 100 + idx), _table(L, d, table)
    rng = np.random.default_rng(200 + idx)
    Cn = rng.standard_normal((n, c)).astype(np.float32) if c else None
    seeds = [int(v) for v in rng.integers(0, 2 ** 64, size=k, dtype=np.uint64)]
    shape = _shape(L, d, c, hidden, act)
    x = torch.empty(k, n, d, device="cuda")
    xt = torch.empty(n, d, k, device="cuda")
    state = pl.new_state(n, d, "cuda")
    _call(shape, _dev(params), _dev(masks, torch.uint8), _dev(Cn), n, ROW0, seeds, None, ROW0 + n, 0, k, k, state, x, xt)
    x = x.cpu().numpy()
    so = Shape.make(L, d, c, hidden, act)
    want = np.stack([oracle64.sample(so, params, oracle64.prior_normal(s, ROW0, n, d), Cn, masks) for s in seeds])
    x32 = np.stack([oracle32.sample(so, params, oracle32.prior_normal(s, ROW0, n, d), Cn, masks) for s in seeds])
    scale = max(1.0, np.abs(want).mean())
    e32 = np.abs(x32 - want).mean() / scale
    err = np.abs(x - want).mean() / scale
    bar = max(5e-6, 4.0 * e32)                                      # test_predict_gpu._bar with max(5e-6, 4 e32) for its 5e-6
    print("geometry %s n=%d K=%d %s: e32 %.2e kernel %.2e bar %.2e" % ((L, d, c, hidden, act), n, k, table, e32, err, bar))
    assert np.isfinite(x).all()
    assert err < bar, (err, e32, bar)
    np.testing.assert_array_equal(xt.cpu().numpy(), np.transpose(x, (1, 2, 0)))
    x64 = x.astype(np.float64)
    mean, std, mn, mx = _finalize(state, n, d, 1)
    _close(mean, x64.mean(0), "mean")
    _close(std, x64.std(0, ddof=1), "std")
    np.testing.assert_array_equal(mn, x.min(0))
    np.testing.assert_array_equal(mx, x.max(0))


# ---------------------------------------------------------------------------------------------------------------------------
# masks == NULL with alt_masks 1 or 2
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,hidden,act", [(2, (10,), "tanh"), (0, (7, 9), "relu")])
def test_null_mask_table_is_the_alternating_table_bitwise(c, hidden, act):
    from probaforms_amd.models import _predict_lib as pl
    L, d, n = 3, 5, N
    params = _dev(_params(L, d, c, hidden, 31))
    rng = np.random.default_rng(32)
    Cd = _dev(rng.standard_normal((n, c)).astype(np.float32)) if c else None
    seeds = [int(v) for v in rng.integers(0, 2 ** 64, size=K, dtype=np.uint64)]

    def run(masks, alt):
        x, xt = torch.empty(K, n, d, device="cuda"), torch.empty(n, d, K, device="cuda")
        state = pl.new_state(n, d, "cuda")
        _call(_shape(L, d, c, hidden, act, alt_masks=alt), params, masks, Cd, n, ROW0, seeds, None, ROW0 + n, 0, K, K, state,
              x, xt)
        return x, xt, state

    for alt in (1, 2):
        table = ((np.arange(d)[None, :] + np.arange(L)[:, None] + (alt == 2)) & 1).astype(np.uint8)     # as mask_of reads it
        a, b = run(None, alt), run(_dev(table, torch.uint8), 0)
        assert np.isfinite(a[0].cpu().numpy()).all()
        for u, v in zip(a, b):
            assert torch.equal(u.view(torch.int32) if u.dtype == torch.float32 else u,
                               v.view(torch.int32) if v.dtype == torch.float32 else v)
    assert not torch.equal(run(None, 1)[0], run(None, 2)[0])
    with pytest.raises(RuntimeError):
        run(None, 0)


# ---------------------------------------------------------------------------------------------------------------------------
# the second iteration of k_draw's grid-stride loop
# ---------------------------------------------------------------------------------------------------------------------------
def test_draw_grid_stride_rows_match_a_call_on_those_rows_alone():
    """65536 + 37 rows: workgroups 0 .. 36 pick up a second row.  The rows on both sides of the seam, and the first rows
    (whose workgroups go on to a second row), equal bitwise a call on those rows alone with the matching row_offset."""
    from probaforms_amd.models import _predict_lib as pl
    L, d, c, hidden, k = 2, 2, 1, (4,), 3
    n = 65536 + 37
    shape, params = _shape(L, d, c, hidden, "tanh"), _dev(_params(L, d, c, hidden, 41))
    masks = _dev(_table(L, d, "alt"), torch.uint8)
    rng = np.random.default_rng(42)
    Cd = _dev(rng.standard_normal((n, c)).astype(np.float32))
    seeds = [int(v) for v in rng.integers(0, 2 ** 64, size=k, dtype=np.uint64)]

    def run(lo, hi):
        m = hi - lo
        x, state = torch.empty(k, m, d, device="cuda"), pl.new_state(m, d, "cuda")
        _call(shape, params, masks, Cd[lo:hi].contiguous(), m, ROW0 + lo, seeds, None, ROW0 + n, 0, k, k, state, x)
        return x, state

    x, state = run(0, n)
    assert torch.isfinite(x).all()
    for lo, hi in ((n - 37 - 16, n), (0, 16)):
        xs, ss = run(lo, hi)
        assert torch.equal(xs.view(torch.int32), x[:, lo:hi].view(torch.int32))
        assert torch.equal(ss, state[lo:hi])
    x64 = x.cpu().numpy().astype(np.float64)
    mean, std, mn, mx = _finalize(state, n, d, 0)
    _close(mean, x64.mean(0), "mean")
    _close(std, x64.std(0), "std")
    np.testing.assert_array_equal(mn, x64.min(0).astype(np.float32))
    np.testing.assert_array_equal(mx, x64.max(0).astype(np.float32))


# ---------------------------------------------------------------------------------------------------------------------------
# output bounds
# ---------------------------------------------------------------------------------------------------------------------------
GUARD = 256                                                          # bytes in front of and behind every array


def _guarded(shape, dtype=torch.float32, fill=True):
    """an array of `shape` at a 256-byte-aligned offset inside a larger buffer of sentinel words -> (array, whole buffer)"""
    item = torch.empty((), dtype=dtype).element_size()
    nbytes = int(np.prod(shape)) * item
    inner = (nbytes + GUARD - 1) // GUARD * GUARD
    buf = torch.full(((2 * GUARD + inner) // 4,), SENTINEL - (1 << 32), dtype=torch.int32, device="cuda")
    arr = buf.view(torch.uint8)[GUARD:GUARD + nbytes].view(dtype).view(shape)
    assert arr.data_ptr() % 256 == 0 and arr.is_contiguous()
    if not fill:
        arr.zero_()
    return arr, buf


def _guards_intact(arr, buf):
    words = buf.cpu().numpy().view(np.uint32)
    nwords = arr.numel() * arr.element_size() // 4
    lo, hi = GUARD // 4, GUARD // 4 + nwords
    assert (words[:lo] == SENTINEL).all() and (words[hi:] == SENTINEL).all()
    return words[lo:hi]


@pytest.mark.parametrize("name", ["tm", "c2"])
@pytest.mark.parametrize("ks", [(0, K), (8, K)])
def test_outputs_stay_inside_their_arrays(name, ks):
    cs, shape, params, masks, Cn, seeds = _setup(name)
    d, (k_lo, k_hi) = cs["d"], ks
    kc = k_hi - k_lo
    x, xb = _guarded((kc, N, d))
    xt, xtb = _guarded((N, d, K))
    st, stb = _guarded((N, d, 32), torch.uint8, fill=False)           # a state is read: all zero = nothing seen yet
    _call(shape, params, masks, _dev(Cn), N, ROW0, seeds[k_lo:k_hi], None, ROW0 + N, k_lo, kc, K, st, x, xt)
    outs = [_guarded((N, d)) for _ in range(4)]
    from probaforms_amd.models import _predict_lib as pl
    pl.finalize(st, N, d, 0, *[o[0] for o in outs])
    torch.cuda.synchronize()
    assert (_guards_intact(x, xb) != SENTINEL).all()
    xtw = _guards_intact(xt, xtb).reshape(N, d, K)
    assert (xtw[:, :, k_lo:k_hi] != SENTINEL).all()
    assert (xtw[:, :, :k_lo] == SENTINEL).all() and (xtw[:, :, k_hi:] == SENTINEL).all()
    np.testing.assert_array_equal(xt.cpu().numpy()[:, :, k_lo:k_hi], np.transpose(x.cpu().numpy(), (1, 2, 0)))
    stw = _guards_intact(st, stb).reshape(N, d, 8)
    assert (stw[:, :, 7] == kc).all()                                 # count, the last word of every state
    for arr, buf in outs:
        assert (_guards_intact(arr, buf) != SENTINEL).all()
        assert torch.isfinite(arr).all()
