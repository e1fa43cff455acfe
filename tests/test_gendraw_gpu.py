"""libpf_gendraw.so (models/gendraw_csrc/pf_gendraw.h) and sample_stats / sample_many of CVAE, ConditionalWGAN and
ConditionalNormal on the GPU: the draws against the same MLP / affine map in float64 on the CPU, the moments and quantiles
against numpy in float64, split invariance, determinism, NaN containment, workspace hygiene, and the public calls against the
notebook loop they replace.  Runs on the GPU box: `pytest -m gpu`.

Shapes: n = 37 rows (not a multiple of 16 or of the 4 waves) and K = 19 draws (crosses one 16-draw tile), rows 11 .. 48 of a
job of 57.  Tolerances: the draws meet the bar tests/test_hip_kernels.py sets for the sampling kernels (mean |err| < 5e-6 *
max(1, mean |want|)); mean / std / quantiles are float64 arithmetic rounded once to float32, compared at 2 float32 ulps
(rtol 2.4e-7); min / max are exact."""
import functools

import numpy as np
import pytest
import torch

import hygiene
import native_libs
import predict_edge_series as E
from cnormal_torch import Normal
from probaforms_amd.models import _cnormal_lib, _gendraw_lib, _predict_lib, _wgan_lib
from wgan_torch import Net

pytestmark = pytest.mark.gpu

native_libs.ensure_built(_cnormal_lib, _gendraw_lib, _predict_lib, _wgan_lib)

N, K, ROW0 = 37, 19, 11
N_TOTAL = N + 20
ULP2 = 2.4e-7
PROBS = (0.0, 0.05, 0.5, 0.95, 1.0)

# (d, c, latent, hidden, act)
WIDE = (3, 2, 2, (256, 256), "tanh")                      # its packed weights do not fit the LDS
MLP_CASES = [(5, 3, 1, (100, 100), "relu"), (5, 3, 2, (10,), "tanh"), (5, 0, 2, (10,), "tanh"), (16, 4, 2, (128,), "tanh"),
             (4, 2, 3, (7, 9), "relu"), (17, 2, 5, (33,), "tanh"), (1, 1, 1, (10,), "tanh"), WIDE]
SMALL = (5, 3, 2, (10,), "tanh")
_ids = lambda c: "d%d-c%d-l%d-%s-%s" % (c[0], c[1], c[2], "x".join(map(str, c[3])), c[4])


def _dev(a, dtype=torch.float32):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a)).to(dtype).cuda().contiguous()


def _close(got, want, what):
    """within 2 float32 ulps of the float64 value"""
    err = np.abs(np.asarray(got, np.float64) - want)
    assert (err <= ULP2 * np.abs(want)).all(), (what, float(err.max()))


def _bar(got, want):
    err = np.abs(got - want)
    assert np.isfinite(got).all()
    assert err.mean() < 5e-6 * max(1.0, np.abs(want).mean()), err.mean()



@functools.lru_cache(maxsize=None)
def _setup(case, k_total=K):
    """the net of the binding, flat parameters (W0, b0, ...: numpy and device), conditions [N, c], z [k_total, N_TOTAL, latent]"""
    from probaforms_amd.models import _gendraw_lib as gl
    d, c, latent, hidden, act = case
    rng = np.random.default_rng([17, MLP_CASES.index(case) if case in MLP_CASES else 99, k_total])
    widths = [latent + c] + list(hidden) + [d]
    parts = []
    for i, o in zip(widths[:-1], widths[1:]):
        parts += [rng.standard_normal(o * i) / np.sqrt(i), 0.1 * rng.standard_normal(o)]
    params = np.concatenate(parts).astype(np.float32)
    Cn = rng.standard_normal((N, c)).astype(np.float32) if c else None
    z = rng.standard_normal((k_total, N_TOTAL, latent)).astype(np.float32)
    return gl.Mlp.make(d, c, latent, hidden, act), params, _dev(params), Cn, z


def _reference(case, params, Cn, z_rows):
    """the same MLP in float64 on the CPU; z_rows [k, n, latent] -> [k, n, d]"""
    d, c, latent, hidden, act = case
    k, n = z_rows.shape[:2]
    x = torch.tensor(z_rows.reshape(k * n, latent), dtype=torch.float64)
    if c:
        x = torch.cat([x, torch.tensor(np.tile(Cn, (k, 1)), dtype=torch.float64)], 1)
    with np.errstate(all="ignore"):
        return Net(latent + c, hidden, d, act)(torch.tensor(params, dtype=torch.float64), x).numpy().reshape(k, n, d)


def _mlp(case, rows=(0, N), ks=None, state=None, want_x=True, want_xt=False, z=None, Cn=None, k_total=K, pattern=None,
         poison=False):
    """one pfg_mlp_draw_accumulate call over rows [lo, hi) of the test's N rows and draws [k_lo, k_hi) of k_total"""
    from probaforms_amd.models import _gendraw_lib as gl
    net, _, params, C0, z0 = _setup(case, k_total)
    Cn = C0 if Cn is None else Cn
    z = z0 if z is None else z
    (lo, hi), (k_lo, k_hi), d = rows, ks or (0, k_total), case[0]
    m, kc = hi - lo, k_hi - k_lo
    x = torch.empty(kc, m, d, device="cuda") if want_x else None
    xt = torch.zeros(m, d, k_total, device="cuda") if want_xt else None
    if poison:
        hygiene.poison_outputs(x, xt)
    nb = gl.workspace_bytes(net, kc)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda") if pattern is None else hygiene.workspace(nb, pattern)
    gl.mlp_draw_accumulate(net, params, None if Cn is None else _dev(Cn[lo:hi]), m, ROW0 + lo, _dev(z[k_lo:k_hi]), N_TOTAL,
                           k_lo, kc, k_total, state, x, xt, ws)
    torch.cuda.synchronize()
    return x, xt


def _finalize(state, n, d, ddof):
    from probaforms_amd.models import _predict_lib as pl
    out = [torch.empty(n, d, device="cuda") for _ in range(4)]
    pl.finalize(state, n, d, ddof, *out)
    return [t.cpu().numpy() for t in out]


def _quantiles(xt, probs=PROBS):
    from probaforms_amd.models import _predict_lib as pl
    n, d, k = xt.shape
    q = torch.empty(len(probs), n, d, device="cuda")
    pl.quantiles(xt, n, d, k, torch.tensor(probs, dtype=torch.float64, device="cuda"), q)
    return q.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _one_call(case):
    """the whole job in one launch: draws, transposed draws and state; shared by the tests below (read only)"""
    from probaforms_amd.models import _predict_lib as pl
    state = pl.new_state(N, case[0], "cuda")
    x, xt = _mlp(case, state=state, want_xt=True)
    return x, xt, state


def _check_stats_of_own_draws(x, xt, state, what):
    """moments and quantiles against numpy float64 over the draws x [k, n, d] the call itself produced"""
    k, n, d = x.shape
    x64 = x.astype(np.float64)
    for ddof in (0, 1):
        mean, std, mn, mx = _finalize(state, n, d, ddof)
        _close(mean, x64.mean(0), (what, "mean"))
        if k > ddof:
            _close(std, x64.std(0, ddof=ddof), (what, "std"))
        np.testing.assert_array_equal(mn, x.min(0))
        np.testing.assert_array_equal(mx, x.max(0))
    if xt is not None:
        _close(_quantiles(xt), np.quantile(x64, PROBS, axis=0), (what, "quantiles"))


@pytest.mark.parametrize("case", MLP_CASES, ids=_ids)
def test_mlp_draws_vs_float64(case):
    from probaforms_amd.models import _gendraw_lib as gl
    net, params, _, Cn, z = _setup(case)
    plan = gl.plan(net, K)
    assert plan.weights_in_lds == (0 if case == WIDE else 1) and plan.waves == 4
    x, xt, state = _one_call(case)
    x = x.cpu().numpy()
    _bar(x, _reference(case, params, Cn, z[:, ROW0:ROW0 + N]))
    np.testing.assert_array_equal(xt.cpu().numpy(), np.transpose(x, (1, 2, 0)))
    _check_stats_of_own_draws(x, xt, state, _ids(case))


@pytest.mark.parametrize("case", [SMALL, (4, 2, 3, (7, 9), "relu"), WIDE], ids=_ids)
def test_every_draw_tile_count_gives_the_same_draws(case):
    """K in {1, 16, 17, 19, 65}: every tile count the plan can pick; a draw's bits do not depend on it"""
    from probaforms_amd.models import _gendraw_lib as gl
    from probaforms_amd.models import _predict_lib as pl
    net, params, _, Cn, z = _setup(case, 65)
    full = None
    tiles = set()
    for k in (65, 1, 16, 17, 19):
        tiles.add(gl.plan(net, k).draw_tiles)
        state = pl.new_state(N, case[0], "cuda")
        x, xt = _mlp(case, ks=(0, k), state=state, want_xt=True, k_total=65)
        if full is None:
            full = x
            _bar(x.cpu().numpy(), _reference(case, params, Cn, z[:, ROW0:ROW0 + N]))
        assert hygiene.same_bits(x, full[:k]), k
        np.testing.assert_array_equal(xt[:, :, :k].cpu().numpy().view(np.uint32),
                                      full[:k].permute(1, 2, 0).cpu().numpy().view(np.uint32))
        _check_stats_of_own_draws(x.cpu().numpy(), None, state, (_ids(case), k))
    assert tiles == ({1} if case == WIDE else {1, 2, 4})


@pytest.mark.parametrize("case", [MLP_CASES[0], SMALL, MLP_CASES[5], WIDE], ids=_ids)
def test_rows_split_over_two_calls_is_bitwise_one_call(case):
    from probaforms_amd.models import _predict_lib as pl
    x1, xt1, st1 = _one_call(case)
    d = case[0]
    for cut in (20, 3):
        state = pl.new_state(N, d, "cuda")
        xa, xta = _mlp(case, rows=(0, cut), state=state[:cut], want_xt=True)
        xb, xtb = _mlp(case, rows=(cut, N), state=state[cut:], want_xt=True)
        assert hygiene.same_bits(torch.cat([xa, xb], 1), x1)
        assert hygiene.same_bits(torch.cat([xta, xtb], 0), xt1)
        assert hygiene.same_bits(state, st1)
    # a rerun, and a call that asks for the state alone
    state = pl.new_state(N, d, "cuda")
    x2, xt2 = _mlp(case, state=state, want_xt=True)
    assert hygiene.same_bits(x2, x1) and hygiene.same_bits(xt2, xt1) and hygiene.same_bits(state, st1)
    state = pl.new_state(N, d, "cuda")
    _mlp(case, state=state, want_x=False)
    assert hygiene.same_bits(state, st1)


@pytest.mark.parametrize("case", [MLP_CASES[0], SMALL, MLP_CASES[3]], ids=_ids)
def test_draws_fed_in_windows(case):
    from probaforms_amd.models import _gendraw_lib as gl
    from probaforms_amd.models import _predict_lib as pl
    x1, xt1, st1 = _one_call(case)
    d = case[0]
    state = pl.new_state(N, d, "cuda")
    xt = torch.zeros(N, d, K, device="cuda")
    xs = []
    net, _, params, Cn, z = _setup(case)
    for k_lo, k_hi in ((0, 7), (7, K)):
        x = torch.empty(k_hi - k_lo, N, d, device="cuda")
        gl.mlp_draw_accumulate(net, params, _dev(Cn), N, ROW0, _dev(z[k_lo:k_hi]), N_TOTAL, k_lo, k_hi - k_lo, K, state, x, xt,
                               torch.empty(gl.workspace_bytes(net, k_hi - k_lo), dtype=torch.uint8, device="cuda"))
        xs.append(x)
    torch.cuda.synchronize()
    assert hygiene.same_bits(torch.cat(xs), x1) and hygiene.same_bits(xt, xt1)
    one, win = _finalize(st1, N, d, 1), _finalize(state, N, d, 1)
    np.testing.assert_array_equal(win[2], one[2])
    np.testing.assert_array_equal(win[3], one[3])
    _close(win[0], one[0].astype(np.float64), "mean, windows against one call")
    _close(win[1], one[1].astype(np.float64), "std, windows against one call")
    _check_stats_of_own_draws(x1.cpu().numpy(), xt, state, "windows")


def test_nan_stays_in_its_row():
    """a NaN in one row's condition and a NaN in one z[k][r] (tanh net): those two rows' series are NaN everywhere, every
    other row carries the bits of the clean run"""
    from probaforms_amd.models import _predict_lib as pl
    case = SMALL
    _, _, _, Cn, z = _setup(case)
    x1, xt1, st1 = _one_call(case)
    Cb, zb = Cn.copy(), z.copy()
    Cb[4, 1] = np.nan
    zb[3, ROW0 + 9, 0] = np.nan
    state = pl.new_state(N, case[0], "cuda")
    x, xt = _mlp(case, state=state, want_xt=True, z=zb, Cn=Cb)
    clean = np.array([r for r in range(N) if r not in (4, 9)])
    got, want = _finalize(state, N, case[0], 1), _finalize(st1, N, case[0], 1)
    q, q1 = _quantiles(xt), _quantiles(xt1)
    for r in (4, 9):
        for a in got:
            assert np.isnan(a[r]).all()
        assert np.isnan(q[:, r]).all()
    xn = x.cpu().numpy()
    assert np.isnan(xn[:, 4]).all() and np.isnan(xn[3, 9]).all() and np.isfinite(np.delete(xn[:, 9], 3, axis=0)).all()
    idx = torch.as_tensor(clean).cuda()
    assert hygiene.same_bits(x[:, idx], x1[:, idx]) and hygiene.same_bits(xt[idx], xt1[idx])
    assert hygiene.same_bits(state[idx], st1[idx])
    for a, b in zip(got + [q.transpose(1, 0, 2)], want + [q1.transpose(1, 0, 2)]):
        np.testing.assert_array_equal(a[clean], b[clean])


@pytest.mark.parametrize("case", [MLP_CASES[0], MLP_CASES[5], WIDE], ids=_ids)
def test_mlp_outputs_do_not_depend_on_the_workspace(case):
    from probaforms_amd.models import _predict_lib as pl
    outs = {}
    for pattern in ("zeros", "ones", "huge"):
        state = pl.new_state(N, case[0], "cuda")
        x, xt = _mlp(case, state=state, want_xt=True, pattern=pattern, poison=True)
        outs[pattern] = dict(x=x, xt=xt, state=state)
        hygiene.assert_all_written(dict(x=x, xt=xt), "pfg_mlp_draw_accumulate / %s" % pattern)
    hygiene.assert_pattern_independent(outs, "pfg_mlp_draw_accumulate")
    assert hygiene.same_bits(outs["huge"]["x"], _one_call(case)[0])


# ---- the affine kernel -------------------------------------------------------------------------------------------

def _affine(d, mu, sigma, W, b, eps, rows=(0, N), ks=None, state=None, want_xt=True, n_total=N_TOTAL, row0=ROW0, xt=None):
    from probaforms_amd.models import _gendraw_lib as gl
    k_total = eps.shape[0]
    (lo, hi), (k_lo, k_hi) = rows, ks or (0, k_total)
    m, kc = hi - lo, k_hi - k_lo
    x = torch.full((kc, m, d), float("nan"), device="cuda")
    if xt is None and want_xt:
        xt = torch.zeros(m, d, k_total, device="cuda")
    gl.affine_draw_accumulate(d, _dev(mu[lo:hi]), _dev(sigma[lo:hi]), _dev(W), _dev(b), _dev(eps[k_lo:k_hi]), m, row0 + lo,
                              n_total, k_lo, kc, k_total, state, x, xt)
    torch.cuda.synchronize()
    return x, xt


@pytest.mark.parametrize("independent", [True, False], ids=["independent", "full"])
@pytest.mark.parametrize("d", [1, 5, 32])
def test_affine_draws_vs_float64(d, independent):
    from probaforms_amd.models import _predict_lib as pl
    c, hidden = 2, (10,)
    model = Normal(d, c, hidden, "tanh", independent)
    rng = np.random.default_rng([29, d, int(independent)])
    params = (rng.standard_normal(model.P) * 0.4).astype(np.float32)
    Cn = rng.standard_normal((N, c)).astype(np.float32)
    eps = rng.standard_normal((K, N_TOTAL, d)).astype(np.float32)
    want = np.stack([model.forward(params, Cn, eps[k, ROW0:ROW0 + N])[0] for k in range(K)])
    _, _, mu, sigma = model.forward(params, Cn)
    mu, sigma = mu.astype(np.float32), sigma.astype(np.float32)
    W = b = None
    if not independent:
        W, b = params[model.P_main:model.P_main + d * d].reshape(d, d), params[model.P_main + d * d:model.P]
    state = pl.new_state(N, d, "cuda")
    x, xt = _affine(d, mu, sigma, W, b, eps, state=state)
    xn = x.cpu().numpy()
    _bar(xn, want)
    np.testing.assert_array_equal(xt.cpu().numpy(), np.transpose(xn, (1, 2, 0)))
    _check_stats_of_own_draws(xn, xt, state, ("affine", d, independent))
    # rows split over two calls, draws in two windows
    st2 = pl.new_state(N, d, "cuda")
    xa, xta = _affine(d, mu, sigma, W, b, eps, rows=(0, 21), state=st2[:21])
    xb, xtb = _affine(d, mu, sigma, W, b, eps, rows=(21, N), state=st2[21:])
    assert hygiene.same_bits(torch.cat([xa, xb], 1), x) and hygiene.same_bits(torch.cat([xta, xtb], 0), xt)
    assert hygiene.same_bits(st2, state)
    st3 = pl.new_state(N, d, "cuda")
    xw = torch.cat([_affine(d, mu, sigma, W, b, eps, ks=ks, state=st3, want_xt=False)[0] for ks in ((0, 7), (7, K))])
    assert hygiene.same_bits(xw, x)
    _check_stats_of_own_draws(xn, None, st3, ("affine windows", d, independent))


def _identity(x, windows):
    """the affine kernel with mu = -0 (x + -0 is x, bit for bit), sigma = 1 and no out: its draws are eps = x [K, n, d]"""
    from probaforms_amd.models import _predict_lib as pl
    k, n, d = x.shape
    mu, sigma = np.full((n, d), -0.0, np.float32), np.ones((n, d), np.float32)
    state = pl.new_state(n, d, "cuda")
    xt = torch.zeros(n, d, k, device="cuda")
    outs = [_affine(d, mu, sigma, None, None, x, rows=(0, n), ks=ks, state=state, n_total=n, row0=0, xt=xt)[0] for ks in windows]
    return torch.cat(outs).cpu().numpy(), xt, state


@pytest.mark.parametrize("k", [19, 40, 65])
def test_affine_identity_nonfinite_series(k):
    x = E.nonfinite(k)
    for windows in E.windows_of(k):
        got, _, state = _identity(x, windows)
        np.testing.assert_array_equal(got, x)                       # NaN == NaN here
        for ddof in (0, 1):
            E.check_moments(_finalize(state, x.shape[1], x.shape[2], ddof), x, ddof, ("nonfinite", k, windows))


@pytest.mark.parametrize("k", E.CONDITIONED_K)
def test_affine_identity_conditioned_series(k):
    x = E.conditioned(k)
    for windows in E.windows_of(k):
        got, _, state = _identity(x, windows)
        np.testing.assert_array_equal(got, x)
        E.check_moments(_finalize(state, x.shape[1], x.shape[2], 0), x, 0, ("conditioned", k, windows))


@pytest.mark.parametrize("k", E.QUANTILE_K)
def test_affine_identity_quantile_series(k):
    series, probs = E.quantile_series(k)                            # [3, 2, k]
    x = np.ascontiguousarray(np.transpose(series, (2, 0, 1)))
    _, xt, _ = _identity(x, [(0, k)])
    np.testing.assert_array_equal(xt.cpu().numpy().view(np.uint32), series.view(np.uint32))
    E.same(_quantiles(xt, tuple(probs)), E.quantile_reference(series, probs), ("quantiles", k))


# ---- the public calls --------------------------------------------------------------------------------------------

KINDS = ("cvae", "wgan", "cnormal", "cnormal_independent")


@functools.lru_cache(maxsize=None)
def _fitted(kind, conditional):
    from probaforms_amd.models import CVAE, ConditionalNormal, ConditionalWGAN
    rng = np.random.default_rng([41, KINDS.index(kind), int(conditional)])
    X = rng.standard_normal((64, 3)).astype(np.float32)
    C = rng.standard_normal((64, 2)).astype(np.float32) if conditional else None
    torch.manual_seed(3)
    m = {"cvae": lambda: CVAE(n_epochs=1), "wgan": lambda: ConditionalWGAN(n_epochs=1),
         "cnormal": lambda: ConditionalNormal(n_epochs=1),
         "cnormal_independent": lambda: ConditionalNormal(use_independent_covariance=True, n_epochs=1)}[kind]()
    m.fit(X, C)
    return m


def _conditions(what):
    if what == "int":
        return 37
    return np.random.default_rng(43).standard_normal((int(what), 2)).astype(np.float32)


@pytest.mark.parametrize("what", ["37", "32", "int"])
@pytest.mark.parametrize("kind", KINDS)
def test_public_calls_are_the_seeded_loop(kind, what):
    from probaforms_amd.models._predict import SampleStats
    m = _fitted(kind, what != "int")
    C = _conditions(what)
    n = 37 if what == "int" else len(C)
    torch.manual_seed(5)
    loop = np.array([m.sample(C) for _ in range(K)])
    end = torch.get_rng_state()
    torch.manual_seed(5)
    many = m.sample_many(C, K)
    assert torch.equal(torch.get_rng_state(), end)
    assert many.shape == (K, n, 3) and many.dtype == np.float32
    _bar(many, loop.astype(np.float64))
    torch.manual_seed(5)
    s = m.sample_stats(C, K, quantiles=(0.05, 0.5, 0.95), ddof=1)
    assert torch.equal(torch.get_rng_state(), end)
    assert isinstance(s, SampleStats)
    for a in s[:4]:
        assert a.shape == (n, 3) and a.dtype == np.float32
    assert s.quantiles.shape == (3, n, 3) and s.quantiles.dtype == np.float32
    x64 = many.astype(np.float64)
    _close(s.mean, x64.mean(0), "mean")
    _close(s.std, x64.std(0, ddof=1), "std")
    np.testing.assert_array_equal(s.min, many.min(0))
    np.testing.assert_array_equal(s.max, many.max(0))
    _close(s.quantiles, np.quantile(x64, (0.05, 0.5, 0.95), axis=0), "quantiles")
    torch.manual_seed(5)
    s0 = m.sample_stats(C, K)
    assert s0.quantiles is None and torch.equal(torch.get_rng_state(), end)
    np.testing.assert_array_equal(s0.mean, s.mean)
    _close(s0.std, x64.std(0), "std, ddof 0")


@pytest.mark.parametrize("kind", KINDS)
def test_empty_conditions(kind):
    m = _fitted(kind, True)
    before = torch.get_rng_state()
    C = np.zeros((0, 2), np.float32)
    assert m.sample_many(C, 5).shape == (5, 0, 3)
    s = m.sample_stats(C, 5, quantiles=(0.5,))
    assert s.mean.shape == (0, 3) and s.quantiles.shape == (1, 0, 3) and s.mean.dtype == np.float32
    assert torch.equal(torch.get_rng_state(), before)


@pytest.mark.parametrize("what", ["37", "32"])
@pytest.mark.parametrize("kind", KINDS)
def test_small_windows_and_row_chunks_give_the_one_chunk_result(kind, what, monkeypatch):
    from probaforms_amd.models import _predict
    m = _fitted(kind, True)
    C = _conditions(what)
    n = len(C)
    width = m.latent_dim if kind in ("cvae", "wgan") else 3
    torch.manual_seed(7)
    many = m.sample_many(C, K)
    torch.manual_seed(7)
    s = m.sample_stats(C, K, quantiles=PROBS, ddof=1)
    end = torch.get_rng_state()
    monkeypatch.setattr(_predict, "Z_WINDOW_BYTES", 4 * n * width * 7)           # windows of 7 draws
    monkeypatch.setattr(_predict, "XT_CHUNK_BYTES", 4 * 3 * K * 10)              # chunks of 10 rows
    assert len(_predict.draw_windows(K, n, width, _predict.Z_WINDOW_BYTES)) == 3
    assert len(_predict.quantile_row_chunks(n, 3, K, _predict.XT_CHUNK_BYTES)) == 4
    torch.manual_seed(7)
    np.testing.assert_array_equal(m.sample_many(C, K).view(np.uint32), many.view(np.uint32))
    assert torch.equal(torch.get_rng_state(), end)
    torch.manual_seed(7)
    t = m.sample_stats(C, K, quantiles=PROBS, ddof=1)
    assert torch.equal(torch.get_rng_state(), end)
    np.testing.assert_array_equal(t.min, s.min)
    np.testing.assert_array_equal(t.max, s.max)
    np.testing.assert_array_equal(t.quantiles, s.quantiles)
    x64 = many.astype(np.float64)
    _close(t.mean, x64.mean(0), "mean")
    _close(t.std, x64.std(0, ddof=1), "std")
    _close(t.mean, s.mean.astype(np.float64), "mean against one chunk")
    _close(t.std, s.std.astype(np.float64), "std against one chunk")
