"""Workspace hygiene (tests/hygiene.py, tests/test_workspace_hygiene_gpu.py) of the other three libraries: the CVAE calls of
librnvp_hip.so, libpf_metrics.so and libpf_wgan.so.  Every call runs once per workspace pattern on poisoned outputs through the raw
bindings (one level below the wrappers that allocate their own workspace); all outputs must carry the bits of the `zeros` run, and
the `zeros` run must meet the reference of the entry point's existing test at that test's bar (named at each check).
"""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import hygiene  # noqa: E402
import metrics1d_numpy as m1  # noqa: E402
import metrics_numpy as mn  # noqa: E402
import native_libs  # noqa: E402
import wgan_torch as wt  # noqa: E402
from probaforms_amd.metrics import _boot, _lib, _m1d  # noqa: E402
from probaforms_amd.models import _wgan_lib as W  # noqa: E402

pytestmark = pytest.mark.gpu

native_libs.ensure_built(_lib, W)


def _dev(a, dtype=torch.float32):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a)).to(dtype).cuda().contiguous()


def _nan(*shape):
    return torch.full(shape, float("nan"), device="cuda")


def _patterns(nbytes, prime_bytes, prime, call):
    """call(ws) -> {name: tensor} once per pattern; `replay`: prime(ws) (a larger call of the same entry point) runs first on a buffer
    of prime_bytes"""
    outs = {}
    for pat in hygiene.PATTERNS:
        ws = hygiene.workspace(prime_bytes if pat == "replay" else nbytes, pat)
        if pat == "replay":
            prime(ws)
        outs[pat] = call(ws)
        torch.cuda.synchronize()
    return outs


def _settle(outs, what):
    hygiene.assert_all_written(outs["zeros"], what)
    hygiene.assert_pattern_independent(outs, what)
    return outs["zeros"]


# ---- CVAE ------------------------------------------------------------------------------------------------------------------------------
# id: (d, c, latent, hidden, activation, family, bar): the bars of test_cvae_gpu.py::test_mfma_step_shapes_vs_oracle (3e-6),
# ::test_lmm_step_shapes_vs_oracle (5e-6) and ::test_loss_grad_and_adam's oracle check, which the generic family runs under (5e-6)
CVAE_FORMS = {
    "mfma":    (16, 4, 2, (32,), "tanh", "auto", 3e-6),
    "lmm":     (4, 2, 3, (7, 9), "relu", "lmm", 5e-6),
    "generic": (4, 2, 3, (7, 9), "relu", "generic", 5e-6),
}
CVAE_PATH = {"mfma": "PATH_MFMA", "lmm": "PATH_LMM", "generic": "PATH_GENERIC"}


@pytest.mark.parametrize("n", [1, 63, 5000, 70001])          # (lmm: 70 001 rows are two row chunks of 65 536)
@pytest.mark.parametrize("form", list(CVAE_FORMS))
def test_cvae_calls_do_not_depend_on_the_workspace(form, n):
    from oracle import CvaeOracle, CvaeShape
    from probaforms_amd import _hip
    d, c, lat, hidden, act, family, bar = CVAE_FORMS[form]
    shape = _hip.CvaeShape.make(d, c, lat, hidden, act, family=family)
    assert _hip.cvae_kernel_path(shape) == getattr(_hip, CVAE_PATH[form])
    o64, so = CvaeOracle(64), CvaeShape.make(d, c, lat, hidden, act)
    P = _hip.cvae_param_count(shape)
    rng = np.random.default_rng(d * 1000 + n)
    N = 2 * n + 777                                              # the priming call's rows
    p = (rng.standard_normal(P) * 0.25).astype(np.float32)
    X = rng.standard_normal((N, d)).astype(np.float32); C = rng.standard_normal((N, c)).astype(np.float32)
    eps = rng.standard_normal((N, lat)).astype(np.float32)
    perm = rng.permutation(N).astype(np.int64)
    pd, xd, cd, ed, idx = _dev(p), _dev(X), _dev(C), _dev(eps), _dev(perm, torch.int64)
    Xg, Cg = X[perm[:n]], C[perm[:n]]
    nb, pb = _hip.cvae_workspace_bytes(shape, n), _hip.cvae_workspace_bytes(shape, N)
    klw, tag = 0.3, "[%s, %d rows]" % (form, n)

    def run(fn):
        return _settle(_patterns(nb, pb, lambda ws: fn(N, ws), lambda ws: fn(n, ws)), fn.__name__ + tag)

    def cvae_encode(rows, ws):
        mu, ls = _nan(rows, lat), _nan(rows, lat)
        _hip.cvae_encode(shape, pd, xd, cd, rows, mu, ls, ws)
        return dict(mu=mu, log_sigma=ls)

    def cvae_decode(rows, ws):
        x = _nan(rows, d)
        _hip.cvae_decode(shape, pd, ed, cd, rows, x, ws)
        return dict(x=x)

    sub = np.arange(n) if n <= 600 else np.concatenate([np.arange(300), np.arange(n - 300, n)])
    o = run(cvae_encode)
    mu_o, ls_o = o64.encode(so, p, X[:n][sub], C[:n][sub])
    x_o = o64.decode(so, p, eps[:n][sub], C[:n][sub])
    xr = run(cvae_decode)["x"]
    for got, want in ((o["mu"], mu_o), (o["log_sigma"], ls_o), (xr, x_o)):
        assert np.abs(got.cpu().numpy()[sub] - want).max() < bar * max(1.0, np.abs(want).max())

    def cvae_loss_grad(rows, ws):
        g, loss = _nan(P), _nan(1)
        _hip.cvae_loss_grad(shape, pd, xd, cd, idx, ed, rows, 1.0 / rows, klw, g, loss, ws)
        return dict(grad=g, loss=loss)

    def cvae_loss_only(rows, ws):                                # grad_out NULL: the per-epoch evaluation
        loss = _nan(1)
        _hip.cvae_loss_grad(shape, pd, xd, cd, idx, ed, rows, 1.0 / rows, klw, None, loss, ws)
        return dict(loss=loss)

    o = run(cvae_loss_grad)
    lo, go = o64.loss_grad(so, p, Xg, Cg, eps[:n], klw)
    assert abs(float(o["loss"]) - lo) < bar * max(1.0, abs(lo))
    assert np.abs(o["grad"].cpu().numpy() - go).max() < bar * np.abs(go).max()
    assert float(run(cvae_loss_only)["loss"]) == float(o["loss"])       # (as both tests require)

    lr, wd, step = 0.01, 0.1, 2
    m0 = (rng.standard_normal(P) * 1e-2).astype(np.float32); v0 = ((rng.standard_normal(P) * 1e-2) ** 2).astype(np.float32)

    def cvae_train_step(rows, ws):
        pp, m, v, g, loss = pd.clone(), _dev(m0), _dev(v0), _nan(P), _nan(1)
        _hip.cvae_train_step(shape, pp, xd, cd, idx, ed, rows, 1.0 / rows, klw, g, loss, m, v, lr, 0.9, 0.999, 1e-8, wd, step, ws)
        return dict(params=pp, exp_avg=m, exp_avg_sq=v, grad=g, loss=loss)

    t = run(cvae_train_step)
    # test_loss_grad_and_adam: the fused step is cvae_loss_grad + rnvp_adam_step bit for bit
    pp, m, v = pd.clone(), _dev(m0), _dev(v0)
    _hip.adam_step(pp, o["grad"], m, v, P, lr, 0.9, 0.999, 1e-8, wd, step)
    assert torch.equal(t["params"], pp) and torch.equal(t["exp_avg"], m) and torch.equal(t["exp_avg_sq"], v)
    assert hygiene.same_bits(t["grad"], o["grad"]) and float(t["loss"]) == float(o["loss"])


@pytest.mark.parametrize("form,n,bs", [("mfma", 2 * 9000 + 1, 9000), ("lmm", 2 * 300 + 77, 300), ("generic", 2 * 300 + 1, 300),
                                       ("resident", 97, 32), ("resident", 65, 32)])
def test_cvae_fit_epoch_does_not_depend_on_the_workspace(form, n, bs):
    from probaforms_amd import _hip
    d, c, lat, hidden, act, family, _ = CVAE_FORMS["mfma" if form == "resident" else form]
    if form == "resident":
        d, c, lat, hidden = 5, 3, 2, (10,)
    shape = _hip.CvaeShape.make(d, c, lat, hidden, act, family=family)
    assert _hip.cvae_fit_epoch_resident(shape, bs) == (form == "resident")
    P = _hip.cvae_param_count(shape)
    rng = np.random.default_rng(n + bs)
    p = (rng.standard_normal(P) * 0.25).astype(np.float32)
    X = rng.standard_normal((2 * n, d)).astype(np.float32); C = rng.standard_normal((2 * n, c)).astype(np.float32)
    eps = rng.standard_normal((2 * n, lat)).astype(np.float32)
    xd, cd, ed = _dev(X), _dev(C), _dev(eps)
    lr, wd, klw = 0.01, 0.05, 0.3

    def fit(n_, bs_, ws):
        perm = _dev(np.random.default_rng(n_).permutation(n_).astype(np.int64), torch.int64)
        pp, m, v = _dev(p), torch.zeros(P, device="cuda"), torch.zeros(P, device="cuda")
        g, hist = _nan(P), _nan((n_ + bs_ - 1) // bs_)
        _hip.cvae_fit_epoch(shape, pp, xd, cd, perm, ed, n_, bs_, klw, g, hist, m, v, lr, 0.9, 0.999, 1e-8, wd, 1, ws)
        return dict(params=pp, exp_avg=m, exp_avg_sq=v, loss_hist=hist), perm

    o = _settle(_patterns(_hip.cvae_workspace_bytes(shape, bs), _hip.cvae_workspace_bytes(shape, 2 * bs),
                          lambda ws: fit(2 * n, 2 * bs, ws), lambda ws: fit(n, bs, ws)[0]), "cvae_fit_epoch[%s]" % form)
    # the epoch as the step loop: cvae_train_step per batch (anchored to the oracle above), the same bits for every family but the
    # resident one, which keeps its own arithmetic: there the bars of test_hip_kernels.py::test_adam_trajectory_vs_reference
    perm = fit(n, bs, hygiene.workspace(_hip.cvae_workspace_bytes(shape, bs), "zeros"))[1]
    pp, m, v = _dev(p), torch.zeros(P, device="cuda"), torch.zeros(P, device="cuda")
    g, hist = _nan(P), _nan((n + bs - 1) // bs)
    ws = hygiene.workspace(_hip.cvae_workspace_bytes(shape, bs), "zeros")
    for k, s in enumerate(range(0, n, bs)):
        e = min(n, s + bs)
        _hip.cvae_train_step(shape, pp, xd, cd, perm[s:e].contiguous(), ed[s:e].contiguous(), e - s, 1.0 / (e - s), klw, g, hist[k:k + 1],
                             m, v, lr, 0.9, 0.999, 1e-8, wd, k + 1, ws)
    if form == "resident":
        np.testing.assert_allclose(o["exp_avg"].cpu().numpy(), m.cpu().numpy(), rtol=2e-5, atol=3e-6 * float(m.abs().max()))
        np.testing.assert_allclose(o["exp_avg_sq"].cpu().numpy(), v.cpu().numpy(), rtol=4e-5, atol=6e-6 * float(v.abs().max()))
        assert float((o["params"] - pp).abs().mean()) < 2e-6
        np.testing.assert_allclose(o["loss_hist"].cpu().numpy(), hist.cpu().numpy(), rtol=5e-5, atol=5e-5)
    else:
        for name, want in (("params", pp), ("exp_avg", m), ("exp_avg_sq", v), ("loss_hist", hist)):
            assert torch.equal(o[name], want), name


# ---- metrics ----------------------------------------------------------------------------------------------------------------------------
METRIC_SIZES = [(50, 51, 3, 5), (1, 2, 2, 4), (1000, 1500, 4, 3)]           # (rows real, rows fake, features, replicates)


def _boot_case(nr, nf, d, reps, seed):
    """data and the reference's bootstrap draws (numpy's global generator) for `reps` replicates, on the host and on the device"""
    rng = np.random.default_rng(seed)
    X = np.round(rng.normal(size=(nr, d)), 2); Y = np.round(rng.normal(0.3, 1.2, size=(nf, d)), 2)
    np.random.seed(seed)
    host = np.empty(reps * (nr + nf), np.int32)
    _boot.draw_indices(host, reps, nr, nf)
    ix, iy = host[:reps * nr].reshape(reps, nr), host[reps * nr:].reshape(reps, nf)
    return X, Y, ix, iy, _dev(ix.reshape(-1), torch.int32), _dev(iy.reshape(-1), torch.int32)


def _primer(nr, nf, d, reps, seed):
    """the `replay` primer: more replicates and more rows"""
    return (nr + 20, nf + 30, d, reps + 2) + _boot_case(nr + 20, nf + 30, d, reps + 2, seed + 1)


@pytest.mark.parametrize("nr,nf,d,reps", METRIC_SIZES)
def test_mmd_and_moments_do_not_depend_on_the_workspace(nr, nf, d, reps):
    X, Y, ix, iy, ixd, iyd = _boot_case(nr, nf, d, reps, 3)
    pr = _primer(nr, nf, d, reps, 3)

    def mmd(A, B, ia, ib, r, ws):
        med, out = torch.full((r,), float("nan"), dtype=torch.float64, device="cuda"), torch.full((r,), float("nan"), dtype=torch.float64, device="cuda")
        _lib.mmd(_dev(A, torch.float64), _dev(B, torch.float64), ia, ib, r, med, out, ws)
        return dict(median=med, mmd=out)

    outs = _patterns(_lib.mmd_workspace_bytes(nr, nf, d, reps), _lib.mmd_workspace_bytes(*pr[:4]),
                     lambda ws: mmd(pr[4], pr[5], pr[8], pr[9], pr[3], ws), lambda ws: mmd(X, Y, ixd, iyd, reps, ws))
    hygiene.assert_pattern_independent(outs, "pfm_mmd")
    med, val = outs["zeros"]["median"].cpu().numpy(), outs["zeros"]["mmd"].cpu().numpy()
    # bars of test_metrics_gpu.py::test_mmd_replicates_match_the_reference (a median of 0 gives a NaN replicate, as there)
    want = [mn.mmd_replicate(X[ix[r]], Y[iy[r]]) for r in range(reps)]
    wmed = np.array([w[0] for w in want]); wval = np.array([w[1] for w in want])
    np.testing.assert_allclose(med, wmed, rtol=1e-12, atol=0)
    ok = wmed > 0
    assert (np.abs(val[ok] - wval[ok]) <= 1e-11 + 1e-9 * np.abs(wval[ok])).all() and np.isnan(val[~ok]).all()

    def moments(A, B, ia, ib, r, ws):
        dd = A.shape[1]
        mean = torch.full((r, 2, dd), float("nan"), dtype=torch.float64, device="cuda")
        cov = torch.full((r, 2, dd, dd), float("nan"), dtype=torch.float64, device="cuda")
        _lib.boot_moments(_dev(A, torch.float64), _dev(B, torch.float64), ia, ib, r, mean, cov, ws)
        return dict(mean=mean, cov=cov)

    outs = _patterns(_lib.moments_workspace_bytes(nr, nf, d, reps), _lib.moments_workspace_bytes(*pr[:4]),
                     lambda ws: moments(pr[4], pr[5], pr[8], pr[9], pr[3], ws), lambda ws: moments(X, Y, ixd, iyd, reps, ws))
    hygiene.assert_pattern_independent(outs, "pfm_boot_moments")
    mean, cov = outs["zeros"]["mean"].cpu().numpy(), outs["zeros"]["cov"].cpu().numpy()
    for r in range(reps):           # np.cov (ddof 1: NaN for a one-row set, as numpy gives); the bar of test_fd_matches_the_reference
        for s, Z in enumerate((X[ix[r]], Y[iy[r]])):
            np.testing.assert_allclose(mean[r, s], Z.mean(0), rtol=1e-9, atol=1e-13)
            if len(Z) > 1:
                np.testing.assert_allclose(cov[r, s], np.cov(Z, rowvar=False).reshape(d, d), rtol=1e-9, atol=1e-13)


# metric id, bins (histograms in LDS: 10; in global memory: 3000), the restated statistic and how the existing tests compare it
M1D = {
    "ks":        (_lib.M1D_KS, 1, "kolmogorov_smirnov_1d"),
    "cvm":       (_lib.M1D_CVM, 1, "cramer_von_mises_1d"),
    "ad":        (_lib.M1D_AD, 1, "anderson_darling_1d"),
    "auc":       (_lib.M1D_AUC, 1, "roc_auc_score_1d"),
    "hist_lds":  (_lib.M1D_HIST, 10, "kullback_leibler_1d"),
    "hist_glob": (_lib.M1D_HIST, 3000, "jensen_shannon_1d"),
    "kde":       (_lib.M1D_KDE, 101, "kullback_leibler_1d_kde"),
}
BITWISE = ("kolmogorov_smirnov_1d", "cramer_von_mises_1d", "kullback_leibler_1d", "jensen_shannon_1d")    # test_metrics1d_gpu.py
RTOL = {"roc_auc_score_1d": 1e-12, "anderson_darling_1d": 1e-12, "kullback_leibler_1d_kde": 1e-9}


@pytest.mark.parametrize("nr,nf,d,reps", METRIC_SIZES)
@pytest.mark.parametrize("which", list(M1D))
def test_metric1d_does_not_depend_on_the_workspace(which, nr, nf, d, reps):
    metric, bins, name = M1D[which]
    X, Y, ix, iy, ixd, iyd = _boot_case(nr, nf, d, reps, 11)
    pr = _primer(nr, nf, d, reps, 11)

    def run(A, B, ia, ib, r, ws):
        p = _m1d.Pooled(_dev(A, torch.float64), _dev(B, torch.float64))
        tail, dtype = _m1d.OUT_SHAPE[metric]
        out = torch.empty((r, p.d) + tuple(bins if t is None else t for t in tail), dtype=dtype, device="cuda")
        hygiene.poison_outputs(out)
        h = (_m1d.silverman(p.nr), _m1d.silverman(p.nf)) if metric == _lib.M1D_KDE else (1.0, 1.0)
        _lib.metric1d(metric, p.cols, p.perm, p.gstart, p.ngroups, p.nr, p.nf, ia, ib, r, bins, h[0], h[1], out, ws)
        return dict(out=out)

    outs = _patterns(_lib.metric1d_workspace_bytes(metric, nr, nf, d, reps, bins), _lib.metric1d_workspace_bytes(metric, *pr[:4], bins),
                     lambda ws: run(pr[4], pr[5], pr[8], pr[9], pr[3], ws), lambda ws: run(X, Y, ixd, iyd, reps, ws))
    hygiene.assert_pattern_independent(outs, "pfm_metric1d[%s]" % which)
    raw = outs["zeros"]["out"].cpu().numpy()
    if metric in (_lib.M1D_CVM, _lib.M1D_AD) and min(nr, nf) < 2:
        return          # scipy gives NaN / raises for a one-row sample (ks1d.py handles it above the kernel): no statistic to compare
    with np.errstate(all="ignore"):
        if metric == _lib.M1D_KS:
            S = _m1d.ks_statistic(raw, nr, nf)
        elif metric == _lib.M1D_CVM:
            S = _m1d.cvm_statistic(raw, nr, nf)
        elif metric == _lib.M1D_AD:
            S = _m1d.ad_statistic(raw, nr, nf)
        elif metric == _lib.M1D_AUC:
            S = _m1d.auc_statistic(raw, nr, nf)
        else:
            P = _m1d.hist_probs(raw) if metric == _lib.M1D_HIST else _m1d.kde_probs(raw, nr, nf)
            S = _m1d.divergence(P[:, :, 0], P[:, :, 1], bins, name.startswith("jensen"))
        want = np.empty((reps, d))
        for r in range(reps):
            for f in range(d):
                want[r, f] = m1.FUNCS[name](X[ix[r], f], Y[iy[r], f], bins)
    # test_metrics1d_gpu.py::assert_close: bitwise for ks / cvm / the histogram divergences, 1e-12 for auc / ad, 1e-9 for the KDE
    S = np.asarray(S, np.float64)
    assert np.array_equal(np.isnan(S), np.isnan(want))
    ok = ~np.isnan(want)
    if name in BITWISE:
        assert np.array_equal(S[ok], want[ok]), np.abs(S[ok] - want[ok]).max()
    else:
        np.testing.assert_allclose(S[ok], want[ok], rtol=RTOL[name], atol=0)


# ---- ConditionalWGAN -------------------------------------------------------------------------------------------------------------------
# the three SHAPES of test_wgan_gpu.py: (d, c, latent, g_hidden, d_hidden, g_act, d_act)
WGAN_SHAPES = {
    "deep_relu": (6, 2, 2, (24, 40, 17), (33, 20, 28, 9), 'relu', 'relu'),
    "nocond_tanh": (4, 0, 3, (30, 30), (25,), 'tanh', 'tanh'),
    "big_batch": (7, 3, 2, (64, 48), (40, 40), 'relu', 'tanh'),
}
GRAD_TOL = 2e-5           # test_wgan_gpu.py


@pytest.mark.parametrize("B", [1, 50, 4096])
@pytest.mark.parametrize("name", sorted(WGAN_SHAPES))
def test_wgan_calls_do_not_depend_on_the_workspace(name, B):
    from probaforms_amd.models.wgan import ConditionalWGAN, step_kinds
    d, c, lat, gh, dh, ga, da = WGAN_SHAPES[name]
    n = 2 * B + 777
    rng = np.random.default_rng(len(name) + B)
    X = rng.normal(size=(n, d)).astype(np.float32); C = rng.normal(size=(n, c)).astype(np.float32) if c else None
    torch.manual_seed(1)
    m = ConditionalWGAN(latent_dim=lat, generator_hidden=gh, discriminator_hidden=dh, generator_activation=ga,
                        discriminator_activation=da, batch_size=B, lr=1e-3, weight_decay=0.001)
    m._model_init(X, C)
    core = m._core
    PG, PD = core.PG, core.PD
    wg = wt.Wgan(d, c, lat, gh, dh, ga, da)
    opt = m.opt_gen.hyper(0.01)
    Xd, Cd = _dev(X), _dev(C)
    Z = rng.normal(size=(n, lat)).astype(np.float32); zd = _dev(Z)
    perm = rng.permutation(n).astype(np.int64); idx = _dev(perm, torch.int64)
    p0 = core.flat.clone(); v0 = (torch.rand_like(core.square_avg) * 1e-4)
    p0n, v0n = p0[:PG + PD].cpu().numpy(), v0[:PG + PD].cpu().numpy()

    for kind in (0, 1):
        Pk = PD if kind else PG
        sl = slice(PG, PG + PD) if kind else slice(0, PG)

        def train_step(rows, ws):
            p, v, g, loss = p0.clone(), v0.clone(), _nan(Pk), _nan(1)
            W.train_step(core.shape, kind, p, v, Xd, Cd, idx[:rows].contiguous(), zd[:rows].contiguous(), rows, opt, g, loss, ws)
            return dict(params=p, square_avg=v, grad=g, loss=loss)

        o = _settle(_patterns(W.workspace_bytes(core.shape, B), W.workspace_bytes(core.shape, n), lambda ws: train_step(n, ws),
                              lambda ws: train_step(B, ws)), "pfw_train_step[%s, kind %d, batch %d]" % (name, kind, B))
        # bars of test_wgan_gpu.py::test_gradients_and_epoch_losses_match_float64 and ::test_rmsprop_and_clamp_to_the_ulp
        l64, g64 = wg.loss_grad(p0n, X, C, perm[:B], Z[:B], kind)
        scale = max(np.abs(g64).max(), wg.grad_scale(p0n, X, C, perm[:B], Z[:B], kind))
        g = o["grad"].cpu().numpy()
        assert np.abs(g - g64).max() <= GRAD_TOL * scale
        assert abs(float(o["loss"]) - l64) <= 1e-5 * max(1.0, abs(l64)) + 1e-6
        pr, vr = wt.rmsprop_f32(p0n[sl], g, v0n[sl], 1e-3, wd=0.001, clamp=0.01 if kind else 0.0)
        p1, v1 = o["params"][:PG + PD].cpu().numpy(), o["square_avg"][:PG + PD].cpu().numpy()
        assert (np.abs(p1[sl] - pr) <= np.spacing(np.abs(pr))).all() and (np.abs(v1[sl] - vr) <= np.spacing(np.abs(vr))).all()

    def epoch_losses(rows, ws):
        out = _nan(2)
        W.epoch_losses(core.shape, p0, Xd, Cd, zd, rows, out, ws)
        return dict(epoch_losses=out)

    o = _settle(_patterns(W.workspace_bytes(core.shape, 0, B), W.workspace_bytes(core.shape, 0, n), lambda ws: epoch_losses(n, ws),
                          lambda ws: epoch_losses(B, ws)), "pfw_epoch_losses[%s, %d rows]" % (name, B))
    gen, disc = wg.epoch_losses(p0n, X[:B], None if C is None else C[:B], Z[:B])
    e = o["epoch_losses"].cpu().numpy()
    assert abs(e[0] - gen) <= 1e-5 * max(1.0, abs(gen)) and abs(e[1] - disc) <= 1e-5 * max(1.0, abs(disc))     # the same test

    ne = 2 * B + 1                               # two full batches and a one-row batch
    kinds = step_kinds(1, 3, 2)

    def fit_epoch(rows, bs, ws):
        p, v, out = p0.clone(), v0.clone(), _nan(2)
        W.fit_epoch(core.shape, p, v, Xd, Cd, idx[:rows].contiguous(), zd[:rows].contiguous(), zd[:rows].contiguous(), rows, bs,
                    step_kinds(1, -(-rows // bs), 2), opt, out, ws)
        return dict(params=p, square_avg=v, epoch_losses=out)

    o = _settle(_patterns(W.workspace_bytes(core.shape, B, ne), W.workspace_bytes(core.shape, B + 300, n), lambda ws: fit_epoch(n, B + 300, ws),
                          lambda ws: fit_epoch(ne, B, ws)), "pfw_fit_epoch[%s, batch %d]" % (name, B))
    # test_wgan_gpu.py::test_fit_epoch_equals_the_step_loop_bitwise: the steps (anchored above) one by one, then pfw_epoch_losses
    p, v, e2 = p0.clone(), v0.clone(), _nan(2)
    ws = hygiene.workspace(W.workspace_bytes(core.shape, B, ne), "zeros")
    for b, s in enumerate(range(0, ne, B)):
        e_ = min(ne, s + B)
        W.train_step(core.shape, int(kinds[b]), p, v, Xd, Cd, idx[s:e_].contiguous(), zd[s:e_].contiguous(), e_ - s, opt, None, None, ws)
    W.epoch_losses(core.shape, p, Xd, Cd, zd[:ne].contiguous(), ne, e2, ws)
    assert torch.equal(o["params"], p) and torch.equal(o["square_avg"], v) and torch.equal(o["epoch_losses"], e2)
