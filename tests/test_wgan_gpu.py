"""ConditionalWGAN on the GPU: the HIP kernels of libpf_wgan.so against the reference's committed fixtures
(tests/golden/wgan_*.npz, tests/golden/make_golden_wgan.py) and a float64 torch restatement (tests/wgan_torch.py) on
shapes the fixtures do not cover; RMSprop and the clamp to the ulp, pfw_fit_epoch against the step loop bit for bit,
the seeded public fit + sample, determinism, tensor inputs and API errors."""
import glob
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import native_libs  # noqa: E402
import wgan_torch as wt  # noqa: E402
from probaforms_amd.models import _wgan_lib as W  # noqa: E402
from probaforms_amd.models.wgan import ConditionalWGAN, step_kinds  # noqa: E402

pytestmark = pytest.mark.gpu

native_libs.ensure_built(W)

FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "wgan_*.npz")))
DEV = torch.device("cuda")
GRAD_TOL = 2e-5           # |g - g_ref| / max |g_ref|: float32 sums in another order


def fid(p):
    return os.path.basename(p)[5:-4]


def load(path):
    f = np.load(path)
    kw = {k[3:]: f[k] for k in f.files if k.startswith("kw_")}
    kw = {k: (tuple(int(x) for x in v) if v.ndim else (str(v) if v.dtype.kind == 'U' else v.item())) for k, v in kw.items()}
    C = f["C"] if f["C"].shape[1] else None
    return f, kw, f["X"], C


def model_of(kw, X, C, params=None):
    """a ConditionalWGAN with its networks built (as fit builds them) and, optionally, the given flat parameters"""
    m = ConditionalWGAN(**kw)
    m._model_init(X, C)
    core = m._core
    if params is not None:
        core.flat[:core.PG + core.PD].copy_(torch.as_tensor(params))
    return m, core


def restatement(m, core):
    return wt.Wgan(core.d, core.c, core.latent, m.generator_hidden, m.discriminator_hidden, m.generator_activation,
                   m.discriminator_activation)


def dev(a, dtype=torch.float32):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def run_steps(m, core, X, C, steps, check=None):
    """pfw_train_step over [(kind, rows, z)]; check(k, kind, p_before, v_before, g, p_after, v_after) per step"""
    Xd, Cd = dev(X), dev(C)
    opt = m.opt_gen.hyper(0.01)
    P = core.PG + core.PD
    for k, (kind, rows, z) in enumerate(steps):
        B = len(rows)
        g = torch.zeros(core.PD if kind else core.PG, device=DEV)
        loss = torch.zeros(1, device=DEV)
        p0, v0 = core.flat[:P].cpu().numpy(), core.square_avg[:P].cpu().numpy()
        W.train_step(core.shape, kind, core.flat, core.square_avg, Xd, Cd, dev(rows, torch.int64), dev(z), B, opt, g, loss,
                     core.workspace(B))
        torch.cuda.synchronize()
        if check is not None:
            check(k, kind, p0, v0, g.cpu().numpy(), core.flat[:P].cpu().numpy(), core.square_avg[:P].cpu().numpy(),
                  float(loss))


def fixture_steps(f):
    off = np.concatenate([[0], np.cumsum(f["batch_sizes"])])
    return [(int(f["kinds"][k]), f["rows"][off[k]:off[k + 1]], f["z"][off[k]:off[k + 1]]) for k in range(int(f["K"]))]


@pytest.mark.parametrize("path", FIXTURES, ids=fid)
def test_step_gradients_and_trajectory_match_the_reference(path):
    f, kw, X, C = load(path)
    m, core = model_of(kw, X, C, f["p0"])
    assert core.PG == int(f["PG"])
    wg = restatement(m, core)
    steps = fixture_steps(f)
    tiny = np.zeros(core.PG + core.PD, bool)
    errs = []

    def check(k, kind, p0, v0, g, p1, v1, loss):
        ref = f["grad_%d" % k]
        l64, g64 = wg.loss_grad(p0, X, C, steps[k][1], steps[k][2], kind)
        e_ref = np.abs(g - ref).max() / np.abs(ref).max()
        e64 = np.abs(g - g64).max() / np.abs(g64).max()
        errs.append((k, kind, e_ref, e64))
        assert e_ref < GRAD_TOL and e64 < GRAD_TOL, errs
        assert abs(loss - l64) <= 1e-5 * max(1.0, abs(l64)), (k, loss, l64)
        sl = slice(core.PG, core.PG + core.PD) if kind else slice(0, core.PG)
        tiny[sl] |= np.abs(g64) < 1e-6 * np.abs(g64).max()

    run_steps(m, core, X, C, steps, check)
    print("gradient errors (step, kind, vs reference, vs float64):", errs)
    # RMSprop's first step is ~10 lr sign(g): only an element whose gradient is ~0 may take the other sign
    p = core.flat[:core.PG + core.PD].cpu().numpy()
    dp = np.abs(p - f["pK"])
    lr = kw.get("lr", 5e-5)
    print("trajectory: max |dp| %.3g, outside the %d near-zero gradients %.3g" % (dp.max(), tiny.sum(), dp[~tiny].max()))
    assert dp[~tiny].max() <= 1e-6 + 0.01 * lr


@pytest.mark.parametrize("path", FIXTURES, ids=fid)
def test_rmsprop_and_clamp_to_the_ulp(path):
    f, kw, X, C = load(path)
    m, core = model_of(kw, X, C, f["p0"])
    lr, wd = kw.get("lr", 5e-5), kw.get("weight_decay", 0)

    def check(k, kind, p0, v0, g, p1, v1, loss):
        sl = slice(core.PG, core.PG + core.PD) if kind else slice(0, core.PG)
        other = slice(0, core.PG) if kind else slice(core.PG, core.PG + core.PD)
        pr, vr = wt.rmsprop_f32(p0[sl], g, v0[sl], lr, wd=wd, clamp=0.01 if kind else 0.0)
        assert (np.abs(p1[sl] - pr) <= np.spacing(np.abs(pr))).all(), np.abs(p1[sl] - pr).max()
        assert (np.abs(v1[sl] - vr) <= np.spacing(np.abs(vr))).all()
        assert np.array_equal(p1[other], p0[other]) and np.array_equal(v1[other], v0[other])   # only the stepped net moves
        if kind:
            assert np.abs(p1[sl]).max() <= np.float32(0.01)

    run_steps(m, core, X, C, fixture_steps(f), check)


SHAPES = {   # name: (n, d, c, latent, g_hidden, d_hidden, g_act, d_act, batch)
    "deep_relu": (300, 6, 2, 2, (24, 40, 17), (33, 20, 28, 9), 'relu', 'relu', 64),
    "nocond_tanh": (200, 4, 0, 3, (30, 30), (25,), 'tanh', 'tanh', 50),
    "big_batch": (5000, 7, 3, 2, (64, 48), (40, 40), 'relu', 'tanh', 4096),   # 4096 rows over many workgroups
}


def synth(name, seed=0):
    n, d, c, lat, gh, dh, ga, da, bs = SHAPES[name]
    rng = np.random.default_rng(seed + len(name))
    X = rng.normal(size=(n, d)).astype(np.float32)
    C = rng.normal(size=(n, c)).astype(np.float32) if c else None
    kw = dict(latent_dim=lat, generator_hidden=gh, discriminator_hidden=dh, generator_activation=ga,
              discriminator_activation=da, batch_size=bs, lr=1e-3, weight_decay=0.001)
    return X, C, kw, rng


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_gradients_and_epoch_losses_match_float64(name):
    X, C, kw, rng = synth(name)
    torch.manual_seed(1)
    m, core = model_of(kw, X, C)
    # a few steps first, so that the critic is clamped and the generator has moved
    n, B, lat = X.shape[0], kw["batch_size"], kw["latent_dim"]
    steps = []
    for k in range(4):
        rows = rng.permutation(n)[:B]
        steps.append((int(k % 2 == 1), rows, rng.normal(size=(B, lat)).astype(np.float32)))
    wg = restatement(m, core)

    def check(k, kind, p0, v0, g, p1, v1, loss):
        l64, g64 = wg.loss_grad(p0, X, C, steps[k][1], steps[k][2], kind)
        scale = max(np.abs(g64).max(), wg.grad_scale(p0, X, C, steps[k][1], steps[k][2], kind))
        assert np.abs(g - g64).max() <= GRAD_TOL * scale, (k, np.abs(g - g64).max(), np.abs(g64).max(), scale)
        assert abs(loss - l64) <= 1e-5 * max(1.0, abs(l64)) + 1e-6

    run_steps(m, core, X, C, steps, check)
    Z = rng.normal(size=(n, lat)).astype(np.float32)
    out = torch.zeros(2, device=DEV)
    W.epoch_losses(core.shape, core.flat, dev(X), dev(C), dev(Z), n, out, core.workspace(0, n))
    gen, disc = wg.epoch_losses(core.flat.cpu().numpy(), X, C, Z)
    o = out.cpu().numpy()
    assert abs(o[0] - gen) <= 1e-5 * max(1.0, abs(gen)) and abs(o[1] - disc) <= 1e-5 * max(1.0, abs(disc)), (o, gen, disc)
    # inference entry points
    p = core.flat.cpu().numpy()
    np.testing.assert_allclose(m.generator(Z[:77], None if C is None else C[:77]).cpu().numpy(),
                               wg.generate(p, Z[:77], None if C is None else C[:77]), rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(m.discriminator(X[:77], None if C is None else C[:77]).cpu().numpy(),
                               wg.critic(p, X[:77], None if C is None else C[:77]), rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("name", ["deep_relu", "big_batch"])
def test_fit_epoch_equals_the_step_loop_bitwise(name):
    X, C, kw, rng = synth(name, 5)
    n, B, lat = X.shape[0], kw["batch_size"], kw["latent_dim"]
    torch.manual_seed(2)
    m1, c1 = model_of(kw, X, C)
    m2, c2 = model_of(kw, X, C, c1.flat[:c1.PG + c1.PD].cpu())
    Xd, Cd = dev(X), dev(C)
    opt = m1.opt_gen.hyper(0.01)
    for epoch in range(2):
        perm = dev(rng.permutation(n), torch.int64)
        z = dev(rng.normal(size=(n, lat)))
        zf = dev(rng.normal(size=(n, lat)))
        kinds = step_kinds(3 * epoch + 1, -(-n // B), 2)
        e1 = torch.zeros(2, device=DEV)
        W.fit_epoch(c1.shape, c1.flat, c1.square_avg, Xd, Cd, perm, z, zf, n, B, kinds, opt, e1, c1.workspace(B, n))
        for b, s in enumerate(range(0, n, B)):
            e = min(n, s + B)
            W.train_step(c2.shape, int(kinds[b]), c2.flat, c2.square_avg, Xd, Cd, perm[s:e], z[s:e], e - s, opt, None, None,
                         c2.workspace(B))
        e2 = torch.zeros(2, device=DEV)
        W.epoch_losses(c2.shape, c2.flat, Xd, Cd, zf, n, e2, c2.workspace(0, n))
        torch.cuda.synchronize()
        assert torch.equal(c1.flat, c2.flat) and torch.equal(c1.square_avg, c2.square_avg) and torch.equal(e1, e2)


def test_n_critic_schedules_match_float64_fit():
    """n_critic 1 (generator steps only), 2 and a float n_critic through the public fit, against the restated loop"""
    X, C, kw, _ = synth("nocond_tanh", 3)
    X, C = X[:90], np.random.default_rng(4).normal(size=(90, 2)).astype(np.float32)
    for n_critic in (1, 2, 2.5):
        args = dict(kw, n_critic=n_critic, n_epochs=2, batch_size=32)
        torch.manual_seed(7)
        m = ConditionalWGAN(**args)
        m.fit(X, C)
        after = torch.rand(1)
        # restate: the same init (the reference builds the nets on the CPU first), then the replayed draws
        torch.manual_seed(7)
        m2 = ConditionalWGAN(**args)
        m2._model_init(X, C)
        p0 = m2._core.flat[:m2._core.PG + m2._core.PD].cpu().numpy()
        epochs, state = wt.replay_draws(torch.get_rng_state(), 90, 32, args["latent_dim"], 2)
        wg = restatement(m2, m2._core)
        p, hist = wt.fit(wg, p0, X, C, epochs, args["lr"], n_critic, wd=args["weight_decay"])
        g = torch.Generator(); g.set_state(state)
        assert torch.equal(after, torch.rand(1, generator=g))
        got = m._core.flat[:p.size].cpu().numpy()
        assert np.abs(got - p).max() <= 1e-6 + 0.01 * args["lr"], (n_critic, np.abs(got - p).max())
        h = np.array([[float(a), float(b)] for a, b in zip(m.gen_loss_history, m.disc_loss_history)])
        # parameters within lr / 100 move the clamped critic's outputs (~1e-2) by up to ~1e-3 of themselves
        np.testing.assert_allclose(h, np.array(hist), rtol=2e-3, atol=1e-3 * np.abs(np.array(hist)).max())


@pytest.mark.parametrize("path", FIXTURES, ids=fid)
def test_seeded_fit_matches_reference(path):
    f, kw, X, C = load(path)
    torch.manual_seed(int(f["seed"]))
    m = ConditionalWGAN(**dict(kw, n_epochs=3))
    assert m.fit(X, C) is None
    assert torch.equal(torch.rand(1), torch.from_numpy(f["rand_after_fit"]))
    assert len(m.gen_loss_history) == 3 and all(t.dim() == 0 and t.dtype == torch.float32 and t.device.type == "cpu"
                                                for t in m.gen_loss_history + m.disc_loss_history)
    gh = np.array([float(v) for v in m.gen_loss_history]); dh = np.array([float(v) for v in m.disc_loss_history])
    scale = max(np.abs(f["gen_hist"]).max(), np.abs(f["disc_hist"]).max())
    print("histories: gen", gh, f["gen_hist"], "disc", dh, f["disc_hist"])
    assert np.abs(gh - f["gen_hist"]).max() <= 1e-4 * scale and np.abs(dh - f["disc_hist"]).max() <= 1e-4 * scale
    g = m._core.flat[:m._core.PG].cpu().numpy()
    lr = kw.get("lr", 5e-5)
    dg = np.abs(g - f["fit_g"])
    print("generator after fit: max |dp| %.3g, elements beyond lr/100: %d" % (dg.max(), (dg > 0.01 * lr).sum()))
    assert (dg > 1e-6 + 0.01 * lr).mean() <= 1e-3 and dg.max() <= 25 * lr
    X_gen = m.sample(C) if C is not None else m.sample(X.shape[0])
    assert X_gen.dtype == np.float32 and X_gen.shape == X.shape
    assert torch.equal(torch.rand(1), torch.from_numpy(f["rand_after_sample"]))
    np.testing.assert_allclose(X_gen, f["sample"], rtol=1e-3, atol=1e-3 * np.abs(f["sample"]).max())
    sd = m.state_dict()
    assert list(sd)[0] == "generator.model.0.weight" and list(sd)[-1] == "discriminator.model.%d.bias" % (
        2 * len(m.discriminator_hidden))


def test_same_seed_gives_bitwise_the_same_fit():
    X, C, kw, _ = synth("deep_relu", 9)
    outs = []
    for _ in range(2):
        torch.manual_seed(11)
        m = ConditionalWGAN(**dict(kw, n_epochs=3))
        m.fit(X, C)
        outs.append((m._core.flat.cpu(), torch.stack(m.gen_loss_history + m.disc_loss_history), torch.from_numpy(m.sample(C))))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_cuda_tensor_and_numpy_inputs_agree():
    X, C, kw, _ = synth("nocond_tanh", 12)
    C = np.random.default_rng(1).normal(size=(X.shape[0], 2)).astype(np.float32)
    res = []
    for to in (lambda a: a, lambda a: torch.from_numpy(a).to(DEV), lambda a: torch.from_numpy(a).double()):
        torch.manual_seed(3)
        m = ConditionalWGAN(**dict(kw, n_epochs=2))
        m.fit(to(X), to(C))
        res.append((m._core.flat.cpu(), m.sample(to(C))))
    for r in res[1:]:
        assert torch.equal(res[0][0], r[0]) and np.array_equal(res[0][1], r[1])


def test_api_errors():
    X, C, kw, _ = synth("nocond_tanh", 13)
    C = np.ones((X.shape[0], 2), np.float32)
    m = ConditionalWGAN(**dict(kw, n_epochs=1))
    m.fit(X, C)
    with pytest.raises(RuntimeError):
        m.sample(10)                              # a conditional generator needs conditions
    with pytest.raises(RuntimeError):
        m.sample(np.ones((5, 3), np.float32))     # the wrong condition width
    assert m.sample(C[:7]).shape == (7, X.shape[1])
    m.fit(X)                                      # fit re-initialises: now unconditional
    assert m.sample(9).shape == (9, X.shape[1])
