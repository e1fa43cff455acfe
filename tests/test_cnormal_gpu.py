"""ConditionalNormal on the GPU: the HIP kernels of libpf_cnormal.so against the reference's committed fixtures
(tests/golden/cnormal_*.npz, tests/golden/make_golden_cnormal.py) and the torch restatement (tests/cnormal_torch.py).

Tolerances are measured, not chosen: for every compared quantity the float32 reference's own error against the float64
restatement on the same inputs, e_ref, is computed here on the CPU (from the fixture, or from the restatement's float32 mode,
which tests/test_cnormal_host.py pins to the fixtures); the GPU's error against the same float64 numbers must be at most
4 e_ref, with a floor of 4 float32 ulp of the quantity's magnitude where e_ref is smaller.  profiles/r09_cnormal_parity.txt
holds both numbers per case and quantity (the PARITY lines this file prints).  RNG consumption, lengths and the bitwise
checks are exact."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import cnormal_torch as ct  # noqa: E402
import hygiene  # noqa: E402
import native_libs  # noqa: E402
from parity import parity  # noqa: E402
from test_cnormal_host import NAMES, cond_of, fixture_batches, load, restatement  # noqa: E402
from probaforms_amd.models import _cnormal_lib as N  # noqa: E402
from probaforms_amd.models.cnormal import ConditionalNormal, Net  # noqa: E402

pytestmark = pytest.mark.gpu

native_libs.ensure_built(N)

DEV = torch.device("cuda")


def dev(a, dtype=torch.float32):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def model_of(kw, X, C, params=None):
    """a ConditionalNormal with its net built (as fit builds it) and, optionally, the given flat parameters"""
    m = ConditionalNormal(**kw)
    m._model_init(X, cond_of(X, C))
    core = m.model._core
    if params is not None:
        core.flat[:core.P].copy_(torch.as_tensor(np.asarray(params, np.float32)))
    return m, core


def gpu_loss_grad(core, Xd, Cd, rows, params=None, ws=None):
    if params is not None:
        core.flat[:core.P].copy_(torch.as_tensor(np.asarray(params, np.float32)))
    g = torch.full((core.P,), float("nan"), device=DEV)
    loss = torch.full((1,), float("nan"), device=DEV)
    st = torch.full((1,), -7, dtype=torch.int32, device=DEV)
    N.loss_grad(core.shape, core.flat, Xd, Cd, dev(rows, torch.int64), len(rows), g, loss, st, ws or core.workspace(len(rows)))
    assert int(st) == 0
    return float(loss), g.cpu().numpy()


@pytest.mark.parametrize("name", NAMES)
def test_forward_matches_the_fixture(name):
    f, kw, X, C = load(name)
    Cz = cond_of(X, C)
    net = restatement(kw, X, C)
    m, core = model_of(kw, X, C, f["p_end"])
    n, d = X.shape
    outs = [torch.full((n, d), float("nan"), device=DEV) for _ in range(4)]
    st = torch.full((1,), -7, dtype=torch.int32, device=DEV)
    N.forward(core.shape, core.flat, dev(Cz), dev(f["fwd_eps"]), dev(X), n, outs[0], outs[1], outs[2], outs[3], st)
    assert int(st) == 0
    ref64 = net.forward(f["p_end"], Cz, f["fwd_eps"], X)            # (x_tilde, inv, mu, sigma)
    for got, r64, key in ((outs[0], ref64[2], "fwd_mu"), (outs[1], ref64[3], "fwd_sigma"), (outs[2], ref64[0], "fwd_xt"),
                          (outs[3], ref64[1], "fwd_inv")):
        parity(name, key, got.cpu().numpy(), f[key], r64)
    # the module: the same numbers, eps from the global generator
    torch.manual_seed(5)
    eps = torch.randn(n, d)
    torch.manual_seed(5)
    xt, inv, mu, sigma = m.model(X, Cz)
    assert torch.equal(torch.rand(1), (torch.manual_seed(5), torch.randn(n, d), torch.rand(1))[2])
    r = net.forward(f["p_end"], Cz, eps.numpy(), X)
    assert all(t.device.type == "cuda" and not t.requires_grad for t in (xt, inv, mu, sigma))
    np.testing.assert_allclose(xt.cpu().numpy(), r[0], rtol=1e-4, atol=1e-4 * np.abs(r[0]).max())
    assert torch.equal(inv, outs[3]) and torch.equal(mu, outs[0]) and m.model(None, Cz)[1] is None


@pytest.mark.parametrize("name", NAMES)
def test_loss_grad_matches_the_recorded_gradients(name):
    f, kw, X, C = load(name)
    Cz = cond_of(X, C)
    net = restatement(kw, X, C)
    m, core = model_of(kw, X, C, f["p0"])
    batches = fixture_batches(f)
    before = {}
    ct.fit(net, f["p0"], X, Cz, batches, kw.get("lr", 1e-4), kw.get("weight_decay", 0), torch.float32,
           lambda k, loss, g, p: before.__setitem__(k, p))       # the reference's parameters in front of each step
    Xd, Cd = dev(X), dev(Cz)
    for k, rows in enumerate(batches):
        l64, g64 = net.loss_grad(before[k], X, Cz, rows)
        loss, g = gpu_loss_grad(core, Xd, Cd, rows, before[k])
        parity(name, "grad step %d" % k, g, f["grad_%d" % k], g64)
        parity(name, "loss step %d" % k, loss, f["loss_history"][k], l64)
        if net.independent:
            assert not g[net.P_main:].any()


@pytest.mark.parametrize("name", NAMES)
def test_seeded_fit_matches_the_reference(name):
    f, kw, X, C = load(name)
    Cz = cond_of(X, C)
    net = restatement(kw, X, C)
    n, d = X.shape
    B, E = kw.get("batch_size", 32), kw.get("n_epochs", 10)
    torch.manual_seed(int(f["seed"]))
    m = ConditionalNormal(**kw)
    assert m.fit(X, C) is None
    assert torch.equal(torch.rand(1), torch.from_numpy(f["rand_after_fit"]))
    assert len(m.loss_history) == E * -(-n // B)
    assert all(t.dim() == 0 and t.dtype == torch.float32 and t.device.type == "cpu" for t in m.loss_history)
    core = m.model._core
    assert m.opt.step_count == len(m.loss_history)
    # the float64 run on the same batches
    torch.manual_seed(int(f["seed"]))
    Net(d, Cz.shape[1], kw.get("hidden", (10,)), kw.get("activation", "tanh"))
    epochs, _ = ct.replay_draws(torch.get_rng_state(), n, B, d, E)
    p64, l64 = ct.fit(net, f["p0"], X, Cz, [b for e in epochs for b in e], kw.get("lr", 1e-4), kw.get("weight_decay", 0))
    parity(name, "fit loss_history", np.array([float(v) for v in m.loss_history]), f["loss_history"], l64)
    got = core.flat[:core.P].cpu().numpy()
    parity(name, "fit parameters", got, f["p_end"], p64)
    # sample: eps is the global generator's next randn(rows, d)
    torch.manual_seed(int(f["seed"]) + 1)
    arg = int(f["sample_arg"])
    Cs = Cz if arg < 0 else np.zeros((arg, 1), np.float32)
    g = torch.Generator(); g.set_state(torch.get_rng_state())
    eps = torch.randn(Cs.shape[0], d, generator=g).numpy()
    S = m.sample(C if arg < 0 else arg)
    assert S.dtype == np.float32 and S.shape == f["sample"].shape == (Cs.shape[0], d)
    assert torch.equal(torch.get_rng_state(), g.get_state())
    x64 = net.forward(got, Cs, eps)[0]
    x32 = net.forward(got, Cs, eps, dtype=torch.float32)[0]
    parity(name, "sample (own params)", S, x32, x64)
    # against the fixture's sample: the fixture's eps is the stream after rand_after_fit
    torch.manual_seed(int(f["seed"]))
    m2 = ConditionalNormal(**kw)
    m2.fit(X, C)
    torch.rand(1)
    g = torch.Generator(); g.set_state(torch.get_rng_state())
    eps = torch.randn(Cs.shape[0], d, generator=g).numpy()
    S2 = m2.sample(C if arg < 0 else arg)
    assert torch.equal(torch.rand(1), torch.from_numpy(f["rand_after_sample"]))
    parity(name, "sample (fixture)", S2, f["sample"], net.forward(p64, Cs, eps)[0])


def test_independent_mode_never_touches_out():
    f, kw, X, C = load("indep")
    assert kw["weight_decay"] > 0 and kw["use_independent_covariance"]
    torch.manual_seed(int(f["seed"]))
    m = ConditionalNormal(**kw)
    m.fit(X, C)
    core = m.model._core
    P, Pm = core.P, core.P - 5 * 5 - 5
    p = core.flat[:P].cpu().numpy()
    assert np.array_equal(p[Pm:].view(np.uint32), f["p0"][Pm:].view(np.uint32))          # bitwise
    assert np.array_equal(m.model.out.weight.detach().cpu().numpy().reshape(-1), f["p0"][Pm:Pm + 25])
    assert not m.opt.exp_avg[Pm:P].any() and not m.opt.exp_avg_sq[Pm:P].any()
    assert m.opt.exp_avg[:Pm].any() and not np.array_equal(p[:Pm], f["p0"][:Pm])


SHAPES = {   # name: (d, c, hidden, activation, independent)
    "d_at_bound": (N.MAX_D, 3, (10,), 'tanh', False),
    "eight_layers": (6, 2, (4,) * 8, 'sigmoid', False),
    "indep_relu": (7, 3, (33, 20), 'relu', True),
}


def synth(name, n=1000, seed=0):
    d, c, hidden, act, indep = SHAPES[name]
    rng = np.random.default_rng(seed + len(name))
    X = rng.normal(size=(n, d)).astype(np.float32)
    C = rng.normal(size=(n, c)).astype(np.float32)
    kw = dict(hidden=hidden, activation=act, use_independent_covariance=indep, batch_size=700, lr=1e-3, weight_decay=0.01)
    torch.manual_seed(seed)
    m, core = model_of(kw, X, C)
    with torch.no_grad():
        m.model.out.weight.add_(torch.eye(d, device=DEV))           # a well-conditioned out.weight for any d
    return m, core, X, C, kw, ct.Normal(d, c, hidden, act, indep), rng


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_many_workgroups_and_ragged_batches_match_float64(name):
    m, core, X, C, kw, net, rng = synth(name)
    n = X.shape[0]
    Xd, Cd = dev(X), dev(C)
    p0 = core.flat[:core.P].cpu().numpy()
    for B in (1, 2, 33, 65, 700):
        rows = rng.permutation(n)[:B]
        l64, g64 = net.loss_grad(p0, X, C, rows)
        l32, g32 = net.loss_grad(p0, X, C, rows, torch.float32)
        loss, g = gpu_loss_grad(core, Xd, Cd, rows)
        parity(name, "grad %d rows" % B, g, g32, g64)
        parity(name, "loss %d rows" % B, loss, l32, l64)
    # one epoch of n = 1000 at batch 700: 700 and 300 rows
    perm = rng.permutation(n)
    batches = [perm[:700], perm[700:]]
    p64, l64 = ct.fit(net, p0, X, C, batches, kw["lr"], kw["weight_decay"])
    p32, l32 = ct.fit(net, p0, X, C, batches, kw["lr"], kw["weight_decay"], torch.float32)
    losses = torch.full((2,), float("nan"), device=DEV)
    st = torch.full((1,), -7, dtype=torch.int32, device=DEV)
    N.fit_epoch(core.shape, core.flat, m.opt.exp_avg, m.opt.exp_avg_sq, Xd, Cd, dev(perm, torch.int64), n, 700,
                N.adam(kw["lr"], kw["weight_decay"]), 1, losses, st, core.workspace(700))
    assert int(st) == 0
    parity(name, "epoch losses", losses.cpu().numpy(), l32, l64)
    parity(name, "epoch parameters", core.flat[:core.P].cpu().numpy(), p32, p64)


@pytest.mark.parametrize("name", ["d_at_bound", "indep_relu"])
def test_fit_epoch_equals_the_step_loop_bitwise(name):
    m1, c1, X, C, kw, net, rng = synth(name, n=333, seed=4)
    m2, c2 = model_of(kw, X, C, c1.flat[:c1.P].cpu().numpy())
    m3, c3 = model_of(kw, X, C, c1.flat[:c1.P].cpu().numpy())
    n, B = X.shape[0], 100
    Xd, Cd = dev(X), dev(C)
    opt = N.adam(kw["lr"], kw["weight_decay"])
    nb = -(-n // B)
    for epoch in range(2):
        perm = dev(rng.permutation(n), torch.int64)
        l1, l3 = torch.zeros(nb, device=DEV), torch.zeros(nb, device=DEV)
        for (m, c, l) in ((m1, c1, l1), (m3, c3, l3)):             # two identical calls: identical bits
            N.fit_epoch(c.shape, c.flat, m.opt.exp_avg, m.opt.exp_avg_sq, Xd, Cd, perm, n, B, opt, epoch * nb + 1, l, None,
                        c.workspace(B))
        l2 = torch.zeros(nb, device=DEV)
        for b, s in enumerate(range(0, n, B)):
            e = min(n, s + B)
            N.train_step(c2.shape, c2.flat, m2.opt.exp_avg, m2.opt.exp_avg_sq, Xd, Cd, perm[s:e], e - s, opt, epoch * nb + b + 1,
                         None, l2[b:b + 1], None, c2.workspace(B))
        torch.cuda.synchronize()
        for a, b in ((c1.flat, c2.flat), (m1.opt.exp_avg, m2.opt.exp_avg), (m1.opt.exp_avg_sq, m2.opt.exp_avg_sq), (l1, l2),
                     (c1.flat, c3.flat), (m1.opt.exp_avg_sq, m3.opt.exp_avg_sq), (l1, l3)):
            assert hygiene.same_bits(a, b)


@pytest.mark.parametrize("entry", ["loss_grad", "train_step", "fit_epoch"])
def test_no_result_depends_on_the_workspace(entry):
    m, core, X, C, kw, net, rng = synth("eight_layers", n=150, seed=6)
    n, B = X.shape[0], 64
    Xd, Cd = dev(X), dev(C)
    p0 = core.flat.clone()
    perm = dev(rng.permutation(n), torch.int64)
    other = dev(rng.permutation(n), torch.int64)
    opt = N.adam(kw["lr"], kw["weight_decay"])
    nbytes = N.workspace_bytes(core.shape, B)
    outs = {}
    for pat in hygiene.PATTERNS:
        ws = hygiene.workspace(nbytes, pattern=pat)
        p, ea, es = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
        g, loss, losses = torch.empty(core.P, device=DEV), torch.empty(1, device=DEV), torch.empty(-(-n // B), device=DEV)
        st = torch.empty(1, dtype=torch.int32, device=DEV)

        def call(rows_perm):
            if entry == "loss_grad":
                N.loss_grad(core.shape, p, Xd, Cd, rows_perm[:B], B, g, loss, st, ws)
                return dict(grad=g, loss=loss, status=st)
            if entry == "train_step":
                N.train_step(core.shape, p, ea, es, Xd, Cd, rows_perm[:B], B, opt, 1, g, loss, st, ws)
                return dict(grad=g, loss=loss, status=st, params=p, exp_avg=ea, exp_avg_sq=es)
            N.fit_epoch(core.shape, p, ea, es, Xd, Cd, rows_perm, n, B, opt, 1, losses, st, ws)
            return dict(losses=losses, status=st, params=p, exp_avg=ea, exp_avg_sq=es)

        if pat == "replay":                 # the workspace as a previous, different call left it
            call(other)
            p.copy_(p0); ea.zero_(); es.zero_()
        hygiene.poison_outputs(g, loss, losses, st)
        got = call(perm)
        torch.cuda.synchronize()
        hygiene.assert_all_written(got, "pfn_%s [%s]" % (entry, pat))
        outs[pat] = {k: v.clone() for k, v in got.items()}
    hygiene.assert_pattern_independent(outs, "pfn_%s" % entry)


def test_singular_out_weight_is_an_error_not_a_fault():
    f, kw, X, C = load("default")
    m, core = model_of(kw, X, C, f["p0"])
    with torch.no_grad():
        m.model.out.weight.zero_()
    with pytest.raises(RuntimeError, match="singular"):
        m.model(X, C)
    assert m.model(None, C)[0].shape == X.shape                  # without X nothing is inverted
    # a training step on it: the error word is set, parameters and optimizer state keep their bits
    before = core.flat.clone()
    st = torch.zeros(1, dtype=torch.int32, device=DEV)
    N.train_step(core.shape, core.flat, m.opt.exp_avg, m.opt.exp_avg_sq, dev(X), dev(C), None, 32, N.adam(1e-3, 0.01), 1, None,
                 None, st, core.workspace(32))
    assert int(st) == 1 and hygiene.same_bits(core.flat, before) and not m.opt.exp_avg.any() and not m.opt.exp_avg_sq.any()
    with pytest.raises(RuntimeError, match="singular"):
        mm = ConditionalNormal(n_epochs=1)
        orig = mm._model_init

        def init(X_, C_):
            orig(X_, C_)
            with torch.no_grad():
                mm.model.out.weight.zero_()
        mm._model_init = init
        mm.fit(X, C)
