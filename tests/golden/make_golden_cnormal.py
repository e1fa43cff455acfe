#!/usr/bin/env python3
"""Golden fixtures for ConditionalNormal, produced by running the REFERENCE on the CPU.

    PYTHONPATH=<reference probaforms checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_cnormal.py

Per case (tests/golden/cnormal_<name>.npz): the seed, X, C and the constructor kwargs; the initial flat parameters; the
first K iterations of a seeded fit -- batch rows (DataLoader(shuffle=True), replayed from the global generator), loss and
the gradient taken with register_step_pre_hook on the reference's optimizer -- and the parameters after those K steps; the
whole fit's loss_history and final parameters, sample(C) and torch.rand(1) after fit and after sample, which pins the RNG
consumption; and one Net.forward(X, C) quadruple with the eps it drew.  Flat parameter order: every nn.Linear's weight
then bias, in module order (model.*, mu, log_sigma, out); a parameter without a gradient (out in independent mode)
is recorded as zeros.

The seeds are chosen so that (asserted below) cond(out.weight) < 100 before and after the fit, the first loss is below 100
and the float32 reference ends within 5 % of max |p_end - p_0| of a float64 run of tests/cnormal_torch.py on the same
batches: a fixture on which float32 itself wanders would make every parameter comparison vacuous."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import cnormal_torch as ct  # noqa: E402
from probaforms.models.cnormal import ConditionalNormal  # the reference

assert not getattr(sys.modules["probaforms"], "__probaforms_amd__", False), "run this against the reference package"
torch.set_num_threads(1)

K = 6
CASES = {   # name: (seed, n, d, c, constructor kwargs, sample argument)
    "default": (3, 100, 5, 3, dict(), None),                                   # the last batch has 4 rows
    "indep": (3, 100, 5, 3, dict(use_independent_covariance=True, weight_decay=0.01), None),
    "nocond": (3, 100, 5, 0, dict(), 7),                                      # C=None; pins sample(7)
    "sigmoid_deep": (3, 70, 12, 4, dict(hidden=(16, 12), activation='sigmoid', batch_size=16, lr=1e-3, weight_decay=0.01,
                                        n_epochs=3), None),                    # the last batch has 6 rows
    "d1": (3, 70, 1, 1, dict(hidden=(7,), activation='relu', batch_size=33), None),   # 1x1 inverse; 33 rows = a 32-row tile + 1
}


def flat(params, grads=False):
    return torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).reshape(-1) if grads else p.detach().reshape(-1)
                      for p in params]).numpy().copy()


def make_case(name, seed=None, write=True):
    seed0, n, d, c, kw, sample_arg = CASES[name]
    seed = seed0 if seed is None else seed
    rng = np.random.default_rng(1000 + seed)
    X = rng.normal(size=(n, d)).astype(np.float32)
    C = rng.normal(size=(n, c)).astype(np.float32) if c else None
    out = dict(seed=np.int64(seed), X=X, C=C if C is not None else np.zeros((n, 0), np.float32), K=np.int64(K))
    for k, v in kw.items():
        out["kw_" + k] = np.asarray(v)

    torch.manual_seed(seed)
    m = ConditionalNormal(**kw)
    rec = dict(grad=[], loss=[])
    orig_init = m._model_init

    def model_init(X_, C_):
        orig_init(X_, C_)
        rec["state"] = torch.get_rng_state()
        rec["p0"] = flat(m.model.parameters())

        def pre(opt, args, kwargs):
            if len(rec["grad"]) == K:
                rec.setdefault("pK", flat(m.model.parameters()))
            if len(rec["grad"]) < K:
                rec["grad"].append(flat(m.model.parameters(), grads=True))
        m.opt.register_step_pre_hook(pre)

    m._model_init = model_init
    assert m.fit(X, C) is None
    out["rand_after_fit"] = torch.rand(1).numpy()
    hist = np.array([float(v) for v in m.loss_history], np.float32)
    Cz = C if C is not None else np.zeros((n, 1), np.float32)
    epochs, _ = ct.replay_draws(rec["state"], n, m.batch_size, d, m.n_epochs)
    batches = [b for e in epochs for b in e]
    assert len(hist) == len(batches) == m.n_epochs * -(-n // m.batch_size)
    p_end = flat(m.model.parameters())
    out.update(p0=rec["p0"], pK=rec["pK"], batch_sizes=np.array([len(r) for r in batches[:K]], np.int64),
               rows=np.concatenate(batches[:K]).astype(np.int64), loss_history=hist, p_end=p_end)
    for k in range(K):
        out["grad_%d" % k] = rec["grad"][k]
    out["sample"] = m.sample(C) if sample_arg is None else m.sample(sample_arg)
    out["sample_arg"] = np.int64(-1 if sample_arg is None else sample_arg)
    out["rand_after_sample"] = torch.rand(1).numpy()

    # one Net.forward(X, C) with the eps it draws
    g = torch.Generator()
    g.set_state(torch.get_rng_state())
    eps = torch.randn(n, d, generator=g).numpy()
    with torch.no_grad():
        xt, inv, mu, sigma = m.model(torch.tensor(X), torch.tensor(Cz))
    out.update(fwd_eps=eps, fwd_xt=xt.numpy(), fwd_inv=inv.numpy(), fwd_mu=mu.numpy(), fwd_sigma=sigma.numpy())

    # the conditions a fixture must meet
    net = ct.Normal(d, Cz.shape[1], m.hidden, m.activation, m.independent_covariance)
    assert net.P == rec["p0"].size
    conds = (net.cond_out(rec["p0"]), net.cond_out(p_end))
    assert max(conds) < 100, (name, seed, conds)
    assert hist[0] < 100, (name, seed, hist[0])
    l32, g32 = net.loss_grad(rec["p0"], X, Cz, batches[0], torch.float32)          # the replayed rows are the fit's rows
    assert abs(float(l32) - hist[0]) <= 1e-5 * max(1.0, abs(hist[0])), (name, seed, l32, hist[0])
    p64, _ = ct.fit(net, rec["p0"], X, Cz, batches, m.lr, m.weight_decay, torch.float64)
    move = np.abs(p_end - rec["p0"]).max()
    drift = np.abs(p_end - p64).max()
    assert drift < 0.05 * move, (name, seed, drift, move)
    info = "%s seed %d: cond %.1f -> %.1f, first loss %.3f, float32 drift %.3g of move %.3g" % (
        name, seed, conds[0], conds[1], hist[0], drift, move)
    if write:
        path = os.path.join(HERE, "cnormal_%s.npz" % name)
        np.savez_compressed(path, **out)
        info += ", %d bytes" % os.path.getsize(path)
    print(info)


if __name__ == "__main__":
    for name in CASES:
        make_case(name)
