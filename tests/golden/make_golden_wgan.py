#!/usr/bin/env python3
"""Golden fixtures for ConditionalWGAN, produced by running the REFERENCE on the CPU.

    PYTHONPATH=<reference probaforms checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_wgan.py

Per case (tests/golden/wgan_<name>.npz): the seed, X and C, the initial generator and discriminator parameters
(wgan.py:175-181), then the first K iterations of a seeded fit -- each one's step kind, noise z (wgan.py:227), batch
rows (DataLoader(shuffle=True), replayed from the global generator and checked against what the networks saw) and the
gradient of the net that steps, taken with register_step_pre_hook on the reference's optimizers -- and both nets'
parameters after those K steps.  Then a 3-epoch fit from the same seed: its two loss histories, the generator's
parameters afterwards, sample(C) (or sample(n) without conditions) and torch.rand(1) after fit and after sample, which
pins the RNG consumption.  Flat parameter order: every nn.Linear's weight then bias, generator first."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
from probaforms.models.wgan import ConditionalWGAN  # the reference

assert not getattr(sys.modules["probaforms"], "__probaforms_amd__", False), "run this against the reference package"
torch.set_num_threads(1)

CASES = {   # name: (n, d, c, constructor kwargs, K iterations)
    "default": (100, 5, 3, dict(), 6),                             # tests/test_models.py shape, ConditionalWGAN defaults
    "nocond": (100, 5, 0, dict(), 6),
    "tanh_wd": (50, 3, 2, dict(latent_dim=3, generator_hidden=(16, 12), discriminator_hidden=(20, 8),
                               generator_activation='tanh', discriminator_activation='tanh', batch_size=16,
                               weight_decay=0.01, n_critic=3, lr=1e-3), 12),   # ragged last batch of 2 rows
}


class Stop(Exception):
    pass


def flat(params):
    return torch.cat([p.detach().reshape(-1) for p in params]).numpy().copy()


def replay(state, n, batch_size, lat, iters):
    """the fit's batch rows and noise, replayed from the global generator's state after _model_init"""
    g = torch.Generator()
    g.set_state(state)
    rows, zs = [], []
    while len(rows) < iters:
        torch.empty((), dtype=torch.int64).random_(generator=g)                     # DataLoader iterator base seed
        seed = int(torch.empty((), dtype=torch.int64).random_(generator=g).item())  # RandomSampler seed
        pg = torch.Generator()
        pg.manual_seed(seed)
        perm = torch.randperm(n, generator=pg)
        for s in range(0, n, batch_size):
            e = min(s + batch_size, n)
            rows.append(perm[s:e].numpy().copy())
            zs.append(torch.normal(0, 1, (e - s, lat), generator=g).numpy().copy())
        torch.normal(0, 1, (n, lat), generator=g)                                    # epoch-end losses
    return rows[:iters], zs[:iters]


def make_case(name):
    n, d, c, kw, K = CASES[name]
    seed = 1000 + len(name) * 17 + d
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, d)).astype(np.float32)
    C = rng.normal(size=(n, c)).astype(np.float32) if c else None
    out = dict(seed=np.int64(seed), X=X, C=C if C is not None else np.zeros((n, 0), np.float32), K=np.int64(K))
    for k, v in kw.items():
        out["kw_" + k] = np.asarray(v)

    # --- the first K iterations
    torch.manual_seed(seed)
    m = ConditionalWGAN(**kw)
    rec = dict(kind=[], grad=[], seen_z=[], seen_c=[], seen_x=[])
    orig_init = m._model_init

    def model_init(X_, C_=None):
        orig_init(X_, C_)
        rec["state"] = torch.get_rng_state()
        rec["p0"] = flat(list(m.generator.parameters()) + list(m.discriminator.parameters()))
        gfwd, dfwd = m.generator.forward, m.discriminator.forward

        def g_forward(Z, Cc=None):
            if Z.shape[0] == n:                        # the epoch-end losses (no batch here holds all n rows)
                return gfwd(Z, Cc)
            rec["seen_z"].append(Z.detach().numpy().copy())
            rec["seen_c"].append(None if Cc is None else Cc.detach().numpy().copy())
            return gfwd(Z, Cc)

        def d_forward(Xx, Cc=None):
            if not Xx.requires_grad and Xx.shape[0] != n:                   # a real batch (fake rows carry the generator's graph)
                rec["seen_x"].append((len(rec["seen_z"]), Xx.detach().numpy().copy()))
            return dfwd(Xx, Cc)

        m.generator.forward, m.discriminator.forward = g_forward, d_forward

        def hook(kind, net):
            def pre(opt, args, kwargs):
                if len(rec["grad"]) == K:
                    rec["pK"] = flat(list(m.generator.parameters()) + list(m.discriminator.parameters()))
                    raise Stop()
                rec["kind"].append(kind)
                rec["grad"].append(flat([p.grad for p in net.parameters()]))
            return pre

        m.opt_gen.register_step_pre_hook(hook(0, m.generator))
        m.opt_disc.register_step_pre_hook(hook(1, m.discriminator))

    m._model_init = model_init
    try:
        m.fit(X, C)
        raise AssertionError("fit ended before %d iterations" % K)
    except Stop:
        pass
    rows, zs = replay(rec["state"], n, m.batch_size, m.latent_dim, K)
    for k in range(K):
        assert np.array_equal(zs[k], rec["seen_z"][k]), (name, k)
        if C is not None:
            assert np.array_equal(C[rows[k]], rec["seen_c"][k]), (name, k)
    for (k, xs) in rec["seen_x"]:
        if k - 1 < K:
            assert np.array_equal(X[rows[k - 1]], xs), (name, k)
    assert rec["kind"] == [1 if i % m.n_critic != 0 else 0 for i in range(K)]
    out.update(p0=rec["p0"], pK=rec["pK"], kinds=np.array(rec["kind"], np.int8),
               batch_sizes=np.array([len(r) for r in rows], np.int64), rows=np.concatenate(rows).astype(np.int64),
               z=np.concatenate(zs).astype(np.float32),
               PG=np.int64(sum(p.numel() for p in m.generator.parameters())))
    for k in range(K):
        out["grad_%d" % k] = rec["grad"][k]

    # --- a seeded 3-epoch fit and sample
    torch.manual_seed(seed)
    m = ConditionalWGAN(**dict(kw, n_epochs=3))
    m.fit(X, C)
    out["rand_after_fit"] = torch.rand(1).numpy()
    out["gen_hist"] = np.array([float(v) for v in m.gen_loss_history], np.float32)
    out["disc_hist"] = np.array([float(v) for v in m.disc_loss_history], np.float32)
    out["fit_g"] = flat(m.generator.parameters())
    out["sample"] = m.sample(C) if C is not None else m.sample(n)
    out["rand_after_sample"] = torch.rand(1).numpy()
    path = os.path.join(HERE, "wgan_%s.npz" % name)
    np.savez_compressed(path, **out)
    print(name, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    for name in CASES:
        make_case(name)
