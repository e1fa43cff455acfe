"""Data-parallel epochs in which a rank's share of a batch is empty (rnvp_fit_epoch_dp_cb / _chunked).

A rank whose share of a global batch has no rows launches no training kernel for it, yet runs the step's Adam launch, which reads
the training error word kept in the workspace.  That word is cleared by the pack launch of the rank's first training kernel -- so a
rank whose share is empty from the FIRST batch of the call on (batch_size < world, n < world) met whatever the workspace held: with
a non-zero word it skipped Adam and wrote the protocol NaN into loss_hist while the other ranks stepped.  Here every rank of a
world of 2 and 4 runs its epoch in one process with the identity exchange (the rank trains on its own share alone: a well-defined
computation), on every workspace pattern of tests/hygiene.py, against the epoch restated with the oracle.
"""
import functools

import numpy as np
import pytest
import torch

import hygiene

pytestmark = pytest.mark.gpu

# (L, d, c, hidden): the C2 flow and a small flow, both on the register-chained kernels
FLOWS = {"c2": (8, 16, 4, (128,)), "small": (4, 5, 3, (16,))}
# (n, batch_size): a ragged one-row last batch; batch_size < world; n < world = 4; a row-parallel batch, then one row
SIZES = [(97, 32), (5, 1), (3, 8), (8192 + 1, 8192)]
LR, WD = 1e-3, 0.05                          # weight decay: a skipped step is visible even where the gradient is zero


def _share(s0, rows, rank, world):
    base, rem = divmod(rows, world)
    lo = s0 + rank * base + min(rank, rem)
    return lo, base + (1 if rank < rem else 0)


# (the 8193-row epoch of the eight-layer C2 flow is restated with the oracle for two ranks only: seconds of CPU per rank)
CASES = [(flow, world, n, bs) for flow in FLOWS for world in (2, 4) for (n, bs) in SIZES if not (flow == "c2" and n > 8192 and world == 4)]


def _data(flow, n, bs):
    L, d, c, hidden = FLOWS[flow]
    g = torch.Generator().manual_seed(n + bs)
    X = torch.randn(n, d, generator=g); C = torch.randn(n, c, generator=g)
    return X, C, torch.randperm(n, generator=g)


def _init_params(flow):
    """the flat parameters every run starts from (torch.manual_seed(0), the reference's layer initialisation)"""
    from probaforms_amd.models import RealNVPLayer
    L, d, c, hidden = FLOWS[flow]
    torch.manual_seed(0)
    layers = [RealNVPLayer(d, c, (torch.arange(d) + i) % 2, hidden, "tanh") for i in range(L)]
    return layers, torch.cat([p.detach().reshape(-1) for l in layers for p in l.parameters()]).numpy().astype(np.float32)


@functools.lru_cache(maxsize=None)
def _oracle_epoch(flow, world, n, bs, rank):
    """the oracle's epoch of one rank (the same for both chunk counts): per batch its rows' loss and gradient scaled by 1 / rows_global,
    zeros where the share is empty, then Adam -> (params, exp_avg, exp_avg_sq, loss history)"""
    from oracle import Oracle, Shape
    oracle32 = Oracle(32)
    L, d, c, hidden = FLOWS[flow]
    so = Shape.make(L, d, c, hidden, "tanh")
    X, C, perm = _data(flow, n, bs)
    Xn, Cn, pn = X.numpy(), C.numpy(), perm.numpy()
    pr = _init_params(flow)[1].copy(); mr = np.zeros_like(pr); vr = np.zeros_like(pr)
    hist = []
    for k in range((n + bs - 1) // bs):
        s0 = k * bs
        rows = min(bs, n - s0)
        lo, mine = _share(s0, rows, rank, world)
        if mine:
            idx = pn[lo:lo + mine]
            loss, grad = oracle32.loss_grad(so, pr, Xn[idx], Cn[idx], inv_B=1.0 / rows)
        else:
            loss, grad = 0.0, np.zeros_like(pr)
        oracle32.adam(pr, grad, mr, vr, k + 1, lr=LR, weight_decay=WD)
        hist.append(loss)
    return pr, mr, vr, hist


@pytest.mark.parametrize("chunks", [1, 3])
@pytest.mark.parametrize("flow,world,n,bs", CASES)
def test_rank_with_an_empty_share_steps_like_the_others(flow, world, n, bs, chunks, oracle32):
    from probaforms_amd import _engine, _hip
    from probaforms_amd.models import NormalizingFlow, RealNVPLayer, StandardNormalPrior
    L, d, c, hidden = FLOWS[flow]
    dev = torch.device("cuda", 0)
    X, C, perm = _data(flow, n, bs)
    Xd, Cd, permd = X.to(dev), C.to(dev), perm.to(dev)
    lr, wd = LR, WD
    nb = (n + bs - 1) // bs

    def run(rank, pattern):
        layers, want_p0 = _init_params(flow)
        nf = NormalizingFlow(layers, StandardNormalPrior(d, dev))
        for p in nf.parameters():
            p.data = p.data.to(dev)
        eng = nf.engine()
        assert _hip.kernel_path(eng.shape, None, _hip.OP_TRAIN) == _hip.PATH_MFMA
        p0 = eng.flat[:eng.P].detach().cpu().numpy().copy()
        assert np.array_equal(p0, want_p0)
        opt = _engine.FlatAdam(eng.flat.numel(), dev, lr=lr, weight_decay=wd)
        ws = eng.workspace(_hip.OP_TRAIN, 2 * bs + 20)         # the engine's own buffer (grown, never shrunk): fit_epoch_dp gets this one
        hygiene.fill(ws, pattern)
        losses = torch.full((nb,), float("nan"), device=dev)
        if pattern == "replay":              # what a previous, larger epoch on the same engine leaves behind
            g2 = torch.Generator().manual_seed(5)
            X2 = torch.randn(4 * bs + 40, d, generator=g2).to(dev); C2 = torch.randn(4 * bs + 40, c, generator=g2).to(dev)
            other = _engine.FlatAdam(eng.flat.numel(), dev, lr=0.0, weight_decay=0.0)        # lr 0: the parameters stay put
            eng.fit_epoch_dp(other, None, X2, C2, torch.randperm(4 * bs + 40, generator=g2).to(dev), 2 * bs + 20,
                             torch.empty(2, device=dev), exchange=lambda t, count: None, rank=0, world=1, chunks=chunks)
            assert np.array_equal(eng.flat[:eng.P].detach().cpu().numpy(), p0)
        eng.fit_epoch_dp(opt, None, Xd, Cd, permd, bs, losses, exchange=lambda t, count: None, rank=rank, world=world, chunks=chunks)
        torch.cuda.synchronize()
        return p0, dict(params=eng.flat[:eng.P].detach().clone(), exp_avg=opt.exp_avg[:eng.P].clone(),
                        exp_avg_sq=opt.exp_avg_sq[:eng.P].clone(), loss_hist=losses)

    for rank in range(world):
        outs = {}
        for pattern in hygiene.PATTERNS:
            p0, outs[pattern] = run(rank, pattern)
        what = "fit_epoch_dp[%s, rank %d of %d, n %d, batch %d, chunks %d]" % (flow, rank, world, n, bs, chunks)
        # the oracle's epoch of this rank: its rows' loss and gradient scaled by 1 / rows_global, zeros where the share is empty
        pr, mr, vr, hist = _oracle_epoch(flow, world, n, bs, rank)
        for pattern in hygiene.PATTERNS:            # (each pattern against the oracle first: the message names what went wrong)
            o = outs[pattern]
            lh = o["loss_hist"].cpu()
            assert bool(torch.isfinite(lh).all()), "%s, workspace %r: loss_hist %s (0x7fc0dead is the protocol NaN: Adam was skipped)" % (
                what, pattern, [hex(v & 0xffffffff) for v in lh.view(torch.int32).tolist()][:8])
            assert all(bool(torch.isfinite(t).all()) for t in o.values()), (what, pattern)
            # bars of test_hip_kernels.py::test_adam_trajectory_vs_reference
            np.testing.assert_allclose(o["exp_avg"].cpu().numpy(), mr, rtol=2e-5, atol=3e-6 * np.abs(mr).max(), err_msg=what + pattern)
            np.testing.assert_allclose(o["exp_avg_sq"].cpu().numpy(), vr, rtol=4e-5, atol=6e-6 * np.abs(vr).max(), err_msg=what + pattern)
            assert np.abs(o["params"].cpu().numpy() - pr).mean() < 2e-6, (what, pattern)
            np.testing.assert_allclose(lh.numpy(), np.array(hist, np.float32), rtol=5e-5, atol=5e-5, err_msg=what + pattern)
        hygiene.assert_pattern_independent(outs, what)
