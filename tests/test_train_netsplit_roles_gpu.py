"""The d <= 16 net-split training kernel (k_mfma_train<2, CQ, R, 1, ACT, BXF>) at the smallest batches that reach each of its
row-tile counts, on the shapes where its layer seams, guarded loads and tile loop can go wrong.

Rows (pick_rows / launch_train): 8 193 is the smallest net-split launch (R = 1, the last tile holds one row), 16 400 takes R = 2
with a ragged last workgroup, 32 784 is the smallest batch that takes R = 4, ragged as well.  Shapes: d 16 with and without a
condition (full vector loads), (14, 3) and (10, 4) (guarded scalar loads, padded features and conditions), hidden 128 and 72 (a
padded last hidden tile: an odd number of tiles per net), L = 3 with both alternating mask patterns (both mask parities run, the
layer count is odd), tanh and relu, forward GEMM1 in f32 and in split bf16.

The axes are crossed by a covering design, not a full product (3 x 4 x 2 x 2 x 2 x 2 = 192 launches would not keep the suite
quick): every row count meets every (d, c), and over the (rows, shape) grid hidden size, mask pattern and activation rotate so
that each value of each axis meets each row count and each (d, c) at least once; every case runs in both precisions against one
shared reference.  The flagship's own combination (d 16, c 4, hidden 128, tanh) runs at all three row counts with both patterns.

Each case checks loss and flat gradient against the float64 oracle under tests/parity.py's bar (4 x the float32 oracle's own error
on the same rows, floor 4 ulp), asserts the dispatched kernel, and runs twice for equal bits.  The float32 reference is Oracle(32)
as it stands, one call over the batch.  (A float32 restatement that adds 1 024-row blocks on a thread pool was tried first, for
speed: its error, 8.7e-8 on a gradient of magnitude 1.3, left only the 4-ulp floor, and one case, n16400-R2-d16-c0-h128-alt2-relu-f32,
read 6.65e-7 against 6.15e-7.  The kernel's arithmetic is the parent commit's bit for bit.)  One case runs rnvp_fit_epoch over
two batches (32 784 + 8 200 rows: R = 4, then R = 1) against a loop of rnvp_train_step, bit for bit."""
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from parity import parity  # noqa: E402

pytestmark = pytest.mark.gpu

L = 3
ROWS = ((8193, 1), (16400, 2), (32784, 4))                       # (rows, row tiles per wave the host picks)
SHAPES = ((16, 4), (16, 0), (14, 3), (10, 4))                     # (d, cond)


def _cases():
    out = []
    for i, (n, R) in enumerate(ROWS):
        for j, (d, c) in enumerate(SHAPES):
            k = i * len(SHAPES) + j
            h = 128 if (i + j) % 2 == 0 else 72
            alt = 1 + (k // 2 + j) % 2
            act = "tanh" if (i + j // 2) % 2 == 0 else "relu"
            out.append((n, R, d, c, h, alt, act))
    # the benchmark's own combination at every row-tile count with both patterns, and the padded hidden tile with relu at R = 4
    for n, R in ROWS:
        for alt in (1, 2):
            out.append((n, R, 16, 4, 128, alt, "tanh"))
    out.append((32784, 4, 16, 4, 72, 2, "relu"))
    out.append((32784, 4, 10, 4, 72, 1, "relu"))
    seen, uniq = set(), []
    for t in out:
        if t not in seen:
            seen.add(t); uniq.append(t)
    return uniq


CASES = _cases()


def _id(t):
    return "n%d-R%d-d%d-c%d-h%d-alt%d-%s" % t


def _dev(a, dtype=torch.float32):
    return None if a is None else torch.tensor(np.ascontiguousarray(a)).to(dtype).cuda().contiguous()


def _threads():
    try:
        from probaforms_amd._engine import effective_cpus
        return max(1, min(effective_cpus(), 16))
    except Exception:  # pragma: no cover
        return max(1, min((os.cpu_count() or 2) // 2, 16))


def _oracle64_loss_grad(s, params, masks, X, C, inv_B, block=1024):
    """float64 loss and gradient: row blocks on a thread pool (ctypes releases the GIL), added in float64 in block order"""
    from oracle import Oracle
    o = Oracle(64)
    p = params.astype(np.float64)
    n = X.shape[0]
    cuts = [(a, min(a + block, n)) for a in range(0, n, block)]

    def one(ab):
        a, b = ab
        lo, g = o.loss_grad(s, p, X[a:b].astype(np.float64), None if C is None else C[a:b].astype(np.float64), masks=masks, inv_B=inv_B)
        return float(lo), np.asarray(g, np.float64)
    with ThreadPoolExecutor(_threads()) as ex:
        parts = list(ex.map(one, cuts))
    return sum(p[0] for p in parts), np.sum([p[1] for p in parts], axis=0)


def _oracle32_loss_grad(s, params, masks, X, C, inv_B):
    """the float32 oracle as it stands: one call over the batch, its own row-by-row accumulation"""
    from oracle import Oracle
    lo, g = Oracle(32).loss_grad(s, params, X, C, masks=masks, inv_B=inv_B)
    return float(lo), np.asarray(g, np.float32)


# ReLU's derivative jumps at 0, so a pre-activation that float32 cannot tell from 0 turns a unit's whole gradient share on or off
# with the summation order: no bar derived from a float32 restatement's error holds there (seen with unscreened rows: one
# pre-activation of 1.5e-9 among 14 M, gradient error 1.6e-5 against a bar of 9.5e-7, the float32 oracle unaffected).  The relu
# cases therefore draw rows whose float64 pre-activations all keep KINK away from 0.  A pre-activation is a sum of at most 20
# products with sum |x w| <= 20 (|x| <= 6.5, |w| <= 0.157) plus the error carried in from the layers before: float32 is off by
# less than 20 * 2^-24 * 20 = 2.4e-5 however it orders the sum; KINK is four times that.  Tanh cases need and get no screening.
KINK = 1e-4


def _near_kink(params, X, C, masks, d, c, h):
    """float64 forward in numpy (the oracle's arithmetic, realnvp.py:91-101): rows with a first-Linear output within KINK of 0"""
    p = params.astype(np.float64); x = X.astype(np.float64); off = 0
    bad = np.zeros(x.shape[0], bool)
    for l in range(masks.shape[0]):
        m = masks[l].astype(np.float64)
        inp = x * m if C is None else np.concatenate([x * m, C.astype(np.float64)], 1)
        out = []
        for _ in range(2):                                  # nn_t, then nn_s
            W1 = p[off:off + h * (d + c)].reshape(h, d + c); off += h * (d + c)
            b1 = p[off:off + h]; off += h
            W2 = p[off:off + d * h].reshape(d, h); off += d * h
            b2 = p[off:off + d]; off += d
            pre = inp @ W1.T + b1
            bad |= (np.abs(pre) < KINK).any(axis=1)
            out.append(np.maximum(pre, 0) @ W2.T + b2)
        x = (x * np.exp(out[1]) + out[0]) * (1 - m) + x * m
    return bad


_PROBLEMS = {}


def _problem(case):
    """inputs and the two references of a case, computed once and shared by its precisions; read-only afterwards"""
    if case in _PROBLEMS:
        return _PROBLEMS[case]
    from oracle import Shape
    n, R, d, c, h, alt, act = case
    rng = np.random.default_rng(7000 + n + 31 * d + 7 * c + h + alt)
    s = Shape.make(L, d, c, (h,), act)
    P = 2 * L * (h * (d + c) + h + d * h + d)
    params = (rng.uniform(-1, 1, size=P) * min(0.5, 1.5 / np.sqrt(h + d + c))).astype(np.float32)
    N = n + 61                                  # rows are gathered through a permutation of a larger table, as fit's batches are
    Xall = rng.standard_normal((N, d)).astype(np.float32)
    Call = rng.standard_normal((N, c)).astype(np.float32) if c else None
    idx = rng.permutation(N)[:n].astype(np.int64)
    masks = ((np.arange(d)[None, :] + np.arange(L)[:, None] + (alt - 1)) % 2).astype(np.uint8)
    while act == "relu":                        # redraw the rows that sit on a ReLU kink (KINK above)
        bad = _near_kink(params, Xall[idx], None if Call is None else Call[idx], masks, d, c, h)
        if not bad.any():
            break
        Xall[idx[bad]] = rng.standard_normal((int(bad.sum()), d)).astype(np.float32)
        if Call is not None:
            Call[idx[bad]] = rng.standard_normal((int(bad.sum()), c)).astype(np.float32)
    X, C = Xall[idx], (None if Call is None else Call[idx])
    l64, g64 = _oracle64_loss_grad(s, params, masks, X, C, 1.0 / n)
    l32, g32 = _oracle32_loss_grad(s, params, masks, X, C, 1.0 / n)
    for a in (params, Xall, idx, g32, g64) + (() if Call is None else (Call,)):
        a.setflags(write=False)
    _PROBLEMS[case] = (params, Xall, Call, idx, (l32, g32), (l64, g64))
    return _PROBLEMS[case]


@pytest.mark.parametrize("prec", ["f32", "bx3"])
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_netsplit_step_matches_float64_and_repeats_bitwise(case, prec):
    from probaforms_amd import _hip
    n, R, d, c, h, alt, act = case
    params, Xall, Call, idx, (l32, g32), (l64, g64) = _problem(case)
    shape = _hip.RnvpShape.make(L, d, c, (h,), act, alt_masks=alt, precision=prec)
    P = _hip.param_count(shape)
    assert P == params.size
    ws = torch.empty(_hip.workspace_bytes(shape, _hip.OP_TRAIN, n), dtype=torch.uint8, device="cuda")
    pd, xd, cd, id_ = _dev(params), _dev(Xall), _dev(Call), _dev(idx, torch.int64)
    outs = []
    for _ in range(2):
        grad = torch.full((P,), float("nan"), device="cuda"); loss = torch.full((1,), float("nan"), device="cuda")
        _hip.loss_grad(shape, pd, None, xd, cd, id_, n, 1.0 / n, grad, loss, ws)
        torch.cuda.synchronize()
        outs.append((grad.clone(), loss.clone()))
    got = _hip.last_dispatch(_hip.PROFILE_TRAIN)
    assert (got["kernel"], got["variant"], got["row_tiles"], got["gemm1_fwd"], got["rows"]) == ("k_mfma_train", "netsplit", R, prec, n), got
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])      # no float atomics: same bits
    cid = _id(case) + "-" + prec
    parity(cid, "grad", outs[0][0].cpu().numpy(), ref32=g32, ref64=g64)
    parity(cid, "loss", float(outs[0][1].item()), ref32=l32, ref64=l64)


def test_fit_epoch_over_r4_and_r1_batches_equals_the_step_loop_bitwise():
    """one rnvp_fit_epoch call over a 32 784-row batch (R = 4) and the 8 200-row rest (R = 1) against rnvp_train_step per batch"""
    from probaforms_amd import _hip
    d, c, h, batch, n = 16, 4, 128, 32784, 32784 + 8200
    shape = _hip.RnvpShape.make(L, d, c, (h,), "tanh", alt_masks=1)
    P = _hip.param_count(shape)
    gen = torch.Generator(device="cuda").manual_seed(4242)
    p0 = (torch.rand(P, device="cuda", generator=gen) - 0.5) * min(0.6, 3.0 / np.sqrt(h + d + c))
    x = torch.randn(n, d, device="cuda", generator=gen)
    cc = torch.randn(n, c, device="cuda", generator=gen)
    perm = torch.randperm(n, device="cuda", generator=gen)
    ws = torch.empty(_hip.workspace_bytes(shape, _hip.OP_TRAIN, batch), dtype=torch.uint8, device="cuda")
    nb = 2
    pa = p0.clone(); ma = torch.zeros(P, device="cuda"); va = torch.zeros(P, device="cuda"); ga = torch.empty(P, device="cuda")
    la = torch.zeros(nb, device="cuda")
    _hip.fit_epoch(shape, pa, None, x, cc, perm, n, batch, ga, la, ma, va, 1e-3, 0.9, 0.999, 1e-8, 0.01, 1, ws)
    got = _hip.last_dispatch(_hip.PROFILE_TRAIN)
    assert (got["kernel"], got["variant"], got["row_tiles"], got["rows"]) == ("k_mfma_train", "netsplit", 1, 8200), got
    pb = p0.clone(); mb = torch.zeros(P, device="cuda"); vb = torch.zeros(P, device="cuda"); gb = torch.empty(P, device="cuda")
    lb = torch.zeros(nb, device="cuda")
    tiles = []
    for k in range(nb):
        lo = k * batch; rows = min(batch, n - lo)
        _hip.train_step(shape, pb, None, x, cc, perm[lo:lo + rows].contiguous(), rows, 1.0 / rows, gb, lb[k:k + 1], mb, vb,
                        1e-3, 0.9, 0.999, 1e-8, 0.01, k + 1, ws)
        tiles.append(_hip.last_dispatch(_hip.PROFILE_TRAIN)["row_tiles"])
    torch.cuda.synchronize()
    assert tiles == [4, 1]
    assert torch.isfinite(la).all() and torch.isfinite(pa).all()
    assert torch.equal(la, lb) and torch.equal(pa, pb) and torch.equal(ma, mb) and torch.equal(va, vb)
    assert not torch.equal(pa, p0)
