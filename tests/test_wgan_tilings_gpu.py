"""libpf_wgan.so at the tile sizes the host can pick but the fixtures never reach (tests/tilings_cases.py): step tiles of
1..128 rows, a critic step whose 2R = 256 LDS rows use every thread, R = cap with an odd LDS stride, more than 256 workgroups,
launches above 64 KiB of LDS up to the last shape that fits, inference and epoch-loss tiles of 1..18 rows with n on either
side of a tile multiple, and pfw_fit_epoch whose ragged last batch picks a smaller tile than the workspace was sized for.

Every case first asserts its regime through pfw_tiling, runs on a workspace of exactly pfw_workspace_bytes() filled with 0xFF
and on poisoned outputs, and is compared with the float64 restatement (tests/wgan_torch.py) under the measured bar of
tests/parity.py: 4 times the float32 restatement's own error (for the long chains of tilings_cases.LONG_FAN_IN
the larger of torch's and the kernel-order float32 restatement's), at least 4 float32 ulp of the quantity's magnitude.  The
magnitude is max |float64 value|; that of a gradient is max(|g|, grad_scale) as in tests/test_wgan_gpu.py (a critic step's
two means cancel), and one loss (tilings_cases.TERMS_MAGNITUDE, with its figures) takes the terms of D's last Linear.
profiles/r11_tilings_parity.txt holds the REGIME and PARITY lines of one run.  Bitwise claims have no tolerance."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import hygiene  # noqa: E402
import native_libs  # noqa: E402
import tilings_cases as tc  # noqa: E402
import wgan_torch as wt  # noqa: E402
from parity import parity  # noqa: E402
from probaforms_amd.models import _wgan_lib as W  # noqa: E402

pytestmark = pytest.mark.gpu

native_libs.ensure_built(W)

DEV = torch.device("cuda")
F32, F64 = torch.float32, torch.float64
BIG_LDS = 64 * 1024


def dev(a, dtype=torch.float32):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def nets(name):
    sh, ga, da = tc.W_SHAPES[name]
    return W.Shape.make(*sh, ga, da), wt.Wgan(*sh, ga, da)


def step_refs(case, p, X, C, ri, z, kind, what=None):
    """CPU only: the float64 and float32 restatements of one step and the magnitudes of its bars, as keyword arguments of
    parity() for the gradient and for the loss.  Long chains add the kernel-order float32 restatement (tilings_cases)"""
    name, rows, R = case[:3]
    sh, ga, da = tc.W_SHAPES[name]
    wg = wt.Wgan(*sh, ga, da)
    l64, g64 = wg.loss_grad(p, X, C, ri, z, kind)
    l32, g32 = wg.loss_grad(p, X, C, ri, z, kind, F32)
    lo, go = None, None
    if tc.w_long(name):
        seq = wt.Wgan(*sh, ga, da, sequential=True)
        lo, go = tc.ordered32(lambda s, e: seq.loss_grad(p, X, C, ri[s:e], z[s:e], kind, F32), rows, R)
    return (dict(ref32=g32, ref64=g64, magnitude=max(np.abs(g64).max(), wg.grad_scale(p, X, C, ri, z, kind)), also32=go),
            dict(ref32=l32, ref64=l64, also32=lo,
                 magnitude=loss_magnitude(wg, p, X, C, ri, z, kind, l64) if (tc.step_id(case), what) in tc.TERMS_MAGNITUDE else None))


def inference_refs(name, entry, p, X, C, Z):
    """CPU only: parity()'s keyword arguments for one inference entry point"""
    sh, ga, da = tc.W_SHAPES[name]
    wg, seq = wt.Wgan(*sh, ga, da), wt.Wgan(*sh, ga, da, sequential=True) if tc.w_long(name) else None
    if entry == "generate":
        f = lambda m, dt: m.generate(p, Z, C, dt)
    elif entry == "critic":
        f = lambda m, dt: m.critic(p, X, C, dt)[:, 0]
    else:
        f = lambda m, dt: np.array(m.epoch_losses(p, X, C, Z, dt))
    return dict(ref32=f(wg, F32), ref64=f(wg, F64), also32=None if seq is None else f(seq, F32))


def regime(case):
    """assert the step regime the case was written for; returns the shape and the restatement"""
    name, rows, R, cap, G, lds = case
    shape, wg = nets(name)
    t = W.tiling(shape, rows)
    print("REGIME wgan %-14s R %3d cap %3d G %3d lds %6d (%s 64 KiB) bound %d" % (
        tc.step_id(case), t.step_tile, t.step_cap, t.step_wgs, t.step_lds_bytes, ">" if t.step_lds_bytes > BIG_LDS else "<=",
        t.step_wg_bound))
    assert (t.step_tile, t.step_cap, t.step_wgs, t.step_lds_bytes) == (R, cap, G, lds)
    assert G <= t.step_wg_bound
    return shape, wg


def d_terms(wg, p, x, c):
    """per row: |b| + sum_i |h_i w_i| over the terms of D's last Linear (float64), the magnitude a float32 D(row) is
    rounded against"""
    layers = wg.D.split(torch.tensor(np.asarray(p[wg.PG:wg.PG + wg.PD], np.float64)))
    h = wg._cat(torch.tensor(np.asarray(x), dtype=F64), None if c is None else torch.tensor(np.asarray(c), dtype=F64))
    for Wk, bk in layers[:-1]:
        h = h @ Wk.T + bk
        h = torch.tanh(h) if wg.D.act == 'tanh' else torch.relu(h)
    Wl, bl = layers[-1]
    return ((h * Wl[0]).abs().sum(1) + bl.abs()).numpy()


def loss_magnitude(wg, p, X, C, ri, z, kind, l64):
    """mean d_terms over the fake rows and, on a critic step, the real rows (tilings_cases.TERMS_MAGNITUDE only)"""
    c = None if C is None else C[ri]
    m = d_terms(wg, p, wg.generate(p, z, c), c).mean()
    if kind == W.STEP_CRITIC:
        m = max(m, d_terms(wg, p, X[ri], c).mean())
    return max(m, abs(l64))


def gpu_loss_grad(shape, wg, kind, pd, Xd, Cd, rid, zd, rows, ws, grad=True, loss=True):
    g = torch.empty(wg.PD if kind == W.STEP_CRITIC else wg.PG, device=DEV) if grad else None
    l = torch.empty(1, device=DEV) if loss else None
    hygiene.poison_outputs(g, l)
    W.loss_grad(shape, kind, pd, Xd, Cd, rid, zd, rows, g, l, ws)
    torch.cuda.synchronize()
    hygiene.assert_all_written({k: v for k, v in (("grad", g), ("loss", l)) if v is not None}, "pfw_loss_grad")
    return g, l


@pytest.mark.parametrize("case", tc.W_STEPS, ids=tc.step_id)
def test_step_matches_float64_at_every_tile(case):
    name, rows, R = case[:3]
    shape, wg = regime(case)
    p, X, C, ri, z = tc.wgan_problem(name, rows, R)
    pd, Xd, Cd, rid, zd = dev(p), dev(X), dev(C), dev(ri, torch.int64), dev(z)
    ws = hygiene.workspace(W.workspace_bytes(shape, rows), "ones")
    got = {}
    for kind in (W.STEP_CRITIC, W.STEP_GEN):
        g, l = gpu_loss_grad(shape, wg, kind, pd, Xd, Cd, rid, zd, rows, ws)
        got[kind] = g
        what = "critic" if kind == W.STEP_CRITIC else "gen"
        gref, lref = step_refs(case, p, X, C, ri, z, kind, what + " loss")
        parity(tc.step_id(case), what + " grad", g.cpu().numpy(), **gref)
        parity(tc.step_id(case), what + " loss", float(l), **lref)
    # one pfw_train_step: the same gradient bit for bit, RMSprop and the clamp to the ulp (tests/test_wgan_gpu.py's check)
    kind = W.STEP_CRITIC if tc.W_STEPS.index(case) % 2 == 0 else W.STEP_GEN
    rng = np.random.default_rng(rows)
    v0 = rng.uniform(0, 1e-3, size=p.size).astype(np.float32)
    p1, v1 = dev(p), dev(v0)
    g = torch.empty_like(got[kind])
    l = torch.empty(1, device=DEV)
    hygiene.poison_outputs(g, l)
    W.train_step(shape, kind, p1, v1, Xd, Cd, rid, zd, rows, W.rmsprop(1e-3, weight_decay=0.001, clamp=0.01), g, l, ws)
    torch.cuda.synchronize()
    hygiene.assert_all_written(dict(grad=g, loss=l), "pfw_train_step")
    assert hygiene.same_bits(g, got[kind])
    sl = slice(wg.PG, wg.PG + wg.PD) if kind == W.STEP_CRITIC else slice(0, wg.PG)
    other = slice(0, wg.PG) if kind == W.STEP_CRITIC else slice(wg.PG, wg.PG + wg.PD)
    pr, vr = wt.rmsprop_f32(p[sl], g.cpu().numpy(), v0[sl], 1e-3, wd=0.001, clamp=0.01 if kind == W.STEP_CRITIC else 0.0)
    p1, v1 = p1.cpu().numpy(), v1.cpu().numpy()
    assert (np.abs(p1[sl] - pr) <= np.spacing(np.abs(pr))).all() and (np.abs(v1[sl] - vr) <= np.spacing(np.abs(vr))).all()
    assert np.array_equal(p1[other], p[other]) and np.array_equal(v1[other], v0[other])       # only the stepped net moves


INDEX_CASES = [c for c in tc.W_STEPS if tc.step_id(c) in ("full_wg-4097", "big_lds-33", "cap2-5")]


@pytest.mark.parametrize("case", INDEX_CASES, ids=tc.step_id)
def test_row_index_none_arange_and_gather_give_the_same_bits(case):
    name, rows, R = case[:3]
    shape, wg = regime(case)
    p, X, C, ri, z = tc.wgan_problem(name, rows, R)
    pd, zd = dev(p), dev(z)
    Xg, Cg = dev(X[ri]), dev(None if C is None else C[ri])
    ws = hygiene.workspace(W.workspace_bytes(shape, rows), "ones")
    for kind in (W.STEP_CRITIC, W.STEP_GEN):
        a = gpu_loss_grad(shape, wg, kind, pd, dev(X), dev(C), dev(ri, torch.int64), zd, rows, ws)
        b = gpu_loss_grad(shape, wg, kind, pd, Xg, Cg, None, zd, rows, ws)
        c = gpu_loss_grad(shape, wg, kind, pd, Xg, Cg, torch.arange(rows, device=DEV), zd, rows, ws)
        for u, v in zip(a + a, b + c):
            assert hygiene.same_bits(u, v)
        # one output at a time: the other keeps its bits
        g_only = gpu_loss_grad(shape, wg, kind, pd, Xg, Cg, None, zd, rows, ws, loss=False)[0]
        l_only = gpu_loss_grad(shape, wg, kind, pd, Xg, Cg, None, zd, rows, ws, grad=False)[1]
        assert hygiene.same_bits(g_only, b[0]) and hygiene.same_bits(l_only, b[1])


@pytest.mark.parametrize("case", INDEX_CASES, ids=tc.step_id)
def test_row_index_with_repeats_and_gaps(case):
    name, rows, R = case[:3]
    shape, wg = regime(case)
    p, X, C, _, z = tc.wgan_problem(name, rows, R)
    ri = np.random.default_rng(rows).integers(0, X.shape[0] // 2, size=rows) * 2        # even table rows only, many twice
    assert len(np.unique(ri)) < rows and len(ri) == rows
    ws = hygiene.workspace(W.workspace_bytes(shape, rows), "ones")
    for kind in (W.STEP_CRITIC, W.STEP_GEN):
        g, l = gpu_loss_grad(shape, wg, kind, dev(p), dev(X), dev(C), dev(ri, torch.int64), dev(z), rows, ws)
        gref, lref = step_refs(case, p, X, C, ri, z, kind)
        parity(tc.step_id(case), "repeats grad %d" % kind, g.cpu().numpy(), **gref)
        parity(tc.step_id(case), "repeats loss %d" % kind, float(l), **lref)


# (shape name, entry point, the tile the host must pick); every one of these launches asks for more than 64 KiB of LDS
INFERENCE = [("cap2", "generate", 18), ("cap2", "critic", 18), ("cap2", "epoch_losses", 4),
             ("cap1", "generate", 8), ("cap1", "critic", 18), ("cap1", "epoch_losses", 2),
             ("gen_only", "generate", 1)]


@pytest.mark.parametrize("name,entry,tile", INFERENCE, ids=["%s-%s" % c[:2] for c in INFERENCE])
def test_inference_tiles_on_both_sides_of_a_multiple(name, entry, tile):
    shape, wg = nets(name)
    (d, c, lat, _, _), _, _ = tc.W_SHAPES[name]
    p = tc.wgan_problem(name, 1, 1)[0]
    pd = dev(p)
    rng = np.random.default_rng(tile)
    for n in (tile - 1, tile, tile + 1, 2 * tile + 1):
        if n < 1:
            continue
        t = W.tiling(shape, n, require_step=False)
        have, lds = {"generate": (t.gen_tile, t.gen_lds_bytes), "critic": (t.crit_tile, t.crit_lds_bytes),
                     "epoch_losses": (t.eloss_tile, t.eloss_lds_bytes)}[entry]
        print("REGIME wgan %-14s %-12s n %3d tile %2d lds %6d" % (name, entry, n, have, lds))
        assert have == tile and BIG_LDS < lds <= 160 * 1024
        X = rng.normal(size=(n, d)).astype(np.float32)
        C = rng.normal(size=(n, c)).astype(np.float32) if c else None
        Z = rng.normal(size=(n, lat)).astype(np.float32)
        case = "%s n=%d" % (name, n)
        if entry == "generate":
            out = torch.empty(n, d, device=DEV)
            hygiene.poison_outputs(out)
            W.generate(shape, pd, dev(Z), dev(C), n, out)
        elif entry == "critic":
            out = torch.empty(n, device=DEV)
            hygiene.poison_outputs(out)
            W.critic(shape, pd, dev(X), dev(C), n, out)
        else:
            out = torch.empty(2, device=DEV)
            hygiene.poison_outputs(out)
            ws = hygiene.workspace(W.workspace_bytes(shape, 0, n), "ones")
            W.epoch_losses(shape, pd, dev(X), dev(C), dev(Z), n, out, ws)
        torch.cuda.synchronize()
        hygiene.assert_all_written(dict(out=out), "pfw_%s" % entry)
        parity(case, entry, out.cpu().numpy(), **inference_refs(name, entry, p, X, C, Z))


# (shape name, n, batch size, (R, G) of the full batch, (R, G) of the ragged last batch)
EPOCHS = [("cap13", 2049 + 2048, 2049, (13, 158), (8, 256)), ("cap2", 5, 3, (2, 2), (2, 1))]


@pytest.mark.parametrize("name,n,B,full,last", EPOCHS, ids=[c[0] for c in EPOCHS])
def test_fit_epoch_with_a_smaller_last_tile_equals_the_step_loop_bitwise(name, n, B, full, last):
    shape, wg = nets(name)
    (d, c, lat, _, _), _, _ = tc.W_SHAPES[name]
    tf, tl = W.tiling(shape, B), W.tiling(shape, n - B)
    print("REGIME wgan %-14s fit_epoch: batch %d R %d G %d, last batch %d R %d G %d, bound %d" % (
        name, B, tf.step_tile, tf.step_wgs, n - B, tl.step_tile, tl.step_wgs, tf.step_wg_bound))
    assert (tf.step_tile, tf.step_wgs) == full and (tl.step_tile, tl.step_wgs) == last
    assert max(tf.step_wgs, tl.step_wgs) <= tf.step_wg_bound
    p, X, C, _, z = tc.wgan_problem(name, n - 3, 8)
    rng = np.random.default_rng(n)
    X, C = X[:n], C[:n]
    z = rng.normal(size=(n, lat)).astype(np.float32)
    Xd, Cd, zd, zf = dev(X), dev(C), dev(z), dev(rng.normal(size=(n, lat)))
    perm = dev(rng.permutation(n), torch.int64)
    kinds = np.array([W.STEP_CRITIC, W.STEP_GEN], np.int8)
    opt = W.rmsprop(1e-3, weight_decay=0.001, clamp=0.01)
    v0 = rng.uniform(0, 1e-3, size=p.size).astype(np.float32)
    p1, v1, p2, v2 = dev(p), dev(v0), dev(p), dev(v0)
    e1, e2 = torch.empty(2, device=DEV), torch.empty(2, device=DEV)
    hygiene.poison_outputs(e1, e2)
    W.fit_epoch(shape, p1, v1, Xd, Cd, perm, zd, zf, n, B, kinds, opt, e1, hygiene.workspace(W.workspace_bytes(shape, B, n), "ones"))
    for b, s in enumerate(range(0, n, B)):
        e = min(n, s + B)
        W.train_step(shape, int(kinds[b]), p2, v2, Xd, Cd, perm[s:e], zd[s:e], e - s, opt, None, None,
                     hygiene.workspace(W.workspace_bytes(shape, e - s), "ones"))
    W.epoch_losses(shape, p2, Xd, Cd, zf, n, e2, hygiene.workspace(W.workspace_bytes(shape, 0, n), "ones"))
    torch.cuda.synchronize()
    hygiene.assert_all_written(dict(params=p1, square_avg=v1, epoch_losses=e1), "pfw_fit_epoch")
    assert hygiene.same_bits(p1, p2) and hygiene.same_bits(v1, v2) and hygiene.same_bits(e1, e2)
    assert not hygiene.same_bits(p1, dev(p))
