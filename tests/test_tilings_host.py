"""The host side of the row tiling of libpf_wgan.so and libpf_cnormal.so, no GPU: what pfw_tiling / pfn_tiling report -- the
values the launches use -- over shapes at every kind of step cap and batches at every hand-over between tiles; the workspace
against the grid; the last shape that fits LDS and the first that does not; and that the large GPU cases of
tests/tilings_cases.py can see a single dropped row."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import cnormal_torch as ct  # noqa: E402
import native_libs  # noqa: E402
import tilings_cases as tc  # noqa: E402
import wgan_torch as wt  # noqa: E402
from parity import bound  # noqa: E402
from probaforms_amd.models import _cnormal_lib as N  # noqa: E402
from probaforms_amd.models import _wgan_lib as W  # noqa: E402

native_libs.ensure_built(W, N)

LDS = 160 * 1024
MAX_ROWS = 40000


def w_shape(d, c, lat, gh, dh, ga='relu', da='relu'):
    return W.Shape.make(d, c, lat, gh, dh, ga, da)


# (shape, step cap): caps of 1, 2..7, 8, 9..15 (no power of two), 111 and the thread bound
W_SWEEP = [(w_shape(5, 3, 1, (h, h), (h, h)), cap) for h, cap in ((1500, 1), (1024, 2), (512, 5), (370, 7), (320, 8), (256, 10))]
W_SWEEP += [(w_shape(*tc.W_SHAPES[k][0]), cap) for k, cap in (("cap13", 13), ("odd_cap", 111), ("full_wg", 128), ("last", 1))]
N_SWEEP = [(N.Shape.make(8, c, (16,), 'relu', False), cap)
           for c, cap in ((20000, 1), (13000, 2), (9000, 3), (6000, 5), (5000, 7), (4400, 8), (3800, 9), (3200, 11), (2400, 15),
                          (300, 107), (242, 128))]
N_SWEEP += [(N.Shape.make(*tc.N_SHAPES[k]), cap) for k, cap in (("full_wg", 256), ("big_lds", 15), ("cap3", 3), ("last", 1))]


def sweep_rows(cap):
    """1..MAX_ROWS at every 2^k 256 +- 1 hand-over between power-of-two tiles and at cap m +- 1, plus the small batches"""
    rows = set(range(1, 70))
    for k in range(3, 9):
        rows.update(((1 << k) * 256 - 1, (1 << k) * 256, (1 << k) * 256 + 1))
    for m in list(range(1, 40)) + [255, 256, 257, 300, 511, 512, 513] + list(range(MAX_ROWS // cap - 2, MAX_ROWS // cap + 1)):
        rows.update((cap * m - 1, cap * m, cap * m + 1))
    return sorted(r for r in rows if 1 <= r <= MAX_ROWS)


def all_wgs(lib, shape):
    """G(r) for every r in 1..MAX_ROWS (index r; index 0 unused)"""
    g = np.zeros(MAX_ROWS + 1, np.int64)
    for r in range(1, MAX_ROWS + 1):
        g[r] = lib.tiling(shape, r).step_wgs
    return g


@pytest.mark.parametrize("k", range(len(W_SWEEP)))
def test_wgan_step_tiling_over_caps_and_batches(k):
    shape, cap = W_SWEEP[k]
    P = W.param_count(shape, W.NET_G) + W.param_count(shape, W.NET_D)
    worst = np.maximum.accumulate(all_wgs(W, shape))          # worst[rows] = max over r <= rows of G(r)
    tiles = set()
    for rows in sweep_rows(cap):
        t = W.tiling(shape, rows)
        R, G = t.step_tile, t.step_wgs
        assert t.step_cap == cap and 1 <= R <= cap and 2 * R <= 256
        assert G == -(-rows // R)
        assert worst[rows] <= t.step_wg_bound, (rows, worst[rows], t.step_wg_bound)      # pfw_fit_epoch's ragged last batch
        assert W.workspace_bytes(shape, rows) >= t.step_wg_bound * P * 4 + t.step_wg_bound * 4
        assert t.step_wg_bound >= G
        assert t.step_lds_bytes <= LDS
        tiles.add(R)
    want = {min(cap, r) for r in (8, 16, 32, 64, 128)}
    assert tiles == want, (tiles, want)                       # the sweep reached every tile the host can pick


@pytest.mark.parametrize("k", range(len(N_SWEEP)))
def test_cnormal_step_tiling_over_caps_and_batches(k):
    shape, cap = N_SWEEP[k]
    P = N.param_count(shape)
    worst = np.maximum.accumulate(all_wgs(N, shape))
    tiles = set()
    for rows in sweep_rows(cap):
        t = N.tiling(shape, rows)
        R, G = t.step_tile, t.step_wgs
        assert t.step_cap == cap and 1 <= R <= cap <= 256
        assert G == -(-rows // R)
        assert worst[rows] <= t.step_wg_bound, (rows, worst[rows], t.step_wg_bound)      # pfn_fit_epoch's ragged last batch
        # the partials, the per-workgroup losses, M = out.weight^-1 and the two error words
        assert N.workspace_bytes(shape, rows) >= t.step_wg_bound * P * 4 + t.step_wg_bound * 4 + N.MAX_D * N.MAX_D * 4 + 8
        assert t.step_wg_bound >= G
        assert t.step_lds_bytes <= LDS
        tiles.add(R)
    want = {min(cap, r) for r in (8, 16, 32, 64, 128, 256)}
    assert tiles == want, (tiles, want)


def test_tiling_refuses_bad_arguments_and_launches_nothing():
    info_w, info_n = W.TilingInfo(), N.TilingInfo()
    sw, sn = w_shape(5, 3, 1, (10,), (10,)), N.Shape.make(5, 3, (10,), 'tanh', False)
    L, M = W.lib(), N.lib()
    assert L.pfw_tiling(ctypes.byref(sw), 0, ctypes.byref(info_w)) == -1 and L.pfw_tiling(ctypes.byref(sw), 4, None) == -1
    assert M.pfn_tiling(ctypes.byref(sn), 0, ctypes.byref(info_n)) == -1 and M.pfn_tiling(ctypes.byref(sn), 4, None) == -1
    assert L.pfw_tiling(None, 4, ctypes.byref(info_w)) == -1 and M.pfn_tiling(None, 4, ctypes.byref(info_n)) == -1
    sw.latent = 0
    sn.c = 0
    assert L.pfw_tiling(ctypes.byref(sw), 4, ctypes.byref(info_w)) == -1
    assert M.pfn_tiling(ctypes.byref(sn), 4, ctypes.byref(info_n)) == -1
    # d beyond PFN_MAX_D: neither the step nor the forward can run
    assert M.pfn_tiling(ctypes.byref(N.Shape.make(N.MAX_D + 1, 3, (10,), 'tanh', False)), 4, ctypes.byref(info_n)) == N.EUNSUPPORTED
    assert (info_n.step_tile, info_n.fwd_tile) == (0, 0)


def test_wgan_last_supported_shape_and_the_first_refused():
    fake = ctypes.c_void_p(256)                                          # never dereferenced: the call returns before
    ok, over = w_shape(1, 0, 1, (3412,), (1,)), w_shape(1, 0, 1, (3413,), (1,))
    t = W.tiling(ok, 2)
    assert (t.step_cap, t.step_tile, t.step_wgs, t.step_lds_bytes) == (1, 1, 2, 163824)
    assert W.workspace_bytes(ok, 2) >= 2 * (W.param_count(ok, W.NET_G) + W.param_count(ok, W.NET_D) + 1) * 4
    st = W.lib().pfw_loss_grad(None, ctypes.byref(over), W.STEP_CRITIC, fake, fake, fake, None, fake, 2, None, None, fake, 1 << 30)
    assert st == W.EUNSUPPORTED
    with pytest.raises(RuntimeError, match="unsupported"):
        W.tiling(over, 2)
    t = W.tiling(over, 2, require_step=False)          # inference still runs: its fields are filled
    assert (t.step_cap, t.step_tile, t.step_wgs, t.step_lds_bytes, t.step_wg_bound) == (0, 0, 0, 0, 0)
    assert t.gen_tile >= 1 and t.crit_tile == 64 and t.eloss_tile >= 1 and t.gen_lds_bytes <= LDS
    assert W.workspace_bytes(over, 2) == 0             # as before: no step workgroups, nothing to hold
    # pfw_generate alone at a tile of one row
    t = W.tiling(w_shape(*tc.W_SHAPES["gen_only"][0]), 3, require_step=False)
    assert (t.step_cap, t.eloss_tile, t.gen_tile, t.crit_tile) == (0, 0, 1, 64) and 65536 < t.gen_lds_bytes <= LDS


def test_cnormal_last_supported_shape_and_the_first_refused():
    fake = ctypes.c_void_p(256)
    ok, over = N.Shape.make(1, 1, (6823,), 'relu', False), N.Shape.make(1, 1, (6824,), 'relu', False)
    t = N.tiling(ok, 2)
    assert (t.step_cap, t.step_tile, t.step_wgs) == (1, 1, 2) and 65536 < t.step_lds_bytes <= LDS
    assert N.workspace_bytes(ok, 2) > 2 * N.param_count(ok) * 4
    assert N.lib().pfn_loss_grad(None, ctypes.byref(over), fake, fake, fake, None, 2, fake, fake, fake, fake, 1 << 30) == N.EUNSUPPORTED
    assert N.workspace_bytes(over, 2) == 0
    with pytest.raises(RuntimeError, match="unsupported"):
        N.tiling(over, 2)
    t = N.tiling(over, 2, require_step=False)
    assert (t.step_cap, t.step_tile, t.step_wgs, t.step_lds_bytes, t.step_wg_bound) == (0, 0, 0, 0, 0) and t.fwd_tile >= 1


def test_gpu_cases_name_the_regime_the_host_picks():
    """the expectations of tests/tilings_cases.py hold here too, so a retuned host fails without a GPU"""
    for name, rows, R, cap, G, lds in tc.W_STEPS:
        sh, ga, da = tc.W_SHAPES[name]
        t = W.tiling(w_shape(*sh, ga, da), rows)
        assert (t.step_tile, t.step_cap, t.step_wgs, t.step_lds_bytes) == (R, cap, G, lds), (name, rows)
    for name, rows, R, cap, G, lds in tc.N_STEPS:
        t = N.tiling(N.Shape.make(*tc.N_SHAPES[name]), rows)
        assert (t.step_tile, t.step_cap, t.step_wgs, t.step_lds_bytes) == (R, cap, G, lds), (name, rows)
    assert {c[2] for c in tc.W_STEPS} >= {1, 2, 8, 13, 32, 64, 111, 128}
    assert {c[2] for c in tc.N_STEPS} >= {1, 3, 8, 15, 16, 32, 64, 128, 256}
    assert any(c[4] > 256 for c in tc.W_STEPS)


BIG_W = [c for c in tc.W_STEPS if c[1] >= tc.BIG]
BIG_N = [c for c in tc.N_STEPS if c[1] >= tc.BIG]


def test_every_large_case_is_covered():
    assert len(BIG_W) == 6 and len(BIG_N) == 6 and tc.BIG == 2049


def kink_distance(wg, p, X, C, ri, z):
    """the smallest |pre-activation| of any ReLU unit of G and of D (on the fake and on the real rows) in float64, and
    printed beside it the largest float32 error of a pre-activation: a unit closer to 0 than that can flip on the GPU"""
    c = None if C is None else torch.tensor(C[ri], dtype=torch.float64)
    best, worst = np.inf, 0.0

    def run(net, flat, x):
        nonlocal best, worst
        L64 = net.split(torch.tensor(np.asarray(flat, np.float64)))
        L32 = net.split(torch.tensor(np.asarray(flat, np.float32)))
        h32 = x.float()
        for (W6, b6), (W3, b3) in zip(L64[:-1], L32[:-1]):
            pre, pre32 = x @ W6.T + b6, h32 @ W3.T + b3
            best, worst = min(best, float(pre.abs().min())), max(worst, float((pre32.double() - pre).abs().median()))
            x, h32 = torch.relu(pre), torch.relu(pre32)
        return x @ L64[-1][0].T + L64[-1][1]

    cat = wg._cat
    fake = run(wg.G, p[:wg.PG], cat(torch.tensor(z, dtype=torch.float64), c))
    run(wg.D, p[wg.PG:], cat(fake, c))
    run(wg.D, p[wg.PG:], cat(torch.tensor(X[ri], dtype=torch.float64), c))
    print("KINK smallest |pre-activation| %.2e, median float32 error of one %.2e" % (best, worst))
    return best


@pytest.mark.parametrize("case", BIG_W, ids=tc.step_id)
def test_wgan_large_cases_see_a_dropped_edge_row(case):
    """Removing any one of the three edge rows from the batch (its term of the mean gone, as a kernel that skipped it would
    compute) moves the float64 gradient by at least 10 bars of the GPU test, in both step kinds.  The edge rows' inputs are
    scaled by tilings_cases.SCALE for exactly this; ReLU nets, so that a scaled input scales the row's gradient."""
    name, rows, R = case[:3]
    (d, c, lat, gh, dh), ga, da = tc.W_SHAPES[name]
    assert ga == da == 'relu'
    p, X, C, ri, z = tc.wgan_problem(name, rows, R)
    wg = wt.Wgan(d, c, lat, gh, dh, ga, da)
    assert kink_distance(wg, p, X, C, ri, z) >= tc.KINK
    for kind in (W.STEP_CRITIC, W.STEP_GEN):
        l64, g64 = wg.loss_grad(p, X, C, ri, z, kind)
        l32, g32 = wg.loss_grad(p, X, C, ri, z, kind, torch.float32)
        bar, e_ref = bound(g32, g64, max(np.abs(g64).max(), wg.grad_scale(p, X, C, ri, z, kind)))
        for r in tc.edge_rows(rows, R):
            _, g1 = wg.loss_grad(p, X, C, ri[r:r + 1], z[r:r + 1], kind)        # the row's own mean = its term times rows
            moved = np.abs(g1).max() / rows
            print("DROP wgan %-14s kind %d row %5d: gradient moves %.3e = %.1f bars (bar %.3e, e_ref %.3e)"
                  % (tc.step_id(case), kind, r, moved, moved / bar, bar, e_ref))
            assert moved >= 10 * bar


@pytest.mark.parametrize("case", BIG_N, ids=tc.step_id)
def test_cnormal_large_cases_see_a_dropped_edge_row(case):
    """as the WGAN test; x is what ConditionalNormal's loss sees of a row beside the net, whatever the activation"""
    name, rows, R = case[:3]
    d, c, hidden, act, indep = tc.N_SHAPES[name]
    p, X, C, ri = tc.cnormal_problem(name, rows, R)
    net = ct.Normal(d, c, hidden, act, indep)
    l64, g64 = net.loss_grad(p, X, C, ri)
    l32, g32 = net.loss_grad(p, X, C, ri, torch.float32)
    bar, e_ref = bound(g32, g64)
    if act == 'relu':                            # no trunk unit within float32 rounding of its kink (tilings_cases.KINK)
        h, near = torch.tensor(C[ri], dtype=torch.float64), np.inf
        for Wk, bk in net.split(torch.tensor(np.asarray(p, np.float64)))[0]:
            pre = h @ Wk.T + bk
            near, h = min(near, float(pre.abs().min())), torch.relu(pre)
        print("KINK smallest |pre-activation| %.2e" % near)
        assert near >= tc.KINK
    off = 0
    for i, o in net.trunk:                       # a dead ReLU trunk would hide the backward sweeps: every block has a gradient
        assert np.abs(g64[off:off + i * o]).max() > 0
        off += i * o + o
    for r in tc.edge_rows(rows, R):
        _, g1 = net.loss_grad(p, X, C, ri[r:r + 1])
        moved = np.abs(g1).max() / rows
        print("DROP cnormal %-14s row %5d: gradient moves %.3e = %.1f bars (bar %.3e, e_ref %.3e)"
              % (tc.step_id(case), r, moved, moved / bar, bar, e_ref))
        assert moved >= 10 * bar
