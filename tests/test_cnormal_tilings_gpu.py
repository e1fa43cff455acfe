"""libpf_cnormal.so at the tile sizes the host can pick but the fixtures never reach (tests/tilings_cases.py): step tiles of
1..256 rows (at 256 every thread of the workgroup is a row), R = cap with a cap that is no power of two, launches above 64 KiB of
LDS up to the last shape that fits, pfn_forward tiles of 4, 7 and 256 rows with n on either side of a tile multiple, and
pfn_fit_epoch whose ragged last batch picks a smaller tile than the workspace was sized for.

Every case first asserts its regime through pfn_tiling, runs on a workspace of exactly pfn_workspace_bytes() filled with 0xFF
and on poisoned outputs, and is compared with the float64 restatement (tests/cnormal_torch.py) under the measured bar of
tests/parity.py (for the long chains of tilings_cases.LONG_FAN_IN, e_ref is the larger of torch's and the
kernel-order float32 restatement's).  profiles/r11_tilings_parity.txt holds the REGIME and PARITY lines of one run.  Bitwise claims have no
tolerance."""
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
import tilings_cases as tc  # noqa: E402
from parity import parity  # noqa: E402
from probaforms_amd.models import _cnormal_lib as N  # noqa: E402

pytestmark = pytest.mark.gpu

native_libs.ensure_built(N)

DEV = torch.device("cuda")
F32 = torch.float32
BIG_LDS = 64 * 1024
LR, WD = 1e-3, 0.01


def dev(a, dtype=torch.float32):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def nets(name):
    return N.Shape.make(*tc.N_SHAPES[name]), ct.Normal(*tc.N_SHAPES[name])


def step_refs(case, p, X, C, ri):
    """CPU only: parity()'s keyword arguments for the gradient and the loss of one step.  Long chains add the kernel-order
    float32 restatement (tilings_cases)"""
    name, rows, R = case[:3]
    net = ct.Normal(*tc.N_SHAPES[name])
    l64, g64 = net.loss_grad(p, X, C, ri)
    l32, g32 = net.loss_grad(p, X, C, ri, F32)
    lo, go = None, None
    if tc.n_long(name):
        seq = ct.Normal(*tc.N_SHAPES[name], sequential=True)
        lo, go = tc.ordered32(lambda s, e: seq.loss_grad(p, X, C, ri[s:e], F32), rows, R)
    return dict(ref32=g32, ref64=g64, also32=go), dict(ref32=l32, ref64=l64, also32=lo)


def forward_refs(name, p, C, eps, X):
    """CPU only: parity()'s keyword arguments for pfn_forward's outputs, in its order (mu, sigma, x_tilde, inv)"""
    net = ct.Normal(*tc.N_SHAPES[name])
    r64, r32 = net.forward(p, C, eps, X), net.forward(p, C, eps, X, F32)            # (x_tilde, inv, mu, sigma)
    ro = ct.Normal(*tc.N_SHAPES[name], sequential=True).forward(p, C, eps, X, F32) if tc.n_long(name) else (None,) * 4
    return [dict(ref32=r32[k], ref64=r64[k], also32=ro[k]) for k in (2, 3, 0, 1)]


def regime(case):
    """assert the step regime the case was written for; returns the shape and the restatement"""
    name, rows, R, cap, G, lds = case
    shape, net = nets(name)
    t = N.tiling(shape, rows)
    print("REGIME cnormal %-14s R %3d cap %3d G %3d lds %6d (%s 64 KiB) bound %d" % (
        tc.step_id(case), t.step_tile, t.step_cap, t.step_wgs, t.step_lds_bytes, ">" if t.step_lds_bytes > BIG_LDS else "<=",
        t.step_wg_bound))
    assert (t.step_tile, t.step_cap, t.step_wgs, t.step_lds_bytes) == (R, cap, G, lds)
    assert G <= t.step_wg_bound
    return shape, net


def gpu_loss_grad(shape, net, pd, Xd, Cd, rid, rows, ws, grad=True, loss=True):
    g = torch.empty(net.P, device=DEV) if grad else None
    l = torch.empty(1, device=DEV) if loss else None
    st = torch.empty(1, dtype=torch.int32, device=DEV)
    hygiene.poison_outputs(g, l, st)
    N.loss_grad(shape, pd, Xd, Cd, rid, rows, g, l, st, ws)
    torch.cuda.synchronize()
    hygiene.assert_all_written({k: v for k, v in (("grad", g), ("loss", l), ("status", st)) if v is not None}, "pfn_loss_grad")
    assert int(st) == 0
    return g, l


def adam_on(net, p, g, dtype):
    """one torch.optim.Adam step (step 1, zero state) in `dtype` on the GIVEN gradient: (params, exp_avg, exp_avg_sq) [P].
    out is its own leaf: in independent mode it has no gradient and Adam leaves it and its state alone"""
    pm = torch.tensor(p[:net.P_main], dtype=dtype, requires_grad=True)
    po = torch.tensor(p[net.P_main:], dtype=dtype, requires_grad=True)
    opt = torch.optim.Adam([pm, po], lr=LR, weight_decay=WD)
    pm.grad = torch.tensor(g[:net.P_main], dtype=dtype)
    if not net.independent:
        po.grad = torch.tensor(g[net.P_main:], dtype=dtype)
    opt.step()
    zero = torch.zeros_like(po)
    state = [[opt.state[t][k] if t in opt.state else zero for t in (pm, po)] for k in ("exp_avg", "exp_avg_sq")]
    return [torch.cat(v).detach().numpy().astype(np.float64) for v in ([pm, po], state[0], state[1])]


@pytest.mark.parametrize("case", tc.N_STEPS, ids=tc.step_id)
def test_step_matches_float64_at_every_tile(case):
    name, rows, R = case[:3]
    shape, net = regime(case)
    p, X, C, ri = tc.cnormal_problem(name, rows, R)
    pd, Xd, Cd, rid = dev(p), dev(X), dev(C), dev(ri, torch.int64)
    ws = hygiene.workspace(N.workspace_bytes(shape, rows), "ones")
    g, l = gpu_loss_grad(shape, net, pd, Xd, Cd, rid, rows, ws)
    gref, lref = step_refs(case, p, X, C, ri)
    parity(tc.step_id(case), "grad", g.cpu().numpy(), **gref)
    parity(tc.step_id(case), "loss", float(l), **lref)
    if net.independent:
        assert not g[net.P_main:].any()
    # one pfn_train_step: the same gradient bit for bit, and Adam on that gradient as torch computes it
    p1, m1, v1 = dev(p), torch.zeros(net.P, device=DEV), torch.zeros(net.P, device=DEV)
    g1, l1, st = torch.empty(net.P, device=DEV), torch.empty(1, device=DEV), torch.empty(1, dtype=torch.int32, device=DEV)
    hygiene.poison_outputs(g1, l1, st)
    N.train_step(shape, p1, m1, v1, Xd, Cd, rid, rows, N.adam(LR, WD), 1, g1, l1, st, ws)
    torch.cuda.synchronize()
    hygiene.assert_all_written(dict(grad=g1, loss=l1, status=st, params=p1, exp_avg=m1, exp_avg_sq=v1), "pfn_train_step")
    assert int(st) == 0 and hygiene.same_bits(g1, g) and hygiene.same_bits(l1, l)
    gn = g1.cpu().numpy()
    a32, a64 = adam_on(net, p, gn, F32), adam_on(net, p, gn, torch.float64)
    for what, got, r32, r64 in zip(("adam params", "adam exp_avg", "adam exp_avg_sq"), (p1, m1, v1), a32, a64):
        parity(tc.step_id(case), what, got.cpu().numpy(), r32, r64)
    if net.independent:
        assert np.array_equal(p1[net.P_main:].cpu().numpy(), p[net.P_main:]) and not m1[net.P_main:].any()


INDEX_CASES = [c for c in tc.N_STEPS if tc.step_id(c) in ("full_wg-4097", "big_lds-33", "cap3-5")]


@pytest.mark.parametrize("case", INDEX_CASES, ids=tc.step_id)
def test_row_index_none_arange_and_gather_give_the_same_bits(case):
    name, rows, R = case[:3]
    shape, net = regime(case)
    p, X, C, ri = tc.cnormal_problem(name, rows, R)
    pd = dev(p)
    Xg, Cg = dev(X[ri]), dev(C[ri])
    ws = hygiene.workspace(N.workspace_bytes(shape, rows), "ones")
    a = gpu_loss_grad(shape, net, pd, dev(X), dev(C), dev(ri, torch.int64), rows, ws)
    b = gpu_loss_grad(shape, net, pd, Xg, Cg, None, rows, ws)
    c = gpu_loss_grad(shape, net, pd, Xg, Cg, torch.arange(rows, device=DEV), rows, ws)
    for u, v in zip(a + a, b + c):
        assert hygiene.same_bits(u, v)
    g_only = gpu_loss_grad(shape, net, pd, Xg, Cg, None, rows, ws, loss=False)[0]
    l_only = gpu_loss_grad(shape, net, pd, Xg, Cg, None, rows, ws, grad=False)[1]
    assert hygiene.same_bits(g_only, b[0]) and hygiene.same_bits(l_only, b[1])
    # repeats and gaps: even table rows only, many of them twice
    rr = np.random.default_rng(rows).integers(0, X.shape[0] // 2, size=rows) * 2
    assert len(np.unique(rr)) < rows or rows < 8
    g, l = gpu_loss_grad(shape, net, pd, dev(X), dev(C), dev(rr, torch.int64), rows, ws)
    gref, lref = step_refs(case, p, X, C, rr)
    parity(tc.step_id(case), "repeats grad", g.cpu().numpy(), **gref)
    parity(tc.step_id(case), "repeats loss", float(l), **lref)


# (shape name, the tile the host must pick, LDS bytes, the n to run)
FORWARD = [("wide_fwd", 256, 132548, (255, 256, 257, 513)), ("cap3", 7, None, (6, 7, 8, 15)), ("cap1", 4, None, (3, 4, 5, 9))]


@pytest.mark.parametrize("name,tile,lds,ns", FORWARD, ids=[c[0] for c in FORWARD])
def test_forward_tiles_on_both_sides_of_a_multiple(name, tile, lds, ns):
    shape, net = nets(name)
    d, c = net.d, net.c
    p = tc.cnormal_problem(name, 1, 1)[0]
    pd = dev(p)
    rng = np.random.default_rng(tile)
    for n in ns:
        t = N.tiling(shape, n)
        print("REGIME cnormal %-14s forward n %3d tile %3d lds %6d" % (name, n, t.fwd_tile, t.fwd_lds_bytes))
        assert t.fwd_tile == tile and BIG_LDS < t.fwd_lds_bytes <= 160 * 1024 and lds in (None, t.fwd_lds_bytes)
        X, C, eps = (rng.normal(size=(n, k)).astype(np.float32) for k in (d, c, d))
        Xd, Cd, ed = dev(X), dev(C), dev(eps)
        refs = forward_refs(name, p, C, eps, X)
        names = ("mu", "sigma", "x_tilde", "inv")
        full = [torch.empty(n, d, device=DEV) for _ in range(4)]
        st = torch.empty(1, dtype=torch.int32, device=DEV)
        hygiene.poison_outputs(st, *full)
        N.forward(shape, pd, Cd, ed, Xd, n, full[0], full[1], full[2], full[3], st)
        torch.cuda.synchronize()
        hygiene.assert_all_written(dict(zip(names, full), status=st), "pfn_forward")
        assert int(st) == 0
        for k in range(4):
            parity("%s n=%d" % (name, n), names[k], full[k].cpu().numpy(), **refs[k])
        for skip in range(4):                                    # each output alone NULL: the others keep their bits
            outs = [None if k == skip else torch.empty(n, d, device=DEV) for k in range(4)]
            hygiene.poison_outputs(st, *outs)
            N.forward(shape, pd, Cd, ed, Xd, n, outs[0], outs[1], outs[2], outs[3], st)
            torch.cuda.synchronize()
            assert int(st) == 0
            assert all(hygiene.same_bits(outs[k], full[k]) for k in range(4) if k != skip), (n, names[skip])


# (shape name, n, batch size, (R, G) of the full batch, (R, G) of the ragged last batch)
EPOCHS = [("cap11", 2049 + 2048, 2049, (11, 187), (8, 256)), ("cap3", 5, 3, (3, 1), (3, 1))]


@pytest.mark.parametrize("name,n,B,full,last", EPOCHS, ids=[c[0] for c in EPOCHS])
def test_fit_epoch_with_a_smaller_last_tile_equals_the_step_loop_bitwise(name, n, B, full, last):
    shape, net = nets(name)
    tf, tl = N.tiling(shape, B), N.tiling(shape, n - B)
    print("REGIME cnormal %-14s fit_epoch: batch %d R %d G %d, last batch %d R %d G %d, bound %d" % (
        name, B, tf.step_tile, tf.step_wgs, n - B, tl.step_tile, tl.step_wgs, tf.step_wg_bound))
    assert (tf.step_tile, tf.step_wgs) == full and (tl.step_tile, tl.step_wgs) == last
    assert max(tf.step_wgs, tl.step_wgs) <= tf.step_wg_bound
    p, X, C, _ = tc.cnormal_problem(name, n - 3, 8)
    rng = np.random.default_rng(n)
    Xd, Cd = dev(X), dev(C)
    perm = dev(rng.permutation(n), torch.int64)
    opt = N.adam(LR, WD)
    nb = -(-n // B)
    p1, m1, v1 = dev(p), torch.zeros(net.P, device=DEV), torch.zeros(net.P, device=DEV)
    p2, m2, v2 = dev(p), torch.zeros(net.P, device=DEV), torch.zeros(net.P, device=DEV)
    l1, l2 = torch.empty(nb, device=DEV), torch.empty(nb, device=DEV)
    s1, s2 = torch.empty(1, dtype=torch.int32, device=DEV), torch.empty(1, dtype=torch.int32, device=DEV)
    hygiene.poison_outputs(l1, l2, s1, s2)
    N.fit_epoch(shape, p1, m1, v1, Xd, Cd, perm, n, B, opt, 1, l1, s1, hygiene.workspace(N.workspace_bytes(shape, B), "ones"))
    for b, s in enumerate(range(0, n, B)):
        e = min(n, s + B)
        N.train_step(shape, p2, m2, v2, Xd, Cd, perm[s:e], e - s, opt, b + 1, None, l2[b:b + 1], s2,
                     hygiene.workspace(N.workspace_bytes(shape, e - s), "ones"))
        torch.cuda.synchronize()
        assert int(s2) == 0
    torch.cuda.synchronize()
    hygiene.assert_all_written(dict(params=p1, exp_avg=m1, exp_avg_sq=v1, losses=l1, status=s1), "pfn_fit_epoch")
    assert int(s1) == 0
    for a, b in ((p1, p2), (m1, m2), (v1, v2), (l1, l2)):
        assert hygiene.same_bits(a, b)
    assert not hygiene.same_bits(p1, dev(p))
