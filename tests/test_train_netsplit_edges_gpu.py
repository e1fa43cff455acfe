"""The d <= 16 row-parallel training kernel k_mfma_train at the smallest sizes where its layer seams and tile loops can go wrong.

The net-split form (rnvp_mfma_train_dev.h, rnvp_mfma_layer.h) addresses its weight fragments from a scalar base that the wave's
role selects, keeps the forward accumulators of the wave's own net only, couples the two nets' outputs behind one branch on the
role and reads its transposition tiles from per-layer LDS bases.  What can break there shows at the edges: one, two and three
layers of either mask parity (first, last, odd layer), one to eight hidden tiles per net (the forward loop takes two per trip), rows
around the wave's 16 and the workgroup's 64, every row-tile count `pick_rows` can choose with a ragged last workgroup, guarded
loads (d = 10, c = 3), the other translation unit (c = 0), ReLU, and both arithmetics of the forward GEMM1.  The same layer code
without net split (more than 256 workgroups) runs once with one and once with two row groups per workgroup.

Each case pins through rnvp_last_dispatch WHICH kernel, variant, row tiles and grid served the call, compares loss and gradient with
the float64 oracle (tolerances of test_bench_sizes_gpu.py::test_training_kernel_at_benchmark_batch_vs_float64_oracle) and asks two
consecutive calls for the same bits.  The mask parity is the kernel's `alt` 0 / 1, which the API spells alt_masks 1 / 2
(include/rnvp_hip.h); alt_masks 0 declares arbitrary masks and leaves the MFMA path.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _dev(a, dtype=torch.float32):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a)).to(dtype).cuda().contiguous()


def _oracle64_loss_grad(s, params, X, C, masks, inv_B, block=1024):
    """float64 loss and gradient: row blocks on a thread pool (ctypes releases the GIL), added in float64 in block order"""
    from concurrent.futures import ThreadPoolExecutor
    from oracle import Oracle
    from probaforms_amd._engine import effective_cpus
    o = Oracle(64)
    p64 = params.astype(np.float64)
    n = X.shape[0]
    cuts = [(a, min(a + block, n)) for a in range(0, n, block)]

    def one(ab):
        a, b = ab
        lo, g = o.loss_grad(s, p64, X[a:b].astype(np.float64), None if C is None else C[a:b].astype(np.float64), masks=masks, inv_B=inv_B)
        return float(lo), np.asarray(g, np.float64)
    with ThreadPoolExecutor(max(1, min(effective_cpus(), 32))) as ex:
        parts = list(ex.map(one, cuts))
    return sum(p[0] for p in parts), np.sum([p[1] for p in parts], axis=0)


def _masks(L, d, alt):
    return ((np.arange(d)[None, :] + np.arange(L)[:, None] + alt - 1) % 2).astype(np.uint8)


def _check(L, d, c, h, act, alt, prec, n, expect, with_index=True, seed=0):
    """loss_grad twice on n rows; expect = (kernel, variant, row_tiles, waves, grid)"""
    from oracle import Shape
    from probaforms_amd import _hip
    rng = np.random.default_rng(9000 + 131 * n + 17 * h + 7 * L + alt + seed)
    s = Shape.make(L, d, c, (h,), act)
    shape = _hip.RnvpShape.make(L, d, c, (h,), act, alt_masks=alt, precision=prec)
    P = _hip.param_count(shape)
    params = (rng.uniform(-1, 1, size=P) * min(0.5, 1.5 / np.sqrt(h + d + c))).astype(np.float32)
    N = n + 37 if with_index else n
    Xall = rng.standard_normal((N, d)).astype(np.float32)
    Call = rng.standard_normal((N, c)).astype(np.float32) if c else None
    idx = rng.permutation(N)[:n].astype(np.int64) if with_index else None
    ws = torch.empty(_hip.workspace_bytes(shape, _hip.OP_TRAIN, n), dtype=torch.uint8, device="cuda")
    pd, xd, cd = _dev(params), _dev(Xall), _dev(Call)
    id_ = _dev(idx, torch.int64) if with_index else None
    outs = []
    for _ in range(2):
        grad = torch.full((P,), float("nan"), device="cuda"); loss = torch.full((1,), float("nan"), device="cuda")
        _hip.loss_grad(shape, pd, None, xd, cd, id_, n, 1.0 / n, grad, loss, ws)
        torch.cuda.synchronize()
        outs.append((grad.clone(), loss.clone()))
    got = _hip.last_dispatch(_hip.PROFILE_TRAIN)
    assert (got["kernel"], got["variant"], got["row_tiles"], got["waves"], got["grid"]) == expect, got
    assert got["gemm1_fwd"] == prec and got["rows"] == n, got
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    X = Xall[idx] if with_index else Xall
    Cn = None if Call is None else (Call[idx] if with_index else Call)
    lo, go = _oracle64_loss_grad(s, params, X, Cn, _masks(L, d, alt), 1.0 / n)
    g = outs[0][0].cpu().numpy().astype(np.float64); l = float(outs[0][1].item())
    gerr = np.abs(g - go).max() / np.abs(go).max()
    lerr = abs(l - lo)
    print("L%d d%d c%d h%d %s alt%d %s n%d: grid %d R %d | loss err %.2e | grad err %.2e of scale" %
          (L, d, c, h, act, alt, prec, n, got["grid"], got["row_tiles"], lerr, gerr))
    assert np.isfinite(g).all()
    assert lerr < max(1e-5, 5e-7 * abs(lo)), (l, lo)
    assert gerr < 3e-6, gerr


def _ns(n, R=1):
    return ("k_mfma_train", "netsplit", R, 8, (n + 64 * R - 1) // (64 * R))


ROWS = (1, 15, 16, 17, 63, 64, 65, 129)
LAYERS = [(L, alt) for L in (1, 2, 3) for alt in (1, 2)]
GEOS = [(16, 4), (16, 0), (10, 3)]          # (d, c): full rows; no condition (rnvp_mfma_train_nf2c0); guarded loads


# every row count with every (layers, parity); geometry, activation, arithmetic and hidden width rotate through the cases
@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("L,alt", LAYERS)
def test_netsplit_one_row_tile_tiny_batches(n, L, alt):
    i = ROWS.index(n) + 3 * LAYERS.index((L, alt))
    d, c = GEOS[i % 3]
    act = ("tanh", "relu")[(i // 3) % 2]
    prec = ("f32", "bx3")[(i // 2) % 2]
    h = (16, 32)[(i // 5) % 2]
    _check(L, d, c, h, act, alt, prec, n, _ns(n))


# every geometry x activation x arithmetic x hidden width at the rows just past a wave and just past a workgroup
@pytest.mark.parametrize("n", (17, 65))
@pytest.mark.parametrize("h", (16, 32))
@pytest.mark.parametrize("prec", ("f32", "bx3"))
@pytest.mark.parametrize("act", ("tanh", "relu"))
@pytest.mark.parametrize("d,c", GEOS)
def test_netsplit_one_row_tile_every_form(d, c, act, prec, h, n):
    alt = 1 + (h // 16 + n + (act == "relu")) % 2
    _check(3, d, c, h, act, alt, prec, n, _ns(n), seed=1)


# 1, 2, 3, 5 and 8 hidden tiles per net: the forward loop takes two tiles per trip; 8 193 rows is the first size past the tile-split
# kernel (one row tile per wave)
@pytest.mark.parametrize("h", (16, 32, 48, 80, 128))
@pytest.mark.parametrize("prec", ("f32", "bx3"))
def test_netsplit_forward_tile_pairs(h, prec):
    _check(2, 16, 4, h, "tanh", 1, prec, 8193, _ns(8193))


# pick_rows: two row tiles per wave from 16 385 rows, four from 32 769; 32 805 rows leave a ragged last workgroup
@pytest.mark.parametrize("with_index", (True, False))
@pytest.mark.parametrize("n,R", [(16385, 2), (16960, 2), (32769, 4), (32805, 4)])
def test_netsplit_row_tiles_per_wave(n, R, with_index):
    _check(2, 16, 4, 80, "tanh", 1, "bx3", n, _ns(n, R), with_index=with_index)


# the same layer code without net split: more than 256 workgroups.  65 537 rows: pick_rows prices three rounds of two row tiles
# (513 row groups) below two rounds of four, and the grid cap of 512 gives workgroup 0 a second, one-row group; 131 333 rows: four
# row tiles, 514 row groups on 512 workgroups -- two of them add a second group to their own partial, and the last group is ragged
@pytest.mark.parametrize("n,R", [(65537, 2), (131072 + 256 + 5, 4)])
def test_row_parallel_without_net_split(n, R):
    _check(1, 16, 4, 32, "tanh", 1, "bx3", n, ("k_mfma_train", "rowpar", R, 4, 512))


def test_fit_epoch_of_three_batches_equals_train_steps_bit_for_bit():
    """the scheme of test_bench_sizes_gpu.py::test_fit_epoch_repack_equals_a_loop_of_train_steps_bit_for_bit on a shape of the
    first group: batches of 129, 129 and 65 rows (above the 128 rows the LDS-resident epoch kernel takes)"""
    from probaforms_amd import _hip
    L, d, c, h, batch = 3, 16, 4, 32, 129
    n = 2 * batch + 65
    shape = _hip.RnvpShape.make(L, d, c, (h,), "tanh", alt_masks=1)
    P = _hip.param_count(shape)
    gen = torch.Generator(device="cuda").manual_seed(4242)
    p0 = (torch.rand(P, device="cuda", generator=gen) - 0.5) * 0.4
    x = torch.randn(n, d, device="cuda", generator=gen); cc = torch.randn(n, c, device="cuda", generator=gen)
    perm = torch.randperm(n, device="cuda", generator=gen)
    ws = torch.empty(_hip.workspace_bytes(shape, _hip.OP_TRAIN, batch), dtype=torch.uint8, device="cuda")
    pa = p0.clone(); ma = torch.zeros(P, device="cuda"); va = torch.zeros(P, device="cuda"); ga = torch.empty(P, device="cuda")
    la = torch.zeros(3, device="cuda")
    _hip.fit_epoch(shape, pa, None, x, cc, perm, n, batch, ga, la, ma, va, 1e-3, 0.9, 0.999, 1e-8, 0.01, 1, ws)
    got = _hip.last_dispatch(_hip.PROFILE_TRAIN)
    assert (got["kernel"], got["variant"], got["row_tiles"], got["grid"], got["rows"]) == ("k_mfma_train", "netsplit", 1, 2, 65), got
    pb = p0.clone(); mb = torch.zeros(P, device="cuda"); vb = torch.zeros(P, device="cuda"); gb = torch.empty(P, device="cuda")
    lb = torch.zeros(3, device="cuda")
    for k in range(3):
        lo = k * batch; rows = min(batch, n - lo)
        _hip.train_step(shape, pb, None, x, cc, perm[lo:lo + rows].contiguous(), rows, 1.0 / rows, gb, lb[k:k + 1], mb, vb,
                        1e-3, 0.9, 0.999, 1e-8, 0.01, k + 1, ws)
    torch.cuda.synchronize()
    assert torch.isfinite(la).all() and torch.isfinite(pa).all()
    assert torch.equal(la, lb) and torch.equal(pa, pb) and torch.equal(ma, mb) and torch.equal(va, vb)
    assert not torch.equal(pa, p0)
