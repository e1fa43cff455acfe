"""No kernel result may depend on what its workspace held before the call.

Every other GPU test hands a kernel a workspace from torch.empty, used once: almost always zeroed memory.  The product reuses one
workspace per operation across calls of different row counts (FlowEngine.workspace) and torch's caching allocator hands back
recycled blocks.  Here every entry point runs once per pattern of tests/hygiene.py (zeros, the leftovers of a previous LARGER call
of the same entry point, 0xFF bytes = NaN / -1, 0x7F bytes = 3.39e38 / a huge count) on freshly poisoned outputs, and

  * every output of every pattern must carry the bits of the `zeros` run (the kernels use no float atomics and are documented as
    run-to-run bit-identical: no tolerance applies), and no output element may still hold the output poison;
  * the `zeros` run must agree with the project's reference for the operation at the bar the existing test of that entry point
    uses (named in a comment at each check), so that two equally wrong runs cannot pass.

Oracle cost bounds the shapes: the flows are the benchmark geometries (C2: d 16 / cdim 4, C3: 32 / 8, C4: 64 / 16, cdim 0) with
two layers and narrow nets; per-row outputs of large calls are checked on their first and last 300 rows (the ragged tail).
"""
import numpy as np
import pytest
import torch

import hygiene

pytestmark = pytest.mark.gpu


def _dev(a, dtype=torch.float32):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a)).to(dtype).cuda().contiguous()


def _nan(*shape):
    return torch.full(shape, float("nan"), device="cuda")


class _Flow:
    """one flow shape with parameters, masks and the oracle's view of it"""

    def __init__(self, L, d, c, hidden, alt=1, precision="f32", small_calls=0, family="auto", act="tanh"):
        from oracle import Shape
        from probaforms_amd import _hip
        self.hip, self.L, self.d, self.c, self.hidden = _hip, L, d, c, hidden
        self.shape = _hip.RnvpShape.make(L, d, c, hidden, act, alt_masks=alt, precision=precision, small_calls=small_calls, family=family)
        self.oshape = Shape.make(L, d, c, hidden, act)
        self.P = _hip.param_count(self.shape)
        rng = np.random.default_rng(1000 * L + 10 * d + c + sum(hidden))
        self.params_np = (rng.uniform(-1, 1, self.P) * min(0.2, 1.0 / np.sqrt(max(hidden) + d + c))).astype(np.float32)
        self.masks_np = ((np.arange(d)[None] + np.arange(L)[:, None]) % 2).astype(np.uint8)
        self.params, self.masks = _dev(self.params_np), _dev(self.masks_np, torch.uint8)
        self.rng = rng

    def data(self, rows):
        X = self.rng.standard_normal((rows, self.d)).astype(np.float32)
        C = self.rng.standard_normal((rows, self.c)).astype(np.float32) if self.c else None
        return X, C

    def ws_bytes(self, op, rows):
        return self.hip.workspace_bytes(self.shape, op, rows)


def _prime_rows(n):
    """rows of the priming call of the `replay` pattern: a LARGER launch grid than the checked call's, so that leftovers (partials,
    dumped activations, counters) exist beyond what the checked call writes"""
    return 2 * n + 777


def _per_pattern(flow, op, n, call):
    """call(rows, ws) -> {name: output tensor}: once per pattern (zeros and replay before the NaN and the huge fill), checked for
    pattern independence and unwritten outputs; returns the `zeros` run"""
    outs = {}
    for pat in hygiene.PATTERNS:
        if pat == "replay":
            ws = hygiene.workspace(flow.ws_bytes(op, _prime_rows(n)), pat)
            call(_prime_rows(n), ws)
        else:
            ws = hygiene.workspace(flow.ws_bytes(op, n), pat)
        outs[pat] = call(n, ws)
        torch.cuda.synchronize()
    return outs


def _settle(outs, what, allow=()):
    hygiene.assert_all_written(outs["zeros"], what, allow)
    hygiene.assert_pattern_independent(outs, what)
    return outs["zeros"]


def _edge_rows(n):
    """the first and the last 300 rows of a call (all of a small one)"""
    return np.arange(n) if n <= 600 else np.concatenate([np.arange(300), np.arange(n - 300, n)])


# ---- rnvp_forward_logprob, rnvp_inverse, rnvp_sample -------------------------------------------------------------------------------
# id: (L, d, c, hidden, alt_masks, precision, small_calls, family)
FLOW_FORMS = {
    "chained_f32":    (2, 16, 4, (32,), 1, "f32", 0, "auto"),        # register-chained, f32-input MFMA
    "bx3_direct":     (2, 16, 4, (32,), 1, "bx3", 0, "auto"),        # split-bf16 GEMM1, the barrier-free d <= 16 form
    "bx3_staged":     (2, 32, 8, (48,), 1, "bx3", 0, "auto"),        # split-bf16 GEMM1, weights staged in LDS
    "tile_split":     (2, 16, 4, (32,), 1, "f32", 1, "auto"),        # small_calls = 'latency': tile-split kernels up to 4096 rows
    "lmm16":          (2, 6, 2, (12, 20), 0, "f32", 0, "lmm16"),     # any-shape MFMA kernels, 16-row blocks
    "valu":           (2, 6, 2, (12, 20), 0, "f32", 0, "valu"),      # one thread per row
}
FLOW_ROWS = (1, 17, 257, 4097, 70001)


@pytest.mark.parametrize("n", FLOW_ROWS)
@pytest.mark.parametrize("form", list(FLOW_FORMS))
def test_flow_calls_do_not_depend_on_the_workspace(form, n, oracle32):
    if form == "tile_split" and n > 4096:
        n = 4096 if n == 4097 else 4095         # the latency kernels serve at most 4096 rows: the limit itself and one ragged below it
    f = _Flow(*FLOW_FORMS[form])
    _hip, d = f.hip, f.d
    for op in (_hip.OP_FORWARD, _hip.OP_INVERSE):
        assert _hip.kernel_path(f.shape, f.masks_np, op) == (_hip.PATH_LMM if form == "lmm16" else _hip.PATH_GENERIC if form == "valu" else _hip.PATH_MFMA)
    X, C = f.data(_prime_rows(n))
    xd, cd = _dev(X), _dev(C)
    sub = _edge_rows(n)
    Cs = None if C is None else C[:n][sub]

    def forward(rows, ws):
        z, ld, lp, tot = _nan(rows, d), _nan(rows), _nan(rows), _nan(1)
        _hip.forward_logprob(f.shape, f.params, f.masks, xd, cd, None, rows, z, ld, lp, tot, ws)
        return dict(z=z, logdet=ld, logp=lp, logp_sum=tot)

    o = _settle(_per_pattern(f, _hip.OP_FORWARD, n, forward), "rnvp_forward_logprob[%s, %d rows]" % (form, n))
    zo, lpo, _ = oracle32.log_prob(f.oshape, f.params_np, X[:n][sub], Cs, f.masks_np)
    z, lp = o["z"].cpu().numpy()[sub], o["logp"].cpu().numpy()[sub]
    # bars of test_hip_kernels.py::test_mfma_path_edge_shapes_vs_oracle (z, log p) and ::test_large_batch_properties (the identity
    # logp == logdet - 0.5 (d ln 2 pi + |z|^2), the sum)
    assert np.abs(z - zo).mean() < 2e-6 and np.abs(z - zo).max() < 2e-4
    assert np.abs(lp - lpo).mean() < max(1e-5, 2.4e-7 * np.abs(lpo).max())
    ident = o["logdet"] - 0.5 * (d * np.log(2 * np.pi) + (o["z"].double() ** 2).sum(1)).float()
    assert (o["logp"] - ident).abs().max().item() < 2e-4 * max(1.0, d / 16)
    tot = o["logp"].double().sum().item()
    assert abs(o["logp_sum"].item() - tot) < 1e-5 * max(1.0, abs(tot))

    def inverse(rows, ws):
        x = _nan(rows, d)
        _hip.inverse(f.shape, f.params, f.masks, xd, cd, rows, x, ws)
        return dict(x=x)

    o = _settle(_per_pattern(f, _hip.OP_INVERSE, n, inverse), "rnvp_inverse[%s, %d rows]" % (form, n))
    want = oracle32.sample(f.oshape, f.params_np, X[:n][sub], Cs, f.masks_np)
    # bar of test_hip_kernels.py::test_fused_sample_equals_prior_then_inverse
    assert np.abs(o["x"].cpu().numpy()[sub] - want).mean() < 5e-6 * max(1.0, np.abs(want).mean())

    seed, off = 99, 5

    def sample(rows, ws):
        x = _nan(rows, d)
        _hip.sample(f.shape, f.params, f.masks, cd, rows, seed, off, x, ws)
        return dict(x=x)

    o = _settle(_per_pattern(f, _hip.OP_INVERSE, n, sample), "rnvp_sample[%s, %d rows]" % (form, n))
    zs = oracle32.prior_normal(seed, off, n, d)[sub]
    want = oracle32.sample(f.oshape, f.params_np, zs, Cs, f.masks_np)
    assert np.abs(o["x"].cpu().numpy()[sub] - want).mean() < 5e-6 * max(1.0, np.abs(want).mean())       # same test, same bar


# ---- rnvp_loss_grad, rnvp_loss_grad_zseed, rnvp_backward, rnvp_train_step -------------------------------------------------------
# id: (L, d, c, hidden, alt_masks, family)
TRAIN_FORMS = {
    "chained_c2":   (2, 16, 4, (16,), 1, "auto"),       # NF 2 / CQ 1; tile-split up to 8192 rows, row-parallel above
    "chained_c3":   (2, 32, 8, (16,), 1, "auto"),       # NF 4
    "chained_c4":   (2, 64, 16, (16,), 1, "auto"),      # NF 8
    "chained_c0":   (2, 16, 0, (16,), 1, "auto"),       # cdim 0
    "lmm16":        (2, 6, 2, (12, 20), 0, "lmm16"),
    "lmm64":        (2, 6, 2, (12, 20), 0, "lmm64"),
    # 128 narrow layers: the dumped weight-gradient operands of the 16-row kernels reach 1 GiB after 8192 rows, so the call runs in row
    # chunks (rnvp_lmm.hip chunk_rows) while the oracle stays affordable; the boundary is read off rnvp_workspace_bytes (_row_chunk)
    "lmm16_chunks": (128, 2, 0, (16, 16), 0, "lmm16"),
    "valu":         (2, 6, 2, (12, 20), 0, "valu"),
}
TRAIN_ROWS = (1, 33, 8191, 8193, 20000, 70001)
TRAIN_CASES = ([(form, n) for form in ("chained_c2", "chained_c3", "chained_c4", "chained_c0", "lmm16", "valu") for n in TRAIN_ROWS] +
               [("lmm64", n) for n in (8192, 8193, 20000, 70001)] +          # (the 64-row kernels serve calls from 8192 rows on)
               [("lmm16_chunks", "chunk+1"), ("lmm16_chunks", "2chunk+1")])   # one row into the second chunk, one into the third


def _row_chunk(f, block):
    """rows per pass of the any-shape training kernels, from the library: the workspace grows with the rows (in blocks of `block`) until
    one chunk is reached"""
    top = f.ws_bytes(f.hip.OP_TRAIN, 1 << 22)
    lo, hi = 1, 1 << 22
    while lo < hi:
        mid = (lo + hi) // 2
        if f.ws_bytes(f.hip.OP_TRAIN, mid) >= top:
            hi = mid
        else:
            lo = mid + 1
    return (lo + block - 1) // block * block


def _train_path(hip, form):
    return hip.PATH_MFMA if form.startswith("chained") else (hip.PATH_GENERIC if form == "valu" else hip.PATH_LMM)


@pytest.mark.parametrize("form,n", TRAIN_CASES)
def test_training_calls_do_not_depend_on_the_workspace(form, n, oracle32, oracle64):
    L, d, c, hidden, alt, family = TRAIN_FORMS[form]
    f = _Flow(L, d, c, hidden, alt=alt, family=family)
    _hip, P = f.hip, f.P
    assert _hip.kernel_path(f.shape, f.masks_np, _hip.OP_TRAIN) == _train_path(_hip, form)
    if isinstance(n, str):
        chunk = _row_chunk(f, 16)
        assert 4096 <= chunk <= 16384, chunk          # (a chunk the float64 oracle can follow)
        n = (2 * chunk if n.startswith("2") else chunk) + 1
    N = max(_prime_rows(n), 20000)
    X, C = f.data(N)
    xd, cd = _dev(X), _dev(C)
    perm = f.rng.permutation(N).astype(np.int64)
    idx = _dev(perm, torch.int64)                        # gathered rows: the priming call reads other rows than the checked one
    Xg, Cg = X[perm[:n]], None if C is None else C[perm[:n]]
    inv_B = 1.0 / n
    tag = "[%s, %d rows]" % (form, n)

    def loss_grad(rows, ws):
        g, loss = _nan(P), _nan(1)
        _hip.loss_grad(f.shape, f.params, f.masks, xd, cd, idx, rows, 1.0 / rows, g, loss, ws)
        return dict(grad=g, loss=loss)

    o = _settle(_per_pattern(f, _hip.OP_TRAIN, n, loss_grad), "rnvp_loss_grad" + tag)
    # the float64 oracle: the float32 one adds its rows up serially in float32 and drifts by more than the bar from some ten thousand rows
    # on (the existing large-batch gradient test, ::test_training_forward_on_split_bf16_keeps_the_gradient_tolerance, takes it too)
    lo, go = oracle64.loss_grad(f.oshape, f.params_np.astype(np.float64), Xg.astype(np.float64),
                                None if Cg is None else Cg.astype(np.float64), f.masks_np)
    lo, go = float(lo), go.astype(np.float32)
    g1 = o["grad"]
    scale = float(np.abs(go).max())
    # bars of test_hip_kernels.py::test_mfma_path_edge_shapes_vs_oracle / ::test_loss_grad (loss, gradient, dead entries)
    assert abs(float(o["loss"]) - lo) < max(1e-5, 5e-7 * abs(lo))
    assert np.abs(g1.cpu().numpy() - go).max() < 3e-6 * scale + 1e-9
    assert np.abs(g1.cpu().numpy()[go == 0]).max(initial=0.0) < 1e-9

    # the seeds of the loss itself: z and log det of the same rows
    z, ld = _nan(n, d), _nan(n)
    _hip.forward_logprob(f.shape, f.params, f.masks, xd, cd, idx, n, z, ld, None, None, hygiene.workspace(f.ws_bytes(_hip.OP_FORWARD, n), "zeros"))

    def zseed(rows, ws):
        g, loss = _nan(P), _nan(1)
        gz = (z * (1.0 / rows)).contiguous() if rows == n else torch.randn(rows, d, device="cuda")
        _hip.loss_grad_zseed(f.shape, f.params, f.masks, xd, cd, idx, rows, 1.0 / rows, gz, g, loss, ws)
        return dict(grad=g, loss=loss)

    o = _settle(_per_pattern(f, _hip.OP_TRAIN, n, zseed), "rnvp_loss_grad_zseed" + tag)
    # gz = z / B is the N(0, I) prior's own seed: the gradient of rnvp_loss_grad up to the seed's rounding, the bar of
    # test_hip_kernels.py::test_backward_entry_point_vs_loss_grad_and_oracle; the loss is -(sum log det) / B alone (rnvp_hip.h), at the
    # loss bar above
    assert float((o["grad"] - g1).abs().max()) < 5e-6 * scale
    want = -float(ld.double().sum()) * inv_B
    assert abs(float(o["loss"]) - want) < max(1e-5, 5e-7 * abs(want))

    if n <= 8192 or family != "auto":        # rnvp_backward: the tile-split kernel (at most 8192 rows) and the any-shape kernels
        gld = torch.full((n,), -inv_B, device="cuda")

        def backward(rows, ws):
            if rows != n and family == "auto":
                # the priming call: rnvp_backward on these kernels takes at most 8192 rows, so the larger grid that leaves partials
                # beyond the checked call's comes from another entry point on the same buffer
                return loss_grad(max(rows, 20000), ws)
            g, gx = _nan(P), _nan(rows, d)
            seeds = ((z * inv_B).contiguous(), gld) if rows == n else (torch.randn(rows, d, device="cuda"), torch.randn(rows, device="cuda"))
            _hip.backward(f.shape, f.params, f.masks, xd, cd, idx, rows, seeds[0], seeds[1], g, gx, ws)
            return dict(grad=g, gx=gx)

        o = _settle(_per_pattern(f, _hip.OP_TRAIN, n, backward), "rnvp_backward" + tag)
        assert float((o["grad"] - g1).abs().max()) < 5e-6 * scale          # test_backward_entry_point_vs_loss_grad_and_oracle
        if n <= 100:      # d loss / d x by central differences of the float64 oracle: the same test's check and bar
            gxh = o["gx"].cpu().numpy()
            for (r, j) in [(0, 0), (n - 1, d // 2)]:
                e = 1e-4
                Xp, Xm = Xg.astype(np.float64).copy(), Xg.astype(np.float64).copy()
                Xp[r, j] += e; Xm[r, j] -= e
                C64 = None if Cg is None else Cg.astype(np.float64)
                lp_, _ = oracle64.loss_grad(f.oshape, f.params_np.astype(np.float64), Xp, C64, f.masks_np)
                lm_, _ = oracle64.loss_grad(f.oshape, f.params_np.astype(np.float64), Xm, C64, f.masks_np)
                fd = (float(lp_) - float(lm_)) / (2 * e)
                assert abs(gxh[r, j] - fd) < 2e-5 * max(1.0, np.abs(gxh).max()) + 1e-7, (r, j, gxh[r, j], fd)

    lr, wd, step = 0.01, 0.2, 3
    rs = np.random.default_rng(7)
    m0 = (rs.standard_normal(P) * 1e-2).astype(np.float32); v0 = ((rs.standard_normal(P) * 1e-2) ** 2).astype(np.float32)

    def train_step(rows, ws):
        p, m, v = f.params.clone(), _dev(m0), _dev(v0)
        g, loss = _nan(P), _nan(1)
        _hip.train_step(f.shape, p, f.masks, xd, cd, idx, rows, 1.0 / rows, g, loss, m, v, lr, 0.9, 0.999, 1e-8, wd, step, ws)
        return dict(params=p, exp_avg=m, exp_avg_sq=v, grad=g, loss=loss)

    o = _settle(_per_pattern(f, _hip.OP_TRAIN, n, train_step), "rnvp_train_step" + tag)
    pr, mr, vr = f.params_np.copy(), m0.copy(), v0.copy()
    oracle32.adam(pr, go, mr, vr, step, lr=lr, weight_decay=wd)
    # bars of test_hip_kernels.py::test_adam_trajectory_vs_reference; the fused step's gradient and loss are rnvp_loss_grad's bit for bit
    # (::test_fused_train_step_equals_loss_grad_plus_adam)
    np.testing.assert_allclose(o["exp_avg"].cpu().numpy(), mr, rtol=2e-5, atol=3e-6 * np.abs(mr).max())
    np.testing.assert_allclose(o["exp_avg_sq"].cpu().numpy(), vr, rtol=4e-5, atol=6e-6 * np.abs(vr).max())
    assert np.abs(o["params"].cpu().numpy() - pr).mean() < 2e-6
    assert hygiene.same_bits(o["grad"], g1)
    assert abs(float(o["loss"]) - lo) < max(1e-5, 5e-7 * abs(lo))


# ---- rnvp_backward_cond, rnvp_inverse_backward -------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 65, 70001])
@pytest.mark.parametrize("form,hidden", [("lmm16", (12, 20)), ("valu", (512,))])
def test_condition_and_inverse_backward_do_not_depend_on_the_workspace(form, hidden, n):
    """the any-shape 16-row MFMA kernel (gradient of the conditions through the `gcw` partials) and the VALU kernel behind it
    (hidden = (512,): the tile image exceeds the LDS budget) against torch autograd over the float64 restatement oracle/torch_cpu.py"""
    from oracle.torch_cpu import EagerFlow
    if form == "valu" and n > 1000:
        n = 4097             # one thread per row through 512 hidden units: the float64 restatement of 70 001 rows takes a minute
    L, d, c = 2, 6, 2
    f = _Flow(L, d, c, hidden, alt=1)
    _hip, P = f.hip, f.P
    X, C = f.data(_prime_rows(n))
    xd, cd = _dev(X), _dev(C)
    gz_np = f.rng.standard_normal((_prime_rows(n), d)).astype(np.float32) / n
    gld_np = f.rng.standard_normal(_prime_rows(n)).astype(np.float32) / n
    gzd, gldd = _dev(gz_np), _dev(gld_np)
    ref = EagerFlow(L, d, c, hidden, "tanh").double()
    ref.load_flat(f.params_np.astype(np.float64))
    ref.masks = [torch.from_numpy(m.astype(np.int64)) for m in f.masks_np]
    f.ws_bytes = lambda op, rows: _hip.backward_cond_workspace_bytes(f.shape, rows)
    assert f.ws_bytes(None, n) > 0

    def ref_grads(fn, a, b, seeds):
        for p in ref.parameters():
            p.grad = None
        a = torch.from_numpy(a[:n].astype(np.float64)).requires_grad_(True)
        b = torch.from_numpy(b[:n].astype(np.float64)).requires_grad_(True)
        outs = fn(a, b)
        outs = outs if isinstance(outs, tuple) else (outs,)
        sum((o * s).sum() for o, s in zip(outs, seeds)).backward()
        gp = []
        for t, s in zip(ref.nets_t, ref.nets_s):
            gp += [p.grad.reshape(-1) for p in list(t.parameters()) + list(s.parameters())]
        return torch.cat(gp), a.grad, b.grad

    def close(got, want, what):          # test_autograd_gpu.py::_close, TOL = 3e-6 of the gradient's scale
        scale = max(float(want.abs().max()), 1e-30)
        err = float((got.double().cpu() - want).abs().max()) / scale
        assert err < 3e-6, "%s[%s, %d rows]: %.2e of scale" % (what, form, n, err)

    def backward_cond(rows, ws):
        g, gx, gc = _nan(P), _nan(rows, d), _nan(rows, c)
        _hip.backward_cond(f.shape, f.params, f.masks, xd, cd, None, rows, gzd, gldd, g, gx, gc, ws)
        return dict(grad=g, gx=gx, gc=gc)

    o = _settle(_per_pattern(f, None, n, backward_cond), "rnvp_backward_cond[%s, %d rows]" % (form, n))

    def fwd(x, cc):                      # z and log det of EagerFlow.log_prob_rows, before the prior
        ld = torch.zeros(x.shape[0], dtype=torch.float64)
        for l in range(L):
            m = ref.masks[l].double()
            xm = torch.cat([x * m, cc], 1)
            s, t = ref.nets_s[l](xm), ref.nets_t[l](xm)
            x = x * m + (1 - m) * (x * torch.exp(s) + t)
            ld = ld + ((1 - m) * s).sum(1)
        return x, ld

    gp, ga, gb = ref_grads(fwd, X, C, (torch.from_numpy(gz_np[:n]).double(), torch.from_numpy(gld_np[:n]).double()))
    close(o["grad"], gp, "d params"); close(o["gx"], ga, "d x"); close(o["gc"], gb, "d c")

    def inverse_backward(rows, ws):
        g, gzo, gc = _nan(P), _nan(rows, d), _nan(rows, c)
        _hip.inverse_backward(f.shape, f.params, f.masks, xd, cd, rows, gzd, g, gzo, gc, ws)
        return dict(grad=g, gz=gzo, gc=gc)

    o = _settle(_per_pattern(f, None, n, inverse_backward), "rnvp_inverse_backward[%s, %d rows]" % (form, n))
    gp, ga, gb = ref_grads(lambda zz, cc: ref.inverse_rows(zz, cc), X, C, (torch.from_numpy(gz_np[:n]).double(),))
    close(o["grad"], gp, "d params"); close(o["gz"], ga, "d z"); close(o["gc"], gb, "d c")


# ---- rnvp_fit_epoch, rnvp_fit_epochs ---------------------------------------------------------------------------------------------------
# id: (L, d, c, hidden, alt_masks, family, n, batch_size): a ragged last batch, a one-row last batch
FIT_CASES = {
    "resident":        (4, 5, 3, (10,), 1, "auto", 97, 32),          # one persistent launch per call
    "resident_1row":   (4, 5, 3, (10,), 1, "auto", 65, 32),
    "chained":         (2, 16, 4, (16,), 1, "auto", 2 * 300 + 77, 300),
    "chained_1row":    (2, 16, 4, (16,), 1, "auto", 2 * 9000 + 1, 9000),     # row-parallel batches, then one row on the tile-split kernel
    "lmm":             (2, 6, 2, (12, 20), 0, "lmm", 2 * 300 + 77, 300),
    "lmm_1row":        (2, 6, 2, (12, 20), 0, "lmm", 2 * 9000 + 1, 9000),    # 64-row blocks, then one row
    "valu":            (2, 6, 2, (12, 20), 0, "valu", 2 * 300 + 1, 300),
}


@pytest.mark.parametrize("entry", ["fit_epoch", "fit_epochs"])
@pytest.mark.parametrize("case", list(FIT_CASES))
def test_fit_epoch_calls_do_not_depend_on_the_workspace(case, entry, oracle32):
    L, d, c, hidden, alt, family, n, bs = FIT_CASES[case]
    f = _Flow(L, d, c, hidden, alt=alt, family=family)
    _hip, P = f.hip, f.P
    assert _hip.fit_epoch_resident(f.shape, bs) == case.startswith("resident")
    n_epochs = 2 if entry == "fit_epochs" else 1
    X, C = f.data(2 * n)
    xd, cd = _dev(X), _dev(C)
    lr, wd = 0.01, 0.05
    nb = (n + bs - 1) // bs

    def call(rows, ws):
        big = rows != n                    # the priming call: twice the rows in batches twice as large, another shuffle
        n_, bs_ = (2 * n, 2 * bs) if big else (n, bs)
        g = torch.Generator().manual_seed(11 + big)
        perms = torch.stack([torch.randperm(n_, generator=g) for _ in range(n_epochs)]).cuda()
        p, m, v = f.params.clone(), torch.zeros(P, device="cuda"), torch.zeros(P, device="cuda")
        gb, hist = _nan(P), _nan(n_epochs, (n_ + bs_ - 1) // bs_)
        if entry == "fit_epochs":
            _hip.fit_epochs(f.shape, p, f.masks, xd, cd, perms, n_, bs_, n_epochs, gb, hist, m, v, lr, 0.9, 0.999, 1e-8, wd, 1, ws)
        else:
            _hip.fit_epoch(f.shape, p, f.masks, xd, cd, perms[0].contiguous(), n_, bs_, gb, hist[0], m, v, lr, 0.9, 0.999, 1e-8, wd, 1, ws)
        return dict(params=p, exp_avg=m, exp_avg_sq=v, loss_hist=hist, perms=perms.float())

    f_ws = f.ws_bytes
    f.ws_bytes = lambda op, rows: f_ws(op, 2 * bs if rows != n else bs)
    o = _settle(_per_pattern(f, _hip.OP_TRAIN, n, call), "rnvp_%s[%s]" % (entry, case))
    # the epoch restated with the float32 oracle: per batch loss + gradient, then Adam
    perms = o["perms"].long().cpu().numpy()
    pr, mr, vr = f.params_np.copy(), np.zeros(P, np.float32), np.zeros(P, np.float32)
    hist = []
    for e in range(n_epochs):
        for k in range(nb):
            rows = perms[e][k * bs:(k + 1) * bs]
            lo, go = oracle32.loss_grad(f.oshape, pr, X[rows], None if C is None else C[rows], f.masks_np)
            oracle32.adam(pr, go, mr, vr, e * nb + k + 1, lr=lr, weight_decay=wd)
            hist.append(lo)
    # bars of test_hip_kernels.py::test_adam_trajectory_vs_reference
    np.testing.assert_allclose(o["exp_avg"].cpu().numpy(), mr, rtol=2e-5, atol=3e-6 * np.abs(mr).max())
    np.testing.assert_allclose(o["exp_avg_sq"].cpu().numpy(), vr, rtol=4e-5, atol=6e-6 * np.abs(vr).max())
    assert np.abs(o["params"].cpu().numpy() - pr).mean() < 2e-6
    np.testing.assert_allclose(o["loss_hist"].cpu().numpy().reshape(-1), np.array(hist), rtol=5e-5, atol=5e-5)


# ---- torch's CPU generator streams on the device: rnvp_randperm_torch_cpu, rnvp_prior_normal_torch_cpu ----------------------------------
def _twister(seed, skip=0):
    from probaforms_amd.models.nflow import HostStreamOnDevice
    g = torch.Generator(); g.manual_seed(seed)
    if skip:
        torch.rand(skip, generator=g)                  # start at an arbitrary position of a block
    ref = torch.Generator(); ref.set_state(g.get_state())
    _, mt = HostStreamOnDevice._unpack(g)
    return torch.from_numpy(mt.copy()).cuda(), ref


@pytest.mark.parametrize("n", [2, 2049, 1_000_003])        # (the tail alone; one block + tail; several rounds of the grid)
def test_randperm_does_not_depend_on_the_workspace(n):
    """torch.randperm bit for bit, values and the advanced twister state, as tests/test_randperm_gpu.py checks it"""
    from probaforms_amd import _hip
    outs = {}
    for pat in hygiene.PATTERNS:
        big = 2 * n + 5
        ws = hygiene.workspace(_hip.randperm_workspace_bytes(big if pat == "replay" else n), pat)
        if pat == "replay":
            mt, _ = _twister(77)
            _hip.randperm_torch_cpu(mt, big, torch.empty(big, dtype=torch.int64, device="cuda"), ws)
        mt, ref_g = _twister(12345)
        out = torch.empty(n, dtype=torch.int64, device="cuda")
        hygiene.poison_outputs(out)
        _hip.randperm_torch_cpu(mt, n, out, ws)
        torch.cuda.synchronize()
        outs[pat] = dict(perm=out, mt_state=mt)
    o = _settle(outs, "rnvp_randperm_torch_cpu[%d]" % n)
    assert torch.equal(o["perm"].cpu(), torch.randperm(n, generator=ref_g))


@pytest.mark.parametrize("n", [17, 2049, 1_000_003])      # (torch.randn takes its 16-element blocks from 16 numbers on)
def test_torch_prior_stream_does_not_depend_on_the_workspace(n):
    """torch.randn of the CPU generator bit for bit, as tests/test_prior_torch.py::test_device_draw_equals_torch_randn checks it"""
    from probaforms_amd import _hip
    from probaforms_amd.models.nflow import HostStreamOnDevice as H
    if not H.usable("cuda"):
        pytest.skip("device draw not validated on this host")          # (as tests/test_prior_torch.py)
    outs = {}
    nb = _hip.prior_torch_workspace_bytes()
    for pat in hygiene.PATTERNS:
        ws = hygiene.workspace(nb, pat)
        if pat == "replay":
            mt, _ = _twister(78, 5)
            _hip.prior_normal_torch_cpu(mt, 2 * n + 5, torch.empty(2 * n + 5, device="cuda"), torch.zeros(16, device="cuda"), ws)
        mt, ref_g = _twister(99 + n % 1000, n % 700)
        out, tail = _nan(n), hygiene.workspace(64, pat).view(torch.float32)       # tail16 is device scratch (rnvp_hip.h): poisoned alike
        _hip.prior_normal_torch_cpu(mt, n, out, tail, ws)
        torch.cuda.synchronize()
        outs[pat] = dict(z=out, mt_state=mt)
    o = _settle(outs, "rnvp_prior_normal_torch_cpu[%d]" % n)
    assert torch.equal(o["z"].cpu().view(torch.int32), torch.randn(n, generator=ref_g).view(torch.int32))
