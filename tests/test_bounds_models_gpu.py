"""No entry point of libpf_wgan.so, libpf_cnormal.so, libpf_gendraw.so and libpf_predict.so, and none of the cvae_* calls of
librnvp_hip.so, writes outside its workspace or its outputs (tests/bounds.py has the driver, tests/hygiene.py the guard bands).  Every
call gets a workspace of exactly what its own size function returns for the call's rows and every output, the in-place ones (params,
optimizer state, running moments) included, a guarded buffer of its own.  Correctness stays in the entry points' own test modules.

entry point (size function)                              cases
  pfw_loss_grad, pfw_train_step (pfw_workspace_bytes)    both step kinds at W_CASES: the small rows of tilings_cases.W_STEPS on cap1, cap2,
                                                         big_lds and cap13 and two everyday shapes; all but (full_wg, 4097) run at
                                                         G == step_wg_bound and must write the last slab of gpart and the last loss partial
  pfw_epoch_losses                                       one tile, a row more, three tiles and a row (eloss_tile rows each)
  pfw_fit_epoch                                          two batches and a one-row batch, with the epoch-end losses (epart is last)
  pfw_generate, pfw_critic (no workspace)                outputs and inputs, gen_only (tile 1) included
  pfn_loss_grad, pfn_train_step (pfn_workspace_bytes)    N_CASES: the small rows of tilings_cases.N_STEPS on cap1, cap3, big_lds, cap11 and
                                                         full_wg, full and independent covariance; the error words are the last sub-buffer
                                                         (cap1 and cap3, millions of weights per thread: pfn_train_step alone, the same k_step)
  pfn_fit_epoch                                          two batches and a one-row batch
  pfn_forward (no workspace)                             every output, 1 / 255 / 257 rows
  pfg_mlp_draw_accumulate (pfg_workspace_bytes)          test_gendraw_gpu.MLP_CASES (WIDE: weights read from the workspace), 19 and 65 draws
  pfg_affine_draw_accumulate (no workspace)              d = 1, 17, 32, full and independent
  pfp_draw_accumulate (pfp_workspace_bytes)              seeds (the workspace holds them) and given z (no interior byte may change); its
                                                         outputs are guarded by tests/test_predict_edges_gpu.py, here once more
  cvae_encode, cvae_decode, cvae_loss_grad,              the three kernel families of test_workspace_hygiene_libs_gpu.CVAE_FORMS at
  cvae_train_step (cvae_workspace_bytes)                 1 / 63 / 65 / 5000 / 70001 rows; the chained family at 131 073 rows, its grid bound
  cvae_fit_epoch                                         that module's epoch cases, the resident ones included

Grid bounds.  pf_rowtile::step_wg_bound is reached by every W_CASES / N_CASES entry marked so (asserted through pfw_tiling /
pfn_tiling before anything runs).  cvae_mfma.hip sizes hsave, its last sub-buffer, for min(kMaxGrid = 512, ceil(rows / 256)) workgroups in
hsave_bytes() and clamps the launch on its own: 131 073 rows are 513 row groups, and the call must write workgroup 511's slab.
Where the cvae_* workspaces end.  cvae_workspace_bytes is the largest of three kernel families' figures plus an error-word block, so
the family that runs may end short of it; _cvae_end restates where.  Asserted: cvae_loss_grad, cvae_train_step and cvae_fit_epoch on
the chained kernels end inside hsave (at 1 to 5000 rows that is the end of the workspace less the block), on one thread per row inside
losspart [256]; cvae_encode and cvae_decode keep their family's packed weights alone, or nothing, and end in front of that
sub-buffer; the resident epoch is handed no workspace at all and may change no interior byte.  Printed, not asserted: the any-shape
MFMA family (lmm), whose last sub-buffer, kSplits x the decoder's gnet_floats, is a sum over every layer's padded tiles
(make_cvae_l) that no query exports; its mark sits at need - 256 from 5000 rows on (profiles/r26_bounds_high_water.txt).
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bounds  # noqa: E402
import native_libs  # noqa: E402
import tilings_cases as tc  # noqa: E402
from bounds import Out, align256  # noqa: E402
from probaforms_amd.models import _cnormal_lib as NL, _gendraw_lib as GL, _predict_lib as PL, _wgan_lib as W  # noqa: E402

pytestmark = pytest.mark.gpu

native_libs.ensure_built(W, NL, GL, PL)

F32, I32, I64, U8 = torch.float32, torch.int32, torch.int64, torch.uint8


def _dev(a, dtype=F32):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a)).to(dtype).cuda().contiguous()


# ---- ConditionalWGAN --------------------------------------------------------------------------------------------------------------
# (shape name, batch rows, runs at G == step_wg_bound)
W_CASES = [("big_lds", 1, True), ("big_lds", 9, True), ("big_lds", 33, True), ("cap2", 1, True), ("cap2", 3, True), ("cap2", 5, True),
           ("cap1", 1, True), ("cap1", 3, True), ("cap13", 3400, True), ("full_wg", 50, True), ("odd_cap", 65, True),
           ("full_wg", 4097, False)]


def _wshape(name):
    dims, ga, da = tc.W_SHAPES[name]
    return W.Shape.make(*dims, ga, da), dims


@pytest.mark.parametrize("name,rows,at_bound", W_CASES, ids=["%s-%d" % c[:2] for c in W_CASES])
def test_wgan_steps(name, rows, at_bound):
    shape, (d, c, lat, gh, dh) = _wshape(name)
    info = W.tiling(shape, rows)
    G, Gb = int(info.step_wgs), int(info.step_wg_bound)
    assert (G == Gb) == at_bound and G <= Gb, (G, Gb)
    PG, PD = W.param_count(shape, W.NET_G), W.param_count(shape, W.NET_D)
    P = PG + PD
    p, X, C, ri, z = tc.wgan_problem(name, rows, int(info.step_tile))
    p0, Xd, Cd, idx, zd = _dev(p), _dev(X), _dev(C), _dev(ri, I64), _dev(z)
    v0 = torch.rand(P, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3)) * 1e-4
    inputs = dict(X=Xd, z=zd, row_index=idx)
    if Cd is not None:
        inputs["C"] = Cd
    need = W.workspace_bytes(shape, rows)
    a = align256(Gb * P * 4)
    assert need == a + align256(Gb * 4)                          # gpart [G][P], lpart [G]; no epoch losses
    opt = W.rmsprop(1e-3, weight_decay=0.001, clamp=0.01)
    for kind in (W.STEP_GEN, W.STEP_CRITIC):
        Pk = PD if kind else PG
        reach = [((G - 1) * P * 4, G * P * 4, "the last workgroup's slab of gpart"), (a + 4 * (G - 1), a + 4 * G, "the last loss partial")]
        tag = "[%s, %d rows, kind %d, G %d of %d]" % (name, rows, kind, G, Gb)
        bounds.run("pfw_train_step" + tag, need,
                   lambda ws, o: W.train_step(shape, kind, o["params"], o["square_avg"], Xd, Cd, idx, zd, rows, opt, o["grad"], o["loss"], ws),
                   dict(params=Out(F32, (P,), p0), square_avg=Out(F32, (P,), v0), grad=Out(F32, (Pk,)), loss=Out(F32, (1,))), inputs,
                   last=4 * Gb, reach=reach)
        bounds.run("pfw_loss_grad" + tag, need,
                   lambda ws, o: W.loss_grad(shape, kind, p0, Xd, Cd, idx, zd, rows, o["grad"], o["loss"], ws),
                   dict(grad=Out(F32, (Pk,)), loss=Out(F32, (1,))), dict(inputs, params=p0), last=4 * Gb, reach=reach)


@pytest.mark.parametrize("name", ["full_wg", "big_lds", "cap1"])
def test_wgan_epoch_losses_and_fit_epoch(name):
    from probaforms_amd.models.wgan import step_kinds
    shape, (d, c, lat, gh, dh) = _wshape(name)
    T = int(W.tiling(shape, 1).eloss_tile)
    P = W.param_count(shape, W.NET_G) + W.param_count(shape, W.NET_D)
    nmax = 3 * T + 1
    p, X, C, ri, z = tc.wgan_problem(name, nmax, 8, seed=5)
    p0, Xd, Cd, zd = _dev(p), _dev(X), _dev(C), _dev(z)
    inputs = dict(params=p0, X=Xd, z_full=zd)
    if Cd is not None:
        inputs["C"] = Cd
    for n in (1, T, T + 1, nmax):
        E = -(-n // T)
        bounds.run("pfw_epoch_losses[%s, %d rows, %d tiles of %d]" % (name, n, E, T), W.workspace_bytes(shape, 0, n),
                   lambda ws, o: W.epoch_losses(shape, p0, Xd, Cd, zd, n, o["epoch_losses"], ws),
                   dict(epoch_losses=Out(F32, (2,))), inputs, last=8 * E)
    B = 7 if name == "full_wg" else 2
    n = 2 * B + 1
    perm = _dev(np.random.default_rng(9).permutation(n), I64)
    v0 = torch.rand(P, device="cuda", generator=torch.Generator(device="cuda").manual_seed(4)) * 1e-4
    opt = W.rmsprop(1e-3, weight_decay=0.001, clamp=0.01)
    kinds = step_kinds(1, 3, 2)
    zb = zd[:n].contiguous()
    bounds.run("pfw_fit_epoch[%s, %d rows in batches of %d]" % (name, n, B), W.workspace_bytes(shape, B, n),
               lambda ws, o: W.fit_epoch(shape, o["params"], o["square_avg"], Xd, Cd, perm, zb, zb, n, B, kinds, opt, o["epoch_losses"], ws),
               dict(params=Out(F32, (P,), p0), square_avg=Out(F32, (P,), v0), epoch_losses=Out(F32, (2,))),
               dict({k: v for k, v in inputs.items() if k != "params"}, perm=perm, z_batches=zb), last=8 * -(-n // T))


@pytest.mark.parametrize("n", [1, 255, 257])
@pytest.mark.parametrize("name", ["full_wg", "big_lds", "gen_only"])
def test_wgan_generate_and_critic(name, n):
    shape, (d, c, lat, gh, dh) = _wshape(name)
    p, X, C, ri, z = tc.wgan_problem(name, n, 8, seed=6)
    p0, Xd, Cd, zd = _dev(p), _dev(X), _dev(C), _dev(z)
    inputs = dict(params=p0, X=Xd, z=zd)
    if Cd is not None:
        inputs["C"] = Cd
    bounds.run_outputs("pfw_generate[%s, %d rows]" % (name, n), lambda o: W.generate(shape, p0, zd, Cd, n, o["out"]), dict(out=Out(F32, (n, d))), inputs)
    bounds.run_outputs("pfw_critic[%s, %d rows]" % (name, n), lambda o: W.critic(shape, p0, Xd, Cd, n, o["out"]), dict(out=Out(F32, (n,))), inputs)


# ---- ConditionalNormal -----------------------------------------------------------------------------------------------------------------
N_CASES = [("big_lds", 1, True), ("big_lds", 9, True), ("big_lds", 33, True), ("cap3", 1, True), ("cap3", 5, True), ("cap1", 3, True),
           ("full_wg", 50, True), ("cap11", 65, True), ("big_lds", 2049, False)]


def _nshape(name):
    d, c, hidden, act, indep = tc.N_SHAPES[name]
    return NL.Shape.make(d, c, hidden, act, indep), d, c


@pytest.mark.parametrize("name,rows,at_bound", N_CASES, ids=["%s-%d" % c[:2] for c in N_CASES])
def test_cnormal_steps(name, rows, at_bound):
    shape, d, c = _nshape(name)
    info = NL.tiling(shape, rows)
    G, Gb = int(info.step_wgs), int(info.step_wg_bound)
    assert (G == Gb) == at_bound and G <= Gb, (G, Gb)
    P = NL.param_count(shape)
    p, X, C, ri = tc.cnormal_problem(name, rows, int(info.step_tile))
    p0, Xd, Cd, idx = _dev(p), _dev(X), _dev(C), _dev(ri, I64)
    inputs = dict(X=Xd, C=Cd, row_index=idx)
    need = NL.workspace_bytes(shape, rows)
    a, b = align256(Gb * P * 4), align256(Gb * 4)
    assert need == a + b + 32 * 32 * 4 + 256                     # gpart [G][P], lpart [G], the inverse of out.weight, the error words
    reach = [((G - 1) * P * 4, G * P * 4, "the last workgroup's slab of gpart"), (a + 4 * (G - 1), a + 4 * G, "the last loss partial")]
    zeros = torch.zeros(P, device="cuda")
    opt = NL.adam(1e-3, weight_decay=0.01)
    tag = "[%s, %d rows, G %d of %d]" % (name, rows, G, Gb)
    bounds.run("pfn_train_step" + tag, need,
               lambda ws, o: NL.train_step(shape, o["params"], o["exp_avg"], o["exp_avg_sq"], Xd, Cd, idx, rows, opt, 2, o["grad"], o["loss"],
                                           o["status"], ws),
               dict(params=Out(F32, (P,), p0), exp_avg=Out(F32, (P,), zeros), exp_avg_sq=Out(F32, (P,), zeros), grad=Out(F32, (P,)),
                    loss=Out(F32, (1,)), status=Out(I32, (1,))), inputs, last=8, reach=reach)
    if P > 2_000_000:                # cap1, cap3: a step of these is one thread through millions of weights; the fused call covers the others' kernel
        return
    bounds.run("pfn_loss_grad" + tag, need,
               lambda ws, o: NL.loss_grad(shape, p0, Xd, Cd, idx, rows, o["grad"], o["loss"], o["status"], ws),
               dict(grad=Out(F32, (P,)), loss=Out(F32, (1,)), status=Out(I32, (1,))), dict(inputs, params=p0), last=8, reach=reach)
    bounds.run("pfn_loss_grad" + tag + ", no status", need,                  # the call's sticky word then lives in the workspace: err[1]
               lambda ws, o: NL.loss_grad(shape, p0, Xd, Cd, idx, rows, o["grad"], o["loss"], None, ws),
               dict(grad=Out(F32, (P,)), loss=Out(F32, (1,))), dict(inputs, params=p0), last=8)


@pytest.mark.parametrize("name", ["full_wg", "big_lds", "cap11"])         # (the epoch is the loop of the steps above: cap1 / cap3 run there)
def test_cnormal_fit_epoch(name):
    shape, d, c = _nshape(name)
    P = NL.param_count(shape)
    B = 7 if name == "full_wg" else 2
    n = 2 * B + 1
    p, X, C, ri = tc.cnormal_problem(name, n, 8, seed=5)
    p0, Xd, Cd, perm = _dev(p), _dev(X), _dev(C), _dev(ri, I64)
    zeros = torch.zeros(P, device="cuda")
    opt = NL.adam(1e-3, weight_decay=0.01)
    bounds.run("pfn_fit_epoch[%s, %d rows in batches of %d]" % (name, n, B), NL.workspace_bytes(shape, B),
               lambda ws, o: NL.fit_epoch(shape, o["params"], o["exp_avg"], o["exp_avg_sq"], Xd, Cd, perm, n, B, opt, 1, o["losses"], o["status"], ws),
               dict(params=Out(F32, (P,), p0), exp_avg=Out(F32, (P,), zeros), exp_avg_sq=Out(F32, (P,), zeros), losses=Out(F32, (3,)),
                    status=Out(I32, (1,))), dict(X=Xd, C=Cd, perm=perm), last=8)


@pytest.mark.parametrize("n", [1, 255, 257])
@pytest.mark.parametrize("name", ["full_wg", "big_lds", "cap1", "wide_fwd"])
def test_cnormal_forward(name, n):
    shape, d, c = _nshape(name)
    p, X, C, ri = tc.cnormal_problem(name, n, 8, seed=6)
    p0, Xd, Cd = _dev(p), _dev(X[:n]), _dev(C[:n])
    eps = torch.randn(n, d, device="cuda", generator=torch.Generator(device="cuda").manual_seed(8))
    bounds.run_outputs("pfn_forward[%s, %d rows]" % (name, n),
                       lambda o: NL.forward(shape, p0, Cd, eps, Xd, n, o["mu"], o["sigma"], o["x_tilde"], o["inv"], o["status"]),
                       dict(mu=Out(F32, (n, d)), sigma=Out(F32, (n, d)), x_tilde=Out(F32, (n, d)), inv=Out(F32, (n, d)), status=Out(I32, (1,))),
                       dict(params=p0, C=Cd, eps=eps, X=Xd))


# ---- the generators' multi-draw statistics ------------------------------------------------------------------------------------------------
import test_gendraw_gpu as tg  # noqa: E402

STATE = ("state",)             # running moments as raw bytes, updated in place from zeros: any byte value is a legitimate one


@pytest.mark.parametrize("K", [19, 65])
@pytest.mark.parametrize("case", tg.MLP_CASES, ids=tg._ids)
def test_mlp_draw_accumulate(case, K):
    net, _, params, Cn, z = tg._setup(case, K)
    d = case[0]
    N, N_TOTAL, ROW0 = tg.N, tg.N_TOTAL, tg.ROW0
    Cd, zd = _dev(Cn), _dev(z)
    plan = GL.plan(net, K)
    inputs = dict(params=params, z=zd)
    if Cd is not None:
        inputs["C"] = Cd
    state0 = PL.new_state(N, d, "cuda")
    bounds.run("pfg_mlp_draw_accumulate[%s, %d draws, weights %s]" % (tg._ids(case), K, "in LDS" if plan.weights_in_lds else "in the workspace"),
               GL.workspace_bytes(net, K),
               lambda ws, o: GL.mlp_draw_accumulate(net, params, Cd, N, ROW0, zd, N_TOTAL, 0, K, K, o["state"], o["x"], o["xt"], ws),
               dict(state=Out(U8, (N, d, PL.STATE_BYTES), state0), x=Out(F32, (K, N, d)), xt=Out(F32, (N, d, K))), inputs,
               last=int(plan.packed_bytes), allow=STATE)


@pytest.mark.parametrize("d,independent", [(1, False), (17, False), (32, False), (17, True)])
def test_affine_draw_accumulate(d, independent):
    N, N_TOTAL, ROW0, K = tg.N, tg.N_TOTAL, tg.ROW0, 19
    g = torch.Generator(device="cuda").manual_seed(d)
    mu, sigma = torch.randn(N, d, device="cuda", generator=g), torch.rand(N, d, device="cuda", generator=g) + 0.5
    Wo = None if independent else torch.randn(d, d, device="cuda", generator=g)
    bo = None if independent else torch.randn(d, device="cuda", generator=g)
    eps = torch.randn(K, N_TOTAL, d, device="cuda", generator=g)
    inputs = dict(mu=mu, sigma=sigma, eps=eps)
    if not independent:
        inputs.update(out_w=Wo, out_b=bo)
    state0 = PL.new_state(N, d, "cuda")
    bounds.run_outputs("pfg_affine_draw_accumulate[d %d%s]" % (d, ", independent" if independent else ""),
                       lambda o: GL.affine_draw_accumulate(d, mu, sigma, Wo, bo, eps, N, ROW0, N_TOTAL, 0, K, K, o["state"], o["x"], o["xt"]),
                       dict(state=Out(U8, (N, d, PL.STATE_BYTES), state0), x=Out(F32, (K, N, d)), xt=Out(F32, (N, d, K))), inputs, allow=STATE)


@pytest.mark.parametrize("K", [1, 19, 65])
@pytest.mark.parametrize("form", ["chained", "lmm"])
def test_flow_draw_accumulate(form, K):
    from test_workspace_hygiene_gpu import _Flow
    f = _Flow(2, 16, 4, (32,)) if form == "chained" else _Flow(2, 6, 2, (12, 20), alt=0)
    N, N_TOTAL, ROW0, d = tg.N, tg.N_TOTAL, tg.ROW0, f.d
    need = PL.workspace_bytes(f.shape, K)
    assert need == align256(8 * K)                              # the seeds, copied for the launch
    _, C = f.data(N)
    Cd = _dev(C)
    z = torch.randn(K, N_TOTAL, d, device="cuda", generator=torch.Generator(device="cuda").manual_seed(K))
    state0 = PL.new_state(N, d, "cuda")
    outs = dict(state=Out(U8, (N, d, PL.STATE_BYTES), state0), x=Out(F32, (K, N, d)), xt=Out(F32, (N, d, K)))
    inputs = dict(params=f.params, masks=f.masks, C=Cd)
    held = []
    bounds.run("pfp_draw_accumulate[%s, %d draws, seeds]" % (form, K), need,
               lambda ws, o: held.append(PL.draw_accumulate(f.shape, f.params, f.masks, Cd, N, ROW0, list(range(100, 100 + K)), None, N_TOTAL, 0, K, K,
                                                            o["state"], o["x"], o["xt"], ws)),
               outs, inputs, last=8 * K, allow=STATE)
    bounds.run("pfp_draw_accumulate[%s, %d draws, z given]" % (form, K), need,
               lambda ws, o: PL.draw_accumulate(f.shape, f.params, f.masks, Cd, N, ROW0, None, z, N_TOTAL, 0, K, K, o["state"], o["x"], o["xt"], ws),
               outs, dict(inputs, z=z), keeps_nothing=True, allow=STATE)


# ---- CVAE ---------------------------------------------------------------------------------------------------------------------------------
import test_workspace_hygiene_libs_gpu as hl  # noqa: E402


CVAE_MFMA_ROWS_PER_WG = 4 * 4 * 16      # cvae_mfma.hip: kWaves x kR row tiles x 16 rows
CVAE_MFMA_MAX_GRID = 512                # its kMaxGrid: hsave_bytes() and the launch each clamp their workgroups to it
CVAE_CASES = [(form, n) for form in hl.CVAE_FORMS for n in (1, 63, 65, 5000, 70001)]
CVAE_CASES.append(("mfma", CVAE_MFMA_MAX_GRID * CVAE_MFMA_ROWS_PER_WG + 1))          # 513 row groups: the smallest call the clamp cuts


def _cvae_end(_hip, shape, form, hidden, rows, need, P):
    """-> (last= / tail= of bounds.run for cvae_loss_grad / cvae_train_step on `rows` rows, the byte at which the family's last
    sub-buffer starts, one workgroup's bytes of it); cvae_workspace_bytes is the largest of the three families' figures, so the
    family that runs may end short of `need` by a tail that is restated here"""
    if form == "mfma":                   # packed weights, gpart [512], losspart [512 x 4], then hsave: per workgroup 4 waves x 2 nets x HT tiles x 4 row tiles KiB
        per_wg = 4 * 2 * -(-hidden[0] // 16) * 4 * 256 * 4
        one = _hip.cvae_workspace_bytes(shape, 1)
        assert _hip.cvae_workspace_bytes(shape, CVAE_MFMA_ROWS_PER_WG + 1) - one == per_wg       # this family sets the size of small calls
        start = one - 256 - per_wg
        hsave = min(CVAE_MFMA_MAX_GRID, -(-rows // CVAE_MFMA_ROWS_PER_WG)) * per_wg
        assert start + hsave + 256 <= need
        return dict(last=hsave, tail=need - start - hsave), start, per_wg
    if form == "generic":                # cvae_generic.hip: gpart [256][P], losspart [256], an error-word block
        start = align256(256 * P * 4)
        assert start + 1024 + 256 <= need
        return dict(last=1024, tail=need - start - 1024), start, 4
    return {}, None, None                # lmm: see the docstring


@pytest.mark.parametrize("form,n", CVAE_CASES)
def test_cvae_calls(form, n):
    from probaforms_amd import _hip
    d, c, lat, hidden, act, family, _ = hl.CVAE_FORMS[form]
    shape = _hip.CvaeShape.make(d, c, lat, hidden, act, family=family)
    assert _hip.cvae_kernel_path(shape) == getattr(_hip, hl.CVAE_PATH[form])
    P = _hip.cvae_param_count(shape)
    rng = np.random.default_rng(d * 1000 + n)
    N = n + 5
    p0 = _dev((rng.standard_normal(P) * 0.25).astype(np.float32))
    xd, cd = _dev(rng.standard_normal((N, d)).astype(np.float32)), _dev(rng.standard_normal((N, c)).astype(np.float32))
    ed, idx = _dev(rng.standard_normal((N, lat)).astype(np.float32)), _dev(rng.permutation(N)[:n], I64)
    need = _hip.cvae_workspace_bytes(shape, n)
    tag = "[%s, %d rows]" % (form, n)
    kw, start, per_wg = _cvae_end(_hip, shape, form, hidden, n, need, P)
    reach = ()
    if form == "mfma" and n > CVAE_MFMA_MAX_GRID * CVAE_MFMA_ROWS_PER_WG:      # at the grid bound the last workgroup's record is the buffer's last
        reach = [(start + (CVAE_MFMA_MAX_GRID - 1) * per_wg, start + CVAE_MFMA_MAX_GRID * per_wg, "workgroup 511's slab of hsave")]
    hw = {}
    hw["encode"], _ = bounds.run("cvae_encode" + tag, need, lambda ws, o: _hip.cvae_encode(shape, p0, xd, cd, n, o["mu"], o["log_sigma"], ws),
                                 dict(mu=Out(F32, (n, lat)), log_sigma=Out(F32, (n, lat))), dict(params=p0, x=xd, c=cd))
    hw["decode"], _ = bounds.run("cvae_decode" + tag, need, lambda ws, o: _hip.cvae_decode(shape, p0, ed, cd, n, o["x"], ws),
                                 dict(x=Out(F32, (n, d))), dict(params=p0, z=ed, c=cd))
    inputs = dict(x=xd, c=cd, row_index=idx, eps=ed)
    hw["loss_grad"], _ = bounds.run("cvae_loss_grad" + tag, need,
                                    lambda ws, o: _hip.cvae_loss_grad(shape, p0, xd, cd, idx, ed, n, 1.0 / n, 0.3, o["grad"], o["loss"], ws),
                                    dict(grad=Out(F32, (P,)), loss=Out(F32, (1,))), dict(inputs, params=p0), reach=reach, **kw)
    bounds.run("cvae_loss_grad" + tag + ", loss alone", need,
               lambda ws, o: _hip.cvae_loss_grad(shape, p0, xd, cd, idx, ed, n, 1.0 / n, 0.3, None, o["loss"], ws),
               dict(loss=Out(F32, (1,))), dict(inputs, params=p0))
    zeros = torch.zeros(P, device="cuda")
    hw["train_step"], _ = bounds.run("cvae_train_step" + tag, need,
                                     lambda ws, o: _hip.cvae_train_step(shape, o["params"], xd, cd, idx, ed, n, 1.0 / n, 0.3, o["grad"], o["loss"],
                                                                        o["exp_avg"], o["exp_avg_sq"], 0.01, 0.9, 0.999, 1e-8, 0.1, 2, ws),
                                     dict(params=Out(F32, (P,), p0), exp_avg=Out(F32, (P,), zeros), exp_avg_sq=Out(F32, (P,), zeros),
                                          grad=Out(F32, (P,)), loss=Out(F32, (1,))), inputs, reach=reach, **kw)
    assert hw["loss_grad"] > 0 and hw["train_step"] > 0, hw
    # cvae_encode / cvae_decode are handed the same workspace but keep the packed weights of their family alone (cvae_mfma::forward,
    # lmm::cvae_forward), or nothing (one thread per row): they end in front of the training layout's last sub-buffer
    if form == "generic":
        assert hw["encode"] == 0 == hw["decode"], hw
    else:
        assert 0 < hw["encode"] and 0 < hw["decode"], hw
        if start is not None:
            assert hw["encode"] <= start and hw["decode"] <= start, (hw, start)


@pytest.mark.parametrize("form,n,bs", [("mfma", 2 * 9000 + 1, 9000), ("lmm", 2 * 300 + 77, 300), ("generic", 2 * 300 + 1, 300),
                                       ("resident", 97, 32), ("resident", 65, 32)])
def test_cvae_fit_epoch(form, n, bs):
    from probaforms_amd import _hip
    d, c, lat, hidden, act, family, _ = hl.CVAE_FORMS["mfma" if form == "resident" else form]
    if form == "resident":
        d, c, lat, hidden = 5, 3, 2, (10,)
    shape = _hip.CvaeShape.make(d, c, lat, hidden, act, family=family)
    assert _hip.cvae_fit_epoch_resident(shape, bs) == (form == "resident")
    P = _hip.cvae_param_count(shape)
    rng = np.random.default_rng(n + bs)
    p0 = _dev((rng.standard_normal(P) * 0.25).astype(np.float32))
    xd, cd = _dev(rng.standard_normal((n, d)).astype(np.float32)), _dev(rng.standard_normal((n, c)).astype(np.float32))
    ed, perm = _dev(rng.standard_normal((n, lat)).astype(np.float32)), _dev(rng.permutation(n), I64)
    zeros = torch.zeros(P, device="cuda")
    nb = -(-n // bs)
    need = _hip.cvae_workspace_bytes(shape, bs)
    kw = {} if form == "resident" else _cvae_end(_hip, shape, form, hidden, bs, need, P)[0]
    hw, _ = bounds.run("cvae_fit_epoch[%s, %d rows in batches of %d]" % (form, n, bs), need,
                       lambda ws, o: _hip.cvae_fit_epoch(shape, o["params"], xd, cd, perm, ed, n, bs, 0.3, o["grad"], o["loss_hist"], o["exp_avg"],
                                                         o["exp_avg_sq"], 0.01, 0.9, 0.999, 1e-8, 0.05, 1, ws),
                       dict(params=Out(F32, (P,), p0), exp_avg=Out(F32, (P,), zeros), exp_avg_sq=Out(F32, (P,), zeros), grad=Out(F32, (P,)),
                            loss_hist=Out(F32, (nb,))), dict(x=xd, c=cd, perm=perm, eps=ed),
                       allow=("grad",) if form == "resident" else (), keeps_nothing=form == "resident", **kw)
    # (the resident epoch, resident::cvae_fit_epoch of cvae_generic.hip, is handed neither grad_buf nor the workspace: all of it lives in LDS)
    assert hw > 0 or form == "resident"
