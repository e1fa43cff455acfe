"""No rnvp_* entry point of librnvp_hip.so writes outside its workspace (tests/bounds.py has the driver, tests/hygiene.py the guard
bands).  Every call gets a workspace of exactly what rnvp_workspace_bytes (or the entry point's own query) returns for the call's
rows; the driver also requires all outputs written, inputs unchanged and the bits of a run on a plain workspace.  The outputs of these
calls have their guard bands in tests/test_hip_kernels.py::test_no_kernel_writes_outside_its_output_buffers; they get them here once
more because the driver guards whatever it is given.  Correctness stays in the entry points' own test modules; the forms and cases are
those of tests/test_workspace_hygiene_gpu.py.

entry point (size function)                                     cases
  rnvp_forward_logprob, rnvp_inverse, rnvp_sample                FLOW_FORMS (chained f32, bx3 direct / staged, tile-split, lmm16, valu)
    (rnvp_workspace_bytes, RNVP_OP_FORWARD / _INVERSE)           at 1 / 17 / 257 / 4097 / 70001 rows (tile-split: up to its 4096);
                                                                 chained f32 and both bx3 forms at 524 289 rows, their grid bound
  rnvp_loss_grad, rnvp_loss_grad_zseed, rnvp_backward,           TRAIN_FORMS (chained c2 / c3 / c4 / cdim 0, lmm16, lmm64, valu) at
  rnvp_train_step (rnvp_workspace_bytes, RNVP_OP_TRAIN)          1 / 17 / 33 / 8191 / 8193 / 70001 rows (rnvp_backward where it is served)
  rnvp_backward_cond, rnvp_inverse_backward                      lmm16 and valu (hidden 512) at 1 / 65 / 4097 rows
    (rnvp_backward_cond_workspace_bytes)
  rnvp_fit_epoch, rnvp_fit_epochs, rnvp_fit_epoch_dp,            FIT_CASES: resident, resident with a one-row batch, chained, lmm, valu; and
  rnvp_fit_epoch_dp_cb, rnvp_fit_epoch_dp_cb_chunked             resident-deep (two hidden layers); the data-parallel epochs as one rank:
    (RNVP_OP_TRAIN at the batch size)                            without a communicator, and with a caller's exchange in one and two chunks
  rnvp_randperm_torch_cpu (rnvp_randperm_workspace_bytes)        2 / 2049 / 1 000 003 entries
  rnvp_prior_normal_torch_cpu (rnvp_prior_torch_workspace_bytes) 17 / 2049 / 1 000 003 values

Where the workspace ends.  rnvp_workspace_bytes adds one unused 256-byte block to the family's own figure.  Asserted, per entry point:
  * rnvp_forward_logprob keeps its log-prob partials last ([kMaxGrid][kWaves] = 2048 x 4 chained and bx3, [4096] lmm, [512] valu): the
    mark lies there in every case, and at 524 289 rows, where rnvp_last_dispatch shows the grid cut off at 2048 (1024 workgroups of 8
    waves for the staged bx3 form), it is the buffer's last byte.  The lmm and valu kernels stride a grid of at most 4096 / 512
    workgroups, which 70001 rows reach.
  * rnvp_inverse, rnvp_sample: the size is the forward call's, but the partials are not handed to these kernels: the mark must be
    positive and end in front of the partials (the packed weights); one thread per row packs nothing and must write nothing.
  * the training calls, rnvp_backward_cond / rnvp_inverse_backward and the five epoch calls on one thread per row (valu): gpart
    [256][P], losspart [256] and the saved layer inputs [256][L][d][256], sized by kMaxGridTrain = 256 of rnvp_generic.hip (70001 rows
    run at that grid): the mark lies in the saved inputs.
  * rnvp_loss_grad, rnvp_loss_grad_zseed, rnvp_train_step and the epoch calls on the register-chained kernels: packed weights, partials and loss partials of kMaxGridTrain = 512
    workgroups, then the waves' saved activations, 512 x 4 waves x L x 1024 floats (_training_end restates it): the mark lies in the
    saved activations, also where the shared size is the any-shape kernels' larger figure.  70001 rows run at the grid bound, 512, or
    256 workgroups of 8 waves for d in (16, 32], asserted through rnvp_last_dispatch.
  * the resident epochs (resident::fit_epoch) are handed no workspace at all: no interior byte may change.
  * rnvp_randperm_torch_cpu: the twister's workspace is last, and a draw of more than a million words reaches the jumped segments'
    states behind its state_in; rnvp_prior_normal_torch_cpu: the same segments' states at 1 000 003 values (a draw of one segment
    writes state_in alone, so 17 and 2049 values end there by construction).
Printed, not asserted, each with its reason:
  * the any-shape MFMA kernels (lmm16, lmm64) in the training calls, rnvp_backward_cond / rnvp_inverse_backward and the epoch calls:
    and in rnvp_backward of the chained forms, which they serve (see test_training_calls);
    their last sub-buffers (kSplits x L x 2 x gnet_floats split partials; grid64 x nnets x nunits x kUnitFloats) are sums over the
    padded tiles of every layer (make_lgeo, make_g64), a page of host code no query exports; restating it here would be a third
    formula to keep in step.  Their marks sit at need - 256 from 4097 rows on (profiles/r26_bounds_high_water.txt).
Left out: TRAIN_FORMS["lmm16_chunks"] (128 layers): its workspace is 1 GiB, and filling, running and scanning it three times takes
far more than a few seconds; its row-chunk addressing is the lmm16 form's.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bounds  # noqa: E402
from bounds import Out, align256  # noqa: E402
from test_workspace_hygiene_gpu import FIT_CASES, FLOW_FORMS, TRAIN_FORMS, _Flow, _dev, _twister  # noqa: E402

pytestmark = pytest.mark.gpu

F32, I64 = torch.float32, torch.int64
API_TAIL = 256                         # rnvp_workspace_bytes: the family's bytes + 256


def _const(f, **more):
    """the const inputs of a call that updates the parameters in place"""
    d = dict(masks=f.masks)
    d.update({k: v for k, v in more.items() if v is not None})
    return d


def _inputs(f, **more):
    return _const(f, params=f.params, **more)


# ---- rnvp_forward_logprob, rnvp_inverse, rnvp_sample ----------------------------------------------------------------------------------
LOGP_PARTIALS = {"lmm16": 4096 * 4, "valu": 512 * 4}          # else chained: kMaxGrid x kWaves floats


FLOW_ROWS = {form: (1, 17, 257, 4097, 70001) for form in FLOW_FORMS}
FLOW_ROWS["tile_split"] = (1, 17, 257, 4095, 4096)            # the latency kernels serve at most 4096 rows
FLOW_CASES = [(form, n) for form in FLOW_FORMS for n in FLOW_ROWS[form]]
# the smallest row count at which every register-chained forward launch is cut off at its grid bound: k_mfma_flow runs 4 waves x 4
# row tiles x 16 = 256 rows per workgroup from 32769 rows on, at most kMaxGrid = 2048 workgroups (rnvp_mfma.hip launch_flow);
# k_flow_bx3 runs 4 waves x 3 tiles = 192 rows and at most 2048 workgroups in its direct form, 8 waves x at most 4 tiles and at most
# kMaxGridBx3 = 1024 in its staged form (rnvp_bx3.hip launch): 2048 x 256 rows fill the first, one row more exceeds all three
FLOW_BOUND_ROWS = 2048 * 256 + 1
FLOW_BOUND_GRID = {"chained_f32": 2048, "bx3_direct": 2048, "bx3_staged": 1024}
FLOW_CASES += [(form, FLOW_BOUND_ROWS) for form in FLOW_BOUND_GRID]


@pytest.mark.parametrize("form,n", FLOW_CASES)
def test_flow_calls(form, n):
    f = _Flow(*FLOW_FORMS[form])
    _hip, d = f.hip, f.d
    X, C = f.data(n + 5)
    xd, cd = _dev(X), _dev(C)
    tag = "[%s, %d rows]" % (form, n)
    need = f.ws_bytes(_hip.OP_FORWARD, n)
    partials = LOGP_PARTIALS.get(form, 2048 * 4 * 4)
    hw, _ = bounds.run("rnvp_forward_logprob" + tag, need,
               lambda ws, o: _hip.forward_logprob(f.shape, f.params, f.masks, xd, cd, None, n, o["z"], o["logdet"], o["logp"], o["logp_sum"], ws),
               dict(z=Out(F32, (n, d)), logdet=Out(F32, (n,)), logp=Out(F32, (n,)), logp_sum=Out(F32, (1,))), _inputs(f, x=xd, c=cd),
               last=partials, tail=API_TAIL)
    if n == FLOW_BOUND_ROWS:                                   # grid x waves partials: the whole buffer, whichever family runs
        disp = _hip.last_dispatch(_hip.PROFILE_FORWARD)
        print("bounds   dispatch %s" % (disp,))
        assert disp["grid"] == FLOW_BOUND_GRID[form] < -(-n // (disp["waves"] * disp["row_tiles"] * 16)), disp
        assert disp["grid"] * disp["waves"] * 4 == partials and hw == need - API_TAIL, (disp, hw, need)
    # rnvp_inverse and rnvp_sample share the forward call's size, but form no log-prob: the partials are not handed to their kernels,
    # and what they keep, the packed weights, ends in front of them.  One thread per row packs nothing: its inverse query is 0 bytes
    need = f.ws_bytes(_hip.OP_INVERSE, n)
    valu = form == "valu"
    assert need == (API_TAIL if valu else f.ws_bytes(_hip.OP_FORWARD, n))
    hw_i, _ = bounds.run("rnvp_inverse" + tag, need, lambda ws, o: _hip.inverse(f.shape, f.params, f.masks, xd, cd, n, o["x"], ws),
                         dict(x=Out(F32, (n, d))), _inputs(f, z=xd, c=cd), keeps_nothing=valu)
    hw_s, _ = bounds.run("rnvp_sample" + tag, need, lambda ws, o: _hip.sample(f.shape, f.params, f.masks, cd, n, 99, 5, o["x"], ws),
                         dict(x=Out(F32, (n, d))), _inputs(f, c=cd), keeps_nothing=valu)
    if not valu:
        assert 0 < hw_i <= need - API_TAIL - partials and 0 < hw_s <= need - API_TAIL - partials, (hw_i, hw_s, need)


# ---- rnvp_loss_grad, rnvp_loss_grad_zseed, rnvp_backward, rnvp_train_step ------------------------------------------------------------
def _training_end(f, form, need, P):
    """last= / tail= of bounds.run for a training workspace of `need` bytes, where the layout's end can be restated"""
    L, d = f.L, f.d
    if form == "valu":                   # rnvp_generic.hip: gpart [256][P], losspart [256], saved layer inputs [256][L][d][256]
        saved = 256 * L * d * 256 * 4
        assert need == align256(256 * P * 4) + align256(256 * 4) + align256(saved) + API_TAIL
        return dict(last=saved, tail=API_TAIL)
    if form.startswith("chained"):
        # train_workspace_bytes (rnvp_mfma_train.hip) does not depend on the rows and ends with the waves' saved activations:
        # kMaxGridTrain = 512 workgroups x kWaves = 4 x scratch_per_wave = L x RMAX x 2 x NF x 64 floats, RMAX x NF = 8 for every
        # NF (TrainRows: 4, 2, 1 row tiles for NF 2, 4, 8).  Where rnvp_workspace_bytes returns more, it is the any-shape kernels'
        # figure (rnvp_backward of more rows than the tile-split kernel takes): the chained call then ends short of it by the difference
        own = f.ws_bytes(f.hip.OP_TRAIN, 1)
        assert own == f.ws_bytes(f.hip.OP_TRAIN, 33) <= need
        return dict(last=512 * 4 * L * 1024 * 4, tail=need - own + API_TAIL)
    return {}


TRAIN_CASES = ([(form, n) for form in ("chained_c2", "chained_c3", "chained_c4", "chained_c0", "lmm16", "valu") for n in (1, 17, 33, 8191, 8193, 70001)] +
               [("lmm64", n) for n in (8192, 8193, 70001)])


@pytest.mark.parametrize("form,n", TRAIN_CASES)
def test_training_calls(form, n):
    L, d, c, hidden, alt, family = TRAIN_FORMS[form]
    f = _Flow(L, d, c, hidden, alt=alt, family=family)
    _hip, P = f.hip, f.P
    N = n + 7
    X, C = f.data(N)
    xd, cd = _dev(X), _dev(C)
    idx = _dev(f.rng.permutation(N)[:n].astype(np.int64), I64)
    g = torch.Generator(device="cuda").manual_seed(n)
    gz = torch.randn(n, d, device="cuda", generator=g) / n
    gld = torch.randn(n, device="cuda", generator=g) / n
    need = f.ws_bytes(_hip.OP_TRAIN, n)
    tag = "[%s, %d rows]" % (form, n)
    inputs = _inputs(f, x=xd, c=cd, row_index=idx)
    kw = _training_end(f, form, need, P)
    bounds.run("rnvp_loss_grad" + tag, need,
               lambda ws, o: _hip.loss_grad(f.shape, f.params, f.masks, xd, cd, idx, n, 1.0 / n, o["grad"], o["loss"], ws),
               dict(grad=Out(F32, (P,)), loss=Out(F32, (1,))), inputs, **kw)
    disp = _hip.last_dispatch()
    print("bounds   dispatch %s" % (disp,))
    if form.startswith("chained") and n == 70001:             # the grid bound of the register-chained training kernels
        per_wg = disp["waves"] * disp["row_tiles"] * 16
        wide = 16 < d <= 32                                   # NF == 4 past 256 workgroups: 8-wave workgroups, at most kMaxGridTrain / 2 (launch_train_r)
        assert disp["variant"] == ("wide" if wide else "rowpar") and disp["grid"] == (256 if wide else 512) < -(-n // per_wg), disp
    if form == "valu" and n == 70001:
        assert disp["grid"] == 256, disp
    bounds.run("rnvp_loss_grad_zseed" + tag, need,
               lambda ws, o: _hip.loss_grad_zseed(f.shape, f.params, f.masks, xd, cd, idx, n, 1.0 / n, gz, o["grad"], o["loss"], ws),
               dict(grad=Out(F32, (P,)), loss=Out(F32, (1,))), dict(inputs, gz=gz), **kw)
    if n <= 8192 or family != "auto":
        bounds.run("rnvp_backward" + tag, need,
                   lambda ws, o: _hip.backward(f.shape, f.params, f.masks, xd, cd, idx, n, gz, gld, o["grad"], o["gx"], ws),
                   dict(grad=Out(F32, (P,)), gx=Out(F32, (n, d))), dict(inputs, gz=gz, gld=gld), **(kw if form == "valu" else {}))
        # (the chained forms here have one 16-unit hidden tile and the tile-split kernel, the only chained one that carries per-row
        # seeds, wants three: ts_max_rows is 0 and their rnvp_backward runs on the any-shape kernels at any row count)
    zeros = torch.zeros(P, device="cuda")
    bounds.run("rnvp_train_step" + tag, need,
               lambda ws, o: _hip.train_step(f.shape, o["params"], f.masks, xd, cd, idx, n, 1.0 / n, o["grad"], o["loss"], o["exp_avg"],
                                             o["exp_avg_sq"], 0.01, 0.9, 0.999, 1e-8, 0.2, 3, ws),
               dict(params=Out(F32, (P,), f.params), exp_avg=Out(F32, (P,), zeros), exp_avg_sq=Out(F32, (P,), zeros), grad=Out(F32, (P,)),
                    loss=Out(F32, (1,))), _const(f, x=xd, c=cd, row_index=idx), **kw)


# ---- rnvp_backward_cond, rnvp_inverse_backward ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 65, 4097])
@pytest.mark.parametrize("form,hidden", [("lmm16", (12, 20)), ("valu", (512,))])
def test_condition_and_inverse_backward(form, hidden, n):
    L, d, c = 2, 6, 2
    f = _Flow(L, d, c, hidden, alt=1)
    _hip, P = f.hip, f.P
    X, C = f.data(n)
    xd, cd = _dev(X), _dev(C)
    g = torch.Generator(device="cuda").manual_seed(n)
    gz, gld = torch.randn(n, d, device="cuda", generator=g) / n, torch.randn(n, device="cuda", generator=g) / n
    need = _hip.backward_cond_workspace_bytes(f.shape, n)
    tag = "[%s, %d rows]" % (form, n)
    kw = _training_end(f, form, need, P)                      # valu: the one-thread-per-row training layout; lmm16: see the docstring
    bounds.run("rnvp_backward_cond" + tag, need,
               lambda ws, o: _hip.backward_cond(f.shape, f.params, f.masks, xd, cd, None, n, gz, gld, o["grad"], o["gx"], o["gc"], ws),
               dict(grad=Out(F32, (P,)), gx=Out(F32, (n, d)), gc=Out(F32, (n, c))), _inputs(f, x=xd, c=cd, gz=gz, gld=gld), **kw)
    bounds.run("rnvp_inverse_backward" + tag, need,
               lambda ws, o: _hip.inverse_backward(f.shape, f.params, f.masks, xd, cd, n, gz, o["grad"], o["gz"], o["gc"], ws),
               dict(grad=Out(F32, (P,)), gz=Out(F32, (n, d)), gc=Out(F32, (n, c))), _inputs(f, z=xd, c=cd, gx=gz), **kw)


# ---- rnvp_fit_epoch, rnvp_fit_epochs, rnvp_fit_epoch_dp ----------------------------------------------------------------------------------
FIT = dict(FIT_CASES, resident_deep=(8, 2, 1, (10, 10), 1, "auto", 161, 32))          # two hidden layers: k_fit_resident_deep


@pytest.mark.parametrize("entry", ["fit_epoch", "fit_epochs", "fit_epoch_dp", "fit_epoch_dp_cb", "fit_epoch_dp_cb_chunked"])
@pytest.mark.parametrize("case", list(FIT))
def test_fit_epoch_calls(case, entry):
    L, d, c, hidden, alt, family, n, bs = FIT[case]
    f = _Flow(L, d, c, hidden, alt=alt, family=family)
    _hip, P = f.hip, f.P
    assert _hip.fit_epoch_resident(f.shape, bs) == case.startswith("resident")
    n_epochs = 2 if entry == "fit_epochs" else 1
    X, C = f.data(n)
    xd, cd = _dev(X), _dev(C)
    gen = torch.Generator().manual_seed(11)
    perms = torch.stack([torch.randperm(n, generator=gen) for _ in range(n_epochs)]).cuda()
    nb = -(-n // bs)
    zeros = torch.zeros(P, device="cuda")
    dp = entry.startswith("fit_epoch_dp")                        # one rank: no communicator, or a caller's exchange that has nothing to add
    resident = case.startswith("resident") and not dp
    G = P + 1 if dp else P                                       # grad_loss [P + 1]: the gradient and the batch loss share

    def call(ws, o):
        a = (o["params"], f.masks, xd, cd)
        b = (o["grad"], o["loss_hist"], o["exp_avg"], o["exp_avg_sq"], 0.01, 0.9, 0.999, 1e-8, 0.05, 1, ws)
        if entry == "fit_epochs":
            return _hip.fit_epochs(f.shape, *a, perms, n, bs, n_epochs, *b)
        if entry == "fit_epoch_dp":
            return _hip.fit_epoch_dp(None, f.shape, *a, perms[0], n, bs, *b)
        if dp:
            return _hip.fit_epoch_dp_cb(lambda buf, count: None, 0, 1, f.shape, *a, perms[0], n, bs, *b,
                                        chunks=2 if entry.endswith("chunked") else 1)
        return _hip.fit_epoch(f.shape, *a, perms[0], n, bs, *b)

    need = f.ws_bytes(_hip.OP_TRAIN, bs)
    chained = _hip.kernel_path(f.shape, f.masks_np, _hip.OP_TRAIN) == _hip.PATH_MFMA          # (resident-deep: two hidden layers, any-shape)
    form = "valu" if family == "valu" else "chained" if chained else "lmm"
    kw = {} if resident else _training_end(f, form, need, P)    # (a resident shape's data-parallel epoch runs the step kernels of its family)
    hw, _ = bounds.run("rnvp_%s[%s]" % (entry, case), need, call,
                       dict(params=Out(F32, (P,), f.params), exp_avg=Out(F32, (P,), zeros), exp_avg_sq=Out(F32, (P,), zeros), grad=Out(F32, (G,)),
                            loss_hist=Out(F32, (n_epochs, nb))), _const(f, x=xd, c=cd, perms=perms),
                       allow=("grad",) if resident else (), keeps_nothing=resident, **kw)
    # (the resident epoch, resident::fit_epoch of rnvp_api.hip, is handed neither grad_buf nor the workspace: all of it lives in LDS)
    assert hw > 0 or resident


# ---- torch's CPU generator streams on the device -------------------------------------------------------------------------------------
MT_STATE_IN = 640 * 4                  # the twister's state as the kernels read it, in front of rnvp_prior_torch_workspace_bytes()


@pytest.mark.parametrize("n", [2, 2049, 1_000_003])
def test_randperm(n):
    from probaforms_amd import _hip
    mt0, _ = _twister(12345)
    need = _hip.randperm_workspace_bytes(n)
    twister = _hip.prior_torch_workspace_bytes()
    # rnvp_randperm.hip: H, two pending lists and the raw words (4 n each), the bids (8 n), 256 bytes of counters, the twister's workspace
    assert need == 4 * align256(4 * n) + align256(8 * n) + 256 + twister and twister % 256 == 0
    bounds.run("rnvp_randperm_torch_cpu[%d]" % n, need, lambda ws, o: _hip.randperm_torch_cpu(o["mt_state"], n, o["perm"], ws),
               dict(mt_state=Out(mt0.dtype, mt0.shape, mt0), perm=Out(I64, (n,))), {},
               last=twister - (MT_STATE_IN if n > 1_000_000 else 0))      # a long draw jumps ahead: the segments' states behind state_in


@pytest.mark.parametrize("n", [17, 2049, 1_000_003])
def test_torch_prior_stream(n):
    from probaforms_amd import _hip
    mt0, _ = _twister(99 + n % 1000, n % 700)
    need = _hip.prior_torch_workspace_bytes()
    # rnvp_prior_torch.hip: state_in [640 words], then the jumped segments' states; a draw of one segment writes state_in alone
    kw = dict(last=need - MT_STATE_IN) if n > 1_000_000 else {}
    bounds.run("rnvp_prior_normal_torch_cpu[%d]" % n, need, lambda ws, o: _hip.prior_normal_torch_cpu(o["mt_state"], n, o["z"], o["tail16"], ws),
               dict(mt_state=Out(mt0.dtype, mt0.shape, mt0), z=Out(F32, (n,)), tail16=Out(F32, (16,))), {},
               allow=("tail16",), **kw)                                  # device scratch (rnvp_hip.h): what it holds afterwards is not specified
