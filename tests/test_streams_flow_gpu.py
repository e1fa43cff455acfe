"""Every rnvp_* entry point of librnvp_hip.so enqueues on the caller's stream alone, returns without waiting, and can be captured
(tests/streams.py has the driver and says what a wrong stream does to its gated run).  The cases are those of
tests/test_bounds_flow_gpu.py, reached through its own test functions with bounds.run wrapped (streams.through_bounds): the write-bounds
checks run first, unchanged, then the stream checks on the same call.  Per entry point one case of every launch path that enqueues
another kernel sequence; the grid-bound row counts (524 289, 70 001, 1 000 003) and lmm16_chunks are left out: which stream a launch
is handed does not depend on the rows once the path is fixed.  rnvp_adam_step, rnvp_dp_finish_step and rnvp_prior_normal take a stream
and are not in the bounds catalogue (no workspace): they have cases of their own below.  tests/test_streams_host.py holds CATALOGUE
against the bounds module.  No form of this library is excepted: include/rnvp_hip.h lets none of these calls wait or read host
memory (the caller's exchange of the *_dp_cb epochs is the caller's; the one here adds nothing and does not wait).
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bounds  # noqa: E402
import streams  # noqa: E402
import test_bounds_flow_gpu as tb  # noqa: E402
from bounds import Out  # noqa: E402

pytestmark = pytest.mark.gpu

F32 = torch.float32
FLOW = ("rnvp_forward_logprob", "rnvp_inverse", "rnvp_sample")
TRAIN = ("rnvp_loss_grad", "rnvp_loss_grad_zseed", "rnvp_backward", "rnvp_train_step")
EPOCHS = ("fit_epoch", "fit_epochs", "fit_epoch_dp", "fit_epoch_dp_cb", "fit_epoch_dp_cb_chunked")

CATALOGUE = (
    # chained f32, bx3 direct / staged, tile-split, lmm16, valu: more than one workgroup's rows, a ragged last tile
    [("test_flow_calls", dict(form=form, n=257), FLOW) for form in tb.FLOW_FORMS] +
    # the register-chained training kernels at every NF, tile-split (33 rows) and row-parallel (8193); lmm16, lmm64, valu;
    # rnvp_backward of 8193 rows is served for a pinned family only
    [("test_training_calls", dict(form=form, n=33), TRAIN) for form in ("chained_c2", "chained_c3", "chained_c4", "chained_c0", "lmm16", "valu")] +
    [("test_training_calls", dict(form="chained_c2", n=8193), TRAIN[:2] + TRAIN[3:]), ("test_training_calls", dict(form="lmm64", n=8193), TRAIN)] +
    [("test_condition_and_inverse_backward", dict(form=form, hidden=hidden, n=65), ("rnvp_backward_cond", "rnvp_inverse_backward"))
     for form, hidden in (("lmm16", (12, 20)), ("valu", (512,)))] +
    # every epoch call, the data-parallel ones as one rank, on every family; each case ends in a ragged batch
    [("test_fit_epoch_calls", dict(case=case, entry=entry), ("rnvp_" + entry,))
     for case in ("resident", "chained", "lmm", "valu", "resident_deep") for entry in EPOCHS] +
    # a one-row last batch (resident), row-parallel batches then one row on the tile-split kernel, 64-row blocks then one row
    [("test_fit_epoch_calls", dict(case=case, entry="fit_epoch"), ("rnvp_fit_epoch",)) for case in ("resident_1row", "chained_1row", "lmm_1row")] +
    [("test_randperm", dict(n=n), ("rnvp_randperm_torch_cpu",)) for n in (2, 2049)] +
    [("test_torch_prior_stream", dict(n=n), ("rnvp_prior_normal_torch_cpu",)) for n in (17, 2049)]
)


def _id(case):
    return "%s-%s" % (case[0][5:], "-".join(str(v) for v in case[1].values()))


@pytest.mark.parametrize("case", CATALOGUE, ids=_id)
def test_bounds_catalogue(case):
    streams.check_catalogue(bounds, tb, case)


# ---- the entry points that take a stream and no workspace ------------------------------------------------------------------------------
ADDED = ("rnvp_adam_step", "rnvp_dp_finish_step", "rnvp_prior_normal")


def _moments(P, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    p = torch.randn(P, device="cuda", generator=g)
    grad = torch.randn(P, device="cuda", generator=g) * 0.1
    m = torch.randn(P, device="cuda", generator=g) * 0.01
    v = torch.rand(P, device="cuda", generator=g) * 1e-4
    return p, grad, m, v


@pytest.mark.parametrize("P", [1, 257, 70001])                  # one thread, a ragged second block, many blocks
def test_adam_step(P):
    from probaforms_amd import _hip
    p, grad, m, v = _moments(P, P)
    streams.run("rnvp_adam_step[%d parameters]" % P, None,
                lambda ws, o: _hip.adam_step(o["params"], grad, o["exp_avg"], o["exp_avg_sq"], P, 0.01, 0.9, 0.999, 1e-8, 0.05, 3),
                dict(params=Out(F32, (P,), p), exp_avg=Out(F32, (P,), m), exp_avg_sq=Out(F32, (P,), v)), dict(grad=grad))


@pytest.mark.parametrize("P", [0, 1, 257, 70001])               # no parameters: the loss alone, a copy on the stream (rnvp_adam.hip)
def test_dp_finish_step(P):
    from probaforms_amd import _hip
    p, grad, m, v = _moments(max(P, 1), P + 7)
    grad_loss = torch.cat([grad[:P], torch.full((1,), 1.25, device="cuda")]).contiguous()
    outs = dict(loss=Out(F32, (1,)))
    if P:
        outs.update(params=Out(F32, (P,), p), exp_avg=Out(F32, (P,), m), exp_avg_sq=Out(F32, (P,), v))
    one = torch.zeros(1, device="cuda")
    streams.run("rnvp_dp_finish_step[%d parameters]" % P, None,
                lambda ws, o: _hip.dp_finish_step(o.get("params", one), grad_loss, o.get("exp_avg", one), o.get("exp_avg_sq", one), P,
                                                  0.01, 0.9, 0.999, 1e-8, 0.05, 3, o["loss"]),
                outs, dict(grad_loss=grad_loss))


@pytest.mark.parametrize("n,d", [(1, 1), (257, 5), (4097, 16)])
def test_prior_normal(n, d):
    from probaforms_amd import _hip
    streams.run("rnvp_prior_normal[%d rows, d %d]" % (n, d), None, lambda ws, o: _hip.prior_normal(99, 5, n, d, o["z"]),
                dict(z=Out(F32, (n, d))), {})
