"""Every entry point of libpf_wgan.so, libpf_cnormal.so, libpf_gendraw.so and libpf_predict.so and every cvae_* call of
librnvp_hip.so enqueues on the caller's stream alone, returns without waiting, and can be captured (tests/streams.py has the driver).
The cases are those of tests/test_bounds_models_gpu.py, reached through its own test functions with bounds.run wrapped
(streams.through_bounds): the write-bounds checks run first, unchanged, then the stream checks on the same call.  Per entry point one
case of every launch path that enqueues another kernel sequence: the row-tile policies of the step kernels (one row per workgroup,
capped tiles, more than 64 KiB of LDS, a full workgroup), at and below the workgroup bound; the epoch calls with a ragged last batch;
the three CVAE kernel families and the resident epoch; weights in LDS and in the workspace.  The grid-bound row counts (70 001,
131 073) and the shapes whose step is one thread through millions of weights (cnormal cap1 / cap3) are left out: which stream a
launch is handed does not depend on the rows once the path is fixed.  tests/test_streams_host.py holds CATALOGUE against the bounds
module.

EXCEPTIONS is the one table of forms that a header lets wait or read host memory: entry point, the form, the header's sentence, what
is still asserted.  Read from the headers, not granted here: a form that is not listed and waits, or cannot be captured, fails.
"""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bounds  # noqa: E402
import streams  # noqa: E402
import test_bounds_models_gpu as tb  # noqa: E402

pytestmark = pytest.mark.gpu

# (entry point, the text in a case's `what` that marks the form, the header's sentence, what is still asserted)
EXCEPTIONS = [
    ("pfp_draw_accumulate", "seeds",
     "models/predict_csrc/pf_predict.h: With seeds ... the HOST array is copied into the workspace by a stream-ordered host-to-device "
     "copy ... from pageable memory that copy may make the call wait for the work enqueued on `stream` before it, and a capture would "
     "record the host address, not the values",
     "the gated run: status 0, inputs unchanged, outputs written, the default-stream run's bits; its other form (z given) in full"),
]


def waits(what):
    for entry, form, sentence, _ in EXCEPTIONS:
        if streams.entry_point(what) == entry and form in what:
            return sentence
    return None


W_STEP = ("pfw_train_step", "pfw_loss_grad")
N_STEP = ("pfn_train_step", "pfn_loss_grad")
CVAE = ("cvae_encode", "cvae_decode", "cvae_loss_grad", "cvae_train_step")

CATALOGUE = (
    [("test_wgan_steps", dict(name=name, rows=rows, at_bound=at_bound), W_STEP)
     for name, rows, at_bound in (("big_lds", 9, True), ("cap2", 3, True), ("cap1", 3, True), ("full_wg", 50, True), ("odd_cap", 65, True), ("full_wg", 4097, False))] +
    [("test_wgan_epoch_losses_and_fit_epoch", dict(name=name), ("pfw_epoch_losses", "pfw_fit_epoch")) for name in ("full_wg", "big_lds")] +
    [("test_wgan_generate_and_critic", dict(name=name, n=n), ("pfw_generate", "pfw_critic")) for name, n in (("full_wg", 255), ("big_lds", 1), ("gen_only", 257))] +
    [("test_cnormal_steps", dict(name=name, rows=rows, at_bound=at_bound), N_STEP)
     for name, rows, at_bound in (("big_lds", 9, True), ("full_wg", 50, True), ("cap11", 65, True), ("big_lds", 2049, False))] +
    [("test_cnormal_fit_epoch", dict(name=name), ("pfn_fit_epoch",)) for name in ("full_wg", "big_lds")] +
    [("test_cnormal_forward", dict(name=name, n=n), ("pfn_forward",)) for name, n in (("full_wg", 255), ("big_lds", 1), ("wide_fwd", 257))] +
    # every network of the generators' tests (the last keeps its weights in the workspace); one draw window, and more than 64 draws
    [("test_mlp_draw_accumulate", dict(case=case, K=19), ("pfg_mlp_draw_accumulate",)) for case in tb.tg.MLP_CASES] +
    [("test_mlp_draw_accumulate", dict(case=tb.tg.WIDE, K=65), ("pfg_mlp_draw_accumulate",))] +
    [("test_affine_draw_accumulate", dict(d=d, independent=independent), ("pfg_affine_draw_accumulate",)) for d, independent in ((1, False), (17, False), (17, True))] +
    [("test_flow_draw_accumulate", dict(form=form, K=K), ("pfp_draw_accumulate",)) for form, K in (("chained", 19), ("lmm", 19), ("chained", 65))] +
    [("test_cvae_calls", dict(form=form, n=n), CVAE) for form, n in (("mfma", 65), ("lmm", 65), ("generic", 65), ("mfma", 5000))] +
    [("test_cvae_fit_epoch", dict(form=form, n=n, bs=bs), ("cvae_fit_epoch",))
     for form, n, bs in (("mfma", 2 * 9000 + 1, 9000), ("lmm", 2 * 300 + 77, 300), ("generic", 2 * 300 + 1, 300), ("resident", 97, 32), ("resident", 65, 32))]
)


def _id(case):
    return "%s-%s" % (case[0][5:], "-".join(tb.tg._ids(v) if isinstance(v, tuple) else str(v) for v in case[1].values()))


@pytest.mark.parametrize("case", CATALOGUE, ids=_id)
def test_bounds_catalogue(case):
    reached = streams.check_catalogue(bounds, tb, case, waits)
    for entry, form, sentence, still in EXCEPTIONS:             # an excepted entry point's other form has run in full beside it
        if any(streams.entry_point(w) == entry for w in reached):
            assert any(waits(w) is None for w in reached if streams.entry_point(w) == entry), reached


def test_print_the_exception_table():
    for entry, form, sentence, still in EXCEPTIONS:
        print("streams exception: %s [%s]\n    header: %s\n    still asserted: %s" % (entry, form, sentence, still))
    # (tests/test_streams_host.py holds every sentence against its header, word for word)
