"""The stream driver (tests/streams.py) reports what it claims to, shown on a fake three-stage entry point made of torch ops:
stage 1 inputs -> workspace, stage 2 workspace -> workspace, stage 3 workspace -> output.  The clean version passes all three
runs; each stage alone on the default stream, and a version that synchronises its stream, is reported by the gated run.  Every stage
reads and writes inside the tensors it is given, whatever they hold: no version can read out of range."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import streams  # noqa: E402
from bounds import Out  # noqa: E402

pytestmark = pytest.mark.gpu

N = 1000
F32 = torch.float32


def _fake(on_default=0, synchronises=False):
    """call(ws, o) of the fake entry point; stage `on_default` (1..3) is enqueued on stream 0 in place of the caller's stream"""
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.randn(N, device="cuda", generator=g) + 3.0
    y = torch.randn(N, device="cuda", generator=g) + 3.0

    def stage(k, op):
        if k == on_default:
            with torch.cuda.stream(torch.cuda.default_stream()):
                op()
        else:
            op()

    def call(ws, o):
        a, b = ws[:4 * N].view(F32), ws[4 * N:8 * N].view(F32)
        stage(1, lambda: torch.mul(x, 2.0, out=a))
        stage(2, lambda: torch.add(a, 1.0, out=b))
        if synchronises:
            torch.cuda.current_stream().synchronize()
        stage(3, lambda: torch.mul(b, y, out=o["out"]))
        return 0

    return call, dict(out=Out(F32, (N,))), dict(x=x, y=y), (2.0 * x + 1.0) * y


def test_the_clean_entry_point_passes_gated_and_captured():
    call, outs, inputs, want = _fake()
    x0, y0 = inputs["x"].clone(), inputs["y"].clone()
    res = streams.run("fake[clean]", 8 * N, call, outs, inputs)
    assert res["pending"] and res["captured"]
    assert 0.5 * streams.GATE_MS < res["gate_ms"] < 3.0 * streams.GATE_MS and res["enqueue_ms"] < 0.5 * res["gate_ms"], res
    assert torch.equal(inputs["x"], x0) and torch.equal(inputs["y"], y0)
    ref = torch.empty(N, device="cuda")
    call(torch.zeros(8 * N, dtype=torch.uint8, device="cuda"), dict(out=ref))
    assert torch.equal(ref, want)


@pytest.mark.parametrize("stage,message", [(1, "differs from the default-stream run"), (2, "differs from the default-stream run"),
                                           (3, "still hold the output poison")])
def test_a_stage_on_the_default_stream_is_reported(stage, message):
    """stage 1 there packs the decoys, and the repair zeroes what it packed; stage 2 there reads a zero workspace before stage 1
    has run, and the repair zeroes its result; stage 3 there writes the output before the repair poisons it again"""
    call, outs, inputs, _ = _fake(on_default=stage)
    x0 = inputs["x"].clone()
    with pytest.raises(AssertionError, match=message):
        streams.run("fake[stage %d on stream 0]" % stage, 8 * N, call, outs, inputs)
    assert torch.equal(inputs["x"], x0)                          # the driver leaves no decoy behind when it fails


def test_a_call_that_synchronises_its_stream_is_reported_by_the_pending_gate():
    call, outs, inputs, _ = _fake(synchronises=True)
    with pytest.raises(AssertionError, match="was no longer pending when the call had returned"):
        streams.run("fake[synchronises]", 8 * N, call, outs, inputs)


def test_a_form_excepted_by_its_header_still_has_to_give_the_bits():
    call, outs, inputs, _ = _fake(synchronises=True)
    res = streams.run("fake[synchronises, excepted]", 8 * N, call, outs, inputs, waits="the fake header says it may wait")
    assert not res["pending"] and not res["captured"]
    call, outs, inputs, _ = _fake(on_default=2)
    with pytest.raises(AssertionError, match="differs from the default-stream run"):
        streams.run("fake[stage 2 on stream 0, excepted]", 8 * N, call, outs, inputs, waits="the fake header says it may wait")
