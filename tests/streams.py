"""One driver for the stream tests (tests/test_streams_*_gpu.py): an entry point must enqueue everything on the caller's stream,
return without waiting for it, and be capturable into a graph on that stream.  Every binding takes its stream from torch's current
stream and nearly every other test runs under the default one, stream 0, where a launch, memset or copy that was handed 0 in place of
the caller's stream gives the same bits, and a synchronisation left in a host path costs nothing that a test sees.

run() takes what bounds.run takes and makes three runs of call(ws, o):
  reference   under the default stream: outputs prepared as bounds.Out.prepare does, a zero workspace.
  gated       on a side stream s.  Before anything is enqueued the state is wrong but valid: every floating-point input holds a decoy
              (its values times a factor of its own, rows rolled by one), in-place outputs the decoy of what they start from, the other
              outputs poison, the workspace zeros.  Integer tensors keep their values: no decoy can send a kernel out of range.  On s
              a gate (torch.cuda._sleep, about GATE_MS) is followed by the repair: real inputs copied back, outputs prepared, workspace
              zeroed, an event recorded.  Then call() runs under torch.cuda.stream(s).  When it returns the default stream is
              synchronised, and the event must still be pending: the call waited neither for s nor for the device, and whatever it
              put on stream 0 has run against the wrong state (it read decoys or a zeroed workspace, or the repair wipes what it
              wrote).  If torch's side streams were blocking ones the same assertion fails: no run passes vacuously.  After
              s.synchronize(): status 0, inputs unchanged, every output written, the reference's bits.
  captured    the same call captured into a torch.cuda.CUDAGraph on s alone (no fork inside the capture), outputs and workspace
              prepared again, one replay, the reference's bits.  A call that allocates device memory, synchronises or touches another
              stream fails the capture.  It follows the gated run, which has done the one-time per-kernel setup.
A form whose header says that it takes a host array or may wait is run with waits="<the header's sentence>": it still runs gated and
must give the reference's bits; the pending assertion and the capture are skipped and what was seen is printed.

The gate's length is measured, not assumed: _sleep is timed once per process with two events and the gate sized from that; every case
prints its gate's measured time and the host time of call(), and the pending assertion is the margin's check.
"""
import time

import torch

import hygiene

GATE_MS = 100.0
_PROBE_CYCLES = 4_000_000
_state = {}


def side_stream():
    """the one side stream of the process: with the default stream, two streams are live in a test"""
    if "stream" not in _state:
        _state["stream"] = torch.cuda.Stream()
    return _state["stream"]


def _time_sleep(s, cycles):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(s):
        a.record()
        torch.cuda._sleep(int(cycles))
        b.record()
    s.synchronize()
    return a.elapsed_time(b)


def gate_cycles():
    """the argument of torch.cuda._sleep that holds a stream for GATE_MS, from one timed probe (after a first, untimed launch)"""
    if "cycles" not in _state:
        s = side_stream()
        _time_sleep(s, 1000)
        ms = _time_sleep(s, _PROBE_CYCLES)
        assert ms > 0.05, "torch.cuda._sleep(%d) took %.4f ms: it does not hold a stream, the gate cannot be built from it" % (_PROBE_CYCLES, ms)
        cycles = int(_PROBE_CYCLES * GATE_MS / ms)
        check = _time_sleep(s, cycles)
        for _ in range(2):                                       # (a clock that ramped during the short probe: size it from the gate itself)
            if 0.8 * GATE_MS < check < 1.25 * GATE_MS:
                break
            cycles = int(cycles * GATE_MS / check)
            check = _time_sleep(s, cycles)
        print("streams gate calibration: _sleep(%d) = %.3f ms -> %.0f cycles/ms; gate of %d cycles measured at %.1f ms (target %.0f)"
              % (_PROBE_CYCLES, ms, _PROBE_CYCLES / ms, cycles, check, GATE_MS))
        assert 0.5 * GATE_MS < check < 3.0 * GATE_MS, "the calibrated gate took %.1f ms, not about %.0f" % (check, GATE_MS)
        _state["cycles"] = cycles
    return _state["cycles"]


def _bits(t):
    return t.contiguous().view(-1).view(torch.uint8).clone()


FACTORS = (0.5, 0.75, 0.625, 0.875, 0.5625, 0.6875, 0.8125, 0.9375)


def decoy(t, i):
    """the values of `t` times the i-th factor, rows rolled by one: finite where t is, same signs, same shape"""
    d = t * FACTORS[i % len(FACTORS)]
    return d.roll(1, 0) if d.dim() > 0 and d.shape[0] > 1 else d


def _empty(outs):
    return {k: torch.empty(o.shape, dtype=o.dtype, device="cuda") for k, o in outs.items()}


def _prepare(outs, o):
    for k in outs:
        outs[k].prepare(o[k])


def _differing(what, run, got, ref):
    for k in ref:
        if not hygiene.same_bits(got[k], ref[k]):
            bad = int((got[k].contiguous().view(-1).view(torch.uint8) != ref[k].contiguous().view(-1).view(torch.uint8)).sum())
            raise AssertionError("%s: output %r of the %s run differs from the default-stream run in %d bytes" % (what, k, run, bad))


def run(what, need, call, outs, inputs, allow=(), reference=None, waits=None):
    """call(ws, o), outs {name: bounds.Out} and inputs {name: const device tensor} as for bounds.run; need None: the call takes no
    workspace.  reference: the outputs of a default-stream run on a zero workspace, where the caller has them already (bounds.run
    returns them).  waits: the header's sentence that lets this form wait or read host memory (see the module's docstring).
    -> dict(enqueue_ms, gate_ms, pending, captured)"""
    s = side_stream()
    cycles = gate_cycles()
    need = None if need is None else int(need)
    ws = None if need is None else hygiene.workspace(need, "zeros")
    if reference is None:
        reference = _empty(outs)
        _prepare(outs, reference)
        st = call(ws, reference)
        torch.cuda.synchronize()
        assert st in (None, 0), "%s, default stream: status %r" % (what, st)
    real = {k: v.clone() for k, v in inputs.items() if v.is_floating_point()}
    wrong = {k: decoy(v, i) for i, (k, v) in enumerate(real.items())}
    before = {k: _bits(v) for k, v in inputs.items()}
    o = _empty(outs)

    # ---- gated ----
    for k, v in wrong.items():
        inputs[k].copy_(v)
    for i, (k, out) in enumerate(outs.items()):
        if out.init is None:
            hygiene.poison_outputs(o[k])
        else:
            start = out.init.view(out.shape)
            o[k].copy_(decoy(start, i + 3) if start.is_floating_point() else start)
    if ws is not None:
        ws.zero_()
    torch.cuda.synchronize()
    t0, t1, ev = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True), torch.cuda.Event()
    try:
        with torch.cuda.stream(s):
            t0.record()
            torch.cuda._sleep(cycles)
            t1.record()
            for k, v in real.items():
                inputs[k].copy_(v)
            _prepare(outs, o)
            if ws is not None:
                ws.zero_()
            ev.record()
            h0 = time.perf_counter()
            st = call(ws, o)
            enqueue_ms = (time.perf_counter() - h0) * 1e3
        torch.cuda.default_stream().synchronize()
        pending = not ev.query()
    finally:
        s.synchronize()
        for k, v in real.items():                                # (an exception out of call() leaves no decoy behind)
            inputs[k].copy_(v)
        torch.cuda.synchronize()
    gate_ms = t0.elapsed_time(t1)
    print("streams %-84s enqueue %8.3f ms  gate %6.1f ms  %s" % (what, enqueue_ms, gate_ms,
                                                                   "gate pending" if pending else "GATE PASSED BEFORE THE CALL RETURNED"))
    assert st in (None, 0), "%s, gated: status %r" % (what, st)
    if waits is None:
        assert pending, ("%s: the gate in front of the call (%.1f ms) was no longer pending when the call had returned after %.3f ms "
                         "on the host: the call waited for its stream or for the device" % (what, gate_ms, enqueue_ms))
    for k, v in inputs.items():
        assert torch.equal(_bits(v), before[k]), "%s, gated: const input %r was changed" % (what, k)
    hygiene.assert_all_written(o, what + ", gated on a side stream", allow=allow)
    _differing(what, "gated side-stream", o, reference)
    result = dict(enqueue_ms=enqueue_ms, gate_ms=gate_ms, pending=pending, captured=False)
    if waits is not None:
        print("streams   excepted by its header (%s): %s; not captured" % (waits, "did not wait here" if pending else "waited"))
        return result

    # ---- captured ----
    _prepare(outs, o)
    if ws is not None:
        ws.zero_()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    failure = None
    with torch.cuda.stream(s):
        g.capture_begin()
        try:
            st = call(ws, o)
        except Exception as e:                                   # a binding that raises on a bad status: the capture is ended first
            failure = e
        try:
            g.capture_end()
        except Exception as e:
            failure = failure or e
    assert failure is None, "%s: the call cannot be captured on its stream: %r" % (what, failure)
    assert st in (None, 0), "%s, captured: status %r" % (what, st)
    _prepare(outs, o)
    if ws is not None:
        ws.zero_()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        g.replay()
    s.synchronize()
    for k, v in inputs.items():
        assert torch.equal(_bits(v), before[k]), "%s, captured: const input %r was changed" % (what, k)
    hygiene.assert_all_written(o, what + ", replayed from a graph", allow=allow)
    _differing(what, "captured and replayed", o, reference)
    del g
    result["captured"] = True
    return result


def entry_point(what):
    """the entry point's name in a case's `what`: 'pfm_mmd[65+64 rows, ...]' -> 'pfm_mmd'"""
    return what.split("[")[0].strip()


def through_bounds(bounds, test, kwargs, waits=lambda what: None):
    """run the bounds module's test function `test(**kwargs)` with bounds.run replaced by a wrapper that runs the original driver, then
    the stream checks on the same case (the original's plain run is the reference), and returns the original's result: the test's own
    assertions on the high-water mark keep working.  bounds.run_outputs goes through bounds.run.  -> the `what` of every case reached"""
    original, reached = bounds.run, []

    def both(what, need, call, outs, inputs, **kw):
        res = original(what, need, call, outs, inputs, **kw)
        run(what, need, call, outs, inputs, allow=kw.get("allow", ()), reference=res[1], waits=waits(what))
        reached.append(what)
        return res

    bounds.run = both
    try:
        test(**kwargs)
    finally:
        bounds.run = original
    return reached


def check_catalogue(bounds, module, case, waits=lambda what: None):
    """one line of a stream module's catalogue, (test function's name, its arguments, the entry points it must reach)"""
    name, kwargs, expect = case
    reached = through_bounds(bounds, getattr(module, name), kwargs, waits)
    got = {entry_point(w) for w in reached}
    assert got == set(expect), "%s(%r) reached %s, the catalogue says %s" % (name, kwargs, sorted(got), sorted(expect))
    return reached
