"""One driver for the write-bounds tests (tests/test_bounds_*_gpu.py): an entry point runs on a guarded workspace of exactly the
size its own *_workspace_bytes() gives and on guarded outputs (hygiene.guarded), once per fill, then once on a plain zero
workspace.  Checked: every guard byte intact, every const input unchanged, every output written, the three runs' outputs the same
bits; returned: the workspace's high-water mark.  Correctness against the references stays in the entry points' own tests.
"""
import torch

import hygiene

FILLS = (0xFF, 0x7F)          # the `ones` and `huge` bytes of hygiene.PATTERNS


def align256(b):
    return (int(b) + 255) & ~255


class Out:
    """an output: dtype, shape and, for one the call updates in place (params, moments), the tensor it starts from"""

    def __init__(self, dtype, shape, init=None):
        self.dtype, self.shape, self.init = dtype, tuple(int(s) for s in shape), init

    def nbytes(self):
        n = torch.empty((), dtype=self.dtype).element_size()
        for s in self.shape:
            n *= s
        return n

    def prepare(self, t):
        if self.init is None:
            hygiene.poison_outputs(t)
        else:
            t.copy_(self.init.view(self.shape))
        return t


def _bits(t):
    return t.contiguous().view(-1).view(torch.uint8).clone()


def run(what, need, call, outs, inputs, last=None, tail=0, keeps_nothing=False, allow=(), reach=()):
    """call(ws, o) runs the entry point on the uint8 workspace `ws` and the output tensors o[name] and returns its status (or None
    where the binding raises on a bad status).  outs {name: Out}, inputs {name: const device tensor}.  `last`: the bytes of the last
    sub-buffer of the workspace's layout (before alignment), `tail` what the size function adds behind it (an unused block); the
    high-water mark must lie inside the sub-buffer.  keeps_nothing: the size function says the call keeps nothing in the workspace, so no interior byte may change.  reach: (lo, hi, name) byte ranges of the
    workspace in which the call must have written something (the last slab of a buffer sized by a bound on the grid).
    -> (high water, the plain run's outputs)
    """
    assert need is None or need > 0, "%s: the workspace query refuses the sizes" % what
    need = None if need is None else int(need)
    before = {k: _bits(v) for k, v in inputs.items()}
    handles, got = [], []
    for fill in FILLS:
        ws = None if need is None else hygiene.guarded(need, fill)
        oh = {k: hygiene.guarded(o.nbytes(), fill) for k, o in outs.items()}
        # typed() is called once per handle: for an output of fewer than 16 bytes (a loss, a status word) it also moves the handle's
        # end up to the output's, so that the back guard starts right behind it (Guarded.typed, Guarded.retract)
        o = {k: outs[k].prepare(oh[k].typed(outs[k].dtype, outs[k].shape)) for k in outs}
        st = call(None if ws is None else ws.view, o)
        torch.cuda.synchronize()
        tag = "%s, fill 0x%02X" % (what, fill)
        assert st in (None, 0), "%s: status %r" % (tag, st)
        if ws is not None:
            ws.assert_guards_intact(tag + ": workspace")
        for k, h in oh.items():
            h.assert_guards_intact("%s: output %r" % (tag, k))
        for k, v in inputs.items():
            assert torch.equal(_bits(v), before[k]), "%s: const input %r was changed" % (tag, k)
        hygiene.assert_all_written(o, tag, allow=allow)
        handles.append(ws)
        got.append(o)
    plain = {k: outs[k].prepare(torch.empty(outs[k].shape, dtype=outs[k].dtype, device="cuda")) for k in outs}
    st = call(None if need is None else hygiene.workspace(need, "zeros"), plain)
    torch.cuda.synchronize()
    assert st in (None, 0), "%s, plain workspace: status %r" % (what, st)
    for k in outs:
        for fill, o in zip(FILLS, got):
            assert hygiene.same_bits(o[k], plain[k]), "%s: output %r on the guarded 0x%02X run differs from the plain run" % (what, k, fill)
    if need is None:
        return 0, plain
    hw = hygiene.high_water(*handles)
    start = None if last is None else need - tail - align256(last)
    print("bounds %-72s need %10d  high_water %10d  %.4f%s" % (what, need, hw, hw / need, "" if start is None else "  last sub-buffer at %d" % start))
    if keeps_nothing:
        assert hw == 0, "%s: the size function says nothing is kept in the workspace, yet bytes up to %d were written" % (what, hw)
    if last is not None:
        assert start < hw <= start + last, ("%s: high-water mark %d is not inside the last sub-buffer [%d, %d) of the %d bytes"
                                            % (what, hw, start, start + last, need))
    if reach:
        a, b = handles
        for lo, hi, name in reach:
            assert 0 <= lo < hi <= need, (what, name, lo, hi, need)
            seen = (a.view[lo:hi] != a.fill) | (b.view[lo:hi] != b.fill)
            assert bool(seen.any()), "%s: no byte of %s, [%d, %d), was written" % (what, name, lo, hi)
    return hw, plain


def run_outputs(what, call, outs, inputs, allow=()):
    """an entry point without a workspace: call(o) on guarded outputs once per fill, then on plain ones; the same checks"""
    return run(what, None, lambda ws, o: call(o), outs, inputs, allow=allow)[1]
