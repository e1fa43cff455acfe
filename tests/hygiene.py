"""Workspace hygiene: what a kernel call may NOT depend on.

Every entry point of the HIP libraries takes a caller-owned workspace and keeps state in it between the launches of one call
(packed weights, per-workgroup partials, counters, an error word).  The contract is that a call writes what it later reads.  The
helpers here hand a call a workspace in a hostile state and poison its outputs, so that a test can require the same bits out
whatever the workspace held before (tests/test_workspace_hygiene_gpu.py, tests/test_dp_empty_share_gpu.py).
"""
import torch

# zeros:  what a fresh allocation usually holds (the state every other GPU test runs in)
# replay: the workspace as a previous, different call of the same entry point left it (the caller runs that priming call on the
#         zero-filled buffer): what FlowEngine's one-workspace-per-operation really produces
# ones:   0xFF bytes -- NaN as float32 / float64, -1 as any integer
# huge:   0x7F bytes -- 3.39e38 as float32: finite, so a stray add overflows instead of vanishing; a large positive count as an integer
PATTERNS = ("zeros", "replay", "ones", "huge")
_FILL = {"zeros": 0x00, "replay": 0x00, "ones": 0xFF, "huge": 0x7F}

INT_SENTINEL = -0x5A5A5A5B


def workspace(nbytes, pattern, device="cuda"):
    """uint8 tensor of exactly `nbytes` bytes (at least 16: the bindings want a non-empty buffer) filled with `pattern`"""
    if pattern not in _FILL:
        raise ValueError("unknown workspace pattern %r" % (pattern,))
    return torch.full((max(int(nbytes), 16),), _FILL[pattern], dtype=torch.uint8, device=device)


def fill(buf, pattern):
    """fill an existing uint8 workspace (an engine's own) with `pattern`"""
    buf.fill_(_FILL[pattern])
    return buf


def poison_outputs(*tensors):
    """float outputs to NaN, integer outputs to a sentinel: an element the call forgets to write is seen"""
    for t in tensors:
        if t is None:
            continue
        if t.is_floating_point():
            t.fill_(float("nan"))
        else:
            t.fill_(INT_SENTINEL if t.dtype in (torch.int32, torch.int64) else 0x5A)
    return tensors


def poisoned(t):
    """number of elements of `t` that still hold the output poison"""
    if t.is_floating_point():
        return int(torch.isnan(t).sum())
    return int((t == (INT_SENTINEL if t.dtype in (torch.int32, torch.int64) else 0x5A)).sum())


def same_bits(a, b):
    """bitwise equality (NaN payloads included)"""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return bool(torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)))


def assert_pattern_independent(outs, what):
    """outs: {pattern: {name: tensor}}; every output of every pattern carries the bits of the `zeros` run"""
    base = outs["zeros"]
    for pat, got in outs.items():
        for name, t in got.items():
            if not same_bits(t, base[name]):
                diff = t.double() - base[name].double()
                bad = int((t.contiguous().view(torch.uint8) != base[name].contiguous().view(torch.uint8)).sum())
                raise AssertionError("%s: output %r depends on the workspace: pattern %r differs from 'zeros' in %d bytes "
                                     "(max |diff| %r, NaNs %d)" % (what, name, pat, bad, float(diff.abs().nan_to_num(0.0).max()),
                                                                    int(torch.isnan(t.double()).sum())))


def assert_all_written(outs, what, allow=()):
    for name, t in outs.items():
        if name in allow:
            continue
        n = poisoned(t)
        assert n == 0, "%s: %d elements of output %r still hold the output poison (never written, or NaN)" % (what, n, name)
