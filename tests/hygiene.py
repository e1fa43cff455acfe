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


GUARD_BYTE = 0xC3
GUARD_FRONT = 4096
GUARD_BACK_MAX = 1 << 20
GUARD_ALIGN = 256             # the libraries lay sub-buffers out with align256


class Guarded:
    """`nbytes` interior bytes (at least 16) at a 256-byte-aligned address inside one larger allocation, GUARD_FRONT guard bytes in
    front and max(4096, min(nbytes, 1 MiB)) behind (an extra workgroup's whole record still lands there); guards hold GUARD_BYTE,
    the interior `fill`.  What a call writes outside the interior is seen by assert_guards_intact, what it writes inside by
    written() / high_water()."""

    def __init__(self, nbytes, fill, device="cuda"):
        if fill not in (_FILL["ones"], _FILL["huge"]):
            raise ValueError("guarded(): fill is 0xFF or 0x7F (the `ones` / `huge` bytes of PATTERNS), not %r" % (fill,))
        self.fill = int(fill)
        self.nbytes = max(int(nbytes), 16)
        self.back = max(4096, min(int(nbytes), GUARD_BACK_MAX))
        self._raw = torch.full((GUARD_FRONT + GUARD_ALIGN - 1 + self.nbytes + self.back,), GUARD_BYTE, dtype=torch.uint8, device=device)
        self._start = GUARD_FRONT + (-(self._raw.data_ptr() + GUARD_FRONT)) % GUARD_ALIGN
        self.view = self._raw[self._start:self._start + self.nbytes]
        self.view.fill_(self.fill)

    def typed(self, dtype, shape):
        """the interior's bytes as an output tensor of `dtype` and `shape`, which must take exactly the bytes asked for; an output of
        fewer than the 16 bytes `view` has at least gives the rest of them to the back guard, so the guard starts where the output ends"""
        want = torch.empty((), dtype=dtype).element_size()
        for s in shape:
            want *= int(s)
        assert want == self.nbytes or 0 < want < self.nbytes == 16, "typed(): %r of %s is not the %d guarded bytes" % (tuple(shape), dtype, self.nbytes)
        if want < self.nbytes:
            self.retract(self.nbytes - want)
        return self.view.view(dtype).view(*shape)

    def retract(self, nbytes):
        """tell the handle that the interior ends `nbytes` earlier than it does: those bytes become guard (the detector's self-test;
        a `view` taken before still spans them)"""
        assert 0 < nbytes < self.nbytes
        self.nbytes -= int(nbytes)
        self.back += int(nbytes)
        self._raw[self._start + self.nbytes:self._start + self.nbytes + int(nbytes)] = GUARD_BYTE
        self.view = self._raw[self._start:self._start + self.nbytes]

    def assert_guards_intact(self, what):
        end = self._start + self.nbytes
        for name, region, origin in (("behind", self._raw[end:], 0), ("in front of", self._raw[:self._start], -self._start)):
            bad = region != GUARD_BYTE
            if bool(bad.any()):
                at = bad.nonzero().flatten()
                raise AssertionError("%s: wrote %s its %d bytes: %d guard bytes changed, the first at %s%+d, the last at %s%+d"
                                     % (what, name, self.nbytes, at.numel(), "end" if origin == 0 else "start", int(at[0]) + origin,
                                        "end" if origin == 0 else "start", int(at[-1]) + origin))

    def written(self):
        """bool mask over the interior: the bytes that differ from `fill`"""
        return self.view != self.fill


def guarded(nbytes, fill, device="cuda"):
    return Guarded(nbytes, fill, device)


def high_water(h1, h2):
    """the offset after the last interior byte written in either of two runs of the same call on the two fills (a byte that one run
    happens to set to its own fill value is seen in the other); 0: nothing written"""
    assert h1.nbytes == h2.nbytes and h1.fill != h2.fill
    step = 1 << 24                                    # from the end, a piece at a time: a workspace can be a gigabyte
    for hi in range(h1.nbytes, 0, -step):
        lo = max(0, hi - step)
        at = ((h1.view[lo:hi] != h1.fill) | (h2.view[lo:hi] != h2.fill)).nonzero().flatten()
        if at.numel():
            return lo + int(at[-1]) + 1
    return 0


def assert_all_written(outs, what, allow=()):
    for name, t in outs.items():
        if name in allow:
            continue
        n = poisoned(t)
        assert n == 0, "%s: %d elements of output %r still hold the output poison (never written, or NaN)" % (what, n, name)
