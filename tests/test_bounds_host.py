"""The guard-band helpers of tests/hygiene.py (guarded, high_water) detect what they claim, shown on the CPU: the GPU tests
(tests/test_bounds_*_gpu.py) rest on them."""
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import hygiene  # noqa: E402

ONES, HUGE = 0xFF, 0x7F
SIZES = [1, 16, 255, 256, 257, (1 << 20) + 1]


def _raises(h, what="call"):
    with pytest.raises(AssertionError) as e:
        h.assert_guards_intact(what)
    return str(e.value)


@pytest.mark.parametrize("nbytes", SIZES)
def test_layout(nbytes):
    h = hygiene.guarded(nbytes, ONES, device="cpu")
    n = max(nbytes, 16)
    assert h.view.dtype == torch.uint8 and h.view.numel() == n and h.nbytes == n
    assert h.view.data_ptr() % 256 == 0
    raw = h._raw
    start = h.view.data_ptr() - raw.data_ptr()
    assert start >= 4096 and raw.numel() - (start + n) >= max(4096, min(nbytes, 1 << 20))
    assert bool((h.view == ONES).all())
    assert bool((raw[:start] == 0xC3).all()) and bool((raw[start + n:] == 0xC3).all())
    assert not bool(h.written().any())
    h.assert_guards_intact("untouched")


def test_only_the_two_hygiene_fills_are_taken():
    assert (hygiene._FILL["ones"], hygiene._FILL["huge"]) == (ONES, HUGE)
    for bad in (0x00, 0xC3, 0x5A):
        with pytest.raises(ValueError):
            hygiene.guarded(64, bad, device="cpu")


@pytest.mark.parametrize("nbytes", [16, 257, 5000])
def test_one_byte_past_the_end_is_reported_with_its_offset(nbytes):
    h = hygiene.guarded(nbytes, HUGE, device="cpu")
    start = h.view.data_ptr() - h._raw.data_ptr()
    h._raw[start + nbytes] = 0
    msg = _raises(h, "past")
    assert msg.startswith("past: wrote behind its %d bytes: 1 guard bytes changed" % nbytes)
    assert re.search(r"the first at end\+0, the last at end\+0$", msg)


@pytest.mark.parametrize("nbytes", [16, 257, 5000])
def test_one_byte_before_the_start_is_reported_with_its_offset(nbytes):
    h = hygiene.guarded(nbytes, ONES, device="cpu")
    start = h.view.data_ptr() - h._raw.data_ptr()
    h._raw[start - 1] = 7
    msg = _raises(h, "before")
    assert msg.startswith("before: wrote in front of its %d bytes: 1 guard bytes changed" % nbytes)
    assert re.search(r"the first at start-1, the last at start-1$", msg)
    h._raw[start - 1] = 0xC3
    h._raw[start - 4096] = 7                                  # the far end of the front guard
    assert re.search(r"the first at start-4096, the last at start-4096$", _raises(h))


@pytest.mark.parametrize("nbytes", [1, 4096, 300000, (1 << 20) + 1])
def test_the_far_end_of_the_back_guard_is_reported_with_its_offset(nbytes):
    h = hygiene.guarded(nbytes, ONES, device="cpu")
    n, back = max(nbytes, 16), max(4096, min(nbytes, 1 << 20))
    start = h.view.data_ptr() - h._raw.data_ptr()
    h._raw[start + n + back - 1] = 1
    assert re.search(r"1 guard bytes changed, the first at end\+%d, the last at end\+%d$" % (back - 1, back - 1), _raises(h))
    h._raw[start + n + 5] = 1
    assert re.search(r"2 guard bytes changed, the first at end\+5, the last at end\+%d$" % (back - 1), _raises(h))


def test_written_and_high_water_are_exact():
    n = 1000
    a, b = hygiene.guarded(n, ONES, device="cpu"), hygiene.guarded(n, HUGE, device="cpu")
    assert hygiene.high_water(a, b) == 0
    # the same "call" on both fills: bytes 3, 4, 700 and 811; it happens to write 0xFF at 811 and 0x7F at 700
    for h in (a, b):
        h.view[3] = 0; h.view[4] = 9; h.view[700] = HUGE; h.view[811] = ONES
    wa, wb = a.written().nonzero().flatten().tolist(), b.written().nonzero().flatten().tolist()
    assert wa == [3, 4, 700] and wb == [3, 4, 811]             # each run misses the byte set to its own fill
    assert hygiene.high_water(a, b) == 812 == hygiene.high_water(b, a)
    a.assert_guards_intact("a"); b.assert_guards_intact("b")
    a.view[n - 1] = 0
    assert hygiene.high_water(a, b) == n
    with pytest.raises(AssertionError):
        hygiene.high_water(a, hygiene.guarded(n, ONES, device="cpu"))      # two runs on one fill prove less


def test_typed_views_share_the_interior_and_small_outputs_end_at_the_guard():
    h = hygiene.guarded(4 * 6, ONES, device="cpu")
    t = h.typed(torch.float32, (2, 3))
    assert t.data_ptr() == h.view.data_ptr() and t.data_ptr() % 256 == 0 and bool(torch.isnan(t).all())
    t[1, 2] = 1.0
    assert h.written().nonzero().flatten().tolist() == [20, 21, 22, 23]    # 1.0f = 00 00 80 3f
    with pytest.raises(AssertionError):
        h.typed(torch.float64, (4,))
    s = hygiene.guarded(8, HUGE, device="cpu")                  # one double: `view` has 16 bytes, the output 8
    assert s.view.numel() == 16
    v = s.typed(torch.float64, (1,))
    assert s.nbytes == 8 and s.view.numel() == 8
    s.assert_guards_intact("scalar")
    start = v.data_ptr() - s._raw.data_ptr()
    s._raw[start + 8] = 0                                       # the ninth byte is guard now
    assert re.search(r"the first at end\+0, the last at end\+0$", _raises(s))


def test_retract_turns_the_interiors_tail_into_guard():
    h = hygiene.guarded(1024, ONES, device="cpu")
    ws = h.view                                                 # what the call is given: all 1024 bytes
    h.retract(256)
    h.assert_guards_intact("nothing written yet")
    ws[1000] = 0                                                # inside what the call owns, behind what the handle was told
    msg = _raises(h)
    assert re.search(r"its 768 bytes: 1 guard bytes changed, the first at end\+232, the last at end\+232$", msg)
