"""tests/seeded_vjp_reference.py without a GPU: the float64 vector-Jacobian products that tests/test_seeded_backward_gpu.py
compares the seeded entry points with are tied to the pinned float64 oracle, and the GPU test's own comparison, at each case's
own bar, is shown to REJECT a reference computed from the seeds a subtly wrong kernel would use -- by at least 100 times the bar."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import seeded_vjp_reference as R  # noqa: E402
import test_seeded_backward_gpu as G  # noqa: E402
from conftest import load_case  # noqa: E402


@pytest.mark.parametrize("name,user_masks", [("tm", False), ("relu_mh", True)])
def test_helper_equals_the_pinned_oracle_on_the_loss_seeds(name, user_masks, oracle64):
    """gz = z / B, gld = -1 / B are the seeds of loss = -mean log_prob under N(0, I): dS/dparams is oracle64.loss_grad's"""
    from oracle import Shape
    k = load_case(name)
    L, d, c, hidden, act = k["L"], k["d"], k["c"], k["hidden"], k["act"]
    rng = np.random.default_rng(3)
    masks = R.random_masks(L, d, rng) if user_masks else R.alternating_masks(L, d)
    assert user_masks or np.array_equal(masks, k["masks"])
    params = np.asarray(k["params"], np.float32)
    X, C = k["X"], k["C"]
    B = X.shape[0]
    geom = (d, c, hidden, act)
    flow = R.build_flow(params, masks, geom)
    with torch.no_grad():
        z, ld = R.forward_rows(flow, torch.from_numpy(X).double(), None if C is None else torch.from_numpy(C).double())
    got = R.forward_vjp(params, masks, geom, X, C, None, z.numpy() / B, np.full(B, -1.0 / B), torch.float64)
    loss, want = oracle64.loss_grad(Shape.make(L, d, c, hidden, act), params.astype(np.float64), X.astype(np.float64),
                                    None if C is None else C.astype(np.float64), masks=masks)
    assert R.rel_err(got["grad"], want) < 1e-10
    assert np.abs(got["z"] - z.numpy()).max() == 0.0
    # the zseed form of the same loss: its own loss_out is the log-det part alone
    zs = R.zseed_vjp(params, masks, geom, X, C, None, z.numpy() / B, 1.0 / B, torch.float64)
    assert R.rel_err(zs["grad"], want) < 1e-10
    prior = float((-0.5 * (z ** 2).sum(dim=1) - 0.5 * d * np.log(2 * np.pi)).sum()) / B
    assert abs(zs["loss"] - prior - float(loss)) < 1e-10 * max(1.0, abs(float(loss)))
    # a gathered batch is the direct walk over the gathered rows
    idx = rng.integers(0, B, size=B // 2)
    a = R.forward_vjp(params, masks, geom, X, C, idx, z.numpy()[:B // 2], np.arange(B // 2) / B, torch.float64)
    b = R.forward_vjp(params, masks, geom, X[idx], None if C is None else C[idx], None, z.numpy()[:B // 2], np.arange(B // 2) / B,
                      torch.float64)
    assert all(np.array_equal(a[key], b[key]) for key in ("grad", "gx") + (("gc",) if c else ()))
    # the inverse undoes the forward
    inv = R.inverse_vjp(params, masks, geom, z.numpy(), C, np.ones((B, d)), torch.float64)
    assert np.abs(inv["x"] - X.astype(np.float64)).max() < 1e-9 * max(1.0, float(np.abs(X).max()))


def _wrong_seeds(k, inp, ref):
    """the seeds a subtly wrong kernel would use, by name"""
    n = k.n
    gz, gld = inp["gz"], inp["gld"]
    out = {}
    if k.entry != "zseed" and n > 1:
        out["gld rolled by one row"] = (gz, np.roll(gld, 1))
        out["gld replaced by its mean"] = (gz, np.full_like(gld, gld.mean()))
    out["gz replaced by z / B"] = ((ref["ref"]["z"] / n).astype(np.float32), gld)
    if k.gather and n > 1:
        j = inp["idx"] % n
        out["seeds indexed through row_index"] = (gz[j], gld[j])
    return out


FORWARD = [k for k in G.CASES if k.entry != "inverse_backward" and not k.null]


@pytest.mark.parametrize("k", FORWARD, ids=[G._id(k) for k in FORWARD])
def test_the_comparison_rejects_a_reference_from_wrong_seeds(k):
    ref = G.reference(k)
    inp, geom = ref["inp"], G.geom_of(k)
    for key in ref["keys"]:             # float32 torch itself passes the comparison it sets the bar for
        if ref["ref"][key] is not None:
            assert R.close(ref["ref32"][key], ref["ref"][key], ref["bars"][key][1])
    for what, (gz, gld) in _wrong_seeds(k, inp, ref).items():
        if k.entry == "zseed":
            wrong = R.zseed_vjp(inp["params"], inp["masks"], geom, inp["X"], inp["C"], inp["idx"], gz, inp["inv_B"])
        else:
            wrong = R.forward_vjp(inp["params"], inp["masks"], geom, inp["X"], inp["C"], inp["idx"], gz, gld)
        e32, bar = ref["bars"]["grad"]
        off = R.rel_err(wrong["grad"], ref["ref"]["grad"])
        print("%s: %s: grad_out %.2e of scale, bar %.2e" % (G._id(k), what, off, bar))
        assert not R.close(wrong["grad"], ref["ref"]["grad"], bar), what
        assert off >= 100 * bar, "%s: only %.2e of scale, bar %.2e" % (what, off, bar)


def test_every_case_is_in_the_docstring_table_and_within_the_limit():
    doc = G.__doc__
    for k in G.CASES:
        assert ("\n%s " % G._id(k)) in doc, G._id(k)
        for key, (e32, bar) in G.reference(k)["bars"].items():
            assert bar <= R.BAR_LIMIT, (G._id(k), key, e32, bar)
