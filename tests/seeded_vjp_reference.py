"""Reference for the library's SEEDED backward entry points (include/rnvp_hip.h: rnvp_backward, rnvp_backward_cond,
rnvp_inverse_backward, rnvp_loss_grad_zseed): the same vector-Jacobian products formed by torch autograd on the CPU over the
eager restatement of the flow, oracle/torch_cpu.py::EagerFlow, in float64 (the reference) or float32 (what plain float32
arithmetic gives: the yardstick the comparison bar is derived from).  TEST INFRASTRUCTURE ONLY; nothing here touches a GPU.

Every function takes
    params     flat float32 parameters in nf.parameters() order (per layer: net t then net s; per Linear: weight, bias)
    masks      [L, d] table of {0, 1}
    geom       (d, c, hidden, activation)
    X or Z     [m, d] source rows;  C  [m, c] or None;  row_index  None or [n] int64: batch row r reads source row row_index[r]
and the caller's seeds IN BATCH ORDER, and returns float64 numpy arrays, the input gradients per BATCH row as the header fixes it
(rnvp_hip.h, rnvp_backward: "with row_index the inputs are gathered, gz / gld / gx_out are not").
"""
import numpy as np
import torch

from oracle.torch_cpu import EagerFlow

TOL = 3e-6              # the project's bar for these gradients (test_autograd_gpu.TOL), of the reference array's largest magnitude
BAR_FACTOR = 4.0        # ... or this many times what float32 eager torch shows against float64 on the same case
BAR_LIMIT = 2e-5        # no case may need more than this


def linear_shapes(d, c, hidden):
    dims = [d + c] + list(hidden) + [d]
    return [(dims[k + 1], dims[k]) for k in range(len(dims) - 1)]


def init_params(L, d, c, hidden, rng, scale=2.0):
    """flat float32 parameters: torch.nn.Linear's default U(-1/sqrt(fan_in), 1/sqrt(fan_in)) times `scale`"""
    parts = []
    for _ in range(2 * L):
        for (o, i) in linear_shapes(d, c, hidden):
            b = scale / np.sqrt(i)
            parts.append(rng.uniform(-b, b, size=o * i))
            parts.append(rng.uniform(-b, b, size=o))
    return np.concatenate(parts).astype(np.float32)


def alternating_masks(L, d):
    return ((np.arange(d)[None] + np.arange(L)[:, None]) % 2).astype(np.uint8)


def random_masks(L, d, rng):
    """a user mask table: random, every layer neither all ones nor all zeros"""
    m = rng.integers(0, 2, size=(L, d)).astype(np.uint8)
    for l in range(L):
        j = int(rng.integers(d))
        m[l, j] = 1; m[l, (j + 1) % d] = 0
    return m


def build_flow(params, masks, geom, dtype=torch.float64):
    d, c, hidden, act = geom
    masks = np.asarray(masks)
    flow = EagerFlow(masks.shape[0], d, c, hidden, act).to(dtype)
    flow.load_flat(np.asarray(params, np.float32).astype(np.float64))
    flow.masks = [torch.from_numpy(m.astype(np.int64)) for m in masks]
    return flow


def _params_of(flow):
    out = []
    for t, s in zip(flow.nets_t, flow.nets_s):
        out += list(t.parameters()) + list(s.parameters())
    return out


def forward_rows(flow, X, C):
    """(z, logdet) rows of the flow: the layers of EagerFlow.log_prob_rows without the prior term"""
    x, ld = X, torch.zeros(X.shape[0], dtype=X.dtype)
    for m, nt, ns in zip(flow.masks, flow.nets_t, flow.nets_s):
        xc = torch.cat([x * m, C], dim=1) if C is not None else x * m
        T, S = nt(xc), ns(xc)
        x = (x * torch.exp(S) + T) * (1 - m) + x * m
        ld = ld + (S * (1 - m)).sum(dim=-1)
    return x, ld


def _t(a, dtype):
    return None if a is None else torch.as_tensor(np.asarray(a)).to(dtype)


def _gather(src, row_index, dtype):
    if src is None:
        return None
    t = _t(src, dtype)
    if row_index is not None:
        t = t[torch.as_tensor(np.asarray(row_index, np.int64))]
    return t.clone().requires_grad_(True)


def _np64(t):
    return None if t is None else t.detach().to(torch.float64).numpy()


def _vjp(S, flow, leaves):
    ps = _params_of(flow)
    ins = ps + [t for t in leaves if t is not None]
    gs = torch.autograd.grad(S, ins, allow_unused=True)
    gs = [torch.zeros_like(t) if g is None else g for g, t in zip(gs, ins)]
    grad = torch.cat([g.reshape(-1) for g in gs[:len(ps)]])
    rest = iter(gs[len(ps):])
    return [_np64(grad)] + [None if t is None else _np64(next(rest)) for t in leaves]


def forward_vjp(params, masks, geom, X, C, row_index, gz, gld, dtype=torch.float64):
    """(z, logdet) = f(x[row_index], c[row_index]);  S = sum(gz * z) + sum(gld * logdet)
    -> dict(grad = dS/dparams [P], gx = dS/dx [n, d], gc = dS/dc [n, c] or None, z [n, d], logdet [n])"""
    flow = build_flow(params, masks, geom, dtype)
    x, c = _gather(X, row_index, dtype), _gather(C, row_index, dtype)
    z, ld = forward_rows(flow, x, c)
    S = (_t(gz, dtype) * z).sum() + (_t(gld, dtype) * ld).sum()
    grad, gx, gc = _vjp(S, flow, [x, c])
    return dict(grad=grad, gx=gx, gc=gc, z=_np64(z), logdet=_np64(ld))


def zseed_vjp(params, masks, geom, X, C, row_index, gz, inv_B, dtype=torch.float64):
    """rnvp_loss_grad_zseed:  S = sum(gz * z) - inv_B * sum(logdet)  -> dict(grad, loss = -inv_B * sum(logdet), z)"""
    flow = build_flow(params, masks, geom, dtype)
    x, c = _gather(X, row_index, dtype), _gather(C, row_index, dtype)
    z, ld = forward_rows(flow, x, c)
    loss = -float(inv_B) * ld.sum()
    S = (_t(gz, dtype) * z).sum() + loss
    grad, _, _ = _vjp(S, flow, [x, c])
    return dict(grad=grad, loss=float(loss.detach()), z=_np64(z))


def inverse_vjp(params, masks, geom, Z, C, gx, dtype=torch.float64):
    """x = g(z, c);  S = sum(gx * x)  -> dict(grad = dS/dparams, gz = dS/dz, gc = dS/dc or None, x)"""
    flow = build_flow(params, masks, geom, dtype)
    z, c = _gather(Z, None, dtype), _gather(C, None, dtype)
    x = flow.inverse_rows(z, c)
    S = (_t(gx, dtype) * x).sum()
    grad, gz, gc = _vjp(S, flow, [z, c])
    return dict(grad=grad, gz=gz, gc=gc, x=_np64(x))


# ---- the comparison --------------------------------------------------------------------------------------------------------
def rel_err(got, want):
    """largest absolute difference, as a fraction of the reference array's largest magnitude"""
    want = np.asarray(want, np.float64); got = np.asarray(got, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    return float(np.abs(got - want).max()) / max(float(np.abs(want).max()), 1e-30)


def bar_for(e32):
    """the bar of one returned array: the project's 3e-6, or four times the error of float32 eager torch on the same case --
    the factor covers another summation order and the kernels' tanh / exp against libm; it is the ratio between the
    project's 3e-6 and what float32 torch shows on the existing autograd cases"""
    return max(TOL, BAR_FACTOR * float(e32))


def bars(ref64, ref32, keys):
    """{key: (e32, bar)} for the arrays named by `keys`; refuses a case whose reference alone pushes a bar past BAR_LIMIT"""
    out = {}
    for k in keys:
        if ref64[k] is None:
            continue
        assert np.isfinite(ref64[k]).all() and np.isfinite(ref32[k]).all(), "%s: the reference overflows: tame the case" % k
        e32 = rel_err(ref32[k], ref64[k])
        out[k] = (e32, bar_for(e32))
        assert out[k][1] <= BAR_LIMIT, "%s: float32 torch is %.2e from float64, bar %.2e > %.0e: tame the case" % (k, e32, out[k][1], BAR_LIMIT)
    return out


def close(got, want, bar):
    """the test's comparison: True when `got` is within `bar` of scale of `want`"""
    return rel_err(got, want) < bar


def loss_close(got, want):
    """the existing bar for a batch loss"""
    return abs(float(got) - float(want)) < max(1e-5, 5e-7 * abs(float(want)))
