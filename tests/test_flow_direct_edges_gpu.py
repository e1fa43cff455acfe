"""The d <= 16 barrier-free ("direct") form of the split-bf16 flow kernel (k_flow_bx3, rnvp_bx3.hip) at the edges of its
schedule: the first and last layer (nothing before / after to prefetch for), one, two, three and an odd number of hidden tiles
per stage, the instantiation without conditions, partial rows, the wave (48 rows) and workgroup (192 rows) edges of 3 row tiles x
4 waves, and one row count above the grid cap, where workgroups take unequal numbers of row groups and the last one is ragged.
Every case runs with precision='bx3', so the direct form runs whatever `auto` would pick.  Tolerances: those of
tests/test_hip_kernels.py (test_mfma_path_edge_shapes_vs_oracle, test_forward_vs_golden_and_oracle,
test_fused_sample_equals_prior_then_inverse) for the same entry points."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# (L, d, c, hidden, activation)
SHAPES = [(1, 16, 4, 128, "tanh"),       # no next layer to prefetch
          (2, 16, 4, 128, "tanh"),
          (3, 16, 0, 128, "tanh"),       # the CQ = 0 instantiation; odd L
          (2, 10, 3, 72, "tanh"),        # partial rows and conditions (guarded loads); 5 hidden tiles: the loop's odd tail
          (2, 16, 4, 16, "tanh"),        # one tile per stage
          (2, 16, 4, 32, "tanh"),        # two
          (2, 16, 4, 48, "tanh"),        # three
          (2, 16, 4, 128, "relu")]
ROWS = [1, 47, 48, 49, 191, 192, 193]    # wave and workgroup edges at 3 row tiles x 4 waves
N_REF = max(ROWS)
WG_ROWS = 192
GRID_CAP_ROWS = 2048 * WG_ROWS           # the direct form's grid cap (2 048 workgroups) in rows
N_LARGE = GRID_CAP_ROWS + WG_ROWS + 5    # workgroups 0 and 1 take a second row group; the last one holds 5 rows
SEED = 1234


def _dev(a, dtype=torch.float32):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a)).to(dtype).cuda().contiguous()


class _Flow:
    """one shape: parameters, inputs and the float64 oracle's results for the first N_REF rows (computed once per module)"""

    def __init__(self, spec, oracle64):
        from oracle import Shape
        from probaforms_amd import _hip
        L, d, c, h, act = spec
        self._hip, self.L, self.d, self.c = _hip, L, d, c
        self.shape = _hip.RnvpShape.make(L, d, c, (h,), act, alt_masks=1, precision="bx3")
        rng = np.random.default_rng(L * 1000 + d * 31 + c * 7 + h)
        P = _hip.param_count(self.shape)
        params = (rng.uniform(-1, 1, size=P) * 0.12).astype(np.float32)
        self.X = rng.normal(size=(N_REF, d)).astype(np.float32)
        self.C = rng.normal(size=(N_REF, c)).astype(np.float32) if c else None
        self.Z = rng.normal(size=(N_REF, d)).astype(np.float32)
        so = Shape.make(L, d, c, (h,), act)
        z, lp, _ = oracle64.log_prob(so, params, self.X, self.C)
        self.z_ref, self.lp_ref = np.asarray(z, np.float64), np.asarray(lp, np.float64)
        self.ld_ref = self.lp_ref + 0.5 * (self.z_ref ** 2).sum(1) + 0.5 * d * np.log(2.0 * np.pi)
        self.x_ref = np.asarray(oracle64.sample(so, params, self.Z, self.C), np.float64)
        self.params = _dev(params)
        self.masks = _dev(((np.arange(d)[None] + np.arange(L)[:, None]) % 2).astype(np.uint8), torch.uint8)

    def ws(self, op, n):
        return torch.empty(max(self._hip.workspace_bytes(self.shape, op, n), 16), dtype=torch.uint8, device="cuda")

    def forward(self, x, c, n, row_index=None):
        z = torch.empty(n, self.d, device="cuda"); ld = torch.empty(n, device="cuda"); lp = torch.empty(n, device="cuda")
        tot = torch.empty(1, device="cuda")
        self._hip.forward_logprob(self.shape, self.params, self.masks, x, c, row_index, n, z, ld, lp, tot, self.ws(self._hip.OP_FORWARD, n))
        disp = self._hip.last_dispatch(self._hip.PROFILE_FORWARD)
        assert disp["kernel"] == "k_flow_bx3" and disp["variant"] == "bx3_direct" and disp["rows"] == n, disp
        assert disp["row_tiles"] * 16 * disp["waves"] == WG_ROWS, disp           # ROWS and the slices below are this geometry's edges
        assert disp["grid"] == min((n + WG_ROWS - 1) // WG_ROWS, GRID_CAP_ROWS // WG_ROWS), disp
        return z, ld, lp, tot

    def inverse(self, z, c, n):
        x = torch.empty(n, self.d, device="cuda")
        self._hip.inverse(self.shape, self.params, self.masks, z, c, n, x, self.ws(self._hip.OP_INVERSE, n))
        disp = self._hip.last_dispatch(self._hip.PROFILE_INVERSE)
        assert disp["kernel"] == "k_flow_bx3" and disp["variant"] == "bx3_direct" and disp["rows"] == n, disp
        return x

    def sample(self, c, n, row_offset):
        x = torch.empty(n, self.d, device="cuda")
        self._hip.sample(self.shape, self.params, self.masks, c, n, SEED, row_offset, x, self.ws(self._hip.OP_INVERSE, n))
        return x


_FLOWS = {}


@pytest.fixture(params=SHAPES, ids=lambda s: "L%d_d%d_c%d_h%d_%s" % s)
def flow(request, oracle64):
    if request.param not in _FLOWS:
        _FLOWS[request.param] = _Flow(request.param, oracle64)
    return _FLOWS[request.param]


def _cut(t, a, b):
    return None if t is None else t[a:b].contiguous()


@pytest.mark.parametrize("n", ROWS)
def test_forward_inverse_vs_float64_oracle_and_round_trip(flow, n):
    f = flow
    x, c = _dev(f.X[:n]), _dev(None if f.C is None else f.C[:n])
    z, ld, lp, tot = f.forward(x, c, n)
    zr, ldr, lpr = f.z_ref[:n], f.ld_ref[:n], f.lp_ref[:n]
    zh, ldh, lph = z.cpu().numpy(), ld.cpu().numpy(), lp.cpu().numpy()
    assert np.abs(zh - zr).mean() < 2e-6 and np.abs(zh - zr).max() < 2e-4
    np.testing.assert_allclose(ldh, ldr, rtol=1e-5, atol=1e-5 * max(1.0, np.abs(ldr).max()))
    assert np.abs(lph - lpr).mean() < max(1e-5, 2.4e-7 * np.abs(lpr).max())
    assert abs(float(tot) - lpr.sum()) < 2e-5 * max(1.0, np.abs(lpr).sum())
    # the inverse on the oracle's own input, against the oracle
    xs = f.inverse(_dev(f.Z[:n]), c, n).cpu().numpy()
    want = f.x_ref[:n]
    assert np.abs(xs - want).mean() < 5e-6 * max(1.0, np.abs(want).mean())
    # round trip
    back = f.inverse(z, c, n).cpu().numpy()
    assert np.abs(back - f.X[:n]).mean() < 2e-6 and np.abs(back - f.X[:n]).max() < 5e-4
    # the same call twice: bit for bit
    z2, ld2, lp2, tot2 = f.forward(x, c, n)
    assert torch.equal(z, z2) and torch.equal(ld, ld2) and torch.equal(lp, lp2) and torch.equal(tot, tot2)
    assert torch.equal(f.sample(c, n, 5), f.sample(c, n, 5))


def _check_slices(f, n, x, c, slices):
    z, ld, lp, _ = f.forward(x, c, n)
    xs = f.sample(c, n, 0)
    z2, ld2, lp2, _ = f.forward(x, c, n)
    assert torch.equal(z, z2) and torch.equal(ld, ld2) and torch.equal(lp, lp2) and torch.equal(xs, f.sample(c, n, 0))
    for a, b in slices:
        m = b - a
        assert torch.equal(f.sample(_cut(c, a, b), m, a), xs[a:b]), (a, b)
        za, lda, lpa, _ = f.forward(_cut(x, a, b), _cut(c, a, b), m)
        assert torch.equal(za, z[a:b]) and torch.equal(lda, ld[a:b]) and torch.equal(lpa, lp[a:b]), (a, b)
        idx = torch.arange(a, b, device="cuda", dtype=torch.int64)
        zi, ldi, lpi, _ = f.forward(x, c, m, idx)
        assert torch.equal(zi, z[a:b]) and torch.equal(ldi, ld[a:b]) and torch.equal(lpi, lp[a:b]), (a, b)
    return z, ld, lp


def test_slices_across_wave_and_workgroup_edges_are_bitwise_equal(flow):
    f = flow
    n = 2 * WG_ROWS + 49
    g = torch.Generator(device="cuda").manual_seed(7)
    x = torch.randn(n, f.d, device="cuda", generator=g)
    c = torch.randn(n, f.c, device="cuda", generator=g) if f.c else None
    z, ld, lp = _check_slices(f, n, x, c, [(150, 250), (47, 49), (WG_ROWS - 1, 2 * WG_ROWS + 1), (WG_ROWS, n), (n - 1, n)])
    # gathered rows in any order: row r of the call is row row_index[r] of the inputs
    idx = torch.randperm(n, device="cuda", generator=g)[:WG_ROWS + 7].contiguous()
    zi, ldi, lpi, _ = f.forward(x, c, idx.numel(), idx)
    assert torch.equal(zi, z[idx]) and torch.equal(ldi, ld[idx]) and torch.equal(lpi, lp[idx])


def test_slices_across_the_grid_stride_edge_are_bitwise_equal(flow):
    """above the grid cap: workgroups 0 and 1 run a second row group (rows GRID_CAP_ROWS ...), the very last holds 5 rows"""
    f = flow
    n = N_LARGE
    g = torch.Generator(device="cuda").manual_seed(11)
    x = torch.randn(n, f.d, device="cuda", generator=g)
    c = torch.randn(n, f.c, device="cuda", generator=g) if f.c else None
    _check_slices(f, n, x, c, [(GRID_CAP_ROWS - 100, GRID_CAP_ROWS + 100),         # the grid-stride edge
                               (GRID_CAP_ROWS + WG_ROWS - 3, n),                    # into the ragged last row group
                               (WG_ROWS - 50, WG_ROWS + 50),                        # a workgroup edge of the first round
                               (GRID_CAP_ROWS - 1, GRID_CAP_ROWS + 1)])
