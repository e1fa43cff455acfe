"""The shapes, batches and expected regimes of the tiling tests, shared by tests/test_tilings_host.py (which proves on the CPU
that the large cases can see a dropped row) and tests/test_wgan_tilings_gpu.py / tests/test_cnormal_tilings_gpu.py.

A regime is what the host picks for a (shape, rows): the step tile R, the workgroups G and whether the launch asks for more
than 64 KiB of LDS.  The numbers here are expectations: every test asserts them through pfw_tiling / pfn_tiling before it runs
anything, so retuning the host constants fails the tests instead of silently moving them to another regime.

Large batches: at 16 385 rows one row is 6e-5 of a mean.  Every case of at least BIG rows scales the inputs of three batch rows
-- the last row (alone in the last tile), the first row of the second tile and the last row of the first tile -- by SCALE, so
that a kernel that dropped one of them misses the bar by a wide margin."""
import numpy as np

BIG = 2049          # cases with at least this many rows carry scaled edge rows
# Chosen on the CPU: test_tilings_host.py::test_*_large_cases_see_a_dropped_edge_row prints, per case and edge row, by how many
# bars of the GPU test the float64 gradient moves when that row's term is removed, and requires 10.  Measured minimum over all
# large cases: 60 bars unscaled (the bar is a few float32 ulp of max |g|, and one row's largest entries are not 6e-5 of it),
# 212 bars at 4, 1730 at 32.  4 keeps a 20-fold margin over the requirement without letting three rows dominate the sums that
# every other row has to show up in.  A power of two: the scaling itself is exact in float32.
SCALE = 4.0

# ---- ConditionalWGAN ------------------------------------------------------------------------------------------------------
W_SHAPES = {   # name: ((d, c, latent, g_hidden, d_hidden), g_act, d_act)
    "full_wg": ((4, 0, 3, (12, 10), (9,)), 'relu', 'relu'),
    "odd_cap": ((4, 0, 3, (30, 30), (25,)), 'relu', 'relu'),
    "big_lds": ((5, 3, 1, (256, 256), (256, 256)), 'tanh', 'relu'),
    "cap13": ((5, 3, 1, (160,) * 3, (160,) * 3), 'relu', 'relu'),
    "cap2": ((5, 3, 1, (1024, 1024), (1024, 1024)), 'relu', 'tanh'),
    "cap1": ((5, 3, 1, (2048, 2048), (1024,)), 'tanh', 'tanh'),
    "last": ((1, 0, 1, (3412,), (1,)), 'relu', 'relu'),          # the largest g_hidden whose step still fits LDS
    "gen_only": ((1, 0, 1, (8000,), (1,)), 'relu', 'relu'),      # no step, no epoch losses: pfw_generate at tile 1
}
W_STEPS = [    # (shape name, rows, R, step cap, G, LDS bytes of k_step)
    ("full_wg", 16385, 128, 128, 129, 77100),     # a critic step stages 2R = 256 LDS rows: every thread a row
    ("full_wg", 4097, 32, 128, 129, 19500),
    ("full_wg", 8193, 64, 128, 129, 38700),
    ("odd_cap", 16385, 111, 111, 148, 163236),    # R = cap, not a power of two; S = 223
    ("big_lds", 1, 8, 10, 1, 122740),
    ("big_lds", 7, 8, 10, 1, 122740),
    ("big_lds", 8, 8, 10, 1, 122740),
    ("big_lds", 9, 8, 10, 2, 122740),
    ("big_lds", 33, 8, 10, 5, 122740),
    ("cap13", 2049, 13, 13, 158, 156924),
    ("cap13", 3400, 13, 13, 262, 156924),         # G > 256
    ("cap2", 1, 2, 2, 1, 143620),
    ("cap2", 2, 2, 2, 1, 143620),
    ("cap2", 3, 2, 2, 2, 143620),
    ("cap2", 5, 2, 2, 3, 143620),
    ("cap1", 1, 1, 1, 1, 135324),
    ("cap1", 3, 1, 1, 3, 135324),
    ("last", 2, 1, 1, 2, 163824),
]

# ---- ConditionalNormal ----------------------------------------------------------------------------------------------------
N_SHAPES = {   # name: (d, c, hidden, activation, independent)
    "full_wg": (6, 2, (4,) * 8, 'relu', False),
    "big_lds": (32, 3, (512, 512), 'tanh', False),
    "cap11": (8, 3200, (16,), 'relu', False),                     # a cap of 9..15 from wide conditions: few parameters
    "cap3": (32, 3, (2048, 2048), 'sigmoid', False),
    "cap1": (32, 2, (4096, 2048), 'relu', True),
    "last": (1, 1, (6823,), 'relu', False),                       # the largest hidden whose step still fits LDS
    "wide_fwd": (32, 3, (10,), 'tanh', False),                    # pfn_forward: tile 256 at 132 548 B
}
N_STEPS = [    # (shape name, rows, R, step cap, G, LDS bytes of k_step)
    ("full_wg", 32769, 256, 256, 129, 63444),     # every thread a row
    ("full_wg", 2049, 16, 256, 129, 4884),
    ("full_wg", 4097, 32, 256, 129, 8788),
    ("full_wg", 8193, 64, 256, 129, 16596),
    ("full_wg", 16385, 128, 256, 129, 32212),
    ("big_lds", 1, 8, 15, 1, 97824),
    ("big_lds", 8, 8, 15, 1, 97824),
    ("big_lds", 9, 8, 15, 2, 97824),
    ("big_lds", 33, 8, 15, 5, 97824),
    ("big_lds", 2049, 15, 15, 137, 157968),       # R = cap, not a power of two
    ("cap3", 1, 3, 3, 1, 153168),
    ("cap3", 3, 3, 3, 1, 153168),
    ("cap3", 5, 3, 3, 2, 153168),
    ("cap1", 1, 1, 1, 1, 135976),
    ("cap1", 3, 1, 1, 3, 135976),
    ("last", 2, 1, 1, 2, 163840),
]


# e_ref of the long chains.  The bar is 4 e_ref (tests/parity.py), e_ref the error of the float32 restatement.  torch's float32
# matmul splits a sum over vector lanes and blocks, so its error hardly grows with the length of the sum; the kernels
# accumulate a layer's fan-in in ONE fmaf chain per row, whose rounding error grows with the chain.  Where a layer has at least
# LONG_FAN_IN inputs, e_ref is therefore the larger of two float32 restatements' errors: torch's, and the same restatement
# summed in the kernels' order on the CPU (`sequential` fan-in, tile by tile in tile order: ordered32 below).  In this class
# gpu / e_ref(torch) is 4.1 .. 19.8 and gpu / e_ref(kernel order) 0.9 .. 1.7 (profiles/r11_tilings_parity.txt).  Every other
# case keeps torch's e_ref alone.
LONG_FAN_IN = 1024

# ReLU kinks.  A pre-activation within float32 rounding of 0 can come out on the other side of the kink on the GPU; the unit's
# whole term of that row then enters or leaves the gradient, which is no rounding error and which no bar covers.  3400 rows x
# 960 ReLU units cannot all be far from 0, but the seed can be chosen so that none is closer than KINK, several times the
# float32 error of a pre-activation here (~2e-7): test_tilings_host.py asserts it for every large ReLU case of both libraries.
KINK = 1e-6
W_SEEDS = {"cap13-2049": 1, "cap13-3400": 7}       # every other case: seed 0

# The floor of a bar is 4 float32 ulp of max |float64 value| (tests/parity.py).  One quantity needs another magnitude: the
# critic loss of big_lds-33 is -0.094, the difference of two means over 33 rows of D outputs whose last Linear sums terms
# of 11.8 in all (mean over the rows of |b| + sum_i |h_i w_i|).  A float32 sum of cancelling terms carries an error relative
# to the terms, not to what is left of them: the GPU is 2.34e-7 from float64, 2.5e-6 of |loss| but 2e-8 of the terms, and
# torch's float32 restatement happened to land 1.8e-8 away, so that the plain bar is 7.2e-8.  For this quantity alone the
# magnitude is that of the terms (profiles/r11_tilings_parity.txt has the figures); every other loss, pfw_critic and
# pfw_epoch_losses comparison keeps max |float64 value|.
TERMS_MAGNITUDE = {("big_lds-33", "critic loss")}


def w_long(name):
    (d, c, lat, gh, dh), _, _ = W_SHAPES[name]
    return max((lat + c, d + c) + tuple(gh) + tuple(dh)) >= LONG_FAN_IN


def n_long(name):
    d, c, hidden, _, _ = N_SHAPES[name]
    return max((c,) + tuple(hidden)) >= LONG_FAN_IN


def ordered32(tile_loss_grad, rows, R):
    """float32 (loss, gradient) of a batch summed as the kernels sum it: tile_loss_grad(s, e) is the float32 restatement's
    mean loss and its gradient over batch rows s..e-1 (one workgroup's tile); the tiles' sums are added in tile order, one
    rounding per add, and divided by the batch size at the end"""
    f = np.float32
    L, G = f(0), None
    for s in range(0, rows, R):
        e = min(rows, s + R)
        l, g = tile_loss_grad(s, e)
        g = np.asarray(g, f) * f(e - s)
        G = g if G is None else G + g
        L = L + f(l) * f(e - s)
    return L / f(rows), G / f(rows)


def step_id(case):
    return "%s-%d" % (case[0], case[1])


def edge_rows(rows, R):
    """batch positions whose inputs are scaled: the last row, the first row of the second tile, the last of the first"""
    return [rows - 1, R, R - 1] if rows >= BIG else []


def _tag(name):
    return sum(ord(ch) * (i + 1) for i, ch in enumerate(name))


def _linear(rng, n_in, n_out, gain):
    """He-style weights (a deep narrow ReLU net must stay alive), a wide bias"""
    W = rng.normal(size=(n_out, n_in)) * gain / np.sqrt(n_in)
    b = rng.uniform(-0.5, 0.5, size=n_out)
    return [W.reshape(-1), b]


def _mlp(rng, n_in, hidden, n_out, gain):
    out, i = [], n_in
    for o in list(hidden) + [n_out]:
        out += _linear(rng, i, o, gain)
        i = o
    return out


def wgan_problem(name, rows, R, seed=None):
    """(params [PG + PD], X, C, row_index, z) of one step case: the batch is `rows` rows picked through row_index from a
    table of rows + 3 rows"""
    (d, c, lat, gh, dh), ga, da = W_SHAPES[name]
    seed = W_SEEDS.get("%s-%d" % (name, rows), 0) if seed is None else seed
    rng = np.random.default_rng([seed, _tag(name)])
    p = np.concatenate(_mlp(rng, lat + c, gh, d, 1.4) + _mlp(rng, d + c, dh, 1, 1.4)).astype(np.float32)
    rng = np.random.default_rng([seed, _tag(name), rows])
    n = rows + 3
    X = rng.normal(size=(n, d)).astype(np.float32)
    C = rng.normal(size=(n, c)).astype(np.float32) if c else None
    ri = rng.permutation(n)[:rows]
    z = rng.normal(size=(rows, lat)).astype(np.float32)
    for r in edge_rows(rows, R):
        X[ri[r]] *= SCALE
        z[r] *= SCALE
        if c:
            C[ri[r]] *= SCALE
    return p, X, C, ri, z


def cnormal_problem(name, rows, R, seed=0):
    """(params [P], X, C, row_index) of one step case; out.weight is I + noise (well conditioned for any d)"""
    d, c, hidden, act, indep = N_SHAPES[name]
    rng = np.random.default_rng([seed, _tag(name)])
    hl = hidden[-1]
    parts = _mlp(rng, c, hidden[:-1], hl, 1.4 if act == 'relu' else 1.0)
    parts += _linear(rng, hl, d, 0.5) + _linear(rng, hl, d, 0.2)
    Wo = np.eye(d) + rng.normal(size=(d, d)) * 0.3 / np.sqrt(d)
    parts += [Wo.reshape(-1), rng.uniform(-0.5, 0.5, size=d)]
    p = np.concatenate(parts).astype(np.float32)
    rng = np.random.default_rng([seed, _tag(name), rows])
    n = rows + 3
    X = rng.normal(size=(n, d)).astype(np.float32)
    C = rng.normal(size=(n, c)).astype(np.float32)
    ri = rng.permutation(n)[:rows]
    for r in edge_rows(rows, R):
        X[ri[r]] *= SCALE
    return p, X, C, ri
