"""The four C entry points that take per-row gradient seeds from the caller -- rnvp_backward, rnvp_backward_cond,
rnvp_inverse_backward and rnvp_loss_grad_zseed (include/rnvp_hip.h) -- called through probaforms_amd._hip with ARBITRARY seeds
(gz ~ N(0,1)/n, gld ~ N(0,1)/n per row) and compared, every returned array in full, with the float64 vector-Jacobian product of
the eager flow under torch autograd on the CPU (tests/seeded_vjp_reference.py).  The loss's own seeds (gz = z / B, a uniform
gld = -1 / B) cannot see a seed read from the wrong row, or a kernel that ignores the caller's gz for its built-in N(0, I) one;
tests/test_seeded_vjp_reference.py shows that this comparison rejects exactly those mistakes.

Each case first asserts with rnvp_last_dispatch that the kernel it was written for ran (kernel, variant, row tiles per
workgroup or wave), so a later change of a dispatch threshold cannot silently empty it.  L = 3 throughout (an inner layer, both
mask parities); weights: torch.nn.Linear's default scale times 2 (times 1 for hidden = (512,), as test_autograd_gpu._build).

The bar of an array is max(3e-6, 4 * e32) of the reference's largest magnitude, e32 being what float32 eager torch on the CPU
shows against float64 on the same case (seeded_vjp_reference.bar_for); it is computed inside the test, and no bar may exceed
2e-5.  The table lists, per case, the kernel that serves it and the largest e32 / bar over its arrays as measured when the
cases were written (e32 moves a little with the BLAS of the host; the test uses its own figure):

case                                   kernel (variant, row tiles)     e32      bar
backward-nf2-n1                        k_mfma_train_ts (tilesplit, 1)  1.8e-07  3.0e-06
backward-nf2-n15                       k_mfma_train_ts (tilesplit, 1)  6.6e-07  3.0e-06
backward-nf2-n16                       k_mfma_train_ts (tilesplit, 1)  5.8e-07  3.0e-06
backward-nf2-n17                       k_mfma_train_ts (tilesplit, 1)  5.3e-07  3.0e-06
backward-nf2-n4096                     k_mfma_train_ts (tilesplit, 1)  1.1e-06  4.6e-06
backward-nf2-n4097                     k_mfma_train_ts (tilesplit, 2)  7.0e-07  3.0e-06
backward-nf2-n8192                     k_mfma_train_ts (tilesplit, 2)  1.7e-06  6.8e-06
backward-nf2-n8193                     k_lmm_train64 (lmm, 4)          7.1e-07  3.0e-06
backward-nf2c0-n1                      k_mfma_train_ts (tilesplit, 1)  2.9e-07  3.0e-06
backward-nf2c0-n15                     k_mfma_train_ts (tilesplit, 1)  4.7e-07  3.0e-06
backward-nf2c0-n16                     k_mfma_train_ts (tilesplit, 1)  3.2e-07  3.0e-06
backward-nf2c0-n17                     k_mfma_train_ts (tilesplit, 1)  3.3e-07  3.0e-06
backward-nf2c0-n4096                   k_mfma_train_ts (tilesplit, 1)  4.1e-07  3.0e-06
backward-nf2c0-n4097                   k_mfma_train_ts (tilesplit, 2)  7.0e-07  3.0e-06
backward-nf2c0-n8192                   k_mfma_train_ts (tilesplit, 2)  5.2e-07  3.0e-06
backward-nf2c0-n8193                   k_lmm_train64 (lmm, 4)          4.7e-07  3.0e-06
backward-nf4-n1                        k_mfma_train_ts (tilesplit, 1)  7.8e-07  3.1e-06
backward-nf4-n15                       k_mfma_train_ts (tilesplit, 1)  5.8e-07  3.0e-06
backward-nf4-n16                       k_mfma_train_ts (tilesplit, 1)  5.6e-07  3.0e-06
backward-nf4-n17                       k_mfma_train_ts (tilesplit, 1)  3.3e-07  3.0e-06
backward-nf4-n4096                     k_mfma_train_ts (tilesplit, 1)  7.0e-07  3.0e-06
backward-nf4-n4097                     k_mfma_train_ts (tilesplit, 2)  9.6e-07  3.8e-06
backward-nf4-n8192                     k_mfma_train_ts (tilesplit, 2)  7.8e-07  3.1e-06
backward-nf4-n8193                     k_lmm_train64 (lmm, 4)          1.1e-06  4.4e-06
backward-nf8-n1                        k_mfma_train_ts (tilesplit, 1)  2.0e-07  3.0e-06
backward-nf8-n15                       k_mfma_train_ts (tilesplit, 1)  4.5e-07  3.0e-06
backward-nf8-n16                       k_mfma_train_ts (tilesplit, 1)  8.8e-07  3.5e-06
backward-nf8-n17                       k_mfma_train_ts (tilesplit, 1)  7.5e-07  3.0e-06
backward-nf8-n4096                     k_mfma_train_ts (tilesplit, 1)  1.7e-06  6.9e-06
backward-nf8-n4097                     k_lmm_train (lmm, 1)            6.9e-07  3.0e-06
backward-nf8-n8192                     k_lmm_train64 (lmm, 4)          8.5e-07  3.4e-06
backward-nf8-n8193                     k_lmm_train64 (lmm, 4)          8.2e-07  3.3e-06
backward-ht2-n17                       k_lmm_train (lmm, 1)            1.2e-06  4.7e-06
backward-ht2-n4097                     k_lmm_train (lmm, 1)            2.3e-06  9.3e-06
backward-ht2-n8193                     k_lmm_train64 (lmm, 4)          1.3e-06  5.0e-06
backward-any-n77-lmm                   k_lmm_train (lmm, 1)            3.5e-07  3.0e-06
backward-any-n8193-lmm                 k_lmm_train64 (lmm, 4)          3.6e-07  3.0e-06
backward-any-n77-lmm16                 k_lmm_train (lmm, 1)            2.7e-07  3.0e-06
backward-any-n8193-lmm16               k_lmm_train (lmm, 1)            6.4e-07  3.0e-06
backward-any-n77-lmm64                 k_lmm_train64 (lmm, 4)          3.0e-07  3.0e-06
backward-any-n8193-lmm64               k_lmm_train64 (lmm, 4)          4.7e-07  3.0e-06
backward-any-n77-valu                  k_generic_train (valu, 0)       2.1e-07  3.0e-06
backward-any-n8193-valu                k_generic_train (valu, 0)       7.5e-07  3.0e-06
backward-umask-n77                     k_lmm_train (lmm, 1)            4.2e-07  3.0e-06
backward-umask-n8193                   k_lmm_train64 (lmm, 4)          4.4e-07  3.0e-06
backward-nf2-n200-relu                 k_mfma_train_ts (tilesplit, 1)  2.8e-07  3.0e-06
backward-any-n77-lmm16-relu            k_lmm_train (lmm, 1)            6.6e-07  3.0e-06
backward-nf2-n4097-gather              k_mfma_train_ts (tilesplit, 2)  1.3e-06  5.3e-06
backward-nf4-n17-gather                k_mfma_train_ts (tilesplit, 1)  1.0e-06  4.0e-06
backward-any-n8193-lmm64-gather        k_lmm_train64 (lmm, 4)          5.4e-07  3.0e-06
backward-any-n77-lmm16-gather          k_lmm_train (lmm, 1)            3.0e-07  3.0e-06
backward-any-n77-valu-gather           k_generic_train (valu, 0)       1.9e-07  3.0e-06
backward-nf2-n4097-no_gx               k_mfma_train_ts (tilesplit, 2)  7.0e-07  3.0e-06
backward-any-n8193-lmm64-no_gx         k_lmm_train64 (lmm, 4)          4.7e-07  3.0e-06
backward-any-n77-lmm16-no_gx           k_lmm_train (lmm, 1)            2.7e-07  3.0e-06
zseed-nf2-n200                         k_mfma_train_ts (tilesplit, 1)  7.9e-07  3.2e-06
zseed-nf2-n8193                        k_mfma_train (netsplit, 1)      1.4e-07  3.0e-06
zseed-nf2-n65537                       k_mfma_train (rowpar, 2)        1.1e-07  3.0e-06
zseed-nf2c0-n8193                      k_mfma_train (netsplit, 1)      1.0e-07  3.0e-06
zseed-nf4-n200                         k_mfma_train_ts (tilesplit, 1)  3.8e-07  3.0e-06
zseed-nf4-n8193                        k_mfma_train (netsplit, 1)      1.9e-07  3.0e-06
zseed-nf4-n32769                       k_mfma_train_wide (wide, 2)     1.2e-07  3.0e-06
zseed-nf8-n4097                        k_mfma_train (rowpar, 1)        4.3e-07  3.0e-06
zseed-ht2-n200                         k_mfma_train (netsplit, 1)      7.5e-07  3.0e-06
zseed-nf2-n8193-gather                 k_mfma_train (netsplit, 1)      1.1e-07  3.0e-06
zseed-nf4-n32769-gather                k_mfma_train_wide (wide, 2)     1.4e-07  3.0e-06
zseed-nf2-n4097-gather                 k_mfma_train_ts (tilesplit, 2)  1.1e-07  3.0e-06
zseed-any-n77-lmm16                    k_lmm_train (lmm, 1)            1.2e-07  3.0e-06
zseed-any-n8193-lmm64-gather           k_lmm_train64 (lmm, 4)          9.3e-08  3.0e-06
zseed-any-n77-valu                     k_generic_train (valu, 0)       1.6e-07  3.0e-06
zseed-umask-n200                       k_lmm_train (lmm, 1)            3.2e-07  3.0e-06
backward_cond-any-n1                   k_lmm_train (lmm, 1)            6.2e-07  3.0e-06
backward_cond-any-n17                  k_lmm_train (lmm, 1)            2.2e-07  3.0e-06
backward_cond-any-n300                 k_lmm_train (lmm, 1)            4.6e-07  3.0e-06
backward_cond-nf2-n300                 k_lmm_train (lmm, 1)            1.3e-06  5.4e-06
backward_cond-nf2c0-n17                k_lmm_train (lmm, 1)            3.3e-07  3.0e-06
backward_cond-umask-n300               k_lmm_train (lmm, 1)            5.6e-07  3.0e-06
backward_cond-any-n77-relu             k_lmm_train (lmm, 1)            4.3e-07  3.0e-06
backward_cond-h512-n37                 k_generic_train (valu, 0)       4.9e-07  3.0e-06
inverse_backward-any-n1                k_lmm_train (lmm, 1)            5.0e-07  3.0e-06
inverse_backward-any-n17               k_lmm_train (lmm, 1)            3.7e-07  3.0e-06
inverse_backward-any-n300              k_lmm_train (lmm, 1)            8.2e-07  3.3e-06
inverse_backward-nf2-n300              k_lmm_train (lmm, 1)            1.5e-06  6.1e-06
inverse_backward-nf2c0-n17             k_lmm_train (lmm, 1)            6.5e-07  3.0e-06
inverse_backward-umask-n300            k_lmm_train (lmm, 1)            7.2e-07  3.0e-06
inverse_backward-any-n77-relu          k_lmm_train (lmm, 1)            3.4e-06  1.4e-05
inverse_backward-h512-n37              k_generic_train (valu, 0)       6.5e-07  3.0e-06
backward_cond-any-n300-gather          k_lmm_train (lmm, 1)            6.4e-07  3.0e-06
backward_cond-h512-n37-gather          k_generic_train (valu, 0)       2.9e-07  3.0e-06
backward_cond-any-n300-no_gx-no_gc     k_lmm_train (lmm, 1)            4.6e-07  3.0e-06
backward_cond-any-n300-no_gc           k_lmm_train (lmm, 1)            4.6e-07  3.0e-06
backward_cond-h512-n37-no_gx-no_gc     k_generic_train (valu, 0)       4.9e-07  3.0e-06
inverse_backward-any-n300-no_gx-no_gc  k_lmm_train (lmm, 1)            8.2e-07  3.3e-06
inverse_backward-any-n300-no_gc        k_lmm_train (lmm, 1)            8.2e-07  3.3e-06
"""
import collections
import functools
import zlib

import numpy as np
import pytest
import torch

import seeded_vjp_reference as R

pytestmark = pytest.mark.gpu

L = 3
GEOMS = {
    # name: (d, c, hidden)
    "nf2": (16, 4, (48,)),         # NF = 2, CQ = 1: three hidden tiles, the fewest the tile-split kernel takes
    "nf2c0": (5, 0, (48,)),        # NF = 2, CQ = 0
    "nf4": (24, 6, (48,)),         # NF = 4
    "nf8": (40, 12, (48,)),        # NF = 8: tile-split up to 4096 rows
    "ht2": (16, 4, (32,)),         # two hidden tiles: trains on the register-chained kernels, never tile-split -- a seeded call
                                   # goes to the any-shape kernels at every row count
    "any": (6, 2, (12, 20)),       # two hidden layers: the any-shape kernels, by family
    "umask": (7, 3, (20,)),        # a user mask table
    "h512": (16, 4, (512,)),       # a 16-row tile image beyond the any-shape kernel's LDS budget: the VALU kernel
}

TS1 = ("k_mfma_train_ts", "tilesplit", 1)
TS2 = ("k_mfma_train_ts", "tilesplit", 2)
L16 = ("k_lmm_train", "lmm", 1)
L64 = ("k_lmm_train64", "lmm", 4)
VALU = ("k_generic_train", "valu", 0)


def NS(r):
    return ("k_mfma_train", "netsplit", r)


def ROWPAR(r):
    return ("k_mfma_train", "rowpar", r)


def WIDE(r):
    return ("k_mfma_train_wide", "wide", r)


Case = collections.namedtuple("Case", "entry geom n expect act family masks gather null")


def _case(entry, geom, n, expect, act="tanh", family="auto", masks="alt", gather=False, null=()):
    return Case(entry, geom, n, expect, act, family, masks, gather, tuple(null))


def _id(k):
    s = "%s-%s-n%d" % (k.entry, k.geom, k.n)
    if k.family != "auto":
        s += "-" + k.family
    if k.act != "tanh":
        s += "-" + k.act
    if k.gather:
        s += "-gather"
    for o in k.null:
        s += "-no_" + o
    return s


def _backward_cases():
    out = []
    # the register-chained geometries: one workgroup with a ragged tile; one -> two row tiles per workgroup at 4096 -> 4097
    # (NF = 8: tile-split -> any-shape); tile-split -> any-shape at 8192 -> 8193 (the 64-row form: auto takes it from 8192 rows)
    for geom in ("nf2", "nf2c0", "nf4"):
        for n in (1, 15, 16, 17, 4096):
            out.append(_case("backward", geom, n, TS1))
        for n in (4097, 8192):
            out.append(_case("backward", geom, n, TS2))
        out.append(_case("backward", geom, 8193, L64))
    for n in (1, 15, 16, 17, 4096):
        out.append(_case("backward", "nf8", n, TS1))
    out.append(_case("backward", "nf8", 4097, L16))
    for n in (8192, 8193):
        out.append(_case("backward", "nf8", n, L64))
    for n, exp in ((17, L16), (4097, L16), (8193, L64)):
        out.append(_case("backward", "ht2", n, exp))
    # the any-shape kernels by family ("lmm" is auto: the 64-row form from 8192 rows on; "lmm16" pins the 16-row form)
    for fam, small, big in (("lmm", L16, L64), ("lmm16", L16, L16), ("lmm64", L64, L64), ("valu", VALU, VALU)):
        out.append(_case("backward", "any", 77, small, family=fam))
        out.append(_case("backward", "any", 8193, big, family=fam))
    out.append(_case("backward", "umask", 77, L16, masks="random"))
    out.append(_case("backward", "umask", 8193, L64, masks="random"))
    out.append(_case("backward", "nf2", 200, TS1, act="relu"))
    out.append(_case("backward", "any", 77, L16, act="relu", family="lmm16"))
    # gathered inputs, seeds and outputs in batch order
    out.append(_case("backward", "nf2", 4097, TS2, gather=True))
    out.append(_case("backward", "nf4", 17, TS1, gather=True))
    out.append(_case("backward", "any", 8193, L64, family="lmm64", gather=True))
    out.append(_case("backward", "any", 77, L16, family="lmm16", gather=True))
    out.append(_case("backward", "any", 77, VALU, family="valu", gather=True))
    # gx_out = NULL
    out.append(_case("backward", "nf2", 4097, TS2, null=("gx",)))
    out.append(_case("backward", "any", 8193, L64, family="lmm64", null=("gx",)))
    out.append(_case("backward", "any", 77, L16, family="lmm16", null=("gx",)))
    return out


def _zseed_cases():
    # 200 rows: tile-split.  Then the smallest row count of each row-parallel launch form (launch_train / launch_train_r /
    # pick_rows, rnvp_mfma_train_dev.h): above the tile-split limit a batch of at most 256 workgroups runs net-split; the first
    # batch that pick_rows gives more than 256 workgroups runs the plain form (NF = 2: 65 537 rows at two tiles per wave) or, for
    # NF = 4, the wide form (32 769 rows at two tiles per wave).  NF = 8 has no net-split form (its LDS image of eight waves
    # exceeds a CU's 160 KB): plain from 4097 rows on
    out = [
        _case("zseed", "nf2", 200, TS1),
        _case("zseed", "nf2", 8193, NS(1)),
        _case("zseed", "nf2", 65537, ROWPAR(2)),
        _case("zseed", "nf2c0", 8193, NS(1)),
        _case("zseed", "nf4", 200, TS1),
        _case("zseed", "nf4", 8193, NS(1)),
        _case("zseed", "nf4", 32769, WIDE(2)),
        _case("zseed", "nf8", 4097, ROWPAR(1)),
        _case("zseed", "ht2", 200, NS(1)),
        _case("zseed", "nf2", 8193, NS(1), gather=True),
        _case("zseed", "nf4", 32769, WIDE(2), gather=True),
        _case("zseed", "nf2", 4097, TS2, gather=True),
        _case("zseed", "any", 77, L16, family="lmm16"),
        _case("zseed", "any", 8193, L64, family="lmm64", gather=True),
        _case("zseed", "any", 77, VALU, family="valu"),
        _case("zseed", "umask", 200, L16, masks="random"),
    ]
    return out


def _cond_cases():
    out = []
    for entry in ("backward_cond", "inverse_backward"):
        for n in (1, 17, 300):
            out.append(_case(entry, "any", n, L16))
        out.append(_case(entry, "nf2", 300, L16))
        out.append(_case(entry, "nf2c0", 17, L16))                      # no condition: gc_out ignored
        out.append(_case(entry, "umask", 300, L16, masks="random"))
        out.append(_case(entry, "any", 77, L16, act="relu"))
        out.append(_case(entry, "h512", 37, VALU))
    out.append(_case("backward_cond", "any", 300, L16, gather=True))
    out.append(_case("backward_cond", "h512", 37, VALU, gather=True))
    out.append(_case("backward_cond", "any", 300, L16, null=("gx", "gc")))
    out.append(_case("backward_cond", "any", 300, L16, null=("gc",)))   # gcw = 0: another packing of the first Linear
    out.append(_case("backward_cond", "h512", 37, VALU, null=("gx", "gc")))
    out.append(_case("inverse_backward", "any", 300, L16, null=("gx", "gc")))
    out.append(_case("inverse_backward", "any", 300, L16, null=("gc",)))
    return out


CASES = _backward_cases() + _zseed_cases() + _cond_cases()
assert len({_id(k) for k in CASES}) == len(CASES)


def geom_of(k):
    d, c, hidden = GEOMS[k.geom]
    return (d, c, hidden, k.act)


@functools.lru_cache(maxsize=None)
def _reference(k):
    d, c, hidden = GEOMS[k.geom]
    rng = np.random.default_rng(zlib.crc32(_id(k).encode()))
    n = k.n
    m = 3 * n if k.gather else n
    # (not the unbounded ReLU nets on 16-d rows: three layers of doubled scales overflow exp(s); nor the wide hidden layer)
    tame = max(hidden) >= 64 or (k.act == "relu" and d > 8)
    params = R.init_params(L, d, c, hidden, rng, scale=1.0 if tame else 2.0)
    masks = R.alternating_masks(L, d) if k.masks == "alt" else R.random_masks(L, d, rng)
    X = rng.standard_normal((m, d)).astype(np.float32)
    C = rng.standard_normal((m, c)).astype(np.float32) if c else None
    idx = None
    if k.gather:        # repeats and gaps: n draws out of 3n source rows, the first source row of the batch taken twice
        idx = rng.integers(0, m, size=n).astype(np.int64)
        if n > 1:
            idx[n // 2] = idx[0]
    gz = (rng.standard_normal((n, d)) / n).astype(np.float32)
    gld = (rng.standard_normal(n) / n).astype(np.float32)
    inp = dict(params=params, masks=masks, X=X, C=C, idx=idx, gz=gz, gld=gld, inv_B=1.0 / n)
    g = geom_of(k)
    if k.entry in ("backward", "backward_cond"):
        r64, r32 = (R.forward_vjp(params, masks, g, X, C, idx, gz, gld, dt) for dt in (torch.float64, torch.float32))
        keys = ("grad", "gx") if k.entry == "backward" else ("grad", "gx", "gc")
    elif k.entry == "zseed":
        r64, r32 = (R.zseed_vjp(params, masks, g, X, C, idx, gz, 1.0 / n, dt) for dt in (torch.float64, torch.float32))
        keys = ("grad",)
    else:
        r64, r32 = (R.inverse_vjp(params, masks, g, X, C, gz, dt) for dt in (torch.float64, torch.float32))      # X holds z, gz holds gx
        r64 = dict(r64, gx=r64["gz"]); r32 = dict(r32, gx=r32["gz"])                        # "gx": the gradient of the rows
        keys = ("grad", "gx", "gc")
    return dict(inp=inp, ref=r64, ref32=r32, keys=keys, bars=R.bars(r64, r32, keys))


def reference(k):
    """inputs, float64 / float32 references and the bars of a case (computed once; a nullable variant shares its base's)"""
    return _reference(k._replace(null=(), expect=None))


def _dev(a, dtype=torch.float32):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a)).to(dtype).cuda().contiguous()


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def make_shape(_hip, k, alt=None):
    d, c, hidden = GEOMS[k.geom]
    if alt is None:
        alt = 1 if k.masks == "alt" else 0
    return _hip.RnvpShape.make(L, d, c, hidden, k.act, alt_masks=alt, family=k.family)


def run_entry(_hip, k, inp, masks_table=True):
    """one call of the case's entry point; the workspace has exactly the size the library asks for -> (outputs, dispatch)"""
    d, c, hidden = GEOMS[k.geom]
    n = k.n
    shape = make_shape(_hip, k)
    P = _hip.param_count(shape)
    pd, mk = _dev(inp["params"]), (_dev(inp["masks"], torch.uint8) if masks_table else None)
    xd, cd, idx = _dev(inp["X"]), _dev(inp["C"]), _dev(inp["idx"], torch.int64)
    gz, gld = _dev(inp["gz"]), _dev(inp["gld"])
    grad = _nan(P)
    gx = None if "gx" in k.null else _nan(n, d)
    gc = None if ("gc" in k.null or k.entry in ("backward", "zseed")) else _nan(n, max(c, 1))
    loss = None
    if k.entry in ("backward", "zseed"):
        nb = _hip.workspace_bytes(shape, _hip.OP_TRAIN, n)
    else:
        nb = _hip.backward_cond_workspace_bytes(shape, n)
    assert nb > 0
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    if k.entry == "backward":
        _hip.backward(shape, pd, mk, xd, cd, idx, n, gz, gld, grad, gx, ws)
    elif k.entry == "zseed":
        loss = _nan(1)
        _hip.loss_grad_zseed(shape, pd, mk, xd, cd, idx, n, inp["inv_B"], gz, grad, loss, ws)
        gx = None
    elif k.entry == "backward_cond":
        _hip.backward_cond(shape, pd, mk, xd, cd, idx, n, gz, gld, grad, gx, gc, ws)
    else:
        _hip.inverse_backward(shape, pd, mk, xd, cd, n, gz, grad, gx, gc, ws)
    torch.cuda.synchronize()
    disp = _hip.last_dispatch(_hip.PROFILE_TRAIN)
    out = dict(grad=grad, gx=gx, gc=gc if c else None, loss=loss)
    return {key: (None if v is None else v.cpu().numpy().astype(np.float64)) for key, v in out.items()}, disp


def check_dispatch(k, disp):
    assert (disp["kernel"], disp["variant"], disp["row_tiles"]) == k.expect, (_id(k), disp)


def compare(k, ref, got):
    """every returned array in full against float64, each at its own bar; the figures are printed before anything is asserted"""
    fails = []
    for key in ref["keys"]:
        want = ref["ref"][key]
        if want is None or got[key] is None:
            continue
        e32, bar = ref["bars"][key]
        assert np.isfinite(got[key]).all(), "%s %s: not every element was written" % (_id(k), key)
        err = R.rel_err(got[key], want)
        print("%s %-4s e32 %.2e bar %.2e err %.2e" % (_id(k), key, e32, bar, err))
        if not R.close(got[key], want, bar):
            rows = np.abs(got[key] - want).reshape(len(want), -1).max(axis=1)
            fails.append("%s: %.2e of scale, bar %.2e (e32 %.2e); worst index %d of %d" % (key, err, bar, e32, int(rows.argmax()), len(rows)))
    if k.entry == "zseed":
        print("%s loss got %.9g want %.9g" % (_id(k), float(got["loss"][0]), ref["ref"]["loss"]))
        if not R.loss_close(got["loss"][0], ref["ref"]["loss"]):
            fails.append("loss_out %.9g, want %.9g" % (float(got["loss"][0]), ref["ref"]["loss"]))
    assert not fails, "%s on %s: %s" % (_id(k), k.expect[0], "; ".join(fails))


@pytest.mark.parametrize("k", CASES, ids=[_id(k) for k in CASES])
def test_seeded_entry_point_vs_float64_vjp(k):
    from probaforms_amd import _hip
    ref = reference(k)
    got, disp = run_entry(_hip, k, ref["inp"])
    check_dispatch(k, disp)
    for o in k.null:
        assert got[o] is None
    compare(k, ref, got)


# ---- the mask table across the hand-over from the tile-split kernel to the any-shape kernels -----------------------------------
def test_backward_on_a_declared_pattern_needs_the_mask_table_past_the_tile_split_limit():
    """rnvp_hip.h, rnvp_backward: a declared alternating pattern (alt_masks = 1) is served without the table while the
    tile-split kernel takes the call (8192 rows for d <= 32); one row more runs on the any-shape kernels, which read it --
    without it the call is RNVP_EINVAL and nothing is launched"""
    from probaforms_amd import _hip
    small = _case("backward", "nf2", 16, TS1)
    ref = reference(small)
    got, disp = run_entry(_hip, small, ref["inp"], masks_table=False)
    check_dispatch(small, disp)
    compare(small, ref, got)
    k = _case("backward", "nf2", 8192, TS2)
    ref = reference(k)
    got, disp = run_entry(_hip, k, ref["inp"], masks_table=False)
    check_dispatch(k, disp)
    compare(k, ref, got)
    got, disp = run_entry(_hip, small, reference(small)["inp"], masks_table=False)
    assert disp["rows"] == 16
    k = _case("backward", "nf2", 8193, L64)
    with pytest.raises(RuntimeError, match=r"invalid argument.*status -1"):
        run_entry(_hip, k, reference(k)["inp"], masks_table=False)
    after = _hip.last_dispatch(_hip.PROFILE_TRAIN)
    assert (after["kernel"], after["rows"]) == ("k_mfma_train_ts", 16), after            # no launch was noted


def test_class_api_gradient_of_x_alone_at_8193_rows(monkeypatch):
    """the class API always hands its mask table over: log_prob with only X requiring a gradient takes rnvp_backward (not
    rnvp_backward_cond), at 8193 rows on the any-shape kernels, and agrees with the reference"""
    from probaforms_amd import _hip
    from probaforms_amd.models import NormalizingFlow, RealNVPLayer, StandardNormalPrior
    k = _case("backward", "nf2", 8193, L64)
    ref = reference(k)
    inp = ref["inp"]
    d, c, hidden = GEOMS[k.geom]
    layers = [RealNVPLayer(d, c, torch.from_numpy(inp["masks"][l].astype(np.int64)), hidden, k.act) for l in range(L)]
    nf = NormalizingFlow(layers, StandardNormalPrior(d, "cuda"))
    with torch.no_grad():
        off = 0
        for p in nf.parameters():
            p.copy_(torch.from_numpy(inp["params"][off:off + p.numel()]).view_as(p)); off += p.numel()
        assert off == inp["params"].size
    nf.engine()
    w = inp["gld"]                                  # per-row weights of the log-prob: loss = sum_r w[r] * log_prob[r]
    X = _dev(inp["X"]).requires_grad_(True)
    C = _dev(inp["C"])
    # rnvp_last_dispatch is per thread and autograd runs the node's backward on its own device thread: read it there, right
    # behind the library call
    seen = []
    real = _hip.backward

    def spy(*args):
        real(*args)
        seen.append(_hip.last_dispatch(_hip.PROFILE_TRAIN))

    monkeypatch.setattr(_hip, "backward", spy)
    monkeypatch.setattr(_hip, "backward_cond", None)            # not this one: C requires no gradient
    lp = nf.log_prob_samples(X, C)
    assert lp.grad_fn is not None and not C.requires_grad
    (_dev(w) * lp).sum().backward()
    torch.cuda.synchronize()
    assert len(seen) == 1
    check_dispatch(k, seen[0])
    assert seen[0]["rows"] == k.n
    # d / dz of w * N(0, I).log_prob(z) is -w z: the same vector-Jacobian product, seeded with the reference's own z
    g = geom_of(k)
    gz = -w[:, None].astype(np.float64) * ref["ref"]["z"]
    r64, r32 = (R.forward_vjp(inp["params"], inp["masks"], g, inp["X"], inp["C"], None, gz, w, dt) for dt in (torch.float64, torch.float32))
    keys = ("grad", "gx")
    want = dict(ref=r64, keys=keys, bars=R.bars(r64, r32, keys))
    got = dict(grad=torch.cat([p.grad.reshape(-1) for p in nf.parameters()]).cpu().numpy().astype(np.float64),
               gx=X.grad.cpu().numpy().astype(np.float64))
    compare(k, want, got)
