"""The yardstick of sample_scores / pfp_scores: CRPS, PIT, quantiles and pinball losses of K draws against a target, straight
from their definitions in numpy float64 -- the CRPS by the explicit O(K^2) pair sum, not by the sorted-series identity the
package uses.  Plain numpy, written independently of the package; no GPU.

Per series x_1 .. x_K (float32) and target y:
    crps       = 1/K sum_k |x_k - y| - 1/(2 K D) sum_k sum_l |x_k - x_l|,   D = K - 1 if fair else K
    pit        = (#{x_k < y} + 0.5 #{x_k == y}) / K
    quantiles  = numpy.quantile (method 'linear') of the float64 copies
    pinball    = (y - Q) (p - [y < Q])
A NaN in the series or in y: crps, pit and every pinball are NaN (quantiles only for a NaN in the series).  Everything else,
infinities included, is whatever the formulas give in float64."""
import collections

import numpy as np

Scores = collections.namedtuple("Scores", "crps pit quantiles pinball")       # float64, not yet rounded
PAIR_BLOCK = 1024                                                             # rows of a K x K difference matrix held at once
PAIR_ELEMS = 1 << 23                                                          # elements of difference matrices held at once


def _pair_sums(x):
    """sum_k sum_l |x_k - x_l| of every series of x [S, K], from the full difference matrices, PAIR_BLOCK rows at a time"""
    S, K = x.shape
    total = np.zeros(S)
    per = max(1, PAIR_ELEMS // (K * min(K, PAIR_BLOCK)))             # series per step
    for s0 in range(0, S, per):
        xs = x[s0:s0 + per]
        for lo in range(0, K, PAIR_BLOCK):
            total[s0:s0 + per] += np.abs(xs[:, lo:lo + PAIR_BLOCK, None] - xs[:, None, :]).sum(axis=(1, 2))
    return total


def scores(xt, y, probs=(), fair=False):
    """xt [n, d, K] float32, y [n, d] -> Scores of float64 arrays: crps, pit [n, d]; quantiles, pinball [Q, n, d]"""
    xt, y = np.asarray(xt, np.float32), np.asarray(y, np.float32)
    n, d, K = xt.shape
    assert y.shape == (n, d)
    x32, y32 = xt.reshape(n * d, K), y.reshape(n * d, 1)
    x64, y64 = x32.astype(np.float64), y32.astype(np.float64)
    p = np.asarray(probs, np.float64).reshape(-1, 1)
    with np.errstate(all="ignore"):
        crps = np.abs(x64 - y64).sum(axis=1) / K - _pair_sums(x64) / np.float64(2.0 * K * (K - 1 if fair else K))
        pit = ((x32 < y32).sum(axis=1) + 0.5 * (x32 == y32).sum(axis=1)) / np.float64(K)
        q = np.quantile(x64, p[:, 0], axis=1) if len(p) else np.zeros((0, n * d))
        pin = (y64[:, 0] - q) * (p - (y64[:, 0] < q))
    bad = np.isnan(x64).any(axis=1) | np.isnan(y64[:, 0])
    crps, pit, pin = np.where(bad, np.nan, crps), np.where(bad, np.nan, pit), np.where(bad, np.nan, pin)
    return Scores(crps.reshape(n, d), pit.reshape(n, d), q.reshape(len(p), n, d), pin.reshape(len(p), n, d))


def scores_of_stacked(X, Y, probs=(), fair=False):
    """the same over stacked draws X [K, n, d], as sample_many returns them"""
    return scores(np.ascontiguousarray(np.moveaxis(np.asarray(X, np.float32), 0, -1)), Y, probs, fair)


def scale_of(xt, y):
    """max(|x|, |y|) per series over its finite values, [n, d]"""
    a = np.abs(np.concatenate([np.asarray(xt, np.float64), np.asarray(y, np.float64)[..., None]], axis=-1))
    return np.where(np.isfinite(a), a, 0.0).max(axis=-1)


def bound(ref, K, scale):
    """ulp32(ref) + 2 K 2^-53 max(|x|, |y|): the float64 rounding of at most K-term sums of terms bounded by max |x|, plus the
    one final rounding to float32"""
    with np.errstate(all="ignore"):
        fin = np.where(np.isfinite(ref), np.abs(ref), 0.0)
        return np.spacing(fin.astype(np.float32)).astype(np.float64) + 2.0 * K * 2.0 ** -53 * scale


def check_close(got, ref, K, scale, what):
    """NaN in the same places, infinities equal, and elsewhere |got - ref| <= bound(ref)"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), (what, "NaN positions", got, ref)
    inf = np.isinf(got) | np.isinf(ref)
    assert np.array_equal(got[inf], ref[inf]), (what, "infinities", got, ref)
    fin = np.isfinite(ref)
    with np.errstate(all="ignore"):
        err = np.abs(got - ref)[fin]
    tol = np.broadcast_to(bound(ref, K, scale), ref.shape)[fin]
    assert (err <= tol).all(), (what, float((err / tol).max()), float(err.max()))


def check_exact(got, ref, what):
    """equal as float32 values, NaN in the same places"""
    got, ref = np.asarray(got, np.float32), np.asarray(ref, np.float64).astype(np.float32)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.array_equal(got, ref, equal_nan=True), (what, got, ref)


def check_all(got, ref, K, scale, what, quantiles_exact=False):
    """got: crps, pit, quantiles, pinball (float32; quantiles / pinball may be None when ref has none) against Scores `ref`"""
    check_close(got[0], ref.crps, K, scale, (what, "crps"))
    check_exact(got[1], ref.pit, (what, "pit"))
    if ref.quantiles.shape[0]:
        if quantiles_exact:
            check_exact(got[2], ref.quantiles, (what, "quantiles"))
        else:
            check_close(got[2], ref.quantiles, K, scale, (what, "quantiles"))
        check_close(got[3], ref.pinball, K, scale, (what, "pinball"))
    else:
        assert got[2] is None and got[3] is None, what
