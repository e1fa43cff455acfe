"""The yardstick of sample_joint_scores / pfp_joint_scores: the energy score and the variogram score of K draws in R^d against
a target, straight from their definitions in numpy float64 -- the explicit K x K pair sum and the full d x d variogram sum,
diagonals included.  Plain numpy, written independently of the package; no GPU.

Per row, with draws x_1 .. x_K (float32, widened) and target y:
    T1        = 1/K sum_k |x_k - y|_2
    spread    = 1/(2 K D) sum_k sum_l |x_k - x_l|_2,   D = K - 1 if fair else K
    energy    = T1 - spread
    m_ij      = 1/K sum_k |x_ki - x_kj|^p              (|.|^p as sqrt, identity or square)
    variogram = sum_i sum_j (|y_i - y_j|^p - m_ij)^2
    V         = sum_i sum_j (|y_i - y_j|^p + m_ij)^2   (the scale of the variogram's rounding errors)
A NaN among the row's draws or in its y: energy, spread and variogram are NaN.  Everything else, infinities included, is
whatever the formulas give in float64 (an infinite draw meets itself on both diagonals: inf - inf).

Tolerances (derived, not measured; u = 2^-53): worst-case sequential float64 summation plus the one rounding to float32,
    energy, spread :  ulp32(ref) + (K^2 / 2 + d + 8) u (T1 + spread)
    variogram      :  ulp32(ref) + (K + d^2 + 16) u 4 V

The second half of the file holds the rows the host and the GPU tests feed the code under test."""
import collections

import numpy as np

Joint = collections.namedtuple("Joint", "t1 spread energy variogram v")       # float64 [n], not yet rounded
PAIR_BLOCK = 1024                                                             # rows of a K x K distance matrix held at once
ELEMS = 1 << 22                                                               # elements of a temporary held at once
U = 2.0 ** -53
POWER = {0.5: np.sqrt, 1.0: lambda a: a, 2.0: np.square}


def _pair_sums(x):
    """sum_k sum_l |x_k - x_l|_2 of every row of x [n, d, K], from the full distance matrices, PAIR_BLOCK rows at a time"""
    n, d, K = x.shape
    total = np.zeros(n)
    per = max(1, ELEMS // (K * min(K, PAIR_BLOCK)))                  # rows of x per step
    for r0 in range(0, n, per):
        xs = x[r0:r0 + per]
        for lo in range(0, K, PAIR_BLOCK):
            sq = np.zeros((xs.shape[0], min(PAIR_BLOCK, K - lo), K))
            for j in range(d):
                sq += np.square(xs[:, j, lo:lo + PAIR_BLOCK, None] - xs[:, j, None, :])
            total[r0:r0 + per] += np.sqrt(sq).sum(axis=(1, 2))
    return total


def _variogram(x, y, order):
    """(variogram, V) of every row: the d x d sums over the full index square"""
    n, d, K = x.shape
    pw = POWER[order]
    vg, vv = np.zeros(n), np.zeros(n)
    per = max(1, ELEMS // (d * d * K))
    for r0 in range(0, n, per):
        xs, ys = x[r0:r0 + per], y[r0:r0 + per]
        m = pw(np.abs(xs[:, :, None, :] - xs[:, None, :, :])).sum(axis=3) / np.float64(K)
        t = pw(np.abs(ys[:, :, None] - ys[:, None, :]))
        vg[r0:r0 + per] = np.square(t - m).sum(axis=(1, 2))
        vv[r0:r0 + per] = np.square(t + m).sum(axis=(1, 2))
    return vg, vv


def scores_grid(xt, y, fairs=(False, True), orders=(0.5, 1.0, 2.0)):
    """xt [n, d, K] float32, y [n, d] -> {(fair, order): Joint of float64 [n] arrays}; order None: variogram and v are None.
    The pair sum is formed once, the variogram once per order."""
    xt, y = np.asarray(xt, np.float32), np.asarray(y, np.float32)
    n, d, K = xt.shape
    assert y.shape == (n, d)
    x64, y64 = xt.astype(np.float64), y.astype(np.float64)
    bad = np.isnan(x64).any(axis=(1, 2)) | np.isnan(y64).any(axis=1)
    nanned = lambda a: None if a is None else np.where(bad, np.nan, a)
    out = {}
    with np.errstate(all="ignore"):
        t1 = np.sqrt(np.square(x64 - y64[:, :, None]).sum(axis=1)).sum(axis=1) / np.float64(K)
        pairs = _pair_sums(x64)
        for order in orders:
            vg, vv = _variogram(x64, y64, order) if order is not None else (None, None)
            for fair in fairs:
                spread = pairs / np.float64(2.0 * K * (K - 1 if fair else K))
                out[(bool(fair), order)] = Joint(t1, nanned(spread), nanned(t1 - spread), nanned(vg), vv)
    return out


def scores(xt, y, fair=False, order=0.5):
    """xt [n, d, K] float32, y [n, d] -> Joint of float64 [n] arrays; order None: variogram and v are None"""
    return scores_grid(xt, y, (fair,), (order,))[(bool(fair), order)]


def scores_of_stacked(X, Y, fair=False, order=0.5):
    """the same over stacked draws X [K, n, d], as sample_many returns them"""
    return scores(np.ascontiguousarray(np.transpose(np.asarray(X, np.float32), (1, 2, 0))), Y, fair, order)


def _ulp32(ref):
    with np.errstate(all="ignore"):
        fin = np.where(np.isfinite(ref), np.abs(ref), 0.0)
        return np.spacing(fin.astype(np.float32)).astype(np.float64)


def _finite(a):
    return np.where(np.isfinite(a), a, 0.0)


def bound_pairs(ref, j, K, d):
    """the bound of energy and spread: ulp32(ref) + (K^2 / 2 + d + 8) u (T1 + spread)"""
    return _ulp32(ref) + (K * K / 2.0 + d + 8.0) * U * (_finite(j.t1) + _finite(np.abs(j.spread)))


def bound_variogram(ref, j, K, d):
    """the bound of variogram: ulp32(ref) + (K + d^2 + 16) u 4 V"""
    return _ulp32(ref) + (K + d * d + 16.0) * U * 4.0 * _finite(j.v)


def check_close(got, ref, tol, what, times=1.0):
    """NaN in the same places, infinities equal, and elsewhere |got - ref| <= times * tol"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), (what, "NaN positions", got, ref)
    inf = np.isinf(got) | np.isinf(ref)
    assert np.array_equal(got[inf], ref[inf]), (what, "infinities", got, ref)
    fin = np.isfinite(ref)
    with np.errstate(all="ignore"):
        err = np.abs(got - ref)[fin]
    t = times * np.broadcast_to(tol, ref.shape)[fin]
    print(what, "max err / bound", float((err / t).max()) if err.size else 0.0)
    assert (err <= t).all(), (what, float((err / t).max()), float(err.max()))


def check_all(got, ref, K, d, what, times=1.0):
    """got: energy, spread, variogram (float32 [n]; variogram None iff ref has none) against Joint `ref`"""
    for a in got:
        assert a is None or (a.dtype == np.float32 and a.shape == ref.t1.shape), what
    check_close(got[0], ref.energy, bound_pairs(ref.energy, ref, K, d), (what, "energy"), times)
    check_close(got[1], ref.spread, bound_pairs(ref.spread, ref, K, d), (what, "spread"), times)
    if ref.variogram is None:
        assert got[2] is None, what
    else:
        check_close(got[2], ref.variogram, bound_variogram(ref.variogram, ref, K, d), (what, "variogram"), times)


# ---------------------------------------------------------------------------------------------------------------------------
# the rows the tests feed
# ---------------------------------------------------------------------------------------------------------------------------
FINITE_ROWS = 5


def finite(K, d, seed=0):
    """(xt [5, d, K], y [5, d]) float32.  Row 0: a tied pair of draws; row 1: y equal to a draw; row 2: draws that differ in
    their last bits only, around 3; row 3: unit spread around 1e6 (cancellation); row 4: y far from every draw."""
    rng = np.random.default_rng(1000 * K + d + seed)
    xt = (rng.standard_normal((FINITE_ROWS, d, K)) * 3 + 1).astype(np.float32)
    y = (rng.standard_normal((FINITE_ROWS, d)) * 3 + 1).astype(np.float32)
    if K > 1:
        xt[0, :, K - 1] = xt[0, :, 0]
    y[1] = xt[1, :, K // 2]
    xt[2] = np.float32(3.0) + (rng.integers(0, 8, (d, K)) * np.spacing(np.float32(3.0))).astype(np.float32)
    y[2] = np.float32(3.0)
    xt[3] = (1e6 + rng.standard_normal((d, K))).astype(np.float32)
    y[3] = np.float32(1e6 + 0.25)
    y[4] = np.float32(1e3)
    return xt, y


NONFINITE_KINDS = ("+nan", "-nan", "y nan", "nan and inf", "+inf", "-inf", "both inf", "inf and y inf", "y +inf", "y -inf", "clean")


def nonfinite(K, d=3, seed=0):
    """(xt [11, d, K], y [11, d]) float32: one row per NONFINITE_KINDS, the special values in draw K // 2 (and draw 0), column
    d - 1 of the draws and column 0 of y; the last row is clean"""
    rng = np.random.default_rng(77 * K + d + seed)
    n = len(NONFINITE_KINDS)
    xt = (rng.standard_normal((n, d, K)) * 3 + 1).astype(np.float32)
    y = (rng.standard_normal((n, d)) * 3 + 1).astype(np.float32)
    kind = {k: i for i, k in enumerate(NONFINITE_KINDS)}
    neg_nan = np.array([0xFFC00001], np.uint32).view(np.float32)[0]
    k, j = K // 2, d - 1
    xt[kind["+nan"], j, k] = np.nan
    xt[kind["-nan"], j, k] = neg_nan
    y[kind["y nan"], 0] = np.nan
    xt[kind["nan and inf"], j, k] = np.nan
    xt[kind["nan and inf"], 0, 0] = np.inf
    xt[kind["+inf"], j, k] = np.inf
    xt[kind["-inf"], j, k] = -np.inf
    xt[kind["both inf"], j, k] = np.inf
    xt[kind["both inf"], 0, 0] = -np.inf
    xt[kind["inf and y inf"], j, k] = np.inf
    y[kind["inf and y inf"], j] = np.inf
    y[kind["y +inf"], 0] = np.inf
    y[kind["y -inf"], 0] = -np.inf
    return xt, y


def table(K, fair, energy, spread, variogram):
    """the non-finite rules, spelled out for the rows of nonfinite(K)"""
    kind = {k: i for i, k in enumerate(NONFINITE_KINDS)}
    undefined = K == 1 and fair
    for k in ("+nan", "-nan", "y nan", "nan and inf"):
        r = kind[k]
        assert np.isnan(energy[r]) and np.isnan(spread[r]) and (variogram is None or np.isnan(variogram[r])), k
    for k in ("+inf", "-inf", "both inf", "inf and y inf"):
        r = kind[k]
        assert np.isnan(energy[r]) and np.isnan(spread[r]) and (variogram is None or np.isnan(variogram[r])), k
    for k in ("y +inf", "y -inf"):
        r = kind[k]
        if undefined:
            assert np.isnan(energy[r]) and np.isnan(spread[r]), k
        else:
            assert energy[r] == np.inf and np.isfinite(spread[r]), k
        assert variogram is None or np.isnan(variogram[r]), k                          # |y_i - y_i| on the diagonal: inf - inf
    r = kind["clean"]
    if not undefined:
        assert np.isfinite(energy[r]) and np.isfinite(spread[r]) and spread[r] >= 0
    assert variogram is None or (np.isfinite(variogram[r]) and variogram[r] >= 0)


def comonotone(K, seed=0):
    """d = 2: (xt, y) with x_k = (t_k, t_k) and y on the diagonal, and the same with the second column's draws permuted: the
    same marginals, another dependence"""
    rng = np.random.default_rng(5 + K + seed)
    t = (rng.standard_normal(K) * 2).astype(np.float32)
    xt = np.stack([t, t])[None].copy()
    y = np.full((1, 2), np.float32(0.5))
    sh = xt.copy()
    sh[0, 1] = t[rng.permutation(K)]
    return xt, sh, y
