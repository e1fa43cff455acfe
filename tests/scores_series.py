"""Series and targets shared by tests/test_scores_host.py (scores_of_draws) and tests/test_scores_gpu.py (pfp_scores).  Plain
numpy; no GPU."""
import numpy as np

POS_NAN = np.array([0x7fc00000], np.uint32).view(np.float32)[0]
NEG_NAN = np.array([0xffc00000], np.uint32).view(np.float32)[0]

FINITE_KINDS = ("gaussian, y inside", "1e6 + N(0, 1), y inside", "constant / half tied, y a draw", "small integers, y an integer",
                "N(0, 1e-3), y far outside")
NONFINITE_KINDS = ("clean", "+nan", "-nan", "nan and inf", "y nan", "+inf", "-inf", "both inf", "y +inf", "y -inf",
                   "+inf and y +inf", "-0 among +0, y +0", "-0 among +0, y -0", "all +inf")


def finite(K, d, seed=0):
    """xt [5, d, K], y [5, d] float32, one of FINITE_KINDS per row: well and badly conditioned series, ties among the draws,
    y equal to a draw, y inside and outside the series' range"""
    rng = np.random.default_rng([seed, K, d])
    xt = np.empty((5, d, K), np.float64)
    y = np.empty((5, d), np.float64)
    xt[0] = rng.standard_normal((d, K)) * 3 + 1
    y[0] = rng.standard_normal(d) * 3 + 1
    xt[1] = 1e6 + rng.standard_normal((d, K))
    y[1] = 1e6 + rng.standard_normal(d)
    xt[2] = rng.standard_normal((d, K)) * 2
    xt[2, 0, :] = 0.7                                                # a constant series: ties everywhere, y tied with all
    if d > 1:
        xt[2, 1, : K // 2] = xt[2, 1, 0]                             # half of a series tied, y in the tie
    y[2] = xt[2, :, 0]
    xt[3] = rng.integers(-3, 4, size=(d, K))
    y[3] = rng.integers(-3, 4, size=d)
    xt[4] = rng.standard_normal((d, K)) * 1e-3
    y[4] = np.where(np.arange(d) % 2 == 0, 10.0, -10.0)
    return xt.astype(np.float32), y.astype(np.float32)


def nonfinite(K, seed=1):
    """xt [14, 2, K], y [14, 2] float32: column 0 holds one of NONFINITE_KINDS per row, column 1 is clean throughout.
    Positions are taken modulo K, so that K = 1, 2, 3 still give valid (if degenerate) series."""
    rng = np.random.default_rng([seed, K])
    R = len(NONFINITE_KINDS)
    xt = (rng.standard_normal((R, 2, K)) * 2 + 1).astype(np.float32)
    y = (rng.standard_normal((R, 2)) * 2 + 1).astype(np.float32)
    at = lambda i: i % K
    xt[1, 0, at(K // 2)] = POS_NAN
    xt[2, 0, at(K // 3)] = NEG_NAN
    xt[3, 0, at(0)] = np.inf
    xt[3, 0, at(K - 1)] = POS_NAN
    y[4, 0] = np.nan
    xt[5, 0, at(1)] = np.inf
    xt[6, 0, at(K - 1)] = -np.inf
    xt[7, 0, at(2)] = np.inf
    xt[7, 0, at(K - 2)] = -np.inf
    y[8, 0] = np.inf
    y[9, 0] = -np.inf
    xt[10, 0, at(0)] = np.inf
    y[10, 0] = np.inf
    xt[11, 0, :] = 0.0
    xt[11, 0, 1::3] = -0.0
    y[11, 0] = 0.0
    xt[12, 0, :] = 0.0
    xt[12, 0, 1::3] = -0.0
    y[12, 0] = -0.0
    xt[13, 0, :] = np.inf
    return xt, y
