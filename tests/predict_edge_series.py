"""Series and comparison rules shared by tests/test_predict_edges_gpu.py (the kernels) and tests/test_predict_host.py (numpy
stand-ins that show the rules can fail).  Plain numpy; no GPU."""
import numpy as np
from test_predict_gpu import _close                                  # 2 float32 ulps of the float64 value

POS_NAN = np.array([0x7fc00000], np.uint32).view(np.float32)[0]
NEG_NAN = np.array([0xffc00000], np.uint32).view(np.float32)[0]

CONDITIONED_K = (1, 2, 15, 16, 17, 19, 40, 65, 1000)
CONDITIONED_KINDS = ("4096 + N(0, 2^-10)", "-3e5 + N(0, 0.01)", "1e6 first", "1e6 last", "1 and 1 + 2^-23")
NONFINITE_KINDS = ("all nan", "nan first", "nan middle", "nan last", "nan at 17", "+inf first", "-inf first", "+inf middle",
                   "both inf", "-0 among +0")
QUANTILE_K = (3, 4, 5, 17, 4097, 8191)
QUANTILE_KINDS = ("gaussian", "+nan", "-nan", "-inf", "+inf", "all +inf")


def windows_of(K):
    """the draws as one call, and as the two windows (0, 8), (8, K) where K > 8"""
    return [[(0, K)]] + ([[(0, 8), (8, K)]] if K > 8 else [])


def conditioned(K, n=3, seed=0):
    """[K, n, 5] float32, one kind per column: data on which a wrong shift or a lost lane shows in the moments"""
    rng = np.random.default_rng([seed, K])
    g = lambda: rng.standard_normal((K, n))
    x = np.empty((K, n, 5), np.float64)
    x[:, :, 0] = 4096.0 + g() * 2.0 ** -10
    x[:, :, 1] = -3e5 + g() * 0.01
    x[:, :, 2] = g() * 1e-3
    x[0, :, 2] = 1e6
    x[:, :, 3] = g() * 1e-3
    x[K - 1, :, 3] = 1e6
    x[:, :, 4] = np.where(np.arange(K) % 2 == 0, 1.0, 1.0 + 2.0 ** -23)[:, None]
    return x.astype(np.float32)


def nonfinite(K, n=3, seed=1):
    """[K, n, 11] float32 (K >= 19): the ten NONFINITE_KINDS and, in the last column, one clean series"""
    rng = np.random.default_rng([seed, K])
    x = (rng.standard_normal((K, n, 11)) * 2 + 1).astype(np.float32)
    x[:, :, 0] = np.nan
    x[0, :, 1] = np.nan
    x[K // 2, :, 2] = np.nan
    x[K - 1, :, 3] = np.nan
    x[17, :, 4] = np.nan                                             # second 16-draw tile
    x[0, :, 5] = np.inf
    x[0, :, 6] = -np.inf
    x[K // 2, :, 7] = np.inf
    x[3, :, 8] = np.inf
    x[K - 2, :, 8] = -np.inf
    x[:, :, 9] = 0.0
    x[1::3, :, 9] = -0.0
    return x


def clean_like(x, seed=2):
    """the same array with its ten poisoned columns replaced by finite data; the clean column is kept"""
    y = (np.random.default_rng(seed).standard_normal(x.shape) * 2 + 1).astype(np.float32)
    y[:, :, 10] = x[:, :, 10]
    return y


def quantile_series(K, seed=3):
    """xt [3, 2, K] float32, one of QUANTILE_KINDS per (row, column), and the probabilities: exact integer positions and both
    branches of the lerp"""
    rng = np.random.default_rng([seed, K])
    xt = (rng.standard_normal((6, K)) * 3 + 1).astype(np.float32)
    xt[1, K // 2] = POS_NAN
    xt[2, K // 3] = NEG_NAN
    xt[3, 1] = -np.inf
    xt[4, K - 1] = np.inf
    xt[5, :] = np.inf
    assert xt[1].view(np.uint32)[K // 2] == 0x7fc00000 and xt[2].view(np.uint32)[K // 3] == 0xffc00000
    probs = [0.0, 1.0 / (K - 1), 0.25, 1.0 / 3.0, 0.5, 1.0 - 1e-12, 1.0]
    return xt.reshape(3, 2, K), probs


def moments_reference(x, ddof):
    """numpy over the stacked draws x [K, ...] in float64: mean, std, min, max"""
    x64 = np.asarray(x, np.float64)
    with np.errstate(all="ignore"):
        return x64.mean(0), x64.std(0, ddof=ddof), x64.min(0), x64.max(0)


def quantile_reference(xt, probs):
    with np.errstate(all="ignore"):
        return np.quantile(np.asarray(xt, np.float64), probs, axis=-1)


def same(got, want, what, exact=False):
    """NaN in the same places, infinities exactly, and elsewhere within 2 float32 ulps of the float64 value (exact: equal)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (what, "NaN positions", got, want)
    inf = np.isinf(want) | np.isinf(got)
    assert np.array_equal(got[inf], want[inf]), (what, "infinities", got, want)
    fin = np.isfinite(want)
    if exact:
        assert np.array_equal(got[fin], want[fin]), (what, got, want)
    elif fin.any():
        _close(got[fin], want[fin], what)


def check_moments(got, x, ddof, what):
    """got = (mean, std, min, max) against numpy over x [K, ...]"""
    mean, std, mn, mx = moments_reference(x, ddof)
    same(got[0], mean, (what, "mean"))
    same(got[1], std, (what, "std"))
    same(got[2], mn, (what, "min"), exact=True)
    same(got[3], mx, (what, "max"), exact=True)
