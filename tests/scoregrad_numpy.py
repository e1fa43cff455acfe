"""Float64 numpy restatement of pfm_score_grad (probaforms_amd/metrics/csrc/pf_scoregrad.hip): per row the energy score of K draws
against the row's target and its derivatives, written from the formulas and independent of the package; no GPU.

Per row i, with draws x_k = X[k, i, :], target y = Y[i, :] and D = K - 1 if fair else K:
    T1          = (1/K) sum_k |x_k - y|_2
    spread      = 1/(2 K D) sum_k sum_l |x_k - x_l|_2
    score       = T1 - spread
    d score/d x_k = (1/K) c_k (x_k - y) - (1/(K D)) sum_l c_kl (x_k - x_l)
    d score/d y   = -(1/K) sum_k c_k (x_k - y)
c = 1 / distance, and exactly 0 where the squared distance is exactly 0 (the subgradient).  Every difference is taken on the values
themselves.  NaN and infinity are whatever the formulas give: they stay inside their row.

value_grad returns, beside scores, spread, grad_x and grad_y, per output the sum of the magnitudes of its terms (all terms of T1
and of the spread are >= 0): smag = T1 + spread for the score, the spread itself for the spread, mx and my for the gradients.  A
float64 sum of N correctly rounded terms, taken in any order, is within N 2^-53 of those sums.

The second half holds the rows the host and the GPU tests feed the code under test."""
import numpy as np

import joint_scores_numpy as js


def value_grad(X, Y, fair):
    """X [K, n, d], Y [n, d] (any float dtype, widened) -> dict of float64 arrays"""
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    K, n, d = X.shape
    assert Y.shape == (n, d) and (K > 1 or not fair)
    D = K - 1 if fair else K
    with np.errstate(all="ignore"):
        dy = X - Y[None]                                              # [K, n, d]
        dist_y = np.sqrt(np.square(dy).sum(axis=2))                   # [K, n]
        cy = np.where(dist_y == 0.0, 0.0, 1.0 / dist_y)
        ey = cy[:, :, None] * dy
        t1 = dist_y.sum(axis=0) / K
        pair = np.zeros(n)
        A, Am = np.zeros((K, n, d)), np.zeros((K, n, d))
        for k in range(K):
            df = X[k][None] - X                                       # [K, n, d]: x_k - x_l
            dist = np.sqrt(np.square(df).sum(axis=2))
            c = np.where(dist == 0.0, 0.0, 1.0 / dist)
            term = c[:, :, None] * df
            A[k], Am[k] = term.sum(axis=0), np.abs(term).sum(axis=0)
            pair += dist.sum(axis=0)
        spread = pair / (2.0 * K * D)
        out = {"scores": t1 - spread, "spread": spread, "t1": t1, "smag": t1 + np.abs(spread),
               "grad_x": ey / K - A / (K * D), "mx": np.abs(ey) / K + Am / (K * D),
               "grad_y": -ey.sum(axis=0) / K, "my": np.abs(ey).sum(axis=0) / K}
    return out


def score_of(X, Y, fair):
    """the mean score alone, for central differences"""
    return float(value_grad(X, Y, fair)["scores"].mean())


# ---------------------------------------------------------------------------------------------------------------------------
# the rows the tests feed
# ---------------------------------------------------------------------------------------------------------------------------

# (K, n, d) where the kernel's shape axes cross: every k_score instantiation and plan branch that one axis at a time leaves out
# (tests/loss_plans.py names them; tests/test_loss_plans_host.py proves the list reaches them).  Each is the smallest shape of its path
CROSSED = [
    (300, 3, 16),      # U = 2, 16 features in registers
    (300, 3, 17),      # U = 2, chunked
    (512, 3, 32),      # U = 2, chunked, 151 816 bytes of LDS
    (600, 3, 1),       # U = 4 with a masked draw slot, one feature
    (1024, 3, 1),      # U = 4 with all four slots live, one feature
    (600, 3, 17),      # U = 4 masked, chunked
    (770, 3, 21),      # U = 4 full, chunked, 152 112 bytes of LDS
    (1, 3, 16384),     # the target read from global memory, even pitch, chunked
    (2, 3, 8192),
    (4, 3, 4096),
    (5, 3, 3276),      # the neighbour whose target is staged again: G = 1, seven eighths of the lanes idle
    (64, 9, 100),      # G 4 -> 2 for the LDS; n odd: the last workgroup has one row
    (16, 40, 100),     # G 16 -> 8
    (128, 3, 128),     # G 2 -> 1
    (33, 2051, 17),    # several passes per workgroup, chunked
]
CROSSED_NAN = [(300, 7, 17), (4, 7, 4096)]
CROSSED_LAYOUT = [(300, 5, 17), (4, 3, 4096)]


RTOL = 1e-12
U53 = 2.0 ** -53


def rtol_of(d):
    """the bound on an output computed in another order, in units of the sum of its terms' magnitudes.  RTOL covers the sums of up
    to 1088 terms and "a few 2^-53" per term.  The latter does not hold where a distance sums thousands of squares: a sum of d
    non-negative squares taken in any order is within d 2^-53 of itself relatively, the square root halves that and the reciprocal
    keeps it, and every term of every output is such a distance or a difference over one.  So d 2^-53 is added for d > 128"""
    return RTOL + (d * U53 if d > 128 else 0.0)


def rows(K, n, d, seed=0):
    """generic rows: a conditional Gaussian sampler's draws, x_k = mu_i + sigma_i eps_k, and targets from a shifted law; no two
    points of a row coincide"""
    rng = np.random.RandomState(100003 * K + 101 * n + d + seed)
    mu, sigma = rng.normal(size=(1, n, d)) * 2.0, 0.5 + rng.uniform(size=(1, n, 1))
    X = mu + sigma * rng.normal(size=(K, n, d))
    Y = mu[0] + 0.3 + 0.8 * rng.normal(size=(n, d))
    return X, Y


def finite_rows(K, d, seed=0):
    """joint_scores_numpy.finite as stacked draws: (X [K, 5, d], Y [5, d]) float32 -- a tied pair, y equal to a draw, draws
    differing in their last bits, unit spread around 1e6, a far y"""
    xt, y = js.finite(K, d, seed)
    return np.ascontiguousarray(np.transpose(xt, (2, 0, 1))), y


def lattice_rows(K, n, d, seed=0):
    """integer-valued rows in {0, 1}^d: at d = 1 every distance is 0 or 1, so with K a power of two and fair=False every sum of
    the restatement and of any other order is exact"""
    rng = np.random.RandomState(7 * K + n + d + seed)
    return rng.randint(0, 2, size=(K, n, d)).astype(np.float64), rng.randint(0, 2, size=(n, d)).astype(np.float64)
