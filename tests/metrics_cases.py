"""Constructed inputs for the edges of pfm_mmd's median select and pfm_boot_moments, shared by tests/test_metrics_host.py
(which proves from the numpy restatement alone that every input has the property it is named for) and
tests/test_metrics_edges_gpu.py (which relies on that property).  Test helper, not product code.

The median of pfm_mmd is a six-digit radix select over the float64 bit pattern of d^2 (pf_metrics.hip: k_shift / k_width).  It
follows the two middle ranks (m*m - 1) / 2 and m*m / 2 of the full m x m matrix with one histogram while their key prefixes agree
and with two once they have parted.  Continuous data part the two keys in digit 0, 1 or 2; the cases here part them in each of the
six digits, never (an exact tie), and with one rank among the diagonal zeros."""
import numpy as np

import metrics_numpy as mn

# moments_longdouble is a yardstick only where long double is wider than float64 (x87: 64-bit significand)
assert np.finfo(np.longdouble).eps <= 2.0 ** -63, "np.longdouble is no wider than float64 on this platform"

SHIFT = (52, 41, 30, 19, 8, 0)            # pf_metrics.hip k_shift
WIDTH = (12, 11, 11, 11, 11, 8)           # pf_metrics.hip k_width
E = 2.0 ** -26


def key(v):
    """the select's key: the bit pattern of the float64 v >= 0, which orders like the value"""
    return int(np.float64(v).view(np.uint64))


def digits(v):
    k = key(v)
    return tuple((k >> s) & ((1 << w) - 1) for s, w in zip(SHIFT, WIDTH))


def parting_digit(a, b):
    """the first of the six digits in which the keys of a and b differ; None for equal keys"""
    for i, (x, y) in enumerate(zip(digits(a), digits(b))):
        if x != y:
            return i
    return None


def middle_values(Z):
    """the d^2 of rank (m*m - 1) // 2 and of rank m*m // 2 in the full m x m matrix of the rows of Z: the m diagonal zeros, then
    every pair i < j twice"""
    m = Z.shape[0]
    u = np.sort(mn.pooled_upper_d2(Z))

    def at(k):
        return 0.0 if k < m else float(u[(k - m) // 2])
    return at((m * m - 1) // 2), at(m * m // 2)


def four_points(ja, b):
    """X = [P0, P1], Y = [P2, P3] in the plane.  The smallest of the six d^2 is |P0 P3|^2 = e^2; the next two, the middle ranks
    7 and 8 of the 16 entries, are |P1 P3|^2 = 1 + (ja - 1)^2 e^2 and |P0 P1|^2 = 1 + ja^2 e^2 for b = 0.5 and ja <= 2^21"""
    X = np.array([[0.0, 0.0], [1.0, ja * E]])
    Y = np.array([[-1.0, b], [0.0, E]])
    return X, Y


# digit in which the two middle keys part -> (ja, b).  With b = 0.5 the middle values are 1 + (ja - 1)^2 2^-52 and
# 1 + ja^2 2^-52, both exact, and ja a power of two makes the lower one end in a run of ones up to the bit ja^2 sets.  With
# b = 0.5 both stay in [1, 2) and share digit 0; for digit 0, ja e = 1 + e and b = 1 make the middle values
# |P2 P3|^2 = 1 + (1 - e)^2 < 2 and |P1 P3|^2 = |P0 P2|^2 = 2.  (tests/test_metrics_host.py asserts each digit.)
PARTING = {5: (1, 0.5), 4: (2 ** 4, 0.5), 3: (2 ** 10, 0.5), 2: (2 ** 15, 0.5), 1: (2 ** 21, 0.5), 0: (2 ** 26 + 1, 1.0)}
# ja e = b = 1/4: |P1 P3|^2 and |P2 P3|^2 are both 1 + (1/4 - e)^2, and they are ranks 6 to 9
TIE = (2 ** 24, 0.25)

# one point each, one feature: the 2 x 2 matrix is [0, 0, d^2, d^2], rank 1 a diagonal zero and rank 2 the pair.  With
# Y = k 2^-537, d^2 = k^2 2^-1074 is the denormal whose key is the integer k^2, so the prefix of rank 1 stays all-zero (the
# diagonal is counted in every digit) and rank 2 leaves it in the digit holding bit 2 log2 k.
LADDER = {5: 1 * 2.0 ** -537, 4: 2 ** 4 * 2.0 ** -537, 3: 2 ** 10 * 2.0 ** -537, 2: 2 ** 15 * 2.0 ** -537,
          1: 2 ** 21 * 2.0 ** -537, 0: 1.5}


def ladder(y):
    return np.array([[0.0]]), np.array([[y]])


DYADIC_SHAPE = (70, 62, 2)
DYADIC_REPS = 4
DYADIC_SEED = 12


def dyadic():
    """-> X, Y, [(ix, iy)]: coordinates k / 4 in [0, 8): every d^2 is a multiple of 1 / 16 below 128, exact in any summation
    order, with or without fma, and shared by many pairs"""
    nx, ny, d = DYADIC_SHAPE
    rng = np.random.default_rng(DYADIC_SEED)
    X = rng.integers(0, 32, size=(nx, d)) / 4.0
    Y = rng.integers(0, 32, size=(ny, d)) / 4.0
    np.random.seed(DYADIC_SEED)
    return X, Y, mn.boot_indices(nx, ny, DYADIC_REPS)


def moments_longdouble(B):
    """-> (mean [d], cov [d, d]) of the rows of B in np.longdouble: the mean, then the centred products / (n - 1) (np.cov, ddof
    1).  One row gives an all-NaN covariance, as np.cov does."""
    B = np.asarray(B, dtype=np.longdouble)
    n = B.shape[0]
    mean = B.sum(axis=0) / np.longdouble(n)
    C = B - mean
    with np.errstate(invalid="ignore", divide="ignore"):
        cov = C.T.dot(C) / np.longdouble(n - 1)
    return mean, cov
