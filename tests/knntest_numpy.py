"""Float64 numpy / scipy restatement of probaforms_amd.metrics.twosample.knn_test (kernels: pf_nn.hip):
  neighbours  every row's k nearest other rows: scipy's cdist(..., "sqeuclidean"), the diagonal set to inf, a stable argsort, so
              that equal squared distances are ordered by row index;
  counts      per labelling, the (row, neighbour) slots whose two labels are both non-zero and both zero;
  shares      the counts as same-label shares of all rows', the real rows' and the fake rows' slots;
  test        the whole public call: twosample_numpy's seed draw and labellings, the observed labelling in front of the drawn
              ones, the statistic, the null values and the p-value;
  min_gap     the condition under which two implementations of d^2 order a continuous data set's neighbours alike.
The yardstick the nearest-neighbour tests hold the GPU kernels and the committed fixtures against.  Test helper, not product code.
"""
import numpy as np
from scipy.spatial.distance import cdist

import twosample_numpy as tn

GAP = 1e-9                        # the least relative gap between consecutive squared distances among a row's first k + 1


def sorted_d2(Z):
    """-> (order [N, N], D2 [N, N]): every row's other rows in ascending (d^2, index) order, itself last (inf)"""
    Z = np.asarray(Z, np.float64)
    D = cdist(Z, Z, "sqeuclidean")
    np.fill_diagonal(D, np.inf)
    return np.argsort(D, axis=1, kind="stable"), D


def neighbours(Z, k):
    """-> (nbr int32 [N, k], d2 float64 [N, k])"""
    order, D = sorted_d2(Z)
    nbr = order[:, :k]
    return nbr.astype(np.int32), np.take_along_axis(D, nbr, axis=1)


def min_gap(Z, k):
    """the smallest relative gap (b - a) / b between consecutive squared distances a <= b among any row's first k + 1
    neighbours (k where there are only k other rows); 0 at a tie"""
    order, D = sorted_d2(Z)
    m = min(k + 1, len(D) - 1)
    v = np.take_along_axis(D, order[:, :m], axis=1)
    if m < 2:
        return np.inf
    a, b = v[:, :-1], v[:, 1:]
    return float(np.min(np.where(b > 0, (b - a) / np.where(b > 0, b, 1.0), 0.0)))


def counts(nbr, L):
    """nbr [N, k], L [reps, N] -> int64 [reps, 2]: slots with both labels non-zero, slots with both zero"""
    L = np.atleast_2d(np.asarray(L)) != 0
    own, other = L[:, :, None], L[:, np.asarray(nbr, np.int64)]           # [reps, N, 1], [reps, N, k]
    return np.stack([(own & other).sum(axis=(1, 2)), (~own & ~other).sum(axis=(1, 2))], axis=1).astype(np.int64)


def shares(C, nr, nf, k):
    """int counts [reps, 2] -> float64 [reps, 3]: Python ints divided, rounded once"""
    return np.array([[(int(a) + int(b)) / ((nr + nf) * k), int(a) / (nr * k), int(b) / (nf * k)] for a, b in C],
                    dtype=np.float64).reshape(-1, 3)


def expected_null(nr, nf):
    """the expected statistic under the null hypothesis"""
    N = nr + nf
    return (nr * (nr - 1) + nf * (nf - 1)) / (N * (N - 1))


def test(X, Y, n_permutations, k, nbr=None):
    """the public call on the samples as given (standardize them first where that is meant) -> dict: key (the drawn seed),
    statistic, null, pvalue, real, fake and the generator's next random(); nbr: the neighbour table, where the caller has one"""
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    nr, nf = len(X), len(Y)
    seed = tn.draw_seed()
    nxt = np.random.random()
    L = np.concatenate([tn.observed(nr + nf, nr)[None], tn.labels(seed, 0, n_permutations, nr + nf, nr)])
    if nbr is None:
        nbr = neighbours(np.concatenate([X, Y]), k)[0]
    V = shares(counts(nbr, L), nr, nf, k)
    return dict(key=seed, statistic=V[0, 0], null=V[1:, 0].copy(), pvalue=np.float64(tn.pvalue(V[0, 0], V[1:, 0])), real=V[0, 1],
                fake=V[0, 2], next=nxt)


test.__test__ = False             # (not a pytest test, whatever imports it)


# ---- the shapes the host and GPU tests share ---------------------------------------------------------------------------

# (nr, nf, d, k) on twosample_numpy.data: 2 and k + 1 pooled rows, 64 / 65 / 129 rows (tile edges), d = 1, 16, 17, 33 (one feature
# chunk exactly, a second, a third), k at both ends of every list length of pfm_nn_index (2, 5, 10, 16), 2200 rows (35 tiles)
LIST_EDGES = [1, 2, 3, 5, 6, 10, 11, 16]
INDEX_CASES = [(1, 1, 1, 1), (1, 1, 17, 1), (2, 2, 3, 3), (9, 8, 16, 16), (40, 24, 1, 5), (40, 24, 1, 1), (33, 32, 16, 16),
               (33, 32, 17, 2), (64, 64, 17, 3), (64, 65, 33, 6), (100, 29, 33, 11), (100, 29, 16, 10), (130, 93, 3, 5),
               (200, 150, 17, 7), (1200, 1000, 3, 16), (1200, 1000, 1, 16), (1200, 1000, 3, 1)]
CKDTREE_CASE = (1200, 1000, 3, 5)
LINE_N = 300                      # rows of line(): five candidate tiles
MOD7 = (200, [5, 16])             # the column j mod 7 at 200 rows: exact ties, many-fold, across lanes and tiles
INTEGER = (65, 63)
COUNT_NS = [2, 64, 257, 2200]     # and the staging limit and one row more
COUNT_REPS = [1, 17, 129, 1000]
SEED = tn.SEED


def mod7(n):
    return (np.arange(n) % 7).astype(np.float64)[:, None]


def line(descending, n=LINE_N):
    """d = 1: row 0 at 0 and the others at distinct distances from it, the nearest rows last (descending) or first"""
    rng = np.random.default_rng(77)
    x = np.sort(rng.uniform(1.0, 2.0, n - 1))
    return np.concatenate([[0.0], x[::-1] if descending else x])[:, None]


def random_nbr(n, k, seed=5):
    return np.random.default_rng(seed + n + k).integers(0, n, size=(n, k)).astype(np.int32)
