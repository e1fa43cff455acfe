#!/usr/bin/env python3
"""Generate tests/golden/knntest_*.npz: the nearest-neighbour permutation two-sample test knn_test, computed apart from the
restatement tests/knntest_numpy.py: the neighbours come from scipy.spatial.cKDTree.query(k + 1) with the row itself dropped by
its index (the restatement sorts scipy's cdist), the labellings from the numpy Philox of tests/twosample_numpy.py, and the counts
from a loop over the rows.  Needs numpy and scipy only:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_knntest.py

Per case the file holds X, Y, seed (np.random.seed before the call), n_permutations, nearest_k, standardize (whether the values
are those of the samples scaled by the real sample's StandardScaler), next (np.random.random() after a call: each call makes the
one seed draw), and
  statistic   the share of the N nearest_k neighbour slots whose neighbour carries the row's own label, samples as given
  real, fake  the same share among the real rows' and among the fake rows' slots
  null        [n_permutations] the statistic of the drawn labellings, labelling p at index p
  pvalue      (1 + #{null >= statistic}) / (1 + n_permutations)
All of them are ratios of integers, rounded once: an implementation that finds the same neighbours gives the same bits.

A KD-tree orders equal distances as it pleases, and two ways of accumulating d^2 may order nearly equal ones differently.  So the
generator asserts, per row, that consecutive squared distances among its first nearest_k + 1 neighbours differ by 1e-9 relative
at least (the row's own copy at distance 0, in the copy case, is followed by a gap of 1).
"""
import os
import sys

import numpy as np
from scipy.spatial import cKDTree

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import twosample_numpy as tn  # noqa: E402

GAP = 1e-9


def kdtree_neighbours(Z, k):
    """-> int [N, k]: cKDTree's k + 1 nearest with the row itself dropped; the gap condition is asserted"""
    N = len(Z)
    m = min(k + 2, N)                                  # one more than needed, for the gap behind rank k - 1
    dist, idx = cKDTree(Z).query(Z, k=m)
    dist, idx = dist.reshape(N, m), idx.reshape(N, m)
    nbr = np.empty((N, k), np.int64)
    for a in range(N):
        keep = idx[a] != a
        assert keep.sum() == m - 1, "row %d is not among its own nearest" % a
        nbr[a] = idx[a][keep][:k]
        v = dist[a][keep] ** 2
        lo, hi = v[:-1], v[1:]
        assert (hi - lo >= GAP * hi).all() and (hi > 0).all(), "row %d: neighbours too close to a tie" % a
    return nbr


def count_pairs(nbr, lab):
    """(slots whose row and neighbour are both labelled, both unlabelled) of one labelling, as Python ints"""
    both1 = both0 = 0
    for a in range(len(nbr)):
        for j in nbr[a]:
            both1 += int(lab[a] != 0 and lab[j] != 0)
            both0 += int(lab[a] == 0 and lab[j] == 0)
    return both1, both0


def case(X, Y, seed, P, k, standardize=False):
    Xs, Ys = tn.standardize(X, Y) if standardize else (X, Y)
    nr, nf = len(X), len(Y)
    N = nr + nf
    nbr = kdtree_neighbours(np.concatenate([Xs, Ys]), k)
    np.random.seed(seed)
    key = tn.draw_seed()
    nxt = np.random.random()
    L = np.concatenate([tn.observed(N, nr)[None], tn.labels(key, 0, P, N, nr)])
    C = [count_pairs(nbr, lab) for lab in L]
    total = np.array([(a + b) / (N * k) for a, b in C], np.float64)
    statistic, null = total[0], total[1:].copy()
    pvalue = np.float64((1 + int((null >= statistic).sum())) / (1 + P))
    return dict(X=X, Y=Y, seed=seed, n_permutations=P, nearest_k=k, standardize=standardize, next=nxt, statistic=statistic,
                null=null, pvalue=pvalue, real=np.float64(C[0][0] / (nr * k)), fake=np.float64(C[0][1] / (nf * k)))


def cases():
    """-> {name: the file's arrays}; numpy and scipy only"""
    rng = np.random.default_rng(1919)
    out = {}
    out["shift_130_93_d3_k1"] = case(rng.normal(size=(130, 3)), rng.normal(0.6, 1.0, size=(93, 3)), seed=81, P=199, k=1)
    out["equal_130_93_d3_k5"] = case(rng.normal(size=(130, 3)), rng.normal(size=(93, 3)), seed=82, P=199, k=5)
    X = rng.normal(size=(70, 3))
    out["copy_70_70_d3_k1"] = case(X, X.copy(), seed=83, P=99, k=1)
    out["tiny_2_3_d2_k4"] = case(rng.normal(size=(2, 2)), rng.normal(size=(3, 2)), seed=84, P=20, k=4)
    real = np.concatenate([rng.normal(-4, 1, size=(60, 3)), rng.normal(4, 1, size=(60, 3))]) * [5.0, 0.1, 1.0] + [100.0, 0, -7]
    fake = np.concatenate([rng.normal(-3, 1, size=(50, 3)), rng.normal(5, 1, size=(50, 3))]) * [5.0, 0.1, 1.0] + [100.0, 0, -7]
    out["clusters_standardized_k3"] = case(real, fake, seed=85, P=99, k=3, standardize=True)
    return out


def main():
    for name, arrays in cases().items():
        path = os.path.join(HERE, "knntest_%s.npz" % name)
        np.savez_compressed(path, **arrays)
        print(name, arrays["X"].shape, arrays["Y"].shape, "k", arrays["nearest_k"], "statistic", arrays["statistic"], "real",
              arrays["real"], "fake", arrays["fake"], "p", arrays["pvalue"], os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
