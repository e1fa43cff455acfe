"""What tests/test_nearest_host.py and tests/test_nearest_gpu.py share: the data sets on which every squared distance is exact in
float64, and the exact order statistic the k-nearest sweep (csrc/pf_nearest.h) has to return on them."""
import numpy as np

import knntest_numpy as kn
import twosample_numpy as tn

LIST_EDGES = kn.LIST_EDGES          # k at both ends of every list length of k_knn_radius<L> and k_nn_index<L>
INTEGER = (70, 65, 3)               # (nr, nf, d) of tn.integer_data: two tiles a side, ragged
LINE_KS = (1, 5, 16)


def exact_d2(Z):
    """the squared-distance matrix of integer rows: differences, squares and sums are integers below 2^53, so every
    convention (fused or not, any order) gives these bits"""
    Z = np.asarray(Z, np.float64)
    return ((Z[:, None, :] - Z[None, :, :]) ** 2).sum(axis=-1)


def kth(D2, k):
    """per row the (k + 1)-th smallest entry, the row's own 0 counted: the squared radius of pfm_prdc"""
    return np.partition(D2, k, axis=1)[:, k]


def integer_samples():
    nr, nf, d = INTEGER
    Z = tn.integer_data(nr, nf, d)
    return Z[:nr], Z[nr:]


def integer_line(descending, n=kn.LINE_N):
    """kn.line on integers: row 0 at 0 and the others at distinct integers in 1000 .. 2999, the nearest rows last
    (descending: every later candidate tile replaces the lists) or first"""
    x = np.sort(np.random.default_rng(77).choice(np.arange(1000, 3000), size=n - 1, replace=False)).astype(np.float64)
    return np.concatenate([[0.0], x[::-1] if descending else x])[:, None]


def is_exact(Z):
    """integer coordinates whose squared distances stay below 2^53"""
    Z = np.asarray(Z, np.float64)
    return bool((Z == np.round(Z)).all()) and float(Z.shape[1] * (2 * np.abs(Z).max()) ** 2) < 2.0 ** 53
