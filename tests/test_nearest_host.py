"""The inputs of tests/test_nearest_gpu.py, checked without a GPU: on them every squared distance is an integer below 2^53, so the
radii the kernels return can be compared with numpy's order statistic byte for byte."""
import numpy as np
import pytest

import nearest_numpy as nn


def test_integer_samples_are_exact():
    X, Y = nn.integer_samples()
    assert (len(X), len(Y), X.shape[1]) == nn.INTEGER
    for S in (X, Y):
        assert nn.is_exact(S)
        D2 = nn.exact_d2(S)
        assert (D2 == np.round(D2)).all() and D2.max() < 2.0 ** 53 and (np.diag(D2) == 0).all()
    assert max(nn.LIST_EDGES) < min(len(X), len(Y))


@pytest.mark.parametrize("descending", [True, False])
def test_integer_line_is_exact_and_ordered(descending):
    Z = nn.integer_line(descending)
    assert nn.is_exact(Z) and len(np.unique(Z)) == len(Z) > 4 * 64       # distinct rows, five candidate tiles
    step = np.diff(Z[1:, 0])
    assert (step < 0).all() if descending else (step > 0).all()
    D2 = nn.exact_d2(Z)
    assert D2.max() < 2.0 ** 53
    for k in nn.LINE_KS:                                                # row 0's radius: its k-th nearest other row
        assert nn.kth(D2, k)[0] == np.sort(Z[1:, 0])[k - 1] ** 2


def test_kth_counts_the_row_itself():
    D2 = nn.exact_d2(np.array([[0.0], [1.0], [1.0], [3.0]]))
    assert nn.kth(D2, 1).tolist() == [1.0, 0.0, 0.0, 4.0] and nn.kth(D2, 2).tolist() == [1.0, 1.0, 1.0, 4.0]
