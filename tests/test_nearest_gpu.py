"""The k-nearest sweep that k_knn_radius<L> (pfm_prdc) and k_nn_index<L> (pfm_nn_index) share (csrc/pf_nearest.h), through the raw
bindings on poisoned outputs, and the replicate driver of the metrics' host side (_boot.replicates).

On the integer data sets every squared distance is exact in float64 (tests/test_nearest_host.py), so a radius is compared with
numpy's order statistic of the exact distance matrix byte for byte.  The two entry points are compared with each other on any
data: pfm_prdc's radius of a sample against itself is the (k + 1)-th smallest of a row with the row's own 0 counted, pfm_nn_index's
d2[:, k - 1] is the k-th nearest OTHER row, and both take their distances from one formula; after the sweep became one piece of
code, they can differ only in what the kernels do not share (row source, candidate filter, list length, output).

The shapes: 70 and 65 rows (two tiles a side, ragged), k at both ends of every list length, d = 17 (two feature chunks), a
duplicated sample (every value twice), and a 300-row line whose nearest rows come last, so that every tile replaces the lists.
"""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import hygiene  # noqa: E402
import native_libs  # noqa: E402
import nearest_numpy as nn  # noqa: E402
import twosample_numpy as tn  # noqa: E402
from probaforms_amd.metrics import _boot, _lib  # noqa: E402

pytestmark = pytest.mark.gpu

native_libs.ensure_built(_lib)


def dev(A, dtype=np.float64):
    return torch.from_numpy(np.array(A, dtype=dtype, order="C")).cuda()


def radii(X, Y, k):
    """pfm_prdc on the samples as given (identity indices, one replicate) -> numpy radius2_r [nr], radius2_f [nf]"""
    (nr, d), nf = X.shape, len(Y)
    ws = hygiene.workspace(_lib.prdc_workspace_bytes(nr, nf, d, 1, k), "ones")
    r2r = torch.empty((1, nr), dtype=torch.float64, device="cuda")
    r2f = torch.empty((1, nf), dtype=torch.float64, device="cuda")
    counts = torch.empty((1, 4), dtype=torch.int64, device="cuda")
    hygiene.poison_outputs(r2r, r2f, counts)
    st = _lib.prdc_status(dev(X), dev(Y), dev(np.arange(nr), np.int32), dev(np.arange(nf), np.int32), 1, k, r2r, r2f, counts, ws)
    torch.cuda.synchronize()
    assert st == 0 and hygiene.poisoned(r2r) == 0 and hygiene.poisoned(r2f) == 0 and hygiene.poisoned(counts) == 0
    return r2r.cpu().numpy()[0], r2f.cpu().numpy()[0]


def neighbour_d2(Z, k):
    """pfm_nn_index -> numpy d2 [n, k]"""
    n, d = Z.shape
    nbr = torch.empty((n, k), dtype=torch.int32, device="cuda")
    d2 = torch.empty((n, k), dtype=torch.float64, device="cuda")
    hygiene.poison_outputs(nbr, d2)
    st = _lib.nn_index_status(dev(Z), k, nbr, d2, hygiene.workspace(_lib.nn_index_workspace_bytes(n, d, k), "ones"))
    torch.cuda.synchronize()
    assert st == 0 and hygiene.poisoned(nbr) == 0 and hygiene.poisoned(d2) == 0
    return d2.cpu().numpy()


def check_exact(X, Y, k):
    got_r, got_f = radii(X, Y, k)
    for name, got, S in (("radius2_r", got_r, X), ("radius2_f", got_f, Y)):
        want = nn.kth(nn.exact_d2(S), k)
        print("k %d %s: %d of %d differ" % (k, name, int((got != want).sum()), want.size))
        assert got.tobytes() == want.tobytes(), (name, k, np.flatnonzero(got != want)[:5].tolist())


@pytest.mark.parametrize("k", nn.LIST_EDGES)
def test_radii_at_both_ends_of_every_list_length(k):
    check_exact(*nn.integer_samples(), k)


@pytest.mark.parametrize("descending", [True, False], ids=["real: nearest rows last", "real: nearest rows first"])
def test_orderings_that_attack_the_pruning(descending):
    """the real sample in one order and the fake sample in the other: in descending order every later tile replaces the lists"""
    X, Y = nn.integer_line(descending), nn.integer_line(not descending)
    assert nn.is_exact(X) and nn.is_exact(Y)
    for k in nn.LINE_KS:
        check_exact(X, Y, k)


def _duplicated():
    X = tn.data(70, 1, 3)[:70]
    return np.concatenate([X, X])


POOLED = {"135 rows, d 3": lambda: tn.data(70, 65, 3), "131 rows, d 17": lambda: tn.data(130, 1, 17), "[X; X]": _duplicated}


@pytest.mark.parametrize("name", list(POOLED))
def test_the_two_entry_points_agree(name):
    Z = POOLED[name]()
    for k in (1, 5, 16):
        with_self, _ = radii(Z, Z, k)
        others = neighbour_d2(Z, k)[:, k - 1]
        print("%s k %d: %d of %d differ" % (name, k, int((with_self != others).sum()), others.size))
        assert with_self.tobytes() == others.tobytes()
    if name == "[X; X]":
        assert (radii(Z, Z, 1)[0] == 0.0).all()                         # every row's copy


# ---- the replicate driver -----------------------------------------------------------------------------------

def test_driver_groups_and_indices(monkeypatch):
    na, nb, n_iters = 7, 5, 5
    monkeypatch.setattr(_boot, "MAX_GROUP", 2)
    calls = []

    def launch(start, reps, ia, ib, ws):
        assert ia.dtype == torch.int32 and ib.dtype == torch.int32 and ws.dtype == torch.uint8 and ws.numel() >= 100 * reps
        calls.append((start, reps, ia.cpu().numpy().copy(), ib.cpu().numpy().copy()))

    np.random.seed(11)
    _boot.replicates(na, nb, torch.device("cuda", torch.cuda.current_device()), n_iters, lambda r: 100 * r, launch)
    after = np.random.random()
    assert [c[:2] for c in calls] == [(0, 2), (2, 2), (4, 1)]
    np.random.seed(11)
    for start, reps, ia, ib in calls:                                   # the stream is drawn group by group
        want = np.empty(reps * (na + nb), np.int32)
        _boot.draw_indices(want, reps, na, nb)
        assert ia.tobytes() == want[:reps * na].tobytes() and ib.tobytes() == want[reps * na:].tobytes()
    assert np.random.random() == after


def test_driver_identity_replicate_draws_nothing():
    na, nb = 7, 5
    calls = []

    def launch(start, reps, ia, ib, ws):
        assert ws.numel() >= 100
        calls.append((start, reps, ia.cpu().numpy(), ib.cpu().numpy()))

    np.random.seed(11)
    before = np.random.get_state()
    _boot.replicates(na, nb, torch.device("cuda", torch.cuda.current_device()), None, lambda r: 100 * r, launch)
    after = np.random.get_state()
    assert before[0] == after[0] and (before[1] == after[1]).all() and before[2:] == after[2:]
    assert len(calls) == 1 and calls[0][:2] == (0, 1)
    for got, n in zip(calls[0][2:], (na, nb)):
        assert got.dtype == np.int32 and got.tolist() == list(range(n))
