"""probaforms_amd.metrics.twosample.knn_test on the GPU (pfm_nn_index and pfm_nn_count in libpf_metrics.so) against the float64
restatement (tests/knntest_numpy.py) and the committed fixtures (tests/golden/knntest_*.npz).

The neighbour rows are compared byte for byte.  On the continuous data sets that is sound because consecutive squared distances
among a row's first k + 1 neighbours differ by 1e-9 relative at least (tests/test_knntest_host.py asserts it for every shape used
here), far above what two ways of accumulating d^2 in float64 differ by; on the integer data sets d^2 is exact, ties are real and
the (d^2, row index) order is fully determined.  A squared distance is compared within 1e-12 relative, the project's tolerance for
float64 sums taken in another order (here: with and without fused multiply-adds), and a duplicate's must be exactly 0.  The counts
and everything the public calls return are integers and ratios of integers: compared with ==.

The shapes: two pooled rows, k + 1 rows, 64 / 65 / 129 rows (tile edges), 2200 rows (35 candidate tiles: the bound shared among a
row's lanes prunes), d = 1, 16, 17, 33 (one feature chunk exactly, a second, a third), k at both ends of every list length the
kernel is instantiated for, and for the counts the staging limit of the labelling's bits and one row more.
"""
import functools
import glob
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, ROOT)

import knntest_numpy as kn  # noqa: E402
import twosample_numpy as tn  # noqa: E402
import hygiene  # noqa: E402
import native_libs  # noqa: E402
from probaforms_amd.metrics import _lib, twosample  # noqa: E402

pytestmark = pytest.mark.gpu

native_libs.ensure_built(_lib)

FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "knntest_*.npz")))
K_MAX = _lib.NN_MAX_K
LIMIT = _lib.NN_STAGE_MAX_N


def fid(p):
    return os.path.basename(p)[8:-4]


def dev(A, dtype=np.float64):
    return torch.from_numpy(np.array(A, dtype=dtype, order="C")).cuda()


def raw_index(Z, k, ws=None, pattern="zeros"):
    """pfm_nn_index through the raw binding on poisoned outputs -> (status, nbr [n, k] int32, d2 [n, k])"""
    n, d = Z.shape
    if ws is None:
        ws = hygiene.workspace(_lib.nn_index_workspace_bytes(n, d, k), pattern)
    nbr = torch.empty((n, k), dtype=torch.int32, device="cuda")
    d2 = torch.empty((n, k), dtype=torch.float64, device="cuda")
    hygiene.poison_outputs(nbr, d2)
    st = _lib.nn_index_status(dev(Z), k, nbr, d2, ws)
    torch.cuda.synchronize()
    return st, nbr, d2


def raw_count(nbr, L, ws=None, pattern="zeros"):
    """pfm_nn_count through the raw binding on poisoned outputs -> (status, counts [reps, 2] int64)"""
    (n, k), reps = nbr.shape, len(L)
    if ws is None:
        ws = hygiene.workspace(_lib.nn_count_workspace_bytes(n, k, reps), pattern)
    C = torch.empty((reps, 2), dtype=torch.int64, device="cuda")
    hygiene.poison_outputs(C)
    st = _lib.nn_count_status(dev(nbr, np.int32), n, k, dev(L, np.uint8), reps, C, ws)
    torch.cuda.synchronize()
    return st, C


# ---- the neighbours ---------------------------------------------------------------------------------------

def check_index(Z, k):
    st, nbr, d2 = raw_index(Z, k)
    assert st == 0 and hygiene.poisoned(nbr) == 0 and hygiene.poisoned(d2) == 0
    want, want_d2 = kn.neighbours(Z, k)
    got, got_d2 = nbr.cpu().numpy(), d2.cpu().numpy()
    assert got.tobytes() == want.tobytes(), "rows differ at %s" % (np.argwhere(got != want)[:5].tolist(),)
    err = np.abs(got_d2 - want_d2)
    print("n %d d %d k %d: largest relative difference of d^2 %.3g" % (Z.shape + (k, (err / np.where(want_d2 > 0, want_d2, 1)).max())))
    assert (err <= 1e-12 * want_d2).all() and (got_d2[want_d2 == 0.0] == 0.0).all() and not np.signbit(got_d2).any()
    assert (got != np.arange(len(Z))[:, None]).all()
    return nbr, d2


@pytest.mark.parametrize("nr,nf,d,k", kn.INDEX_CASES)
def test_index_equals_the_restatement(nr, nf, d, k):
    check_index(tn.data(nr, nf, d), k)


@pytest.mark.parametrize("k", kn.LIST_EDGES)
def test_index_at_both_ends_of_every_list_length(k):
    nr, nf, d = tn.OTHER[0]
    check_index(tn.data(nr, nf, d), k)


@pytest.mark.parametrize("descending", [True, False], ids=["nearest rows last", "nearest rows first"])
def test_orderings_that_attack_the_pruning(descending):
    """descending: every later tile holds rows nearer to row 0, so its lists are replaced tile after tile"""
    Z = kn.line(descending)
    for k in (1, 5, K_MAX):
        nbr, _ = check_index(Z, k)
        first = nbr[0].cpu().numpy().tolist()
        assert first == (list(range(kn.LINE_N - 1, kn.LINE_N - 1 - k, -1)) if descending else list(range(1, k + 1)))


def test_ties_are_ordered_by_row_index():
    n, ks = kn.MOD7
    for k in ks:                                                   # 28 or 29 rows at distance 0 from every row
        nbr, d2 = check_index(kn.mod7(n), k)
        assert (d2 == 0.0).all()
        assert nbr[8].cpu().numpy().tolist() == [j for j in range(1, n, 7) if j != 8][:k]
    Z = tn.integer_data(*kn.INTEGER)
    for k in (1, 6, K_MAX):
        check_index(Z, k)
    X = tn.data(70, 1, 3)[:70]                                       # Z = [X; X]: every row's nearest neighbour is its copy
    for k in (1, 3):
        nbr, d2 = check_index(np.concatenate([X, X]), k)
        assert (nbr[:, 0].cpu().numpy() == (np.arange(140) + 70) % 140).all() and (d2[:, 0] == 0.0).all() and (d2[:, 1:] > 0).all()


def test_a_rows_neighbours_do_not_depend_on_the_call():
    nr, nf, d = tn.OTHER[2]
    Z = tn.data(nr, nf, d)
    st, a, a2 = raw_index(Z, 7)
    st2, b, b2 = raw_index(Z, 7)
    st3, c, c2 = raw_index(Z, 7, ws=hygiene.workspace(4096, "ones"))
    assert st == 0 and st2 == 0 and st3 == 0
    assert hygiene.same_bits(a, b) and hygiene.same_bits(a2, b2) and hygiene.same_bits(a, c) and hygiene.same_bits(a2, c2)
    st, e, e2 = raw_index(Z, 10)                                    # the first 7 of 10 neighbours: another list length
    assert st == 0 and hygiene.same_bits(a, e[:, :7].contiguous()) and hygiene.same_bits(a2, e2[:, :7].contiguous())


@pytest.mark.parametrize("nr,nf,d", tn.OTHER[1:])
def test_index_results_do_not_depend_on_the_workspace(nr, nf, d):
    Z, PZ = tn.data(nr, nf, d), tn.data(nr + 70, nf + 30, d)        # the `replay` primer: a larger call
    need = max(_lib.nn_index_workspace_bytes(nr + nf, d, 5), _lib.nn_index_workspace_bytes(nr + nf + 100, d, 7))
    outs = {}
    for pat in hygiene.PATTERNS:
        ws = hygiene.workspace(need, pat)
        if pat == "replay":
            assert raw_index(PZ, 7, ws=ws)[0] == 0
        st, nbr, d2 = raw_index(Z, 5, ws=ws)
        assert st == 0
        outs[pat] = dict(nbr=nbr, d2=d2)
    hygiene.assert_all_written(outs["zeros"], "pfm_nn_index")
    hygiene.assert_pattern_independent(outs, "pfm_nn_index")


def test_index_statuses_leave_the_outputs_alone():
    nr, nf, d = tn.OTHER[1]
    Z = tn.data(nr, nf, d)
    short = torch.empty(_lib.nn_index_workspace_bytes(nr + nf, d, 3) - 1, dtype=torch.uint8, device="cuda")
    for want, (A, k, ws) in ((_lib.PFM_EWORKSPACE, (Z, 3, short)), (_lib.PFM_EINVAL, (Z[:9], 9, None)),
                             (_lib.PFM_EUNSUPPORTED, (Z, K_MAX + 1, None)), (_lib.PFM_EINVAL, (Z[:1], 1, None))):
        st, nbr, d2 = raw_index(A, k, ws=ws)
        assert st == want and hygiene.poisoned(nbr) == nbr.numel() and hygiene.poisoned(d2) == d2.numel(), (want, k)


# ---- the counts -------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def labellings(n, reps):
    L = tn.labels(kn.SEED, 0, reps, n, max(1, (2 * n) // 5))
    L.setflags(write=False)
    return L


def check_count(n, k, reps):
    nbr, L = kn.random_nbr(n, k), labellings(n, reps)
    st, C = raw_count(nbr, L)
    assert st == 0 and hygiene.poisoned(C) == 0
    assert np.array_equal(C.cpu().numpy(), kn.counts(nbr, L)), (n, k, reps)
    return C


@pytest.mark.parametrize("k", [1, K_MAX])
@pytest.mark.parametrize("n", kn.COUNT_NS)
def test_counts_equal_the_restatement(n, k):
    for reps in kn.COUNT_REPS:
        check_count(n, k, reps)


@pytest.mark.parametrize("k", [1, K_MAX])
@pytest.mark.parametrize("n", [LIMIT, LIMIT + 1], ids=["staging limit", "limit + 1"])
def test_counts_on_both_sides_of_the_staging_limit(n, k):
    C = check_count(n, k, 3)
    assert int(C.sum()) > 0


@pytest.mark.parametrize("n", [2, 257, 2200])
def test_constant_labellings(n):
    for k in (1, K_MAX):
        nbr = kn.random_nbr(n, k)
        L = np.stack([np.ones(n, np.uint8), np.zeros(n, np.uint8), np.full(n, 255, np.uint8)])       # any non-zero byte is a label
        st, C = raw_count(nbr, L)
        assert st == 0 and C.cpu().numpy().tolist() == [[n * k, 0], [0, n * k], [n * k, 0]]


def test_a_labelling_alone_equals_the_labelling_inside_a_group():
    n, k = 2200, 5
    nbr, L = kn.random_nbr(n, k), labellings(n, 129)
    st, together = raw_count(nbr, L)
    st2, again = raw_count(nbr, L)
    assert st == 0 and st2 == 0 and hygiene.same_bits(together, again)
    for r in (0, 1, 64, 128):
        st, alone = raw_count(nbr, L[r:r + 1])
        assert st == 0 and hygiene.same_bits(alone, together[r:r + 1]), r
    st, part = raw_count(nbr, L[100:129])                           # and at another place in another call
    assert st == 0 and hygiene.same_bits(part, together[100:129])


@pytest.mark.parametrize("n,k", [(257, 3), (70000, 9)], ids=["one slice", "three slices"])
def test_count_results_do_not_depend_on_the_workspace(n, k):
    reps = 5
    nbr, L = kn.random_nbr(n, k), labellings(n, reps)
    pn = n + 5000
    pnbr, PL = kn.random_nbr(pn, k + 1), labellings(pn, reps + 2)    # the `replay` primer: more of everything
    need = max(_lib.nn_count_workspace_bytes(n, k, reps), _lib.nn_count_workspace_bytes(pn, k + 1, reps + 2))
    outs = {}
    for pat in hygiene.PATTERNS:
        ws = hygiene.workspace(need, pat)
        if pat == "replay":
            assert raw_count(pnbr, PL, ws=ws)[0] == 0
        st, C = raw_count(nbr, L, ws=ws)
        assert st == 0
        outs[pat] = dict(counts=C)
    hygiene.assert_all_written(outs["zeros"], "pfm_nn_count")
    hygiene.assert_pattern_independent(outs, "pfm_nn_count")
    assert np.array_equal(outs["zeros"]["counts"].cpu().numpy(), kn.counts(nbr, L))


def test_count_statuses_leave_the_outputs_alone():
    n, k, reps = 70000, 9, 5
    nbr, L = kn.random_nbr(n, k), labellings(n, reps)
    need = _lib.nn_count_workspace_bytes(n, k, reps)
    st, C = raw_count(nbr, L, ws=torch.empty(need - 1, dtype=torch.uint8, device="cuda"))
    assert st == _lib.PFM_EWORKSPACE and hygiene.poisoned(C) == C.numel()
    C = torch.empty((reps, 2), dtype=torch.int64, device="cuda")
    hygiene.poison_outputs(C)
    dn, dl, ws = dev(nbr, np.int32), dev(L, np.uint8), hygiene.workspace(need, "zeros")
    st = _lib.lib().pfm_nn_count(None, dn.data_ptr(), n, 0, dl.data_ptr(), reps, C.data_ptr(), ws.data_ptr(), need)
    torch.cuda.synchronize()
    assert st == _lib.PFM_EINVAL and hygiene.poisoned(C) == C.numel()


# ---- the public calls -------------------------------------------------------------------------------------

def check_result(t, P):
    assert isinstance(t, twosample.KnnTest)
    for v in (t.statistic, t.pvalue, t.real, t.fake):
        assert isinstance(v, np.float64) and 0.0 <= v <= 1.0
    assert isinstance(t.null, np.ndarray) and t.null.dtype == np.float64 and t.null.shape == (P,)
    assert t.pvalue.tobytes() == np.float64((1 + int((t.null >= t.statistic).sum())) / (1 + P)).tobytes()


def same(t, u):
    return all(np.asarray(a).tobytes() == np.asarray(b).tobytes() for a, b in zip(t, u))


@pytest.mark.parametrize("path", FIXTURES, ids=fid)
def test_fixtures(path):
    f = np.load(path)
    X, Y, P, k, std = f["X"], f["Y"], int(f["n_permutations"]), int(f["nearest_k"]), bool(f["standardize"])
    np.random.seed(int(f["seed"]))
    t = twosample.knn_test(X, Y, n_permutations=P, nearest_k=k, standardize=std)
    assert np.random.random() == float(f["next"])
    check_result(t, P)
    print("statistic %r (fixture %r), p %r (%r)" % (t.statistic, float(f["statistic"]), t.pvalue, float(f["pvalue"])))
    assert t.statistic == f["statistic"] and t.real == f["real"] and t.fake == f["fake"] and t.pvalue == f["pvalue"]
    assert np.array_equal(t.null, f["null"])
    np.random.seed(int(f["seed"]))                                   # a seeded call is bitwise reproducible
    assert same(t, twosample.knn_test(X, Y, n_permutations=P, nearest_k=k, standardize=std))
    state = np.random.get_state()
    a = twosample.nn_accuracy_full_sample(X, Y, nearest_k=k, standardize=std)
    assert isinstance(a, twosample.NnAccuracy) and all(isinstance(v, np.float64) for v in a)
    assert tuple(a) == (t.statistic, t.real, t.fake)
    after = np.random.get_state()
    assert state[0] == after[0] and np.array_equal(state[1], after[1]) and state[2:] == after[2:]


def test_the_rows_are_relabelled_exactly_as_energy_test_relabels_them():
    nr, nf, d = tn.OTHER[0]
    Z = tn.data(nr, nf, d)
    X, Y = Z[:nr], Z[nr:]
    for k in (1, 5):
        np.random.seed(11)
        twosample.energy_test(X, Y, n_permutations=40)
        after_energy = np.random.random()
        np.random.seed(11)
        t = twosample.knn_test(X, Y, n_permutations=40, nearest_k=k)
        assert np.random.random() == after_energy
        np.random.seed(11)
        o = kn.test(X, Y, 40, k)                                     # tn.draw_seed(): the draw energy_test makes
        assert o["next"] == after_energy
        check_result(t, 40)
        assert same(t, twosample.KnnTest(o["statistic"], o["pvalue"], o["null"], o["real"], o["fake"]))


def test_a_copy_scores_zero():
    X = tn.data(70, 1, 3)[:70]
    np.random.seed(12)
    t = twosample.knn_test(X, X.copy(), n_permutations=99, nearest_k=1)
    check_result(t, 99)
    assert t.statistic == 0.0 and t.real == 0.0 and t.fake == 0.0 and t.pvalue == 1.0 and (t.null > 0).all()
    assert not np.signbit(t.statistic)


def test_separated_samples_score_one():
    Z = tn.data(70, 50, 2)
    np.random.seed(13)
    t = twosample.knn_test(Z[:70], Z[70:] + 100.0, n_permutations=99, nearest_k=1)
    check_result(t, 99)
    assert t.statistic == 1.0 and t.real == 1.0 and t.fake == 1.0 and t.pvalue == 1 / 100
    t = twosample.knn_test(Z[:70], Z[70:] + 100.0, n_permutations=99, nearest_k=K_MAX)
    assert t.statistic == 1.0 and t.pvalue == 1 / 100


def test_groups(monkeypatch):
    """n_permutations of 1 and of 300; the latter in several pfm_nn_count calls and one pfm_nn_index call, which give the bits
    of the one group"""
    nr, nf, d = tn.OTHER[0]
    Z = tn.data(nr, nf, d)
    X, Y = Z[:nr], Z[nr:]
    for k in (1, 5):
        np.random.seed(5)
        one = twosample.knn_test(X, Y, n_permutations=1, nearest_k=k)
        check_result(one, 1)
        np.random.seed(5)
        whole = twosample.knn_test(X, Y, n_permutations=300, nearest_k=k)
        check_result(whole, 300)
        assert whole.statistic == one.statistic and whole.null[0] == one.null[0] and whole.real == one.real
        counted, indexed = [], []
        real_count, real_index = _lib.nn_count, _lib.nn_index

        def count(*a):
            counted.append(a[4])
            real_count(*a)

        def index(*a):
            indexed.append(a[1])
            real_index(*a)

        with monkeypatch.context() as m:
            per = nr + nf + _lib.nn_count_workspace_bytes(nr + nf, k, 1)
            m.setattr(twosample, "GROUP_BYTES", 128 * per)
            m.setattr(_lib, "nn_count", count)
            m.setattr(_lib, "nn_index", index)
            np.random.seed(5)
            split = twosample.knn_test(X, Y, n_permutations=300, nearest_k=k)
        assert counted == [128, 128, 45] and indexed == [k]
        assert same(split, whole)


def test_inputs_give_the_same_bits():
    Z = tn.data(200, 150, 2)
    X32, Y32 = torch.from_numpy(Z[:200]).float(), torch.from_numpy(Z[200:]).float()
    X64, Y64 = X32.double(), Y32.double()
    forms = {"numpy": (X64.numpy(), Y64.numpy()), "lists": (X64.numpy().tolist(), Y64.numpy().tolist()),
             "cuda float32": (X32.cuda(), Y32.cuda()), "cuda float64": (X64.cuda(), Y64.cuda()), "mixed": (X64.numpy(), Y32.cuda())}
    want = None
    for name, (A, B) in forms.items():
        np.random.seed(4)
        t = twosample.knn_test(A, B, n_permutations=20, nearest_k=3)
        want = want or t
        assert same(t, want), name
        assert tuple(twosample.nn_accuracy_full_sample(A, B, nearest_k=3)) == (want.statistic, want.real, want.fake), name


def test_standardize():
    nr, nf, d = tn.OTHER[0]
    Z = tn.data(nr, nf, d) * [30.0, 0.02, 1.0] + [10.0, -4.0, 0.0]
    X, Y = Z[:nr], Z[nr:]
    outs = []
    for std in (False, True):
        Xs, Ys = tn.standardize(X, Y) if std else (X, Y)
        assert kn.min_gap(np.concatenate([Xs, Ys]), 5) >= kn.GAP
        np.random.seed(6)
        o = kn.test(Xs, Ys, 30, 5)
        np.random.seed(6)
        t = twosample.knn_test(X, Y, n_permutations=30, nearest_k=5, standardize=std)
        assert np.random.random() == o["next"]
        assert same(t, twosample.KnnTest(o["statistic"], o["pvalue"], o["null"], o["real"], o["fake"]))
        outs.append(t)
    assert not same(*outs)                                           # the scales matter


def test_bad_arguments_raise_value_error_and_draw_nothing():
    X, Y = torch.zeros(9, 2, device="cuda"), torch.zeros(8, 2, device="cuda")
    bad = X.clone()
    bad[2, 0] = float("inf")
    np.random.seed(3)
    want = np.random.random()
    calls = [((bad, Y), {}), ((Y, bad * float("nan")), {})]
    calls += [((X, Y), dict(nearest_k=k)) for k in (0, True, 2.0, K_MAX + 1)] + [((X[:4], Y[:3]), dict(nearest_k=7))]
    for fn in (twosample.knn_test, twosample.nn_accuracy_full_sample):
        for args, kw in calls:
            np.random.seed(3)
            with pytest.raises(ValueError):
                fn(*args, **kw)
            assert np.random.random() == want
    t = twosample.knn_test(np.ones((9, 2)), np.ones((7, 2)), n_permutations=5, nearest_k=15)    # all rows equal, k = N - 1
    assert t.statistic == kn.expected_null(9, 7) and (t.null == t.statistic).all() and t.pvalue == 1.0
