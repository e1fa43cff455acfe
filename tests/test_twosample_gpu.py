"""probaforms_amd.metrics.twosample on the GPU (pfm_perm_labels and pfm_perm_form in libpf_metrics.so) against the float64
restatement (tests/twosample_numpy.py) and the committed fixtures (tests/golden/twosample_*.npz).

The labellings are compared byte for byte: they are integer work (Philox, a radix select, a count).  A signed pair sum S is
compared within 1e-12 A, A = sum_ab |s[a] s[b]| G(a, b) taken from the restatement: the project's tolerance for float64 sums
taken in another order, applied to the sum of magnitudes because S itself cancels (tests/test_twosample_host.py measures the
kernel's order against the restatement's at every shape used here, below 1e-14 A).  The shapes: two and three pooled rows, one
tile exactly and one row more, tiles that hold rows of both samples, one feature chunk exactly (d = 16), a second of one feature
(d = 17), a third (d = 33), labelling counts around the block of 16 and the slice of 128, and 35 tiles per side (1200 + 1000
rows: lists of several tiles, many workgroups, two slices).
"""
import functools
import glob
import os
import sys

import numpy as np
import pytest
import torch
from scipy.spatial.distance import cdist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, ROOT)

import twosample_numpy as tn  # noqa: E402
import hygiene  # noqa: E402
import native_libs  # noqa: E402
from probaforms_amd.metrics import _lib, energy as energy_mod, twosample  # noqa: E402

pytestmark = pytest.mark.gpu

native_libs.ensure_built(_lib)

FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "twosample_*.npz")))
KINDS = [("energy", tn.ENERGY), ("gauss", tn.GAUSS)]
BOUND = 1e-12


def fid(p):
    return os.path.basename(p)[10:-4]


def dev(A, dtype=np.float64):
    return torch.from_numpy(np.array(A, dtype=dtype, order="C")).cuda()


def raw_labels(first, reps, N, nr, mask=tn.ALL, seed=tn.SEED, ws=None, pattern="zeros"):
    """pfm_perm_labels through the raw binding on poisoned outputs -> (status, labels tensor [reps, N])"""
    if ws is None:
        ws = hygiene.workspace(_lib.perm_labels_workspace_bytes(reps, N, nr), pattern)
    L = torch.empty((reps, N), dtype=torch.uint8, device="cuda")
    hygiene.poison_outputs(L)
    st = _lib.perm_labels_status(seed, mask, first, reps, N, nr, L, ws)
    torch.cuda.synchronize()
    return st, L


def raw_form(kind, gamma, Z, nr, L, ws=None, pattern="zeros"):
    """pfm_perm_form through the raw binding on poisoned outputs -> (status, S tensor [reps])"""
    reps, (N, d) = len(L), Z.shape
    if ws is None:
        ws = hygiene.workspace(_lib.perm_form_workspace_bytes(N, d, nr, reps), pattern)
    S = torch.empty(reps, dtype=torch.float64, device="cuda")
    hygiene.poison_outputs(S)
    st = _lib.perm_form_status(kind, gamma, dev(Z), nr, dev(L, np.uint8), reps, S, ws)
    torch.cuda.synchronize()
    return st, S


# ---- the labellings ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,nr", tn.LABEL_CASES)
def test_labels_equal_the_restatement(N, nr):
    for mask in tn.MASKS:
        want = tn.labels(tn.SEED, 0, 12, N, nr, mask)              # labellings 0 .. 11
        for reps in (1, 5):
            for first in (0, 7):
                st, L = raw_labels(first, reps, N, nr, mask)
                assert st == 0 and hygiene.poisoned(L) == 0
                got = L.cpu().numpy()
                assert got.tobytes() == want[first:first + reps].tobytes(), (mask, reps, first)
                assert (got.sum(axis=1) == nr).all()
        # labelling 7 made with first_perm = 0 is labelling 0 made with first_perm = 7
        st, a = raw_labels(0, 8, N, nr, mask)
        st2, b = raw_labels(7, 1, N, nr, mask)
        assert st == 0 and st2 == 0 and hygiene.same_bits(a[7:8], b)
        if mask == 0:
            assert (a.cpu().numpy() == tn.observed(N, nr)[None]).all()


def test_labels_depend_on_the_seed_and_on_nothing_else():
    N, nr = 600, 333
    st, a = raw_labels(0, 3, N, nr, seed=1)
    st, b = raw_labels(0, 3, N, nr, seed=1 << 32)                 # the other key word
    st, c = raw_labels(0, 3, N, nr, seed=1)
    assert hygiene.same_bits(a, c) and not hygiene.same_bits(a, b)
    assert a.cpu().numpy().tobytes() == tn.labels(1, 0, 3, N, nr).tobytes()
    assert b.cpu().numpy().tobytes() == tn.labels(1 << 32, 0, 3, N, nr).tobytes()


# ---- the quadratic forms ----------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def labellings(N, nr, reps):
    """the observed labelling and reps - 1 drawn ones (a labelling does not depend on how many are made)"""
    L = np.concatenate([tn.observed(N, nr)[None], tn.labels(tn.SEED, 0, reps - 1, N, nr)]) if reps > 1 else tn.observed(N, nr)[None]
    L.setflags(write=False)
    return L


def check_form(kind, Z, nr, L, gamma):
    st, S = raw_form(kind, gamma, Z, nr, L)
    assert st == 0 and hygiene.poisoned(S) == 0
    want, A = tn.form(Z, L, nr, kind, gamma)
    err = np.abs(S.cpu().numpy() - want)
    print("reps %d d %d: largest |S - S_ref| / A = %.3g" % (len(L), Z.shape[1], (err / A).max()))
    assert (err <= BOUND * A).all()
    return S


@pytest.mark.parametrize("name,kind", KINDS)
@pytest.mark.parametrize("nr,nf", tn.FORM_SHAPES)
def test_form_equals_the_restatement(nr, nf, name, kind):
    for d in tn.FORM_DS:
        Z = tn.data(nr, nf, d)
        all_l = labellings(nr + nf, nr, max(tn.FORM_REPS))
        for reps in tn.FORM_REPS:
            check_form(kind, Z, nr, all_l[:reps], tn.gamma_of(d))


@pytest.mark.parametrize("name,kind", KINDS)
def test_form_many_tiles_and_workgroups(name, kind):
    nr, nf, d, reps = tn.LARGE
    check_form(kind, tn.data(nr, nf, d), nr, labellings(nr + nf, nr, reps), tn.gamma_of(d))


def test_integer_data_is_exact():
    """every distance and weight is an integer and every partial sum is below 2^53: a wrong weight, a missed or doubled tile
    or a diagonal tile weighed twice shows in the last bit"""
    nr, nf, d = tn.INTEGER
    for shape in ((nr, nf), (2 * tn.TILE + 5, tn.TILE + 1)):
        Z = tn.integer_data(*shape)
        L = labellings(sum(shape), shape[0], 17)
        want, A = tn.form(Z, L, shape[0], tn.ENERGY)
        assert A.max() < 2 ** 53 and np.array_equal(want, np.round(want))
        st, S = raw_form(tn.ENERGY, 0.0, Z, shape[0], L)
        assert st == 0 and S.cpu().numpy().tobytes() == want.tobytes()


@pytest.mark.parametrize("name,kind", KINDS)
def test_a_labelling_alone_equals_the_labelling_inside_a_group(name, kind):
    nr, nf, d = tn.OTHER[0]
    Z, L = tn.data(nr, nf, d), labellings(nr + nf, nr, 129)
    st, together = raw_form(kind, 0.3, Z, nr, L)
    st2, again = raw_form(kind, 0.3, Z, nr, L)
    assert st == 0 and st2 == 0 and hygiene.same_bits(together, again)
    for r in (0, 1, 15, 16, 127, 128):
        st, alone = raw_form(kind, 0.3, Z, nr, L[r:r + 1])
        assert st == 0 and hygiene.same_bits(alone, together[r:r + 1]), r
    st, part = raw_form(kind, 0.3, Z, nr, L[100:129])              # and at another place in another call
    assert st == 0 and hygiene.same_bits(part, together[100:129])


@pytest.mark.parametrize("nr,nf,d", tn.OTHER[1:])
def test_results_do_not_depend_on_the_workspace(nr, nf, d):
    N, reps = nr + nf, 17
    Z, L = tn.data(nr, nf, d), labellings(nr + nf, nr, 17)
    PZ, PL = tn.data(nr + 70, nf + 30, d), labellings(N + 100, nr + 70, 19)     # the `replay` primer: more of everything
    fbytes, pbytes = _lib.perm_form_workspace_bytes(N, d, nr, reps), _lib.perm_form_workspace_bytes(N + 100, d, nr + 70, 19)
    lbytes = _lib.perm_labels_workspace_bytes(reps, N, nr)
    for kind in (tn.ENERGY, tn.GAUSS):
        outs = {}
        for pat in hygiene.PATTERNS:
            ws = hygiene.workspace(pbytes if pat == "replay" else fbytes, pat)
            if pat == "replay":
                assert raw_form(kind, 0.2, PZ, nr + 70, PL, ws=ws)[0] == 0
            st, S = raw_form(kind, 0.2, Z, nr, L, ws=ws)
            assert st == 0
            outs[pat] = dict(S=S)
        hygiene.assert_all_written(outs["zeros"], "pfm_perm_form")
        hygiene.assert_pattern_independent(outs, "pfm_perm_form")
    outs = {}
    for pat in hygiene.PATTERNS:
        ws = hygiene.workspace(max(lbytes, _lib.perm_labels_workspace_bytes(19, N + 100, nr + 70)), pat)
        if pat == "replay":
            assert raw_labels(2, 19, N + 100, nr + 70, ws=ws)[0] == 0
        st, got = raw_labels(1, reps, N, nr, ws=ws)
        assert st == 0
        outs[pat] = dict(labels=got)
    hygiene.assert_all_written(outs["zeros"], "pfm_perm_labels")
    hygiene.assert_pattern_independent(outs, "pfm_perm_labels")
    assert outs["zeros"]["labels"].cpu().numpy().tobytes() == tn.labels(tn.SEED, 1, reps, N, nr).tobytes()


def test_workspace_and_argument_statuses():
    nr, nf, d = tn.OTHER[1]
    N, Z, L = nr + nf, tn.data(nr, nf, d), labellings(nr + nf, nr, 5)
    need = _lib.perm_form_workspace_bytes(N, d, nr, 5)
    st, S = raw_form(tn.ENERGY, 0.0, Z, nr, L, ws=torch.empty(need - 1, dtype=torch.uint8, device="cuda"))
    assert st == _lib.PFM_EWORKSPACE and hygiene.poisoned(S) == S.numel()
    st, S = raw_form(2, 0.0, Z, nr, L)
    assert st == _lib.PFM_EUNSUPPORTED and hygiene.poisoned(S) == S.numel()
    st, S = raw_form(tn.GAUSS, 0.0, Z, nr, L)
    assert st == _lib.PFM_EINVAL and hygiene.poisoned(S) == S.numel()
    st, got = raw_labels(0, 5, N, N)
    assert st == _lib.PFM_EINVAL and hygiene.poisoned(got) == got.numel()


# ---- the public calls -------------------------------------------------------------------------------------

def check_result(t, P):
    assert isinstance(t, twosample.TwoSampleTest)
    assert isinstance(t.statistic, np.float64) and isinstance(t.pvalue, np.float64)
    assert isinstance(t.null, np.ndarray) and t.null.dtype == np.float64 and t.null.shape == (P,)
    assert t.pvalue.tobytes() == np.float64((1 + int((t.null >= t.statistic).sum())) / (1 + P)).tobytes()


@pytest.mark.parametrize("path", FIXTURES, ids=fid)
def test_fixtures(path):
    f = np.load(path)
    X, Y, P, std = f["X"], f["Y"], int(f["n_permutations"]), bool(f["standardize"])
    Xs, Ys = tn.standardize(X, Y) if std else (X, Y)
    for name, kind, fn in (("energy", tn.ENERGY, twosample.energy_test), ("mmd", tn.GAUSS, twosample.mmd_test)):
        np.random.seed(int(f["seed"]))
        bound = tn.test(Xs, Ys, P, kind, 1.0 / (2 * float(f["median"]) ** 2))["bound"]       # 1e-12 A / (nr nf)^2
        np.random.seed(int(f["seed"]))
        t = fn(X, Y, n_permutations=P, standardize=std)
        assert np.random.random() == float(f["next"])
        check_result(t, P)
        err = np.abs(np.concatenate([[t.statistic], t.null]) - np.concatenate([[f[name + "_statistic"]], f[name + "_null"]]))
        print("%s: largest difference / bound %.3g" % (name, (err / bound).max()))
        assert (err <= bound).all()
        assert t.pvalue == float(f[name + "_pvalue"])
        np.random.seed(int(f["seed"]))                                   # a seeded call is bitwise reproducible
        u = fn(X, Y, n_permutations=P, standardize=std)
        assert u.statistic.tobytes() == t.statistic.tobytes() and u.null.tobytes() == t.null.tobytes() and u.pvalue == t.pvalue


def test_energy_statistic_is_the_full_sample_energy_distance():
    for nr, nf, d in tn.OTHER:
        Z = tn.data(nr, nf, d)
        X, Y = Z[:nr], Z[nr:]
        E = max(cdist(X, X).mean(), cdist(Y, Y).mean(), cdist(X, Y).mean())
        t = twosample.energy_test(X, Y, n_permutations=3)
        full = energy_mod.energy_distance_full_sample(X, Y, squared=True)
        print("|statistic - D^2| = %.3g, bound %.3g" % (abs(t.statistic - full), 4e-12 * E))
        assert abs(t.statistic - full) <= 4e-12 * E


def test_mmd_statistic_is_pfm_mmds_identity_replicate():
    for nr, nf, d in tn.OTHER:
        Z = tn.data(nr, nf, d)
        X, Y = dev(Z[:nr]), dev(Z[nr:])
        out = torch.empty(2, dtype=torch.float64, device="cuda")
        ws = torch.empty(_lib.mmd_workspace_bytes(nr, nf, d, 1), dtype=torch.uint8, device="cuda")
        _lib.mmd(X, Y, torch.arange(nr, dtype=torch.int32, device="cuda"), torch.arange(nf, dtype=torch.int32, device="cuda"), 1,
                 out[:1], out[1:], ws)
        med, want = out.cpu().numpy()
        assert twosample._median(X, Y) == med
        _, A = tn.form(Z, tn.observed(nr + nf, nr), nr, tn.GAUSS, 1.0 / (2 * med ** 2))
        t = twosample.mmd_test(X, Y, n_permutations=3)
        print("|statistic - pfm_mmd| = %.3g, bound %.3g" % (abs(t.statistic - want), BOUND * A[0] / (nr * nf) ** 2))
        assert abs(t.statistic - want) <= BOUND * A[0] / np.float64((nr * nf) ** 2)


def test_a_sample_against_itself_on_integer_data():
    Z = tn.integer_data(65, 63)
    X = Z[:65]
    t = twosample.energy_test(X, X.copy(), n_permutations=99)
    check_result(t, 99)
    assert t.statistic == 0.0 and not np.signbit(t.statistic) and t.pvalue == 1.0 and (t.null >= 0.0).all()


def test_groups(monkeypatch):
    """n_permutations of 1 and of 300; the latter in several groups, which give the bits of the one group"""
    nr, nf, d = tn.OTHER[0]
    Z = tn.data(nr, nf, d)
    X, Y = Z[:nr], Z[nr:]
    for fn in (twosample.energy_test, twosample.mmd_test):
        np.random.seed(5)
        one = fn(X, Y, n_permutations=1)
        check_result(one, 1)
        np.random.seed(5)
        whole = fn(X, Y, n_permutations=300)
        check_result(whole, 300)
        assert whole.statistic.tobytes() == one.statistic.tobytes() and whole.null[:1].tobytes() == one.null.tobytes()
        calls = []
        real_form = _lib.perm_form

        def counted(*a):
            calls.append(a[5])
            real_form(*a)

        with monkeypatch.context() as m:
            per = nr + nf + _lib.perm_form_workspace_bytes(nr + nf, d, nr, 1)
            m.setattr(twosample, "GROUP_BYTES", 128 * per)
            m.setattr(_lib, "perm_form", counted)
            np.random.seed(5)
            split = fn(X, Y, n_permutations=300)
        assert calls == [128, 128, 45]
        assert split.statistic.tobytes() == whole.statistic.tobytes() and split.null.tobytes() == whole.null.tobytes()
        assert split.pvalue == whole.pvalue


def test_inputs_give_the_same_bits():
    Z = tn.data(200, 150, 2)
    X32, Y32 = torch.from_numpy(Z[:200]).float(), torch.from_numpy(Z[200:]).float()
    X64, Y64 = X32.double(), Y32.double()
    forms = {"numpy": (X64.numpy(), Y64.numpy()), "lists": (X64.numpy().tolist(), Y64.numpy().tolist()),
             "cuda float32": (X32.cuda(), Y32.cuda()), "cuda float64": (X64.cuda(), Y64.cuda()), "mixed": (X64.numpy(), Y32.cuda())}
    for fn in (twosample.energy_test, twosample.mmd_test):
        want = None
        for name, (A, B) in forms.items():
            np.random.seed(4)
            t = fn(A, B, n_permutations=20)
            want = want or t
            assert t.statistic.tobytes() == want.statistic.tobytes() and t.null.tobytes() == want.null.tobytes(), name
            assert t.pvalue == want.pvalue


def test_bandwidth_and_standardize():
    nr, nf, d = tn.OTHER[0]
    Z = tn.data(nr, nf, d) * [3.0, 0.2, 1.0] + [10.0, -4.0, 0.0]
    X, Y = Z[:nr], Z[nr:]
    for std in (False, True):
        Xs, Ys = tn.standardize(X, Y) if std else (X, Y)
        np.random.seed(6)
        o = tn.test(Xs, Ys, 30, tn.GAUSS, 1.0 / (2 * 1.5 ** 2))
        np.random.seed(6)
        t = twosample.mmd_test(X, Y, n_permutations=30, standardize=std, bandwidth=1.5)
        assert np.random.random() == o["next"]
        err = np.abs(np.concatenate([[t.statistic], t.null]) - np.concatenate([[o["statistic"]], o["null"]]))
        assert (err <= o["bound"]).all()
    np.random.seed(6)
    assert twosample.mmd_test(X, Y, n_permutations=30, bandwidth=1.5).null.tobytes() != t.null.tobytes()      # the scales matter


def test_bad_data_raises_value_error():
    X = torch.zeros(9, 2, device="cuda")
    X[2, 0] = float("inf")
    for fn in (twosample.energy_test, twosample.mmd_test):
        with pytest.raises(ValueError):
            fn(X, torch.zeros(8, 2, device="cuda"))
        with pytest.raises(ValueError):
            fn(torch.zeros(8, 2, device="cuda"), X * float("nan"))
    with pytest.raises(ValueError, match="the median pairwise distance is 0"):
        twosample.mmd_test(np.ones((9, 2)), np.ones((7, 2)))
    t = twosample.energy_test(np.ones((9, 2)), np.ones((7, 2)), n_permutations=5)           # all rows equal: D^2 = 0 throughout
    assert t.statistic == 0.0 and t.pvalue == 1.0
