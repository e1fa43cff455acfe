"""pfm_mmd and pfm_boot_moments (pf_metrics.hip) at the edges of their kernels, through the raw bindings of _lib, against float64 /
long-double numpy restatements (tests/metrics_numpy.py, tests/metrics_cases.py).  tests/test_metrics_host.py proves on the host that
every constructed input has the property its test here relies on.

MMD median (k_mmd_hist / k_mmd_scan, a six-digit radix select following two ranks):
  four points   the two middle keys part in digit 0, 1, 2, 3, 4, 5, and never (an exact tie, m * m even): bitwise median
  zeros ladder  rank 1 a diagonal zero, rank 2 a denormal d^2 that leaves the all-zero prefix in digit 5 ... 1, or 2.25 (digit 0)
  dyadic        70 + 62 rows on a 1/4 grid: every d^2 exact, the middle value shared by many pairs, medians bitwise
  mixed call    distinct-point, half-zero-matrix and permuted replicates in one launch, each bitwise what it gives alone
  siblings      130 + 100 rows (ten tiles), 7 replicates: each median bitwise what the replicate gives alone
  seams         (64, 64, 16), (63, 66, 17), (1, 130, 32), (130, 1, 33), (65, 1, 1): the X / Y seam on and off a tile edge, a one-row
                sample on either side, one feature chunk exactly, then + 1, then two exactly, then + 1
Moments (k_mean_partial / k_cov_partial and the finals), mean at rtol 1e-12 / atol 1e-14, covariance within
1e-11 sqrt(C_ii C_jj) of the long-double two-pass value and exactly symmetric:
  parts         samples with different numbers of row parts (2048 | 2049, 4097 | 100, 100 | 4097), and 133122 rows (66 > MAX_PARTS)
  features      d = 2, 3 (PG does not divide 256), 22, 23 (npair 253, 276), 65 (RT 63), 257 (mean chunk loop), 2049 (RT 1)
  rows          n = 2; n = 1 (exact mean, all-NaN covariance)
  offset        samples centred at +1e6 and -1e6: a one-pass covariance errs by 1e-4 on the bar's scale
  siblings      every replicate bitwise what it gives alone
Statuses: PFM_EINVAL, PFM_EUNSUPPORTED and PFM_EWORKSPACE leave poisoned outputs untouched.
Every workspace is handed over filled with 0xFF bytes (NaN), so a read of a part no workgroup wrote is seen.
"""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import hygiene  # noqa: E402
import metrics_cases as mc  # noqa: E402
import metrics_numpy as mn  # noqa: E402
import native_libs  # noqa: E402
from probaforms_amd.metrics import _lib, fd  # noqa: E402

pytestmark = pytest.mark.gpu

native_libs.ensure_built(_lib)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def upload(rows):
    """[reps] index vectors -> the flat int32 device view [reps * n]"""
    return torch.from_numpy(np.ascontiguousarray(np.stack(rows), dtype=np.int32).reshape(-1)).cuda()


def identity(n):
    return [np.arange(n)]


def split(idx):
    return [i[0] for i in idx], [i[1] for i in idx]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def run_mmd(X, Y, ix, iy, nbytes=None):
    """pfm_mmd on poisoned outputs and a NaN-filled workspace -> (status, median tensor, mmd tensor)"""
    reps = len(ix)
    if nbytes is None:
        nbytes = _lib.mmd_workspace_bytes(len(X), len(Y), X.shape[1], reps)
    ws = hygiene.workspace(nbytes, "ones")
    med = torch.empty(reps, dtype=torch.float64, device="cuda")
    out = torch.empty(reps, dtype=torch.float64, device="cuda")
    hygiene.poison_outputs(med, out)
    st = _lib.mmd_status(_dev(X), _dev(Y), upload(ix), upload(iy), reps, med, out, ws)
    torch.cuda.synchronize()
    return st, med, out


def mmd_ok(X, Y, ix, iy):
    st, med, out = run_mmd(X, Y, ix, iy)
    assert st == 0 and hygiene.poisoned(med) == 0
    return med.cpu().numpy(), out.cpu().numpy()


def restated(X, Y, ix, iy):
    want = [mn.mmd_replicate(X[a], Y[b]) for a, b in zip(ix, iy)]
    return np.array([w[0] for w in want]), np.array([w[1] for w in want])


def within_mmd_bar(val, ref):
    """the bar of test_metrics_gpu.py::test_mmd_against_numpy_restatement"""
    ok = ~np.isnan(ref)
    err = np.abs(val[ok] - ref[ok])
    print("mmd: max |got - ref| %.3g (ref %s)" % (err.max(initial=0), np.array2string(ref, precision=6, threshold=8)))
    return bool((err <= 1e-11 + 1e-9 * np.abs(ref[ok])).all() and np.isnan(val[~ok]).all())


# ---- MMD ---------------------------------------------------------------------------------------------------------------------------

FOUR = dict(("digit%d" % k, v) for k, v in mc.PARTING.items())
FOUR["tie"] = mc.TIE


@pytest.mark.parametrize("name", sorted(FOUR))
def test_median_where_the_middle_keys_part(name):
    X, Y = mc.four_points(*FOUR[name])
    ix, iy = identity(2), identity(2)
    med, val = mmd_ok(X, Y, ix, iy)
    wmed, wval = restated(X, Y, ix, iy)
    print("median %r, restated %r" % (med[0], wmed[0]))
    assert np.array_equal(bits(med), bits(wmed))
    assert within_mmd_bar(val, wval)


@pytest.mark.parametrize("digit", sorted(mc.LADDER))
def test_median_with_one_rank_among_the_diagonal_zeros(digit):
    X, Y = mc.ladder(mc.LADDER[digit])
    med, val = mmd_ok(X, Y, identity(1), identity(1))
    want = mn.median_distance(np.concatenate((X, Y)))
    print("median %r, restated %r, mmd %r" % (med[0], want, val[0]))
    assert want > 0 and np.array_equal(bits(med), bits([want]))
    # median^2 underflows for the denormal rungs (gamma is infinite): only that mmd stays a number in its range
    assert np.isfinite(val[0]) and 0.0 <= val[0] <= 2.0


def test_dyadic_medians_are_bitwise():
    X, Y, idx = mc.dyadic()
    ix, iy = split(idx)
    med, val = mmd_ok(X, Y, ix, iy)
    wmed, wval = restated(X, Y, ix, iy)
    assert np.array_equal(bits(med), bits(wmed)), (med, wmed)
    assert within_mmd_bar(val, wval)


def test_mixed_replicates_in_one_call():
    """distinct points, two points twice each (half of the 16 entries are zeros: one middle rank inside them, one outside), and the
    points swapped.  m <= 64: one tile and one workgroup per replicate whatever `reps` is, so mmd is bitwise too."""
    X, Y = mc.four_points(2 ** 10, 0.5)
    rows = [np.array(r) for r in ((0, 1), (0, 0), (1, 1), (1, 0))]
    med, val = mmd_ok(X, Y, rows, rows)
    wmed, wval = restated(X, Y, rows, rows)
    assert np.array_equal(bits(med), bits(wmed)), (med, wmed)
    assert wmed[1] == np.sqrt(1.25) / 2 and (wmed > 0).all()
    for r, row in enumerate(rows):
        m1, v1 = mmd_ok(X, Y, [row], [row])
        assert bits(m1)[0] == bits(med)[r] and bits(v1)[0] == bits(val)[r], (r, m1, med, v1, val)
    assert np.array_equal(np.isnan(val), ~(wmed > 0))              # (a replicate whose median is 0 gives NaN)
    assert within_mmd_bar(val, wval)


def test_mmd_replicate_does_not_depend_on_its_siblings():
    nx, ny, d, reps = 130, 100, 3, 7
    rng = np.random.default_rng(41)
    X, Y = rng.normal(size=(nx, d)), rng.normal(size=(ny, d)) * 1.3 + 0.2
    np.random.seed(41)
    ix, iy = split(mn.boot_indices(nx, ny, reps))
    med, val = mmd_ok(X, Y, ix, iy)
    wmed, wval = restated(X, Y, ix, iy)
    np.testing.assert_allclose(med, wmed, rtol=1e-12, atol=0)
    assert within_mmd_bar(val, wval)
    worst = 0.0
    for r in range(reps):
        m1, v1 = mmd_ok(X, Y, [ix[r]], [iy[r]])
        assert bits(m1)[0] == bits(med)[r]                         # the select is exact: integer counts, order-free
        # the number of workgroups per replicate depends on `reps`, and with it the order of the RBF partial sums: mmd may
        # differ in its last bits, and is held to the bar against the restatement instead
        worst = max(worst, abs(v1[0] - val[r]))
        assert within_mmd_bar(v1, wval[r:r + 1])
    print("mmd alone against mmd among %d replicates: max |difference| %.3g" % (reps, worst))


@pytest.mark.parametrize("nx,ny,d", [(64, 64, 16), (63, 66, 17), (1, 130, 32), (130, 1, 33), (65, 1, 1)])
def test_mmd_seam_and_chunk_shapes(nx, ny, d):
    rng = np.random.default_rng(nx * 1000 + ny * 10 + d)
    X, Y = rng.normal(size=(nx, d)), rng.normal(size=(ny, d)) * 1.3 + 0.2
    np.random.seed(17)
    ix, iy = split(mn.boot_indices(nx, ny, 2))
    med, val = mmd_ok(X, Y, ix, iy)
    wmed, wval = restated(X, Y, ix, iy)
    print("median: max relative difference %.3g" % np.max(np.abs(med - wmed) / wmed))
    np.testing.assert_allclose(med, wmed, rtol=1e-12, atol=0)
    assert (wmed > 0).all() and within_mmd_bar(val, wval)


def test_mmd_statuses_leave_the_outputs_alone():
    rng = np.random.default_rng(5)
    nx, ny, d, reps = 40, 30, 3, 3
    X, Y = rng.normal(size=(nx, d)), rng.normal(size=(ny, d))
    np.random.seed(5)
    ix, iy = split(mn.boot_indices(nx, ny, reps))
    need = _lib.mmd_workspace_bytes(nx, ny, d, reps)
    assert need > 16
    st, med, out = run_mmd(X, Y, ix, iy, need - 1)
    assert st == _lib.PFM_EWORKSPACE and hygiene.poisoned(med) == reps == hygiene.poisoned(out)
    st, med, out = run_mmd(X, Y, ix, iy, need)
    assert st == 0 and hygiene.poisoned(med) == 0 == hygiene.poisoned(out)
    wmed, wval = restated(X, Y, ix, iy)
    np.testing.assert_allclose(med.cpu().numpy(), wmed, rtol=1e-12, atol=0)
    assert within_mmd_bar(out.cpu().numpy(), wval)

    big = 65536                                                   # one above the largest grid.y
    one = np.zeros((1, 1))
    st, med, out = run_mmd(one, one + 1.0, [np.zeros(1)] * big, [np.zeros(1)] * big, 1 << 20)
    assert st == _lib.PFM_EINVAL and hygiene.poisoned(med) == big == hygiene.poisoned(out)
    assert _lib.mmd_workspace_bytes(1, 1, 1, big) == 0 and _lib.mmd_workspace_bytes(1, 1, 1, big - 1) > 0
    assert _lib.mmd_workspace_bytes(0, ny, d, reps) == 0


# ---- moments -----------------------------------------------------------------------------------------------------------------------

def run_moments(X, Y, ix, iy, nbytes=None):
    """pfm_boot_moments on poisoned outputs and a NaN-filled workspace -> (status, mean tensor, cov tensor)"""
    reps, d = len(ix), X.shape[1]
    if nbytes is None:
        nbytes = _lib.moments_workspace_bytes(len(X), len(Y), d, reps)
    ws = hygiene.workspace(nbytes, "ones")
    mean = torch.empty((reps, 2, d), dtype=torch.float64, device="cuda")
    cov = torch.empty((reps, 2, d, d), dtype=torch.float64, device="cuda")
    hygiene.poison_outputs(mean, cov)
    st = _lib.boot_moments_status(_dev(X), _dev(Y), upload(ix), upload(iy), reps, mean, cov, ws)
    torch.cuda.synchronize()
    return st, mean, cov


def check_moments(X, Y, ix, iy, what):
    """every replicate's two means and covariances against moments_longdouble.  Mean: rtol 1e-12, atol 1e-14 (the bar of
    test_metrics_gpu.py::test_fd_moments_against_numpy).  Covariance: |got - ref| <= 1e-11 sqrt(C_ii C_jj), that test's
    rtol = 1e-11 on the scale of the two variances so that a near-zero off-diagonal needs no atol, and cov == cov.T exactly."""
    st, mean, cov = run_moments(X, Y, ix, iy)
    assert st == 0
    mean, cov = mean.cpu().numpy(), cov.cpu().numpy()
    worst_m = worst_c = 0.0
    for r in range(len(ix)):
        for s, B in enumerate((X[ix[r]], Y[iy[r]])):
            wm, wc = mc.moments_longdouble(B)
            if len(B) == 1:                                        # np.cov of one row: 0 / 0 everywhere
                assert np.array_equal(mean[r, s], B[0]) and np.isnan(cov[r, s]).all()
                continue
            em = np.abs(mean[r, s] - wm) / (1e-12 * np.abs(wm) + 1e-14)
            sd = np.sqrt(np.diag(wc))
            scale = sd[:, None] * sd[None, :]                      # (0 where the draw repeats one row: the bar is then 0)
            err = np.abs(cov[r, s] - wc)
            assert (err <= 1e-11 * scale).all(), "replicate %d sample %d: %r / sqrt(C_ii C_jj)" % (
                r, s, float((err[scale > 0] / scale[scale > 0]).max()))
            worst_m = max(worst_m, float(em.max()))
            worst_c = max(worst_c, float((err[scale > 0] / scale[scale > 0]).max(initial=0)))
            assert np.array_equal(cov[r, s], cov[r, s].T), "replicate %d sample %d: cov is not symmetric" % (r, s)
    print("%s: mean error %.3g of its bar, covariance error %.3g / sqrt(C_ii C_jj) (bar 1e-11)" % (what, worst_m, worst_c))
    assert worst_m <= 1.0 and worst_c <= 1e-11
    return mean, cov


def moments_case(nr, nf, d, reps, seed=0, shift=(3.0, 0.0)):
    rng = np.random.default_rng(nr * 31 + nf * 7 + d + seed)
    X = rng.normal(size=(nr, d)) * rng.uniform(0.5, 2.0, d) + shift[0]
    Y = rng.normal(size=(nf, d)) * 0.7 + shift[1]
    np.random.seed(nr + d + seed)
    ix, iy = split(mn.boot_indices(nr, nf, reps))
    return X, Y, ix, iy


@pytest.mark.parametrize("nr,nf,d,reps", [
    (2048, 2049, 2, 2),        # one part | two parts: the real sample's workgroup p = 1 returns early
    (4097, 100, 3, 2),         # three parts | one
    (100, 4097, 3, 2),         # one | three
    (133122, 10, 1, 1),        # ceil(n / 2048) = 66 > MAX_PARTS: 64 parts of 2080 or 2081 rows
])
def test_moments_with_unequal_row_parts(nr, nf, d, reps):
    check_moments(*moments_case(nr, nf, d, reps), what="parts (%d, %d, %d)" % (nr, nf, d))


@pytest.mark.parametrize("nr,nf,d", [
    (50, 37, 2), (50, 37, 3),      # npair = 3, 6: PG does not divide 256, the last threads idle
    (50, 37, 22), (50, 37, 23),    # npair = 253 (one pair group, one lane), 276 (two groups)
    (70, 37, 65),                  # RT = 63: 70 rows are two row tiles
    (20, 9, 257),                  # the mean kernel loops its 256-feature chunk; n < d: singular covariance
    (5, 3, 2049),                  # RT = 1
])
def test_moments_feature_geometry(nr, nf, d):
    check_moments(*moments_case(nr, nf, d, 2), what="features (%d, %d, %d)" % (nr, nf, d))


@pytest.mark.parametrize("nr,nf", [(2, 3), (1, 4), (4, 1)])
def test_moments_of_the_smallest_samples(nr, nf):
    X, Y, ix, iy = moments_case(nr, nf, 3, 2)
    mean, cov = check_moments(X, Y, ix, iy, what="rows (%d, %d)" % (nr, nf))
    assert np.isfinite(mean).all()
    assert np.isfinite(cov[:, 0]).all() == (nr > 1) and np.isfinite(cov[:, 1]).all() == (nf > 1)


@pytest.mark.parametrize("n,d", [(5000, 16), (300, 100)])
def test_moments_far_from_the_origin(n, d):
    """X = N(0, 1) + 1e6, Y = 0.7 N(0, 1) - 1e6: sum x^2 - n mean^2 loses 1e12 * 2^-53 ~ 1e-4 of a variance of 1; the two-pass
    centred products lose nothing (x - mean is exact here)"""
    rng = np.random.default_rng(n + d)
    X = rng.normal(size=(n, d)) + 1e6
    Y = rng.normal(size=(n, d)) * 0.7 - 1e6
    np.random.seed(n)
    ix, iy = split(mn.boot_indices(n, n, 2))
    check_moments(X, Y, ix, iy, what="offset 1e6 (%d, %d)" % (n, d))


def test_moments_replicate_does_not_depend_on_its_siblings():
    X, Y, ix, iy = moments_case(4097, 100, 3, 5, seed=1)
    mean, cov = check_moments(X, Y, ix, iy, what="siblings")
    for r in range(5):             # the grid is (parts, 2 * reps) and no part reads another job's: the same bits alone
        st, m1, c1 = run_moments(X, Y, [ix[r]], [iy[r]])
        assert st == 0
        assert np.array_equal(bits(m1.cpu().numpy()[0]), bits(mean[r])) and np.array_equal(bits(c1.cpu().numpy()[0]), bits(cov[r]))


def test_moments_statuses_leave_the_outputs_alone():
    def untouched(mean, cov):
        return hygiene.poisoned(mean) == mean.numel() and hygiene.poisoned(cov) == cov.numel()

    X, Y, ix, iy = moments_case(60, 50, 4, 3)
    need = _lib.moments_workspace_bytes(60, 50, 4, 3)
    assert need > 16
    st, mean, cov = run_moments(X, Y, ix, iy, need - 1)
    assert st == _lib.PFM_EWORKSPACE and untouched(mean, cov)
    st, mean, cov = run_moments(X, Y, ix, iy, need)
    assert st == 0 and hygiene.poisoned(mean) == 0 == hygiene.poisoned(cov)

    d = _lib.MOMENTS_MAX_D + 1                                     # one centred row no longer fits the LDS row tile
    assert _lib.moments_workspace_bytes(2, 2, d, 1) == 0 and _lib.moments_workspace_bytes(2, 2, d - 1, 1) > 0
    wide = np.zeros((2, d))
    st, mean, cov = run_moments(wide, wide, identity(2), identity(2), 1 << 20)
    assert st == _lib.PFM_EUNSUPPORTED and untouched(mean, cov)
    del mean, cov

    big = 32768                                                    # 2 * reps jobs: one above the largest grid.y
    one = np.ones((1, 1))
    assert _lib.moments_workspace_bytes(1, 1, 1, big) == 0 and _lib.moments_workspace_bytes(1, 1, 1, big - 1) > 0
    st, mean, cov = run_moments(one, one, [np.zeros(1)] * big, [np.zeros(1)] * big, 1 << 20)
    assert st == _lib.PFM_EINVAL and untouched(mean, cov)


def test_fd_moments_of_a_sample_against_itself_use_the_drawn_indices():
    """frechet_distance(X, X) differs from 0 by bootstrap noise only, which checks no kernel; what the public path owes is the
    moments of exactly the rows the reference's draws name, for the real and the fake side separately"""
    rng = np.random.default_rng(9)
    X = rng.normal(size=(333, 5)) + 1.0
    np.random.seed(21)
    mean, cov = fd.moments(X, X.copy(), 3)
    nxt = np.random.random()
    np.random.seed(21)
    ix, iy = split(mn.boot_indices(len(X), len(X), 3))
    assert np.random.random() == nxt
    assert not np.array_equal(ix[0], iy[0])
    st, m2, c2 = run_moments(X, X.copy(), ix, iy)
    assert st == 0
    assert np.array_equal(bits(mean), bits(m2.cpu().numpy())) and np.array_equal(bits(cov), bits(c2.cpu().numpy()))
