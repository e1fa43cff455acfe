"""pfm_metric1d (pf_metrics1d.hip, pf_scan1d.h) at the edges of its kernels, through the raw binding of _lib, against the raw forms of
the float64 numpy restatement (tests/metrics1d_numpy.py) on the constructed inputs of tests/column_cases.py.
tests/test_column_cases_host.py proves on the host that every constructed input has the property its test here relies on.

The scan (k_scan1d<M>, chunks of 1024 tie groups with carries) and the range (extreme(), passes of 256 groups):
  seams         one column of G = 1, 2, 1023, 1024, 1025, 2048, 2049 tie groups: all-distinct values split 49 : 51 (G >= 2: one
                distinct value cannot give both samples a row), and every value once in either sample; the identity (no empty
                group) and a bootstrap draw (a third of the groups empty) in one launch; all six statistics
  deep          400 + 400 distinct values, draws from pooled ranks [300, 499] and [600, 799] only: the first and the last non-empty
                group are found in the second, third or first pass of extreme(); all six statistics
Histogram (LDS up to 2048 bins, global atomics beyond):
  grid          700 + 650 rows on k / 4096 holding 0 and 1, bins 1, 2, 2047, 2048, 2049, 4096: counts equal np.histogram's, the
                reference's own call (at 4096 bins every value is an edge, at 2048 bins 661 of them)
  single value  one row of each sample, equal (the range is value -+ 0.5; bins 1, 2, 7, 8: inside the middle bin or on edge
                bins / 2) and different
KDE (k_kde, 8 grid points per workgroup), bins 1, 7, 8, 9, 16, 101 on 40 + 300 and 300 + 3 rows: the identity, a draw, a single row
                of the small sample, one pooled value (a constant grid)
Cap           N = 2^20 pooled rows (k_counts strides its 1024 workgroups four times), about 8000 tie groups: the int64
                Cramer-von Mises and AUC sums exactly; N = 2^20 + 1: PFM_EUNSUPPORTED, ValueError, the AUC still answers
KS switch     (10000, 64) and (10001, 64) rows: the public call bitwise on either side of ks_2samp's exact / asymptotic switch
Siblings      (130, 100, 3), 7 replicates, every statistic: each replicate bitwise what it gives in a launch of its own
Statuses      PFM_EINVAL, PFM_EUNSUPPORTED and PFM_EWORKSPACE leave poisoned outputs untouched (the histogram's memset included)

Comparisons.  KS: bitwise ks_raw.  CvM, AUC, histogram: exact integers.  AD: `distinct` exact, the two sums at rtol 1e-12: the
terms are not negative and computed in scipy's operation order, only the order of the sum differs, and G <= 2049 terms give
G 2^-53 < 2.3e-13.  KDE: |got - want| <= 1e-12 max(1, |want|) elementwise: the argument -0.5 dx^2 / h^2 carries three roundings,
3 |m| 2^-53, the sum of at most n positive terms after the max shift (n + c) 2^-53; with n <= 3000 both are under a third of the
bar, and the host test shows the float64 yardstick itself within a tenth of it of the long-double value.
Every output is handed over poisoned and every workspace filled with 0xFF bytes, so an element no workgroup wrote is seen.

Out of scope: linspace_at's zero-step branch.  For a histogram it is reached only over a range so narrow that np.histogram itself
raises "Too many bins for data range", so there is no reference value to hold it to.
"""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import column_cases as cc  # noqa: E402
import hygiene  # noqa: E402
import metrics1d_numpy as m1  # noqa: E402
import native_libs  # noqa: E402
from probaforms_amd.metrics import _lib, _m1d, ks1d  # noqa: E402

pytestmark = pytest.mark.gpu

native_libs.ensure_built(_lib)

KS, CVM, AD, AUC, HIST, KDE = _lib.M1D_KS, _lib.M1D_CVM, _lib.M1D_AD, _lib.M1D_AUC, _lib.M1D_HIST, _lib.M1D_KDE
NAMES = {KS: "KS", CVM: "CvM", AD: "AD", AUC: "AUC", HIST: "HIST", KDE: "KDE"}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def upload(rows):
    """[reps, n] index vectors -> the flat int32 device view [reps * n]"""
    return torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int32).reshape(-1)).cuda()


def bandwidths(c):
    return _m1d.silverman(len(c.X)), _m1d.silverman(len(c.Y))


class Launch:
    """one case on the device: its pooled columns and index vectors, for any number of pfm_metric1d calls"""

    def __init__(self, c):
        self.c = c
        self.p = _m1d.Pooled(_dev(c.X), _dev(c.Y))
        self.ix, self.iy, self.reps = upload(c.ix), upload(c.iy), len(c.ix)
        self.h = bandwidths(c)

    def out(self, metric, bins):
        tail, dtype = _m1d.OUT_SHAPE[metric]
        o = torch.empty((self.reps, self.p.d) + tuple(bins if t is None else t for t in tail), dtype=dtype, device="cuda")
        hygiene.poison_outputs(o)
        return o

    def status(self, metric, bins=1, nbytes=None, out=None):
        """pfm_metric1d on a poisoned output and a 0xFF-filled workspace -> (status, output tensor)"""
        p, reps = self.p, self.reps
        if nbytes is None:
            nbytes = _lib.metric1d_workspace_bytes(metric, p.nr, p.nf, p.d, reps, bins)
        ws = hygiene.workspace(nbytes, "ones")
        out = self.out(metric, bins) if out is None else out
        st = _lib.metric1d_status(metric, p.cols, p.perm, p.gstart, p.ngroups, p.nr, p.nf, self.ix, self.iy, reps, bins, self.h[0],
                                  self.h[1], out, ws)
        torch.cuda.synchronize()
        return st, out

    def ok(self, metric, bins=1, allow_nan=False):
        st, out = self.status(metric, bins)
        assert st == 0
        if not allow_nan:
            hygiene.assert_all_written({NAMES[metric]: out}, "pfm_metric1d[%s] %s" % (NAMES[metric], self.c.name))
        return out


def want(metric, c, bins=1):
    """the restatement's raw form of every (replicate, feature), in the layout of the kernel's output"""
    tail, dtype = _m1d.OUT_SHAPE[metric]
    reps, d = len(c.ix), c.X.shape[1]
    w = np.empty((reps, d) + tuple(bins if t is None else t for t in tail), dtype=np.float64 if dtype == torch.float64 else np.int64)
    h = bandwidths(c)
    for r in range(reps):
        for f in range(d):
            x, y = cc.resampled(c, r, f)
            if metric == KS:
                w[r, f] = m1.ks_raw(x, y)
            elif metric == CVM:
                w[r, f] = m1.cvm_sums(x, y)
            elif metric == AD:
                w[r, f] = m1.ad_sums(x, y)
            elif metric == AUC:
                w[r, f] = m1.auc_u2(x, y)
            elif metric == HIST:
                e = np.histogram(np.concatenate([x, y]), bins)[1]      # the reference's own calls
                w[r, f, 0], w[r, f, 1] = np.histogram(x, e)[0], np.histogram(y, e)[0]
            else:
                z = np.concatenate([x, y])
                grid = np.linspace(z.min(), z.max(), bins)
                w[r, f, 0], w[r, f, 1] = m1.kde_logsum(x, grid, h[0]), m1.kde_logsum(y, grid, h[1])
    return w


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def compare(metric, got, ref, what):
    got = got.cpu().numpy()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if metric == KS:
        assert np.array_equal(bits(got), bits(ref)), "%s KS: %r != %r" % (what, got.ravel()[:4], ref.ravel()[:4])
    elif metric in (CVM, AUC, HIST):
        assert np.array_equal(got.astype(np.int64), ref), "%s %s: %d elements differ, first got %r want %r" % (
            what, NAMES[metric], int((got != ref).sum()), got[got != ref][:4], ref[got != ref][:4])
    elif metric == AD:
        assert np.array_equal(got[..., 2], ref[..., 2]), "%s AD distinct: %r != %r" % (what, got[..., 2], ref[..., 2])
        many = ref[..., 2] > 1                                     # (one distinct value: the sums are 0 / 0 and not compared)
        g, w = got[many][:, :2], ref[many][:, :2]                   # (a sum of terms >= 0; exactly 0 where the samples are the same)
        err = np.abs(g - w)
        print("%s AD: max relative error of the sums %.3g (bar 1e-12)" % (what, (err[w > 0] / w[w > 0]).max(initial=0)))
        assert (w >= 0).all() and (err <= 1e-12 * w).all()
    else:
        err = np.abs(got - ref) / (1e-12 * np.maximum(1.0, np.abs(ref)))
        print("%s KDE: error %.3g of the bar 1e-12 max(1, |want|)" % (what, err.max()))
        assert np.isfinite(ref).all() and (err <= 1.0).all()


def check_all(c, hist_bins=10, kde_bins=16):
    """all six statistics of a case against the restatement"""
    L = Launch(c)
    one_value = any(len(np.unique(np.concatenate(cc.resampled(c, r, f)))) == 1 for r in range(len(c.ix)) for f in range(c.X.shape[1]))
    for metric, bins in ((KS, 1), (CVM, 1), (AD, 1), (AUC, 1), (HIST, hist_bins), (KDE, kde_bins)):
        compare(metric, L.ok(metric, bins, allow_nan=metric == AD and one_value), want(metric, c, bins), c.name)
    return L


# ---- the scan's chunks and extreme()'s passes ------------------------------------------------------------------------------------

@pytest.mark.parametrize("G,dup", cc.SEAMS, ids=["%d-%s" % (G, "dup" if dup else "distinct") for G, dup in cc.SEAMS])
def test_chunk_seams(G, dup):
    c = cc.seam(G, dup)
    L = check_all(c)
    if G == 1:
        ad = L.ok(AD, allow_nan=True).cpu().numpy()
        assert (ad[..., 2] == 1).all()


@pytest.mark.parametrize("window", cc.DEEP_WINDOWS, ids=["%d-%d" % w for w in cc.DEEP_WINDOWS])
def test_first_and_last_group_beyond_the_first_pass(window):
    check_all(cc.deep(window))


# ---- histogram -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bins", cc.HIST_BINS)
def test_histogram_counts_are_np_histograms(bins):
    c = cc.hist_grid()
    out = Launch(c).ok(HIST, bins)
    compare(HIST, out, want(HIST, c, bins), "%s bins %d" % (c.name, bins))
    sums = out.cpu().numpy().astype(np.int64).sum(axis=-1)
    assert (sums[:, 0, 0] == 700).all() and (sums[:, 0, 1] == 650).all()


@pytest.mark.parametrize("bins", cc.ONE_VALUE_BINS)
def test_histogram_of_single_value_replicates(bins):
    c = cc.hist_single()
    out = Launch(c).ok(HIST, bins)
    compare(HIST, out, want(HIST, c, bins), "%s bins %d" % (c.name, bins))
    h = out.cpu().numpy()
    assert h[0, 0, 0, bins // 2] == 700 and h[0, 0, 1, bins // 2] == 650           # equal rows: the middle bin
    assert h[1, 0, 0, 0] == 700 and h[1, 0, 1, bins - 1] == 650                   # different rows: the first and the last bin


# ---- KDE -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nr,nf", cc.KDE_SHAPES)
@pytest.mark.parametrize("bins", cc.KDE_BINS)
def test_kde_logsum_at_the_grid_chunk_edges(bins, nr, nf):
    c = cc.kde(nr, nf)
    out = Launch(c).ok(KDE, bins)
    compare(KDE, out, want(KDE, c, bins), "%s bins %d" % (c.name, bins))
    g = out.cpu().numpy()
    np.testing.assert_allclose(g[3, 0, 0], np.log(nr), rtol=1e-15)                 # the constant grid: every term is exp(0)
    np.testing.assert_allclose(g[3, 0, 1], np.log(nf), rtol=1e-15)


# ---- the cap ---------------------------------------------------------------------------------------------------------------------

def test_cvm_and_auc_sums_are_exact_at_the_cap():
    c = cc.big()
    L = Launch(c)
    assert L.p.nr + L.p.nf == _lib.CVM_MAX_N == cc.CVM_MAX_N
    sums = L.ok(CVM)
    ref = want(CVM, c)
    compare(CVM, sums, ref, c.name)
    compare(AUC, L.ok(AUC), want(AUC, c), c.name)
    compare(KS, L.ok(KS), want(KS, c), c.name)
    # the finished statistic: the sums exceed 2^53, the host's astype(float64) rounds once where the reference rounds as it
    # accumulates, so it is held to rtol 1e-12 and not compared bitwise
    assert (ref > 2 ** 53).all()
    t = _m1d.cvm_statistic(sums.cpu().numpy(), L.p.nr, L.p.nf)
    np.testing.assert_allclose(t[:, 0], [m1.cvm(*cc.resampled(c, r)) for r in range(2)], rtol=1e-12, atol=0)


def test_one_row_above_the_cap():
    c = cc.big(1)
    L = Launch(c)
    assert L.p.nr + L.p.nf == _lib.CVM_MAX_N + 1
    assert _lib.metric1d_workspace_bytes(CVM, L.p.nr, L.p.nf, 1, 2, 1) > 0
    st, out = L.status(CVM)
    assert st == _lib.PFM_EUNSUPPORTED and hygiene.poisoned(out) == out.numel()
    with pytest.raises(ValueError):
        ks1d.cramer_von_mises_1d(c.X, c.Y, n_iters=1)
    compare(AUC, L.ok(AUC), want(AUC, c), c.name)
    np.random.seed(3)
    got = ks1d.REPLICATES["roc_auc_score_1d"](c.X, c.Y, 1)
    np.random.seed(3)
    np.testing.assert_allclose(got, m1.replicates("roc_auc_score_1d", c.X, c.Y, 1), rtol=1e-12, atol=0)


# ---- the KS switch ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nr,nf", cc.KS_SWITCH)
def test_ks_on_either_side_of_the_exact_switch(nr, nf):
    X, Y = cc.ks_switch(nr, nf)
    np.random.seed(cc.KS_SEED)
    ref = m1.replicates("kolmogorov_smirnov_1d", X, Y, cc.KS_ITERS)
    nxt = np.random.random()
    np.random.seed(cc.KS_SEED)
    S = ks1d.REPLICATES["kolmogorov_smirnov_1d"](X, Y, cc.KS_ITERS)
    assert np.random.random() == nxt
    assert np.array_equal(bits(S), bits(ref)), np.abs(S - ref).max()
    np.random.seed(cc.KS_SEED)
    mu, sd = ks1d.kolmogorov_smirnov_1d(X, Y, cc.KS_ITERS)
    assert np.array_equal(bits([mu, sd]), bits(m1.feature_average(ref)))


# ---- siblings --------------------------------------------------------------------------------------------------------------------

def test_replicate_does_not_depend_on_its_siblings():
    c = cc.bootstrap(130, 100, 3, 7, decimals=1)
    L = Launch(c)
    singles = [Launch(cc.alone(c, r)) for r in range(7)]
    for metric, bins in ((KS, 1), (CVM, 1), (AD, 1), (AUC, 1), (HIST, 10), (HIST, 2049), (KDE, 16)):
        out = L.ok(metric, bins)
        compare(metric, out, want(metric, c, bins), c.name)
        for r, one in enumerate(singles):
            assert hygiene.same_bits(one.ok(metric, bins)[0], out[r]), "%s: replicate %d alone differs" % (NAMES[metric], r)


# ---- statuses --------------------------------------------------------------------------------------------------------------------

def test_statuses_leave_the_outputs_alone():
    c = cc.bootstrap(30, 20, 2, 2)
    L = Launch(c)
    p = L.p

    def untouched(out):
        return hygiene.poisoned(out) == out.numel() > 0

    for bad in (-1, 6):                                            # a metric id out of range
        st, out = L.status(bad, 8, nbytes=1 << 20, out=L.out(HIST, 8))
        assert st == _lib.PFM_EINVAL and untouched(out)
        assert _lib.metric1d_workspace_bytes(bad, 30, 20, 2, 2, 8) == 0
    for metric in (HIST, KDE):                                     # bins = 0
        st, out = L.status(metric, 0, nbytes=1 << 20, out=L.out(metric, 8))
        assert st == _lib.PFM_EINVAL and untouched(out)
        assert _lib.metric1d_workspace_bytes(metric, 30, 20, 2, 2, 0) == 0 < _lib.metric1d_workspace_bytes(metric, 30, 20, 2, 2, 1)

    need = _lib.metric1d_workspace_bytes(HIST, 30, 20, 2, 2, 8)    # one byte short: refused before HIST's memset of `out`
    assert need > 16
    st, out = L.status(HIST, 8, nbytes=need - 1)
    assert st == _lib.PFM_EWORKSPACE and untouched(out)
    st, out = L.status(HIST, 8, nbytes=need)
    assert st == 0 and hygiene.poisoned(out) == 0
    compare(HIST, out, want(HIST, c, 8), c.name)

    big = 65536                                                    # one above the largest grid.y
    one = cc.Case("one-row", np.zeros((1, 1)), np.ones((1, 1)), np.zeros((big, 1), np.int32), np.zeros((big, 1), np.int32))
    B = Launch(one)
    for metric in (KS, HIST):
        st, out = B.status(metric, 2, nbytes=1 << 20)
        assert st == _lib.PFM_EINVAL and untouched(out)
        assert _lib.metric1d_workspace_bytes(metric, 1, 1, 1, big, 2) == 0 < _lib.metric1d_workspace_bytes(metric, 1, 1, 1, big - 1, 2)

    # nr = 0: no binding builds such a call, so it is made on the library itself with real pointers
    ws, out = hygiene.workspace(1 << 20, "ones"), L.out(HIST, 8)
    ptr = lambda t: t.data_ptr()
    st = _lib.lib().pfm_metric1d(torch.cuda.current_stream().cuda_stream, HIST, ptr(p.cols), ptr(p.perm), ptr(p.gstart), ptr(p.ngroups),
                                 0, 20, 2, ptr(L.ix), ptr(L.iy), 2, 8, 1.0, 1.0, ptr(out), ptr(ws), ws.numel())
    torch.cuda.synchronize()
    assert st == _lib.PFM_EINVAL and untouched(out)
    assert _lib.metric1d_workspace_bytes(HIST, 0, 20, 2, 2, 8) == 0
