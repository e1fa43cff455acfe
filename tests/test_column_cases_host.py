"""tests/column_cases.py without a GPU: every constructed input has the property that tests/test_metrics1d_edges_gpu.py and
tests/test_wasserstein_edges_gpu.py rely on, from numpy alone; and the raw forms of tests/metrics1d_numpy.py are what its finished
statistics are made of."""
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import column_cases as cc  # noqa: E402
import metrics1d_numpy as m1  # noqa: E402
import wasserstein_numpy as wn  # noqa: E402
from probaforms_amd.metrics import _lib, _m1d  # noqa: E402

# kde_logsum_longdouble is a yardstick only where long double is wider than float64 (x87: 64-bit significand)
assert np.finfo(np.longdouble).eps <= 2.0 ** -63, "np.longdouble is no wider than float64 on this platform"


def test_constants_are_the_kernels():
    def text(name):
        return open(os.path.join(ROOT, "probaforms_amd", "metrics", "csrc", name)).read()
    scan, m1d, wass = text("pf_scan1d.h"), text("pf_metrics1d.hip"), text("pf_wasserstein.hip")
    assert '#include "pf_common.h"' in scan and "constexpr int NT = 256;" in text("pf_common.h")
    assert "constexpr int IPT = 4;" in scan and cc.CHUNK == 256 * 4 and cc.PASS == 256
    assert "constexpr int GP = %d;" % cc.GP in m1d and "constexpr int HIST_LDS = %d;" % cc.HIST_LDS in m1d
    assert "CVM_MAX_N = int64_t(1) << 20;" in m1d and cc.CVM_MAX_N == 1 << 20 == _lib.CVM_MAX_N
    assert "constexpr int WP_LDS = %d;" % cc.WP_LDS in wass and "TILE = WP_LDS / 2" in wass and cc.TILE == cc.WP_LDS // 2
    assert _m1d.KS_EXACT_MAX_N == 10000


# ---- chunk seams -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("G,dup", cc.SEAMS)
def test_seam_cases_have_G_groups(G, dup):
    c = cc.seam(G, dup)
    nr, nf = len(c.X), len(c.Y)
    assert cc.pooled_groups(c) == G and c.X.shape[1] == 1 and len(c.ix) == 2
    if dup:
        assert nr == nf == G and np.array_equal(np.sort(c.X[:, 0]), np.sort(c.Y[:, 0]))
    else:
        assert nr + nf == G and nr >= 1 and nf >= 1 and (G < 100 or abs(nr / G - 0.49) < 0.001)
    a, b = cc.group_counts(c, 0)                                   # the identity: every group drawn, as often as it has rows
    assert ((a + b) == (2 if dup else 1)).all() and (not dup or ((a == 1) & (b == 1)).all())
    a, b = cc.group_counts(c, 1)
    assert a.sum() == nr and b.sum() == nf
    if G >= 1023:                                                  # the draw leaves groups empty: exp(-1) of them, exp(-2) with dup
        empty = ((a + b) == 0).mean()
        print("G %d: %.3f of the groups are empty in the draw" % (G, empty))
        assert (0.10 < empty < 0.17) if dup else (0.33 < empty < 0.41)


# ---- deep first and last group ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("window,first_pass,last_pass", [(cc.DEEP_WINDOWS[0], 1, 1), (cc.DEEP_WINDOWS[1], 2, 0)])
def test_deep_cases_end_in_the_named_pass_of_extreme(window, first_pass, last_pass):
    c = cc.deep(window)
    assert len(c.X) == len(c.Y) == 400 and cc.pooled_groups(c) == 800
    for r in range(len(c.ix)):
        first, last, G = cc.nonempty_span(c, r)
        assert window[0] <= first and last <= window[1] and G == 800
        # extreme(first) looks at groups [256 k, 256 k + 256) in pass k, extreme(last) at [G - 256 k - 256, G - 256 k)
        assert first // cc.PASS == first_pass and (G - 1 - last) // cc.PASS == last_pass
        if window == cc.DEEP_WINDOWS[0]:
            assert first >= 256 and G - 1 - last >= 256
        x, y = cc.resampled(c, r)
        assert len(np.unique(x)) > 20 and len(np.unique(y)) > 20   # (both samples are drawn from many rows of the window)


# ---- histogram -------------------------------------------------------------------------------------------------------------------

def np_hist(x, y, bins):
    """the reference's own call: np.histogram of either sample in the bins of np.histogram of the pooled one"""
    e = np.histogram(np.concatenate([x, y]), bins)[1]
    return np.histogram(x, e)[0], np.histogram(y, e)[0]


def test_hist_grid_lies_on_edges_and_the_restatement_is_np_histogram():
    c = cc.hist_grid()
    assert (len(c.X), len(c.Y)) == (700, 650)
    Z = np.concatenate([c.X[:, 0], c.Y[:, 0]])
    assert np.array_equal(Z * 4096, np.round(Z * 4096)) and Z.min() == 0.0 and Z.max() == 1.0
    assert 0.0 in c.X and 1.0 in c.Y
    assert np.array_equal(c.ix[0], np.arange(700)) and np.array_equal(c.iy[0], np.arange(650))
    # with the range [0, 1] the edges at 4096 bins are the grid itself, at 2048 bins its even points
    assert cc.on_edge(Z, 4096) == 1350 and cc.on_edge(Z, 2048) == 661 == int((np.round(Z * 4096) % 2 == 0).sum())
    assert cc.on_edge(Z, 2048) > 0 and cc.on_edge(Z, 4096) > 0
    for bins in cc.HIST_BINS:
        for r in range(2):
            x, y = cc.resampled(c, r)
            hx, hy = m1.hist_counts(x, y, bins)
            wx, wy = np_hist(x, y, bins)
            assert np.array_equal(hx, wx) and np.array_equal(hy, wy), (bins, r)
            assert hx.sum() == 700 and hy.sum() == 650


@pytest.mark.parametrize("bins", cc.ONE_VALUE_BINS)
def test_hist_single_value_replicates(bins):
    c = cc.hist_single()
    x, y = cc.resampled(c, 0)
    assert len(np.unique(np.concatenate([x, y]))) == 1 and x[0] == 0.5
    hx, hy = m1.hist_counts(x, y, bins)
    wx, wy = np_hist(x, y, bins)
    assert np.array_equal(hx, wx) and np.array_equal(hy, wy)
    e = np.histogram(np.concatenate([x, y]), bins)[1]
    assert e[0] == 0.0 and e[-1] == 1.0                            # the range value -+ 0.5
    assert (0.5 in e) == (bins % 2 == 0)                          # even: on edge bins / 2; odd: inside the middle bin
    assert hx[bins // 2] == 700 and hy[bins // 2] == 650
    x, y = cc.resampled(c, 1)
    assert len(np.unique(x)) == 1 == len(np.unique(y)) and x[0] != y[0]
    hx, hy = m1.hist_counts(x, y, bins)
    wx, wy = np_hist(x, y, bins)
    assert np.array_equal(hx, wx) and np.array_equal(hy, wy)
    assert hx[0] == 700 and hy[-1] == 650


# ---- KDE -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nr,nf", cc.KDE_SHAPES)
def test_kde_cases_and_the_margin_of_the_float64_restatement(nr, nf):
    """the GPU test's bar is 1e-12 max(1, |want|); kde_logsum in float64 is within a tenth of it of the long-double value"""
    c = cc.kde(nr, nf)
    assert (len(c.X), len(c.Y)) == (nr, nf) and max(nr, nf) <= 3000 and min(nr, nf) < 256
    small = 0 if nr < nf else 1
    assert len(np.unique(cc.resampled(c, 2)[small])) == 1 and len(np.unique(cc.resampled(c, 2)[1 - small])) > 100
    x, y = cc.resampled(c, 3)
    assert len(np.unique(np.concatenate([x, y]))) == 1
    worst = 0.0
    for bins in cc.KDE_BINS:
        for r in range(len(c.ix)):
            x, y = cc.resampled(c, r)
            z = np.concatenate([x, y])
            grid = np.linspace(z.min(), z.max(), bins)
            assert len(grid) == bins and (r != 3 or (grid == x[0]).all())
            for s, n in ((x, nr), (y, nf)):
                h = _m1d.silverman(n)
                got, ref = m1.kde_logsum(s, grid, h), cc.kde_logsum_longdouble(s, grid, h)
                assert ref.dtype == np.longdouble and np.isfinite(got).all()
                err = np.abs(got - ref) / (1e-12 * np.maximum(1.0, np.abs(ref)))
                worst = max(worst, float(err.max()))
    print("float64 kde_logsum against long double: %.3g of the bar" % worst)
    assert worst <= 0.1


def test_kde_constant_grid_gives_log_n():
    c = cc.kde(40, 300)
    x, y = cc.resampled(c, 3)
    np.testing.assert_array_equal(m1.kde_logsum(x, np.full(7, x[0]), 0.5), np.log(40.0))
    np.testing.assert_array_equal(m1.kde_logsum(y, np.full(7, x[0]), 0.5), np.log(300.0))


# ---- the cap ---------------------------------------------------------------------------------------------------------------------

def test_big_case_sits_on_the_cap():
    c = cc.big()
    assert len(c.X) == len(c.Y) == 1 << 19 and len(c.X) + len(c.Y) == cc.CVM_MAX_N
    assert len(c.X) + len(c.Y) > 1024 * 256                        # more rows than k_counts' 1024 workgroups of 256 threads
    G = cc.pooled_groups(c)
    print("groups: %d" % G)
    assert 6000 < G < 10000
    assert np.array_equal(c.ix[0], np.arange(1 << 19)) and not np.array_equal(c.ix[1], c.ix[0])
    # the rows past the first 262144 carry draws in both samples and both replicates
    assert (c.ix[1] >= 262144).sum() > 200000 and (c.iy[1] >= 262144).sum() > 200000
    for r in range(2):
        sx, sy = m1.cvm_sums(*cc.resampled(c, r))
        assert 2 ** 53 < sx < 2 ** 63 and 2 ** 53 < sy < 2 ** 63   # past float64's integers, inside int64
    one = cc.big(1)
    assert len(one.X) + len(one.Y) == cc.CVM_MAX_N + 1


# ---- the KS switch ---------------------------------------------------------------------------------------------------------------

def test_ks_switch_cases_tell_the_two_expressions_apart():
    """at 10001 rows the raw difference is returned as it is; the exact method's h / lcm would differ from it in some replicate"""
    seen = {}
    for nr, nf in cc.KS_SWITCH:
        X, Y = cc.ks_switch(nr, nf)
        assert X.shape == (nr, 3) and Y.shape == (nf, 3)
        np.random.seed(cc.KS_SEED)
        differ = 0
        for r in range(cc.KS_ITERS):
            ix, iy = np.random.randint(0, nr, size=nr), np.random.randint(0, nf, size=nf)
            for f in range(3):
                d = m1.ks_raw(X[ix, f], Y[iy, f])
                lcm = (nr // math.gcd(nr, nf)) * nf
                exact = int(np.round(d * lcm)) * 1.0 / lcm
                differ += exact != d
                assert m1.ks(X[ix, f], Y[iy, f]) == (exact if nr <= 10000 else d)
        seen[nr] = differ
    print("replicates whose h / lcm differs from the raw difference: %r" % seen)
    assert seen[10000] > 0 and seen[10001] > 0


# ---- raw forms -------------------------------------------------------------------------------------------------------------------

def test_raw_forms_are_what_the_finished_statistics_use():
    c = cc.bootstrap(130, 100, 3, 7, decimals=1)
    for r in range(7):
        for f in range(3):
            x, y = cc.resampled(c, r, f)
            assert m1.auc(x, y) == abs((m1.auc_u2(x, y) / 2.0) / (130 * 100) - 0.5) + 0.5
            sr, sf, distinct = m1.ad_sums(x, y)
            assert distinct == len(np.unique(np.concatenate([x, y]))) and sr > 0 and sf > 0
            # U counted pair by pair
            assert m1.auc_u2(x, y) == int(2 * (y[:, None] > x[None, :]).sum() + (y[:, None] == x[None, :]).sum())
            z = np.unique(np.concatenate([x, y]))
            d = (np.searchsorted(np.sort(x), z, side="right") / 130 - np.searchsorted(np.sort(y), z, side="right") / 100)
            assert m1.ks_raw(x, y) == max(d.max(), -d.min())
    assert m1.ad_sums(np.ones(3), np.ones(4))[2] == 1


# ---- Wasserstein tables and merges -----------------------------------------------------------------------------------------------

def table_sizes(c, r):
    """(Mr, Mf, bound): the non-empty real and fake groups of replicate r, and the kernel's bound min(G, nr) + min(G, nf)"""
    a, b = cc.group_counts(c, r)
    G = len(a)
    return int((a > 0).sum()), int((b > 0).sum()), min(G, len(c.X)) + min(G, len(c.Y))


@pytest.mark.parametrize("nr,nf", cc.FULL_TABLE)
def test_full_table_cases(nr, nf):
    c = cc.full_table(nr, nf)
    assert cc.pooled_groups(c) == nr + nf <= 3001
    Mr, Mf, bound = table_sizes(c, 0)
    assert (Mr, Mf) == (nr, nf) and bound == nr + nf               # exactly full: cap = WP_LDS in LDS, cap = N in the workspace
    assert (bound <= cc.WP_LDS) == (nf == 1024)
    Mr, Mf, _ = table_sizes(c, 1)
    assert Mr < nr and Mf < nf


@pytest.mark.parametrize("G", cc.TIED_G)
def test_tied_cases(G):
    c = cc.tied(G)
    assert len(c.X) == len(c.Y) == 1500 and len(c.X) + len(c.Y) > cc.WP_LDS
    assert cc.pooled_groups(c) == G
    assert len(np.unique(c.X)) == G == len(np.unique(c.Y))         # both samples hit every value
    Mr, Mf, bound = table_sizes(c, 0)
    assert (Mr, Mf) == (G, G) and bound == 2 * G and (bound <= cc.WP_LDS) == (G == 1024)
    assert (G - 1) % cc.CHUNK == (cc.CHUNK - 1 if G == 1024 else 0)   # k_w1's last counted group: the chunk's last, the next one's first


@pytest.mark.parametrize("apart", [False, True], ids=["mixed", "apart"])
@pytest.mark.parametrize("Mr,Mf", cc.HANDOFF)
def test_handoff_cases(Mr, Mf, apart):
    c = cc.handoff(Mr, Mf, apart)
    assert len(c.X) == len(c.Y) == 1500 and cc.pooled_groups(c) == 3000
    assert (c.X.max() < c.Y.min()) == apart
    for r in range(2):
        a, b = cc.group_counts(c, r)
        assert table_sizes(c, r) == (Mr, Mf, 3000) and a.sum() == 1500 == b.sum()
        if r == 0:                                                 # evenly: the draw counts differ by at most one
            assert a[a > 0].max() - a[a > 0].min() <= 1 and b[b > 0].max() - b[b > 0].min() <= 1
        else:                                                      # all on one row
            assert sorted(a[a > 0])[:-1] == [1] * (Mr - 1) and a.max() == 1500 - Mr + 1
            assert sorted(b[b > 0])[:-1] == [1] * (Mf - 1) and b.max() == 1500 - Mf + 1
    assert [m + f for m, f in cc.HANDOFF] == [2, 1024, 1025, 2048, 1501, 1501, 3000]


def test_coprime_case():
    c = cc.coprime()
    assert (len(c.X), len(c.Y)) == (1499, 1501) and math.gcd(1499, 1501) == 1 and cc.pooled_groups(c) == 3000
    for r in range(2):
        Mr, Mf, bound = table_sizes(c, r)
        assert bound == 3000 and Mr + Mf > cc.TILE


def test_every_wasserstein_case_stays_inside_the_bars_derivation():
    """tests/test_wasserstein_gpu.py derives rtol 1e-12 for N up to 3002"""
    cases = [cc.full_table(*s) for s in cc.FULL_TABLE] + [cc.tied(G) for G in cc.TIED_G] + [cc.coprime(), cc.handoff(1, 1, False),
                                                                                            cc.bootstrap(1000, 1500, 2, 3)]
    assert all(len(c.X) + len(c.Y) <= 3001 for c in cases)
    x, y = cc.resampled(cases[0], 1)
    np.testing.assert_allclose(wn.wp_pow(x, y, 1), wn.w1(x, y), rtol=1e-12)
