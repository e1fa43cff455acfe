"""Constructed inputs for the edges of the per-column bootstrap kernels (pf_metrics1d.hip, pf_wasserstein.hip, pf_scan1d.h), shared by
tests/test_column_cases_host.py (which proves from numpy alone that every input has the property it is named for) and
tests/test_metrics1d_edges_gpu.py / tests/test_wasserstein_edges_gpu.py (which rely on that property).  Test helper, not product code.

Every case is data plus explicit int32 index vectors: Case(name, X [nr, d], Y [nf, d], ix [reps, nr], iy [reps, nf]).  Replicate r of
column f is the pair of resampled columns X[ix[r], f], Y[iy[r], f].  The generators are private RandomStates: no case touches numpy's
global stream.  What the kernels' constants are (the tests of the properties restate them):"""
import collections

import numpy as np

CHUNK = 1024            # pf_scan1d.h NT * IPT: tie groups per chunk of the block scan
PASS = 256              # pf_metrics1d.hip extreme(): groups per pass (NT)
HIST_LDS = 2048         # pf_metrics1d.hip: bins counted in LDS
GP = 8                  # pf_metrics1d.hip: KDE grid points per workgroup
WP_LDS = 2048           # pf_wasserstein.hip: table entries held in LDS
TILE = WP_LDS // 2      # pf_wasserstein.hip: merge steps per tile of the workspace path
CVM_MAX_N = 1 << 20     # pf_metrics1d.hip / _lib.CVM_MAX_N

Case = collections.namedtuple("Case", "name X Y ix iy")


def _case(name, X, Y, ix, iy):
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    if X.ndim == 1:
        X, Y = X[:, None], Y[:, None]
    ix, iy = np.stack(ix).astype(np.int32), np.stack(iy).astype(np.int32)
    assert ix.shape[1] == len(X) and iy.shape[1] == len(Y) and len(ix) == len(iy)
    assert 0 <= ix.min() and ix.max() < len(X) and 0 <= iy.min() and iy.max() < len(Y)
    for a in (X, Y, ix, iy):
        a.setflags(write=False)
    return Case(name, X, Y, ix, iy)


def draw(rng, nr, nf):
    """one bootstrap replicate's index vectors"""
    return rng.randint(0, nr, size=nr), rng.randint(0, nf, size=nf)


def resampled(c, r, f=0):
    """replicate r's two resampled columns of feature f"""
    return c.X[c.ix[r], f], c.Y[c.iy[r], f]


def pooled_groups(c, f=0):
    """the number of tie groups of the pooled original column"""
    return len(np.unique(np.concatenate([c.X[:, f], c.Y[:, f]])))


def group_counts(c, r, f=0):
    """(real, fake) draw counts of replicate r per tie group of the pooled original column, in value order"""
    vals, inv = np.unique(np.concatenate([c.X[:, f], c.Y[:, f]]), return_inverse=True)
    nr = len(c.X)
    a = np.bincount(inv[:nr][c.ix[r]], minlength=len(vals))
    b = np.bincount(inv[nr:][c.iy[r]], minlength=len(vals))
    return a, b


# ---- the scan's chunk seam -------------------------------------------------------------------------------------------------------

SEAM_G = (1, 2, 1023, 1024, 1025, 2048, 2049)
# (G, dup).  One distinct value cannot give both samples a row: G = 1 exists only with the value in both samples
SEAMS = tuple((G, dup) for dup in (False, True) for G in SEAM_G if dup or G > 1)


def seam(G, dup):
    """one column of G tie groups.  dup = False: G distinct values split nr : nf near 49 : 51 (G >= 2: each sample needs a row).
    dup = True: every value once in either sample (nr = nf = G), so each group holds a real and a fake row.
    Replicate 0 is the identity (no empty group), replicate 1 a bootstrap draw."""
    rng = np.random.RandomState(1000 + G)
    vals = rng.normal(size=G)
    if dup:
        X, Y = vals, vals[rng.permutation(G)]
    else:
        nr = min(max(int(round(0.49 * G)), 1), G - 1)
        X, Y = vals[:nr], vals[nr:]
    a, b = draw(rng, len(X), len(Y))
    return _case("seam-%d-%s" % (G, "dup" if dup else "distinct"), X, Y, [np.arange(len(X)), a], [np.arange(len(Y)), b])


# ---- first and last non-empty group deep inside the column -----------------------------------------------------------------------

DEEP_WINDOWS = ((300, 499), (600, 799))


def deep(window):
    """400 + 400 distinct values; two replicates draw only rows whose pooled rank lies in `window` (inclusive)"""
    rng = np.random.RandomState(window[0])
    Z = rng.normal(size=800)
    rank = np.argsort(np.argsort(Z))
    X, Y = Z[:400], Z[400:]
    rx = np.flatnonzero((rank[:400] >= window[0]) & (rank[:400] <= window[1]))
    ry = np.flatnonzero((rank[400:] >= window[0]) & (rank[400:] <= window[1]))
    ix = [rx[rng.randint(0, len(rx), size=400)] for _ in range(2)]
    iy = [ry[rng.randint(0, len(ry), size=400)] for _ in range(2)]
    return _case("deep-%d-%d" % window, X, Y, ix, iy)


def nonempty_span(c, r, f=0):
    """(index of the first non-empty group, index of the last, number of groups) of replicate r"""
    a, b = group_counts(c, r, f)
    g = np.flatnonzero(a + b)
    return int(g[0]), int(g[-1]), len(a)


# ---- histogram -------------------------------------------------------------------------------------------------------------------

HIST_BINS = (1, 2, 2047, 2048, 2049, 4096)
HIST_SEED = 30          # (chosen so that 661 of the 1350 values are even grid points)
ONE_VALUE_BINS = (1, 2, 7, 8)


def _hist_k():
    rng = np.random.RandomState(HIST_SEED)
    k = rng.randint(0, 4097, size=1350)
    k[0], k[700] = 0, 4096                  # the range is [0, 1]: at 4096 bins every value is an edge
    k[1], k[701], k[702] = 2048, 2048, 3000  # rows for the single-value replicates: X[1] == Y[1] = 0.5, Y[2] differs
    return rng, k


def hist_grid():
    """700 + 650 rows on the grid k / 4096 holding 0 and 1.  Replicate 0 is the identity, replicate 1 a bootstrap draw."""
    rng, k = _hist_k()
    a, b = draw(rng, 700, 650)
    return _case("hist-grid", k[:700] / 4096.0, k[700:] / 4096.0, [np.arange(700), a], [np.arange(650), b])


def on_edge(values, bins):
    """how many of `values` equal an edge of np.histogram(values, bins)"""
    e = np.histogram(values, bins)[1]
    return int(np.isin(values, e).sum())


def hist_single():
    """the same data; replicate 0 draws one row of each sample and the two are equal (lo == hi: the range is value -+ 0.5),
    replicate 1 draws one row of each and they differ"""
    _, k = _hist_k()
    one = lambda n, i: np.full(n, i)
    return _case("hist-single", k[:700] / 4096.0, k[700:] / 4096.0, [one(700, 1), one(700, 1)], [one(650, 1), one(650, 2)])


# ---- KDE -------------------------------------------------------------------------------------------------------------------------

KDE_BINS = (1, 7, 8, 9, 16, 101)
KDE_SHAPES = ((40, 300), (300, 3))


def kde(nr, nf):
    """replicate 0 identity, 1 a bootstrap draw, 2 a single row of the smaller sample against a draw of the larger, 3 one pooled
    value (X[0] == Y[0], both samples draw only that row: the grid is constant)"""
    rng = np.random.RandomState(nr * 7 + nf)
    X, Y = rng.normal(size=nr), rng.normal(0.4, 1.3, size=nf)
    Y[0] = X[0]
    a, b = draw(rng, nr, nf)
    a2, b2 = draw(rng, nr, nf)
    if nr < nf:
        a2 = np.full(nr, nr - 1)
    else:
        b2 = np.full(nf, nf - 1)
    return _case("kde-%d-%d" % (nr, nf), X, Y, [np.arange(nr), a, a2, np.zeros(nr, int)], [np.arange(nf), b, b2, np.zeros(nf, int)])


def kde_logsum_longdouble(s, grid, h):
    """metrics1d_numpy.kde_logsum in np.longdouble from the same float64 inputs"""
    s, grid, h = s.astype(np.longdouble), grid.astype(np.longdouble), np.longdouble(h)
    t = np.longdouble(-0.5) * (grid[:, None] - s[None, :]) ** 2 / (h * h)
    m = t.max(axis=1)
    return m + np.log(np.exp(t - m[:, None]).sum(axis=1))


# ---- the Cramer-von Mises cap and k_counts' stride loop --------------------------------------------------------------------------

def big(extra=0):
    """nr = 2^19 + extra, nf = 2^19, values rounded to 3 decimals (heavy ties).  Replicate 0 identity, replicate 1 a draw."""
    nr, nf = (CVM_MAX_N >> 1) + extra, CVM_MAX_N >> 1
    rng = np.random.RandomState(20 + extra)
    X, Y = np.round(rng.normal(size=nr), 3), np.round(rng.normal(0.05, 1.1, size=nf), 3)
    a, b = draw(rng, nr, nf)
    return _case("big+%d" % extra, X, Y, [np.arange(nr), a], [np.arange(nf), b])


# ---- ks_2samp's exact / asymptotic switch ----------------------------------------------------------------------------------------

KS_SWITCH = ((10000, 64), (10001, 64))
KS_SEED, KS_ITERS = 31, 3


def ks_switch(nr, nf):
    """(X [nr, 3], Y [nf, 3]) for the public call; the draws come from numpy's global generator seeded with KS_SEED"""
    rng = np.random.RandomState(nr)
    return rng.normal(size=(nr, 3)), rng.normal(0.1, 1.0, size=(nf, 3))


# ---- siblings --------------------------------------------------------------------------------------------------------------------

def bootstrap(nr, nf, d, reps, decimals=None, seed=0):
    """ordinary data and `reps` bootstrap replicates"""
    rng = np.random.RandomState(nr * 3 + nf + d + seed)
    X, Y = rng.normal(size=(nr, d)), rng.normal(0.3, 1.2, size=(nf, d))
    if decimals is not None:
        X, Y = np.round(X, decimals), np.round(Y, decimals)
    idx = [draw(rng, nr, nf) for _ in range(reps)]
    return _case("boot-%d-%d-%d" % (nr, nf, d), X, Y, [i[0] for i in idx], [i[1] for i in idx])


def alone(c, r):
    """replicate r of `c` as a case of its own"""
    return Case("%s[%d]" % (c.name, r), c.X, c.Y, c.ix[r:r + 1], c.iy[r:r + 1])


# ---- the table exactly fills LDS, or misses it by one ----------------------------------------------------------------------------

FULL_TABLE = ((1024, 1024), (1024, 1025))


def full_table(nr, nf):
    """all-distinct values: the bound min(G, nr) + min(G, nf) is nr + nf.  Replicate 0 is the identity: Mr + Mf == nr + nf, the table is
    exactly full and the front-filled and back-filled halves touch.  Replicate 1 is a bootstrap draw."""
    rng = np.random.RandomState(nr + nf)
    X, Y = rng.normal(size=nr), rng.normal(0.2, 1.5, size=nf)
    a, b = draw(rng, nr, nf)
    return _case("full-%d-%d" % (nr, nf), X, Y, [np.arange(nr), a], [np.arange(nf), b])


# ---- ties decide where the table lives -------------------------------------------------------------------------------------------

TIED_G = (1024, 1025)


def tied(G):
    """nr = nf = 1500 rows over G distinct numbers, both samples holding every one of them.  N = 3000 > WP_LDS: the caller passes
    a workspace; the bound is 2 G.  Replicate 0 identity, replicate 1 a bootstrap draw."""
    rng = np.random.RandomState(G)
    vals = rng.normal(size=G)
    X = np.concatenate([vals, vals[rng.randint(0, G, size=1500 - G)]])[rng.permutation(1500)]
    Y = np.concatenate([vals, vals[rng.randint(0, G, size=1500 - G)]])[rng.permutation(1500)]
    a, b = draw(rng, 1500, 1500)
    return _case("tied-%d" % G, X, Y, [np.arange(1500), a], [np.arange(1500), b])


# ---- the tile hand-off of the workspace path -------------------------------------------------------------------------------------

HANDOFF = ((1, 1), (512, 512), (512, 513), (1024, 1024), (1500, 1), (1, 1500), (1500, 1500))


def _spread(rng, n, m, even):
    """an index vector of n draws over m distinct rows: the n - m surplus draws spread evenly over them, or all on the first"""
    rows = rng.permutation(n)[:m]
    idx = np.resize(rows, n) if even else np.concatenate([rows, np.full(n - m, rows[0])])
    return idx[rng.permutation(n)]


def handoff(Mr, Mf, apart):
    """1500 + 1500 distinct values (the bound is 3000: the table is in the workspace).  Both replicates draw exactly Mr distinct real
    and Mf distinct fake rows, so the merge has T = Mr + Mf steps: replicate 0 spreads the surplus draws evenly over the drawn rows,
    replicate 1 puts them all on one row.  apart: every real value lies below every fake value; else the supports interleave."""
    rng = np.random.RandomState(Mr * 3 + Mf + (7 if apart else 0))
    Z = rng.normal(size=3000)
    if apart:
        Z = np.sort(Z)
        X, Y = Z[:1500][rng.permutation(1500)], Z[1500:][rng.permutation(1500)]
    else:
        X, Y = Z[:1500], Z[1500:]
    ix = [_spread(rng, 1500, Mr, even) for even in (True, False)]
    iy = [_spread(rng, 1500, Mf, even) for even in (True, False)]
    return _case("handoff-%d-%d-%s" % (Mr, Mf, "apart" if apart else "mixed"), X, Y, ix, iy)


def coprime():
    """1499 + 1501 distinct values, two bootstrap draws: coprime sizes, so no two breakpoints but the last coincide"""
    rng = np.random.RandomState(1499)
    X, Y = rng.normal(size=1499), rng.normal(0.3, 0.8, size=1501)
    idx = [draw(rng, 1499, 1501) for _ in range(2)]
    return _case("coprime", X, Y, [i[0] for i in idx], [i[1] for i in idx])
