"""energy_test, mmd_test, knn_test: permutation two-sample tests on the GPU (kernels: csrc/pf_perm.hip, pfm_perm_labels and
pfm_perm_form; csrc/pf_nn.hip, pfm_nn_index and pfm_nn_count; host side: _boot.py, _m1d.py).  The reference has no such test;
the arguments follow energy_distance.

The question the bootstrap (mean, std) of the other metrics does not answer: can the difference between the real and the
generated sample be told from chance?  Pool the nr + nf rows, relabel them at random n_permutations times (nr rows "real"
each time) and see where the statistic of the samples as given falls among the relabelled ones:
  pvalue = (1 + #{null >= statistic}) / (1 + n_permutations).

With s[a] = +nf on a row labelled real and -nr otherwise, the statistic of a labelling is the signed pair sum
S = sum_ab s[a] s[b] G(a, b) over the pooled rows, scaled by (nr nf)^2:
  energy_test   G = |z_a - z_b|,            D^2 = -S / (nr nf)^2: energy_distance_full_sample(squared=True), the V-statistic,
                which rounding may leave a few 1e-16 below 0;
  mmd_test      G = exp(-gamma |z_a - z_b|^2), MMD^2 = +S / (nr nf)^2: the reference's mmd_calc, mean K_XX + mean K_YY - 2 mean
                K_XY with the diagonals included.  gamma = 1 / (2 median^2) of the pooled distance matrix, or 1 / (2 bandwidth^2);
                the pooled sample does not change under relabelling, so gamma is the same for every labelling.
G does not depend on the labelling: the kernel forms every pair value once per group of labellings and spends one float64
multiply-add per labelling and pair.

knn_test (Schilling 1986; Henze 1988) has a statistic that reads as a rate: the share of the rows' nearest_k nearest neighbours
in the pooled sample that carry the row's own label; with nearest_k = 1 the leave-one-out 1-NN classifier accuracy.  The
neighbours do not depend on the labelling either: one sweep over the pairs finds them (pfm_nn_index), and a labelling then
costs N nearest_k label look-ups (pfm_nn_count).  It draws and uses the same labellings as energy_test.

The labellings are drawn on the device by a counter-based generator (Philox4x32-10; pf_metrics.h states the definition), seeded
by the ONE draw a call makes from numpy's global generator: lo, hi = np.random.randint(0, 2**32, size=2, dtype=np.uint64),
seed = lo | hi << 32.  A seeded call is bitwise reproducible.  The observed labelling is not drawn.

Inputs may be numpy arrays, array-likes or torch tensors; a CUDA tensor stays on its device.  NaN or infinite input, a bad
n_permutations, a non-bool standardize, a bad bandwidth and a bad nearest_k raise ValueError before anything is drawn.
Importing this module needs no GPU.
"""
import collections
import math

import numpy as np
import torch

from . import _boot, _lib, _m1d

TwoSampleTest = collections.namedtuple("TwoSampleTest", ("statistic", "pvalue", "null"))
KnnTest = collections.namedtuple("KnnTest", ("statistic", "pvalue", "null", "real", "fake"))
NnAccuracy = collections.namedtuple("NnAccuracy", ("total", "real", "fake"))

GROUP_BYTES = 256 << 20     # labels and kernel workspace of one group of labellings
MAX_GROUP = 1 << 16         # labellings per group, at most


def group_size(n_labellings, rows, ws_per_rep):
    """labellings per group: a group's label bytes [G, rows] and its kernel workspace stay within GROUP_BYTES"""
    return int(max(1, min(n_labellings, MAX_GROUP, GROUP_BYTES // (rows + max(1, ws_per_rep)))))


def _check(X_real, X_fake, n_permutations, standardize, bandwidth=None):
    _m1d.check_positive_int(n_permutations, "n_permutations")
    _m1d.check_bool(standardize, "standardize")
    _m1d.check_positive(bandwidth, "bandwidth", none_ok=True)
    _m1d.check_args(X_real, X_fake, 1)


def _median(Xr, Xf):
    """the median of the pooled distance matrix of the samples as given: pfm_mmd's identity replicate"""
    (nr, d), nf = Xr.shape, Xf.shape[0]
    out = torch.empty(2, dtype=torch.float64, device=Xr.device)
    _boot.replicates(nr, nf, Xr.device, None, lambda r: _lib.mmd_workspace_bytes(nr, nf, d, r),
                     lambda start, reps, ir, jf, ws: _lib.mmd(Xr, Xf, ir, jf, reps, out[:1], out[1:], ws))
    return float(out[0])


def pvalue_of(statistic, null):
    """(1 + #{null >= statistic}) / (1 + n_permutations)"""
    null = np.asarray(null, np.float64)
    return np.float64(1 + int(np.count_nonzero(null >= statistic))) / np.float64(1 + null.size)


def values_of(S, nr, nf, kind):
    """[n] raw signed pair sums -> D^2 = -S / (nr nf)^2 (energy) or MMD^2 = +S / (nr nf)^2 (Gauss); a zero sum gives +0.0"""
    S = np.asarray(S, np.float64)
    den = np.float64((nr * nf) ** 2)
    return (0.0 - S) / den if kind == _lib.PERM_ENERGY else (0.0 + S) / den


def _seed():
    """the one draw of a call from numpy's global generator"""
    lo, hi = np.random.randint(0, 2 ** 32, size=2, dtype=np.uint64)
    return int(lo) | int(hi) << 32


def _labellings(seed, total, N, nr, workspace_bytes, statistic, device):
    """The labellings of one call, group by group: the observed one (the first nr of the N pooled rows are real) in front of
    the total - 1 drawn from `seed`.  statistic(lab, reps, start, ws) enqueues the statistic of the labellings lab
    [reps, N] (uint8) into slots start .. start + reps - 1 of its output; ws holds workspace_bytes(reps) bytes at least."""
    G = group_size(total, N, workspace_bytes(1))
    ws = torch.empty(max(workspace_bytes(G), _lib.perm_labels_workspace_bytes(G, N, nr)), dtype=torch.uint8, device=device)
    labels = torch.empty((G, N), dtype=torch.uint8, device=device)
    for start in range(0, total, G):
        reps = min(G, total - start)
        lab = labels[:reps]
        own = 1 if start == 0 else 0                                  # labelling 0 of the call is the observed one
        if own:
            lab[0] = (torch.arange(N, device=device) < nr).to(torch.uint8)
        if reps > own:
            _lib.perm_labels(seed, _lib.KEY_MASK_ALL, start + own - 1, reps - own, N, nr, lab[own:], ws)
        statistic(lab, reps, start, ws)


def _test(kind, X_real, X_fake, n_permutations, standardize, bandwidth):
    _check(X_real, X_fake, n_permutations, standardize, bandwidth)
    Xr, Xf = _boot.prepare(X_real, X_fake, ("X_real", "X_fake"), 1, standardize)
    (nr, d), nf = Xr.shape, Xf.shape[0]
    N, total = nr + nf, int(n_permutations) + 1                       # the observed labelling in front of the drawn ones
    with torch.cuda.device(Xr.device):
        gamma = 0.0
        if kind == _lib.PERM_GAUSS:
            sigma = float(bandwidth) if bandwidth is not None else _median(Xr, Xf)
            if not sigma > 0:
                raise ValueError("the median pairwise distance is 0, so gamma = 1 / (2 median^2) is infinite (too few "
                                 "distinct rows)")
            gamma = 1.0 / (2 * sigma ** 2)
            if not (math.isfinite(gamma) and gamma > 0):
                raise ValueError("gamma = 1 / (2 sigma^2) is not a positive finite number for sigma = %r" % (sigma,))
        seed = _seed()
        Z = torch.cat([Xr, Xf], dim=0).contiguous()
        S = torch.empty(total, dtype=torch.float64, device=Xr.device)
        _labellings(seed, total, N, nr, lambda r: _lib.perm_form_workspace_bytes(N, d, nr, r),
                    lambda lab, reps, start, ws: _lib.perm_form(kind, gamma, Z, nr, lab, reps, S[start:start + reps], ws),
                    Xr.device)
        V = values_of(S.cpu().numpy(), nr, nf, kind)
    statistic, null = V[0], V[1:].copy()
    return TwoSampleTest(statistic, pvalue_of(statistic, null), null)


def energy_test(X_real, X_fake, n_permutations=999, standardize=False):
    '''
    Permutation test of the energy distance (Szekely & Rizzo) between real and fake samples.

    Parameters:
    -----------
    X_real: array of shape [n_samples, n_features] (numpy, array-like or torch; a CUDA tensor stays on the device)
        Real sample.
    X_fake: array of shape [m_samples, n_features]
        Generated sample.
    n_permutations: int
        The number of random relabellings of the pooled sample. Default = 999.
    standardize: boolean
        If True, the StandardScaler fitted on the real sample is applied to both. Default = False.

    Return:
    -------
    TwoSampleTest(statistic, pvalue, null): D^2 of the samples as given (energy_distance_full_sample(squared=True)),
    (1 + #{null >= statistic}) / (1 + n_permutations), and D^2 of every relabelling [n_permutations]; numpy float64.
    '''
    return _test(_lib.PERM_ENERGY, X_real, X_fake, n_permutations, standardize, None)


def mmd_test(X_real, X_fake, n_permutations=999, standardize=False, bandwidth=None):
    '''
    Permutation test of the Maximum Mean Discrepancy (RBF kernel) between real and fake samples.

    Parameters:
    -----------
    X_real, X_fake, n_permutations, standardize: as energy_test.
    bandwidth: None or float
        sigma of the kernel exp(-d^2 / (2 sigma^2)). Default = None: the median of the pooled distance matrix of the samples
        as given, as the reference's mmd_calc takes it.

    Return:
    -------
    TwoSampleTest(statistic, pvalue, null): mean K_XX + mean K_YY - 2 mean K_XY of the samples as given (diagonals included),
    (1 + #{null >= statistic}) / (1 + n_permutations), and the same of every relabelling [n_permutations]; numpy float64.

    Raises ValueError if bandwidth is None and the median pairwise distance is 0.
    '''
    return _test(_lib.PERM_GAUSS, X_real, X_fake, n_permutations, standardize, bandwidth)


def _check_k(nearest_k, N):
    if not _m1d.is_int(nearest_k) or not 1 <= nearest_k <= min(_lib.NN_MAX_K, N - 1):
        raise ValueError("nearest_k must be an integer in 1 .. min(%d, n_real + n_fake - 1 = %d), got %r"
                         % (_lib.NN_MAX_K, N - 1, nearest_k))


def shares_of(counts, nr, nf, k):
    """[n, 2] int64 counts (both labelled real, both labelled fake) -> float64 [n, 3] same-label shares of all rows' neighbours,
    of the real rows' and of the fake rows': Python ints divided, rounded once"""
    return np.array([[(int(cr) + int(cf)) / ((nr + nf) * k), int(cr) / (nr * k), int(cf) / (nf * k)] for cr, cf in counts],
                    dtype=np.float64).reshape(-1, 3)


def _knn(X_real, X_fake, n_permutations, nearest_k, standardize):
    """-> (shares_of the observed labelling [3], the statistic of the drawn ones [n_permutations]); n_permutations = None draws
    nothing"""
    _check(X_real, X_fake, 1 if n_permutations is None else n_permutations, standardize)
    _check_k(nearest_k, _boot._check_2d(X_real, "X_real")[1][0] + _boot._check_2d(X_fake, "X_fake")[1][0])
    Xr, Xf = _boot.prepare(X_real, X_fake, ("X_real", "X_fake"), 1, standardize)
    (nr, d), nf = Xr.shape, Xf.shape[0]
    N, k = nr + nf, int(nearest_k)
    total = 1 + int(n_permutations or 0)                              # the observed labelling in front of the drawn ones
    with torch.cuda.device(Xr.device):
        seed = _seed() if total > 1 else None
        dev = Xr.device
        Z = torch.cat([Xr, Xf], dim=0).contiguous()
        nbr = torch.empty((N, k), dtype=torch.int32, device=dev)
        d2 = torch.empty((N, k), dtype=torch.float64, device=dev)
        _lib.nn_index(Z, k, nbr, d2, torch.empty(_lib.nn_index_workspace_bytes(N, d, k), dtype=torch.uint8, device=dev))
        counts = torch.empty((total, 2), dtype=torch.int64, device=dev)
        _labellings(seed, total, N, nr, lambda r: _lib.nn_count_workspace_bytes(N, k, r),
                    lambda lab, reps, start, ws: _lib.nn_count(nbr, N, k, lab, reps, counts[start:start + reps], ws), dev)
        C = counts.cpu().tolist()                                     # Python ints: every ratio is rounded once
    return shares_of(C[:1], nr, nf, k)[0], np.array([(cr + cf) / (N * k) for cr, cf in C[1:]], dtype=np.float64)


def knn_test(X_real, X_fake, n_permutations=999, nearest_k=1, standardize=False):
    '''
    Nearest-neighbour permutation two-sample test (Schilling 1986; Henze 1988) between real and fake samples. With
    nearest_k = 1 the statistic is the leave-one-out 1-NN classifier accuracy (Lopez-Paz & Oquab 2017).

    Parameters:
    -----------
    X_real, X_fake, n_permutations, standardize: as energy_test; the same labellings are drawn from the same seed draw.
    nearest_k: int
        The number of nearest neighbours of a row, in 1 .. min(16, n_samples + m_samples - 1). Default = 1. The neighbours are
        the nearest other rows of the pooled sample by squared Euclidean distance, ties by row index (real rows first); a
        duplicate of a row is its neighbour at distance 0.

    Return:
    -------
    KnnTest(statistic, pvalue, null, real, fake): the share of all N * nearest_k neighbour slots whose neighbour carries the
    row's own label; (1 + #{null >= statistic}) / (1 + n_permutations); the share under every relabelling [n_permutations];
    the same share among the real rows' and among the fake rows' slots; numpy float64.

    Under the null hypothesis the expected statistic is (nr (nr - 1) + nf (nf - 1)) / (N (N - 1)), about 0.5 for samples of
    equal size; samples that differ push it towards 1. pvalue is the upper tail. A statistic BELOW the null values is what
    generated rows that copy real rows look like (each row's nearest neighbour is its copy in the other sample; 0.0 for an exact
    copy at nearest_k = 1): null is returned so that the lower tail, (1 + #{null <= statistic}) / (1 + n_permutations), can be
    taken by hand.
    '''
    if n_permutations is None:
        raise ValueError("n_permutations must be a positive integer, got None")
    (statistic, real, fake), null = _knn(X_real, X_fake, n_permutations, nearest_k, standardize)
    return KnnTest(statistic, pvalue_of(statistic, null), null, real, fake)


def nn_accuracy_full_sample(X_real, X_fake, nearest_k=1, standardize=False):
    '''
    The statistic of knn_test alone: nothing is drawn and numpy's global generator is left untouched.

    Return:
    -------
    NnAccuracy(total, real, fake): knn_test's statistic, real and fake; with nearest_k = 1 the leave-one-out 1-NN accuracy over
    all rows, over the real rows and over the fake rows; numpy float64.
    '''
    return NnAccuracy(*_knn(X_real, X_fake, None, nearest_k, standardize)[0])
