"""ctypes binding of libpf_metrics.so (C ABI: probaforms_amd/metrics/csrc/pf_metrics.h).

The library is built in-tree by `make -C probaforms_amd/metrics/csrc` (see __graft_entry__.build) and
loaded on the first call, so importing probaforms_amd.metrics needs no GPU.  There is NO fallback: a
missing library or a tensor off the HIP device raises.
"""
import ctypes as C
import os

import torch

from .._cbind import Library, LibraryMissing, ptr as _ptr

ABI_VERSION = 101          # pfm_version() of the library this binding matches (pf_metrics.h PFM_VERSION)
MOMENTS_MAX_D = 4096       # PFM_MOMENTS_MAX_D
# pfm_metric1d's statistics (pf_metrics.h PFM_M1D_*)
M1D_KS, M1D_CVM, M1D_AD, M1D_AUC, M1D_HIST, M1D_KDE = range(6)
CVM_MAX_N = 1 << 20        # pooled rows pfm_metric1d's Cramer-von Mises sums hold exactly
KNN_MAX_K = 16             # PFM_KNN_MAX_K: the largest nearest_k of pfm_prdc
NN_MAX_K = 16              # PFM_NN_MAX_K: the largest k of pfm_nn_index
NN_STAGE_MAX_N = 262144    # PFM_NN_STAGE_MAX_N: rows up to which pfm_nn_count keeps a labelling in LDS
ENERGY_TILE = 64           # PFM_ENERGY_TILE: rows per side of a pair tile of pfm_energy
ENERGY_REP_BLOCK = 16      # PFM_ENERGY_REP_BLOCK: replicates per count tile of pfm_energy
PERM_ENERGY, PERM_GAUSS = 0, 1   # PFM_PERM_*: the pair value of pfm_perm_form
KEY_MASK_ALL = 2 ** 64 - 1 # pfm_perm_labels' key_mask in use: all 64 key bits count
PAIR_MAX_GAMMAS = 8        # PFM_PAIR_MAX_GAMMAS: Gaussians in pfm_pair_grad's kernel sum
SLICE_LDS_ROWS = 13312     # PFM_SLICE_LDS_ROWS: rows per sample pfm_slice_grad sorts itself, in LDS
SCORE_MAX_K = 1024         # PFM_SCORE_MAX_K: draws per row of pfm_score_grad
SCORE_MAX_KD = 16384       # PFM_SCORE_MAX_KD: draws times features of pfm_score_grad (a row's draws in LDS)
VARIO_MAX_D = 64           # PFM_VARIO_MAX_D: features of pfm_variogram_grad (a row's pair table in LDS beside its draws)
SORT_MAX_K = 8192          # PFM_SORT_MAX_K: draws per series of pfm_sort_score (a series' entries and ranks in the LDS of one CU)
SORT_MAX_Q = 16            # PFM_SORT_MAX_Q: quantile levels of pfm_sort_score and pfm_pinball_grad
FRECHET_MAX_D = 64         # PFM_FRECHET_MAX_D: rows of a matrix of pfm_sym_eig, features of pfm_frechet_grad (four matrices in LDS)
EIG_MAX_SWEEPS = 30        # PFM_EIG_MAX_SWEEPS: the sweeps after which pfm_sym_eig stops whatever the matrix holds
PFM_EINVAL, PFM_EUNSUPPORTED, PFM_EWORKSPACE = -1, -2, -3

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libpf_metrics.so")

_VP, _I64, _SZ = C.c_void_p, C.c_int64, C.c_size_t

_SIGNATURES = {
    "pfm_version": (C.c_int, []),
    "pfm_status_string": (C.c_char_p, [C.c_int]),
    "pfm_mmd_workspace_bytes": (_SZ, [_I64, _I64, _I64, _I64]),
    "pfm_mmd": (C.c_int, [_VP, _VP, _I64, _VP, _I64, _I64, _VP, _VP, _I64, _VP, _VP, _VP, _SZ]),
    "pfm_moments_workspace_bytes": (_SZ, [_I64, _I64, _I64, _I64]),
    "pfm_boot_moments": (C.c_int, [_VP, _VP, _I64, _VP, _I64, _I64, _VP, _VP, _I64, _VP, _VP, _VP, _SZ]),
    "pfm_metric1d_workspace_bytes": (_SZ, [C.c_int, _I64, _I64, _I64, _I64, _I64]),
    "pfm_metric1d": (C.c_int, [_VP, C.c_int, _VP, _VP, _VP, _VP, _I64, _I64, _I64, _VP, _VP, _I64, _I64, C.c_double,
                               C.c_double, _VP, _VP, _SZ]),
    "pfm_project": (C.c_int, [_VP, _VP, _I64, _VP, _I64, _I64, _VP, _I64, _VP]),
    "pfm_wasserstein1d_workspace_bytes": (_SZ, [_I64, _I64, _I64, _I64, C.c_int]),
    "pfm_wasserstein1d": (C.c_int, [_VP, C.c_int, _VP, _VP, _VP, _VP, _I64, _I64, _I64, _VP, _VP, _I64, _VP, _VP, _SZ]),
    "pfm_prdc_workspace_bytes": (_SZ, [_I64, _I64, _I64, _I64, _I64]),
    "pfm_prdc": (C.c_int, [_VP, _VP, _I64, _VP, _I64, _I64, _VP, _VP, _I64, _I64, _VP, _VP, _VP, _VP, _SZ]),
    "pfm_energy_workspace_bytes": (_SZ, [_I64, _I64, _I64, _I64]),
    "pfm_energy": (C.c_int, [_VP, _VP, _I64, _VP, _I64, _I64, _VP, _VP, _I64, _VP, _VP, _SZ]),
    "pfm_sinkhorn_workspace_bytes": (_SZ, [_I64, _I64, _I64, _I64]),
    "pfm_sinkhorn": (C.c_int, [_VP, _VP, _I64, _VP, _I64, _I64, _VP, _VP, _I64, C.c_int, C.c_double, _I64, _VP, _VP, _VP,
                               _VP, _SZ]),
    "pfm_perm_labels_workspace_bytes": (_SZ, [_I64, _I64, _I64]),
    "pfm_perm_labels": (C.c_int, [_VP, C.c_uint64, C.c_uint64, _I64, _I64, _I64, _I64, _VP, _VP, _SZ]),
    "pfm_perm_form_workspace_bytes": (_SZ, [_I64, _I64, _I64, _I64]),
    "pfm_perm_form": (C.c_int, [_VP, C.c_int, C.c_double, _VP, _I64, _I64, _I64, _VP, _I64, _VP, _VP, _SZ]),
    "pfm_nn_index_workspace_bytes": (_SZ, [_I64, _I64, _I64]),
    "pfm_nn_index": (C.c_int, [_VP, _VP, _I64, _I64, _I64, _VP, _VP, _VP, _SZ]),
    "pfm_nn_count_workspace_bytes": (_SZ, [_I64, _I64, _I64]),
    "pfm_nn_count": (C.c_int, [_VP, _VP, _I64, _I64, _VP, _I64, _VP, _VP, _SZ]),
    "pfm_pair_grad_workspace_bytes": (_SZ, [_I64, _I64, _I64]),
    "pfm_pair_grad": (C.c_int, [_VP, C.c_int, _VP, C.c_int, _VP, _I64, _I64, _I64, _VP, _VP, _VP, _SZ]),
    "pfm_sinkhorn_grad_workspace_bytes": (_SZ, [_I64, _I64, _I64]),
    "pfm_sinkhorn_grad": (C.c_int, [_VP, _VP, _I64, _I64, _I64, C.c_int, C.c_double, _I64, _VP, _VP, _VP, _VP, _VP, _SZ]),
    "pfm_slice_grad_workspace_bytes": (_SZ, [_I64, _I64, _I64, _I64]),
    "pfm_slice_grad": (C.c_int, [_VP, C.c_int, _VP, _I64, _I64, _I64, _VP, _I64, _VP, _VP, _VP, _VP, _VP, _VP, _SZ]),
    "pfm_score_grad_workspace_bytes": (_SZ, [_I64, _I64, _I64]),
    "pfm_score_plan": (C.c_int, [_I64, _I64, _I64, _VP]),
    "pfm_score_grad": (C.c_int, [_VP, _VP, _VP, _I64, _I64, _I64, C.c_int, _VP, _VP, _VP, _VP, _VP, _SZ]),
    "pfm_variogram_grad_workspace_bytes": (_SZ, [_I64, _I64, _I64]),
    "pfm_variogram_plan": (C.c_int, [_I64, _I64, _I64, _VP]),
    "pfm_variogram_grad": (C.c_int, [_VP, _VP, _VP, _VP, _I64, _I64, _I64, C.c_double, _VP, _VP, _VP, _VP, _SZ]),
    "pfm_sort_score_workspace_bytes": (_SZ, [_I64, _I64, _I64]),
    "pfm_sort_score_plan": (C.c_int, [_I64, _I64, _VP]),
    "pfm_sort_score": (C.c_int, [_VP, _VP, _VP, _I64, _I64, C.c_int, _VP, C.c_int, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _SZ]),
    "pfm_pinball_grad": (C.c_int, [_VP, _VP, _VP, _VP, _VP, C.c_int, _I64, _I64, _VP, _VP, _VP, _SZ]),
    "pfm_sym_eig_workspace_bytes": (_SZ, [_I64, _I64]),
    "pfm_sym_eig": (C.c_int, [_VP, _VP, _I64, _I64, _VP, _VP, _VP, _VP, _SZ]),
    "pfm_frechet_grad_workspace_bytes": (_SZ, [_I64, _I64, _I64]),
    "pfm_frechet_grad": (C.c_int, [_VP, _VP, _I64, _I64, _I64, C.c_double, C.c_int, _VP, _VP, _VP, _VP, _VP, _VP, _SZ]),
}
EXPORTS = tuple(_SIGNATURES)


class MetricsLibraryMissing(LibraryMissing):
    pass


LIBRARY = Library(LIB_PATH, os.path.dirname(LIB_PATH), "pfm_", ABI_VERSION, _SIGNATURES, MetricsLibraryMissing,
                  "probaforms_amd.metrics has no CPU fallback.")
lib = LIBRARY.load
check = LIBRARY.check


def mmd_workspace_bytes(nx, ny, d, reps):
    return int(lib().pfm_mmd_workspace_bytes(int(nx), int(ny), int(d), int(reps)))


def moments_workspace_bytes(nr, nf, d, reps):
    return int(lib().pfm_moments_workspace_bytes(int(nr), int(nf), int(d), int(reps)))


def mmd_status(X, Y, idx_x, idx_y, reps, median, out, ws):
    """enqueue `reps` MMD replicates on the current stream and return the status; idx_x / idx_y are flat int32 device
    views [reps * nx] / [reps * ny]; median / out are float64 device views of `reps` elements"""
    nx, d = X.shape
    ny = Y.shape[0]
    assert idx_x.numel() == reps * nx and idx_y.numel() == reps * ny and median.numel() == reps == out.numel()
    return int(lib().pfm_mmd(torch.cuda.current_stream().cuda_stream, _ptr(X, torch.float64, "X"), nx,
                             _ptr(Y, torch.float64, "Y"), ny, d, _ptr(idx_x, torch.int32, "idx_x"),
                             _ptr(idx_y, torch.int32, "idx_y"), int(reps), _ptr(median, torch.float64, "median"),
                             _ptr(out, torch.float64, "mmd"), _ptr(ws, torch.uint8, "workspace"), ws.numel()))


def mmd(*args):
    check(mmd_status(*args), "pfm_mmd")


def boot_moments_status(Xr, Xf, idx_r, idx_f, reps, mean, cov, ws):
    """enqueue the bootstrap means [reps, 2, d] and covariances [reps, 2, d, d] on the current stream and return the
    status"""
    nr, d = Xr.shape
    nf = Xf.shape[0]
    assert idx_r.numel() == reps * nr and idx_f.numel() == reps * nf
    assert mean.numel() == reps * 2 * d and cov.numel() == reps * 2 * d * d
    return int(lib().pfm_boot_moments(torch.cuda.current_stream().cuda_stream, _ptr(Xr, torch.float64, "X_real"), nr,
                                      _ptr(Xf, torch.float64, "X_fake"), nf, d, _ptr(idx_r, torch.int32, "idx_real"),
                                      _ptr(idx_f, torch.int32, "idx_fake"), int(reps), _ptr(mean, torch.float64, "mean"),
                                      _ptr(cov, torch.float64, "cov"), _ptr(ws, torch.uint8, "workspace"), ws.numel()))


def boot_moments(*args):
    check(boot_moments_status(*args), "pfm_boot_moments")


def metric1d_workspace_bytes(metric, nr, nf, d, reps, bins):
    return int(lib().pfm_metric1d_workspace_bytes(int(metric), int(nr), int(nf), int(d), int(reps), int(bins)))


def metric1d_status(metric, cols, perm, gstart, ngroups, nr, nf, idx_r, idx_f, reps, bins, h_r, h_f, out, ws):
    """enqueue `reps` replicates of one pfm_metric1d statistic on the current stream and return the status; cols /
    perm / gstart / ngroups describe the pooled columns (pf_metrics.h), `out` is the statistic's output view"""
    d = cols.shape[0]
    assert idx_r.numel() == reps * nr and idx_f.numel() == reps * nf and cols.shape[1] == nr + nf
    return int(lib().pfm_metric1d(torch.cuda.current_stream().cuda_stream, int(metric), _ptr(cols, torch.float64, "cols"),
                                  _ptr(perm, torch.int32, "perm"), _ptr(gstart, torch.int32, "gstart"),
                                  _ptr(ngroups, torch.int32, "ngroups"), int(nr), int(nf), int(d),
                                  _ptr(idx_r, torch.int32, "idx_real"), _ptr(idx_f, torch.int32, "idx_fake"), int(reps),
                                  int(bins), float(h_r), float(h_f), _ptr(out, out.dtype, "out"), _ptr(ws, torch.uint8, "workspace"),
                                  ws.numel()))


def metric1d(*args):
    check(metric1d_status(*args), "pfm_metric1d")


def project(Xr, Xf, theta, cols):
    """enqueue cols[k, i] = sum_j [Xr; Xf][i, j] * theta[k, j] (feature order, product and sum rounded separately) on
    the current stream; cols [n_proj, nr + nf] float64"""
    nr, d = Xr.shape
    nf = Xf.shape[0]
    n_proj = theta.shape[0]
    assert Xf.shape[1] == d == theta.shape[1] and tuple(cols.shape) == (n_proj, nr + nf)
    st = lib().pfm_project(torch.cuda.current_stream().cuda_stream, _ptr(Xr, torch.float64, "X_real"), nr,
                           _ptr(Xf, torch.float64, "X_fake"), nf, d, _ptr(theta, torch.float64, "theta"), n_proj,
                           _ptr(cols, torch.float64, "cols"))
    check(st, "pfm_project")


def wasserstein1d_workspace_bytes(nr, nf, d, reps, p):
    return int(lib().pfm_wasserstein1d_workspace_bytes(int(nr), int(nf), int(d), int(reps), int(p)))


def wasserstein1d_status(p, cols, perm, gstart, ngroups, nr, nf, idx_r, idx_f, reps, out, ws):
    """enqueue W_p^p of `reps` replicates of every pooled column on the current stream and return the status; `out` is a
    float64 view of reps * d elements"""
    d = cols.shape[0]
    assert idx_r.numel() == reps * nr and idx_f.numel() == reps * nf and cols.shape[1] == nr + nf
    assert out.numel() == reps * d
    return int(lib().pfm_wasserstein1d(torch.cuda.current_stream().cuda_stream, int(p), _ptr(cols, torch.float64, "cols"),
                                       _ptr(perm, torch.int32, "perm"), _ptr(gstart, torch.int32, "gstart"),
                                       _ptr(ngroups, torch.int32, "ngroups"), int(nr), int(nf), int(d),
                                       _ptr(idx_r, torch.int32, "idx_real"), _ptr(idx_f, torch.int32, "idx_fake"), int(reps),
                                       _ptr(out, torch.float64, "out"), _ptr(ws, torch.uint8, "workspace"), ws.numel()))


def wasserstein1d(*args):
    check(wasserstein1d_status(*args), "pfm_wasserstein1d")


def prdc_workspace_bytes(nr, nf, d, reps, k):
    return int(lib().pfm_prdc_workspace_bytes(int(nr), int(nf), int(d), int(reps), int(k)))


def prdc_status(Xr, Xf, idx_r, idx_f, reps, k, radius2_r, radius2_f, counts, ws):
    """enqueue `reps` replicates of the k-nearest-neighbour counts on the current stream and return the status;
    radius2_r / radius2_f are float64 views of reps * nr / reps * nf elements (the squared k-th-neighbour radii), counts an
    int64 view of reps * 4 elements (P, Rc, Dn, Cv)"""
    nr, d = Xr.shape
    nf = Xf.shape[0]
    assert Xf.shape[1] == d and idx_r.numel() == reps * nr and idx_f.numel() == reps * nf
    assert radius2_r.numel() == reps * nr and radius2_f.numel() == reps * nf and counts.numel() == reps * 4
    return int(lib().pfm_prdc(torch.cuda.current_stream().cuda_stream, _ptr(Xr, torch.float64, "X_real"), nr,
                              _ptr(Xf, torch.float64, "X_fake"), nf, d, _ptr(idx_r, torch.int32, "idx_real"),
                              _ptr(idx_f, torch.int32, "idx_fake"), int(reps), int(k),
                              _ptr(radius2_r, torch.float64, "radius2_r"), _ptr(radius2_f, torch.float64, "radius2_f"),
                              _ptr(counts, torch.int64, "counts"), _ptr(ws, torch.uint8, "workspace"), ws.numel()))


def prdc(*args):
    check(prdc_status(*args), "pfm_prdc")


def energy_workspace_bytes(nr, nf, d, reps):
    return int(lib().pfm_energy_workspace_bytes(int(nr), int(nf), int(d), int(reps)))


def energy_status(Xr, Xf, idx_r, idx_f, reps, sums, ws):
    """enqueue `reps` replicates of the energy distance's three raw pair sums on the current stream and return the status;
    sums is a float64 view of reps * 3 elements (Srr, Sff, Srf)"""
    nr, d = Xr.shape
    nf = Xf.shape[0]
    assert Xf.shape[1] == d and idx_r.numel() == reps * nr and idx_f.numel() == reps * nf and sums.numel() == reps * 3
    return int(lib().pfm_energy(torch.cuda.current_stream().cuda_stream, _ptr(Xr, torch.float64, "X_real"), nr,
                                _ptr(Xf, torch.float64, "X_fake"), nf, d, _ptr(idx_r, torch.int32, "idx_real"),
                                _ptr(idx_f, torch.int32, "idx_fake"), int(reps), _ptr(sums, torch.float64, "sums"),
                                _ptr(ws, torch.uint8, "workspace"), ws.numel()))


def energy(*args):
    check(energy_status(*args), "pfm_energy")


def sinkhorn_workspace_bytes(nr, nf, d, reps):
    return int(lib().pfm_sinkhorn_workspace_bytes(int(nr), int(nf), int(d), int(reps)))


def sinkhorn_status(Xr, Xf, idx_r, idx_f, reps, p, eps, n_sinkhorn, value, drift, potentials, ws):
    """enqueue `reps` replicates of the debiased Sinkhorn divergence (n_sinkhorn + 1 steps) on the current stream and return
    the status; value / drift are float64 views of reps elements, potentials None or a float64 view of reps * 2 * (nr + nf)
    elements ((f, g) then (u, v) on the pooled rows)"""
    nr, d = Xr.shape
    nf = Xf.shape[0]
    assert Xf.shape[1] == d and idx_r.numel() == reps * nr and idx_f.numel() == reps * nf
    assert value.numel() == reps == drift.numel() and (potentials is None or potentials.numel() == reps * 2 * (nr + nf))
    return int(lib().pfm_sinkhorn(torch.cuda.current_stream().cuda_stream, _ptr(Xr, torch.float64, "X_real"), nr,
                                  _ptr(Xf, torch.float64, "X_fake"), nf, d, _ptr(idx_r, torch.int32, "idx_real"),
                                  _ptr(idx_f, torch.int32, "idx_fake"), int(reps), int(p), float(eps), int(n_sinkhorn),
                                  _ptr(value, torch.float64, "value"), _ptr(drift, torch.float64, "drift"),
                                  _ptr(potentials, torch.float64, "potentials", nullable=True),
                                  _ptr(ws, torch.uint8, "workspace"), ws.numel()))


def sinkhorn(*args):
    check(sinkhorn_status(*args), "pfm_sinkhorn")


def perm_labels_workspace_bytes(reps, n, n_first):
    return int(lib().pfm_perm_labels_workspace_bytes(int(reps), int(n), int(n_first)))


def perm_labels_status(seed, key_mask, first_perm, reps, n, n_first, labels, ws):
    """enqueue labellings first_perm .. first_perm + reps - 1 of n pooled rows (n_first ones each) on the current stream
    and return the status; labels is a uint8 view of reps * n elements"""
    assert labels.numel() == reps * n
    return int(lib().pfm_perm_labels(torch.cuda.current_stream().cuda_stream, int(seed), int(key_mask), int(first_perm),
                                     int(reps), int(n), int(n_first), _ptr(labels, torch.uint8, "labels"),
                                     _ptr(ws, torch.uint8, "workspace"), ws.numel()))


def perm_labels(*args):
    check(perm_labels_status(*args), "pfm_perm_labels")


def perm_form_workspace_bytes(n, d, n_first, reps):
    return int(lib().pfm_perm_form_workspace_bytes(int(n), int(d), int(n_first), int(reps)))


def perm_form_status(kind, gamma, Z, n_first, labels, reps, S, ws):
    """enqueue the signed pair sums of `reps` labellings of the pooled sample Z [n, d] on the current stream and return the
    status; labels is a uint8 view of reps * n elements, S a float64 view of reps elements"""
    n, d = Z.shape
    assert labels.numel() == reps * n and S.numel() == reps
    return int(lib().pfm_perm_form(torch.cuda.current_stream().cuda_stream, int(kind), float(gamma),
                                   _ptr(Z, torch.float64, "Z"), n, d, int(n_first), _ptr(labels, torch.uint8, "labels"),
                                   int(reps), _ptr(S, torch.float64, "S"), _ptr(ws, torch.uint8, "workspace"), ws.numel()))


def perm_form(*args):
    check(perm_form_status(*args), "pfm_perm_form")


def nn_index_workspace_bytes(n, d, k):
    return int(lib().pfm_nn_index_workspace_bytes(int(n), int(d), int(k)))


def nn_index_status(Z, k, nbr, d2, ws):
    """enqueue the k nearest other rows of every row of Z [n, d] on the current stream and return the status; nbr is an int32
    view of n * k elements (the rows, nearest first, ties by row index), d2 a float64 view of as many (their squared
    distances)"""
    n, d = Z.shape
    assert nbr.numel() == n * k == d2.numel()
    return int(lib().pfm_nn_index(torch.cuda.current_stream().cuda_stream, _ptr(Z, torch.float64, "Z"), n, d, int(k),
                                  _ptr(nbr, torch.int32, "nbr"), _ptr(d2, torch.float64, "d2"),
                                  _ptr(ws, torch.uint8, "workspace"), ws.numel()))


def nn_index(*args):
    check(nn_index_status(*args), "pfm_nn_index")


def nn_count_workspace_bytes(n, k, reps):
    return int(lib().pfm_nn_count_workspace_bytes(int(n), int(k), int(reps)))


def nn_count_status(nbr, n, k, labels, reps, counts, ws):
    """enqueue the same-label neighbour counts of `reps` labellings on the current stream and return the status; nbr is an
    int32 view of n * k elements, labels a uint8 view of reps * n, counts an int64 view of reps * 2 elements (slots with both
    labels non-zero, slots with both zero)"""
    assert nbr.numel() == n * k and labels.numel() == reps * n and counts.numel() == reps * 2
    return int(lib().pfm_nn_count(torch.cuda.current_stream().cuda_stream, _ptr(nbr, torch.int32, "nbr"), int(n), int(k),
                                  _ptr(labels, torch.uint8, "labels"), int(reps), _ptr(counts, torch.int64, "counts"),
                                  _ptr(ws, torch.uint8, "workspace"), ws.numel()))


def nn_count(*args):
    check(nn_count_status(*args), "pfm_nn_count")


def pair_grad_workspace_bytes(n, d, n_first):
    return int(lib().pfm_pair_grad_workspace_bytes(int(n), int(d), int(n_first)))


def pair_grad_status(kind, gammas, Z, n_first, value, grad, ws):
    """enqueue the value [1] and, unless grad is None, the row gradients [n, d] of the energy (PERM_ENERGY) or Gaussian-sum
    (PERM_GAUSS) statistic of the pooled sample Z [n, d] on the current stream and return the status; gammas is a sequence of
    Python floats (a host array of the C call, read before it returns)"""
    n, d = Z.shape
    assert value.numel() == 1 and (grad is None or tuple(grad.shape) == (n, d))
    g = (C.c_double * max(1, len(gammas)))(*[float(v) for v in gammas])
    return int(lib().pfm_pair_grad(torch.cuda.current_stream().cuda_stream, int(kind), C.cast(g, _VP), len(gammas),
                                   _ptr(Z, torch.float64, "Z"), n, d, int(n_first), _ptr(value, torch.float64, "value"),
                                   _ptr(grad, torch.float64, "grad", nullable=True), _ptr(ws, torch.uint8, "workspace"),
                                   ws.numel()))


def pair_grad(*args):
    check(pair_grad_status(*args), "pfm_pair_grad")


def sinkhorn_grad_workspace_bytes(n, d, n_first):
    return int(lib().pfm_sinkhorn_grad_workspace_bytes(int(n), int(d), int(n_first)))


def sinkhorn_grad_status(Z, n_first, p, eps, n_sinkhorn, value, drift, grad, potentials, ws):
    """enqueue the debiased Sinkhorn divergence of the pooled sample Z [n, d] (n_sinkhorn + 1 steps) and, unless grad is None,
    its row gradients [n, d] on the current stream and return the status; value / drift are float64 views of one element,
    potentials None or a float64 view of 2 * 2 * n elements (the last step's output, then its input)"""
    n, d = Z.shape
    assert value.numel() == 1 == drift.numel() and (grad is None or tuple(grad.shape) == (n, d))
    assert potentials is None or potentials.numel() == 4 * n
    return int(lib().pfm_sinkhorn_grad(torch.cuda.current_stream().cuda_stream, _ptr(Z, torch.float64, "Z"), n, d, int(n_first),
                                       int(p), float(eps), int(n_sinkhorn), _ptr(value, torch.float64, "value"),
                                       _ptr(drift, torch.float64, "drift"), _ptr(grad, torch.float64, "grad", nullable=True),
                                       _ptr(potentials, torch.float64, "potentials", nullable=True),
                                       _ptr(ws, torch.uint8, "workspace"), ws.numel()))


def sinkhorn_grad(*args):
    check(sinkhorn_grad_status(*args), "pfm_sinkhorn_grad")


def slice_grad_workspace_bytes(n, d, n_first, n_proj):
    return int(lib().pfm_slice_grad_workspace_bytes(int(n), int(d), int(n_first), int(n_proj)))


def slice_grad_status(p, Z, n_first, theta, n_proj, perm_in, value, rows, cols_out, perm_out, ws):
    """enqueue the sliced Wasserstein value [1] (no p-th root) of the pooled sample Z [n, d] over the directions theta [n_proj, d]
    (None: the coordinate axes, n_proj = d) and, unless rows is None, its row gradients [n, d] on the current stream and return the
    status; perm_in None (the kernel sorts, at most SLICE_LDS_ROWS rows per sample) or int32 [n_proj, n], each direction's real rows
    in order, then its fake rows; cols_out (float64) / perm_out (int32) None or [n_proj, n]: the projections and the order used"""
    n, d = Z.shape
    assert value.numel() == 1 and (rows is None or tuple(rows.shape) == (n, d))
    assert theta is None or tuple(theta.shape) == (n_proj, d)
    for t in (perm_in, cols_out, perm_out):
        assert t is None or tuple(t.shape) == (n_proj, n)
    return int(lib().pfm_slice_grad(torch.cuda.current_stream().cuda_stream, int(p), _ptr(Z, torch.float64, "Z"), n, d,
                                    int(n_first), _ptr(theta, torch.float64, "theta", nullable=True), int(n_proj),
                                    _ptr(perm_in, torch.int32, "perm_in", nullable=True), _ptr(value, torch.float64, "value"),
                                    _ptr(rows, torch.float64, "rows", nullable=True),
                                    _ptr(cols_out, torch.float64, "cols_out", nullable=True),
                                    _ptr(perm_out, torch.int32, "perm_out", nullable=True), _ptr(ws, torch.uint8, "workspace"),
                                    ws.numel()))


def slice_grad(*args):
    check(slice_grad_status(*args), "pfm_slice_grad")


def score_grad_workspace_bytes(n, K, d):
    return int(lib().pfm_score_grad_workspace_bytes(int(n), int(K), int(d)))


def score_plan_status(n, K, d):
    """-> (status, (rows per workgroup, lanes that share a row, LDS bytes, workgroups)): how pfm_score_grad tiles a call; no
    device is touched"""
    plan = (C.c_int64 * 4)()
    st = int(lib().pfm_score_plan(int(n), int(K), int(d), C.cast(plan, _VP)))
    return st, tuple(int(v) for v in plan)


def score_plan(n, K, d):
    st, plan = score_plan_status(n, K, d)
    check(st, "pfm_score_plan")
    return plan


def score_grad_status(X, Y, fair, scores, spread, grad_x, grad_y, ws):
    """enqueue the per-row energy scores [n] of the draws X [K, n, d] against the targets Y [n, d] and, where given, the spread
    [n] and the derivatives grad_x [K, n, d], grad_y [n, d] on the current stream and return the status"""
    K, n, d = X.shape
    assert tuple(Y.shape) == (n, d) and scores.numel() == n and (spread is None or spread.numel() == n)
    assert (grad_x is None or tuple(grad_x.shape) == (K, n, d)) and (grad_y is None or tuple(grad_y.shape) == (n, d))
    return int(lib().pfm_score_grad(torch.cuda.current_stream().cuda_stream, _ptr(X, torch.float64, "X_draws"),
                                    _ptr(Y, torch.float64, "Y"), n, K, d, int(bool(fair)), _ptr(scores, torch.float64, "scores"),
                                    _ptr(spread, torch.float64, "spread", nullable=True),
                                    _ptr(grad_x, torch.float64, "grad_x", nullable=True),
                                    _ptr(grad_y, torch.float64, "grad_y", nullable=True), _ptr(ws, torch.uint8, "workspace"),
                                    ws.numel()))


def score_grad(*args):
    check(score_grad_status(*args), "pfm_score_grad")


def variogram_grad_workspace_bytes(n, K, d):
    return int(lib().pfm_variogram_grad_workspace_bytes(int(n), int(K), int(d)))


def variogram_plan_status(n, K, d):
    """-> (status, (rows per workgroup, lanes that share a row, LDS bytes, workgroups, rows in flight, slices of the draws)): how
    pfm_variogram_grad tiles a call; no device is touched"""
    plan = (C.c_int64 * 6)()
    st = int(lib().pfm_variogram_plan(int(n), int(K), int(d), C.cast(plan, _VP)))
    return st, tuple(int(v) for v in plan)


def variogram_plan(n, K, d):
    st, plan = variogram_plan_status(n, K, d)
    check(st, "pfm_variogram_plan")
    return plan


def variogram_grad_status(X, Y, W, order, scores, grad_x, grad_y, ws):
    """enqueue the per-row variogram scores [n] of order 0.5, 1 or 2 of the draws X [K, n, d] against the targets Y [n, d] under the
    weights W [d, d] (None: all 1) and, where given, the derivatives grad_x [K, n, d], grad_y [n, d] on the current stream and
    return the status"""
    K, n, d = X.shape
    assert tuple(Y.shape) == (n, d) and scores.numel() == n and (W is None or tuple(W.shape) == (d, d))
    assert (grad_x is None or tuple(grad_x.shape) == (K, n, d)) and (grad_y is None or tuple(grad_y.shape) == (n, d))
    return int(lib().pfm_variogram_grad(torch.cuda.current_stream().cuda_stream, _ptr(X, torch.float64, "X_draws"),
                                        _ptr(Y, torch.float64, "Y"), _ptr(W, torch.float64, "weights", nullable=True), n, K, d,
                                        float(order), _ptr(scores, torch.float64, "scores"),
                                        _ptr(grad_x, torch.float64, "grad_x", nullable=True),
                                        _ptr(grad_y, torch.float64, "grad_y", nullable=True), _ptr(ws, torch.uint8, "workspace"),
                                        ws.numel()))


def variogram_grad(*args):
    check(variogram_grad_status(*args), "pfm_variogram_grad")


def sort_score_workspace_bytes(M, K, n_levels=0):
    return int(lib().pfm_sort_score_workspace_bytes(int(M), int(K), int(n_levels)))


def sort_score_plan_status(M, K):
    """-> (status, (series per workgroup, pitch of a series in LDS, LDS bytes, workgroups)): how pfm_sort_score tiles a call; no
    device is touched"""
    plan = (C.c_int64 * 4)()
    st = int(lib().pfm_sort_score_plan(int(M), int(K), C.cast(plan, _VP)))
    return st, tuple(int(v) for v in plan)


def sort_score_plan(M, K):
    st, plan = sort_score_plan_status(M, K)
    check(st, "pfm_sort_score_plan")
    return plan


def _levels(levels):
    """a sequence of Python floats as the HOST array of the C call (read before it returns) -> (pointer or None, count, keep-alive)"""
    arr = (C.c_double * max(1, len(levels)))(*[float(v) for v in levels])
    return (C.cast(arr, _VP) if len(levels) else None), len(levels), arr


def sort_score_status(X, Y, fair, levels, crps, grad_x, grad_y, pinball, side, idx, ws):
    """enqueue, from the sorted series of the draws X [K, M] against the targets Y [M], whichever are given of the CRPS [M], its
    derivatives grad_x [K, M] and grad_y [M], and for the sequence `levels` of Q Python floats the pinball scores [Q, M], side [Q, M]
    and idx [Q, M, 2] (int32) on the current stream and return the status"""
    K, M = X.shape
    Q = len(levels)
    assert Y.numel() == M and (crps is None or crps.numel() == M) and (grad_y is None or grad_y.numel() == M)
    assert grad_x is None or tuple(grad_x.shape) == (K, M)
    assert all(t is None or t.numel() == Q * M for t in (pinball, side)) and (idx is None or idx.numel() == 2 * Q * M)
    lp, Q, keep = _levels(levels)
    return int(lib().pfm_sort_score(torch.cuda.current_stream().cuda_stream, _ptr(X, torch.float64, "X_draws"),
                                    _ptr(Y, torch.float64, "Y"), M, K, int(bool(fair)), lp, Q,
                                    _ptr(crps, torch.float64, "crps", nullable=True),
                                    _ptr(grad_x, torch.float64, "grad_x", nullable=True),
                                    _ptr(grad_y, torch.float64, "grad_y", nullable=True),
                                    _ptr(pinball, torch.float64, "pinball", nullable=True),
                                    _ptr(side, torch.float64, "side", nullable=True), _ptr(idx, torch.int32, "idx", nullable=True),
                                    _ptr(ws, torch.uint8, "workspace"), ws.numel()))


def sort_score(*args):
    check(sort_score_status(*args), "pfm_sort_score")


def pinball_grad_status(idx, side, g, levels, K, grad_x, grad_y, ws):
    """enqueue the derivatives of sum g * pinball by the draws, grad_x [K, M], and by the targets, grad_y [M] (either may be None),
    from pfm_sort_score's idx [Q, M, 2] and side [Q, M], the incoming g [Q, M] and the same `levels`, on the current stream and
    return the status"""
    Q, M = side.shape
    assert len(levels) == Q and tuple(g.shape) == (Q, M) and idx.numel() == 2 * Q * M
    assert (grad_x is None or tuple(grad_x.shape) == (K, M)) and (grad_y is None or grad_y.numel() == M)
    lp, Q, keep = _levels(levels)
    return int(lib().pfm_pinball_grad(torch.cuda.current_stream().cuda_stream, _ptr(idx, torch.int32, "idx"),
                                      _ptr(side, torch.float64, "side"), _ptr(g, torch.float64, "g"), lp, Q, M, int(K),
                                      _ptr(grad_x, torch.float64, "grad_x", nullable=True),
                                      _ptr(grad_y, torch.float64, "grad_y", nullable=True), _ptr(ws, torch.uint8, "workspace"),
                                      ws.numel()))


def pinball_grad(*args):
    check(pinball_grad_status(*args), "pfm_pinball_grad")


def sym_eig_workspace_bytes(batch, d):
    return int(lib().pfm_sym_eig_workspace_bytes(int(batch), int(d)))


def sym_eig_status(A, w, V, sweeps, ws):
    """enqueue the eigenvalues w [batch, d] (ascending) and, where given, the eigenvectors V [batch, d, d] (columns) and the sweep
    counts [batch] (int32) of the symmetric matrices A [batch, d, d] (lower triangles read) on the current stream and return the
    status"""
    batch, d, d2 = A.shape
    assert d == d2 and tuple(w.shape) == (batch, d) and (V is None or tuple(V.shape) == (batch, d, d))
    assert sweeps is None or sweeps.numel() == batch
    return int(lib().pfm_sym_eig(torch.cuda.current_stream().cuda_stream, _ptr(A, torch.float64, "A"), batch, d,
                                 _ptr(w, torch.float64, "w"), _ptr(V, torch.float64, "V", nullable=True),
                                 _ptr(sweeps, torch.int32, "sweeps", nullable=True), _ptr(ws, torch.uint8, "workspace"), ws.numel()))


def sym_eig(*args):
    check(sym_eig_status(*args), "pfm_sym_eig")


def frechet_grad_workspace_bytes(n, d, n_first):
    return int(lib().pfm_frechet_grad_workspace_bytes(int(n), int(d), int(n_first)))


def frechet_moments(ws, d):
    """the views mean [2, d] and cov [2, d, d] of the moments a pfm_frechet_grad call left in its workspace `ws`"""
    off = (16 * d + 255) & ~255
    return ws[:16 * d].view(torch.float64).view(2, d), ws[off:off + 16 * d * d].view(torch.float64).view(2, d, d)


def frechet_grad_status(Z, n_first, rcond, sides, value, grad, parts, eig, rank, ws):
    """enqueue the Frechet distance [1] of the pooled sample Z [n, d] and, where given, its row gradients [n, d] (sides: bit 0 the
    real rows, bit 1 the fake rows), parts [5], the eigenvalues [d] and the ranks [2] (int32) on the current stream and return the
    status"""
    n, d = Z.shape
    assert value.numel() == 1 and (grad is None or tuple(grad.shape) == (n, d))
    assert (parts is None or parts.numel() == 5) and (eig is None or eig.numel() == d) and (rank is None or rank.numel() == 2)
    return int(lib().pfm_frechet_grad(torch.cuda.current_stream().cuda_stream, _ptr(Z, torch.float64, "Z"), n, d, int(n_first),
                                      float(rcond), int(sides), _ptr(value, torch.float64, "value"),
                                      _ptr(grad, torch.float64, "grad", nullable=True),
                                      _ptr(parts, torch.float64, "parts", nullable=True),
                                      _ptr(eig, torch.float64, "eig", nullable=True),
                                      _ptr(rank, torch.int32, "rank", nullable=True), _ptr(ws, torch.uint8, "workspace"),
                                      ws.numel()))


def frechet_grad(*args):
    check(frechet_grad_status(*args), "pfm_frechet_grad")
