"""No entry point of libpf_metrics.so writes outside its workspace or its outputs (tests/bounds.py has the driver, tests/hygiene.py
the guard bands).  Every call gets a workspace of exactly its own *_workspace_bytes() and every output a guarded buffer of its own;
the driver also requires status 0, all outputs written, inputs unchanged and the bits of a run on a plain workspace, and prints the
workspace's high-water mark.  Correctness against the references stays in the entry points' own test modules.

entry point (size function)                         cases (rows real, rows fake, ...)
  pfm_mmd (pfm_mmd_workspace_bytes)                 MMD_CASES: one tile and a row more, d 16 / 17, 16 / 17 replicates;
                                                    (2465, 2464, 2, 1): 3081 tiles, so MMD_TARGET_WG = 3072 workgroups bound the grid
  pfm_boot_moments (pfm_moments_workspace_bytes)    MOMENT_CASES: 2048 / 2049 rows (one part, two), d 16 / 17;
                                                    (129025, 7, 3, 1) and (131073, 7, 2, 1): 64 = MAX_PARTS parts, at and past the bound
  pfm_metric1d (pfm_metric1d_workspace_bytes)       every statistic at M1D_CASES (the extremes, the last sub-buffer, are kept by KDE
                                                    only)
  pfm_project (no workspace)                        PROJECT_CASES: output and inputs
  pfm_wasserstein1d (..._workspace_bytes)           p = 1, 2; 2048 / 2049 pooled rows without ties (WP_LDS: the tables of a column with
                                                    more than 2048 entries move to the workspace)
  pfm_prdc (pfm_prdc_workspace_bytes)               64 / 65 rows either side, k = 1 and 16 (PFM_KNN_MAX_K), 17 replicates
  pfm_energy (pfm_energy_workspace_bytes)           64 / 65 rows, 16 / 17 and 128 / 129 replicates; (4097, 4097, 2, 1): 8515 tiles,
                                                    lists of 5 tiles (TARGET_WGS = 2048 reached), a ragged last list per block
  pfm_sinkhorn (pfm_sinkhorn_workspace_bytes)       64 / 65 rows, 16 / 17 replicates, p = 1, 2, with and without potentials
  pfm_perm_labels (keeps nothing)                   64 / 65 / 1025 rows, 17 and 129 labellings: no interior byte may change
  pfm_perm_form (pfm_perm_form_workspace_bytes)     both kinds, 64 / 65 rows, 16 / 17 / 129 labellings; 8193 rows: 8385 tiles, lists of 5
  pfm_nn_index (keeps nothing)                      k = 1 and 16 (PFM_NN_MAX_K), 64 / 65 rows, d 16 / 17: no interior byte may change
  pfm_nn_count (pfm_nn_count_workspace_bytes)       n = 262144 / 262145 (PFM_NN_STAGE_MAX_N: one slice of 4 n slots, five of 65536),
                                                    k = 1; 4097 rows, k = 16: two slices, the last ragged
  pfm_pair_grad (pfm_pair_grad_workspace_bytes)     both kinds, loss_plans.SWEEP_PATHS (slices_of at its TARGET_WORKGROUPS bound:
                                                    per > 1, ragged last slice), value alone
  pfm_sinkhorn_grad (..._workspace_bytes)           the same SWEEP_PATHS, p = 1, 2, with potentials; value alone
  pfm_slice_grad (pfm_slice_grad_workspace_bytes)   loss_plans.SLICE_CASES; 13312 / 13313 rows (PFM_SLICE_LDS_ROWS: sorted in LDS, and
                                                    with perm_in); the coordinate axes; value alone; every optional output
  pfm_score_grad (keeps nothing)                    loss_plans.SCORE_LAYOUT_CASES and two plan edges: no interior byte may change

Read from the size functions: pfm_perm_labels, pfm_nn_index and pfm_score_grad return a constant least allocation and their kernels take
no workspace pointer, so their high-water mark must be 0.  No grid bound is left out: each is reached in well under a second.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bounds  # noqa: E402
import hygiene  # noqa: E402
import loss_plans as lp  # noqa: E402
import native_libs  # noqa: E402
from bounds import Out  # noqa: E402
from probaforms_amd.metrics import _lib, _m1d  # noqa: E402

pytestmark = pytest.mark.gpu

native_libs.ensure_built(_lib)

F64, I32, I64, U8 = torch.float64, torch.int32, torch.int64, torch.uint8
TILE, NT = 64, 256


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _sample(n, d, seed, shift=0.0, ties=True):
    """rows rounded to two decimals (ties and duplicates, as the metrics' own tests draw them), or as drawn"""
    x = torch.randn(n, d, dtype=F64, device="cuda", generator=_gen(seed)) * 1.2 + shift
    return x.mul(100).round().div(100).contiguous() if ties else x.contiguous()


def _draws(n, reps, seed):
    return torch.randint(0, n, (reps * n,), dtype=I32, device="cuda", generator=_gen(seed))


def _two(nr, nf, d, reps, seed, ties=True):
    return _sample(nr, d, seed, 0.0, ties), _sample(nf, d, seed + 1, 0.3, ties), _draws(nr, reps, seed + 2), _draws(nf, reps, seed + 3)


def _tiles(n):
    return -(-n // TILE)


def _quad_plan(na, nb):
    """plan_of of pf_quadform.h: (tiles per list, first[4])"""
    ta, tb = _tiles(na), _tiles(nb)
    nt = (ta * (ta + 1) // 2, tb * (tb + 1) // 2, ta * tb)
    per = max(4, -(-sum(nt) // 2048))
    first = [0]
    for q in range(3):
        first.append(first[-1] + -(-nt[q] // per))
    return per, first


# ---- pfm_mmd, pfm_boot_moments -------------------------------------------------------------------------------------------------
MMD_CASES = [(64, 64, 16, 16), (65, 64, 17, 17), (5, 6, 2, 3), (2465, 2464, 2, 1)]


def _mmd_wg(m, reps):
    T = _tiles(m) * (_tiles(m) + 1) // 2
    return max(1, max(min(-(-3072 // reps), T), -(-T // 65536)))


@pytest.mark.parametrize("nx,ny,d,reps", MMD_CASES)
def test_mmd(nx, ny, d, reps):
    X, Y, ix, iy = _two(nx, ny, d, reps, 5)
    wg = _mmd_wg(nx + ny, reps)
    if nx > 2000:
        assert wg == 3072 < _tiles(nx + ny) * (_tiles(nx + ny) + 1) // 2        # the grid's bound, tiles left over
    bounds.run("pfm_mmd[%d+%d rows, d %d, %d replicates]" % (nx, ny, d, reps), _lib.mmd_workspace_bytes(nx, ny, d, reps),
               lambda ws, o: _lib.mmd_status(X, Y, ix, iy, reps, o["median"], o["mmd"], ws),
               dict(median=Out(F64, (reps,)), mmd=Out(F64, (reps,))), dict(X=X, Y=Y, idx_x=ix, idx_y=iy), last=8 * 3 * wg * reps)


MOMENT_CASES = [(2048, 2049, 16, 2), (2049, 5, 17, 3), (1, 2, 2, 17), (129025, 7, 3, 1), (131073, 7, 2, 1)]


@pytest.mark.parametrize("nr,nf,d,reps", MOMENT_CASES)
def test_boot_moments(nr, nf, d, reps):
    X, Y, ix, iy = _two(nr, nf, d, reps, 7)
    parts = min(64, max(1, -(-max(nr, nf) // 2048)))
    bounds.run("pfm_boot_moments[%d+%d rows, d %d, %d replicates]" % (nr, nf, d, reps), _lib.moments_workspace_bytes(nr, nf, d, reps),
               lambda ws, o: _lib.boot_moments_status(X, Y, ix, iy, reps, o["mean"], o["cov"], ws),
               dict(mean=Out(F64, (reps, 2, d)), cov=Out(F64, (reps, 2, d, d))), dict(X=X, Y=Y, idx_r=ix, idx_f=iy),
               last=8 * 2 * reps * parts * (d * (d + 1) // 2), allow=("cov",) if min(nr, nf) < 2 else ())   # np.cov of one row: NaN


# ---- pfm_metric1d, pfm_project, pfm_wasserstein1d ---------------------------------------------------------------------------
M1D = {"ks": (_lib.M1D_KS, 1), "cvm": (_lib.M1D_CVM, 1), "ad": (_lib.M1D_AD, 1), "auc": (_lib.M1D_AUC, 1),
       "hist_lds": (_lib.M1D_HIST, 10), "hist_glob": (_lib.M1D_HIST, 3000), "kde": (_lib.M1D_KDE, 101)}
M1D_CASES = [(64, 65, 16, 17), (1025, 1024, 17, 2), (2, 3, 1, 129)]


@pytest.mark.parametrize("nr,nf,d,reps", M1D_CASES)
@pytest.mark.parametrize("which", list(M1D))
def test_metric1d(which, nr, nf, d, reps):
    metric, bins = M1D[which]
    X, Y, ix, iy = _two(nr, nf, d, reps, 11)
    p = _m1d.Pooled(X, Y)
    tail, dtype = _m1d.OUT_SHAPE[metric]
    shape = (reps, p.d) + tuple(bins if t is None else t for t in tail)
    h = (_m1d.silverman(p.nr), _m1d.silverman(p.nf)) if metric == _lib.M1D_KDE else (1.0, 1.0)
    keeps_extremes = metric == _lib.M1D_KDE                     # k_scan1d hands the extremes to k_kde; the histograms use them in place
    bounds.run("pfm_metric1d[%s, %d+%d rows, d %d, %d replicates]" % (which, nr, nf, d, reps),
               _lib.metric1d_workspace_bytes(metric, nr, nf, d, reps, bins),
               lambda ws, o: _lib.metric1d_status(metric, p.cols, p.perm, p.gstart, p.ngroups, p.nr, p.nf, ix, iy, reps, bins, h[0], h[1],
                                                  o["out"], ws),
               dict(out=Out(dtype, shape)), dict(cols=p.cols, perm=p.perm, gstart=p.gstart, ngroups=p.ngroups, idx_r=ix, idx_f=iy),
               last=8 * 2 * reps * d if keeps_extremes else None)


PROJECT_CASES = [(64, 65, 16, 17), (1, 2, 17, 1), (1025, 1023, 3, 129)]


@pytest.mark.parametrize("nr,nf,d,P", PROJECT_CASES)
def test_project(nr, nf, d, P):
    X, Y = _sample(nr, d, 3), _sample(nf, d, 4)
    theta = torch.randn(P, d, dtype=F64, device="cuda", generator=_gen(9))
    bounds.run_outputs("pfm_project[%d+%d rows, d %d, %d directions]" % (nr, nf, d, P), lambda o: _lib.project(X, Y, theta, o["cols"]),
                       dict(cols=Out(F64, (P, nr + nf))), dict(X=X, Y=Y, theta=theta))


W1D_CASES = [(1, 64, 65, 16, 17), (2, 64, 65, 17, 16), (2, 1024, 1024, 2, 3), (2, 1025, 1024, 2, 3), (1, 1025, 1024, 2, 3)]


@pytest.mark.parametrize("p,nr,nf,d,reps", W1D_CASES)
def test_wasserstein1d(p, nr, nf, d, reps):
    N = nr + nf
    X, Y, ix, iy = _two(nr, nf, d, reps, 13, ties=N <= 2048)    # past WP_LDS every row its own tie group: min(G, nr) + min(G, nf) = N
    pl = _m1d.Pooled(X, Y)
    tables = p != 1 and N > 2048                                # values [reps, d, N], then cumulative counts [reps, d, N]
    if N > 2048:
        assert int(pl.ngroups.min()) == N
    bounds.run("pfm_wasserstein1d[p %d, %d+%d rows, d %d, %d replicates]" % (p, nr, nf, d, reps),
               _lib.wasserstein1d_workspace_bytes(nr, nf, d, reps, p),
               lambda ws, o: _lib.wasserstein1d_status(p, pl.cols, pl.perm, pl.gstart, pl.ngroups, nr, nf, ix, iy, reps, o["out"], ws),
               dict(out=Out(F64, (reps, d))), dict(cols=pl.cols, perm=pl.perm, gstart=pl.gstart, ngroups=pl.ngroups, idx_r=ix, idx_f=iy),
               last=4 * reps * d * N if tables else 4 * reps * N)


# ---- pfm_prdc, pfm_energy, pfm_sinkhorn -------------------------------------------------------------------------------------
PRDC_CASES = [(64, 65, 16, 17, 1), (65, 64, 17, 17, 16), (129, 18, 2, 16, 16), (18, 129, 2, 3, 1)]


@pytest.mark.parametrize("nr,nf,d,reps,k", PRDC_CASES)
def test_prdc(nr, nf, d, reps, k):
    X, Y, ix, iy = _two(nr, nf, d, reps, 17)
    bounds.run("pfm_prdc[%d+%d rows, d %d, %d replicates, k %d]" % (nr, nf, d, reps, k), _lib.prdc_workspace_bytes(nr, nf, d, reps, k),
               lambda ws, o: _lib.prdc_status(X, Y, ix, iy, reps, k, o["radius2_r"], o["radius2_f"], o["counts"], ws),
               dict(radius2_r=Out(F64, (reps, nr)), radius2_f=Out(F64, (reps, nf)), counts=Out(I64, (reps, 4))),
               dict(X=X, Y=Y, idx_r=ix, idx_f=iy), last=4 * 2 * reps * _tiles(nr))


ENERGY_CASES = [(64, 65, 16, 16), (65, 64, 17, 17), (64, 64, 2, 128), (65, 1, 2, 129), (4097, 4097, 2, 1)]


@pytest.mark.parametrize("nr,nf,d,reps", ENERGY_CASES)
def test_energy(nr, nf, d, reps):
    X, Y, ix, iy = _two(nr, nf, d, reps, 19)
    per, first = _quad_plan(nr, nf)
    if nr > 4000:
        assert per == 5 and first[3] == 429 + 429 + 845         # lists grown past MIN_LIST: the TARGET_WGS regime, ragged last lists
    bounds.run("pfm_energy[%d+%d rows, d %d, %d replicates]" % (nr, nf, d, reps), _lib.energy_workspace_bytes(nr, nf, d, reps),
               lambda ws, o: _lib.energy_status(X, Y, ix, iy, reps, o["sums"], ws),
               dict(sums=Out(F64, (reps, 3))), dict(X=X, Y=Y, idx_r=ix, idx_f=iy), last=8 * reps * first[3])


SINKHORN_CASES = [(64, 65, 16, 16, 1, True), (65, 64, 17, 17, 2, True), (1, 129, 2, 3, 2, False), (16, 16, 2, 1, 1, True)]


@pytest.mark.parametrize("nr,nf,d,reps,p,pots", SINKHORN_CASES)
def test_sinkhorn(nr, nf, d, reps, p, pots):
    X, Y, ix, iy = _two(nr, nf, d, reps, 23)
    outs = dict(value=Out(F64, (reps,)), drift=Out(F64, (reps,)))
    if pots:
        outs["potentials"] = Out(F64, (reps, 2, nr + nf))
    bounds.run("pfm_sinkhorn[%d+%d rows, d %d, %d replicates, p %d]" % (nr, nf, d, reps, p), _lib.sinkhorn_workspace_bytes(nr, nf, d, reps),
               lambda ws, o: _lib.sinkhorn_status(X, Y, ix, iy, reps, p, 0.5, 3, o["value"], o["drift"], o.get("potentials"), ws),
               outs, dict(X=X, Y=Y, idx_r=ix, idx_f=iy), last=8 * 2 * reps * (nr + nf))          # pot[2]: the last step's output


def test_the_detector_sees_a_write_behind_a_shortened_workspace():
    """pfm_sinkhorn writes all of pot[2], the end of its workspace, in every call: a handle told that the interior ends 256 bytes
    earlier must report those writes.  The call itself owns every byte it is given."""
    nr = nf = 16
    reps = 1
    X, Y, ix, iy = _two(nr, nf, 2, reps, 29)
    need = _lib.sinkhorn_workspace_bytes(nr, nf, 2, reps)
    assert 8 * 2 * reps * (nr + nf) == 512                       # pot[2] ends at the workspace's end, no alignment tail behind it
    for fill in bounds.FILLS:
        h = hygiene.guarded(need, fill)
        ws = h.view
        value, drift = torch.empty(1, dtype=F64, device="cuda"), torch.empty(1, dtype=F64, device="cuda")
        _lib.sinkhorn(X, Y, ix, iy, reps, 2, 0.5, 3, value, drift, None, ws)
        torch.cuda.synchronize()
        h.assert_guards_intact("pfm_sinkhorn on its true size")
        h.retract(256)                                           # the call still gets all `need` bytes
        _lib.sinkhorn(X, Y, ix, iy, reps, 2, 0.5, 3, value, drift, None, ws)
        torch.cuda.synchronize()
        with pytest.raises(AssertionError, match=r"wrote behind its %d bytes: \d+ guard bytes changed, the first at end\+\d+, the last at end\+255$"
                           % (need - 256)):
            h.assert_guards_intact("pfm_sinkhorn, told 256 bytes less")


# ---- pfm_perm_labels, pfm_perm_form, pfm_nn_index, pfm_nn_count ---------------------------------------------------------------
LABEL_CASES = [(17, 64, 1), (129, 65, 64), (3, 1025, 1000)]         # (labellings, rows, rows of the first sample)


@pytest.mark.parametrize("reps,n,n_first", LABEL_CASES)
def test_perm_labels(reps, n, n_first):
    bounds.run("pfm_perm_labels[%d labellings, %d rows]" % (reps, n), _lib.perm_labels_workspace_bytes(reps, n, n_first),
               lambda ws, o: _lib.perm_labels_status(12345, _lib.KEY_MASK_ALL, 7, reps, n, n_first, o["labels"], ws),
               dict(labels=Out(U8, (reps, n))), {}, keeps_nothing=True)


def _labels(reps, n, n_first, seed):
    lab = torch.empty(reps, n, dtype=U8, device="cuda")
    _lib.perm_labels(seed, _lib.KEY_MASK_ALL, 0, reps, n, n_first, lab, hygiene.workspace(_lib.perm_labels_workspace_bytes(reps, n, n_first), "zeros"))
    return lab


FORM_CASES = [(64, 16, 16), (65, 17, 17), (129, 2, 129), (8193, 2, 1)]       # (rows, features, labellings)


@pytest.mark.parametrize("kind", [_lib.PERM_ENERGY, _lib.PERM_GAUSS])
@pytest.mark.parametrize("n,d,reps", FORM_CASES)
def test_perm_form(kind, n, d, reps):
    Z, n_first = _sample(n, d, 31), n // 3 + 1
    lab = _labels(reps, n, n_first, 77)
    per, first = _quad_plan(n, 0)
    if n > 8000:
        assert per == 5 and first[1] == 1677                      # 8385 tiles: the lists have grown to hold TARGET_WGS
    bounds.run("pfm_perm_form[kind %d, %d rows, d %d, %d labellings]" % (kind, n, d, reps), _lib.perm_form_workspace_bytes(n, d, n_first, reps),
               lambda ws, o: _lib.perm_form_status(kind, 0.7, Z, n_first, lab, reps, o["S"], ws),
               dict(S=Out(F64, (reps,))), dict(Z=Z, labels=lab), last=8 * reps * first[1])


INDEX_CASES = [(64, 16, 1), (65, 17, 16), (17, 2, 16), (1025, 3, 7)]            # (rows, features, k)


@pytest.mark.parametrize("n,d,k", INDEX_CASES)
def test_nn_index(n, d, k):
    Z = _sample(n, d, 37)
    bounds.run("pfm_nn_index[%d rows, d %d, k %d]" % (n, d, k), _lib.nn_index_workspace_bytes(n, d, k),
               lambda ws, o: _lib.nn_index_status(Z, k, o["nbr"], o["d2"], ws),
               dict(nbr=Out(I32, (n, k)), d2=Out(F64, (n, k))), dict(Z=Z), keeps_nothing=True)


COUNT_CASES = [(64, 1, 17), (65, 16, 129), (4097, 16, 3), (_lib.NN_STAGE_MAX_N, 1, 2), (_lib.NN_STAGE_MAX_N + 1, 1, 2)]   # (rows, k, labellings)


def _count_slices(n, k):
    per = 1 << 16
    if n <= _lib.NN_STAGE_MAX_N and 4 * n > per:
        per = 4 * n
    per = max(per, -(-n * k // 65535))
    return -(-n * k // per)


@pytest.mark.parametrize("n,k,reps", COUNT_CASES)
def test_nn_count(n, k, reps):
    nbr = torch.randint(0, n, (n, k), dtype=I32, device="cuda", generator=_gen(41))
    lab = _labels(reps, n, n // 2, 78)
    slices = _count_slices(n, k)
    assert slices == {64: 1, 65: 1, 4097: 2, _lib.NN_STAGE_MAX_N: 1, _lib.NN_STAGE_MAX_N + 1: 5}[n]
    bounds.run("pfm_nn_count[%d rows, k %d, %d labellings]" % (n, k, reps), _lib.nn_count_workspace_bytes(n, k, reps),
               lambda ws, o: _lib.nn_count_status(nbr, n, k, lab, reps, o["counts"], ws),
               dict(counts=Out(I64, (reps, 2))), dict(nbr=nbr, labels=lab), last=8 * 2 * reps * slices if slices > 1 else None,
               keeps_nothing=slices == 1)                       # one slice: its counts are the labelling's, written straight to `counts`


# ---- the loss gradients: pfm_pair_grad, pfm_sinkhorn_grad, pfm_slice_grad, pfm_score_grad -------------------------------------
SWEEPS = sorted(lp.SWEEP_PATHS) + [(64, 1, 16), (33, 32, 17)]


@pytest.mark.parametrize("kind", [_lib.PERM_ENERGY, _lib.PERM_GAUSS])
@pytest.mark.parametrize("nr,nf,d", SWEEPS)
def test_pair_grad(kind, nr, nf, d):
    n = nr + nf
    Z = _sample(n, d, 43)
    nb, fc, per, count = lp.slices(n, d)
    need = _lib.pair_grad_workspace_bytes(n, d, nr)
    gam = (0.3, 1.1, 2.0)
    bounds.run("pfm_pair_grad[kind %d, %d+%d rows, d %d]" % (kind, nr, nf, d), need,
               lambda ws, o: _lib.pair_grad_status(kind, gam, Z, nr, o["value"], o["grad"], ws),
               dict(value=Out(F64, (1,)), grad=Out(F64, (n, d))), dict(Z=Z), last=8 * count * n * d)
    hw, _ = bounds.run("pfm_pair_grad[kind %d, %d+%d rows, d %d, value alone]" % (kind, nr, nf, d), need,
                       lambda ws, o: _lib.pair_grad_status(kind, gam, Z, nr, o["value"], None, ws), dict(value=Out(F64, (1,))), dict(Z=Z))
    assert hw <= bounds.align256(8 * nb * count)                  # without a gradient only the value partials are kept


@pytest.mark.parametrize("p", [1, 2])
@pytest.mark.parametrize("nr,nf,d", SWEEPS)
def test_sinkhorn_grad(p, nr, nf, d):
    n = nr + nf
    Z = _sample(n, d, 47)
    nb, fc, per, count = lp.slices(n, d)
    need = _lib.sinkhorn_grad_workspace_bytes(n, d, nr)
    bounds.run("pfm_sinkhorn_grad[p %d, %d+%d rows, d %d]" % (p, nr, nf, d), need,
               lambda ws, o: _lib.sinkhorn_grad_status(Z, nr, p, 0.5, 2, o["value"], o["drift"], o["grad"], o["potentials"], ws),
               dict(value=Out(F64, (1,)), drift=Out(F64, (1,)), grad=Out(F64, (n, d)), potentials=Out(F64, (2, 2, n))), dict(Z=Z),
               last=8 * count * n * d)
    hw, _ = bounds.run("pfm_sinkhorn_grad[p %d, %d+%d rows, d %d, value alone]" % (p, nr, nf, d), need,
                       lambda ws, o: _lib.sinkhorn_grad_status(Z, nr, p, 0.5, 2, o["value"], o["drift"], None, None, ws),
                       dict(value=Out(F64, (1,)), drift=Out(F64, (1,))), dict(Z=Z))
    assert hw <= 3 * bounds.align256(8 * 2 * n)                   # the three potential buffers


SLICES = list(lp.SLICE_CASES) + [(64, 65, 16, 17), (_lib.SLICE_LDS_ROWS, 5, 2, 2), (_lib.SLICE_LDS_ROWS + 1, 5, 2, 2)]


@pytest.mark.parametrize("p", [1, 2])
@pytest.mark.parametrize("nr,nf,d,P", SLICES)
def test_slice_grad(p, nr, nf, d, P):
    n = nr + nf
    Z = _sample(n, d, 53)
    theta = torch.randn(P, d, dtype=F64, device="cuda", generator=_gen(59))
    inputs = dict(Z=Z, theta=theta)
    perm_in = None
    if max(nr, nf) > _lib.SLICE_LDS_ROWS:                         # the caller sorts: each direction's real rows in order, then its fake rows
        u = theta @ Z.t()
        perm_in = torch.cat([torch.argsort(u[:, :nr], dim=1, stable=True), nr + torch.argsort(u[:, nr:], dim=1, stable=True)], dim=1).to(I32).contiguous()
        inputs["perm_in"] = perm_in
    need = _lib.slice_grad_workspace_bytes(n, d, nr, P)
    last = 8 * P * -(-n // NT)
    tag = "pfm_slice_grad[p %d, %d+%d rows, d %d, %d directions%s" % (p, nr, nf, d, P, ", perm_in" if perm_in is not None else "")
    bounds.run(tag + "]", need,
               lambda ws, o: _lib.slice_grad_status(p, Z, nr, theta, P, perm_in, o["value"], o["rows"], o["cols_out"], o["perm_out"], ws),
               dict(value=Out(F64, (1,)), rows=Out(F64, (n, d)), cols_out=Out(F64, (P, n)), perm_out=Out(I32, (P, n))), inputs, last=last)
    bounds.run(tag + ", value alone]", need,
               lambda ws, o: _lib.slice_grad_status(p, Z, nr, theta, P, perm_in, o["value"], None, None, None, ws),
               dict(value=Out(F64, (1,))), inputs, last=last)


@pytest.mark.parametrize("nr,nf,d", lp.SLICE_AXES_CASES + [(65, 64, 16)])
def test_slice_grad_on_the_coordinate_axes(nr, nf, d):
    n = nr + nf
    Z = _sample(n, d, 61)
    bounds.run("pfm_slice_grad[axes, %d+%d rows, d %d]" % (nr, nf, d), _lib.slice_grad_workspace_bytes(n, d, nr, d),
               lambda ws, o: _lib.slice_grad_status(2, Z, nr, None, d, None, o["value"], o["rows"], o["cols_out"], o["perm_out"], ws),
               dict(value=Out(F64, (1,)), rows=Out(F64, (n, d)), cols_out=Out(F64, (d, n)), perm_out=Out(I32, (d, n))), dict(Z=Z),
               last=8 * d * -(-n // NT))


SCORES = list(lp.SCORE_LAYOUT_CASES) + [(64, 9, 100), (33, 2051, 17), (16, 65, 16), (17, 64, 17)]       # (K, n, d)


@pytest.mark.parametrize("K,n,d", SCORES)
def test_score_grad(K, n, d):
    X = torch.randn(K, n, d, dtype=F64, device="cuda", generator=_gen(67))
    Y = torch.randn(n, d, dtype=F64, device="cuda", generator=_gen(71))
    need = _lib.score_grad_workspace_bytes(n, K, d)
    bounds.run("pfm_score_grad[%d draws, %d rows, d %d]" % (K, n, d), need,
               lambda ws, o: _lib.score_grad_status(X, Y, True, o["scores"], o["spread"], o["grad_x"], o["grad_y"], ws),
               dict(scores=Out(F64, (n,)), spread=Out(F64, (n,)), grad_x=Out(F64, (K, n, d)), grad_y=Out(F64, (n, d))), dict(X=X, Y=Y),
               keeps_nothing=True)
    bounds.run("pfm_score_grad[%d draws, %d rows, d %d, values alone]" % (K, n, d), need,
               lambda ws, o: _lib.score_grad_status(X, Y, False, o["scores"], None, None, None, ws),
               dict(scores=Out(F64, (n,))), dict(X=X, Y=Y), keeps_nothing=True)
