"""Every entry point of libpf_metrics.so enqueues on the caller's stream alone, returns without waiting, and can be captured
(tests/streams.py has the driver).  The cases are those of tests/test_bounds_metrics_gpu.py, reached through its own test functions
with bounds.run wrapped (streams.through_bounds): the write-bounds checks run first, unchanged, then the stream checks on the same
call.  Per entry point one case of every launch path that enqueues another kernel sequence; the grid-bound sizes (3081 / 8515 / 8385
tiles, 129 025 / 131 073 rows, PFM_NN_STAGE_MAX_N rows) are left out: which stream a launch is handed does not depend on the rows
once the path is fixed.  tests/test_streams_host.py holds CATALOGUE against the bounds module.  No form of this library is excepted:
pf_metrics.h names one host pointer, the gammas of pfm_pair_grad, "read before the call returns", which lets nothing wait.
"""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bounds  # noqa: E402
import streams  # noqa: E402
import test_bounds_metrics_gpu as tb  # noqa: E402
from probaforms_amd.metrics import _lib  # noqa: E402

pytestmark = pytest.mark.gpu

E, G = _lib.PERM_ENERGY, _lib.PERM_GAUSS
BIG = _lib.SLICE_LDS_ROWS + 1            # rows of one sample past which the caller sorts: pfm_slice_grad with perm_in


def _c(test, expect, **kwargs):
    return (test, kwargs, (expect,))


CATALOGUE = [
    _c("test_mmd", "pfm_mmd", nx=65, ny=64, d=17, reps=17), _c("test_mmd", "pfm_mmd", nx=5, ny=6, d=2, reps=3),
    # one part of the rows, two parts
    _c("test_boot_moments", "pfm_boot_moments", nr=1, nf=2, d=2, reps=17), _c("test_boot_moments", "pfm_boot_moments", nr=2049, nf=5, d=17, reps=3),
] + [   # every statistic, the histogram with its bins in LDS and in global memory
    _c("test_metric1d", "pfm_metric1d", which=which, nr=64, nf=65, d=16, reps=17) for which in tb.M1D
] + [
    _c("test_project", "pfm_project", nr=64, nf=65, d=16, P=17),
    # p = 1 and p = 2; the tables in LDS (2048 pooled rows) and in the workspace (2049)
    _c("test_wasserstein1d", "pfm_wasserstein1d", p=1, nr=64, nf=65, d=16, reps=17),
    _c("test_wasserstein1d", "pfm_wasserstein1d", p=2, nr=64, nf=65, d=17, reps=16),
    _c("test_wasserstein1d", "pfm_wasserstein1d", p=2, nr=1024, nf=1024, d=2, reps=3),
    _c("test_wasserstein1d", "pfm_wasserstein1d", p=2, nr=1025, nf=1024, d=2, reps=3),
    _c("test_wasserstein1d", "pfm_wasserstein1d", p=1, nr=1025, nf=1024, d=2, reps=3),
    _c("test_prdc", "pfm_prdc", nr=64, nf=65, d=16, reps=17, k=1), _c("test_prdc", "pfm_prdc", nr=65, nf=64, d=17, reps=17, k=16),
    _c("test_energy", "pfm_energy", nr=65, nf=64, d=17, reps=17), _c("test_energy", "pfm_energy", nr=64, nf=64, d=2, reps=128),
    # p = 1, 2, with and without potentials
    _c("test_sinkhorn", "pfm_sinkhorn", nr=64, nf=65, d=16, reps=16, p=1, pots=True),
    _c("test_sinkhorn", "pfm_sinkhorn", nr=65, nf=64, d=17, reps=17, p=2, pots=True),
    _c("test_sinkhorn", "pfm_sinkhorn", nr=1, nf=129, d=2, reps=3, p=2, pots=False),
    _c("test_perm_labels", "pfm_perm_labels", reps=17, n=64, n_first=1), _c("test_perm_labels", "pfm_perm_labels", reps=3, n=1025, n_first=1000),
    _c("test_perm_form", "pfm_perm_form", kind=E, n=65, d=17, reps=17), _c("test_perm_form", "pfm_perm_form", kind=G, n=65, d=17, reps=17),
    _c("test_perm_form", "pfm_perm_form", kind=E, n=129, d=2, reps=129),
    _c("test_nn_index", "pfm_nn_index", n=64, d=16, k=1), _c("test_nn_index", "pfm_nn_index", n=65, d=17, k=16),
    # one slice (the counts go straight to the output), two slices (partials in the workspace, a finishing launch)
    _c("test_nn_count", "pfm_nn_count", n=65, k=16, reps=129), _c("test_nn_count", "pfm_nn_count", n=4097, k=16, reps=3),
] + [   # both kinds, gradient and value alone: one slice of the sweep, several (per > 1, ragged last), the resident form
    _c("test_pair_grad", "pfm_pair_grad", kind=kind, nr=nr, nf=nf, d=d) for kind in (E, G) for nr, nf, d in ((33, 32, 17), (600, 560, 33), (1040, 1010, 5))
] + [
    _c("test_sinkhorn_grad", "pfm_sinkhorn_grad", p=p, nr=nr, nf=nf, d=d) for p in (1, 2) for nr, nf, d in ((33, 32, 17), (600, 560, 33), (1040, 1010, 5))
] + [   # sorted in LDS without perm_in, sorted by the caller with perm_in; all outputs and the value alone
    _c("test_slice_grad", "pfm_slice_grad", p=p, nr=nr, nf=nf, d=d, P=P) for p in (1, 2) for nr, nf, d, P in ((64, 65, 16, 17), (BIG, 5, 2, 2))
] + [
    _c("test_slice_grad_on_the_coordinate_axes", "pfm_slice_grad", nr=65, nf=64, d=16),
    # launch_mode<1>, <2>, <4> (K up to 256, 512, 1024), the y row outside LDS; with the gradients and the values alone
    _c("test_score_grad", "pfm_score_grad", K=16, n=65, d=16), _c("test_score_grad", "pfm_score_grad", K=300, n=5, d=17),
    _c("test_score_grad", "pfm_score_grad", K=600, n=3, d=17), _c("test_score_grad", "pfm_score_grad", K=4, n=3, d=4096),
]


def _id(case):
    return "%s-%s" % (case[0][5:], "-".join(str(v) for v in case[1].values()))


@pytest.mark.parametrize("case", CATALOGUE, ids=_id)
def test_bounds_catalogue(case):
    streams.check_catalogue(bounds, tb, case)
