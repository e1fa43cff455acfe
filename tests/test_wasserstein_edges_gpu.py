"""pfm_wasserstein1d (pf_wasserstein.hip: k_w1, k_wp<2>, merge_steps; pf_scan1d.h) at the edges of its kernels, through the raw binding
of _lib, against wasserstein_numpy.wp_pow on the constructed inputs of tests/column_cases.py.  tests/test_column_cases_host.py proves
on the host that every constructed input has the property its test here relies on.  p = 1 and p = 2 in every case.

k_wp keeps the table of a column's non-empty groups in LDS while min(G, nr) + min(G, nf) <= 2048 and in the workspace beyond, where
the merge runs in tiles of 1024 steps that hand (i, j) and the two previous breakpoints on through next[0..3]:
  full table    all-distinct (1024, 1024): the bound is 2048, LDS; (1024, 1025): 2049, workspace.  The identity fills the table
                exactly (Mr + Mf == cap: the front-filled and the back-filled halves touch); and a bootstrap draw
  ties          1500 + 1500 rows over G = 1024 distinct numbers: the bound is 2048, LDS although N > 2048 and a workspace is
                passed; over G = 1025: 2050, workspace.  For k_w1 this pair puts its last counted group G - 2 and the skipped
                group G - 1 on either side of the scan's chunk boundary
  hand-off      1500 + 1500 distinct values, index vectors that draw exactly (Mr, Mf) distinct rows: (1, 1), (512, 512), (512, 513),
                (1024, 1024), (1500, 1), (1, 1500), (1500, 1500), so T = Mr + Mf = 2, 1024, 1025, 2048, 1501, 1501, 3000 merge
                steps; the surplus draws spread evenly or all on one row; interleaved supports, and every real value below every
                fake one; and (1499, 1501) with bootstrap draws (coprime sizes)
  siblings      (1000, 1500, 2), 3 replicates, p = 2 (tables in the workspace at rf * N), and (50, 51, 3), 5 replicates, both p: each
                replicate bitwise what it gives in a launch of its own
Statuses: PFM_EUNSUPPORTED (p = 3) and PFM_EINVAL (65536 replicates, nf = 0) leave a poisoned output untouched.

Tolerance: that of tests/test_wasserstein_gpu.py, rtol 1e-12 plus atol 1e-12 spread^p, whose derivation covers N up to 3002; every
case here has N <= 3001.  Every output is handed over poisoned and every workspace filled with 0xFF bytes (NaN values, counts of -1),
so a table entry read before this launch wrote it is seen.
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
import native_libs  # noqa: E402
import wasserstein_numpy as wn  # noqa: E402
from probaforms_amd.metrics import _lib, _m1d  # noqa: E402

pytestmark = pytest.mark.gpu

native_libs.ensure_built(_lib)

RTOL = 1e-12


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def upload(rows):
    """[reps, n] index vectors -> the flat int32 device view [reps * n]"""
    return torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int32).reshape(-1)).cuda()


class Launch:
    """one case on the device: its pooled columns and index vectors, for any number of pfm_wasserstein1d calls"""

    def __init__(self, c):
        self.c = c
        self.p = _m1d.Pooled(_dev(c.X), _dev(c.Y))
        self.ix, self.iy, self.reps = upload(c.ix), upload(c.iy), len(c.ix)

    def status(self, p, nbytes=None):
        """pfm_wasserstein1d on a poisoned output and a 0xFF-filled workspace -> (status, out [reps, d])"""
        P = self.p
        if nbytes is None:
            nbytes = _lib.wasserstein1d_workspace_bytes(P.nr, P.nf, P.d, self.reps, p)
        ws = hygiene.workspace(nbytes, "ones")
        out = torch.empty((self.reps, P.d), dtype=torch.float64, device="cuda")
        hygiene.poison_outputs(out)
        st = _lib.wasserstein1d_status(p, P.cols, P.perm, P.gstart, P.ngroups, P.nr, P.nf, self.ix, self.iy, self.reps, out, ws)
        torch.cuda.synchronize()
        return st, out

    def ok(self, p):
        st, out = self.status(p)
        assert st == 0
        hygiene.assert_all_written(dict(out=out), "pfm_wasserstein1d[p=%d] %s" % (p, self.c.name))
        return out


def spread(c):
    return float(max(c.X.max(), c.Y.max()) - min(c.X.min(), c.Y.min()))


def want(c, p):
    return np.array([[wn.wp_pow(*cc.resampled(c, r, f), p) for f in range(c.X.shape[1])] for r in range(len(c.ix))])


def check(c, ps=(1, 2)):
    """W_p^p of every replicate and column against wp_pow, under the bar of tests/test_wasserstein_gpu.py"""
    assert len(c.X) + len(c.Y) <= 3001
    L = Launch(c)
    outs = {}
    for p in ps:
        outs[p] = L.ok(p)
        got, ref = outs[p].cpu().numpy(), want(c, p)
        err = np.abs(got - ref)
        print("%s p=%d: max |diff| %.3g, max relative %.3g" % (c.name, p, err.max(), (err / np.maximum(np.abs(ref), 1e-300)).max()))
        np.testing.assert_allclose(got, ref, rtol=RTOL, atol=RTOL * spread(c) ** p)
    return L, outs


@pytest.mark.parametrize("nr,nf", cc.FULL_TABLE)
def test_table_exactly_full_in_lds_and_in_the_workspace(nr, nf):
    c = cc.full_table(nr, nf)
    ws1, ws2 = (_lib.wasserstein1d_workspace_bytes(nr, nf, 1, 2, p) for p in (1, 2))
    assert (ws2 > ws1) == (nr + nf > cc.WP_LDS)                    # the host sizes a table for k_wp beyond 2048 pooled rows
    check(c)


@pytest.mark.parametrize("G", cc.TIED_G)
def test_ties_decide_where_the_table_lives(G):
    c = cc.tied(G)
    assert _lib.wasserstein1d_workspace_bytes(1500, 1500, 1, 2, 2) > _lib.wasserstein1d_workspace_bytes(1500, 1500, 1, 2, 1)
    check(c)


@pytest.mark.parametrize("apart", [False, True], ids=["mixed", "apart"])
@pytest.mark.parametrize("Mr,Mf", cc.HANDOFF)
def test_tile_hand_off(Mr, Mf, apart):
    check(cc.handoff(Mr, Mf, apart))


def test_coprime_sizes():
    check(cc.coprime())


@pytest.mark.parametrize("nr,nf,d,reps,ps", [(1000, 1500, 2, 3, (2,)), (50, 51, 3, 5, (1, 2))], ids=["workspace", "lds"])
def test_replicate_does_not_depend_on_its_siblings(nr, nf, d, reps, ps):
    c = cc.bootstrap(nr, nf, d, reps)
    _, outs = check(c, ps)
    for r in range(reps):
        one = Launch(cc.alone(c, r))
        for p in ps:
            assert hygiene.same_bits(one.ok(p)[0], outs[p][r]), "p=%d: replicate %d alone differs" % (p, r)


def test_statuses_leave_the_output_alone():
    c = cc.bootstrap(30, 20, 2, 2)
    L = Launch(c)
    st, out = L.status(3, nbytes=1 << 20)
    assert st == _lib.PFM_EUNSUPPORTED and hygiene.poisoned(out) == out.numel() == 4
    assert _lib.wasserstein1d_workspace_bytes(30, 20, 2, 2, 3) == 0
    for p in (1, 2):
        st, out = L.status(p)
        assert st == 0 and hygiene.poisoned(out) == 0

    big = 65536                                                    # one above the largest grid.y
    one = cc.Case("one-row", np.zeros((1, 1)), np.ones((1, 1)), np.zeros((big, 1), np.int32), np.zeros((big, 1), np.int32))
    B = Launch(one)
    for p in (1, 2):
        st, out = B.status(p, nbytes=1 << 20)
        assert st == _lib.PFM_EINVAL and hygiene.poisoned(out) == big
        assert _lib.wasserstein1d_workspace_bytes(1, 1, 1, big, p) == 0 < _lib.wasserstein1d_workspace_bytes(1, 1, 1, big - 1, p)

    # nf = 0: no binding builds such a call, so it is made on the library itself with real pointers
    P = L.p
    ptr = lambda t: t.data_ptr()
    for p in (1, 2):
        ws = hygiene.workspace(1 << 20, "ones")
        out = torch.empty((2, 2), dtype=torch.float64, device="cuda")
        hygiene.poison_outputs(out)
        st = _lib.lib().pfm_wasserstein1d(torch.cuda.current_stream().cuda_stream, p, ptr(P.cols), ptr(P.perm), ptr(P.gstart),
                                          ptr(P.ngroups), 30, 0, 2, ptr(L.ix), ptr(L.iy), 2, ptr(out), ptr(ws), ws.numel())
        torch.cuda.synchronize()
        assert st == _lib.PFM_EINVAL and hygiene.poisoned(out) == 4
        assert _lib.wasserstein1d_workspace_bytes(30, 0, 2, 2, p) == 0
