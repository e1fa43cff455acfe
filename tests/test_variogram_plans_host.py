"""The tiling decisions of pfm_variogram_grad without a GPU: tests/variogram_plans.py (a Python restatement of plan_of and
launch_mode of pf_variogram.hip) is pinned to the library, and then used to prove that the case list tests/test_variogram_loss_gpu.py
is parametrised with reaches every compiled variant and every plan branch of variogram_plans.CELLS and BRANCHES.

The GPU module is imported for its lists only (its parametrize marks are read, so a case taken out of the module is missed here even
if a helper still lists it); importing it builds nothing that is not built and touches no device.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import native_libs  # noqa: E402
import variogram_plans as vp  # noqa: E402
from probaforms_amd.metrics import _lib  # noqa: E402

FEATURES = (1, 2, 3, 4, 5, 15, 16, 17, 22, 23, 33, 48, 49, 63, 64)
ROWS = (1, 7, 3000, 70000)


def params(fn, name):
    """the values a test function is parametrised with for one argument"""
    found = [list(m.args[1]) for m in getattr(fn, "pytestmark", []) if m.name == "parametrize" and m.args[0] == name]
    assert len(found) == 1, (fn.__name__, name)
    return found[0]


def test_constants_are_the_librarys():
    assert (vp.MAX_K, vp.MAX_KD, vp.MAX_D) == (_lib.SCORE_MAX_K, _lib.SCORE_MAX_KD, _lib.VARIO_MAX_D)
    src = open(os.path.join(ROOT, "probaforms_amd", "metrics", "csrc", "pf_variogram.hip")).read()
    assert "constexpr int DC = 16;" in src and vp.DC == 16
    assert "order == 0.5 ? launch_mode<0>" in src and "order == 1.0 ? launch_mode<1>" in src and ": launch_mode<2>" in src
    assert "if (!a.gx) return launch<ORDER, 0>" in src and "a.d <= DC ? launch<ORDER, 1>(st, p, a) : launch<ORDER, 2>" in src
    assert "if (d == 1) {" in src and "k_vario_d1" in src


def test_plan_equals_pfm_variogram_plan_for_every_k():
    native_libs.ensure_built(_lib)
    seen, largest = 0, 0
    for K in range(1, vp.MAX_K + 1):
        top = min(vp.MAX_D, vp.MAX_KD // K)
        for d in sorted({d for d in FEATURES if d <= top} | {top}):
            for n in ROWS:
                st, got = _lib.variogram_plan_status(n, K, d)
                p = vp.plan(n, K, d)
                assert st == 0 and got == vp.as_tuple(p), (n, K, d, got, p)
                seen += 1
                # what the mirror derives is consistent with itself, and every shape within the limits fits one CU's LDS
                assert p["lds"] <= vp.LDS_MAX and p["R"] % p["G"] == 0 and p["S"] * p["G"] <= vp.NT and 1 <= p["last_rows"] <= p["R"]
                assert p["T"] == 1 or p["T"] * p["P"] <= p["S"], (n, K, d, p)     # the slice sums of a row: at most one per lane
                largest = max(largest, p["lds"])
    print("%d (n, K, d) triples agree; the largest workgroup takes %d bytes of LDS" % (seen, largest))
    assert seen > 30000


def test_variant_follows_launch_mode():
    assert vp.variant(1, True) == vp.variant(1, False) == "d1"
    assert [vp.variant(d, True) for d in (2, 16, 17, 64)] == [1, 1, 2, 2] and [vp.variant(d, False) for d in (2, 16, 17, 64)] == [0] * 4
    assert len(vp.CELLS) == 12 and len(set(vp.CELLS)) == 12


def test_gpu_cases_reach_every_instantiation_and_plan_branch():
    import test_variogram_loss_gpu as gpu
    cases = params(gpu.test_scores_and_gradients_equal_the_restatement, "case")
    assert params(gpu.test_scores_and_gradients_equal_the_restatement, "order") == list(vp.ORDERS)
    assert len(set(cases)) == len(cases)
    # what the issue lists
    for K in (1, 2, 3, 31, 32, 33, 63, 64, 65, 257, 1024):
        assert (K, 7, 3) in cases, K
    for d in (1, 2, 3, 4, 5, 15, 16, 17, 33, 63, 64):
        assert (33, 7, d) in cases, d
    R = vp.plan(1, 3, 3)["R"]
    for n in (1, 2, R - 1, R, R + 1, 3 * R + 1):
        assert (3, n, 3) in cases, n
    assert (1024, 3, 16) in cases and (256, 3, 64) in cases
    # every K and every d at which the lanes per row or the rows in flight change, and the value one above
    at_k, at_d = vp.changes_in_k(3), vp.changes_in_d(3)
    assert {2, 3, 5, 9, 17, 33, 65, 129} <= set(at_k) and len(at_d) >= 4
    for K in at_k:
        assert (K, 7, 3) in cases, K
    for d in at_d + vp.changes_in_d(33):
        assert (3, 7, d) in cases or (33, 7, d) in cases, d
    assert any(vp.plan(n, K, d)["passes"] > 1 for K, n, d in cases)
    cells, branches = set(), set()
    for K, n, d in cases:
        for order in vp.ORDERS:
            cells |= vp.cells(K, n, d, order)
        branches |= vp.branches(K, n, d)
    assert [c for c in vp.CELLS if c not in cells] == []
    assert [b for b in vp.BRANCHES if b not in branches] == []
    for case, wanted in vp.PATHS.items():
        assert case in cases, case
        K, n, d = case
        p, hit = vp.plan(n, K, d), vp.branches(K, n, d)
        for w in wanted:
            if isinstance(w, dict):
                assert all(p[k] == v for k, v in w.items()), (case, w, p)
            else:
                assert w in hit, (case, w, hit)
    # the write-bounds and stream tests: one packed shape and one workgroup-per-row shape
    for fn in (gpu.test_no_write_outside_the_workspace_and_the_outputs, gpu.test_everything_is_enqueued_on_the_callers_stream):
        shapes = params(fn, "case")
        assert any(vp.plan(n, K, d)["G"] > 1 for K, n, d in shapes) and any(vp.plan(n, K, d)["S"] == vp.NT for K, n, d in shapes)
