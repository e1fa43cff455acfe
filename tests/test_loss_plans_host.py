"""The tiling decisions of the loss-gradient kernels without a GPU: tests/loss_plans.py (a Python restatement of plan_of,
launch_mode and slices_of) is pinned to the library, and then used to prove that the case lists the GPU modules are parametrised
with reach every compiled variant and every plan branch of loss_plans.SCORE_CELLS, SCORE_BRANCHES and SWEEP_CELLS.

The GPU modules are imported for their lists only (their parametrize marks are read, so a case taken out of a module is missed here
even if a helper still lists it); importing them builds nothing that is not built and touches no device.
"""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import loss_plans as lp  # noqa: E402
import native_libs  # noqa: E402
from probaforms_amd.metrics import _lib  # noqa: E402


def params(fn, name):
    """the values a test function is parametrised with for one argument"""
    found = [list(m.args[1]) for m in getattr(fn, "pytestmark", []) if m.name == "parametrize" and m.args[0] == name]
    assert len(found) == 1, (fn.__name__, name)
    return found[0]


# ---- the mirror is the library's ---------------------------------------------------------------------------------------

FEATURES = (1, 2, 4, 5, 16, 17, 33, 64, 100, 128)
ROWS = (1, 7, 3000, 70000)


def test_constants_are_the_librarys():
    assert lp.SCORE_MAX_K == _lib.SCORE_MAX_K and lp.SCORE_MAX_KD == _lib.SCORE_MAX_KD
    src = open(os.path.join(ROOT, "probaforms_amd", "metrics", "csrc", "pf_scoregrad.hip")).read()
    assert "p.U == 1 ? launch_mode<1>" in src and "p.U == 2 ? launch_mode<2>" in src and ": launch_mode<4>" in src
    assert lp.DC == 16 and "constexpr int DC = 16;" in src


def test_score_plan_equals_pfm_score_plan_for_every_k():
    native_libs.ensure_built(_lib)
    seen = 0
    for K in range(1, lp.SCORE_MAX_K + 1):
        top = lp.SCORE_MAX_KD // K
        for d in sorted({d for d in FEATURES if d <= top} | {top}):
            for n in ROWS:
                st, got = _lib.score_plan_status(n, K, d)
                p = lp.score_plan(n, K, d)
                assert st == 0 and tuple(got) == (p["R"], p["S"], p["lds"], p["wgs"]), (n, K, d, tuple(got), p)
                seen += 1
        # what the mirror derives is consistent with itself
        p = lp.score_plan(ROWS[2], K, top)
        assert p["lds"] <= lp.LDS_MAX and p["R"] % p["G"] == 0 and p["U"] <= p["tU"] <= 4 and p["S"] * p["G"] <= lp.NT
        assert (1 <= p["last_rows"] <= p["R"]) and p["rp"] >= K * top
    print("%d (n, K, d) triples agree" % seen)
    assert seen > 30000


def test_score_variant_follows_launch_mode():
    assert lp.score_variant(3, 2, False, False) == (1, 0, 1) and lp.score_variant(3, 1, True, False) == (1, 1, 1)
    assert lp.score_variant(256, 4, False, True) == (1, 1, 4) and lp.score_variant(257, 5, True, True) == (2, 1, 16)
    assert lp.score_variant(512, 16, True, True) == (2, 1, 16) and lp.score_variant(513, 17, True, True) == (4, 2, 16)
    assert lp.score_variant(769, 21, True, True) == (4, 2, 16) and lp.score_variant(1024, 1, False, False) == (4, 0, 1)
    assert len(lp.SCORE_CELLS) == 17 and len(set(lp.SCORE_CELLS)) == 17


def test_slices_equal_the_workspace_queries():
    native_libs.ensure_built(_lib)
    for n in (2, 3, 128, 500, 1160, 1473, 2200, 5000):
        for d in (1, 2, 16, 17, 33, 49):
            nb, fc, per, count = lp.slices(n, d)
            assert nb == -(-n // 64) and fc == -(-d // 16) and (count - 1) * per < nb <= count * per, (n, d)
            for n_first in (1, n - 1):
                assert _lib.pair_grad_workspace_bytes(n, d, n_first) == lp.pair_grad_bytes(n, d), (n, d)
                assert _lib.sinkhorn_grad_workspace_bytes(n, d, n_first) == lp.sinkhorn_grad_bytes(n, d), (n, d)
    assert [lp.sweep_form(d) for d in (1, 4, 5, 16, 17, 33)] == ["gf4", "gf4", "resident", "resident", "chunked", "chunked"]
    assert lp.slices(2200, 17) == (35, 2, 3, 12) and lp.slices(500, 17) == (8, 2, 1, 8)


# ---- the GPU modules' lists reach every cell -----------------------------------------------------------------------------

def reached(plan, wanted, cells, branches):
    for w in wanted:
        if isinstance(w, dict):
            assert all(plan[k] == v for k, v in w.items()), (w, plan)
        elif isinstance(w, tuple):
            assert w in cells, (w, cells)
        else:
            assert w in branches, (w, branches)


def test_score_cases_reach_every_instantiation_and_plan_branch():
    import test_score_loss_gpu as gpu
    cases = params(gpu.test_scores_spread_and_gradients_equal_the_restatement, "case")
    assert params(gpu.test_scores_spread_and_gradients_equal_the_restatement, "fair") == [False, True]
    assert len(set(cases)) == len(cases)
    # the lattice test compares both gradients bit for bit at its (K, n, 1) shapes: <2, 1, 1> is reached there, at (512, 9, 1)
    lattice = params(gpu.test_integer_valued_rows_agree_bit_for_bit, "shape")
    assert all(d == 1 for K, n, d in lattice)
    cells, branches = set(), set()
    for K, n, d in cases:
        cells |= lp.score_cells(K, n, d)
        branches |= lp.score_branches(K, n, d)
    for K, n, d in lattice:
        cells |= {c for c in lp.score_cells(K, n, d) if c[1] != "value"}
    assert [c for c in lp.SCORE_CELLS if c not in cells] == []
    assert [b for b in lp.SCORE_BRANCHES if b not in branches] == []
    for case, wanted in lp.SCORE_PATHS.items():
        assert case in cases, case
        K, n, d = case
        reached(lp.score_plan(n, K, d), wanted, lp.score_cells(K, n, d), lp.score_branches(K, n, d))
    nan = params(gpu.test_a_nan_stays_in_its_row, "case")
    position = params(gpu.test_a_rows_outputs_do_not_depend_on_n_position_or_split, "case")
    workspace = params(gpu.test_outputs_do_not_depend_on_the_workspace_and_are_all_written, "case")
    assert set(lp.SCORE_NAN_CASES) <= set(nan)
    assert set(lp.SCORE_LAYOUT_CASES) <= set(position) and set(lp.SCORE_LAYOUT_CASES) <= set(workspace)


def sweep_coverage(shapes, who):
    hit = set()
    for nr, nf, d in shapes:
        hit |= lp.sweep_cells(nr, nf, d)
    assert [c for c in lp.SWEEP_CELLS if c not in hit] == [], who
    for shape, wanted in lp.SWEEP_PATHS.items():
        assert shape in shapes, (who, shape)
        nb, fc, per, count = lp.slices(shape[0] + shape[1], shape[2])
        reached({"nb": nb, "fc": fc, "per": per, "count": count}, wanted, (), lp.sweep_cells(*shape))


def test_pair_cases_reach_every_form_of_the_sweep():
    import test_losses_gpu as gpu
    cases = params(gpu.test_value_and_gradient_equal_the_restatement, "case")
    assert params(gpu.test_value_and_gradient_equal_the_restatement, "kind") == ["energy", "gauss1", "gauss3"]
    sweep_coverage({c[:3] for c in cases if c[3] == "plain"}, "pfm_pair_grad")


def test_sinkhorn_cases_reach_every_form_of_the_sweep():
    import test_sinkhorn_loss_gpu as gpu
    configs = params(gpu.test_value_drift_and_gradient_equal_the_restatement, "cfg")
    for p in (1, 2):                                                        # each cost on its own
        sweep_coverage({c[:3] for c, q, n, reg in configs if q == p and c[3] == "plain"}, "pfm_sinkhorn_grad p=%d" % p)
        for shape in lp.SWEEP_PATHS:
            assert (shape + ("plain",), p, 2, 0.1) in configs, (shape, p)
    workspace = {c[:3] for c in params(gpu.test_outputs_do_not_depend_on_the_workspace, "case")}
    assert set(lp.SINKHORN_WORKSPACE_CASES) <= workspace and params(gpu.test_outputs_do_not_depend_on_the_workspace, "p") == [1, 2]


def test_sliced_cases_cross_row_blocks_feature_chunks_and_direction_groups():
    import test_sliced_loss_gpu as gpu
    cases = params(gpu.test_value_gradient_projections_and_order_equal_the_restatement, "case")
    assert params(gpu.test_value_gradient_projections_and_order_equal_the_restatement, "p") == [1, 2]
    assert set(lp.SLICE_CASES) <= set(cases)
    # k_slice_project: blocks of 256 rows, chunks of 16 features, groups of 8 directions
    assert any(nr + nf > 512 and d > 16 and P > 8 and P % 8 for nr, nf, d, P in cases)
    assert any(nr == 1 and nf > 1024 for nr, nf, d, P in cases) and any(nf == 1 and nr > 1024 for nr, nf, d, P in cases)
    axes = params(gpu.test_wasserstein_1d_loss_is_the_restatement_on_the_coordinate_axes, "size")
    assert set(lp.SLICE_AXES_CASES) <= set(axes) and any(nr + nf > 256 and d > 8 for nr, nf, d in axes)


def test_every_required_case_is_held_to_autograd_on_the_host():
    import test_losses_host as pair_host
    import test_score_loss_host as score_host
    import test_sinkhorn_loss_host as sinkhorn_host
    import test_sliced_loss_host as sliced_host
    held = params(score_host.test_restatement_equals_torch_autograd, "case")
    assert set(lp.SCORE_PATHS) | set(lp.SCORE_NAN_CASES) | set(lp.SCORE_LAYOUT_CASES) <= set(held)
    held = {c[:3] for c in params(pair_host.test_restatement_equals_torch_autograd, "case")}
    assert set(lp.SWEEP_PATHS) <= held
    held = {c[:3] for c in params(sinkhorn_host.test_restatement_equals_torch_autograd_of_the_last_step, "case")}
    assert set(lp.SWEEP_PATHS) <= held
    held = params(sliced_host.test_restatement_equals_torch_autograd_at_the_crossed_shapes, "case")
    assert set(lp.SLICE_CASES) | {s + (None,) for s in lp.SLICE_AXES_CASES} <= set(held)
