"""The host's tiling decisions of the loss-gradient kernels, restated in Python, and the table of compiled variants and plan
branches the GPU tests of the losses must reach between them; no GPU, no package import.

  score_plan, score_variant    plan_of and launch_mode of probaforms_amd/metrics/csrc/pf_scoregrad.hip (pfm_score_grad)
  slices, sweep_form           slices_of of pf_gradsweep.h and the template choice of k_pair_sweep (pf_pairgrad.hip) and
                               k_sinkhorn_sweep (pf_sinkgrad.hip)
  pair_grad_bytes, sinkhorn_grad_bytes    the workspace sizes those slices imply

tests/test_loss_plans_host.py pins every function here to the library (pfm_score_plan and the two workspace queries) and then uses
them to prove that the case lists of the GPU modules reach every cell of SCORE_CELLS, SCORE_BRANCHES and SWEEP_CELLS.
"""
NT = 256                         # threads of a workgroup
DC = 16                          # features of a gradient chunk
TILE = 64                        # rows per side of a pair tile
LDS_MAX = 160 * 1024
LDS_SOFT = 64 * 1024
MIN_WGS = 256
TARGET_WORKGROUPS = 1024
SCORE_MAX_K = 1024
SCORE_MAX_KD = 16384


# ---- pfm_score_grad ---------------------------------------------------------------------------------------------------

def _lds_bytes(rows, G, K, d, S, rp, y_lds):
    return 8 * (rows * rp + (rows * d if y_lds else 0) + 3 * G * K + 2 * G * S)


def score_plan(n, K, d):
    """plan_of(n, K, d) as a dict: R rows per workgroup, S lanes per row, G rows in flight, U draws per lane, tU the template's U
    (1, 2 or 4), the LDS pitches dp and rp, y_lds, the LDS bytes and the workgroups; and, derived, even_pitch (no room for odd
    pitches), g_shrunk (the LDS holds fewer rows in flight than the lanes would take), idle_lanes (S G < 256), passes (the most
    passes over G rows a workgroup of this call makes) and last_rows (the rows of the call's last workgroup)"""
    assert n >= 1 and 1 <= K <= SCORE_MAX_K and 1 <= d <= SCORE_MAX_KD // K
    S = 1
    while S < K and S < NT:
        S <<= 1
    U = -(-K // S)
    dp, y_lds = d | 1, 1
    rp = (K * dp) | 1
    even_pitch = _lds_bytes(1, 1, K, d, S, rp, 1) > LDS_MAX
    if even_pitch:
        dp, rp = d, K * d
    if _lds_bytes(1, 1, K, d, S, rp, 1) > LDS_MAX:
        y_lds = 0
    G = NT // S
    while G > 1 and _lds_bytes(G, G, K, d, S, rp, y_lds) > LDS_MAX:
        G >>= 1
    limit = LDS_SOFT if _lds_bytes(G, G, K, d, S, rp, y_lds) <= LDS_SOFT else LDS_MAX
    per_pass, aux = _lds_bytes(G, 0, K, d, S, rp, y_lds), _lds_bytes(0, G, K, d, S, rp, y_lds)
    passes = max(1, min((limit - aux) // per_pass, n // (MIN_WGS * G)))
    R = G * passes
    wgs = -(-n // R)
    return {"R": R, "S": S, "G": G, "U": U, "tU": 4 if U > 2 else U, "dp": dp, "rp": rp, "y_lds": y_lds,
            "lds": _lds_bytes(R, G, K, d, S, rp, y_lds), "wgs": wgs,
            "even_pitch": even_pitch, "g_shrunk": G < NT // S, "idle_lanes": S * G < NT,
            "passes": -(-min(n, R) // G), "last_rows": n - (wgs - 1) * R}


def score_variant(K, d, want_gx, want_gy):
    """(template U, MODE, QF) of the k_score instantiation launch_mode picks"""
    tU = score_plan(1, K, d)["tU"]
    if not (want_gx or want_gy):
        return tU, 0, 1
    if d == 1:
        return tU, 1, 1
    if d <= 4:
        return tU, 1, 4
    if d <= DC:
        return tU, 1, DC
    return tU, 2, DC


FORMS = {(0, 1): "value", (1, 1): "qf1", (1, 4): "qf4", (1, DC): "qf16", (2, DC): "chunked"}
# the 15 instantiations, and the chunked one at U = 4 with all four draw slots of a lane live and with one masked
SCORE_CELLS = [(tU, form) for tU in (1, 2, 4) for form in ("value", "qf1", "qf4", "qf16", "chunked")]
SCORE_CELLS += [(4, "chunked, four slots live"), (4, "chunked, a masked slot")]
SCORE_BRANCHES = ["y_lds == 0", "y_lds == 1, G == 1, idle lanes", "G shrunk, G > 1 left", "even pitch, chunked",
                  "several passes, chunked", "last workgroup has fewer rows than G"]


def score_cells(K, n, d):
    """the cells of SCORE_CELLS a (K, n, d) case reaches when it is run with both gradients and once for the value alone"""
    tU, mode, qf = score_variant(K, d, True, True)
    cells = {(tU, "value"), (tU, FORMS[mode, qf])}
    if tU == 4 and mode == 2:
        cells.add((4, "chunked, four slots live" if K > 3 * NT else "chunked, a masked slot"))
    return cells


def score_branches(K, n, d):
    """the entries of SCORE_BRANCHES a (K, n, d) case reaches with both gradients asked for"""
    p = score_plan(n, K, d)
    chunked = d > DC
    hit = {"y_lds == 0": not p["y_lds"],
           "y_lds == 1, G == 1, idle lanes": p["y_lds"] and p["G"] == 1 and p["idle_lanes"],
           "G shrunk, G > 1 left": p["g_shrunk"] and p["G"] > 1,
           "even pitch, chunked": p["even_pitch"] and chunked,
           "several passes, chunked": p["passes"] > 1 and chunked,
           "last workgroup has fewer rows than G": p["last_rows"] < p["G"]}
    assert set(hit) == set(SCORE_BRANCHES)
    return {name for name, yes in hit.items() if yes}


# ---- the pair sweeps: pfm_pair_grad, pfm_sinkhorn_grad --------------------------------------------------------------

def slices(n, d):
    """slices_of(n, d): (tiles per side, feature chunks, column tiles per slice, slices)"""
    nb = -(-n // TILE)
    fc = -(-d // DC)
    want = min(max(-(-TARGET_WORKGROUPS // (nb * fc)), 1), nb)
    per = -(-nb // want)
    return nb, fc, per, -(-nb // per)


def sweep_form(d):
    """which sweep a feature count gets: four features in registers, one chunk resident in LDS, or chunks re-staged per tile"""
    return "gf4" if d <= 4 else "resident" if d <= DC else "chunked"


def _align256(b):
    return (b + 255) & ~255


def pair_grad_bytes(n, d):
    nb, fc, per, count = slices(n, d)
    return _align256(8 * nb * count) + _align256(8 * count * n * d)


def sinkhorn_grad_bytes(n, d):
    nb, fc, per, count = slices(n, d)
    return 3 * _align256(8 * 2 * n) + _align256(8 * count * n * d)


SWEEP_CELLS = ["gf4, per > 1", "resident, per > 1", "chunked, per > 1", "chunked, fc >= 3, per > 1", "ragged last slice"]


def sweep_cells(nr, nf, d):
    """the entries of SWEEP_CELLS a sweep over nr + nf pooled rows of d features reaches"""
    nb, fc, per, count = slices(nr + nf, d)
    form = sweep_form(d)
    hit = set()
    if per > 1:
        hit.add(form + ", per > 1")
        if form == "chunked" and fc >= 3:
            hit.add("chunked, fc >= 3, per > 1")
    if count * per > nb:
        hit.add("ragged last slice")
    assert hit <= set(SWEEP_CELLS)
    return hit


# ---- the cases the GPU modules must hold, and the path each was chosen for ---------------------------------------------
# tests/test_loss_plans_host.py checks that each is in its module's parametrised list and that the functions above say it reaches
# what stands here: a cell of SCORE_CELLS, an entry of SCORE_BRANCHES or of SWEEP_CELLS, or a field of score_plan

SCORE_PATHS = {                          # (K, n, d)
    (300, 3, 16): [(2, "qf16")],
    (300, 3, 17): [(2, "chunked")],
    (512, 3, 32): [(2, "chunked"), {"lds": 151816}],
    (600, 3, 1): [(4, "qf1"), {"U": 3}],
    (1024, 3, 1): [(4, "qf1"), {"U": 4}],
    (600, 3, 17): [(4, "chunked, a masked slot")],
    (770, 3, 21): [(4, "chunked, four slots live"), {"lds": 152112}],
    (1, 3, 16384): ["y_lds == 0", "even pitch, chunked"],
    (2, 3, 8192): ["y_lds == 0", "even pitch, chunked"],
    (4, 3, 4096): ["y_lds == 0", "even pitch, chunked"],
    (5, 3, 3276): ["y_lds == 1, G == 1, idle lanes", {"S": 8, "even_pitch": False}],
    (64, 9, 100): ["G shrunk, G > 1 left", "last workgroup has fewer rows than G", {"G": 2, "last_rows": 1}],
    (16, 40, 100): ["G shrunk, G > 1 left", {"G": 8}],
    (128, 3, 128): [{"g_shrunk": True, "G": 1}],
    (33, 2051, 17): ["several passes, chunked", {"passes": 2}],
}
SCORE_NAN_CASES = [(300, 7, 17), (4, 7, 4096)]
SCORE_LAYOUT_CASES = [(300, 5, 17), (4, 3, 4096)]          # position independence; workspace, with one gradient alone
SWEEP_PATHS = {                          # (nr, nf, d), for pfm_pair_grad and for pfm_sinkhorn_grad
    (760, 713, 17): ["chunked, per > 1"],
    (600, 560, 33): ["chunked, fc >= 3, per > 1", "ragged last slice", {"fc": 3, "per": 2, "count": 10}],
    (1040, 1010, 5): ["resident, per > 1"],
    (1, 130, 2): [{"nb": 3}],
    (130, 1, 17): [{"nb": 3, "fc": 2}],
}
SINKHORN_WORKSPACE_CASES = [(760, 713, 17), (600, 560, 33)]
SLICE_CASES = [(300, 250, 17, 9), (1, 1025, 2, 3), (1025, 1, 2, 3)]          # (nr, nf, d, P)
SLICE_AXES_CASES = [(300, 250, 17)]
