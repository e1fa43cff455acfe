"""The host's tiling decisions of pfm_variogram_grad (plan_of and launch_mode of probaforms_amd/metrics/csrc/pf_variogram.hip),
restated in Python, and the table of compiled variants and plan branches the GPU test of variogram_score_loss must reach; no GPU, no
package import.  tests/test_variogram_plans_host.py pins plan() to pfm_variogram_plan and then uses it to prove that the case list of
tests/test_variogram_loss_gpu.py reaches every cell of CELLS and every entry of BRANCHES.
"""
NT = 256                         # threads of a workgroup
DC = 16                          # features of a gradient chunk
LDS_MAX = 160 * 1024
LDS_SOFT = 64 * 1024
MIN_WGS = 256
MAX_K = 1024
MAX_KD = 16384
MAX_D = 64
ORDERS = (0.5, 1, 2)


def _lds_bytes(rows, G, d, S, rp, tp, pp):
    return 8 * (rows * (rp + d) + G * (tp + pp + S))


def plan(n, K, d):
    """plan_of(n, K, d) as a dict: R rows per workgroup, S lanes per row, G rows in flight, T slices of the draws, P pairs, the LDS
    pitches, the LDS bytes and the workgroups; and, derived, g_shrunk (the LDS holds fewer rows in flight than the lanes would
    take), idle_lanes (S G < 256), passes (the most passes over G rows a workgroup of this call makes), last_rows (the rows of the
    call's last workgroup), draws_per_lane and pair_rounds (how often a row's pairs go round its lanes)"""
    assert n >= 1 and 1 <= K <= MAX_K and 1 <= d <= min(MAX_D, MAX_KD // K)
    if d == 1:
        wgs = -(-n // NT)
        return {"R": NT, "S": 1, "G": NT, "T": 1, "P": 0, "lds": 0, "wgs": wgs, "g_shrunk": False, "idle_lanes": False, "passes": 1,
                "last_rows": n - (wgs - 1) * NT, "draws_per_lane": K, "pair_rounds": 0}
    S = 1
    while S < K and S < NT:
        S <<= 1
    P = d * (d - 1) // 2
    T = min(S // P if P < S else 1, K)
    per_slice = -(-K // T)
    T = -(-K // per_slice)
    dp = d | 1
    rp = (K * dp) | 1
    tp = P | 1
    pp = (T * P) | 1 if T > 1 else 0
    G = NT // S
    while G > 1 and _lds_bytes(G, G, d, S, rp, tp, pp) > LDS_MAX:
        G >>= 1
    limit = LDS_SOFT if _lds_bytes(G, G, d, S, rp, tp, pp) <= LDS_SOFT else LDS_MAX
    per_pass, aux = _lds_bytes(G, 0, d, S, rp, tp, pp), _lds_bytes(0, G, d, S, rp, tp, pp)
    passes = max(1, min((limit - aux) // per_pass, n // (MIN_WGS * G)))
    R = G * passes
    wgs = -(-n // R)
    return {"R": R, "S": S, "G": G, "T": T, "P": P, "dp": dp, "rp": rp, "tp": tp, "pp": pp, "lds": _lds_bytes(R, G, d, S, rp, tp, pp),
            "wgs": wgs, "g_shrunk": G < NT // S, "idle_lanes": S * G < NT, "passes": -(-min(n, R) // G),
            "last_rows": n - (wgs - 1) * R, "draws_per_lane": -(-K // S), "pair_rounds": -(-P * T // S)}


def as_tuple(p):
    """what pfm_variogram_plan writes"""
    return p["R"], p["S"], p["lds"], p["wgs"], p["G"], p["T"]


def variant(d, want_gx):
    """which kernel launch_mode picks: 'd1' (k_vario_d1), or MODE 0 (no grad_x), 1 (d <= 16, through the image), 2 (chunks)"""
    if d == 1:
        return "d1"
    if not want_gx:
        return 0
    return 1 if d <= DC else 2


# the 9 instantiations of k_vario, by (order, MODE), and k_vario_d1
CELLS = [(order, mode) for order in ORDERS for mode in (0, 1, 2)] + [(order, "d1") for order in ORDERS]
BRANCHES = ["one slice", "several slices", "several slices, the last shorter", "pairs go round the lanes more than once",
            "a lane owns several draws", "G shrunk", "idle lanes", "several passes", "several passes, chunked",
            "last workgroup has fewer rows than G", "one feature chunk with a ragged end", "several feature chunks, the last ragged",
            "a full last chunk", "one draw", "one lane per row"]


def cells(K, n, d, order):
    """the cells a (K, n, d) case of one order reaches when it is run with both gradients and once for the value alone"""
    return {(order, variant(d, True)), (order, variant(d, False))}


def branches(K, n, d):
    """the entries of BRANCHES a (K, n, d) case reaches with both gradients asked for"""
    if d == 1:
        return set()
    p = plan(n, K, d)
    per_slice = -(-K // p["T"])
    hit = {"one slice": p["T"] == 1,
           "several slices": p["T"] > 1,
           "several slices, the last shorter": p["T"] > 1 and p["T"] * per_slice > K,
           "pairs go round the lanes more than once": p["pair_rounds"] > 1,
           "a lane owns several draws": p["draws_per_lane"] > 1,
           "G shrunk": p["g_shrunk"],
           "idle lanes": p["idle_lanes"],
           "several passes": p["passes"] > 1,
           "several passes, chunked": p["passes"] > 1 and d > DC,
           "last workgroup has fewer rows than G": p["last_rows"] < p["G"],
           "one feature chunk with a ragged end": d < DC,
           "several feature chunks, the last ragged": d > DC and d % DC != 0,
           "a full last chunk": d % DC == 0,
           "one draw": K == 1,
           "one lane per row": p["S"] == 1}
    assert set(hit) == set(BRANCHES)
    return {name for name, yes in hit.items() if yes}


def packing(K, d):
    """(lanes per row, rows in flight) of a shape: what the case list follows along K and along d"""
    p = plan(1, K, d)
    return p["S"], p["G"]


def changes_in_k(d):
    """every K at which the packing changes at d features, and the value one above"""
    top = min(MAX_K, MAX_KD // d)
    at = [K for K in range(2, top + 1) if packing(K, d) != packing(K - 1, d)]
    return sorted(set(at) | {K + 1 for K in at if K + 1 <= top})


def changes_in_d(K):
    """every d at which the packing changes at K draws, and the value one above"""
    top = min(MAX_D, MAX_KD // K)
    at = [d for d in range(3, top + 1) if packing(K, d) != packing(K, d - 1)]
    return sorted(set(at) | {d + 1 for d in at if d + 1 <= top})


# the cases the GPU module must hold beside its axes, and what each was chosen for (a field of plan(), or an entry of BRANCHES)
PATHS = {                                # (K, n, d)
    (1024, 3, 16): [{"S": 256, "G": 1, "T": 2, "draws_per_lane": 4}, "a lane owns several draws", "a full last chunk"],
    (256, 3, 64): [{"S": 256, "G": 1, "T": 1, "P": 2016, "lds": 151824}, "pairs go round the lanes more than once"],
    (33, 2051, 3): ["several passes", {"passes": 2}],
    (33, 2051, 17): ["several passes, chunked", {"passes": 2}],
    (129, 769, 3): ["several passes", {"S": 256, "G": 1, "passes": 3}],
    (3, 7, 64): ["G shrunk", "idle lanes", "last workgroup has fewer rows than G"],
    (1, 7, 3): ["one draw", "one lane per row"],
}
