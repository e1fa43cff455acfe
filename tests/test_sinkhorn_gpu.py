"""probaforms_amd.metrics.sinkhorn on the GPU (pfm_sinkhorn in libpf_metrics.so) against the float64 restatement
(tests/sinkhorn_numpy.py: scipy's cdist and logsumexp on the gathered rows) and the committed fixtures
(tests/golden/sinkhorn_*.npz): value, drift and every potential entry of every replicate, through the raw binding on poisoned
outputs and workspaces and through the public calls.

The tolerance is atol = 1e-11 cmax with no rtol, cmax the largest cost between two pooled rows: each softmin carries a few ulps of
the potentials' magnitude, which cmax bounds, the averaged map is non-expansive, so 101 steps add at most about 1e-13 cmax
(tests/test_sinkhorn_host.py measures that floor on the restatement itself); the bound leaves 100 x for the device's exp and log.
The largest deviation seen is printed by test_zz_largest_deviation.

The shapes are one sweep per axis around (65, 130) rows, 3 features, p = 2, 7 steps, 3 replicates: one and two rows, ragged and
exact tile edges, more than one strip and tile per sample; one feature chunk exactly (d = 16), a second of one feature (17), a
third (33); both costs; 0, 1, 7 and 100 steps; replicate counts around the replicate block; two index groups (n_iters = 130).
"""
import functools
import glob
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, ROOT)

import hygiene  # noqa: E402
import native_libs  # noqa: E402
import sinkhorn_numpy as sn  # noqa: E402
from probaforms_amd.metrics import _boot, _lib, energy as energy_mod, sinkhorn as sk  # noqa: E402
from probaforms_amd.metrics.twosample import _median  # noqa: E402

pytestmark = pytest.mark.gpu

native_libs.ensure_built(_lib)

FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "sinkhorn_*.npz")))
REP = sk.REPLICATES["sinkhorn_divergence"]
REP_BLOCK = _lib.ENERGY_REP_BLOCK
ATOL = 1e-11                # times cmax
WORST = {"dev": 0.0, "what": None}


def fid(p):
    return os.path.basename(p)[9:-4]


def upload(ix):
    return torch.from_numpy(np.ascontiguousarray(np.stack(ix), dtype=np.int32).reshape(-1)).cuda()


def dev(A):
    return torch.from_numpy(np.ascontiguousarray(A, dtype=np.float64)).cuda()


def raw(X, Y, IX, IY, p, eps, n, ws=None, pattern="zeros", potentials=True):
    """pfm_sinkhorn through the raw binding on poisoned outputs -> (status, dict of value [reps], drift [reps], potentials
    [reps, 2, N] tensors)"""
    reps, N = len(IX), len(X) + len(Y)
    if ws is None:
        ws = hygiene.workspace(_lib.sinkhorn_workspace_bytes(len(X), len(Y), X.shape[1], reps), pattern)
    out = dict(value=torch.empty(reps, dtype=torch.float64, device="cuda"),
               drift=torch.empty(reps, dtype=torch.float64, device="cuda"))
    if potentials:
        out["potentials"] = torch.empty((reps, 2, N), dtype=torch.float64, device="cuda")
    hygiene.poison_outputs(*out.values())
    st = _lib.sinkhorn_status(dev(X), dev(Y), upload(IX), upload(IY), reps, p, eps, n, out["value"], out["drift"],
                              out.get("potentials"), ws)
    torch.cuda.synchronize()
    return st, out


def close(got, want, cm, what):
    """every output within ATOL cmax of the restatement's; S >= -ATOL cmax"""
    for key in ("value", "drift", "potentials"):
        if key not in got:
            continue
        g = got[key].cpu().numpy() if isinstance(got[key], torch.Tensor) else np.asarray(got[key])
        w = np.asarray(want[key])
        assert g.shape == w.shape and np.isfinite(g).all(), (what, key)
        dv = float(np.abs(g - w).max()) / cm
        if dv > WORST["dev"]:
            WORST.update(dev=dv, what="%s, %s" % (what, key))
        print("%s: %s deviates by at most %.3g cmax" % (what, key, dv))
        assert dv <= ATOL, (what, key, dv)
    v = got["value"].cpu().numpy() if isinstance(got["value"], torch.Tensor) else np.asarray(got["value"])
    assert (v >= -ATOL * cm).all()


@functools.lru_cache(maxsize=None)
def restated(case):
    nr, nf, d, p, n, reps = case
    X, Y = sn.data(nr, nf, d)
    IX, IY = sn.bootstrap(nr, nf, reps, sn.SEED)
    eps = sn.REG * sn.median(X, Y) ** p
    o = sn.solve_many(X, Y, IX, IY, p, eps, n)
    for a in o.values():
        a.setflags(write=False)
    return X, Y, IX, IY, eps, sn.cmax(X, Y, p), o


def check_case(case):
    nr, nf, d, p, n, reps = case
    X, Y, IX, IY, eps, cm, want = restated(case)
    st, got = raw(X, Y, IX, IY, p, eps, n)
    assert st == 0
    hygiene.assert_all_written(got, "pfm_sinkhorn")
    close(got, want, cm, str(case))
    if n == 0:
        assert float(got["drift"].abs().max()) == 0.0
    return got


@pytest.mark.parametrize("case", sn.CASES, ids=str)
def test_shapes_costs_steps_and_replicate_blocks(case):
    check_case(case)


@pytest.mark.parametrize("path", FIXTURES, ids=fid)
def test_fixtures(path):
    f = np.load(path)
    X, Y, p, eps, n = f["X"], f["Y"], int(f["p"]), float(f["eps"]), int(f["n_sinkhorn"])
    st, got = raw(X, Y, f["ix"], f["iy"], p, eps, n)
    assert st == 0
    hygiene.assert_all_written(got, "pfm_sinkhorn")
    close(got, f, sn.cmax(X, Y, p), "fixture " + fid(path))


def test_a_far_outlier_does_not_underflow():
    """one row at distance 1e3 with eps = 1e-2: exp of an unshifted term is exp(-1e5) = 0 for every column of that row, and the
    sum would be log 0"""
    f = np.load(os.path.join(GOLDEN, "sinkhorn_outlier_20_20_d2_p1.npz"))
    X, Y = f["X"], f["Y"]
    assert float(f["eps"]) == 1e-2 and np.abs(X).max() == 1000.0
    for p in (1, 2):
        want = sn.solve_many(X, Y, f["ix"], f["iy"], p, 1e-2, 7)
        st, got = raw(X, Y, f["ix"], f["iy"], p, 1e-2, 7)
        assert st == 0 and all(bool(torch.isfinite(t).all()) for t in got.values())
        close(got, want, sn.cmax(X, Y, p), "outlier, p = %d" % p)


def test_weights_all_draws_on_one_row_and_duplicated_rows():
    nr, nf, d, p, n = 65, 70, 3, 2, 7
    X, Y = sn.data(nr, nf, d)
    X[5], X[64], Y[3] = X[0], X[0], X[0]                                 # duplicated rows, within and across the samples
    eps, cm = sn.REG * sn.median(X, Y) ** p, sn.cmax(X, Y, p)
    IX, IY = sn.bootstrap(nr, nf, 3, sn.SEED + 1)
    IX[0][:], IY[0][:] = 64, 0                                           # every draw on one row (of the second strip)
    IX[1][:] = 7                                                         # one sample only
    assert (np.bincount(IX[2], minlength=nr) == 0).any()                 # natural draws leave rows out
    want = sn.solve_many(X, Y, IX, IY, p, eps, n)
    st, got = raw(X, Y, IX, IY, p, eps, n)
    assert st == 0
    hygiene.assert_all_written(got, "pfm_sinkhorn")
    close(got, want, cm, "one-row and duplicated weights")
    P = got["potentials"].cpu().numpy()
    assert np.array_equal(P[:, :, 0], P[:, :, 5]) and np.array_equal(P[:, :, 0], P[:, :, 64])    # a duplicate has the same bits


def test_a_sample_against_itself_and_symmetry():
    nr, nf, d, n = 65, 130, 3, 7
    X, Y = sn.data(nr, nf, d)
    IX, IY = sn.bootstrap(nr, nf, 2, sn.SEED + 2)
    for p in (1, 2):
        eps, cm = sn.REG * sn.median(X, Y) ** p, sn.cmax(X, Y, p)
        st, a = raw(X, Y, IX, IY, p, eps, n)
        st2, b = raw(Y, X, IY, IX, p, eps, n)
        assert st == 0 and st2 == 0
        dv = float((a["value"] - b["value"]).abs().max())
        print("p = %d: |S(X, Y) - S(Y, X)| = %.3g cmax" % (p, dv / cm))
        assert dv <= ATOL * cm and float((a["drift"] - b["drift"]).abs().max()) <= ATOL * cm
        st, s = raw(X, X.copy(), IX, IX, p, eps, n)
        assert st == 0
        print("p = %d: S(X, X) = %.3g cmax" % (p, float(s["value"].abs().max()) / cm))
        assert float(s["value"].abs().max()) <= ATOL * cm


def test_bitwise_the_same_twice_alone_and_in_groups():
    nr, nf, d, p, n = 65, 130, 3, 2, 7
    X, Y = sn.data(nr, nf, d)
    eps = sn.REG * sn.median(X, Y) ** p
    IX, IY = sn.bootstrap(nr, nf, REP_BLOCK + 1, sn.SEED + 3)
    st, g17 = raw(X, Y, IX, IY, p, eps, n)
    st2, again = raw(X, Y, IX, IY, p, eps, n, pattern="ones")
    assert st == 0 and st2 == 0
    for key in g17:
        assert hygiene.same_bits(g17[key], again[key]), key
    st, g16 = raw(X, Y, IX[1:], IY[1:], p, eps, n)                       # the same replicates at other places of a group of 16
    assert st == 0
    for key in g17:
        assert hygiene.same_bits(g16[key], g17[key][1:]), key
    for r in (0, 3, REP_BLOCK - 1, REP_BLOCK):
        st, alone = raw(X, Y, IX[r:r + 1], IY[r:r + 1], p, eps, n)
        assert st == 0
        for key in g17:
            assert hygiene.same_bits(alone[key], g17[key][r:r + 1]), (key, r)
    st, nopot = raw(X, Y, IX, IY, p, eps, n, potentials=False)          # potentials = NULL changes nothing else
    assert st == 0 and hygiene.same_bits(nopot["value"], g17["value"]) and hygiene.same_bits(nopot["drift"], g17["drift"])


@pytest.mark.parametrize("nr,nf,d,reps,n", [(50, 51, 3, 5, 7), (3, 2, 2, 4, 0), (130, 70, 17, REP_BLOCK + 1, 2)])
def test_results_do_not_depend_on_the_workspace(nr, nf, d, reps, n):
    p = 2
    X, Y = sn.data(nr, nf, d)
    IX, IY = sn.bootstrap(nr, nf, reps, 11)
    eps = sn.REG * sn.median(X, Y) ** p
    pr = (nr + 70, nf + 30, d, reps + 2)                                 # the `replay` primer: more replicates and rows
    PX, PY = sn.data(*pr[:3])
    PIX, PIY = sn.bootstrap(pr[0], pr[1], pr[3], 12)
    nbytes, pbytes = _lib.sinkhorn_workspace_bytes(nr, nf, d, reps), _lib.sinkhorn_workspace_bytes(*pr)
    outs = {}
    for pat in hygiene.PATTERNS:
        ws = hygiene.workspace(pbytes if pat == "replay" else nbytes, pat)
        if pat == "replay":
            assert raw(PX, PY, PIX, PIY, 1, 0.7, 3, ws=ws)[0] == 0
        st, outs[pat] = raw(X, Y, IX, IY, p, eps, n, ws=ws)
        assert st == 0
    hygiene.assert_all_written(outs["zeros"], "pfm_sinkhorn")
    hygiene.assert_pattern_independent(outs, "pfm_sinkhorn")
    close(outs["zeros"], sn.solve_many(X, Y, IX, IY, p, eps, n), sn.cmax(X, Y, p), "hygiene %s" % ((nr, nf, d, reps, n),))


def test_workspace_and_argument_statuses_write_nothing():
    nr, nf, d, reps = 30, 20, 2, 3
    X, Y = sn.data(nr, nf, d)
    IX, IY = sn.bootstrap(nr, nf, reps, 1)
    need = _lib.sinkhorn_workspace_bytes(nr, nf, d, reps)
    st, got = raw(X, Y, IX, IY, 2, 0.5, 3, ws=torch.empty(need - 1, dtype=torch.uint8, device="cuda"))
    assert st == _lib.PFM_EWORKSPACE and all(hygiene.poisoned(t) == t.numel() for t in got.values())
    for kw in (dict(p=3), dict(p=0)):
        st, got = raw(X, Y, IX, IY, kw["p"], 0.5, 3)
        assert st == _lib.PFM_EUNSUPPORTED and all(hygiene.poisoned(t) == t.numel() for t in got.values())
    for eps, n in ((0.0, 3), (-1.0, 3), (float("inf"), 3), (float("nan"), 3), (0.5, -1)):
        st, got = raw(X, Y, IX, IY, 2, eps, n)
        assert st == _lib.PFM_EINVAL and all(hygiene.poisoned(t) == t.numel() for t in got.values()), (eps, n)
    st, got = raw(X, Y, IX, IY, 2, 0.5, 3, ws=torch.empty(need, dtype=torch.uint8, device="cuda"))
    assert st == 0
    hygiene.assert_all_written(got, "pfm_sinkhorn")


# ---- the public calls ---------------------------------------------------------------------------------

def test_public_mean_std_replicates_and_generator_state():
    nr, nf, d, n_iters, n = 65, 63, 2, 5, 7
    X, Y = sn.data(nr, nf, d)
    for p, kw in ((2, {}), (1, dict(reg=0.3)), (2, dict(epsilon=0.8))):
        eps = kw.get("epsilon", kw.get("reg", 0.1) * sn.median(X, Y) ** p)
        cm = sn.cmax(X, Y, p)
        np.random.seed(31)
        want = sn.replicates(X, Y, n_iters, p, eps, n)
        np.random.seed(31)
        V = REP(X, Y, n_iters, p=p, n_sinkhorn=n, **kw)
        assert np.random.random() == want["next"]
        assert V.dtype == np.float64 and V.shape == (n_iters, 2)
        close(dict(value=V[:, 0], drift=V[:, 1]), want, cm, "REPLICATES p = %d %s" % (p, kw))
        np.random.seed(31)
        got = sk.sinkhorn_divergence(X, Y, n_iters=n_iters, p=p, n_sinkhorn=n, **kw)
        assert np.random.random() == want["next"]
        assert isinstance(got, tuple) and len(got) == 2 and all(isinstance(g, np.float64) for g in got)
        assert got[0].tobytes() == V[:, 0].mean().tobytes() and got[1].tobytes() == V[:, 0].std().tobytes()
        assert abs(got[0] - want["value"].mean()) <= ATOL * cm and abs(got[1] - want["value"].std()) <= ATOL * cm
    # the generator ends where energy_distance leaves it, for equal shapes and n_iters
    np.random.seed(9)
    energy_mod.energy_distance(X, Y, n_iters=7)
    nxt = np.random.random()
    np.random.seed(9)
    sk.sinkhorn_divergence(X, Y, n_iters=7, n_sinkhorn=2)
    assert np.random.random() == nxt


def test_two_index_groups_equal_the_groups_run_separately():
    nr, nf, d, p, n, n_iters = 40, 35, 3, 2, 7, _boot.MAX_GROUP + 2
    assert n_iters == 130 and _boot.group_size(n_iters, nr + nf, _lib.sinkhorn_workspace_bytes(nr, nf, d, 1)) == _boot.MAX_GROUP
    X, Y = sn.data(nr, nf, d)
    eps = 0.5
    np.random.seed(41)
    V = REP(X, Y, n_iters, p=p, epsilon=eps, n_sinkhorn=n)
    nxt = np.random.random()
    IX, IY = sn.bootstrap(nr, nf, n_iters, 41)
    assert np.random.random() == nxt
    G = _boot.MAX_GROUP
    parts = [raw(X, Y, IX[a:b], IY[a:b], p, eps, n, potentials=False)[1] for a, b in ((0, G), (G, n_iters))]
    assert np.array_equal(torch.cat([q["value"] for q in parts]).cpu().numpy(), V[:, 0])
    assert np.array_equal(torch.cat([q["drift"] for q in parts]).cpu().numpy(), V[:, 1])
    rows = [0, 1, G - 1, G, n_iters - 1]                                   # a few replicates against the restatement
    want = sn.solve_many(X, Y, IX[rows], IY[rows], p, eps, n)
    close(dict(value=V[rows, 0], drift=V[rows, 1]), want, sn.cmax(X, Y, p), "n_iters = 130")


def test_full_sample_epsilon_and_inputs():
    nr, nf, d, n = 65, 130, 3, 7
    X, Y = sn.data(nr, nf, d)
    for p, reg in ((2, 0.1), (1, 0.25)):
        cm = sn.cmax(X, Y, p)
        np.random.seed(5)
        nxt = np.random.random()
        np.random.seed(5)
        r = sk.sinkhorn_divergence_full_sample(X, Y, p=p, reg=reg, n_sinkhorn=n)
        assert np.random.random() == nxt                                 # draws nothing
        assert isinstance(r, sk.Sinkhorn) and all(isinstance(v, np.float64) for v in r)
        med = _median(dev(X), dev(Y))
        assert r.epsilon.tobytes() == (np.float64(reg) * np.float64(med) ** p).tobytes()
        assert abs(med - sn.median(X, Y)) <= 1e-12 * med
        want = sn.full_sample(X, Y, p, float(r.epsilon), n)
        close(dict(value=np.array([r.value]), drift=np.array([r.drift])), {k: np.array([want[k]]) for k in ("value", "drift")},
              cm, "full sample p = %d" % p)
        e = sk.sinkhorn_divergence_full_sample(X, Y, p=p, reg=123.0, epsilon=float(r.epsilon), n_sinkhorn=n)
        assert e.value.tobytes() == r.value.tobytes() and e.drift.tobytes() == r.drift.tobytes()      # reg is not used
        # a CUDA tensor stays on its device and gives the same bits; so do lists
        for A, B in ((dev(X), dev(Y)), (X.tolist(), Y.tolist()), (X, dev(Y))):
            c = sk.sinkhorn_divergence_full_sample(A, B, p=p, reg=reg, n_sinkhorn=n)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(c, r))
    # standardize is the call on the standardized samples
    Xs, Ys = _boot.standardize(dev(X * [3.0, 0.2, 1.0]), dev(Y * [3.0, 0.2, 1.0]))
    a = sk.sinkhorn_divergence_full_sample(X * [3.0, 0.2, 1.0], Y * [3.0, 0.2, 1.0], n_sinkhorn=n, standardize=True)
    b = sk.sinkhorn_divergence_full_sample(Xs, Ys, n_sinkhorn=n)
    assert all(u.tobytes() == v.tobytes() for u, v in zip(a, b))


def test_a_median_of_zero_and_nonfinite_cuda_input_raise_before_any_draw():
    X, Y = np.zeros((6, 2)), np.zeros((5, 2))
    Y[0] = [1.0, 2.0]
    bad = torch.zeros(9, 2, device="cuda")
    bad[2, 0] = float("inf")
    np.random.seed(3)
    want = np.random.random()
    for fn in (sk.sinkhorn_divergence, sk.sinkhorn_divergence_full_sample, REP):
        for args in ((X, Y), (bad, torch.zeros(8, 2, device="cuda"))):
            np.random.seed(3)
            with pytest.raises(ValueError):
                fn(*args)
            assert np.random.random() == want
    r = sk.sinkhorn_divergence_full_sample(X, Y, epsilon=0.5, n_sinkhorn=3)      # an explicit epsilon needs no median
    assert np.isfinite(r.value) and r.epsilon == 0.5


def test_zz_largest_deviation():
    """(runs last in this file) the largest deviation from the restatement that the tests above saw, in units of cmax"""
    print("largest deviation from the restatement: %.3g cmax (%s); bound %.3g" % (WORST["dev"], WORST["what"], ATOL))
    assert WORST["dev"] <= ATOL
