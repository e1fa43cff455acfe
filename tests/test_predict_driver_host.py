"""models/_predict.py's reduce_draws -- the one driver behind sample_many / sample_stats / sample_scores / sample_joint_scores of
all four models -- on CPU tensors: a recording source in place of the kernels' launches and a stand-in for the _predict_lib
module.  What is pinned: which (row chunk, draw window) pairs are launched, in which order and on which slices; that every
chunk walks the same K draws; where torch's generator stands afterwards; and where a partial chunk's results land."""
import collections

import numpy as np
import pytest
import torch

from probaforms_amd.models import _predict as P

N, D, K, WIDTH = 5, 3, 7, 2
CHUNKS = [(0, 2), (2, 2), (4, 1)]
WINDOWS = [(0, 3), (3, 3), (6, 1)]


def value(k, r, j):
    """what the recording source writes for draw k of row r, column j"""
    return 1000.0 * k + 10.0 * r + j


@pytest.fixture
def small_budgets(monkeypatch):
    monkeypatch.setattr(P, "XT_CHUNK_BYTES", 2 * D * K * 4)              # chunks of 2 rows
    monkeypatch.setattr(P, "Z_WINDOW_BYTES", 3 * N * WIDTH * 4)          # windows of 3 draws
    assert P.quantile_row_chunks(N, D, K, P.XT_CHUNK_BYTES) == CHUNKS
    assert P.draw_windows(K, N, WIDTH, P.Z_WINDOW_BYTES) == WINDOWS


Launch = collections.namedtuple("Launch", "lo m k_lo k_cnt noise state x_out xt")


class NoiseSource(P.WindowedSource):
    """a source in the style of the host prior and the generator jobs: windows of torch.randn noise"""

    def __init__(self):
        self.device, self.d, self.width = torch.device("cpu"), D, WIDTH
        self.launches, self.brackets = [], []

    def begin(self):
        self.brackets.append("begin")

    def end(self):
        self.brackets.append("end")

    def noise(self, k_cnt):
        return torch.stack([torch.randn(self.n, self.width) for _ in range(k_cnt)])

    def launch(self, lo, m, zw, k_lo, k_cnt, state, x_out, xt):
        self.launches.append(Launch(lo, m, k_lo, k_cnt, zw.clone(), state, x_out, xt))
        v = torch.tensor([[[value(k, r, j) for j in range(D)] for r in range(lo, lo + m)] for k in range(k_lo, k_lo + k_cnt)])
        if state is not None:
            assert tuple(state.shape[:2]) == (m, D)
            state[:, :, 0] += k_cnt                                     # "count"
            state[:, :, 1] += v.sum(dim=0)
        if x_out is not None:
            assert tuple(x_out.shape) == (k_cnt, m, D)                  # the kernels write rows 0 .. m of [k_cnt, m, d]
            x_out.copy_(v)
        if xt is not None:
            assert tuple(xt.shape) == (m, D, self.K)
            xt[:, :, k_lo:k_lo + k_cnt] = v.permute(1, 2, 0)


class SeedSource:
    """a source in the style of the device prior: K seeds from torch's generator, one launch per chunk"""

    def __init__(self):
        self.device, self.d = torch.device("cpu"), D
        self.seeds, self.launches, self.closed = None, [], 0

    def open(self, n, K):
        self.seeds = [int(torch.empty((), dtype=torch.int64).random_().item()) for _ in range(K)]

    def draw(self, lo, m, state, x_out, xt):
        self.launches.append((lo, m))

    def close(self):
        self.closed += 1


class Lib:
    """stands in for the _predict_lib module: records its calls and writes recognisable values"""

    def __init__(self):
        self.calls = []
        self.state = None

    def new_state(self, n, d, device):
        self.state = torch.zeros((n, d, 6))
        return self.state

    def finalize(self, state, n, d, ddof, mean, std, mn, mx):
        self.calls.append(("finalize", n, d, ddof))
        assert state is self.state
        mean.copy_(state[:, :, 1] / state[:, :, 0])
        std.fill_(float(ddof)); mn.fill_(-1.0); mx.fill_(1.0)

    def quantiles(self, xt, m, d, K, probs, out):
        self.calls.append(("quantiles", m, d, K))
        assert out.is_contiguous() and tuple(out.shape) == (len(probs), m, d) and probs.dtype == torch.float64
        for i, p in enumerate(probs.tolist()):
            out[i] = xt[:, :, 0] + p

    def scores(self, xt, Y, m, d, K, fair, probs, crps, pit, q, pb):
        self.calls.append(("scores", m, d, K, fair))
        assert tuple(Y.shape) == (m, d) and tuple(crps.shape) == (m, d)
        crps.copy_(xt[:, :, 0] + Y)
        pit.copy_(xt[:, :, K - 1])
        if probs is not None:
            assert q.is_contiguous() and pb.is_contiguous()
            for i, p in enumerate(probs.tolist()):
                q[i] = xt[:, :, 0] + p
                pb[i] = -(xt[:, :, 0] + p)

    def joint_scores(self, xt, Y, m, d, K, fair, order, energy, spread, variogram):
        self.calls.append(("joint_scores", m, d, K, fair, order))
        assert tuple(energy.shape) == (m,)
        energy.copy_(xt[:, 0, 0])
        spread.copy_(Y[:, 0])
        if variogram is not None:
            variogram.copy_(xt[:, D - 1, K - 1])


def first_draw():
    """[n, d]: value(0, r, j)"""
    return torch.tensor([[value(0, r, j) for j in range(D)] for r in range(N)])


def state_after_k_draws(seed):
    torch.manual_seed(seed)
    for _ in range(K):
        torch.randn(N, WIDTH)
    return torch.get_rng_state()


def test_every_chunk_and_window_is_launched_once_in_order_on_its_own_slices(small_budgets):
    src, lib = NoiseSource(), Lib()
    torch.manual_seed(11)
    stats, draws = P.reduce_draws(src, N, K, (0.25, 0.5), 1, True, False, lib=lib)
    assert draws is None
    assert [(l.lo, l.m, l.k_lo, l.k_cnt) for l in src.launches] == [(lo, m, k_lo, k_cnt) for lo, m in CHUNKS for k_lo, k_cnt in WINDOWS]
    assert src.brackets == ["begin", "end"] * len(CHUNKS)
    for l in src.launches:
        assert l.x_out is None
        assert l.state.data_ptr() == lib.state[l.lo:l.lo + l.m].data_ptr() and l.state.shape[0] == l.m
    for lo, m in CHUNKS:                                                 # one xt per chunk, shared by its windows
        xts = {l.xt.data_ptr() for l in src.launches if l.lo == lo}
        assert len(xts) == 1
    assert torch.equal(lib.state[:, :, 0], torch.full((N, D), float(K)))  # every (row, draw) folded exactly once
    assert lib.calls == [("quantiles", 2, D, K), ("quantiles", 2, D, K), ("quantiles", 1, D, K), ("finalize", N, D, 1)]
    mean = torch.tensor([[np.mean([value(k, r, j) for k in range(K)]) for j in range(D)] for r in range(N)], dtype=torch.float32)
    assert torch.equal(stats.mean, mean) and torch.equal(stats.std, torch.ones(N, D))
    assert tuple(stats.quantiles.shape) == (2, N, D)
    assert torch.equal(stats.quantiles[0], first_draw() + 0.25) and torch.equal(stats.quantiles[1], first_draw() + 0.5)


def test_every_chunk_walks_the_same_draws_and_the_generator_ends_after_k_draws(small_budgets):
    src = NoiseSource()
    torch.manual_seed(5)
    P.reduce_draws(src, N, K, (0.5,), 0, True, False, lib=Lib())
    after = torch.get_rng_state()
    assert torch.equal(after, state_after_k_draws(5))
    torch.manual_seed(5)
    ref = torch.stack([torch.randn(N, WIDTH) for _ in range(K)])
    for lo, _ in CHUNKS:
        got = torch.cat([l.noise for l in src.launches if l.lo == lo])
        assert torch.equal(got, ref)


def test_one_chunk_keeps_the_draws_and_never_rewinds(small_budgets, monkeypatch):
    monkeypatch.setattr(torch, "set_rng_state", lambda s: pytest.fail("one chunk: nothing to rewind"))
    src = NoiseSource()
    torch.manual_seed(3)
    stats, draws = P.reduce_draws(src, N, K, None, 0, False, True, lib=Lib())
    assert stats is None and tuple(draws.shape) == (K, N, D)
    assert [(l.lo, l.m, l.k_lo, l.k_cnt) for l in src.launches] == [(0, N, k_lo, k_cnt) for k_lo, k_cnt in WINDOWS]
    for l in src.launches:
        assert l.state is None and l.xt is None and l.x_out.data_ptr() == draws[l.k_lo:l.k_lo + l.k_cnt].data_ptr()
    want = torch.tensor([[[value(k, r, j) for j in range(D)] for r in range(N)] for k in range(K)])
    assert torch.equal(draws, want)
    assert torch.equal(torch.get_rng_state(), state_after_k_draws(3))


def test_draws_with_more_than_one_chunk_are_refused(small_budgets):
    with pytest.raises(AssertionError):
        P.reduce_draws(NoiseSource(), N, K, (0.5,), 0, True, True, lib=Lib())


def test_no_rows_only_a_seed_source_takes_from_the_generator(small_budgets):
    torch.manual_seed(9)
    start = torch.get_rng_state()
    src, lib = NoiseSource(), Lib()
    stats, draws = P.reduce_draws(src, 0, K, (0.5,), 0, True, True, lib=lib)
    assert torch.equal(torch.get_rng_state(), start) and src.launches == [] and src.brackets == []
    assert tuple(stats.mean.shape) == (0, D) and tuple(stats.quantiles.shape) == (1, 0, D) and tuple(draws.shape) == (K, 0, D)
    assert lib.calls == []
    seeds = SeedSource()
    P.reduce_draws(seeds, 0, K, None, 0, True, False, lib=Lib())
    assert len(seeds.seeds) == K and seeds.launches == [] and seeds.closed == 1
    torch.manual_seed(9)
    assert seeds.seeds == [int(torch.empty((), dtype=torch.int64).random_().item()) for _ in range(K)]
    assert not torch.equal(torch.get_rng_state(), start)


def test_a_seed_source_is_opened_once_and_launched_once_per_chunk(small_budgets):
    seeds = SeedSource()
    torch.manual_seed(2)
    P.reduce_draws(seeds, N, K, (0.5,), 0, True, False, lib=Lib())
    after = torch.get_rng_state()
    assert seeds.launches == CHUNKS and seeds.closed == 1
    torch.manual_seed(2)
    for _ in range(K):
        torch.empty((), dtype=torch.int64).random_()
    assert torch.equal(after, torch.get_rng_state())                     # the rewinds between chunks put back what open() left


def test_scores_of_a_partial_chunk_land_in_its_rows(small_budgets):
    src, lib = NoiseSource(), Lib()
    Y = np.arange(N * D, dtype=np.float64).reshape(N, D) / 8.0
    torch.manual_seed(1)
    res, draws = P.reduce_draws(src, N, K, (0.1, 0.9), 0, False, False, scores=(Y, True), lib=lib)
    assert draws is None and isinstance(res, P.SampleScores)
    assert lib.calls == [("scores", 2, D, K, True), ("scores", 2, D, K, True), ("scores", 1, D, K, True)]
    assert all(l.state is None and l.x_out is None for l in src.launches)
    Yt = torch.from_numpy(Y).float()
    assert torch.equal(res.crps, first_draw() + Yt)
    assert torch.equal(res.pit, first_draw() + 1000.0 * (K - 1))
    for i, p in enumerate((0.1, 0.9)):
        assert torch.equal(res.quantiles[i], first_draw() + p) and torch.equal(res.pinball[i], -(first_draw() + p))
    res, _ = P.reduce_draws(NoiseSource(), N, K, None, 0, False, False, scores=(Y, False), lib=Lib())
    assert res.quantiles is None and res.pinball is None and torch.equal(res.crps, first_draw() + Yt)


def test_joint_scores_of_a_partial_chunk_land_in_its_rows(small_budgets):
    lib = Lib()
    Y = torch.arange(N * D, dtype=torch.float32).reshape(N, D)
    res, draws = P.reduce_draws(NoiseSource(), N, K, None, 0, False, False, joint=(Y, False, 0.5), lib=lib)
    assert draws is None and isinstance(res, P.JointScores)
    assert lib.calls == [("joint_scores", m, D, K, False, 0.5) for _, m in CHUNKS]
    assert torch.equal(res.energy, first_draw()[:, 0]) and torch.equal(res.spread, Y[:, 0])
    assert torch.equal(res.variogram, first_draw()[:, D - 1] + 1000.0 * (K - 1))
    res, _ = P.reduce_draws(NoiseSource(), N, K, None, 0, False, False, joint=(Y, True, None), lib=Lib())
    assert res.variogram is None


@pytest.mark.parametrize("path", ["scores", "joint"])
def test_targets_of_the_wrong_shape_raise_before_anything_is_drawn(path, small_budgets):
    src = NoiseSource()
    torch.manual_seed(4)
    start = torch.get_rng_state()
    kw = dict(scores=(np.zeros((N, D + 1)), False)) if path == "scores" else dict(joint=(np.zeros((N, D + 1)), False, 0.5))
    with pytest.raises(ValueError) as e:
        P.reduce_draws(src, N, K, None, 0, False, False, lib=Lib(), **kw)
    assert str(e.value) == "Y must have shape (5, 3) (one target per condition row and column), got (5, 4)"
    assert src.launches == [] and torch.equal(torch.get_rng_state(), start)


def test_end_runs_when_a_window_raises(small_budgets):
    class Failing(NoiseSource):
        def launch(self, *a):
            raise RuntimeError("launch failed")
    src = Failing()
    with pytest.raises(RuntimeError, match="launch failed"):
        P.reduce_draws(src, N, K, None, 0, True, False, lib=Lib())
    assert src.brackets == ["begin", "end"]


def test_predictive_takes_the_kernel_or_the_loop_and_converts():
    calls = []

    def sample(C):
        calls.append(C)
        return np.full((2, 3), float(len(calls)), dtype=np.float64)
    host = lambda X: P.SampleStats(X.mean(axis=0), X.std(axis=0), X.min(axis=0), X.max(axis=0), None)
    s = P.predictive(None, sample, "C", 4, host, P.SampleStats, P.as_numpy)
    assert calls == ["C"] * 4 and s.quantiles is None
    assert isinstance(s.mean, np.ndarray) and np.array_equal(s.mean, np.full((2, 3), 2.5)) and np.array_equal(s.max, np.full((2, 3), 4.0))
    X = P.predictive(None, sample, 2, 3, lambda X: X, None, P.as_numpy)
    assert X.dtype == np.float32 and X.shape == (3, 2, 3)
    t = P.predictive(None, sample, 2, 1, host, P.SampleStats, P.as_tensor_on("cpu"))
    assert isinstance(t.mean, torch.Tensor) and t.quantiles is None
    n = len(calls)
    dev = P.SampleStats(torch.ones(2, 3), torch.zeros(2, 3), torch.ones(2, 3), torch.ones(2, 3), None)
    k = P.predictive(lambda: dev, sample, 2, 9, host, P.SampleStats, P.as_numpy)
    assert len(calls) == n and isinstance(k.mean, np.ndarray) and np.array_equal(k.mean, np.ones((2, 3)))
    k = P.predictive(lambda: dev, sample, 2, 9, host, P.SampleStats, P.as_tensor_on("cpu"))
    assert k.mean is dev.mean
