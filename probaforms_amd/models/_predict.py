"""Multi-draw predictive statistics of a RealNVP flow: the orchestration behind ``sample_stats`` / ``sample_many``.

What the reference's notebooks do by hand (docs/examples/regression.ipynb, forecast.ipynb) --

    X = np.array([model.sample(C) for _ in range(K)]);  X.mean(axis=0), X.std(axis=0), np.quantile(X, q, axis=0)

-- as one call: libpf_predict.so (predict_csrc/pf_predict.h) draws the K prior samples per condition row, pushes them through
the inverse flow and reduces across the draws on the device; only [n, d] statistics leave it.

``sample_scores`` scores those draws against observed targets (CRPS, PIT, quantiles, pinball loss; pfp_scores): the same draws,
the same sort, one more pass over each sorted series.

``sample_joint_scores`` scores each row's draws as vectors in R^d (energy score, variogram score; pfp_joint_scores): the same
draws again, one workgroup per row over its K (K - 1) / 2 pairs.

The arithmetic that needs no GPU lives here as plain functions (argument validation, the draw windows, the row chunks, the
routing between the kernels and the host loop) so that the CPU suite covers it.  So does the one driver of all four models'
calls, reduce_draws(): it owns the outputs, the row chunks and torch's generator around them and takes the launches from a
*source* (SeededFlow and HostPriorFlow here, _gendraw.JobSource) and the finishing kernels from `lib`, so that
tests/test_predict_driver_host.py runs it on CPU tensors.  predictive() is the pattern of every public sample_* method.
"""
import collections

import numpy as np
import torch

Z_WINDOW_BYTES = 256 << 20        # the z buffer of a window of host-prior draws stays at or below this
XT_CHUNK_BYTES = 1 << 30          # the transposed draws the quantile kernel sorts: above this, row chunks
MAX_QUANTILE_DRAWS = 8192         # pf_predict.h PFP_MAX_QUANTILE_DRAWS

SampleStats = collections.namedtuple("SampleStats", "mean std min max quantiles")
SampleScores = collections.namedtuple("SampleScores", "crps pit quantiles pinball")
JointScores = collections.namedtuple("JointScores", "energy spread variogram")
VARIOGRAM_ORDERS = (0.5, 1.0, 2.0)
PAIR_BLOCK_ELEMS = 1 << 22        # joint_scores_of_draws: elements of the squared-distance block held at once


def validate(n_draws, quantiles=None, ddof=0):
    """-> (K, probs) with probs a tuple of floats or None; ValueError for n_draws < 1, a probability outside [0, 1],
    quantiles with more than MAX_QUANTILE_DRAWS draws, or a negative ddof"""
    if isinstance(n_draws, bool) or int(n_draws) != n_draws:
        raise ValueError("n_draws must be an integer, got %r" % (n_draws,))
    K = int(n_draws)
    if K < 1:
        raise ValueError("n_draws must be at least 1, got %d" % K)
    if int(ddof) != ddof or int(ddof) < 0:
        raise ValueError("ddof must be a non-negative integer, got %r" % (ddof,))
    probs = None
    if quantiles is not None:
        probs = tuple(float(q) for q in np.atleast_1d(np.asarray(quantiles, dtype=np.float64)))
        if len(probs) == 0:
            probs = None
    if probs is not None:
        for q in probs:
            if not 0.0 <= q <= 1.0:           # (NaN fails both comparisons)
                raise ValueError("quantiles must lie in [0, 1], got %r" % (q,))
        if K > MAX_QUANTILE_DRAWS:
            raise ValueError("quantiles need n_draws <= %d (one series is sorted inside one workgroup), got %d"
                             % (MAX_QUANTILE_DRAWS, K))
    return K, probs


def validate_scores(n_draws, quantiles=None):
    """-> (K, probs) as validate(); the series is always sorted, so n_draws > MAX_QUANTILE_DRAWS raises ValueError with or
    without quantiles"""
    K, probs = validate(n_draws, quantiles)
    if K > MAX_QUANTILE_DRAWS:
        raise ValueError("sample_scores needs n_draws <= %d (one series is sorted inside one workgroup), got %d"
                         % (MAX_QUANTILE_DRAWS, K))
    return K, probs


def validate_joint(n_draws, variogram_order=0.5):
    """-> (K, order) with order None or one of VARIOGRAM_ORDERS as a float; n_draws as validate_scores(); ValueError for any
    other order (|.|^p is evaluated as sqrt, identity or square, never pow)"""
    K, _ = validate(n_draws)
    if K > MAX_QUANTILE_DRAWS:
        raise ValueError("sample_joint_scores needs n_draws <= %d (one row's pairs are walked by one workgroup), got %d"
                         % (MAX_QUANTILE_DRAWS, K))
    if variogram_order is None:
        return K, None
    try:
        order = float(variogram_order)
    except (TypeError, ValueError):
        raise ValueError("variogram_order must be None or one of %s, got %r" % (VARIOGRAM_ORDERS, variogram_order))
    if isinstance(variogram_order, bool) or order not in VARIOGRAM_ORDERS:
        raise ValueError("variogram_order must be None or one of %s, got %r" % (VARIOGRAM_ORDERS, variogram_order))
    return K, order


def draw_windows(K, n, d, budget=Z_WINDOW_BYTES):
    """[(k_lo, k_cnt)] covering K draws so that a window's z buffer [k_cnt, n, d] float32 stays within `budget`
    (one draw per window when even a single draw exceeds it)"""
    per = max(1, int(n) * int(d) * 4)
    cnt = max(1, min(int(K), budget // per))
    return [(lo, min(cnt, K - lo)) for lo in range(0, int(K), cnt)]


def quantile_row_chunks(n, d, K, budget=XT_CHUNK_BYTES):
    """[(lo, m)] covering n rows so that a chunk's transposed draws [m, d, K] float32 stay within `budget` (one row per
    chunk when even a single row exceeds it); one chunk when everything fits"""
    n = int(n)
    if n == 0:
        return []
    per = max(1, int(d) * int(K) * 4)
    rows = max(1, min(n, budget // per))
    return [(lo, min(rows, n - lo)) for lo in range(0, n, rows)]


def route(nf, supported=None):
    """'kernel' or the reason the call runs as the notebook's loop on the host: 'layerwise' (layers that cannot run as one
    fused stack), 'prior' (a prior object the user assigned), 'shape' (the kernels do not hold the shape in LDS).
    `supported`: callable () -> bool asked last (it needs the engine); None skips that question."""
    from .nflow import StandardNormalPrior
    if nf._layerwise():
        return "layerwise"
    if not isinstance(nf.prior, StandardNormalPrior):
        return "prior"
    if supported is not None and not supported():
        return "shape"
    return "kernel"


def stats_of_draws(X, probs, ddof):
    """the notebook's numpy reductions over stacked draws X [K, n, d], in float64, rounded once to float32"""
    X64 = np.asarray(X, dtype=np.float64)
    K = X64.shape[0]
    f = lambda a: np.asarray(a, dtype=np.float32)
    with np.errstate(all="ignore"):
        std = X64.std(axis=0, ddof=ddof) if K > ddof else np.full(X64.shape[1:], np.nan)
        q = None if probs is None else f(np.quantile(X64, list(probs), axis=0).reshape((len(probs),) + X64.shape[1:]))
        return SampleStats(f(X64.mean(axis=0)), f(std), f(X64.min(axis=0)), f(X64.max(axis=0)), q)


def scores_of_draws(X, Y, probs, fair):
    """SampleScores (float32 numpy) of stacked draws X [K, n, d] against the targets Y [n, d]: the host route of
    ``sample_scores``.  Per (row, column) series x_1 .. x_K and target y, in float64 with one rounding (D = K - 1 if fair
    else K):
        crps    = 1/K sum_k |x_k - y| - 1/(2 K D) sum_k sum_l |x_k - x_l|    (pair sum = 2 sum_i (2 i - K + 1) x_(i), sorted)
        pit     = (#{x_k < y} + 0.5 #{x_k == y}) / K
        pinball = (y - Q) (p - [y < Q]),  Q = numpy.quantile(x, p)
    A NaN in the series or in y: crps, pit and pinball NaN (quantiles only for a NaN in the series).  A series holding an
    infinity: crps NaN, as the pair sum's inf - inf gives."""
    X64 = np.asarray(X, dtype=np.float32).astype(np.float64)
    Y32 = np.asarray(Y, dtype=np.float32)
    if X64.ndim != 3 or Y32.shape != X64.shape[1:]:
        raise ValueError("Y must have shape %s (one target per condition row and column), got %s"
                         % (X64.shape[1:], Y32.shape))
    Y64 = Y32.astype(np.float64)
    K = X64.shape[0]
    f = lambda a: np.asarray(a, dtype=np.float32)
    with np.errstate(all="ignore"):
        nan = np.isnan(X64).any(axis=0)
        bad = nan | np.isnan(Y64)
        S = np.sort(X64, axis=0)
        mid = S[K // 2]
        mid = np.where(np.isfinite(mid), mid, 0.0)
        w = (2.0 * np.arange(K) - K + 1.0).reshape((K,) + (1,) * (X64.ndim - 1))
        s1 = np.abs(S - Y64).sum(axis=0)
        s2 = (w * (S - mid)).sum(axis=0)
        crps = s1 / K - s2 / (float(K) * float(K - 1 if fair else K))
        crps = np.where(bad | np.isinf(X64).any(axis=0), np.nan, crps)
        pit = np.where(bad, np.nan, ((X64 < Y64).sum(axis=0) + 0.5 * (X64 == Y64).sum(axis=0)) / K)
        q = pin = None
        if probs is not None:
            p = np.asarray(list(probs), dtype=np.float64)
            q = np.quantile(X64, p, axis=0).reshape((len(p),) + X64.shape[1:])
            q = np.where(nan, np.nan, q)
            pw = p.reshape((len(p),) + (1,) * (X64.ndim - 1))
            pin = f(np.where(bad, np.nan, (Y64 - q) * (pw - (Y64 < q))))
            q = f(q)
        return SampleScores(f(crps), f(pit), q, pin)


def joint_scores_of_draws(X, Y, fair, order):
    """JointScores (float32 numpy [n]; variogram None when order is None) of stacked draws X [K, n, d] against the targets
    Y [n, d]: the host route of ``sample_joint_scores``.  Per row, with draws x_k in R^d and target y, in float64 with one
    rounding (D = K - 1 if fair else K):
        spread    = 1/(2 K D) sum_k sum_l |x_k - x_l|_2
        energy    = 1/K sum_k |x_k - y|_2 - spread
        variogram = sum_i sum_j (|y_i - y_j|^p - 1/K sum_k |x_ki - x_kj|^p)^2,  p = order
    The pair sum is blocked over rows and draws: the squared distances of one block are summed column by column, so no
    K x K x d array is ever held.  A NaN among the row's draws or in its y: all three NaN.  An infinity among the draws: energy
    and spread NaN (the pair sum's diagonal forms inf - inf); an infinity among the draws or in y: variogram NaN (its (i, i)
    terms do)."""
    X64 = np.asarray(X, dtype=np.float32).astype(np.float64)
    Y32 = np.asarray(Y, dtype=np.float32)
    if X64.ndim != 3 or Y32.shape != X64.shape[1:]:
        raise ValueError("Y must have shape %s (one target per condition row and column), got %s"
                         % (X64.shape[1:], Y32.shape))
    Y64 = Y32.astype(np.float64)
    K, n, d = X64.shape
    f = lambda a: np.asarray(a, dtype=np.float32)
    pw = {0.5: np.sqrt, 1.0: lambda a: a, 2.0: np.square, None: None}[order]
    with np.errstate(all="ignore"):
        nan = np.isnan(X64).any(axis=(0, 2)) | np.isnan(Y64).any(axis=1)
        xinf = np.isinf(X64).any(axis=(0, 2))
        t1 = np.sqrt(np.square(X64 - Y64).sum(axis=2)).sum(axis=0)
        pairs = np.zeros(n)
        cols = np.ascontiguousarray(X64.transpose(2, 0, 1))          # [d, K, n]
        kb = max(1, min(K, 256))
        rows = max(1, PAIR_BLOCK_ELEMS // (kb * K))
        for r0 in range(0, n, rows):
            for lo in range(0, K, kb):
                sq = np.zeros((min(kb, K - lo), K, min(rows, n - r0)))
                df = np.empty_like(sq)
                for j in range(d):
                    col = cols[j, :, r0:r0 + rows]
                    np.subtract(col[lo:lo + kb, None], col[None], out=df)
                    np.square(df, out=df)
                    sq += df
                pairs[r0:r0 + rows] += np.sqrt(sq, out=sq).sum(axis=(0, 1))
        spread = pairs / (2.0 * K * float(K - 1 if fair else K))
        energy = t1 / K - spread
        dead = nan | xinf
        energy, spread = np.where(dead, np.nan, energy), np.where(dead, np.nan, spread)
        vario = None
        if order is not None:
            vario = np.zeros(n)
            for i in range(d):
                for j in range(i + 1, d):
                    m = pw(np.abs(X64[:, :, i] - X64[:, :, j])).sum(axis=0) / K
                    vario += 2.0 * np.square(pw(np.abs(Y64[:, i] - Y64[:, j])) - m)
            vario = f(np.where(nan | xinf | np.isinf(Y64).any(axis=1), np.nan, vario))
        return JointScores(f(energy), f(spread), vario)


def targets_on_host(Y):
    """the observed targets as float32 numpy, for the host route"""
    if isinstance(Y, torch.Tensor):
        Y = Y.detach().cpu().numpy()
    return np.asarray(Y, dtype=np.float32)


def targets_on_device(Y, device):
    """the observed targets as a contiguous float32 tensor on `device` (a tensor already there is not copied)"""
    if not isinstance(Y, torch.Tensor):
        Y = torch.from_numpy(np.ascontiguousarray(np.asarray(Y, dtype=np.float32)))
    return Y.detach().to(device=device, dtype=torch.float32).contiguous()


def _conditions(nf, C, eng):
    if type(C) == type(1):            # python int only, as nflow.py:135
        return C, None
    return len(C), nf._on_device(C, eng)


def _host_draws(n, d, dev):
    """how the host prior makes one draw of randn(n, d): 'device' (the generator's bits drawn on the device) or 'host'"""
    from .nflow import HostStreamOnDevice
    return "device" if (n * d >= 16 and HostStreamOnDevice.usable(dev)) else "host"


def targets_checked(Y, n, d, device):
    """targets_on_device(Y); ValueError unless its shape is (n, d)"""
    Y = targets_on_device(Y, device)
    if tuple(Y.shape) != (n, d):
        raise ValueError("Y must have shape (%d, %d) (one target per condition row and column), got %s" % (n, d, tuple(Y.shape)))
    return Y


class ScoreSink:
    """the scores path of reduce_draws(): the device outputs, and pfp_scores on one row chunk's transposed draws"""

    def __init__(self, Y, n, d, K, probs, fair, device):
        self.Y = targets_checked(Y, n, d, device)
        f32 = dict(dtype=torch.float32, device=device)
        self.n, self.d, self.K, self.fair = n, d, K, bool(fair)
        self.crps, self.pit = torch.empty((n, d), **f32), torch.empty((n, d), **f32)
        self.probs = self.q = self.pinball = None
        if probs is not None:
            self.probs = torch.tensor(probs, dtype=torch.float64, device=device)
            self.q, self.pinball = torch.empty((len(probs), n, d), **f32), torch.empty((len(probs), n, d), **f32)

    def chunk(self, pl, xt, lo, m):
        """scores of rows lo .. lo + m"""
        q, pb = self.q, self.pinball
        part = q is not None and m != self.n                      # [Q, m, d] of [Q, n, d] is not contiguous
        if part:
            q, pb = (torch.empty((q.shape[0], m, self.d), dtype=torch.float32, device=q.device) for _ in range(2))
        pl.scores(xt, self.Y[lo:lo + m], m, self.d, self.K, self.fair, self.probs, self.crps[lo:lo + m],
                  self.pit[lo:lo + m], q, pb)
        if part:
            self.q[:, lo:lo + m].copy_(q)
            self.pinball[:, lo:lo + m].copy_(pb)

    def result(self):
        return SampleScores(self.crps, self.pit, self.q, self.pinball)


class JointSink:
    """the joint-scores path of reduce_draws(), with ScoreSink's protocol: the device outputs, and pfp_joint_scores on one row
    chunk's transposed draws"""

    def __init__(self, Y, n, d, K, fair, order, device):
        self.Y = targets_checked(Y, n, d, device)
        f32 = dict(dtype=torch.float32, device=device)
        self.n, self.d, self.K, self.fair, self.order = n, d, K, bool(fair), order
        self.energy, self.spread = torch.empty((n,), **f32), torch.empty((n,), **f32)
        self.variogram = None if order is None else torch.empty((n,), **f32)

    def chunk(self, pl, xt, lo, m):
        """joint scores of rows lo .. lo + m"""
        pl.joint_scores(xt, self.Y[lo:lo + m], m, self.d, self.K, self.fair, self.order, self.energy[lo:lo + m],
                        self.spread[lo:lo + m], None if self.variogram is None else self.variogram[lo:lo + m])

    def result(self):
        return JointScores(self.energy, self.spread, self.variogram)


def reduce_draws(source, n, K, probs, ddof, want_stats, want_draws, scores=None, joint=None, lib=None):
    """K draws of each of n condition rows, reduced across the draws on the device -> (SampleStats of device tensors or None,
    draws [K, n, d] device tensor or None).  scores = (Y, fair): the scores path -- neither statistics nor draws; only the
    transposed draws are kept, per row chunk, and the first item returned is a SampleScores of device tensors.
    joint = (Y, fair, order): the same path with a JointSink, and a JointScores of device tensors.

    `source` makes the draws; this function owns the outputs, the row chunks and torch's generator around them.  A source has
    `device`, `d`, and
        open(n, K)                      once, before any chunk and also when n == 0: only a source whose draws are K seeds
                                        takes anything from torch's generator for n == 0
        draw(lo, m, state, x_out, xt)   queues all K draws of rows lo .. lo + m: folded into state [m, d, ...] (or None), written
                                        to x_out [K, n rows of this call, d] (or None) and transposed to xt [m, d, K] (or None)
        close()                         once, after the last chunk's work is queued
    Quantiles and scores may force row chunks; every chunk then walks the same K draws: the generator's state is saved before
    the first chunk and put back before every later one, so the generator ends where K successive sample(C) calls leave it.  The
    draws are not kept in that case.  `lib`: the _predict_lib module (None: import it); a CPU test hands in a stand-in."""
    if lib is None:
        from . import _predict_lib as lib
    dev, d = source.device, source.d
    f32 = dict(dtype=torch.float32, device=dev)
    x_out = torch.empty((K, n, d), **f32) if want_draws else None
    state = lib.new_state(n, d, dev) if want_stats else None
    q_out = torch.empty((len(probs), n, d), **f32) if (want_stats and probs is not None) else None
    probs_dev = torch.tensor(probs, dtype=torch.float64, device=dev) if q_out is not None else None
    sink = None
    if scores is not None:
        assert not (want_stats or want_draws)
        sink = ScoreSink(scores[0], n, d, K, probs, scores[1], dev)
    if joint is not None:
        assert not (want_stats or want_draws) and scores is None
        sink = JointSink(joint[0], n, d, K, joint[1], joint[2], dev)
    want_xt = q_out is not None or sink is not None
    chunks = quantile_row_chunks(n, d, K, XT_CHUNK_BYTES) if want_xt else ([(0, n)] if n else [])
    assert not (want_draws and len(chunks) > 1)
    source.open(n, K)
    start = torch.get_rng_state() if len(chunks) > 1 else None
    for ci, (lo, m) in enumerate(chunks):
        if ci > 0:
            torch.set_rng_state(start)                            # every row chunk walks the same K draws
        xt = torch.empty((m, d, K), **f32) if want_xt else None
        source.draw(lo, m, None if state is None else state[lo:lo + m], x_out, xt)
        if sink is not None:
            sink.chunk(lib, xt, lo, m)
        elif xt is not None:
            _chunk_quantiles(lib, xt, lo, m, d, K, probs_dev, q_out)
    source.close()
    if sink is not None:
        return sink.result(), None
    if not want_stats:
        return None, x_out
    mean, std, mn, mx = (torch.empty((n, d), **f32) for _ in range(4))
    if n > 0:
        lib.finalize(state, n, d, ddof, mean, std, mn, mx)
    return SampleStats(mean, std, mn, mx, q_out), x_out


def _chunk_quantiles(pl, xt, lo, m, d, K, probs_dev, q_out):
    """quantiles of one row chunk into rows lo .. lo + m of q_out [Q, n, d]"""
    if m == q_out.shape[1]:
        pl.quantiles(xt, m, d, K, probs_dev, q_out)
        return
    t = torch.empty((q_out.shape[0], m, d), dtype=torch.float32, device=q_out.device)
    pl.quantiles(xt, m, d, K, probs_dev, t)
    q_out[:, lo:lo + m].copy_(t)


class WindowedSource:
    """A source of reduce_draws() whose draws come from noise made on torch's generator: the K draws of a chunk are made and
    launched window by window (draw_windows: a window's noise [k_cnt, n, width] stays within Z_WINDOW_BYTES).  A subclass sets
    device, d, width and gives noise(k_cnt) -> the next k_cnt draws of (n, width) normals on the device, and
    launch(lo, m, zw, k_lo, k_cnt, state, x_out, xt) for draws k_lo .. k_lo + k_cnt of rows lo .. lo + m; begin() / end()
    bracket a chunk's windows (end() also runs when a window raised).  Nothing touches the generator when n == 0."""

    def open(self, n, K):
        self.n, self.K = n, K
        self.windows = draw_windows(K, n, self.width, Z_WINDOW_BYTES) if n > 0 else []

    def begin(self):
        pass
    end = close = begin

    def draw(self, lo, m, state, x_out, xt):
        self.begin()
        try:
            for k_lo, k_cnt in self.windows:
                self.launch(lo, m, self.noise(k_cnt), k_lo, k_cnt, state, None if x_out is None else x_out[k_lo:k_lo + k_cnt], xt)
        finally:
            self.end()


class SeededFlow:
    """the flow with the device prior: the K draws are K seeds of the counter-based stream (what K successive sample() calls
    consume, taken even when n == 0) and one pfp_draw_accumulate per row chunk, which draws z inside the kernel"""

    def __init__(self, nf, eng, Cd):
        self.nf, self.eng, self.Cd, self.device, self.d = nf, eng, Cd, eng.device, eng.d

    def open(self, n, K):
        self.n, self.K = n, K
        self.seeds = [self.nf.prior.next_seed() for _ in range(K)]
        self.keep = []

    def draw(self, lo, m, state, x_out, xt):
        c = None if self.Cd is None else self.Cd[lo:lo + m]
        self.keep.append(self.eng.predict_draw(c, m, lo, self.seeds, None, self.n, 0, self.K, self.K, state, x_out, xt))

    def close(self):
        torch.cuda.current_stream(self.device).synchronize()     # the host seed arrays have been consumed
        del self.keep


class HostPriorFlow(WindowedSource):
    """the flow with the host prior: a window's z is k_cnt successive randn(n, d) of torch's generator, drawn on the device
    with the generator's bits (HostStreamOnDevice, one state round trip per chunk) or on the host"""

    def __init__(self, nf, eng, Cd):
        self.eng, self.Cd, self.device, self.d, self.width = eng, Cd, eng.device, eng.d, eng.d

    def open(self, n, K):
        super().open(n, K)
        if n > 0:
            self.on_device = _host_draws(n, self.d, self.device) == "device"
            self.zbuf = torch.empty((self.windows[0][1], n, self.d), dtype=torch.float32, device=self.device)

    def begin(self):
        from .nflow import HostStreamOnDevice
        self.hs = HostStreamOnDevice(self.device).begin() if self.on_device else None

    def end(self):
        if self.hs is not None:
            self.hs.end()

    def noise(self, k_cnt):
        zw = self.zbuf[:k_cnt]
        if self.hs is None:
            zw.copy_(torch.stack([torch.randn((self.n, self.d)) for _ in range(k_cnt)]))
        elif (self.n * self.d) % 16 == 0:
            self.hs.draw(zw)                                      # whole 16-blocks: k_cnt draws of n d numbers are one draw
        else:
            for k in range(k_cnt):
                self.hs.draw(zw[k])
        return zw

    def launch(self, lo, m, zw, k_lo, k_cnt, state, x_out, xt):
        c = None if self.Cd is None else self.Cd[lo:lo + m]
        self.eng.predict_draw(c, m, lo, None, zw, self.n, k_lo, k_cnt, self.K, state, x_out, xt)


def flow_draws(nf, C, K, *args, **kwargs):
    """reduce_draws() of a flow whose route() is 'kernel': (C, K, probs, ddof, want_stats, want_draws, scores=, joint=)"""
    eng = nf.engine()
    eng.sync_params()
    n, Cd = _conditions(nf, C, eng)
    Cd = eng._cond(Cd, n)
    source = (HostPriorFlow if nf.prior.host_rng else SeededFlow)(nf, eng, Cd)
    return reduce_draws(source, n, K, *args, **kwargs)


def loop_draws(sample, C, K):
    """the notebook's loop: K successive sample(C) calls, stacked [K, n, d] (numpy float32)"""
    return np.array([np.asarray(sample(C), dtype=np.float32) for _ in range(K)], dtype=np.float32)


def as_numpy(a):
    """a result array as numpy: a device tensor comes to the host, the host route's numpy passes"""
    return a.cpu().numpy() if isinstance(a, torch.Tensor) else a


def as_tensor_on(device):
    """-> the conversion to a tensor on `device`: the host route's numpy goes there, a device tensor passes"""
    return lambda a: a if isinstance(a, torch.Tensor) else torch.from_numpy(a).to(device)


def predictive(kernel, sample, C, K, host, kind, convert):
    """The pattern of every sample_* method.  kernel: () -> the device result (reduce_draws), or None when the call runs as
    the notebook's loop on the host: K successive sample(C) calls, then host(X [K, n, d] numpy) -> the numpy result.  The
    result is one array (kind None) or a named tuple `kind` whose fields may be None; convert is as_numpy or as_tensor_on()."""
    s = kernel() if kernel is not None else host(loop_draws(sample, C, K))
    if kind is None:
        return convert(s)
    return kind(*(None if a is None else convert(a) for a in s))
