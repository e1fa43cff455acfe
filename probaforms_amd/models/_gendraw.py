"""Multi-draw predictive statistics of the generators that are not flows: the orchestration behind ``sample_stats`` /
``sample_many`` of CVAE, ConditionalWGAN and ConditionalNormal.

What the reference's notebooks do by hand (docs/examples/regression.ipynb, forecast.ipynb) --

    X = np.array([model.sample(C) for _ in range(K)]);  X.mean(axis=0), X.std(axis=0), np.quantile(X, q, axis=0)

-- as one call: the K noise draws are made on the CPU from torch's global generator exactly as K successive ``sample(C)``
calls make them, stacked per window of draws and uploaded once per window; libpf_gendraw.so (gendraw_csrc/pf_gendraw.h)
evaluates every draw and reduces across the draws on the device into the running-moment state of libpf_predict.so, whose
pfp_finalize / pfp_quantiles finish the job.  Argument validation, the draw windows, the row chunks and the host loop are
those of models/_predict.py.
"""
import torch

from . import _predict
from ._predict import (JointScores, JointSink, SampleScores, SampleStats, ScoreSink, _chunk_quantiles, draw_windows,
                       joint_scores_of_draws, loop_draws, quantile_row_chunks, scores_of_draws, stats_of_draws, targets_on_host,
                       validate, validate_joint, validate_scores)


def one_stream(n, width):
    """K successive draws of (n, width) normals are ONE draw of K n width numbers: torch fills 16 numbers at a time and
    redraws a tail, so only whole 16-blocks concatenate"""
    return n * width >= 16 and (n * width) % 16 == 0


def noise(k_cnt, n, width):
    """[k_cnt, n, width] float32 on the CPU: what k_cnt successive ``torch.normal(0, 1, (n, width))`` (or ``torch.randn(n,
    width)``: the same generator calls) return, stacked"""
    if one_stream(n, width):
        return torch.normal(0, 1, (k_cnt, n, width))
    buf = torch.empty(k_cnt, n, width)
    for k in range(k_cnt):
        torch.normal(0, 1, (n, width), out=buf[k])
    return buf


class MlpJob:
    """x = MLP([z || c]) with flat parameters W0, b0, ..., in module order (CVAE's Decoder, ConditionalWGAN's Generator)"""

    def __init__(self, params, d, c, latent, hidden, activation, device):
        """params: () -> the net's flat float32 device tensor (asked for only once the call is known to run on the device)"""
        from . import _gendraw_lib as gl
        self.gl = gl
        self.net = gl.Mlp.make(d, c, latent, hidden, activation)
        self.params_of, self.d, self.c, self.width, self.device = params, int(d), int(c), int(latent), device
        self.ws = None

    def supported(self):
        return self.gl.supported(self.net)

    def prepare(self, Cd, n, k_max):
        self.Cd, self.params = Cd, self.params_of()
        self.ws = torch.empty(self.gl.workspace_bytes(self.net, k_max), dtype=torch.uint8, device=self.device)

    def launch(self, lo, m, n, zw, k_lo, k_cnt, K, state, x_out, xt):
        c = None if self.Cd is None else self.Cd[lo:lo + m]
        self.gl.mlp_draw_accumulate(self.net, self.params, c, m, lo, zw, n, k_lo, k_cnt, K, state, x_out, xt, self.ws)


class AffineJob:
    """x = out(mu + eps * sigma) (ConditionalNormal); mu and sigma of every row from one pfn_forward call, which draws nothing"""

    def __init__(self, core):
        from . import _gendraw_lib as gl
        self.gl, self.core = gl, core
        self.d, self.c, self.width, self.device = core.d, core.c, core.d, core.device

    def supported(self):
        return self.d <= self.gl.MAX_D

    def prepare(self, Cd, n, k_max):
        from . import _cnormal_lib as N
        core, d = self.core, self.d
        flat = core.sync()
        self.mu, self.sigma = (torch.empty(n, d, dtype=torch.float32, device=self.device) for _ in range(2))
        if n > 0:
            N.forward(core.shape, flat, Cd, None, None, n, self.mu, self.sigma, None, None, None)
        self.out_w = self.out_b = None
        if not core.shape.independent:
            self.out_w, self.out_b = flat[core.P - d * d - d:core.P - d], flat[core.P - d:core.P]

    def launch(self, lo, m, n, zw, k_lo, k_cnt, K, state, x_out, xt):
        self.gl.affine_draw_accumulate(self.d, self.mu[lo:lo + m], self.sigma[lo:lo + m], self.out_w, self.out_b, zw, m, lo, n,
                                       k_lo, k_cnt, K, state, x_out, xt)


def run(job, Cd, n, K, probs, ddof, want_stats, want_draws, scores=None, joint=None):
    """-> (SampleStats of device tensors or None, draws [K, n, d] device tensor or None).  The caller has asked
    job.supported().  Quantiles may force row chunks; every chunk then walks the same K noise draws (the generator is
    rewound), so the draws are not kept in that case (want_draws and quantiles are separate public calls).
    scores = (Y, fair): the scores path -- neither statistics nor draws; only the transposed draws are kept, per row chunk,
    and the first item returned is a SampleScores of device tensors.  joint = (Y, fair, order): the same path with a
    JointSink, and a JointScores of device tensors."""
    from . import _predict_lib as pl
    dev, d, width = job.device, job.d, job.width
    f32 = dict(dtype=torch.float32, device=dev)
    want_q = want_stats and probs is not None
    x_out = torch.empty((K, n, d), **f32) if want_draws else None
    state = pl.new_state(n, d, dev) if want_stats else None
    q_out = torch.empty((len(probs), n, d), **f32) if want_q else None
    probs_dev = torch.tensor(probs, dtype=torch.float64, device=dev) if want_q else None
    sink = None
    if scores is not None:
        assert not (want_stats or want_draws)
        sink = ScoreSink(scores[0], n, d, K, probs, scores[1], dev)
    if joint is not None:
        assert not (want_stats or want_draws) and scores is None
        sink = JointSink(joint[0], n, d, K, joint[1], joint[2], dev)
    want_xt = want_q or sink is not None
    chunks = quantile_row_chunks(n, d, K, _predict.XT_CHUNK_BYTES) if want_xt else ([(0, n)] if n else [])
    assert not (want_draws and len(chunks) > 1)
    if n > 0:
        windows = draw_windows(K, n, width, _predict.Z_WINDOW_BYTES)
        job.prepare(Cd, n, max(cnt for _, cnt in windows))
        start = torch.get_rng_state() if len(chunks) > 1 else None
        for ci, (lo, m) in enumerate(chunks):
            if ci > 0:
                torch.set_rng_state(start)                        # every row chunk walks the same K draws
            xt = torch.empty((m, d, K), **f32) if want_xt else None
            for k_lo, k_cnt in windows:
                zw = noise(k_cnt, n, width).to(dev)               # one upload per window
                job.launch(lo, m, n, zw, k_lo, k_cnt, K, None if state is None else state[lo:lo + m],
                           None if x_out is None else x_out[k_lo:k_lo + k_cnt], xt)
            if sink is not None:
                sink.chunk(pl, xt, lo, m)
            elif xt is not None:
                _chunk_quantiles(pl, xt, lo, m, d, K, probs_dev, q_out)
    stats = None
    if want_stats:
        mean, std, mn, mx = (torch.empty((n, d), **f32) for _ in range(4))
        if n > 0:
            pl.finalize(state, n, d, ddof, mean, std, mn, mx)
        stats = SampleStats(mean, std, mn, mx, q_out)
    if sink is not None:
        return sink.result(), None
    return stats, x_out


def _mismatch(C, c):
    raise RuntimeError("conditions of shape %s do not fit a model fitted with %d condition columns"
                       % (tuple(C.shape) if C is not None else None, c))


def _mlp_conditions(C, c, device):
    """(n, conditions on the device or None), as the models' sample reads C: an array, or a python int for no conditions"""
    from .wgan import _dev
    if type(C) == type(1):
        if c != 0:
            _mismatch(None, c)
        return C, None
    Cd = _dev(C, device)
    if Cd.dim() != 2 or Cd.shape[1] != c:
        _mismatch(Cd, c)
    return Cd.shape[0], (Cd if c > 0 else None)


def job_of(model):
    """(job, condition reader) of a fitted CVAE, ConditionalWGAN or ConditionalNormal"""
    from .cnormal import ConditionalNormal
    from .cvae import CVAE
    from .wgan import ConditionalWGAN, _dev
    if isinstance(model, CVAE):
        core = model._core
        s = core.shape
        widths = [s.lat + s.c] + list(model.hidden) + [s.d]
        n_dec = sum(i * o + o for i, o in zip(widths[:-1], widths[1:]))          # the decoder is the tail of the flat buffer
        job = MlpJob(lambda: core.sync()[core.P - n_dec:core.P], s.d, s.c, s.lat, model.hidden, model.activation, core.device)
        return job, lambda C: _mlp_conditions(C, job.c, core.device)
    if isinstance(model, ConditionalWGAN):
        core = model._core
        job = MlpJob(lambda: core.sync()[:core.PG], core.d, core.c, core.latent, model.generator_hidden, model.generator_activation,
                     core.device)
        return job, lambda C: _mlp_conditions(C, job.c, core.device)
    if isinstance(model, ConditionalNormal):
        core = model.model.core()
        job = AffineJob(core)

        def conditions(C):
            Cd = torch.zeros(C, 1, device=core.device) if type(C) == type(1) else _dev(C, core.device)   # as sample
            if Cd.dim() != 2 or Cd.shape[1] != core.c:
                _mismatch(Cd, core.c)
            return Cd.shape[0], Cd
        return job, conditions
    raise TypeError("no generator draw kernel for %s" % type(model).__name__)


def sample_many(model, C, n_draws):
    """``np.array([model.sample(C) for _ in range(n_draws)])`` -> float32 numpy [n_draws, n, d]"""
    K, _ = validate(n_draws)
    job, conditions = job_of(model)
    if not job.supported():
        return loop_draws(model.sample, C, K)
    n, Cd = conditions(C)
    return run(job, Cd, n, K, None, 0, False, True)[1].cpu().numpy()


def sample_stats(model, C, n_draws, quantiles, ddof):
    """SampleStats of float32 numpy arrays over n_draws samples per condition row"""
    K, probs = validate(n_draws, quantiles, ddof)
    job, conditions = job_of(model)
    if not job.supported():
        return stats_of_draws(loop_draws(model.sample, C, K), probs, int(ddof))
    n, Cd = conditions(C)
    s = run(job, Cd, n, K, probs, int(ddof), True, False)[0]
    return SampleStats(*(None if a is None else a.cpu().numpy() for a in s))


def sample_scores(model, C, Y, n_draws, quantiles, fair):
    """SampleScores of float32 numpy arrays: n_draws samples per condition row scored against the observed targets Y"""
    K, probs = validate_scores(n_draws, quantiles)
    job, conditions = job_of(model)
    if not job.supported():
        return scores_of_draws(loop_draws(model.sample, C, K), targets_on_host(Y), probs, fair)
    n, Cd = conditions(C)
    s = run(job, Cd, n, K, probs, 0, False, False, scores=(Y, fair))[0]
    return SampleScores(*(None if a is None else a.cpu().numpy() for a in s))


def sample_joint_scores(model, C, Y, n_draws, fair, variogram_order):
    """JointScores of float32 numpy arrays [n]: n_draws samples per condition row scored as vectors against the targets Y"""
    K, order = validate_joint(n_draws, variogram_order)
    job, conditions = job_of(model)
    if not job.supported():
        return joint_scores_of_draws(loop_draws(model.sample, C, K), targets_on_host(Y), fair, order)
    n, Cd = conditions(C)
    s = run(job, Cd, n, K, None, 0, False, False, joint=(Y, fair, order))[0]
    return JointScores(*(None if a is None else a.cpu().numpy() for a in s))
