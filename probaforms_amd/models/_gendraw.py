"""Multi-draw predictive statistics of the generators that are not flows: the orchestration behind ``sample_stats`` /
``sample_many`` of CVAE, ConditionalWGAN and ConditionalNormal.

What the reference's notebooks do by hand (docs/examples/regression.ipynb, forecast.ipynb) --

    X = np.array([model.sample(C) for _ in range(K)]);  X.mean(axis=0), X.std(axis=0), np.quantile(X, q, axis=0)

-- as one call: the K noise draws are made on the CPU from torch's global generator exactly as K successive ``sample(C)``
calls make them, stacked per window of draws and uploaded once per window; libpf_gendraw.so (gendraw_csrc/pf_gendraw.h)
evaluates every draw and reduces across the draws on the device into the running-moment state of libpf_predict.so, whose
pfp_finalize / pfp_quantiles finish the job.  Argument validation, the draw windows, the row chunks, the driver
(reduce_draws) and the host loop are those of models/_predict.py; this module gives it the generators' jobs as a source.
"""
import torch

from ._predict import (JointScores, SampleScores, SampleStats, WindowedSource, as_numpy, joint_scores_of_draws, predictive,
                       reduce_draws, scores_of_draws, stats_of_draws, targets_on_host, validate, validate_joint, validate_scores)


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


class JobSource(WindowedSource):
    """a job as a source of _predict.reduce_draws(): a window's noise is made on the CPU as the model's sample makes it and
    uploaded once"""

    def __init__(self, job, Cd):
        self.job, self.Cd, self.device, self.d, self.width = job, Cd, job.device, job.d, job.width

    def open(self, n, K):
        super().open(n, K)
        if n > 0:
            self.job.prepare(self.Cd, n, max(cnt for _, cnt in self.windows))

    def noise(self, k_cnt):
        return noise(k_cnt, self.n, self.width).to(self.device)

    def launch(self, lo, m, zw, k_lo, k_cnt, state, x_out, xt):
        self.job.launch(lo, m, self.n, zw, k_lo, k_cnt, self.K, state, x_out, xt)


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


def _predictive(model, C, K, host, kind, *args, **kwargs):
    """predictive() of a generator: the job's kernels where they hold the shape (args: reduce_draws' after K), else the loop"""
    job, conditions = job_of(model)

    def kernel():
        n, Cd = conditions(C)
        return reduce_draws(JobSource(job, Cd), n, K, *args, **kwargs)[0 if kind is not None else 1]
    return predictive(kernel if job.supported() else None, model.sample, C, K, host, kind, as_numpy)


def sample_many(model, C, n_draws):
    """``np.array([model.sample(C) for _ in range(n_draws)])`` -> float32 numpy [n_draws, n, d]"""
    K, _ = validate(n_draws)
    return _predictive(model, C, K, lambda X: X, None, None, 0, False, True)


def sample_stats(model, C, n_draws, quantiles, ddof):
    """SampleStats of float32 numpy arrays over n_draws samples per condition row"""
    K, probs = validate(n_draws, quantiles, ddof)
    return _predictive(model, C, K, lambda X: stats_of_draws(X, probs, int(ddof)), SampleStats, probs, int(ddof), True, False)


def sample_scores(model, C, Y, n_draws, quantiles, fair):
    """SampleScores of float32 numpy arrays: n_draws samples per condition row scored against the observed targets Y"""
    K, probs = validate_scores(n_draws, quantiles)
    return _predictive(model, C, K, lambda X: scores_of_draws(X, targets_on_host(Y), probs, fair), SampleScores,
                       probs, 0, False, False, scores=(Y, fair))


def sample_joint_scores(model, C, Y, n_draws, fair, variogram_order):
    """JointScores of float32 numpy arrays [n]: n_draws samples per condition row scored as vectors against the targets Y"""
    K, order = validate_joint(n_draws, variogram_order)
    return _predictive(model, C, K, lambda X: joint_scores_of_draws(X, targets_on_host(Y), fair, order), JointScores,
                       None, 0, False, False, joint=(Y, fair, order))
