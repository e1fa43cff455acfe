"""Conditional normal model, MI355X build.

Mirrors `probaforms.models.cnormal` (reference probaforms/models/cnormal.py): `Net` and `ConditionalNormal(GenModel)` with
the reference's constructor defaults, attribute names, module layout (so the `state_dict` keys are `model.0.weight`, ...,
`mu.*`, `log_sigma.*`, `out.*`), return values and RNG consumption.  The net is RE-BUILT on the CPU on every fit and
flattened into one device buffer; each epoch's shuffle comes from the global CPU generator in the reference's order, and
the `randn(rows, d)` the reference draws on every forward -- training included, although its loss never uses it -- is
consumed from the same stream and never sent to the GPU (the CVAE's `_FitDraws` replays both ahead of the GPU).  The
trunk, the two heads, the d x d inverse of `out.weight`, the loss, its backward and Adam run in libpf_cnormal.so
(probaforms_amd/models/cnormal_csrc/pf_cnormal.h); a whole epoch is one library call.  There is no CPU fallback.

`Net.forward` is inference only: it returns device tensors with no autograd graph.
"""
import numpy as np
import torch
import torch.nn as nn

from . import _cnormal_lib as N
from .._engine import FlatAdam, batch_bounds, default_device, flatten_parameters, is_flat, require_hip
from .cvae import _FitDraws
from .interfaces import GenModel
from .wgan import _dev

DEVICE = default_device()
_DEVICE_DRAW = 1 << 16      # normals from which sample's eps is drawn on the device (the same bits: nflow.HostStreamOnDevice)

SINGULAR = ("out.weight is singular to working precision: the inverse of the %dx%d matrix has a zero pivot or a "
            "non-finite entry (the Adam update of that step was skipped)")


class _NormalCore:
    """flat storage of a Net (pf_cnormal.h: model.*, mu, log_sigma, out) and its Adam state"""

    def __init__(self, net, device, lr=0.0001, weight_decay=0):
        require_hip(device)
        self.device = torch.device(device)
        lin = [m for m in net.model if isinstance(m, nn.Linear)]
        self.d, self.c = net.out.in_features, lin[0].in_features
        self.shape = N.Shape.make(self.d, self.c, [m.out_features for m in lin], net.activation, net.independent_covariance)
        self.P = N.param_count(self.shape)
        self.plist = list(net.parameters())
        assert sum(p.numel() for p in self.plist) == self.P
        self.flat = None
        self.sync()
        self.opt = FlatAdam(self.flat.numel(), self.device, lr=lr, weight_decay=weight_decay)
        self.status = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.ws = None

    def sync(self):
        if not is_flat(self.plist, self.flat):
            self.flat = flatten_parameters(self.plist, self.device)
        return self.flat

    def workspace(self, batch_rows):
        nb = N.workspace_bytes(self.shape, batch_rows)
        if nb == 0:
            N.check(N.EUNSUPPORTED, "ConditionalNormal(d=%d, hidden=%s)" % (self.d, list(self.shape.hidden)[:self.shape.n_hidden]))
        if self.ws is None or self.ws.numel() < nb:
            self.ws = torch.empty(nb, dtype=torch.uint8, device=self.device)
        return self.ws


def _activation(name):
    return {'tanh': nn.Tanh, 'relu': nn.ReLU, 'sigmoid': nn.Sigmoid}.get(name, nn.ReLU)()     # cnormal.py:39-46


class Net(nn.Module):
    """C -> hidden MLP -> (mu, log_sigma); x_tilde = mu + eps * sigma, through `out` unless independent   (cnormal.py:18-91)"""

    def __init__(self, var_size, cond_size, hidden=(10,), activation='tanh', independent_covariance=False):
        super().__init__()
        self.independent_covariance = independent_covariance
        self.activation = activation
        self.model = nn.Sequential()
        widths = [cond_size] + list(hidden)
        for w_in, w_out in zip(widths[:-1], widths[1:]):
            self.model.append(nn.Linear(w_in, w_out))
            self.model.append(_activation(activation))
        self.mu = nn.Linear(hidden[-1], var_size)              # creation order = RNG order: model, mu, log_sigma, out
        self.log_sigma = nn.Linear(hidden[-1], var_size)
        self.out = nn.Linear(var_size, var_size)               # exists in independent mode too (cnormal.py:53)
        self._core = None

    def core(self, device=None):
        if self._core is None:
            self._core = _NormalCore(self, DEVICE if device is None else device)
        return self._core

    def forward(self, X, C):
        """-> (x_tilde, inv, mu, sigma), inv None when X is None; draws randn(n, d) from the global CPU generator"""
        core = self.core()
        dev = core.device
        C = _dev(C, dev)
        X = _dev(X, dev)
        if C.dim() != 2 or C.shape[1] != core.c:
            # the reference's first nn.Linear raises from its matmul
            raise RuntimeError("mat1 and mat2 shapes cannot be multiplied (%s and %dx%d)"
                               % ("x".join(map(str, C.shape)), core.c, self.model[0].out_features))
        n, d = C.shape[0], core.d
        if X is not None and tuple(X.shape) != (n, d):
            raise RuntimeError("X must have shape (%d, %d), got %s" % (n, d, tuple(X.shape)))
        eps = None
        if n * d >= _DEVICE_DRAW:
            from .nflow import HostStreamOnDevice
            if HostStreamOnDevice.usable(dev):
                eps = HostStreamOnDevice(dev).randn((n, d))
        if eps is None:
            eps = torch.randn(n, d).to(dev)                                    # cnormal.py:81
        mu, sigma, x_tilde = (torch.empty(n, d, dtype=torch.float32, device=dev) for _ in range(3))
        inv = None if X is None else torch.empty(n, d, dtype=torch.float32, device=dev)
        if n > 0:
            N.forward(core.shape, core.sync(), C, eps, X, n, mu, sigma, x_tilde, inv, core.status)
            if inv is not None and int(core.status.item()):
                raise RuntimeError(SINGULAR % (d, d))
        return x_tilde, inv, mu, sigma


class ConditionalNormal(GenModel):
    """Conditional normal model with the reference's interface (cnormal.py:94-240).

    ConditionalNormal(use_independent_covariance=False, hidden=(10,), activation='tanh', batch_size=32, n_epochs=10,
                      lr=0.0001, weight_decay=0, verbose=0); fit(X, C=None) -> None; sample(C=100)."""

    def __init__(self, use_independent_covariance=False, hidden=(10,), activation='tanh', batch_size=32, n_epochs=10,
                 lr=0.0001, weight_decay=0, verbose=0):
        super().__init__()
        self.independent_covariance = use_independent_covariance
        self.hidden = hidden
        self.activation = activation
        self.batch_size = batch_size
        self.n_epochs = n_epochs
        self.lr = lr
        self.weight_decay = weight_decay
        self.verbose = verbose
        self.opt = None

    def _model_init(self, X, C):
        """a fresh net and optimizer on EVERY fit, built on the CPU as the reference does (cnormal.py:153-164)"""
        require_hip(DEVICE)
        self.model = Net(var_size=X.shape[1], cond_size=C.shape[1], hidden=self.hidden, activation=self.activation,
                         independent_covariance=self.independent_covariance)
        self.model._core = _NormalCore(self.model, DEVICE, self.lr, self.weight_decay)
        self.opt = self.model._core.opt

    def fit(self, X, C=None):
        if C is None:
            C = torch.zeros(X.shape[0], 1)
        self._model_init(X, C)
        core = self.model._core
        dev = core.device
        Xd, Cd = _dev(X, dev), _dev(C, dev)
        n = Xd.shape[0]
        bounds = batch_bounds(n, self.batch_size)
        nb = len(bounds)
        lr, b1, b2, eps_adam, wd = self.opt.hyper
        hyper = N.adam(lr, wd, (b1, b2), eps_adam)
        ws = core.workspace(min(n, self.batch_size))
        self.model.train(True)
        self.loss_history = []
        losses = torch.empty(self.n_epochs, nb, dtype=torch.float32, device=dev)      # every batch's loss, read back once
        status = torch.zeros(max(self.n_epochs, 1), dtype=torch.int32, device=dev)
        bar = None
        if self.verbose >= 1:
            from tqdm.auto import tqdm
            bar = tqdm(total=self.n_epochs, unit='epoch')
        # DataLoader(shuffle=True)'s two seed draws per epoch and the forward's randn(rows, d) per batch; no epoch-end draw
        draws = _FitDraws(n, bounds, core.d, self.n_epochs, dev, epoch_end=False)
        try:
            for epoch in range(self.n_epochs):
                slot, perm_h, _, _ = draws.next_epoch()
                perm = perm_h.to(dev, non_blocking=True)
                if perm_h.is_cuda:                  # drawn on the worker's stream: tell the allocator who reads it
                    perm.record_stream(torch.cuda.current_stream(dev))
                N.fit_epoch(core.shape, core.sync(), self.opt.exp_avg, self.opt.exp_avg_sq, Xd, Cd, perm, n, self.batch_size,
                            hyper, self.opt.step_count + 1, losses[epoch], status[epoch:epoch + 1], ws)
                self.opt.step_count += nb
                ev = torch.cuda.Event()
                ev.record()
                draws.release(slot, ev)
                if int(status[epoch].item()):       # the epoch's end: a step whose out.weight could not be inverted
                    raise RuntimeError(SINGULAR % (core.d, core.d))
                if bar is not None:
                    bar.update(1)
                    bar.set_description("loss: %.4f" % float(losses[epoch, -1]))
            h = losses.cpu()
            draws.finish()
        finally:
            draws.abort()
        for e in range(self.n_epochs):              # cnormal.py:209: one 0-d float32 CPU tensor per BATCH
            for b in range(nb):
                self.loss_history.append(h[e, b].clone())
        if bar is not None:
            bar.close()

    def sample(self, C=100):
        if type(C) != type(1):
            C = torch.tensor(np.asarray(C.detach().cpu() if isinstance(C, torch.Tensor) else C), dtype=torch.float)
        else:
            C = torch.zeros(C, 1)                   # meaningful only after fit(X, None)   (cnormal.py:236)
        x_tilde, _, _, _ = self.model(None, C)
        return x_tilde.cpu().detach().numpy()

    def sample_many(self, C=100, n_draws=100):
        """``np.array([self.sample(C) for _ in range(n_draws)])`` -> float32 numpy [n_draws, n, d] (a name the reference does
        not have): the trunk runs once per condition row, the draws are one launch per window of draws.  Consumes torch's
        global CPU generator exactly as the loop does."""
        from . import _gendraw
        return _gendraw.sample_many(self, C, n_draws)

    def sample_stats(self, C=100, n_draws=100, quantiles=None, ddof=0):
        """Predictive statistics per condition row over ``n_draws`` samples, as ``RealNVP.sample_stats``:
        ``SampleStats(mean, std, min, max, quantiles)`` of float32 numpy arrays [n, d] (quantiles [Q, n, d], numpy's 'linear'
        method, or None).  eps comes from torch's global CPU generator exactly as ``n_draws`` successive ``sample(C)`` calls
        draw it; mu and sigma are computed once per row, the draws and the reductions across them run on the device.
        ``n_draws < 1``, a probability outside [0, 1] or quantiles with ``n_draws > 8192`` raise ValueError."""
        from . import _gendraw
        return _gendraw.sample_stats(self, C, n_draws, quantiles, ddof)

    def sample_scores(self, C, Y, n_draws=1000, quantiles=(0.05, 0.95), fair=False):
        """Scores of the predictive draws against the observed targets ``Y`` [n, d], as ``RealNVP.sample_scores``:
        ``SampleScores(crps, pit, quantiles, pinball)`` of float32 numpy arrays [n, d] (quantiles and pinball [Q, n, d], or
        None).  The eps draws come from torch's global CPU generator exactly as ``n_draws`` successive ``sample(C)`` calls
        draw them, so a seeded call scores bitwise the draws a seeded ``sample_many`` returns; the draws, the sort and
        the scores run on the device.  ``n_draws < 1``, ``n_draws > 8192``, a probability outside [0, 1] or a ``Y`` whose
        shape is not (n, d) raise ValueError."""
        from . import _gendraw
        return _gendraw.sample_scores(self, C, Y, n_draws, quantiles, fair)

    def sample_joint_scores(self, C, Y, n_draws=1000, fair=False, variogram_order=0.5):
        """Joint scores of the predictive draws against the observed targets ``Y`` [n, d], as ``RealNVP.sample_joint_scores``:
        ``JointScores(energy, spread, variogram)`` of float32 numpy arrays [n] (variogram None when ``variogram_order`` is
        None), each row's draws scored as vectors in R^d.  The noise draws come from torch's global CPU generator exactly as
        ``n_draws`` successive ``sample(C)`` calls draw them, so a seeded call scores the draws a seeded ``sample_many``
        returns; the generator and the scores run on the device.  ``n_draws < 1``, ``n_draws > 8192``, an order other than
        0.5, 1 or 2, or a ``Y`` whose shape is not (n, d) raise ValueError.
        A width the kernel does not serve falls back to the loop on the host (``self.sample`` n_draws times plus numpy)."""
        from . import _gendraw
        return _gendraw.sample_joint_scores(self, C, Y, n_draws, fair, variogram_order)
