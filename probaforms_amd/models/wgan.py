"""Conditional Wasserstein GAN, MI355X build.

Mirrors `probaforms.models.wgan` (reference probaforms/models/wgan.py): `Generator`, `Discriminator` and
`ConditionalWGAN(GenModel)` with the reference's constructor defaults, `.model` `nn.Sequential` layouts (so the
`state_dict` keys are `generator.model.0.weight`, ..., `discriminator.model.4.bias`), RNG consumption and return values.
The networks are RE-BUILT on the CPU on every fit (wgan.py:168-187: Generator first, then Discriminator) and flattened
into one device buffer; each epoch's shuffle, per-batch noise and epoch-end noise come from the global CPU generator in
the reference's order, replayed ahead of the GPU by the CVAE's `_FitDraws`.  Every iteration -- G forward, D forward on
the real and fake rows, the backward of the net that steps, RMSprop and the critic's clamp -- runs in libpf_wgan.so
(probaforms_amd/models/wgan_csrc/pf_wgan.h); a whole epoch is one library call.  There is no CPU fallback.

`Generator.forward` / `Discriminator.forward` are inference only: they return device tensors with no autograd graph.
"""
import numpy as np
import torch
import torch.nn as nn

from . import _wgan_lib as W
from .._engine import batch_bounds, default_device, flatten_parameters, is_flat, require_hip
from .cvae import _FitDraws
from .interfaces import GenModel

DEVICE = default_device()
CLAMP = 0.01          # wgan.py:248


def _mlp(n_inputs, hidden, activation, n_outputs):
    net = nn.Sequential()
    widths = [n_inputs] + list(hidden)
    for w_in, w_out in zip(widths[:-1], widths[1:]):
        net.append(nn.Linear(w_in, w_out))
        net.append(nn.Tanh() if activation == 'tanh' else nn.ReLU())    # wgan.py:26-32: anything else is ReLU
    net.append(nn.Linear(hidden[-1], n_outputs))
    return net


class _WganCore:
    """flat storage of a Generator / Discriminator pair ([G | D], pf_wgan.h) and the RMSprop state of both"""

    def __init__(self, generator, discriminator, d, c, latent, g_hidden, d_hidden, g_act, d_act, device):
        require_hip(device)
        self.device = torch.device(device)
        self.shape = W.Shape.make(d, c, latent, g_hidden, d_hidden, g_act, d_act)
        self.d, self.c, self.latent = d, c, latent
        self.PG = W.param_count(self.shape, W.NET_G)
        self.PD = W.param_count(self.shape, W.NET_D)
        self.plist = list(generator.parameters()) + list(discriminator.parameters())
        assert sum(p.numel() for p in self.plist) == self.PG + self.PD
        self.flat = None
        self.sync()
        self.square_avg = torch.zeros_like(self.flat)
        self.ws = None

    def sync(self):
        if not is_flat(self.plist, self.flat):
            self.flat = flatten_parameters(self.plist, self.device)
        return self.flat

    def workspace(self, batch_rows, loss_rows=0):
        nb = W.workspace_bytes(self.shape, batch_rows, loss_rows)
        if nb == 0:
            raise RuntimeError("invalid ConditionalWGAN shape")
        if self.ws is None or self.ws.numel() < nb:
            self.ws = torch.empty(nb, dtype=torch.uint8, device=self.device)
        return self.ws


def _dev(t, device):
    """numpy array, array-like or tensor (any device) -> contiguous float32 tensor on `device`"""
    if t is None:
        return None
    if isinstance(t, torch.Tensor):
        return t.detach().to(device=device, dtype=torch.float32).contiguous()
    return torch.tensor(np.asarray(t), dtype=torch.float32, device=device).contiguous()


def _check_width(net, X, C):
    lin = net.model[0]
    got = X.shape[1] + (0 if C is None else C.shape[1])
    if X.dim() != 2 or (C is not None and (C.dim() != 2 or C.shape[0] != X.shape[0])) or got != lin.in_features:
        # the reference's first nn.Linear raises from its matmul
        raise RuntimeError("mat1 and mat2 shapes cannot be multiplied (%dx%d and %dx%d)"
                           % (X.shape[0], got, lin.in_features, lin.out_features))


class Generator(nn.Module):
    """[Z || C] -> hidden MLP -> X   (wgan.py:12-59)"""

    def __init__(self, n_inputs, n_outputs, hidden=(10,), activation='tanh'):
        super().__init__()
        self.model = _mlp(n_inputs, hidden, activation, n_outputs)
        self.n_inputs, self.n_outputs = n_inputs, n_outputs
        self._core = None

    def forward(self, X, C=None):
        core = self._core
        if core is None:
            raise RuntimeError("Generator must belong to a ConditionalWGAN (its weights live in the model's flat HIP buffer)")
        Z, C = _dev(X, core.device), _dev(C, core.device)
        _check_width(self, Z, C)
        out = torch.empty(Z.shape[0], self.n_outputs, dtype=torch.float32, device=core.device)
        if Z.shape[0] > 0:
            W.generate(core.shape, core.sync(), Z, C, Z.shape[0], out)
        return out


class Discriminator(nn.Module):
    """[X || C] -> hidden MLP -> critic value   (wgan.py:62-107)"""

    def __init__(self, n_inputs, hidden=(10,), activation='tanh'):
        super().__init__()
        self.model = _mlp(n_inputs, hidden, activation, 1)
        self.n_inputs = n_inputs
        self._core = None

    def forward(self, X, C=None):
        core = self._core
        if core is None:
            raise RuntimeError("Discriminator must belong to a ConditionalWGAN (its weights live in the model's flat HIP buffer)")
        X, C = _dev(X, core.device), _dev(C, core.device)
        _check_width(self, X, C)
        out = torch.empty(X.shape[0], 1, dtype=torch.float32, device=core.device)
        if X.shape[0] > 0:
            W.critic(core.shape, core.sync(), X, C, X.shape[0], out)
        return out


class _FlatRMSprop:
    """torch.optim.RMSprop(net.parameters(), lr, weight_decay) of wgan.py:183-184 (alpha 0.99, eps 1e-8, no momentum,
    not centred); its state is one slice of the model's flat square_avg buffer and the step runs in the library"""

    def __init__(self, square_avg, lr, weight_decay, alpha=0.99, eps=1e-8):
        self.square_avg = square_avg
        self.defaults = dict(lr=lr, alpha=alpha, eps=eps, weight_decay=weight_decay, momentum=0, centered=False)

    def hyper(self, clamp=0.0):
        d = self.defaults
        return W.rmsprop(d['lr'], d['alpha'], d['eps'], d['weight_decay'], clamp)


def step_kinds(iter_i, n_batches, n_critic):
    """PFW_STEP_* of the batches iter_i, iter_i + 1, ...: a critic step where iter_i % n_critic != 0 (wgan.py:233, Python's %)"""
    return np.array([W.STEP_CRITIC if (iter_i + b) % n_critic != 0 else W.STEP_GEN for b in range(n_batches)], dtype=np.int8)


class ConditionalWGAN(GenModel):
    """Conditional Wasserstein GAN with the reference's interface (wgan.py:110-320).

    ConditionalWGAN(latent_dim=1, generator_hidden=(100, 100), discriminator_hidden=(100, 100),
                    generator_activation='relu', discriminator_activation='relu', batch_size=32, n_epochs=1000,
                    lr=5e-5, weight_decay=0, n_critic=5, verbose=0); fit(X, C=None) -> None; sample(C=10)."""

    def __init__(self, latent_dim=1, generator_hidden=(100, 100), discriminator_hidden=(100, 100),
                 generator_activation='relu', discriminator_activation='relu', batch_size=32, n_epochs=1000,
                 lr=0.00005, weight_decay=0, n_critic=5, verbose=0):
        super().__init__()
        self.generator_hidden = generator_hidden
        self.discriminator_hidden = discriminator_hidden
        self.generator_activation = generator_activation
        self.discriminator_activation = discriminator_activation
        self.batch_size = batch_size
        self.n_epochs = n_epochs
        self.latent_dim = latent_dim
        self.lr = lr
        self.weight_decay = weight_decay
        self.n_critic = n_critic
        self.verbose = verbose
        self.generator = None
        self.discriminator = None
        self.opt_gen = None
        self.opt_disc = None
        self._core = None

    def _model_init(self, X, C=None):
        """fresh networks and optimizers on EVERY fit, built on the CPU in the reference's order (wgan.py:168-187)"""
        require_hip(DEVICE)
        c_len = 0 if C is None else C.shape[1]
        self.generator = Generator(n_inputs=self.latent_dim + c_len, n_outputs=X.shape[1], hidden=self.generator_hidden,
                                   activation=self.generator_activation)
        self.discriminator = Discriminator(n_inputs=X.shape[1] + c_len, hidden=self.discriminator_hidden,
                                           activation=self.discriminator_activation)
        core = _WganCore(self.generator, self.discriminator, X.shape[1], c_len, self.latent_dim, self.generator_hidden,
                         self.discriminator_hidden, self.generator_activation, self.discriminator_activation, DEVICE)
        self.generator._core = self.discriminator._core = self._core = core
        self.opt_gen = _FlatRMSprop(core.square_avg[:core.PG], self.lr, self.weight_decay)
        self.opt_disc = _FlatRMSprop(core.square_avg[core.PG:core.PG + core.PD], self.lr, self.weight_decay)

    def fit(self, X, C=None):
        self._model_init(X, C)
        core = self._core
        dev = core.device
        Xd = _dev(X, dev)
        Cd = _dev(C, dev)
        n = Xd.shape[0]
        bounds = batch_bounds(n, self.batch_size)
        nb = len(bounds)
        opt = self.opt_gen.hyper(CLAMP)        # both optimizers carry the same hyper-parameters (wgan.py:183-184)
        ws = core.workspace(min(n, self.batch_size), n)
        self.generator.train(True)
        self.discriminator.train(True)
        self.disc_loss_history = []
        self.gen_loss_history = []
        hist = torch.empty(self.n_epochs, 2, dtype=torch.float32, device=dev)   # (gen, disc) per epoch, read back once
        bar = None
        if self.verbose >= 1:
            from tqdm.auto import tqdm
            bar = tqdm(total=self.n_epochs, unit='epoch')
        draws = _FitDraws(n, bounds, self.latent_dim, self.n_epochs, dev)

        def upload(t):
            return t.to(dev, non_blocking=True)

        iter_i = 0
        try:
            for epoch in range(self.n_epochs):
                slot, perm_h, z_h, z_full_h = draws.next_epoch()          # DataLoader(shuffle=True) + the epoch's normals
                perm = upload(perm_h)
                if perm_h.is_cuda:                  # drawn on the worker's stream: tell the allocator who reads it
                    perm.record_stream(torch.cuda.current_stream(dev))
                z_all, z_full = upload(z_h), upload(z_full_h)
                kinds = step_kinds(iter_i, nb, self.n_critic)
                iter_i += nb
                W.fit_epoch(core.shape, core.sync(), core.square_avg, Xd, Cd, perm, z_all, z_full, n, self.batch_size, kinds,
                            opt, hist[epoch], ws)
                ev = torch.cuda.Event()
                ev.record()
                draws.release(slot, ev)             # behind the epoch's last kernel: device-resident noise is read in place
                if bar is not None:
                    if epoch > 0:
                        g, dsc = hist[epoch - 1].tolist()
                        bar.set_description("G loss: %.4f, D loss: %.4f" % (g, dsc))
                    bar.update(1)
            h = hist.cpu()
            draws.finish()
        finally:
            draws.abort()
        for e in range(self.n_epochs):              # wgan.py:291-292: 0-d float32 CPU tensors
            self.gen_loss_history.append(h[e, 0].clone())
            self.disc_loss_history.append(h[e, 1].clone())
        if bar is not None:
            if self.n_epochs:
                bar.set_description("G loss: %.4f, D loss: %.4f" % (float(h[-1, 0]), float(h[-1, 1])))
            bar.close()
        self.generator.train(False)
        self.discriminator.train(False)

    def sample(self, C=10):
        if type(C) != type(1):
            Z = torch.normal(0, 1, (len(C), self.latent_dim))                   # wgan.py:314 (CPU generator)
            X = self.generator(Z, _dev(C, self._core.device))
        else:
            Z = torch.normal(0, 1, (C, self.latent_dim))
            X = self.generator(Z, None)
        return X.cpu().detach().numpy()

    def sample_many(self, C=10, n_draws=100):
        """``np.array([self.sample(C) for _ in range(n_draws)])`` -> float32 numpy [n_draws, n, d] (a name the reference does
        not have): the draws of the notebooks' predictive loop in one launch per window of draws.  Consumes torch's global
        CPU generator exactly as the loop does.  A generator the kernel does not hold in LDS runs the loop itself."""
        from . import _gendraw
        return _gendraw.sample_many(self, C, n_draws)

    def sample_stats(self, C=10, n_draws=100, quantiles=None, ddof=0):
        """Predictive statistics per condition row over ``n_draws`` samples, as ``RealNVP.sample_stats``:
        ``SampleStats(mean, std, min, max, quantiles)`` of float32 numpy arrays [n, d] (quantiles [Q, n, d], numpy's 'linear'
        method, or None).  The latent draws come from torch's global CPU generator exactly as ``n_draws`` successive
        ``sample(C)`` calls draw them; the generator and the reductions across the draws run on the device.  ``n_draws < 1``,
        a probability outside [0, 1] or quantiles with ``n_draws > 8192`` raise ValueError.  A generator the kernel does
        not hold in LDS falls back to the loop on the host (``self.sample`` n_draws times plus numpy)."""
        from . import _gendraw
        return _gendraw.sample_stats(self, C, n_draws, quantiles, ddof)

    def sample_scores(self, C, Y, n_draws=1000, quantiles=(0.05, 0.95), fair=False):
        """Scores of the predictive draws against the observed targets ``Y`` [n, d], as ``RealNVP.sample_scores``:
        ``SampleScores(crps, pit, quantiles, pinball)`` of float32 numpy arrays [n, d] (quantiles and pinball [Q, n, d], or
        None).  The latent draws come from torch's global CPU generator exactly as ``n_draws`` successive ``sample(C)`` calls
        draw them, so a seeded call scores bitwise the draws a seeded ``sample_many`` returns; the generator, the sort and
        the scores run on the device.  ``n_draws < 1``, ``n_draws > 8192``, a probability outside [0, 1] or a ``Y`` whose
        shape is not (n, d) raise ValueError.  A generator the kernel does not hold in LDS falls back to the loop on
        the host (``self.sample`` n_draws times plus numpy)."""
        from . import _gendraw
        return _gendraw.sample_scores(self, C, Y, n_draws, quantiles, fair)

    def sample_joint_scores(self, C, Y, n_draws=1000, fair=False, variogram_order=0.5):
        """Joint scores of the predictive draws against the observed targets ``Y`` [n, d], as ``RealNVP.sample_joint_scores``:
        ``JointScores(energy, spread, variogram)`` of float32 numpy arrays [n] (variogram None when ``variogram_order`` is
        None), each row's draws scored as vectors in R^d.  The latent draws come from torch's global CPU generator exactly as
        ``n_draws`` successive ``sample(C)`` calls draw them, so a seeded call scores the draws a seeded ``sample_many``
        returns; the generator and the scores run on the device.  ``n_draws < 1``, ``n_draws > 8192``, an order other than
        0.5, 1 or 2, or a ``Y`` whose shape is not (n, d) raise ValueError.
        A generator the kernel does not hold in LDS falls back to the loop on the host (``self.sample`` n_draws times
        plus numpy)."""
        from . import _gendraw
        return _gendraw.sample_joint_scores(self, C, Y, n_draws, fair, variogram_order)
