"""Float64 torch-CPU restatement of ConditionalWGAN (reference probaforms/models/wgan.py) for the GPU tests: one iteration's
loss and gradient, RMSprop + clamp in float32 with torch's separately rounded order, the epoch-end losses, the RNG replay
of a fit, and a whole fit.  Parameters are flat: every nn.Linear's weight then bias, generator first."""
import numpy as np
import torch

from restatement_ops import affine


def widths(n_in, hidden, n_out):
    return list(zip([n_in] + list(hidden), list(hidden) + [n_out]))


def n_params(n_in, hidden, n_out):
    return sum(i * o + o for i, o in widths(n_in, hidden, n_out))


class Net:
    def __init__(self, n_in, hidden, n_out, act, sequential=False):
        self.w = widths(n_in, hidden, n_out)
        self.act = act
        self.P = n_params(n_in, hidden, n_out)
        self.sequential = sequential

    def split(self, flat):
        out, off = [], 0
        for i, o in self.w:
            W = flat[off:off + i * o].reshape(o, i); off += i * o
            b = flat[off:off + o]; off += o
            out.append((W, b))
        return out

    def __call__(self, flat, x):
        layers = self.split(flat)
        for k, (W, b) in enumerate(layers):
            x = affine(x, W, b, self.sequential)
            if k < len(layers) - 1:
                x = torch.tanh(x) if self.act == 'tanh' else torch.relu(x)
        return x


class Wgan:
    """the two nets of one shape; G: latent + c -> d, D: d + c -> 1"""

    def __init__(self, d, c, latent, g_hidden, d_hidden, g_act='relu', d_act='relu', sequential=False):
        self.d, self.c, self.latent = d, c, latent
        self.G = Net(latent + c, g_hidden, d, g_act, sequential)
        self.D = Net(d + c, d_hidden, 1, d_act, sequential)
        self.PG, self.PD = self.G.P, self.D.P

    @staticmethod
    def _cat(a, c):
        return a if c is None or c.shape[1] == 0 else torch.cat([a, c], 1)

    def loss_grad(self, params, X, C, rows, z, kind, dtype=torch.float64):
        """(loss, gradient of the stepped net) in `dtype`; kind 1 = critic step, 0 = generator step"""
        p = torch.tensor(np.asarray(params[:self.PG + self.PD]), dtype=dtype, requires_grad=True)
        pG, pD = p[:self.PG], p[self.PG:]
        x = torch.tensor(np.asarray(X)[rows], dtype=dtype)
        c = None if C is None or np.asarray(C).shape[1] == 0 else torch.tensor(np.asarray(C)[rows], dtype=dtype)
        fake = self.G(pG, self._cat(torch.tensor(np.asarray(z), dtype=dtype), c))
        if kind == 1:
            loss = -self.D(pD, self._cat(x, c)).mean() + self.D(pD, self._cat(fake, c)).mean()
        else:
            loss = -self.D(pD, self._cat(fake, c)).mean()
        loss.backward()
        g = p.grad.numpy()
        return float(loss.detach()), (g[self.PG:] if kind == 1 else g[:self.PG]).copy()

    def grad_scale(self, params, X, C, rows, z, kind):
        """max |gradient| of each of the loss's mean terms alone: a critic step's two terms cancel, and float32 sums of
        them carry an error relative to the terms, not to their difference"""
        if kind == 0:
            return np.abs(self.loss_grad(params, X, C, rows, z, 0)[1]).max()
        p = torch.tensor(np.asarray(params[:self.PG + self.PD], np.float64), requires_grad=True)
        x = torch.tensor(np.asarray(X)[rows], dtype=torch.float64)
        c = None if C is None or np.asarray(C).shape[1] == 0 else torch.tensor(np.asarray(C)[rows], dtype=torch.float64)
        fake = self.G(p[:self.PG], self._cat(torch.tensor(np.asarray(z), dtype=torch.float64), c)).detach()
        out = 0.0
        for inp in (x, fake):
            g, = torch.autograd.grad(self.D(p[self.PG:], self._cat(inp, c)).mean(), p)
            out = max(out, float(g[self.PG:].abs().max()))
        return out

    def epoch_losses(self, params, X, C, Z, dtype=torch.float64):
        p = torch.tensor(np.asarray(params[:self.PG + self.PD]), dtype=dtype)
        x = torch.tensor(np.asarray(X), dtype=dtype)
        c = None if C is None or np.asarray(C).shape[1] == 0 else torch.tensor(np.asarray(C), dtype=dtype)
        fake = self.G(p[:self.PG], self._cat(torch.tensor(np.asarray(Z), dtype=dtype), c))
        gen = -self.D(p[self.PG:], self._cat(fake, c)).mean()
        disc = self.D(p[self.PG:], self._cat(x, c)).mean() + gen
        return float(gen), float(disc)

    def generate(self, params, Z, C, dtype=torch.float64):
        p = torch.tensor(np.asarray(params[:self.PG]), dtype=dtype)
        c = None if C is None else torch.tensor(np.asarray(C), dtype=dtype)
        return self.G(p, self._cat(torch.tensor(np.asarray(Z), dtype=dtype), c)).numpy()

    def critic(self, params, X, C, dtype=torch.float64):
        p = torch.tensor(np.asarray(params[self.PG:self.PG + self.PD]), dtype=dtype)
        c = None if C is None else torch.tensor(np.asarray(C), dtype=dtype)
        return self.D(p, self._cat(torch.tensor(np.asarray(X), dtype=dtype), c)).numpy()


def rmsprop_f32(p, g, v, lr, alpha=0.99, eps=1e-8, wd=0.0, clamp=0.0):
    """torch.optim.RMSprop's single-tensor step in float32, one rounding per op; then clamp_(-clamp, clamp) if clamp"""
    f = np.float32
    p, g, v = p.astype(f), g.astype(f), v.astype(f)
    if wd != 0:
        g = g + f(wd) * p
    v = v * f(alpha) + (f(1.0 - alpha) * g) * g
    avg = np.sqrt(v) + f(eps)
    p = p + f(-lr) * (g / avg)
    if clamp:
        p = np.minimum(np.maximum(p, f(-clamp)), f(clamp))
    return p, v


def replay_draws(state, n, batch_size, latent, n_epochs):
    """the fit's per-epoch batch rows, per-batch noise and epoch-end noise, replayed from the global generator state the
    fit starts its batch loop from; returns (epochs, end_state)"""
    g = torch.Generator()
    g.set_state(state)
    epochs = []
    for _ in range(n_epochs):
        torch.empty((), dtype=torch.int64).random_(generator=g)
        seed = int(torch.empty((), dtype=torch.int64).random_(generator=g).item())
        pg = torch.Generator()
        pg.manual_seed(seed)
        perm = torch.randperm(n, generator=pg).numpy()
        batches = []
        for s in range(0, n, batch_size):
            e = min(s + batch_size, n)
            batches.append((perm[s:e], torch.normal(0, 1, (e - s, latent), generator=g).numpy()))
        Z = torch.normal(0, 1, (n, latent), generator=g).numpy()
        epochs.append((batches, Z))
    return epochs, g.get_state()


def fit(wg, params, X, C, epochs, lr, n_critic, wd=0.0, clamp=0.01):
    """the reference's fit loop on replayed draws: float64 gradients, float32 RMSprop (the parameters stay float32)"""
    p = np.asarray(params, np.float32).copy()
    v = np.zeros_like(p)
    it = 0
    hist = []
    for batches, Z in epochs:
        for rows, z in batches:
            kind = 1 if it % n_critic != 0 else 0
            _, g = wg.loss_grad(p, X, C, rows, z, kind)
            sl = slice(wg.PG, wg.PG + wg.PD) if kind == 1 else slice(0, wg.PG)
            p[sl], v[sl] = rmsprop_f32(p[sl], g, v[sl], lr, wd=wd, clamp=clamp if kind == 1 else 0.0)
            it += 1
        hist.append(wg.epoch_losses(p, X, C, Z))
    return p, hist
