"""Torch-CPU restatement of ConditionalNormal (reference probaforms/models/cnormal.py) for the tests, written from the model's
description: one batch's loss and gradient by autograd, torch.optim.Adam over the flat parameters, Net.forward, the RNG
replay of a fit, and a whole fit -- in float64 (the yardstick the GPU tests measure errors against) or float32 (which must
reproduce the reference's own numbers, tests/test_cnormal_host.py).  Parameters are flat: every nn.Linear's weight then
bias, in module order model.*, mu, log_sigma, out."""
import numpy as np
import torch

from restatement_ops import affine

ACTS = {'tanh': torch.tanh, 'relu': torch.relu, 'sigmoid': torch.sigmoid}


class Normal:
    def __init__(self, d, c, hidden=(10,), activation='tanh', independent=False, sequential=False):
        self.d, self.c, self.hidden, self.independent = d, c, tuple(hidden), bool(independent)
        self.sequential = sequential
        self.act = ACTS.get(activation, torch.relu)           # anything else means ReLU
        w = list(zip([c] + list(hidden[:-1]), hidden))
        self.trunk = w
        self.heads = [(hidden[-1], d), (hidden[-1], d)]
        self.P_main = sum(i * o + o for i, o in w + self.heads)
        self.P = self.P_main + d * d + d

    def split(self, flat):
        out, off = [], 0
        for i, o in self.trunk + self.heads + [(self.d, self.d)]:
            W = flat[off:off + i * o].reshape(o, i); off += i * o
            b = flat[off:off + o]; off += o
            out.append((W, b))
        return out[:-3], out[-3], out[-2], out[-1]

    def net(self, flat, C, X=None, eps=None):
        """(x_tilde, inv, mu, sigma) as tensors of flat's dtype; x_tilde None without eps, inv None without X"""
        trunk, (Wm, bm), (Wl, bl), (Wo, bo) = self.split(flat)
        h = C
        for W, b in trunk:
            h = self.act(affine(h, W, b, self.sequential))
        mu = affine(h, Wm, bm, self.sequential)
        sigma = torch.exp(affine(h, Wl, bl, self.sequential))
        xt = None
        if eps is not None:
            xt = mu + eps * sigma
            if not self.independent:
                xt = affine(xt, Wo, bo, self.sequential)
        inv = None if X is None else (X - bo) @ torch.linalg.inv(Wo.T)
        return xt, inv, mu, sigma

    def loss(self, flat, X, C):
        _, inv, mu, sigma = self.net(flat, C, X)
        t = X if self.independent else inv
        return ((t - mu) ** 2 / (2 * sigma ** 2) + torch.log(sigma)).mean()

    def loss_grad(self, params, X, C, rows=None, dtype=torch.float64):
        """(loss, gradient [P]) of the batch rows; in independent mode the out block of the gradient is zero"""
        p = torch.tensor(np.asarray(params)[:self.P], dtype=dtype, requires_grad=True)
        rows = slice(None) if rows is None else np.asarray(rows)
        x = torch.tensor(np.asarray(X)[rows], dtype=dtype)
        c = torch.tensor(np.asarray(C)[rows], dtype=dtype)
        loss = self.loss(p, x, c)
        loss.backward()
        g = p.grad.numpy().copy()
        if self.independent:
            g[self.P_main:] = 0
        return loss.detach().numpy().copy(), g

    def forward(self, params, C, eps=None, X=None, dtype=torch.float64):
        p = torch.tensor(np.asarray(params)[:self.P], dtype=dtype)
        t = lambda a: None if a is None else torch.tensor(np.asarray(a), dtype=dtype)
        return tuple(None if o is None else o.numpy() for o in self.net(p, t(C), t(X), t(eps)))

    def cond_out(self, params):
        W = np.asarray(params, np.float64)[self.P_main:self.P_main + self.d * self.d].reshape(self.d, self.d)
        return float(np.linalg.cond(W))


def replay_draws(state, n, batch_size, d, n_epochs):
    """the fit's per-epoch batch rows, replayed from the global generator state the fit starts its batch loop from: per
    epoch two int64 seed draws (a fresh DataLoader(shuffle=True)), a randperm on a private generator, and one randn(rows, d)
    per batch (the forward's noise, unused by the loss); returns (epochs, end_state)"""
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
            batches.append(perm[s:e].copy())
            torch.randn(e - s, d, generator=g)
        epochs.append(batches)
    return epochs, g.get_state()


def fit(model, params, X, C, batches, lr, wd=0.0, dtype=torch.float64, hook=None):
    """the reference's loop over `batches` (a flat list of row arrays): autograd + torch.optim.Adam(lr, weight_decay), all
    in `dtype`.  out is its own leaf: in independent mode it gets no gradient and Adam skips it entirely.
    hook(k, loss, grad [P], params_before [P]) per step.  Returns (final parameters [P] as float64, losses)"""
    p0 = np.asarray(params)[:model.P]
    pm = torch.tensor(p0[:model.P_main], dtype=dtype, requires_grad=True)
    po = torch.tensor(p0[model.P_main:], dtype=dtype, requires_grad=True)
    opt = torch.optim.Adam([pm, po], lr=lr, weight_decay=wd)
    x, c = torch.tensor(np.asarray(X), dtype=dtype), torch.tensor(np.asarray(C), dtype=dtype)
    losses = []
    for k, rows in enumerate(batches):
        rows = torch.as_tensor(np.asarray(rows))
        loss = model.loss(torch.cat([pm, po.detach() if model.independent else po]), x[rows], c[rows])
        opt.zero_grad()
        loss.backward()
        if hook is not None:
            g = torch.cat([pm.grad, po.grad if po.grad is not None else torch.zeros_like(po)])
            hook(k, loss.detach().numpy().copy(), g.numpy().copy(), torch.cat([pm, po]).detach().numpy().copy())
        opt.step()
        losses.append(loss.detach().numpy().copy())
    return torch.cat([pm, po]).detach().numpy().astype(np.float64), np.array(losses)
