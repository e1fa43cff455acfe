"""Arithmetic shared by the torch restatements (tests/wgan_torch.py, tests/cnormal_torch.py)."""


def affine(x, W, b, sequential=False):
    """x W^T + b.  sequential: one rounded multiply and one rounded add per input, in input order -- the order of the
    kernels' fmaf chain over a layer's fan-in (torch's matmul splits the sum over vector lanes and blocks)"""
    if not sequential:
        return x @ W.T + b
    acc = b.expand(x.shape[0], -1)
    for xi, wi in zip(x.unbind(1), W.unbind(1)):          # unbind: one backward node for all columns
        acc = acc + xi[:, None] * wi
    return acc
