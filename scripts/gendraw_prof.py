"""Where a sample_stats call of CVAE, ConditionalWGAN or ConditionalNormal spends its time: run one shape
under `rocprofv3 --kernel-trace --stats -- python scripts/gendraw_prof.py <shape>` for the per-kernel times
(profiles/r12_gendraw_<shape>_kernel_stats.csv: 15 calls with quantiles, so every kernel of the call shows 15 dispatches per
draw window); the script itself prints the host side: the call's wall time, the CPU noise draw and its upload, medians of 10.
Shapes: wgan, cvae, c5, cnormal (those of scripts/gendraw_time.py)."""
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from probaforms_amd.models import CVAE, ConditionalNormal, ConditionalWGAN  # noqa: E402
from probaforms_amd.models import _gendraw as G  # noqa: E402

SHAPES = {"wgan": (lambda: ConditionalWGAN(n_epochs=1), 1, 1, 1000, 1000),
          "cvae": (lambda: CVAE(n_epochs=1), 1, 1, 1000, 1000),
          "c5": (lambda: CVAE(latent_dim=2, hidden=(128,), n_epochs=1, batch_size=64), 16, 4, 4096, 256),
          "cnormal": (lambda: ConditionalNormal(n_epochs=1), 1, 1, 1000, 1000)}


def main():
    name = sys.argv[1]
    make, d, c, n, K = SHAPES[name]
    rng = np.random.default_rng(0)
    torch.manual_seed(0)
    m = make()
    m.fit(rng.standard_normal((256, d)).astype(np.float32), rng.standard_normal((256, c)).astype(np.float32))
    C = rng.standard_normal((n, c)).astype(np.float32)
    width = d if name == "cnormal" else m.latent_dim
    for _ in range(5):
        m.sample_stats(C, K, quantiles=(0.05, 0.95))
    torch.cuda.synchronize()
    wall, draw, up = [], [], []
    for _ in range(10):
        t0 = time.perf_counter()
        m.sample_stats(C, K, quantiles=(0.05, 0.95))
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
    for _ in range(10):
        t0 = time.perf_counter()
        z = G.noise(K, n, width)
        t1 = time.perf_counter()
        z.to("cuda")
        torch.cuda.synchronize()
        draw.append((t1 - t0) * 1e3)
        up.append((time.perf_counter() - t1) * 1e3)
    print("HOST %s n=%d K=%d width=%d one_stream=%s: sample_stats + quantiles %.3f ms; noise on the CPU %.3f ms; upload %.3f ms"
          % (name, n, K, width, G.one_stream(n, width), statistics.median(wall), statistics.median(draw), statistics.median(up)),
          flush=True)


if __name__ == "__main__":
    main()
