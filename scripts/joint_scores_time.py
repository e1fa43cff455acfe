"""Warm timings of the joint scores (energy score, variogram score of order 0.5) of the predictive draws, three ways, in one
process (profiles/r14_joint_time.txt), with the method of scripts/scores_time.py:
  (a) model.sample_many(C, K), the download it includes, then the scores in blocked numpy (joint_scores_of_draws)
  (b) the draws kept on the device [K, n, d], then torch.cdist over [n, K, K] and torch reductions in float32; the peak of
      torch's allocator during the call is noted
  (c) model.sample_joint_scores(C, Y, K)
  (s) model.sample_scores(C, Y, K) at the same shape: the same draws, scored per column
  (k) pfp_joint_scores alone on resident transposed draws of that shape (all three outputs)
Each variant is warmed for as many calls as are timed; the figure is the median wall time per call with a device
synchronisation at both ends.  The numbers to read are (c) against (b), and (c) - (s).
Usage: python scripts/joint_scores_time.py [out.txt]"""
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from probaforms_amd.models import CVAE, ConditionalNormal, RealNVP  # noqa: E402
from probaforms_amd.models import _gendraw, _predict_lib  # noqa: E402
from probaforms_amd.models._predict import joint_scores_of_draws  # noqa: E402


def timed(fn, reps):
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def device_draws(m, C, K):
    """[K, n, d] on the device: sample_many without its download"""
    if isinstance(m, RealNVP):
        return m.nf.sample_many(torch.from_numpy(C).cuda(), K)
    job, conditions = _gendraw.job_of(m)
    n, Cd = conditions(C)
    return _gendraw.reduce_draws(_gendraw.JobSource(job, Cd), n, K, None, 0, False, True)[1]


def torch_scores(X, Y):
    """energy, spread and the variogram of order 0.5 from device draws X [K, n, d], as one would write them with torch"""
    K = X.shape[0]
    x = X.permute(1, 0, 2).contiguous()                              # [n, K, d]
    spread = torch.cdist(x, x).sum(dim=(1, 2)) / (2.0 * K * K)       # [n, K, K]
    energy = (x - Y[:, None]).norm(dim=2).mean(dim=1) - spread
    m = (x[:, :, :, None] - x[:, :, None, :]).abs().sqrt().mean(dim=1)
    v = ((Y[:, :, None] - Y[:, None, :]).abs().sqrt() - m).square().sum(dim=(1, 2))
    return energy, spread, v


def main():
    out = open(sys.argv[1], "w") if len(sys.argv) > 1 else sys.stdout
    nvp = lambda prior_rng: (lambda: RealNVP(n_epochs=1, batch_size=64, prior_rng=prior_rng, hidden=(128,)))
    shapes = [("C2 net: 8 layers hidden=(128,), d=16 c=4 n=4096 K=256, prior_rng=host", nvp("host"), 16, 4, 4096, 256),
              ("C2 net: 8 layers hidden=(128,), d=16 c=4 n=4096 K=256, prior_rng=device", nvp("device"), 16, 4, 4096, 256),
              ("CVAE C5 net (hidden 128 tanh, latent 2), d=16 c=4 n=4096 K=256",
               lambda: CVAE(latent_dim=2, hidden=(128,), n_epochs=1, batch_size=64), 16, 4, 4096, 256),
              ("ConditionalNormal, full covariance, d=5 c=1 n=1000 K=1000", lambda: ConditionalNormal(n_epochs=1), 5, 1, 1000,
               1000)]
    print("median [min .. max] ms per call; warm-up = as many calls as timed; %s" % torch.cuda.get_device_name(0), file=out)
    for title, make, d, c, n, K in shapes:
        rng = np.random.default_rng(0)
        torch.manual_seed(0)
        m = make()
        m.fit(rng.standard_normal((256, d)).astype(np.float32), rng.standard_normal((256, c)).astype(np.float32))
        C = rng.standard_normal((n, c)).astype(np.float32)
        Y = rng.standard_normal((n, d)).astype(np.float32)
        Yd = torch.from_numpy(Y).cuda()
        t = _predict_lib.joint_tiling(d, K)
        xt = torch.randn(n, d, K, device="cuda")
        outs = [torch.empty(n, device="cuda") for _ in range(3)]

        def many_numpy():
            return joint_scores_of_draws(m.sample_many(C, K), Y, False, 0.5)

        def on_device():
            return [a.cpu() for a in torch_scores(device_draws(m, C, K), Yd)]

        def joint():
            return m.sample_joint_scores(C, Y, K)

        def scores():
            return m.sample_scores(C, Y, K)

        def kernel():
            _predict_lib.joint_scores(xt, Yd, n, d, K, False, 0.5, *outs)

        print("\n%s   [tile %d draws x %d, %d B of LDS]" % (title, t.tile_draws, t.n_tiles, t.lds_bytes), file=out)
        med = {}
        for label, fn, reps in [("(a) sample_many + blocked numpy", many_numpy, 1),
                                ("(b) device draws + torch.cdist + reductions", on_device, 10),
                                ("(c) sample_joint_scores", joint, 20),
                                ("(s) sample_scores", scores, 20),
                                ("(k) pfp_joint_scores alone", kernel, 20)]:
            if label[:3] == "(b)":
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
            med[label[:3]] = timed(fn, reps)
            print("  %-50s %10.3f  [%9.3f .. %9.3f]" % ((label,) + med[label[:3]]), file=out)
            if label[:3] == "(b)":
                print("      peak device memory of (b): %.2f GiB" % (torch.cuda.max_memory_allocated() / 2.0 ** 30), file=out)
            out.flush()
        print("  (c) - (s) = %.3f ms; (c) / (b) = %.4f; (c) / (a) = %.5f"
              % (med["(c)"][0] - med["(s)"][0], med["(c)"][0] / med["(b)"][0], med["(c)"][0] / med["(a)"][0]), file=out)
        out.flush()
    if out is not sys.stdout:
        out.close()


if __name__ == "__main__":
    main()
