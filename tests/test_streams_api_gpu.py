"""The public API under a current stream that is not the default one: every model, metric, two-sample test and loss gives, under
`with torch.cuda.stream(s)`, the bits it gives under the default stream.  The entry points' own stream argument is held by
tests/test_streams_{flow,metrics,models}_gpu.py; this module covers the hand-offs the Python layer makes itself -- draws and copies on
side streams of its own with wait_event / record_stream (nflow.py, cvae.py, wgan.py, cnormal.py, _engine.py), the pinned double buffers
of metrics/_boot.run_groups -- which are right only if they are ordered against the CALLER's stream, not against stream 0.

A side-stream run starts behind a gate (streams.gate_cycles, about 0.1 s): the inputs are device tensors that hold decoys (half the
values, rows rolled by one: valid data, wrong numbers) until a copy enqueued on s behind the gate puts the real rows there, so work
that the layer orders against stream 0 in place of s reads the decoys.  Both runs start from the same seeds of torch's and numpy's
global generators.  Shapes are the smallest of the models' own tests: two epochs, a ragged last batch.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import streams  # noqa: E402

pytestmark = pytest.mark.gpu

N, D, CD = 70, 3, 2                     # 70 rows in batches of 32: two full batches and a ragged one of 6


def _data(seed, n=N, d=D, c=CD):
    rng = np.random.default_rng(seed)
    C = rng.standard_normal((n, c)).astype(np.float32)
    X = (C @ rng.standard_normal((c, d)) + 0.3 * rng.standard_normal((n, d))).astype(np.float32)
    return X, C


def _flat(v, out):
    """every array in a result (tensors, numpy arrays, numbers, tuples of them), in order"""
    if v is None:
        return out
    if torch.is_tensor(v):
        out.append(v.detach().cpu().numpy())
    elif isinstance(v, (list, tuple)):
        for e in v:
            _flat(e, out)
    else:
        out.append(np.asarray(v))
    return out


def _run(job, arrays, side):
    torch.manual_seed(11)
    np.random.seed(11)
    if not side:
        dev = [torch.from_numpy(a).cuda() for a in arrays]
        out = _flat(job(*dev), [])
        torch.cuda.synchronize()
        return out
    s = streams.side_stream()
    pinned = [torch.from_numpy(a).pin_memory() for a in arrays]
    dev = [streams.decoy(torch.from_numpy(a).cuda(), 0).contiguous() for a in arrays]
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        torch.cuda._sleep(streams.gate_cycles())
        for t, p in zip(dev, pinned):
            t.copy_(p, non_blocking=True)
        out = _flat(job(*dev), [])
    s.synchronize()
    torch.cuda.synchronize()
    return out


def _same_under_a_side_stream(what, job, arrays):
    want = _run(job, arrays, side=False)
    got = _run(job, arrays, side=True)
    assert len(want) == len(got) and len(want) > 0, what
    for i, (a, b) in enumerate(zip(want, got)):
        assert a.shape == b.shape and a.dtype == b.dtype, (what, i, a.shape, b.shape)
        assert a.tobytes() == b.tobytes(), "%s: result %d of %d differs under a side stream (max |diff| %r)" % (
            what, i, len(want), float(np.nanmax(np.abs(a.astype(np.float64) - b.astype(np.float64)))) if a.size else 0.0)
    again = _run(job, arrays, side=False)                        # the comparison means something: the default-stream run repeats itself
    assert all(a.tobytes() == b.tobytes() for a, b in zip(want, again)), "%s: two default-stream runs differ" % what


# ---- the models ---------------------------------------------------------------------------------------------------------------------
def _model_job(make, history, host=None):
    """host: the arrays themselves, for a model whose fit takes numpy arrays alone (CVAE, as the reference's): its uploads are
    the model's own, made under the current stream behind the gate"""
    def job(X, C):
        if host is not None:
            X, C = host
        m = make()
        m.fit(X, C)
        out = [torch.stack([torch.as_tensor(v).reshape(()) for v in getattr(m, h)]) for h in history]
        out.append(m.sample(C))
        out.append(tuple(m.sample_stats(C, n_draws=19, quantiles=(0.1, 0.9))))
        out.append(tuple(m.sample_scores(C, X, n_draws=19)))
        out.append(tuple(m.sample_joint_scores(C, X, n_draws=19)))
        out.append(m.sample_many(C, n_draws=3))
        return out
    return job


def _models():
    from probaforms_amd.models import CVAE, ConditionalNormal, ConditionalWGAN, RealNVP
    kw = dict(batch_size=32, n_epochs=2, lr=1e-2)
    return {
        "RealNVP": (lambda: RealNVP(n_layers=2, hidden=(10,), **kw), ["loss_history"]),                       # the resident epoch
        "RealNVP-device-prior": (lambda: RealNVP(n_layers=2, hidden=(10,), prior_rng="device", **kw), ["loss_history"]),   # host seeds
        "RealNVP-two-hidden": (lambda: RealNVP(n_layers=2, hidden=(40, 40), **kw), ["loss_history"]),         # the batch-by-batch loop
        "CVAE": (lambda: CVAE(latent_dim=2, hidden=(10,), **kw), ["loss_history"]),
        "CVAE-device-noise": (lambda: CVAE(latent_dim=2, hidden=(40, 40), noise_rng="device", **kw), ["loss_history"]),
        "ConditionalWGAN": (lambda: ConditionalWGAN(latent_dim=2, generator_hidden=(10,), discriminator_hidden=(10,), n_critic=2, **kw),
                            ["gen_loss_history", "disc_loss_history"]),
        "ConditionalNormal": (lambda: ConditionalNormal(hidden=(10,), **kw), ["loss_history"]),
        "ConditionalNormal-independent": (lambda: ConditionalNormal(use_independent_covariance=True, hidden=(10,), **kw), ["loss_history"]),
    }


@pytest.mark.parametrize("name", ["RealNVP", "RealNVP-device-prior", "RealNVP-two-hidden", "CVAE", "CVAE-device-noise", "ConditionalWGAN",
                                  "ConditionalNormal", "ConditionalNormal-independent"])
def test_fit_and_sampling(name):
    make, history = _models()[name]
    arrays = _data(3)
    _same_under_a_side_stream(name, _model_job(make, history, host=arrays if name.startswith("CVAE") else None), arrays)


# ---- metrics and two-sample tests ------------------------------------------------------------------------------------------------------
def _metrics():
    from probaforms_amd.metrics import div1d, energy, fd, ks1d, mmd, prdc, sinkhorn, twosample, wasserstein
    it = dict(n_iters=7)
    return {
        "maximum_mean_discrepancy": lambda A, B: mmd.maximum_mean_discrepancy(A, B, **it),
        # more replicates than one group holds: the second group's indices upload while the first group's kernels run
        "maximum_mean_discrepancy-two-groups": lambda A, B: mmd.maximum_mean_discrepancy(A, B, n_iters=130, standardize=True),
        "frechet_distance": lambda A, B: fd.frechet_distance(A, B, **it),
        "kolmogorov_smirnov_1d": lambda A, B: ks1d.kolmogorov_smirnov_1d(A, B, **it),
        "cramer_von_mises_1d": lambda A, B: ks1d.cramer_von_mises_1d(A, B, **it),
        "roc_auc_score_1d": lambda A, B: ks1d.roc_auc_score_1d(A, B, **it),
        "anderson_darling_1d": lambda A, B: ks1d.anderson_darling_1d(A, B, **it),
        "kullback_leibler_1d": lambda A, B: div1d.kullback_leibler_1d(A, B, **it),
        "jensen_shannon_1d": lambda A, B: div1d.jensen_shannon_1d(A, B, **it),
        "kullback_leibler_1d_kde": lambda A, B: div1d.kullback_leibler_1d_kde(A, B, **it),
        "jensen_shannon_1d_kde": lambda A, B: div1d.jensen_shannon_1d_kde(A, B, **it),
        "wasserstein_1d": lambda A, B: wasserstein.wasserstein_1d(A, B, **it),
        "sliced_wasserstein_distance": lambda A, B: wasserstein.sliced_wasserstein_distance(A, B, n_projections=9, **it),
        "sliced_wasserstein_full_sample": lambda A, B: wasserstein.sliced_wasserstein_full_sample(A, B, n_projections=9),
        "prdc": lambda A, B: prdc.prdc(A, B, nearest_k=3, **it),
        "prdc_full_sample": lambda A, B: prdc.prdc_full_sample(A, B, nearest_k=3),
        "energy_distance": lambda A, B: energy.energy_distance(A, B, **it),
        "energy_distance_full_sample": lambda A, B: energy.energy_distance_full_sample(A, B),
        "sinkhorn_divergence": lambda A, B: sinkhorn.sinkhorn_divergence(A, B, n_sinkhorn=5, **it),
        "sinkhorn_divergence_full_sample": lambda A, B: sinkhorn.sinkhorn_divergence_full_sample(A, B, n_sinkhorn=5),
        "energy_test": lambda A, B: twosample.energy_test(A, B, n_permutations=19),
        "mmd_test": lambda A, B: twosample.mmd_test(A, B, n_permutations=19),
        "knn_test": lambda A, B: twosample.knn_test(A, B, n_permutations=19, nearest_k=2),
        "nn_accuracy_full_sample": lambda A, B: twosample.nn_accuracy_full_sample(A, B),
    }


METRICS = ["maximum_mean_discrepancy", "maximum_mean_discrepancy-two-groups", "frechet_distance", "kolmogorov_smirnov_1d",
           "cramer_von_mises_1d", "roc_auc_score_1d", "anderson_darling_1d", "kullback_leibler_1d", "jensen_shannon_1d",
           "kullback_leibler_1d_kde", "jensen_shannon_1d_kde", "wasserstein_1d", "sliced_wasserstein_distance",
           "sliced_wasserstein_full_sample", "prdc", "prdc_full_sample", "energy_distance", "energy_distance_full_sample",
           "sinkhorn_divergence", "sinkhorn_divergence_full_sample", "energy_test", "mmd_test", "knn_test", "nn_accuracy_full_sample"]


def test_the_metric_list_is_the_table():
    assert METRICS == list(_metrics())


@pytest.mark.parametrize("name", METRICS)
def test_metrics_and_two_sample_tests(name):
    A, _ = _data(5, n=70)
    B, _ = _data(6, n=65)
    _same_under_a_side_stream(name, _metrics()[name], (A.astype(np.float64), B.astype(np.float64) + 0.2))


# ---- the losses, with backward -----------------------------------------------------------------------------------------------------------
def _losses():
    from probaforms_amd.metrics import losses
    return {
        "energy_loss": lambda A, B: losses.energy_loss(A, B),
        "mmd_loss": lambda A, B: losses.mmd_loss(A, B),
        "sinkhorn_loss": lambda A, B: losses.sinkhorn_loss(A, B, n_sinkhorn=5),
        "sliced_wasserstein_loss": lambda A, B: losses.sliced_wasserstein_loss(A, B, n_projections=9),
        "wasserstein_1d_loss": lambda A, B: losses.wasserstein_1d_loss(A, B),
    }


@pytest.mark.parametrize("name", ["energy_loss", "mmd_loss", "sinkhorn_loss", "sliced_wasserstein_loss", "wasserstein_1d_loss"])
def test_two_sample_losses_with_backward(name):
    fn = _losses()[name]

    def job(A, B):
        fake = B.clone().requires_grad_(True)
        real = A.clone().requires_grad_(True)
        loss = fn(real, fake)
        loss.backward()
        return [loss, fake.grad, real.grad]

    A, _ = _data(7, n=70)
    B, _ = _data(8, n=65)
    _same_under_a_side_stream(name, job, (A.astype(np.float64), B.astype(np.float64) + 0.2))


@pytest.mark.parametrize("name", ["energy_score_loss", "crps_loss"])
@pytest.mark.parametrize("fair", [False, True])
def test_score_losses_with_backward(name, fair):
    from probaforms_amd.metrics import losses
    fn = getattr(losses, name)

    def job(Xk, Y):
        draws = Xk.clone().requires_grad_(True)
        target = Y.clone().requires_grad_(True)
        loss = fn(draws, target, fair=fair)
        loss.backward()
        return [loss, draws.grad, target.grad]

    rng = np.random.default_rng(9)
    _same_under_a_side_stream("%s, fair %s" % (name, fair), job, (rng.standard_normal((19, 33, D)), rng.standard_normal((33, D))))
