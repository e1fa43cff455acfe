"""probaforms_amd -- the conditional RealNVP hot path of hse-cs/probaforms, rebuilt for MI355X.

    from probaforms_amd.models import RealNVP      # mirrors `from probaforms.models import RealNVP`
    from probaforms_amd.metrics import maximum_mean_discrepancy, frechet_distance   # probaforms.metrics, GPU

Only the path named in BASELINE.json is implemented: the affine
coupling stack forward/inverse/backward as hand-written HIP kernels behind the reference's
sklearn-style ``RealNVP.fit(X, C)`` / ``.sample(C)`` API, the CVAE, the ConditionalWGAN and the ConditionalNormal (training and
sampling kernels in their own HIP libraries), and the metrics of ``probaforms.metrics`` on their own HIP library:
the two multivariate ones (MMD, Frechet distance) and the eight 1-D ones in ``probaforms_amd.metrics.ks1d`` and
``probaforms_amd.metrics.div1d``.  There is no CPU fallback.
"""
__version__ = "0.1.0"


def install_as_probaforms():
    """Make `from probaforms.models import RealNVP` (the reference's import path, README.md:48) and
    `from probaforms import metrics` resolve to this package: registers `probaforms`, `probaforms.models`, the
    model modules and `probaforms.metrics` in sys.modules.  `probaforms.metrics` exports exactly
    maximum_mean_discrepancy and frechet_distance: the reference's 1-D metrics are served from
    probaforms_amd.metrics.ks1d / div1d only, so importing one of them (e.g. kolmogorov_smirnov_1d) from
    probaforms.metrics raises ImportError.
    Call it before anything imports the reference; it refuses to shadow an already imported one."""
    import sys
    import types
    from . import models
    from .models import cnormal, cvae, interfaces, nflow, realnvp, wgan
    existing = sys.modules.get("probaforms")
    if existing is not None and getattr(existing, "__probaforms_amd__", False) is False:
        raise RuntimeError("a different `probaforms` package is already imported (%s)"
                           % getattr(existing, "__file__", "?"))
    pkg = types.ModuleType("probaforms")
    pkg.__probaforms_amd__ = True
    pkg.__path__ = []                      # a package, with no importable submodules of its own
    pkg.models = models
    from . import metrics as _metrics
    met = types.ModuleType("probaforms.metrics", _metrics.__doc__)
    for name in _metrics.__all__:
        setattr(met, name, getattr(_metrics, name))
    met.__all__ = list(_metrics.__all__)
    pkg.metrics = met
    sys.modules["probaforms.metrics"] = met
    sys.modules["probaforms"] = pkg
    sys.modules["probaforms.models"] = models
    for name, mod in (("realnvp", realnvp), ("nflow", nflow), ("interfaces", interfaces), ("cvae", cvae), ("wgan", wgan),
                      ("cnormal", cnormal)):
        sys.modules["probaforms.models." + name] = mod
    return pkg
