"""sample_stats / sample_many of CVAE, ConditionalWGAN and ConditionalNormal: everything that needs no GPU -- the binding
against the header's text, the launch plan, the noise stream, the routing to the host loop and argument validation."""
import os
import re
import types

import numpy as np
import pytest
import torch

import native_libs
from probaforms_amd.models import _cnormal_lib, _gendraw_lib, _predict_lib, _wgan_lib

native_libs.ensure_built(_cnormal_lib, _gendraw_lib, _predict_lib, _wgan_lib)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "probaforms_amd", "models", "gendraw_csrc", "pf_gendraw.h")
LDS_BYTES = 160 * 1024


def _header():
    with open(HEADER) as f:
        return f.read()


def test_exports_and_version_match_the_header_text():
    from probaforms_amd.models import _cnormal_lib, _gendraw_lib as gl, _predict_lib
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    declared = set(re.findall(r"\b(pfg_[a-z_]+)\s*\(", text))
    assert declared == set(gl.EXPORTS)
    for name, (_, args) in gl._SIGNATURES.items():
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, text)
        params = [p for p in m.group(1).split(",") if p.strip() and p.strip() != "void"]
        assert len(params) == len(args), name
    consts = dict(re.findall(r"#define\s+(PFG_[A-Z_]+)\s+\(?(-?\d+)\)?", _header()))
    assert int(consts["PFG_VERSION"]) == gl.ABI_VERSION
    assert int(consts["PFG_EUNSUPPORTED"]) == gl.EUNSUPPORTED == _predict_lib.EUNSUPPORTED
    assert int(consts["PFG_MAX_HIDDEN"]) == gl.MAX_HIDDEN
    assert int(consts["PFG_MAX_D"]) == gl.MAX_D == _cnormal_lib.MAX_D
    assert int(consts["PFG_WAVES"]) == gl.WAVES == 4
    # the two structs, field for field
    for struct, cls in (("pfg_mlp", gl.Mlp), ("pfg_plan_info", gl.PlanInfo)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), text, flags=re.S).group(1)
        names = [re.sub(r"\[.*\]", "", n.strip()) for decl in body.split(";") if decl.strip()
                 for n in decl.strip().split(None, 1)[1].split(",")]
        assert names == [f[0] for f in cls._fields_], struct


def test_library_reports_the_version_and_has_every_export():
    from probaforms_amd.models import _gendraw_lib as gl
    L = gl.lib()
    assert L.pfg_version() == gl.ABI_VERSION
    for name in gl.EXPORTS:
        assert hasattr(L, name)
    assert L.pfg_status_string(0) == b"ok"
    assert b"supported" in L.pfg_status_string(gl.EUNSUPPORTED)


# (d, c, latent, hidden, act)
CVAE_DEFAULT = (1, 1, 2, (10,), "tanh")
WGAN_DEFAULT = (1, 1, 1, (100, 100), "relu")
C5 = (16, 4, 2, (128,), "tanh")


def _packed_floats(d, c, latent, hidden):
    """the pack layout of pf_gendraw.hip: per Linear [out tiles of 16][groups of 4 k-steps of 4][64 lanes][4], the first
    Linear over the latent columns only, then the biases of every Linear but the first, each padded to 4 floats"""
    widths = [latent] + list(hidden) + [d]
    frag = sum(-(-o // 16) * -(-(-(-i // 4)) // 4) * 256 for i, o in zip(widths[:-1], widths[1:]))
    return frag + sum(-(-o // 4) * 4 for o in widths[2:])


@pytest.mark.parametrize("case", [CVAE_DEFAULT, WGAN_DEFAULT, C5])
def test_plan_keeps_the_weights_in_lds(case):
    from probaforms_amd.models import _gendraw_lib as gl
    net = gl.Mlp.make(*case)
    assert gl.supported(net)
    for K in (1, 19, 256, 1000):
        p = gl.plan(net, K)
        assert p.weights_in_lds == 1 and p.waves == 4 and p.draw_tiles in (1, 2, 4)
        assert p.draw_tiles <= (4 if K > 32 else 2 if K > 16 else 1)
        assert p.packed_bytes == 4 * _packed_floats(case[0], case[1], case[2], case[3])
        assert p.packed_bytes < p.lds_bytes <= LDS_BYTES
        assert gl.workspace_bytes(net, K) >= p.packed_bytes


def test_plan_draw_tiles_follow_the_draws():
    from probaforms_amd.models import _gendraw_lib as gl
    net = gl.Mlp.make(5, 3, 2, (10,), "tanh")
    assert [gl.plan(net, K).draw_tiles for K in (1, 16, 17, 19, 32, 33, 65)] == [1, 1, 2, 2, 2, 4, 4]


def test_plan_wide_net_reads_its_weights_from_the_workspace():
    from probaforms_amd.models import _gendraw_lib as gl
    net = gl.Mlp.make(3, 2, 2, (256, 256), "tanh")
    assert gl.supported(net)
    p = gl.plan(net, 19)
    assert p.weights_in_lds == 0 and p.draw_tiles == 1 and p.lds_bytes <= LDS_BYTES
    assert p.packed_bytes > LDS_BYTES and gl.workspace_bytes(net, 19) >= p.packed_bytes


def test_plan_refuses_what_does_not_fit():
    from probaforms_amd.models import _gendraw_lib as gl
    net = gl.Mlp.make(1, 1, 2, (4096,), "tanh")
    assert not gl.supported(net) and gl.workspace_bytes(net, 10) == 0
    with pytest.raises(gl.Unsupported):
        gl.plan(net, 10)
    info = gl.PlanInfo()
    import ctypes
    assert gl.lib().pfg_plan(ctypes.byref(net), 0, ctypes.byref(info)) == -1          # PFG_EINVAL: k_cnt < 1
    bad = gl.Mlp.make(1, 1, 2, (10,), "tanh")
    bad.latent = 0
    assert gl.workspace_bytes(bad, 10) == 0
    assert gl.lib().pfg_plan(ctypes.byref(bad), 10, ctypes.byref(info)) == -1


@pytest.mark.parametrize("n,width", [(32, 1), (8, 2), (37, 1), (5, 2), (3, 5), (1, 1)])
def test_noise_is_the_loops_stream(n, width):
    """stacked per window, the draws are those of K successive torch.normal / torch.randn calls, and the generator ends
    where the loop leaves it"""
    from probaforms_amd.models import _gendraw as G
    K = 7
    torch.manual_seed(5)
    want = torch.stack([torch.normal(0, 1, (n, width)) for _ in range(K)])
    end = torch.get_rng_state()
    torch.manual_seed(5)
    want2 = torch.stack([torch.randn(n, width) for _ in range(K)])
    assert torch.equal(want, want2)
    torch.manual_seed(5)
    got = torch.cat([G.noise(3, n, width), G.noise(4, n, width)])
    assert got.shape == (K, n, width) and torch.equal(got, want)
    assert torch.equal(torch.get_rng_state(), end)
    assert G.one_stream(n, width) == (n * width in (32, 16))


def _unsupported_cvae():
    from probaforms_amd import _hip
    from probaforms_amd.models import CVAE
    m = CVAE(latent_dim=2, hidden=(4096,))
    m._core = types.SimpleNamespace(shape=_hip.CvaeShape.make(3, 2, 2, (4096,), "tanh"), device=torch.device("cpu"))
    return m


def _unsupported_wgan():
    from probaforms_amd.models import ConditionalWGAN
    m = ConditionalWGAN(latent_dim=2, generator_hidden=(4096,))
    m._core = types.SimpleNamespace(d=3, c=2, latent=2, device=torch.device("cpu"))
    return m


def _unsupported_cnormal():
    """d = 33 is above PFG_MAX_D (the GPU ConditionalNormal itself stops at 32: only a stand-in core can carry it)"""
    from probaforms_amd.models import ConditionalNormal
    m = ConditionalNormal()
    core = types.SimpleNamespace(d=33, c=2, device=torch.device("cpu"))
    m.model = types.SimpleNamespace(core=lambda: core)
    return m


@pytest.mark.parametrize("make,d", [(_unsupported_cvae, 3), (_unsupported_wgan, 3), (_unsupported_cnormal, 33)])
def test_fallback_is_the_notebook_loop(make, d):
    """a net the kernel does not hold: sample_stats / sample_many are self.sample n_draws times plus numpy"""
    m = make()
    rng = np.random.default_rng(3)
    calls = []

    def fake_sample(C):
        calls.append(len(C))
        return rng.standard_normal((len(C), d)).astype(np.float32)

    m.sample = fake_sample
    C = np.zeros((4, 2), np.float32)
    s = m.sample_stats(C, 7, quantiles=(0.05, 0.95), ddof=1)
    assert calls == [4] * 7
    rng = np.random.default_rng(3)
    X = np.array([rng.standard_normal((4, d)).astype(np.float32) for _ in range(7)])
    np.testing.assert_array_equal(s.mean, X.astype(np.float64).mean(0).astype(np.float32))
    np.testing.assert_array_equal(s.std, X.astype(np.float64).std(0, ddof=1).astype(np.float32))
    np.testing.assert_array_equal(s.min, X.min(0))
    np.testing.assert_array_equal(s.max, X.max(0))
    np.testing.assert_array_equal(s.quantiles, np.quantile(X.astype(np.float64), [0.05, 0.95], axis=0).astype(np.float32))
    assert s.mean.dtype == np.float32 and s.quantiles.shape == (2, 4, d)
    assert m.sample_stats(C, 3).quantiles is None
    rng = np.random.default_rng(3)
    calls.clear()
    np.testing.assert_array_equal(m.sample_many(C, 7), X)
    assert calls == [4] * 7


BAD_CALLS = [dict(n_draws=0), dict(n_draws=-3), dict(n_draws=2.5), dict(n_draws=True), dict(n_draws=10, quantiles=(0.5, 1.01)),
             dict(n_draws=10, quantiles=(-0.01,)), dict(n_draws=10, quantiles=(float("nan"),)),
             dict(n_draws=8193, quantiles=(0.5,)), dict(n_draws=10, ddof=-1), dict(n_draws=10, ddof=0.5)]


@pytest.mark.parametrize("kw", BAD_CALLS)
def test_validation_errors_are_realnvps(kw):
    from probaforms_amd.models import CVAE, ConditionalNormal, ConditionalWGAN, RealNVP
    C = np.zeros((4, 2), np.float32)
    with pytest.raises(ValueError) as want:
        RealNVP().sample_stats(C, **kw)
    for cls in (CVAE, ConditionalWGAN, ConditionalNormal):
        with pytest.raises(ValueError) as got:
            cls().sample_stats(C, **kw)
        assert str(got.value) == str(want.value), cls.__name__
        if set(kw) == {"n_draws"}:
            with pytest.raises(ValueError) as got:
                cls().sample_many(C, **kw)
            assert str(got.value) == str(want.value), cls.__name__


def test_signatures_and_defaults_are_realnvps():
    import inspect
    from probaforms_amd.models import CVAE, ConditionalNormal, ConditionalWGAN, RealNVP
    for cls in (CVAE, ConditionalWGAN, ConditionalNormal):
        for name in ("sample_many", "sample_stats"):
            want, got = (inspect.signature(getattr(k, name)).parameters for k in (RealNVP, cls))
            assert list(got) == list(want), (cls.__name__, name)
            for p in want:
                if p != "C":                               # C defaults to what the model's own sample() defaults to
                    assert got[p].default == want[p].default, (cls.__name__, name, p)
            assert got["C"].default == inspect.signature(cls.sample).parameters["C"].default
