"""ConditionalWGAN host side, no GPU: the committed fixtures, the noise stream, the step-kind schedule, the ctypes mirror of
pf_wgan.h, the import path and the module layout."""
import ctypes
import glob
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
HEADER = os.path.join(ROOT, "probaforms_amd", "models", "wgan_csrc", "pf_wgan.h")
sys.path.insert(0, ROOT)

import native_libs  # noqa: E402
from probaforms_amd.models import _wgan_lib  # noqa: E402

native_libs.ensure_built(_wgan_lib)


def test_fixtures_exist_and_are_small():
    names = sorted(os.path.basename(p) for p in glob.glob(os.path.join(GOLDEN, "wgan_*.npz")))
    assert names == ["wgan_default.npz", "wgan_nocond.npz", "wgan_tanh_wd.npz"]
    for n in names:
        p = os.path.join(GOLDEN, n)
        assert os.path.getsize(p) < 512 * 1024, n
        f = np.load(p)
        K = int(f["K"])
        assert 6 <= K <= 12 and f["kinds"].size == K and f["batch_sizes"].sum() == f["rows"].size == f["z"].shape[0]
        assert all(("grad_%d" % k) in f.files for k in range(K)) and f["p0"].shape == f["pK"].shape
    f = np.load(os.path.join(GOLDEN, "wgan_tanh_wd.npz"))
    assert int(f["kw_n_critic"]) == 3 and float(f["kw_weight_decay"]) > 0 and int(f["kw_latent_dim"]) == 3
    assert f["batch_sizes"][3] == 2                 # the ragged last batch


def test_normal_and_randn_give_the_same_bits():
    """wgan.py draws torch.normal(0, 1, size); the CVAE's _FitDraws replays torch.randn(size)"""
    for shape in ((32, 1), (4, 1), (100, 3), (7, 2), (1, 1)):
        g1, g2 = torch.Generator(), torch.Generator()
        g1.manual_seed(5); g2.manual_seed(5)
        a = torch.normal(0, 1, shape, generator=g1)
        b = torch.randn(*shape, generator=g2)
        assert torch.equal(a, b)
        assert torch.equal(g1.get_state(), g2.get_state())


def test_step_kind_schedule_is_python_modulo():
    from probaforms_amd.models.wgan import step_kinds
    from probaforms_amd.models import _wgan_lib as W
    for n_critic in (5, 3, 2, 1, 2.5, 0.7):
        for start in (0, 3, 17):
            k = step_kinds(start, 9, n_critic)
            want = [W.STEP_CRITIC if (start + b) % n_critic != 0 else W.STEP_GEN for b in range(9)]
            assert k.dtype == np.int8 and k.tolist() == want
    assert step_kinds(0, 6, 5).tolist() == [0, 1, 1, 1, 1, 0]
    assert step_kinds(0, 4, 1).tolist() == [0, 0, 0, 0]
    assert step_kinds(0, 6, 2.5).tolist() == [0, 1, 1, 1, 1, 0]      # 0 and 5 are the multiples of 2.5


def test_shape_struct_matches_the_c_header():
    from probaforms_amd.models import _wgan_lib as W
    S, O = W.Shape, W.RMSprop
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "pf_wgan.h"\n'
           'int main(void){printf("%zu %zu %zu %zu %zu %zu %zu %zu %d %d %d %d %d %d %d %d %d",'
           'sizeof(pfw_shape), offsetof(pfw_shape, g_hidden), offsetof(pfw_shape, g_act), offsetof(pfw_shape, d_n_hidden),'
           'offsetof(pfw_shape, d_hidden), offsetof(pfw_shape, d_act), sizeof(pfw_rmsprop), offsetof(pfw_rmsprop, clamp),'
           'PFW_VERSION, PFW_MAX_HIDDEN, PFW_ACT_TANH, PFW_ACT_RELU, PFW_NET_G, PFW_NET_D, PFW_STEP_GEN, PFW_STEP_CRITIC,'
           'PFW_EUNSUPPORTED);return 0;}\n')
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "s.c"); exe = os.path.join(td, "s")
        open(c, "w").write(src)
        subprocess.check_call(["gcc", "-std=c99", "-I", os.path.dirname(HEADER), c, "-o", exe])
        v = list(map(int, subprocess.check_output([exe]).split()))
    assert v[:8] == [ctypes.sizeof(S), S.g_hidden.offset, S.g_act.offset, S.d_n_hidden.offset, S.d_hidden.offset,
                     S.d_act.offset, ctypes.sizeof(O), O.clamp.offset]
    assert v[8:] == [W.ABI_VERSION, W.MAX_HIDDEN, W.ACT_TANH, W.ACT_RELU, W.NET_G, W.NET_D, W.STEP_GEN, W.STEP_CRITIC,
                     W.EUNSUPPORTED]


def test_tiling_struct_matches_the_c_header():
    from probaforms_amd.models import _wgan_lib as W
    T = W.TilingInfo
    names = [n for n, _ in T._fields_]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "pf_wgan.h"\n'
           'int main(void){printf("%zu", sizeof(pfw_tiling_info));\n' +
           "".join('printf(" %%zu %%zu", offsetof(pfw_tiling_info, %s), sizeof(((pfw_tiling_info *)0)->%s));\n' % (n, n)
                   for n in names) + 'return 0;}\n')
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "s.c"); exe = os.path.join(td, "s")
        open(c, "w").write(src)
        subprocess.check_call(["gcc", "-std=c99", "-I", os.path.dirname(HEADER), c, "-o", exe])
        v = list(map(int, subprocess.check_output([exe]).split()))
    assert v[0] == ctypes.sizeof(T)
    assert v[1:] == [x for n in names for x in (getattr(T, n).offset, getattr(T, n).size)]
    declared = re.search(r"typedef struct pfw_tiling_info \{(.*?)\} pfw_tiling_info;", open(HEADER).read(), flags=re.S).group(1)
    declared = re.sub(r"/\*.*?\*/", "", declared, flags=re.S)
    assert re.findall(r"int(?:32|64)_t\s+(\w+);", declared) == names            # every field, in order


def test_header_declarations_equal_the_binding_exports():
    from probaforms_amd.models import _wgan_lib as W
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = re.findall(r"\b(pfw_[a-z_]+)\s*\(", text)
    assert sorted(set(declared)) == sorted(W.EXPORTS) and len(declared) == len(W.EXPORTS)


def test_parameter_counts_match_the_modules():
    from probaforms_amd.models import Discriminator, Generator
    from probaforms_amd.models import _wgan_lib as W
    for d, c, lat, gh, dh in ((5, 3, 1, (100, 100), (100, 100)), (3, 0, 3, (16, 12), (20, 8)), (7, 2, 2, (4,) * 8, (9,))):
        s = W.Shape.make(d, c, lat, gh, dh, 'relu', 'tanh')
        G, D = Generator(lat + c, d, gh, 'relu'), Discriminator(d + c, dh, 'tanh')
        assert W.param_count(s, W.NET_G) == sum(p.numel() for p in G.parameters())
        assert W.param_count(s, W.NET_D) == sum(p.numel() for p in D.parameters())
        assert W.workspace_bytes(s, 32, 100) > 0
    wide = W.Shape.make(5, 3, 1, (20000,), (10,), 'relu', 'relu')        # one row does not fit LDS: refused, no fallback
    fake = ctypes.c_void_p(256)                                          # never dereferenced: the call returns before
    st = W.lib().pfw_loss_grad(None, ctypes.byref(wide), W.STEP_CRITIC, fake, fake, fake, None, fake, 4, None, None, fake, 1 << 30)
    assert st == W.EUNSUPPORTED


def test_modules_keep_the_reference_layout():
    from probaforms_amd.models import ConditionalWGAN, Discriminator, Generator
    G = Generator(4, 5, (100, 100), 'relu')
    assert list(G.state_dict()) == ["model.%d.%s" % (k, w) for k in (0, 2, 4) for w in ("weight", "bias")]
    assert isinstance(G.model[1], torch.nn.ReLU) and isinstance(Generator(2, 2, (3,), 'elu').model[1], torch.nn.ReLU)
    assert isinstance(Discriminator(3, (4,), 'tanh').model[1], torch.nn.Tanh)
    assert Discriminator(8, (100, 100)).model[4].out_features == 1
    m = ConditionalWGAN()
    assert (m.latent_dim, m.generator_hidden, m.discriminator_hidden, m.generator_activation, m.discriminator_activation,
            m.batch_size, m.n_epochs, m.lr, m.weight_decay, m.n_critic, m.verbose) == (
        1, (100, 100), (100, 100), 'relu', 'relu', 32, 1000, 0.00005, 0, 5, 0)
    assert m.generator is None and m.discriminator is None and m.opt_gen is None and m.opt_disc is None


def _run(code):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    return subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)


def test_import_needs_no_gpu():
    r = _run("import torch\nfrom probaforms_amd.models.wgan import ConditionalWGAN\nassert not torch.cuda.is_available()\n"
             "m = ConditionalWGAN(n_epochs=2)\nprint('ok', m.n_critic)")
    assert r.returncode == 0 and r.stdout.strip() == "ok 5", r.stderr


def test_install_as_probaforms_serves_the_wgan():
    r = _run("import sys, probaforms_amd\nprobaforms_amd.install_as_probaforms()\n"
             "from probaforms.models import ConditionalWGAN, Generator, Discriminator\nimport probaforms.models.wgan as w\n"
             "from probaforms import metrics\n"
             "assert w.ConditionalWGAN is ConditionalWGAN and sys.modules['probaforms.models.wgan'] is w\n"
             "assert sorted(metrics.__all__) == ['frechet_distance', 'maximum_mean_discrepancy']\nprint('ok')")
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr
