"""ConditionalNormal host side, no GPU: the committed fixtures, the float32 / float64 restatement against them, the ctypes
mirror of pf_cnormal.h, the refusal of unsupported shapes, the import path and the module layout."""
import ctypes
import glob
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
HEADER = os.path.join(ROOT, "probaforms_amd", "models", "cnormal_csrc", "pf_cnormal.h")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import cnormal_torch as ct  # noqa: E402
import native_libs  # noqa: E402
from probaforms_amd.models import ConditionalNormal, Net  # noqa: E402
from probaforms_amd.models import _cnormal_lib as N  # noqa: E402

native_libs.ensure_built(N)

NAMES = ["d1", "default", "indep", "nocond", "sigmoid_deep"]


def load(name):
    f = np.load(os.path.join(GOLDEN, "cnormal_%s.npz" % name))
    kw = {k[3:]: f[k] for k in f.files if k.startswith("kw_")}
    kw = {k: (tuple(int(x) for x in v) if v.ndim else (str(v) if v.dtype.kind == 'U' else v.item())) for k, v in kw.items()}
    C = f["C"] if f["C"].shape[1] else None
    return f, kw, f["X"], C


def restatement(kw, X, C):
    c = 1 if C is None else C.shape[1]
    return ct.Normal(X.shape[1], c, kw.get("hidden", (10,)), kw.get("activation", "tanh"),
                     kw.get("use_independent_covariance", False))


def cond_of(X, C):
    return np.zeros((X.shape[0], 1), np.float32) if C is None else C


def fixture_batches(f):
    off = np.concatenate([[0], np.cumsum(f["batch_sizes"])])
    return [f["rows"][off[k]:off[k + 1]] for k in range(int(f["K"]))]


def test_fixtures_exist_and_are_small():
    names = sorted(os.path.basename(p)[8:-4] for p in glob.glob(os.path.join(GOLDEN, "cnormal_*.npz")))
    assert names == NAMES
    for n in names:
        assert os.path.getsize(os.path.join(GOLDEN, "cnormal_%s.npz" % n)) < 200 * 1024, n
        f, kw, X, C = load(n)
        K = int(f["K"])
        B, E = kw.get("batch_size", 32), kw.get("n_epochs", 10)
        assert f["batch_sizes"].sum() == f["rows"].size and all(("grad_%d" % k) in f.files for k in range(K))
        assert f["loss_history"].size == E * -(-X.shape[0] // B) and f["p0"].shape == f["pK"].shape == f["p_end"].shape
    assert load("default")[0]["batch_sizes"][3] == 4 and load("sigmoid_deep")[0]["batch_sizes"][4] == 6
    assert load("d1")[0]["batch_sizes"][0] == 33 and int(load("nocond")[0]["sample_arg"]) == 7


@pytest.mark.parametrize("name", NAMES)
def test_restatement_reproduces_the_reference(name):
    """float32: the reference's recorded gradients to a few ulp of the largest one, losses and final parameters; float64:
    the same within float32's own error.  Observed (float32 mode): the gradients of four fixtures bit for bit, d1's within
    1.1e-7 of max |g| (1 ulp); the bounds asserted are 4 ulp."""
    f, kw, X, C = load(name)
    net = restatement(kw, X, C)
    Cz = cond_of(X, C)
    assert net.P == f["p0"].size
    n, B, E = X.shape[0], kw.get("batch_size", 32), kw.get("n_epochs", 10)
    K = int(f["K"])
    batches = fixture_batches(f)
    seen = {}

    def hook(k, loss, g, p):
        if k < K:
            seen[k] = (loss, g)
        if k == K:
            seen["pK"] = p
    # every batch of the fit: the K recorded ones, then the rest replayed from the fit's seed
    torch.manual_seed(int(f["seed"]))
    Net(X.shape[1], Cz.shape[1], kw.get("hidden", (10,)), kw.get("activation", "tanh"))     # the init's RNG consumption
    epochs, _ = ct.replay_draws(torch.get_rng_state(), n, B, X.shape[1], E)
    allb = [b for e in epochs for b in e]
    assert all(np.array_equal(a, b) for a, b in zip(allb, batches))
    p32, l32 = ct.fit(net, f["p0"], X, Cz, allb, kw.get("lr", 1e-4), kw.get("weight_decay", 0), torch.float32, hook)
    worst = 0.0
    for k in range(K):
        ref = f["grad_%d" % k]
        err = np.abs(seen[k][1] - ref).max() / np.abs(ref).max()
        worst = max(worst, err)
        assert err <= 4 * np.finfo(np.float32).eps, (name, k, err)
    print(name, "float32 restatement: worst gradient error %.3g of max |g|" % worst)
    scale = np.abs(f["p_end"]).max()
    np.testing.assert_allclose(l32, f["loss_history"], rtol=4e-7, atol=4e-7)
    assert np.abs(seen["pK"] - f["pK"]).max() <= 4 * np.finfo(np.float32).eps * scale
    assert np.abs(p32 - f["p_end"]).max() <= 4 * np.finfo(np.float32).eps * scale, np.abs(p32 - f["p_end"]).max()
    # float64 on the same batches: within float32's own error of the reference
    p64, l64 = ct.fit(net, f["p0"], X, Cz, allb, kw.get("lr", 1e-4), kw.get("weight_decay", 0), torch.float64)
    assert np.abs(p64 - f["p_end"]).max() < 0.05 * np.abs(f["p_end"] - f["p0"]).max()
    np.testing.assert_allclose(l64, f["loss_history"], rtol=2e-5, atol=2e-5)
    if net.independent:
        assert np.array_equal(p32[net.P_main:], f["p0"][net.P_main:]) and np.array_equal(f["p_end"][net.P_main:], f["p0"][net.P_main:])
    # Net.forward
    xt, inv, mu, sigma = net.forward(f["p_end"], Cz, f["fwd_eps"], X, torch.float32)
    for got, key in ((xt, "fwd_xt"), (inv, "fwd_inv"), (mu, "fwd_mu"), (sigma, "fwd_sigma")):
        np.testing.assert_allclose(got, f[key], rtol=1e-5, atol=1e-5 * np.abs(f[key]).max())


def test_out_gradient_formulas_match_autograd():
    """dL/dW = -M^T sum_r G_r inv_r^T and dL/db = -M^T sum_r G_r with G_r = (inv_r - mu_r) / (sigma_r^2 R d), M = W^-1:
    what the kernels compute, against autograd in float64"""
    rng = np.random.default_rng(0)
    d, c, R = 4, 2, 9
    net = ct.Normal(d, c, (6,), 'tanh', False)
    p = rng.normal(size=net.P) * 0.5
    p[net.P_main:net.P_main + d * d] += np.eye(d).reshape(-1)
    X, C = rng.normal(size=(R, d)), rng.normal(size=(R, c))
    _, g = net.loss_grad(p, X, C)
    _, inv, mu, sigma = net.forward(p, C, None, X)
    M = np.linalg.inv(p[net.P_main:net.P_main + d * d].reshape(d, d))
    G = (inv - mu) / (sigma ** 2 * R * d)
    np.testing.assert_allclose(g[net.P_main:net.P_main + d * d].reshape(d, d), -M.T @ (G.T @ inv), rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(g[net.P_main + d * d:], -M.T @ G.sum(0), rtol=1e-10, atol=1e-12)


def test_shape_struct_matches_the_c_header():
    S, O = N.Shape, N.Adam
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "pf_cnormal.h"\n'
           'int main(void){printf("%zu %zu %zu %zu %zu %zu %zu %d %d %d %d %d %d %d",'
           'sizeof(pfn_shape), offsetof(pfn_shape, n_hidden), offsetof(pfn_shape, hidden), offsetof(pfn_shape, act),'
           'offsetof(pfn_shape, independent), sizeof(pfn_adam), offsetof(pfn_adam, weight_decay),'
           'PFN_VERSION, PFN_MAX_HIDDEN, PFN_MAX_D, PFN_ACT_TANH, PFN_ACT_RELU, PFN_ACT_SIGMOID, PFN_EUNSUPPORTED);return 0;}\n')
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "s.c"); exe = os.path.join(td, "s")
        open(c, "w").write(src)
        subprocess.check_call(["gcc", "-std=c99", "-I", os.path.dirname(HEADER), c, "-o", exe])
        v = list(map(int, subprocess.check_output([exe]).split()))
    assert v[:7] == [ctypes.sizeof(S), S.n_hidden.offset, S.hidden.offset, S.act.offset, S.independent.offset,
                     ctypes.sizeof(O), O.weight_decay.offset]
    assert v[7:] == [N.ABI_VERSION, N.MAX_HIDDEN, N.MAX_D, N.ACT_TANH, N.ACT_RELU, N.ACT_SIGMOID, N.EUNSUPPORTED]


def test_tiling_struct_matches_the_c_header():
    T = N.TilingInfo
    names = [n for n, _ in T._fields_]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "pf_cnormal.h"\n'
           'int main(void){printf("%zu", sizeof(pfn_tiling_info));\n' +
           "".join('printf(" %%zu %%zu", offsetof(pfn_tiling_info, %s), sizeof(((pfn_tiling_info *)0)->%s));\n' % (n, n)
                   for n in names) + 'return 0;}\n')
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "s.c"); exe = os.path.join(td, "s")
        open(c, "w").write(src)
        subprocess.check_call(["gcc", "-std=c99", "-I", os.path.dirname(HEADER), c, "-o", exe])
        v = list(map(int, subprocess.check_output([exe]).split()))
    assert v[0] == ctypes.sizeof(T)
    assert v[1:] == [x for n in names for x in (getattr(T, n).offset, getattr(T, n).size)]
    declared = re.search(r"typedef struct pfn_tiling_info \{(.*?)\} pfn_tiling_info;", open(HEADER).read(), flags=re.S).group(1)
    declared = re.sub(r"/\*.*?\*/", "", declared, flags=re.S)
    assert re.findall(r"int(?:32|64)_t\s+(\w+);", declared) == names            # every field, in order


def test_header_declarations_equal_the_binding_exports():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = re.findall(r"\b(pfn_[a-z_]+)\s*\(", text)
    assert sorted(set(declared)) == sorted(N.EXPORTS) and len(declared) == len(N.EXPORTS)


def test_parameter_counts_match_the_modules():
    for d, c, hidden in ((5, 3, (10,)), (12, 4, (16, 12)), (N.MAX_D, 2, (4,) * 8)):
        s = N.Shape.make(d, c, hidden, 'sigmoid', False)
        assert N.param_count(s) == sum(p.numel() for p in Net(d, c, hidden, 'sigmoid').parameters())
        assert N.param_count(s) == ct.Normal(d, c, hidden).P
        assert N.workspace_bytes(s, 32) > 0
    assert (N.Shape.make(2, 2, (3,), 'tanh', True).act, N.Shape.make(2, 2, (3,), 'elu', True).act,
            N.Shape.make(2, 2, (3,), 'sigmoid', True).act) == (N.ACT_TANH, N.ACT_RELU, N.ACT_SIGMOID)


def test_unsupported_shapes_are_refused_before_anything_is_read():
    fake = ctypes.c_void_p(256)                    # never dereferenced: the calls return before
    L = N.lib()
    for s in (N.Shape.make(N.MAX_D + 1, 3, (10,), 'tanh', False),          # the d x d system no longer fits one workgroup
              N.Shape.make(5, 3, (50000,), 'tanh', False)):                # one row does not fit LDS
        by = ctypes.byref(s)
        assert N.workspace_bytes(s, 32) == 0
        assert L.pfn_forward(None, by, fake, fake, fake, fake, 4, fake, fake, fake, fake, fake) == N.EUNSUPPORTED
        assert L.pfn_loss_grad(None, by, fake, fake, fake, None, 4, fake, fake, fake, fake, 1 << 30) == N.EUNSUPPORTED
        opt = N.adam(1e-3)
        assert L.pfn_train_step(None, by, fake, fake, fake, fake, fake, None, 4, ctypes.byref(opt), 1, fake, fake, fake, fake,
                                1 << 30) == N.EUNSUPPORTED
        assert L.pfn_fit_epoch(None, by, fake, fake, fake, fake, fake, fake, 8, 4, ctypes.byref(opt), 1, fake, fake, fake,
                               1 << 30) == N.EUNSUPPORTED
    assert b"unsupported" in L.pfn_status_string(N.EUNSUPPORTED)


def test_modules_keep_the_reference_layout():
    net = Net(5, 3, (10, 20), 'sigmoid')
    assert list(net.state_dict()) == ["model.0.weight", "model.0.bias", "model.2.weight", "model.2.bias", "mu.weight", "mu.bias",
                                      "log_sigma.weight", "log_sigma.bias", "out.weight", "out.bias"]
    assert isinstance(net.model[1], torch.nn.Sigmoid) and isinstance(Net(2, 2, (3,), 'elu').model[1], torch.nn.ReLU)
    assert isinstance(Net(2, 2).model[1], torch.nn.Tanh) and isinstance(Net(2, 2, (3,), 'relu').model[1], torch.nn.ReLU)
    assert Net(4, 2, independent_covariance=True).out.weight.shape == (4, 4)        # out always exists
    m = ConditionalNormal()
    assert (m.independent_covariance, m.hidden, m.activation, m.batch_size, m.n_epochs, m.lr, m.weight_decay, m.verbose,
            m.opt) == (False, (10,), 'tanh', 32, 10, 0.0001, 0, 0, None)
    assert ConditionalNormal(use_independent_covariance=True).independent_covariance is True


def _run(code):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    return subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)


def test_import_needs_no_gpu():
    r = _run("import torch\nfrom probaforms_amd.models.cnormal import ConditionalNormal, Net\nassert not torch.cuda.is_available()\n"
             "m = ConditionalNormal(n_epochs=2)\nprint('ok', m.batch_size, len(list(Net(3, 2).parameters())))")
    assert r.returncode == 0 and r.stdout.strip() == "ok 32 8", r.stderr


def test_install_as_probaforms_serves_cnormal():
    r = _run("import sys, probaforms_amd\nprobaforms_amd.install_as_probaforms()\n"
             "from probaforms.models import ConditionalNormal, ConditionalWGAN, CVAE, RealNVP\nimport probaforms.models.cnormal as n\n"
             "from probaforms import metrics\n"
             "assert n.ConditionalNormal is ConditionalNormal and sys.modules['probaforms.models.cnormal'] is n\n"
             "assert sorted(metrics.__all__) == ['frechet_distance', 'maximum_mean_discrepancy']\nprint('ok')")
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr
