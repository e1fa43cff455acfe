"""probaforms_amd._cbind, no GPU: every binding module loads its library through the one Library, reports a missing, stale
or foreign build as its own ...LibraryMissing with nothing cached, and validates tensor arguments with the one ptr()."""
import ctypes as C
import importlib
import os
import subprocess
import sys

import pytest
import torch

import native_libs
from probaforms_amd import _cbind

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# binding module -> (symbol prefix, its LibraryMissing subclass)
BINDINGS = {
    "probaforms_amd._hip": ("rnvp_", "HipLibraryMissing"),
    "probaforms_amd.metrics._lib": ("pfm_", "MetricsLibraryMissing"),
    "probaforms_amd.models._wgan_lib": ("pfw_", "WganLibraryMissing"),
    "probaforms_amd.models._cnormal_lib": ("pfn_", "CnormalLibraryMissing"),
    "probaforms_amd.models._predict_lib": ("pfp_", "PredictLibraryMissing"),
    "probaforms_amd.models._gendraw_lib": ("pfg_", "GendrawLibraryMissing"),
}


@pytest.fixture(params=sorted(BINDINGS), ids=lambda n: n.rsplit(".", 1)[1].strip("_"))
def binding(request):
    """(module, prefix, missing class); the handle is dropped afterwards, so that no test sees what another one patched"""
    mod = importlib.import_module(request.param)
    native_libs.ensure_built(mod)
    prefix, missing = BINDINGS[request.param]
    yield mod, prefix, getattr(mod, missing)
    mod.LIBRARY.forget()


@pytest.fixture(scope="module")
def fresh_imports():
    """one fresh interpreter that sees no GPU imports the six modules; one line per module: name, LIBRARY.loaded, names bound"""
    code = ("import importlib, sys\n"
            "for n in sys.argv[1:]:\n"
            "    m = importlib.import_module(n)\n"
            "    print(n, m.LIBRARY.loaded, m.lib == m.LIBRARY.load and m.check == m.LIBRARY.check)\n")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, "-c", code] + sorted(BINDINGS), cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr
    return r.stdout.splitlines()


@pytest.mark.parametrize("name", sorted(BINDINGS), ids=lambda n: n.rsplit(".", 1)[1].strip("_"))
def test_import_without_a_gpu_loads_nothing(name, fresh_imports):
    assert "%s False True" % name in fresh_imports


def test_lib_is_loaded_once_and_reports_the_abi_version(binding):
    mod, prefix, missing = binding
    assert issubclass(missing, _cbind.LibraryMissing) and issubclass(missing, RuntimeError)
    assert mod.LIBRARY.missing is missing and mod.LIBRARY.prefix == prefix and mod.LIBRARY.path == mod.LIB_PATH
    assert mod.LIBRARY.signatures is mod._SIGNATURES and mod.EXPORTS == tuple(mod._SIGNATURES)
    L = mod.lib()
    assert mod.lib() is L and mod.LIBRARY.loaded is True
    assert getattr(L, prefix + "version")() == mod.ABI_VERSION == mod.LIBRARY.abi_version
    mod.check(0, "x")
    with pytest.raises(RuntimeError, match=r"^x failed: .* \(status -1\)$"):
        mod.check(-1, "x")


def _refused(mod, missing, match):
    mod.LIBRARY.forget()
    with pytest.raises(missing, match=match) as e:
        mod.lib()
    assert isinstance(e.value, _cbind.LibraryMissing)
    assert "make -C %s" % os.path.relpath(mod.LIBRARY.make_dir, ROOT) in str(e.value)
    assert mod.LIBRARY.loaded is False


def test_a_library_without_an_entry_point_is_missing(binding, monkeypatch):
    mod, prefix, missing = binding
    monkeypatch.setitem(mod._SIGNATURES, prefix + "not_there", (C.c_int, []))
    _refused(mod, missing, r"has no %snot_there: rebuild" % prefix)


def test_a_library_of_another_abi_version_is_missing(binding, monkeypatch):
    mod, prefix, missing = binding
    monkeypatch.setattr(mod.LIBRARY, "abi_version", mod.ABI_VERSION + 1)
    _refused(mod, missing, r"reports %sversion\(\) = %d, this binding is written for %d" % (prefix, mod.ABI_VERSION,
                                                                                          mod.ABI_VERSION + 1))


def test_a_library_that_is_not_there_is_missing(binding, monkeypatch, tmp_path):
    mod, prefix, missing = binding
    monkeypatch.setattr(mod.LIBRARY, "path", str(tmp_path / "libnot_built.so"))
    _refused(mod, missing, "libnot_built.so not found: build it")


def test_unsupported_is_an_exception_of_its_own_only_where_the_binding_registered_one(binding):
    mod, prefix, missing = binding
    if prefix in ("pfp_", "pfg_"):
        assert (mod.LIBRARY.unsupported_status, mod.LIBRARY.unsupported) == (mod.EUNSUPPORTED, mod.Unsupported) == (-2, mod.Unsupported)
        with pytest.raises(mod.Unsupported, match="^x: shape not supported$"):
            mod.check(-2, "x")
    else:
        assert mod.LIBRARY.unsupported is None
        with pytest.raises(RuntimeError, match=r"^x failed: .* \(status -2\)$") as e:
            mod.check(-2, "x")
        assert type(e.value) is RuntimeError


def test_ptr_refuses_what_is_not_a_contiguous_device_tensor_of_the_dtype():
    with pytest.raises(RuntimeError, match=r"^grad_out must be a tensor on a HIP device \(got cpu\)$"):
        _cbind.ptr(torch.zeros(3), torch.float32, "grad_out")
    with pytest.raises(RuntimeError, match=r"^grad_out must be a tensor on a HIP device \(got <class 'list'>\)$"):
        _cbind.f32([0.0], "grad_out")
    assert _cbind.ptr(None, torch.float32, "grad_out", nullable=True) is None
    assert _cbind.f32(None, "grad_out", True) is None
    with pytest.raises(RuntimeError, match="^grad_out is required$"):
        _cbind.ptr(None, torch.float32, "grad_out")
    with pytest.raises(RuntimeError, match="^grad_out is required$"):
        _cbind.f32(None, "grad_out")


def test_hip_ptr_keeps_its_suffix_and_takes_none_anywhere():
    from probaforms_amd import _hip
    assert _hip._ptr(None, torch.float32, "c") is None
    with pytest.raises(RuntimeError, match=r"^x must be a tensor on a HIP device \(got cpu\); probaforms_amd has no CPU path$"):
        _hip._ptr(torch.zeros(3), torch.float32, "x")
