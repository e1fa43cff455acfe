"""ctypes binding of libpf_cnormal.so (C ABI: probaforms_amd/models/cnormal_csrc/pf_cnormal.h).

The library is built in-tree by `make -C probaforms_amd/models/cnormal_csrc` (see __graft_entry__.build) and loaded on the
first call, so importing probaforms_amd.models.cnormal needs no GPU.  There is NO fallback: a missing library, a shape the
kernels do not support or a tensor off the HIP device raises.
"""
import ctypes as C
import os

import torch

from .._cbind import Library, LibraryMissing, f32 as _f32, ptr as _ptr, stream as _stream

ABI_VERSION = 101          # pfn_version() of the library this binding matches (pf_cnormal.h PFN_VERSION)
MAX_HIDDEN = 8             # PFN_MAX_HIDDEN
MAX_D = 32                 # PFN_MAX_D
ACT_TANH, ACT_RELU, ACT_SIGMOID = 0, 1, 2  # PFN_ACT_*
EUNSUPPORTED = -2

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "cnormal_csrc", "libpf_cnormal.so")
_ACTS = {'tanh': ACT_TANH, 'relu': ACT_RELU, 'sigmoid': ACT_SIGMOID}


class Shape(C.Structure):
    """pfn_shape"""
    _fields_ = [("d", C.c_int32), ("c", C.c_int32), ("n_hidden", C.c_int32), ("hidden", C.c_int32 * MAX_HIDDEN),
                ("act", C.c_int32), ("independent", C.c_int32)]

    @classmethod
    def make(cls, d, c, hidden, activation, independent):
        hidden = [int(h) for h in hidden]
        if not 1 <= len(hidden) <= MAX_HIDDEN:
            raise ValueError("ConditionalNormal on the GPU supports 1..%d hidden layers (got %d)" % (MAX_HIDDEN, len(hidden)))
        s = cls()
        s.d, s.c, s.n_hidden = int(d), int(c), len(hidden)
        for i, h in enumerate(hidden):
            s.hidden[i] = h
        s.act = _ACTS.get(activation, ACT_RELU)            # cnormal.py:39-46: anything else is ReLU
        s.independent = 1 if independent else 0
        return s


class Adam(C.Structure):
    """pfn_adam"""
    _fields_ = [("lr", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double),
                ("weight_decay", C.c_double)]


class TilingInfo(C.Structure):
    """pfn_tiling_info"""
    _fields_ = [("step_tile", C.c_int32), ("step_cap", C.c_int32), ("fwd_tile", C.c_int32), ("reserved", C.c_int32),
                ("step_wgs", C.c_int64), ("step_wg_bound", C.c_int64), ("step_lds_bytes", C.c_int64),
                ("fwd_lds_bytes", C.c_int64)]


_VP, _I64, _SZ, _SP, _OP = C.c_void_p, C.c_int64, C.c_size_t, C.POINTER(Shape), C.POINTER(Adam)

_SIGNATURES = {
    "pfn_version": (C.c_int, []),
    "pfn_status_string": (C.c_char_p, [C.c_int]),
    "pfn_param_count": (_I64, [_SP]),
    "pfn_workspace_bytes": (_SZ, [_SP, _I64]),
    "pfn_tiling": (C.c_int, [_SP, _I64, C.POINTER(TilingInfo)]),
    "pfn_forward": (C.c_int, [_VP, _SP, _VP, _VP, _VP, _VP, _I64, _VP, _VP, _VP, _VP, _VP]),
    "pfn_loss_grad": (C.c_int, [_VP, _SP, _VP, _VP, _VP, _VP, _I64, _VP, _VP, _VP, _VP, _SZ]),
    "pfn_train_step": (C.c_int, [_VP, _SP, _VP, _VP, _VP, _VP, _VP, _VP, _I64, _OP, _I64, _VP, _VP, _VP, _VP, _SZ]),
    "pfn_fit_epoch": (C.c_int, [_VP, _SP, _VP, _VP, _VP, _VP, _VP, _VP, _I64, _I64, _OP, _I64, _VP, _VP, _VP, _SZ]),
}
EXPORTS = tuple(_SIGNATURES)


class CnormalLibraryMissing(LibraryMissing):
    pass


LIBRARY = Library(LIB_PATH, os.path.dirname(LIB_PATH), "pfn_", ABI_VERSION, _SIGNATURES, CnormalLibraryMissing,
                  "ConditionalNormal has no CPU fallback.")
lib = LIBRARY.load
check = LIBRARY.check


def param_count(shape):
    n = int(lib().pfn_param_count(C.byref(shape)))
    if n < 0:
        raise ValueError("invalid ConditionalNormal shape")
    return n


def workspace_bytes(shape, batch_rows):
    return int(lib().pfn_workspace_bytes(C.byref(shape), int(batch_rows)))


def tiling(shape, rows, require_step=True):
    """pfn_tiling_info of a training step / a forward call on `rows` rows (host only: no GPU needed).  A shape whose step
    cannot run raises, as every other call does, unless require_step is False: the step fields are then 0"""
    info = TilingInfo()
    st = lib().pfn_tiling(C.byref(shape), int(rows), C.byref(info))
    if st != EUNSUPPORTED or require_step:
        check(st, "pfn_tiling")
    return info


def adam(lr, weight_decay=0.0, betas=(0.9, 0.999), eps=1e-8):
    return Adam(float(lr), float(betas[0]), float(betas[1]), float(eps), float(weight_decay))


def forward(shape, params, c, eps, x, n, mu, sigma, x_tilde, inv, status):
    """Net.forward on the current stream (inference only: no autograd); every output is nullable"""
    check(lib().pfn_forward(_stream(), C.byref(shape), _f32(params, "params"), _f32(c, "C"), _f32(eps, "eps", True),
                            _f32(x, "X", True), int(n), _f32(mu, "mu", True), _f32(sigma, "sigma", True),
                            _f32(x_tilde, "x_tilde", True), _f32(inv, "inv", True),
                            _ptr(status, torch.int32, "status", True)), "pfn_forward")


def loss_grad(shape, params, x, c, row_index, rows, grad_out, loss_out, status, ws):
    check(lib().pfn_loss_grad(_stream(), C.byref(shape), _f32(params, "params"), _f32(x, "X"), _f32(c, "C"),
                              _ptr(row_index, torch.int64, "row_index", True), int(rows), _f32(grad_out, "grad_out", True),
                              _f32(loss_out, "loss_out", True), _ptr(status, torch.int32, "status", True),
                              _ptr(ws, torch.uint8, "workspace"), ws.numel()), "pfn_loss_grad")


def train_step(shape, params, exp_avg, exp_avg_sq, x, c, row_index, rows, opt, step, grad_out, loss_out, status, ws):
    check(lib().pfn_train_step(_stream(), C.byref(shape), _f32(params, "params"), _f32(exp_avg, "exp_avg"),
                               _f32(exp_avg_sq, "exp_avg_sq"), _f32(x, "X"), _f32(c, "C"),
                               _ptr(row_index, torch.int64, "row_index", True), int(rows), C.byref(opt), int(step),
                               _f32(grad_out, "grad_out", True), _f32(loss_out, "loss_out", True),
                               _ptr(status, torch.int32, "status", True), _ptr(ws, torch.uint8, "workspace"), ws.numel()),
          "pfn_train_step")


def fit_epoch(shape, params, exp_avg, exp_avg_sq, x, c, perm, n, batch_size, opt, first_step, losses, status, ws):
    check(lib().pfn_fit_epoch(_stream(), C.byref(shape), _f32(params, "params"), _f32(exp_avg, "exp_avg"),
                              _f32(exp_avg_sq, "exp_avg_sq"), _f32(x, "X"), _f32(c, "C"), _ptr(perm, torch.int64, "perm"),
                              int(n), int(batch_size), C.byref(opt), int(first_step), _f32(losses, "losses"),
                              _ptr(status, torch.int32, "status", True), _ptr(ws, torch.uint8, "workspace"), ws.numel()),
          "pfn_fit_epoch")
