"""ctypes binding of libpf_wgan.so (C ABI: probaforms_amd/models/wgan_csrc/pf_wgan.h).

The library is built in-tree by `make -C probaforms_amd/models/wgan_csrc` (see __graft_entry__.build) and loaded on the
first call, so importing probaforms_amd.models.wgan needs no GPU.  There is NO fallback: a missing library, a shape the
kernels do not support or a tensor off the HIP device raises.
"""
import ctypes as C
import os

import torch

from .._cbind import Library, LibraryMissing, f32 as _f32, ptr as _ptr, stream as _stream

ABI_VERSION = 101          # pfw_version() of the library this binding matches (pf_wgan.h PFW_VERSION)
MAX_HIDDEN = 8             # PFW_MAX_HIDDEN
ACT_TANH, ACT_RELU = 0, 1  # PFW_ACT_*
NET_G, NET_D = 0, 1        # PFW_NET_*
STEP_GEN, STEP_CRITIC = 0, 1   # PFW_STEP_*
EUNSUPPORTED = -2

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "wgan_csrc", "libpf_wgan.so")


class Shape(C.Structure):
    """pfw_shape"""
    _fields_ = [("d", C.c_int32), ("c", C.c_int32), ("latent", C.c_int32),
                ("g_n_hidden", C.c_int32), ("g_hidden", C.c_int32 * MAX_HIDDEN), ("g_act", C.c_int32),
                ("d_n_hidden", C.c_int32), ("d_hidden", C.c_int32 * MAX_HIDDEN), ("d_act", C.c_int32)]

    @classmethod
    def make(cls, d, c, latent, g_hidden, d_hidden, g_act, d_act):
        g_hidden, d_hidden = [int(h) for h in g_hidden], [int(h) for h in d_hidden]
        for h in (g_hidden, d_hidden):
            if not 1 <= len(h) <= MAX_HIDDEN:
                raise ValueError("ConditionalWGAN on the GPU supports 1..%d hidden layers per net (got %d)" % (MAX_HIDDEN, len(h)))
        s = cls()
        s.d, s.c, s.latent = int(d), int(c), int(latent)
        s.g_n_hidden, s.d_n_hidden = len(g_hidden), len(d_hidden)
        for i, h in enumerate(g_hidden):
            s.g_hidden[i] = h
        for i, h in enumerate(d_hidden):
            s.d_hidden[i] = h
        s.g_act = ACT_TANH if g_act == 'tanh' else ACT_RELU          # wgan.py:26-32: anything else is ReLU
        s.d_act = ACT_TANH if d_act == 'tanh' else ACT_RELU
        return s


class RMSprop(C.Structure):
    """pfw_rmsprop"""
    _fields_ = [("lr", C.c_double), ("alpha", C.c_double), ("eps", C.c_double), ("weight_decay", C.c_double),
                ("clamp", C.c_double)]


class TilingInfo(C.Structure):
    """pfw_tiling_info"""
    _fields_ = [("step_tile", C.c_int32), ("step_cap", C.c_int32), ("eloss_tile", C.c_int32), ("gen_tile", C.c_int32),
                ("crit_tile", C.c_int32), ("reserved", C.c_int32), ("step_wgs", C.c_int64), ("step_wg_bound", C.c_int64),
                ("step_lds_bytes", C.c_int64), ("eloss_lds_bytes", C.c_int64), ("gen_lds_bytes", C.c_int64),
                ("crit_lds_bytes", C.c_int64)]


_VP, _I64, _SZ, _SP, _OP = C.c_void_p, C.c_int64, C.c_size_t, C.POINTER(Shape), C.POINTER(RMSprop)

_SIGNATURES = {
    "pfw_version": (C.c_int, []),
    "pfw_status_string": (C.c_char_p, [C.c_int]),
    "pfw_param_count": (_I64, [_SP, C.c_int]),
    "pfw_workspace_bytes": (_SZ, [_SP, _I64, _I64]),
    "pfw_tiling": (C.c_int, [_SP, _I64, C.POINTER(TilingInfo)]),
    "pfw_generate": (C.c_int, [_VP, _SP, _VP, _VP, _VP, _I64, _VP]),
    "pfw_critic": (C.c_int, [_VP, _SP, _VP, _VP, _VP, _I64, _VP]),
    "pfw_loss_grad": (C.c_int, [_VP, _SP, C.c_int, _VP, _VP, _VP, _VP, _VP, _I64, _VP, _VP, _VP, _SZ]),
    "pfw_train_step": (C.c_int, [_VP, _SP, C.c_int, _VP, _VP, _VP, _VP, _VP, _VP, _I64, _OP, _VP, _VP, _VP, _SZ]),
    "pfw_fit_epoch": (C.c_int, [_VP, _SP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _I64, _I64, _VP, _OP, _VP, _VP, _SZ]),
    "pfw_epoch_losses": (C.c_int, [_VP, _SP, _VP, _VP, _VP, _VP, _I64, _VP, _VP, _SZ]),
}
EXPORTS = tuple(_SIGNATURES)


class WganLibraryMissing(LibraryMissing):
    pass


LIBRARY = Library(LIB_PATH, os.path.dirname(LIB_PATH), "pfw_", ABI_VERSION, _SIGNATURES, WganLibraryMissing,
                  "ConditionalWGAN has no CPU fallback.")
lib = LIBRARY.load
check = LIBRARY.check


def param_count(shape, net):
    n = int(lib().pfw_param_count(C.byref(shape), int(net)))
    if n < 0:
        raise ValueError("invalid ConditionalWGAN shape")
    return n


def workspace_bytes(shape, batch_rows, loss_rows=0):
    return int(lib().pfw_workspace_bytes(C.byref(shape), int(batch_rows), int(loss_rows)))


def tiling(shape, rows, require_step=True):
    """pfw_tiling_info of a training step / an inference call on `rows` rows (host only: no GPU needed).  A shape whose step
    cannot run raises, as every other call does, unless require_step is False: the step fields are then 0"""
    info = TilingInfo()
    st = lib().pfw_tiling(C.byref(shape), int(rows), C.byref(info))
    if st != EUNSUPPORTED or require_step:
        check(st, "pfw_tiling")
    return info


def rmsprop(lr, alpha=0.99, eps=1e-8, weight_decay=0.0, clamp=0.0):
    return RMSprop(float(lr), float(alpha), float(eps), float(weight_decay), float(clamp))


def generate(shape, params, z, c, n, out):
    """out [n, d] = G([z || c]) on the current stream (inference only: no autograd)"""
    check(lib().pfw_generate(_stream(), C.byref(shape), _f32(params, "params"), _f32(z, "z"), _f32(c, "C", True), int(n),
                             _f32(out, "out")), "pfw_generate")


def critic(shape, params, x, c, n, out):
    """out [n] = D([x || c]) on the current stream (inference only: no autograd)"""
    check(lib().pfw_critic(_stream(), C.byref(shape), _f32(params, "params"), _f32(x, "X"), _f32(c, "C", True), int(n),
                           _f32(out, "out")), "pfw_critic")


def loss_grad(shape, kind, params, x, c, row_index, z, rows, grad_out, loss_out, ws):
    check(lib().pfw_loss_grad(_stream(), C.byref(shape), int(kind), _f32(params, "params"), _f32(x, "X"), _f32(c, "C", True),
                              _ptr(row_index, torch.int64, "row_index", True), _f32(z, "z"), int(rows),
                              _f32(grad_out, "grad_out", True), _f32(loss_out, "loss_out", True),
                              _ptr(ws, torch.uint8, "workspace"), ws.numel()), "pfw_loss_grad")


def train_step(shape, kind, params, square_avg, x, c, row_index, z, rows, opt, grad_out, loss_out, ws):
    check(lib().pfw_train_step(_stream(), C.byref(shape), int(kind), _f32(params, "params"), _f32(square_avg, "square_avg"),
                               _f32(x, "X"), _f32(c, "C", True), _ptr(row_index, torch.int64, "row_index", True), _f32(z, "z"),
                               int(rows), C.byref(opt), _f32(grad_out, "grad_out", True), _f32(loss_out, "loss_out", True),
                               _ptr(ws, torch.uint8, "workspace"), ws.numel()), "pfw_train_step")


def fit_epoch(shape, params, square_avg, x, c, perm, z_batches, z_full, n, batch_size, kinds, opt, epoch_losses, ws):
    """kinds: a host int8 numpy array, one PFW_STEP_* per batch"""
    import numpy as np
    kinds = np.ascontiguousarray(kinds, dtype=np.int8)
    assert kinds.size == -(-int(n) // int(batch_size))
    check(lib().pfw_fit_epoch(_stream(), C.byref(shape), _f32(params, "params"), _f32(square_avg, "square_avg"), _f32(x, "X"),
                              _f32(c, "C", True), _ptr(perm, torch.int64, "perm"), _f32(z_batches, "z_batches"),
                              _f32(z_full, "z_full", True), int(n), int(batch_size), kinds.ctypes.data, C.byref(opt),
                              _f32(epoch_losses, "epoch_losses", True), _ptr(ws, torch.uint8, "workspace"), ws.numel()),
          "pfw_fit_epoch")


def epoch_losses(shape, params, x, c, z_full, n, out, ws):
    check(lib().pfw_epoch_losses(_stream(), C.byref(shape), _f32(params, "params"), _f32(x, "X"), _f32(c, "C", True),
                                 _f32(z_full, "z_full"), int(n), _f32(out, "epoch_losses"), _ptr(ws, torch.uint8, "workspace"),
                                 ws.numel()), "pfw_epoch_losses")
