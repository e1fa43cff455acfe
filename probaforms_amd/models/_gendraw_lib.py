"""ctypes binding of libpf_gendraw.so (C ABI: probaforms_amd/models/gendraw_csrc/pf_gendraw.h).

The library is built in-tree by `make -C probaforms_amd/models/gendraw_csrc` (see __graft_entry__.build) and loaded on the
first call, so importing probaforms_amd.models needs no GPU.  A missing library or a tensor off the HIP device raises; a shape
the kernels do not hold in LDS is reported by `supported()` / `Unsupported`, and the callers then run the loop the call
replaces (see models/_gendraw.py).
"""
import ctypes as C
import os

import torch

from .._cbind import Library, LibraryMissing, f32 as _f32, ptr as _ptr, stream as _stream

ABI_VERSION = 100                  # pfg_version() of the library this binding matches (pf_gendraw.h PFG_VERSION)
EUNSUPPORTED = -2                  # PFG_EUNSUPPORTED
MAX_HIDDEN = 8                     # PFG_MAX_HIDDEN
MAX_D = 32                         # PFG_MAX_D
WAVES = 4                          # PFG_WAVES
ACT_TANH, ACT_RELU = 0, 1          # RNVP_ACT_*

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "gendraw_csrc", "libpf_gendraw.so")


class Mlp(C.Structure):
    """pfg_mlp"""
    _fields_ = [("n_out", C.c_int32), ("c", C.c_int32), ("latent", C.c_int32), ("n_hidden", C.c_int32),
                ("hidden", C.c_int32 * MAX_HIDDEN), ("act", C.c_int32)]

    @classmethod
    def make(cls, n_out, c, latent, hidden, activation):
        hidden = [int(h) for h in hidden]
        if not 1 <= len(hidden) <= MAX_HIDDEN:
            raise ValueError("the generator draw kernel supports 1..%d hidden layers (got %d)" % (MAX_HIDDEN, len(hidden)))
        s = cls()
        s.n_out, s.c, s.latent, s.n_hidden = int(n_out), int(c), int(latent), len(hidden)
        for i, h in enumerate(hidden):
            s.hidden[i] = h
        s.act = ACT_TANH if activation == 'tanh' else ACT_RELU      # anything but 'tanh' is ReLU, as the models build it
        return s


class PlanInfo(C.Structure):
    """pfg_plan_info"""
    _fields_ = [("draw_tiles", C.c_int32), ("waves", C.c_int32), ("weights_in_lds", C.c_int32), ("reserved", C.c_int32),
                ("lds_bytes", C.c_int64), ("packed_bytes", C.c_int64)]


_VP, _I64, _I32, _SZ, _MP = C.c_void_p, C.c_int64, C.c_int32, C.c_size_t, C.POINTER(Mlp)

_SIGNATURES = {
    "pfg_version": (C.c_int, []),
    "pfg_status_string": (C.c_char_p, [C.c_int]),
    "pfg_workspace_bytes": (_SZ, [_MP, _I64]),
    "pfg_plan": (C.c_int, [_MP, _I64, C.POINTER(PlanInfo)]),
    "pfg_mlp_draw_accumulate": (C.c_int, [_VP, _MP, _VP, _VP, _I64, _I64, _VP, _I64, _I64, _I64, _I64, _VP, _VP, _VP, _VP,
                                          _SZ]),
    "pfg_affine_draw_accumulate": (C.c_int, [_VP, _I32, _VP, _VP, _VP, _VP, _VP, _I64, _I64, _I64, _I64, _I64, _I64, _VP,
                                             _VP, _VP]),
}
EXPORTS = tuple(_SIGNATURES)


class GendrawLibraryMissing(LibraryMissing):
    pass


class Unsupported(RuntimeError):
    """one draw tile's activations do not fit the LDS, or d > MAX_D (PFG_EUNSUPPORTED)"""


LIBRARY = Library(LIB_PATH, os.path.dirname(LIB_PATH), "pfg_", ABI_VERSION, _SIGNATURES, GendrawLibraryMissing,
                  unsupported=(EUNSUPPORTED, Unsupported))
lib = LIBRARY.load
check = LIBRARY.check


def workspace_bytes(net, k_cnt):
    """bytes of workspace of pfg_mlp_draw_accumulate; 0 = the kernel does not serve this shape"""
    return int(lib().pfg_workspace_bytes(C.byref(net), int(k_cnt)))


def supported(net):
    """host only: does one tile of 16 draws per wave fit the LDS?"""
    return workspace_bytes(net, 1) > 0


def plan(net, k_cnt):
    """pfg_plan_info of a launch with k_cnt draws (host only: no GPU needed); Unsupported where the kernel cannot run"""
    info = PlanInfo()
    check(lib().pfg_plan(C.byref(net), int(k_cnt), C.byref(info)), "pfg_plan")
    return info


def mlp_draw_accumulate(net, params, c, n_rows, row_offset, z, n_total, k_lo, k_cnt, k_total, state, x_out, xt_out, ws):
    """z: device tensor [k_cnt, n_total, latent]; state / x_out / xt_out nullable"""
    check(lib().pfg_mlp_draw_accumulate(_stream(), C.byref(net), _f32(params, "params"), _f32(c, "C", True), int(n_rows),
                                        int(row_offset), _f32(z, "z"), int(n_total), int(k_lo), int(k_cnt), int(k_total),
                                        _ptr(state, torch.uint8, "state", True), _f32(x_out, "x_out", True),
                                        _f32(xt_out, "xt_out", True), _ptr(ws, torch.uint8, "workspace", True),
                                        0 if ws is None else ws.numel()), "pfg_mlp_draw_accumulate")


def affine_draw_accumulate(d, mu, sigma, out_w, out_b, eps, n_rows, row_offset, n_total, k_lo, k_cnt, k_total, state, x_out,
                           xt_out):
    """mu, sigma [n_rows, d]; out_w [d, d] / out_b [d] or both None (independent covariance); eps [k_cnt, n_total, d]"""
    check(lib().pfg_affine_draw_accumulate(_stream(), int(d), _f32(mu, "mu"), _f32(sigma, "sigma"), _f32(out_w, "out_w", True),
                                           _f32(out_b, "out_b", True), _f32(eps, "eps"), int(n_rows), int(row_offset),
                                           int(n_total), int(k_lo), int(k_cnt), int(k_total),
                                           _ptr(state, torch.uint8, "state", True), _f32(x_out, "x_out", True),
                                           _f32(xt_out, "xt_out", True)), "pfg_affine_draw_accumulate")
