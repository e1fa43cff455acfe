"""ctypes binding of libpf_predict.so (C ABI: probaforms_amd/models/predict_csrc/pf_predict.h).

The library is built in-tree by `make -C probaforms_amd/models/predict_csrc` (see __graft_entry__.build) and loaded on the
first call, so importing probaforms_amd.models needs no GPU.  A missing library or a tensor off the HIP device raises; a shape
the kernels do not hold in LDS is reported by `supported()` / `Unsupported`, and the callers then run the loop the call
replaces (see NormalizingFlow.sample_stats).
"""
import ctypes as C
import os

import numpy as np
import torch

from .._cbind import Library, LibraryMissing, f32 as _f32, ptr as _ptr, stream as _stream
from .._hip import RnvpShape

ABI_VERSION = 101                  # pfp_version() of the library this binding matches (pf_predict.h PFP_VERSION)
EUNSUPPORTED = -2                  # PFP_EUNSUPPORTED
STATE_BYTES = 32                   # PFP_STATE_BYTES
MAX_QUANTILE_DRAWS = 8192          # PFP_MAX_QUANTILE_DRAWS

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "predict_csrc", "libpf_predict.so")

_VP, _I64, _I32, _SZ, _SP = C.c_void_p, C.c_int64, C.c_int32, C.c_size_t, C.POINTER(RnvpShape)


class JointTile(C.Structure):
    """pfp_joint_tile: how pfp_joint_scores walks one row of (d, K)"""
    _fields_ = [(name, _I32) for name in ("tile_draws", "n_tiles", "chunk_cols", "n_chunks", "budget_bytes", "lds_bytes",
                                          "threads", "max_grid")]


_SIGNATURES = {
    "pfp_version": (C.c_int, []),
    "pfp_status_string": (C.c_char_p, [C.c_int]),
    "pfp_workspace_bytes": (_SZ, [_SP, _I64]),
    "pfp_draw_accumulate": (C.c_int, [_VP, _SP, _VP, _VP, _VP, _I64, _I64, _VP, _VP, _I64, _I64, _I64, _I64, _VP, _VP, _VP,
                                      _VP, _SZ]),
    "pfp_finalize": (C.c_int, [_VP, _VP, _I64, _I32, _I32, _VP, _VP, _VP, _VP]),
    "pfp_quantiles": (C.c_int, [_VP, _VP, _I64, _I32, _I64, _VP, _I32, _VP]),
    "pfp_scores": (C.c_int, [_VP, _VP, _VP, _I64, _I32, _I64, _I32, _VP, _I32, _VP, _VP, _VP, _VP]),
    "pfp_joint_scores": (C.c_int, [_VP, _VP, _VP, _I64, _I32, _I64, _I32, C.c_double, _VP, _VP, _VP]),
    "pfp_joint_tiling": (C.c_int, [_I32, _I64, C.POINTER(JointTile)]),
}
EXPORTS = tuple(_SIGNATURES)


class PredictLibraryMissing(LibraryMissing):
    pass


class Unsupported(RuntimeError):
    """the shape's per-tile image does not fit the LDS (PFP_EUNSUPPORTED)"""


LIBRARY = Library(LIB_PATH, os.path.dirname(LIB_PATH), "pfp_", ABI_VERSION, _SIGNATURES, PredictLibraryMissing,
                  unsupported=(EUNSUPPORTED, Unsupported))
lib = LIBRARY.load
check = LIBRARY.check


def workspace_bytes(shape, k_cnt):
    """bytes of workspace for k_cnt draws per call; 0 = the kernels do not serve this shape"""
    return int(lib().pfp_workspace_bytes(C.byref(shape), int(k_cnt)))


def supported(shape):
    return workspace_bytes(shape, 1) > 0


def new_state(n_rows, d, device):
    """zeroed running moments [n_rows, d] (PFP_STATE_BYTES each): nothing seen yet"""
    return torch.zeros((int(n_rows), int(d), STATE_BYTES), dtype=torch.uint8, device=device)


def draw_accumulate(shape, params, masks, c, n_rows, row_offset, seeds, z, n_total, k_lo, k_cnt, k_total, state, x_out, xt_out,
                    ws):
    """seeds: sequence of k_cnt ints (host) or None; z: device tensor [k_cnt, n_total, d] or None.  Returns the host seed
    array, which the caller keeps alive until the stream has consumed it."""
    hseeds = None
    if seeds is not None:
        hseeds = np.ascontiguousarray(np.asarray([int(s) & 0xFFFFFFFFFFFFFFFF for s in seeds], dtype=np.uint64))
        if hseeds.size != int(k_cnt):
            raise ValueError("seeds must hold k_cnt = %d entries, got %d" % (k_cnt, hseeds.size))
    check(lib().pfp_draw_accumulate(_stream(), C.byref(shape), _f32(params, "params"), _ptr(masks, torch.uint8, "masks", True),
                                    _f32(c, "C", True), int(n_rows), int(row_offset),
                                    None if hseeds is None else hseeds.ctypes.data, _f32(z, "z", True), int(n_total),
                                    int(k_lo), int(k_cnt), int(k_total), _ptr(state, torch.uint8, "state", True),
                                    _f32(x_out, "x_out", True), _f32(xt_out, "xt_out", True),
                                    _ptr(ws, torch.uint8, "workspace", True), 0 if ws is None else ws.numel()),
          "pfp_draw_accumulate")
    return hseeds


def finalize(state, n_rows, d, ddof, mean, std, mn, mx):
    check(lib().pfp_finalize(_stream(), _ptr(state, torch.uint8, "state"), int(n_rows), int(d), int(ddof),
                             _f32(mean, "mean", True), _f32(std, "std", True), _f32(mn, "min", True), _f32(mx, "max", True)),
          "pfp_finalize")


def quantiles(xt, n_rows, d, k_total, probs, q_out):
    """probs: float64 device tensor [Q]; q_out: float32 [Q, n_rows, d]"""
    check(lib().pfp_quantiles(_stream(), _f32(xt, "xt"), int(n_rows), int(d), int(k_total),
                              _ptr(probs, torch.float64, "probs"), int(probs.numel()), _f32(q_out, "q_out")), "pfp_quantiles")


def scores(xt, y, n_rows, d, k_total, fair, probs, crps, pit, q_out, pinball):
    """xt [n_rows, d, k_total], y [n_rows, d] float32; probs: float64 device tensor [Q] or None; crps, pit [n_rows, d] and
    q_out, pinball [Q, n_rows, d] float32, each nullable"""
    py, px = _f32(y, "y"), _f32(xt, "xt")
    nq = 0 if probs is None else int(probs.numel())
    check(lib().pfp_scores(_stream(), px, py, int(n_rows), int(d), int(k_total), int(bool(fair)),
                           _ptr(probs, torch.float64, "probs", True) if nq else None, nq, _f32(crps, "crps", True),
                           _f32(pit, "pit", True), _f32(q_out, "q_out", True), _f32(pinball, "pinball", True)), "pfp_scores")


def joint_scores(xt, y, n_rows, d, k_total, fair, variogram_order, energy, spread, variogram):
    """xt [n_rows, d, k_total], y [n_rows, d] float32; energy, spread, variogram [n_rows] float32, each nullable;
    variogram_order 0.5, 1 or 2 (anything when variogram is None)"""
    py, px = _f32(y, "y"), _f32(xt, "xt")
    order = 0.5 if variogram_order is None else float(variogram_order)
    check(lib().pfp_joint_scores(_stream(), px, py, int(n_rows), int(d), int(k_total), int(bool(fair)), order,
                                 _f32(energy, "energy", True), _f32(spread, "spread", True),
                                 _f32(variogram, "variogram", True)), "pfp_joint_scores")


def joint_tiling(d, k_total):
    """JointTile of one row of (d, k_total): decided on the host, no GPU"""
    t = JointTile()
    check(lib().pfp_joint_tiling(int(d), int(k_total), C.byref(t)), "pfp_joint_tiling")
    return t
