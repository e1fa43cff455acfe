"""The write-bounds and stream drivers (tests/bounds.py, tests/streams.py) on pfm_sym_eig and pfm_frechet_grad at d = 17 and d = 64 (the
LDS limit): guards intact, const inputs unchanged, every output written, the same bits on hostile workspaces, nothing put on stream
0, no wait for the device, and capturable into a graph.  Correctness against the references is in tests/test_frechet_gpu.py.

The module sorts among the other stream modules on purpose: the stream driver keeps one side stream per process, made on its first
use, and tests/test_streams_driver_gpu.py holds that driver against a fake entry point whose stages sit on stream 0.  When these cases
ran from tests/test_frechet_gpu.py, which sorts before every other user of the driver, that module's stage-1 case saw its gate pass in
the whole suite (supposed, not established: the side stream made that early shares a hardware queue with stream 0)."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bounds  # noqa: E402
import frechet_numpy as fr  # noqa: E402
import native_libs  # noqa: E402
import streams  # noqa: E402
from bounds import Out  # noqa: E402
from test_frechet_gpu import dev, eig_matrices  # noqa: E402
from probaforms_amd.metrics import _lib, fd  # noqa: E402

pytestmark = pytest.mark.gpu

native_libs.ensure_built(_lib)

F64, I32 = torch.float64, torch.int32


@pytest.mark.parametrize("d", (17, 64))
def test_bounds_and_streams(d):
    mats = eig_matrices(d)
    A = dev(np.stack([mats["cov"], mats["indef"], mats["diag"]]))
    need = _lib.sym_eig_workspace_bytes(3, d)
    outs = dict(w=Out(F64, (3, d)), V=Out(F64, (3, d, d)), sweeps=Out(I32, (3,)))
    call = lambda ws, o: _lib.sym_eig_status(A, o["w"], o["V"], o["sweeps"], ws)  # noqa: E731
    what = "pfm_sym_eig[3 matrices, d %d]" % d
    ref = bounds.run(what, need, call, outs, dict(A=A), keeps_nothing=True)[1]
    res = streams.run(what, need, call, outs, dict(A=A), reference=ref)
    assert res["pending"] and res["captured"]

    nr, nf = (90, 70) if d == 17 else (300, 260)
    Xr, Xf = fr.data(nr, nf, d)
    Z = dev(np.concatenate([Xr, Xf]))
    n = nr + nf
    need = _lib.frechet_grad_workspace_bytes(n, d, nr)
    rc = d * 2.0 ** -52
    outs = dict(value=Out(F64, (1,)), grad=Out(F64, (n, d)), parts=Out(F64, (5,)), eig=Out(F64, (d,)), rank=Out(I32, (2,)))
    call = lambda ws, o: _lib.frechet_grad_status(Z, nr, rc, 3, o["value"], o["grad"], o["parts"], o["eig"], o["rank"], ws)  # noqa: E731
    what = "pfm_frechet_grad[%d+%d rows, d %d]" % (nr, nf, d)
    ref = bounds.run(what, need, call, outs, dict(Z=Z))[1]
    res = streams.run(what, need, call, outs, dict(Z=Z), reference=ref)
    assert res["pending"] and res["captured"]
    outs = dict(value=Out(F64, (1,)), rank=Out(I32, (2,)))
    call = lambda ws, o: _lib.frechet_grad_status(Z, nr, rc, 2, o["value"], None, None, None, o["rank"], ws)  # noqa: E731
    what = "pfm_frechet_grad[%d+%d rows, d %d, value alone]" % (nr, nf, d)
    ref = bounds.run(what, need, call, outs, dict(Z=Z))[1]
    streams.run(what, need, call, outs, dict(Z=Z), reference=ref)
    assert ref["value"].cpu().numpy()[0] == fd.frechet_distance_full_sample(Xr, Xf)
