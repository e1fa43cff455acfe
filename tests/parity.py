"""The measured tolerance of the GPU tests (tests/test_cnormal_gpu.py, tests/test_*_tilings_gpu.py): a GPU result may be as far
from the float64 restatement as 4 times the float32 reference's own error on the same inputs, with a floor of 4 float32 ulp
of the quantity's magnitude.  The 4x margin is profiles/r09_cnormal_parity.txt's."""
import numpy as np

EPS32 = float(np.finfo(np.float32).eps)


def bound(ref32, ref64, magnitude=None, also32=None):
    """(bound, e_ref): max(4 e_ref, 4 ulp of the magnitude), e_ref = max |ref32 - ref64|; magnitude defaults to max |ref64|.
    also32: a second float32 restatement of the same quantity (the kernels' summation order, tests/tilings_cases.py);
    e_ref is then the larger of the two errors"""
    ref64 = np.asarray(ref64, np.float64)
    e_ref = max(float(np.abs(np.asarray(r, np.float64) - ref64).max()) for r in (ref32, also32) if r is not None)
    mag = float(np.abs(ref64).max()) if magnitude is None else float(magnitude)
    return max(4 * e_ref, 4 * EPS32 * mag), e_ref


def parity(case, what, got, ref32, ref64, magnitude=None, also32=None):
    """assert |got - ref64| <= max(4 e_ref, 4 ulp of the magnitude), e_ref = |ref32 - ref64|; max norms"""
    got = np.asarray(got, np.float64)
    b, e_ref = bound(ref32, ref64, magnitude, also32)
    err = float(np.abs(got - np.asarray(ref64, np.float64)).max())
    print("PARITY %-14s %-22s e_ref %.3e  gpu %.3e  bound %.3e%s" % (case, what, e_ref, err, b,
                                                                      "" if also32 is None else "  (kernel-order e_ref)"))
    assert err <= b, (case, what, err, e_ref, b)
