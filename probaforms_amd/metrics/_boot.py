"""Host side shared by the bootstrapped metrics: argument checks, the float64 device copies, the
StandardScaler step, the bootstrap index stream of the reference, and the one driver of a call's replicates.

The reference resamples with `sklearn.utils.resample(X)` (mmd.py:54-55, fd.py:41-42), which on numpy's
global legacy generator draws `randint(0, n, size=n)`; per iteration X's indices first, then Y's.  The
same draws are made here, in the same order, so the generator ends where the reference leaves it.
Replicates run in groups whose indices are drawn on the host, uploaded as int32 and consumed by the
kernels; the next group is drawn while the current group's kernels run.  replicates() is what a metric
calls: it sizes the groups and the workspace, and runs either the drawn replicates or the identity one.
"""
import numpy as np
import torch

INDEX_BYTES_PER_GROUP = 64 << 20      # int32 indices of one group of replicates
WORKSPACE_BYTES_PER_GROUP = 256 << 20 # kernel workspace of one group (beyond one replicate's own)
MAX_GROUP = 128                       # replicates per group: a default call (n_iters = 100) is one group


def _check_2d(A, name):
    """shape and dtype checks on the caller's object, before anything touches a device"""
    if isinstance(A, torch.Tensor):
        if A.is_complex() or A.dtype == torch.bool:
            raise ValueError("%s: expected a real numeric tensor, got %s" % (name, A.dtype))
        shape = tuple(A.shape)
    else:
        A = np.asarray(A)
        if A.dtype.kind not in "fiu":
            raise ValueError("%s: expected a real numeric array, got dtype %s" % (name, A.dtype))
        shape = A.shape
    if len(shape) != 2:
        raise ValueError("%s: expected a 2-D array [n_samples, n_features], got shape %s" % (name, shape))
    if shape[0] < 1 or shape[1] < 1:
        raise ValueError("%s: expected at least one sample and one feature, got shape %s" % (name, shape))
    if shape[0] >= 2 ** 31:
        raise ValueError("%s: at most 2**31 - 1 samples (int32 bootstrap indices), got %d" % (name, shape[0]))
    return A, shape


def prepare(A, B, names, n_iters, standardize=False, graph=False):
    """-> (A, B) as contiguous float64 tensors on one HIP device, standardized there if asked.  A CUDA tensor
    stays on its device (float32 is upcast there); anything else is converted with numpy and uploaded.
    graph: tensors are not detached, so the cast, the copy and the scaler stay in their autograd graph (losses.py)."""
    from . import _m1d                    # (imports this module)
    A, sa = _check_2d(A, names[0])
    B, sb = _check_2d(B, names[1])
    if sa[1] != sb[1]:
        raise ValueError("%s and %s have different numbers of features: %d and %d" % (names[0], names[1], sa[1], sb[1]))
    _m1d.check_positive_int(n_iters, "n_iters")
    if not torch.cuda.is_available():
        raise RuntimeError("probaforms_amd.metrics runs on a HIP device and none is visible (there is no CPU fallback)")
    dev = None
    for t in (A, B):
        if isinstance(t, torch.Tensor) and t.is_cuda:
            dev = t.device
            break
    if dev is None:
        dev = torch.device("cuda", torch.cuda.current_device())

    def dev64(t):
        if not isinstance(t, torch.Tensor):
            t = torch.from_numpy(np.ascontiguousarray(t, dtype=np.float64))
        return (t if graph else t.detach()).to(device=dev, dtype=torch.float64).contiguous()
    A, B = dev64(A), dev64(B)
    if standardize:
        with torch.cuda.device(dev):
            A, B = globals()["standardize"](A, B)      # (the argument shadows the function)
    return A, B


def standardize(A, B):
    """StandardScaler fitted on A (mean, population std; a std of 0 becomes 1), applied to A and B"""
    mu = A.mean(dim=0)
    sd = A.var(dim=0, unbiased=False).sqrt()
    sd = torch.where(sd == 0, torch.ones_like(sd), sd)
    return ((A - mu) / sd).contiguous(), ((B - mu) / sd).contiguous()


def group_size(n_iters, rows, ws_per_rep=0):
    g = min(INDEX_BYTES_PER_GROUP // (4 * rows), WORKSPACE_BYTES_PER_GROUP // max(1, ws_per_rep))
    return int(max(1, min(n_iters, MAX_GROUP, g)))


def draw_indices(out, reps, na, nb):
    """the reference's stream: per replicate randint(0, na, na) then randint(0, nb, nb), into the int32
    host view `out` laid out [reps, na] then [reps, nb]"""
    xa = out[:reps * na].reshape(reps, na)
    xb = out[reps * na:reps * (na + nb)].reshape(reps, nb)
    randint = np.random.randint           # numpy's global legacy RandomState, as sklearn.utils.resample uses it
    for r in range(reps):
        xa[r] = randint(0, na, size=na)
        xb[r] = randint(0, nb, size=nb)


def group_sizes(n_iters, rows, ws_per_rep=0):
    """the distinct replicate counts of the groups of a call (the last group may be shorter)"""
    G = group_size(n_iters, rows, ws_per_rep)
    return sorted({G, n_iters - (n_iters - 1) // G * G})


def run_groups(n_iters, na, nb, device, launch, ws_per_rep=0):
    """Draw and upload the indices group by group and call launch(start, reps, idx_a, idx_b) for each.
    Two pinned host buffers and two device buffers alternate: a group's draw overlaps the kernels of the
    group before it; a pinned buffer is refilled only once its previous upload has finished."""
    rows = na + nb
    G = group_size(n_iters, rows, ws_per_rep)
    nbuf = 1 if G >= n_iters else 2
    host = [torch.empty(G * rows, dtype=torch.int32, pin_memory=True) for _ in range(nbuf)]
    dev = [torch.empty(G * rows, dtype=torch.int32, device=device) for _ in range(nbuf)]
    done = [None] * nbuf
    stream = torch.cuda.current_stream()
    for gi, start in enumerate(range(0, n_iters, G)):
        reps = min(G, n_iters - start)
        k = gi % nbuf
        if done[k] is not None:
            done[k].synchronize()
        draw_indices(host[k].numpy(), reps, na, nb)
        d = dev[k][:reps * rows]
        d.copy_(host[k][:reps * rows], non_blocking=True)
        done[k] = torch.cuda.Event()
        done[k].record(stream)
        launch(start, reps, d[:reps * na], d[reps * na:])


def replicates(na, nb, device, n_iters, workspace_bytes, launch, ws_per_rep=None):
    """The replicates of one call on samples of na and nb rows: launch(start, reps, idx_a, idx_b, ws) enqueues
    replicates start .. start + reps - 1 from their int32 indices [reps, na] and [reps, nb], with the
    workspace ws of workspace_bytes(reps) bytes at least (the metric's own size function of a group's replicate
    count).  The groups are run_groups', sized by ws_per_rep: workspace_bytes(1) unless the metric counts
    other bytes per replicate.  The first group is the largest.
    n_iters = None is the identity replicate, the samples as given: one launch, nothing is drawn from numpy's
    generator and no pinned buffer is made."""
    def empty(nbytes):
        return torch.empty(nbytes, dtype=torch.uint8, device=device)

    if n_iters is None:
        ia, ib = (torch.arange(n, dtype=torch.int32, device=device) for n in (na, nb))
        launch(0, 1, ia, ib, empty(workspace_bytes(1)))
        return
    if ws_per_rep is None:
        ws_per_rep = workspace_bytes(1)
    ws = empty(max(workspace_bytes(r) for r in group_sizes(n_iters, na + nb, ws_per_rep)))
    run_groups(n_iters, na, nb, device, lambda start, reps, ia, ib: launch(start, reps, ia, ib, ws), ws_per_rep)
