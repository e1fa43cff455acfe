"""Float64 numpy / scipy restatement of probaforms_amd.metrics.twosample (kernels: pf_perm.hip):
  philox4x32_10  the counter-based generator, checked against the Random123 known answers (KNOWN_ANSWERS);
  labels         the labellings of pfm_perm_labels: a stable argsort of the masked 64-bit keys, the first nr get label 1;
  form           the signed pair sums S = s G s and the sums of magnitudes A = |s| G |s| of given labellings, with scipy's cdist
                 and einsum;
  form_tiles     the same S added in the kernel's order (tiles of the upper triangle, lists per workgroup, a row's 64 b in
                 order, the lanes' and the waves' order), without its fused multiply-adds and whatever order the matrix
                 instruction adds its four products in;
  test           the whole public call: one seed draw from numpy's global generator, the observed labelling in front of the
                 drawn ones, the statistic, the null values and the p-value.
The yardstick the two-sample tests hold the GPU kernels and the committed fixtures against.  Test helper, not product code.
"""
import numpy as np
from scipy.spatial.distance import cdist

from wasserstein_numpy import standardize  # noqa: F401

ENERGY, GAUSS = 0, 1              # pf_metrics.h PFM_PERM_*
ALL = 2 ** 64 - 1                 # key_mask in use
TILE = 64                         # pf_quadform.h: rows per side of a pair tile,
MIN_LIST, TARGET_WGS = 4, 2048    # tiles per workgroup at least, workgroups per call about
M32 = np.uint64(0xFFFFFFFF)

# (counter, key) -> output: Random123's kat_vectors for philox4x32 with 10 rounds
KNOWN_ANSWERS = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def philox4x32_10(counter, key):
    """counter: four arrays (or scalars) of 32-bit words, key: two words -> four uint64 arrays of 32-bit words"""
    c = [np.asarray(v, dtype=np.uint64) & M32 for v in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = np.uint64(int(key[0]) & 0xFFFFFFFF), np.uint64(int(key[1]) & 0xFFFFFFFF)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]             # 32 x 32 -> 64 bits: no overflow
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & M32]
        k0 = (k0 + np.uint64(0x9E3779B9)) & M32
        k1 = (k1 + np.uint64(0xBB67AE85)) & M32
    return c


def keys(seed, p, N, mask=ALL):
    """the masked 64-bit sort keys of the N pooled rows under labelling p"""
    w = philox4x32_10((np.arange(N, dtype=np.uint64), 0, p, 0), (seed & 0xFFFFFFFF, seed >> 32))
    return (w[0] | w[1] << np.uint64(32)) & np.uint64(mask)


def labels(seed, first, reps, N, nr, mask=ALL):
    """-> uint8 [reps, N]: labelling first + r has label 1 on the nr rows of smallest (key, row)"""
    out = np.zeros((reps, N), np.uint8)
    for r in range(reps):
        out[r, np.argsort(keys(seed, first + r, N, mask), kind="stable")[:nr]] = 1
    return out


def observed(N, nr):
    return (np.arange(N) < nr).astype(np.uint8)


def pair_values(Z, kind, gamma=0.0):
    Z = np.asarray(Z, np.float64)
    return cdist(Z, Z) if kind == ENERGY else np.exp(-(gamma * cdist(Z, Z, "sqeuclidean")))


def weights(L, nr):
    L = np.asarray(L)
    return np.where(L != 0, float(L.shape[-1] - nr), -float(nr))


def form(Z, L, nr, kind, gamma=0.0):
    """-> (S, A) [reps]: the signed pair sums and the sums of the terms' magnitudes, all ordered pairs, diagonal included"""
    s, G = weights(np.atleast_2d(L), nr), pair_values(Z, kind, gamma)
    return np.einsum("pa,pa->p", s @ G, s), np.einsum("pa,pa->p", np.abs(s) @ G, np.abs(s))


def form_tiles(Z, L, nr, kind, gamma=0.0):
    """S in the kernel's order of summation (products and sums rounded separately where the kernel fuses them)"""
    s, G = weights(np.atleast_2d(L), nr), pair_values(Z, kind, gamma)
    R, N = s.shape
    tn = -(-N // TILE)
    Gp, sp = np.zeros((tn * TILE, tn * TILE)), np.zeros((R, tn * TILE))       # rows past the end weigh 0
    Gp[:N, :N], sp[:, :N] = G, s
    tiles = [(I, J) for I in range(tn) for J in range(I, tn)]
    per_wg = max(MIN_LIST, -(-len(tiles) // TARGET_WGS))
    S = np.zeros(R)
    lk = np.arange(4)
    for first in range(0, len(tiles), per_wg):
        acc = np.zeros((R, 4, 4))                    # the accumulator of lane (wave w, lk) for each labelling
        for I, J in tiles[first:first + per_wg]:
            wgt = 2.0 if I != J else 1.0
            Gt = Gp[I * TILE:(I + 1) * TILE, J * TILE:(J + 1) * TILE]
            sa, sb = sp[:, I * TILE:(I + 1) * TILE], sp[:, J * TILE:(J + 1) * TILE]
            T = np.zeros((R, TILE))                  # T[a] over all 64 b (the wave's MFMA chain; four b per instruction)
            for b in range(TILE):
                T = T + Gt[None, :, b] * sb[:, b, None]
            for w in range(4):
                for i in range(4):                   # the lane's rows 16 w + lk + 4 i
                    rows = slice(16 * w + 4 * i, 16 * w + 4 * i + 4)
                    acc[:, w] = acc[:, w] + (wgt * sa[:, rows]) * T[:, rows]
        for x in (1, 2):
            acc = acc + acc[:, :, lk ^ x]
        part = acc[:, 0, 0]
        for w in range(1, 4):
            part = part + acc[:, w, 0]
        S = S + part
    return S


def values(S, nr, nf, kind):
    """raw sums -> D^2 = -S / (nr nf)^2 or MMD^2 = +S / (nr nf)^2"""
    S, den = np.asarray(S, np.float64), np.float64((nr * nf) ** 2)
    return (0.0 - S) / den if kind == ENERGY else (0.0 + S) / den


def pvalue(statistic, null):
    return (1 + int(np.count_nonzero(np.asarray(null) >= statistic))) / (1 + len(null))


def median(X, Y):
    return np.median(cdist(np.concatenate([X, Y]), np.concatenate([X, Y])))


def draw_seed():
    lo, hi = np.random.randint(0, 2 ** 32, size=2, dtype=np.uint64)
    return int(lo) | int(hi) << 32


def test(X, Y, n_permutations, kind, gamma=0.0):
    """the public call on the samples as given (standardize them first where that is meant) -> dict: key (the drawn seed),
    statistic, null, pvalue, bound (1e-12 A / (nr nf)^2 of the observed labelling and of every drawn one) and the generator's
    next random()"""
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    nr, nf = len(X), len(Y)
    seed = draw_seed()
    nxt = np.random.random()
    L = np.concatenate([observed(nr + nf, nr)[None], labels(seed, 0, n_permutations, nr + nf, nr)])
    S, A = form(np.concatenate([X, Y]), L, nr, kind, gamma)
    V = values(S, nr, nf, kind)
    return dict(key=seed, statistic=V[0], null=V[1:], pvalue=pvalue(V[0], V[1:]), bound=1e-12 * A / np.float64((nr * nf) ** 2),
                next=nxt)


test.__test__ = False             # (not a pytest test, whatever imports it)


# ---- the shapes the host and GPU tests share ---------------------------------------------------------------------------

LABEL_CASES = [(2, 1), (3, 1), (3, 2), (64, 1), (255, 100), (256, 128), (257, 256), (600, 333), (2200, 1200)]   # (N, nr)
MASKS = [ALL, 3, 0]
FORM_SHAPES = [(1, 1), (1, 2), (40, 24), (33, 32), (64, 64), (100, 29)]                                       # (nr, nf)
FORM_DS = [1, 16, 17, 33]
FORM_REPS = [1, 15, 16, 17, 127, 128, 129]
LARGE = (1200, 1000, 3, 130)      # (nr, nf, d, reps): 35 tiles per side, 630 tiles, lists of 4, two slices of labellings
INTEGER = (65, 63, 1)
# the other shapes of tests/test_twosample_gpu.py (independence, hygiene)
OTHER = [(130, 93, 3), (70, 50, 2), (200, 150, 17)]
SEED = 0x123456789ABCDEF          # the labellings' seed in the kernel tests


def data(nr, nf, d):
    """continuous data: standard normal first rows, normal(0.3, 1.2) second rows"""
    rng = np.random.default_rng(1000 * nr + nf + 7 * d)
    return np.concatenate([rng.normal(size=(nr, d)), rng.normal(0.3, 1.2, size=(nf, d))])


def integer_data(nr, nf, d=1):
    """integers within +-1000: at d = 1 every distance, weight and sum is an integer below 2^53, so S is exact"""
    rng = np.random.default_rng(31)
    return np.concatenate([rng.integers(-1000, 1001, size=(nr, d)), rng.integers(-900, 1001, size=(nf, d))]).astype(np.float64)


def gamma_of(d):
    """a Gaussian kernel of unit order on the data above: sigma^2 = d"""
    return 1.0 / (2.0 * d)
