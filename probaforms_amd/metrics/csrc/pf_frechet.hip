// pf_frechet.hip -- a batched symmetric eigensolver and the Frechet distance with its row gradients for gfx950 (C ABI:
// pf_metrics.h, pfm_sym_eig and pfm_frechet_grad).
//
// Eigensolver: cyclic Jacobi in a parallel (round-robin) order, one workgroup of 1024 threads per matrix, everything in LDS at a row pitch of
// d | 1 doubles.  With m = d rounded up to even, a sweep is m - 1 rounds of m / 2 disjoint index pairs (the circle method: index
// m - 1 stays, the others turn; for odd d the index d is a bye).  A round is three steps with a barrier after each:
//   rotations   one lane per pair (p < q): skipped where |a_pq| <= 2^-53 sqrt|a_pp| sqrt|a_qq| (the relative criterion of Demmel &
//               Veselic), else tau = (a_qq - a_pp) / (2 a_pq), t = sgn(tau) / (|tau| + sqrt(1 + tau^2)), c = 1 / sqrt(1 + t^2),
//               s = t c, and the new diagonal a_pp - t a_pq, a_qq + t a_pq
//   columns     X = A J, V = V J: one item per (row, pair)
//   rows        A = J^T X: one item per (pair, column); only the entries above the diagonal are kept and each is written to both
//               triangles, the pair's own 2 x 2 block is written from the rotation step's values (a_pq = 0 exactly): A stays
//               exactly symmetric
// The loop ends after a sweep without a rotation and after PFM_EIG_MAX_SWEEPS at the latest; a NaN compares false with the
// threshold, so a matrix that holds one rotates in every sweep and ends at the bound, all NaN.  The eigenvalues are the diagonal,
// ranked ascending (NaN last, ties by index).
//
// Frechet distance, pfm_frechet_grad, three steps:
//   moments     k_mean_* / k_cov_* of pf_metrics.hip with null indices (pf_moments.h): bitwise pfm_boot_moments'
//   k_frechet_core   one workgroup per route, four d x d matrices in LDS.  Route 0 (A = cov_r, B = cov_f): S = A^(1/2) from the
//               eigen-decomposition of A (eigenvalues clipped at 0), M = sym(S B S), its eigenvalues lambda, tr sqrt = sum
//               sqrt(max(lambda, 0)) ascending, the value and the parts, and G_f = I - S M^(-1/2)_cut S.  Route 1 swaps A and B
//               and gives G_r; it runs only where the real rows' gradient is asked for
//   k_frechet_rows   64 rows of one sample per workgroup: G_s, mu_s and the mean term in LDS, the features summed ascending
// Every sum runs in a fixed order: no float atomics, the same bits in any call.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "pf_common.h"
#include "pf_metrics.h"
#include "pf_moments.h"

namespace {

constexpr int MAXD = PFM_FRECHET_MAX_D;
constexpr int HALF = MAXD / 2;
constexpr int ROWS = 64;                         // rows per workgroup of k_frechet_rows
constexpr int ET = 1024;                         // threads of the two kernels that hold the eigensolver: one workgroup per matrix is
                                                 // pure latency, and a round's d * ceil(d / 2) items are 2 per thread, not 8, at d = 64
constexpr double EPS = 1.1102230246251565e-16;   // 2^-53

struct Scratch {                                 // behind the matrices in LDS
    double c[HALF], s[HALF], app[HALF], aqq[HALF], apq[HALF];   // a round's rotations and the pairs' new 2 x 2 blocks
    double w[MAXD];                              // the eigenvalues, ascending
    double f[MAXD];                              // a function of them (the caller's)
    int p[HALF], q[HALF];                        // a round's pairs, p < q; q >= d: p has a bye
    int order[MAXD];                             // order[i]: the column of V that belongs to w[i]
    int rot;                                     // 1 + the last sweep that rotated
};

__host__ __device__ inline int pitch_of(int d) { return d | 1; }

inline size_t lds_bytes(int d, int matrices) {
    return sizeof(double) * (size_t)matrices * (size_t)d * (size_t)pitch_of(d) + sizeof(Scratch);
}

__device__ inline bool less_nan_last(double a, double b) { return a < b || (a == a && b != b); }

// the lower triangle and the diagonal of src [d, d] as a full symmetric matrix at pitch P; ends with a barrier
__device__ inline void load_sym(double *A, const double *src, int d, int P) {
    for (int e = threadIdx.x; e < d * d; e += ET) {
        const int i = e / d, j = e - i * d;
        A[i * P + j] = i >= j ? src[(int64_t)i * d + j] : src[(int64_t)j * d + i];
    }
    __syncthreads();
}

// Eigen-decomposition of the symmetric A [d, d] (pitch P, in LDS; destroyed): V's columns are the eigenvectors, sc.w the
// eigenvalues ascending, column sc.order[i] of V belongs to sc.w[i].  X is a third matrix of scratch.  A must be complete when the
// call begins (a barrier has passed); ends with a barrier.  -> the sweeps that rotated something
__device__ int jacobi(double *__restrict__ A, double *__restrict__ V, double *__restrict__ X, int d, int P, Scratch &sc) {
    const int tid = threadIdx.x;
    const int m = (d + 1) & ~1, np = m / 2, rounds = m - 1;
    for (int e = tid; e < d * d; e += ET) {
        const int i = e / d, j = e - i * d;
        V[i * P + j] = i == j ? 1.0 : 0.0;
    }
    if (tid == 0) sc.rot = 0;
    __syncthreads();
    int sweeps = 0;
    for (int sweep = 0; sweep < PFM_EIG_MAX_SWEEPS; ++sweep) {
        for (int r = 0; r < rounds; ++r) {
            if (tid < np) {
                int i, j;
                if (tid == 0) { i = m - 1; j = r; }
                else { i = (r + tid) % rounds; j = (r + rounds - tid) % rounds; }
                const int p = i < j ? i : j, q = i < j ? j : i;
                double c = 1.0, s = 0.0, app = A[p * P + p], aqq = 0.0, apq = 0.0;
                if (q < d) {
                    aqq = A[q * P + q];
                    apq = A[p * P + q];
                    const double thr = EPS * (sqrt(fabs(app)) * sqrt(fabs(aqq)));
                    if (!(fabs(apq) <= thr)) {
                        const double tau = (aqq - app) / (2.0 * apq);
                        const double t = copysign(1.0, tau) / (fabs(tau) + sqrt(fma(tau, tau, 1.0)));
                        c = 1.0 / sqrt(fma(t, t, 1.0));
                        s = t * c;
                        app = fma(-t, apq, app);
                        aqq = fma(t, apq, aqq);
                        apq = 0.0;
                        sc.rot = sweep + 1;
                    }
                }
                sc.p[tid] = p; sc.q[tid] = q;
                sc.c[tid] = c; sc.s[tid] = s;
                sc.app[tid] = app; sc.aqq[tid] = aqq; sc.apq[tid] = apq;
            }
            __syncthreads();
            for (int e = tid; e < d * np; e += ET) {               // X = A J, V = V J
                const int k = e / np, pr = e - k * np;
                const int p = sc.p[pr], q = sc.q[pr];
                if (q < d) {
                    const double c = sc.c[pr], s = sc.s[pr];
                    const double ap = A[k * P + p], aq = A[k * P + q];
                    X[k * P + p] = fma(-s, aq, c * ap);
                    X[k * P + q] = fma(s, ap, c * aq);
                    const double vp = V[k * P + p], vq = V[k * P + q];
                    V[k * P + p] = fma(-s, vq, c * vp);
                    V[k * P + q] = fma(s, vp, c * vq);
                } else {
                    X[k * P + p] = A[k * P + p];
                }
            }
            __syncthreads();
            for (int e = tid; e < np * d; e += ET) {               // A = J^T X, the upper triangle mirrored
                const int pr = e / d, k = e - pr * d;
                const int p = sc.p[pr], q = sc.q[pr];
                if (k == p) {
                    A[p * P + p] = sc.app[pr];
                } else if (q < d) {
                    if (k == q) {
                        A[q * P + q] = sc.aqq[pr];
                        A[p * P + q] = A[q * P + p] = sc.apq[pr];
                    } else {
                        const double c = sc.c[pr], s = sc.s[pr];
                        const double xp = X[p * P + k], xq = X[q * P + k];
                        if (p < k) A[p * P + k] = A[k * P + p] = fma(-s, xq, c * xp);
                        if (q < k) A[q * P + k] = A[k * P + q] = fma(s, xp, c * xq);
                    }
                } else if (p < k) {
                    A[p * P + k] = A[k * P + p] = X[p * P + k];
                }
            }
            __syncthreads();
        }
        if (sc.rot <= sweep) break;       // (rot only grows: a lane that is already in the next sweep cannot mislead this one)
        ++sweeps;
    }
    if (tid < d) {
        const double wi = A[tid * P + tid];
        int rank = 0;
        for (int j = 0; j < d; ++j) {
            const double wj = A[j * P + j];
            if (less_nan_last(wj, wi) || (!less_nan_last(wi, wj) && j < tid)) ++rank;
        }
        sc.order[rank] = tid;
        sc.w[rank] = wi;
    }
    __syncthreads();
    return sweeps;
}

// out = sum_i sc.f[i] v_i v_i^T over the eigenvectors in ascending order of their eigenvalues; no barrier
__device__ inline void spectral(double *out, const double *V, int d, int P, const Scratch &sc) {
    for (int e = threadIdx.x; e < d * d; e += ET) {
        const int a = e / d, b = e - a * d;
        double acc = 0.0;
        for (int i = 0; i < d; ++i) {
            const int col = sc.order[i];
            acc = fma(sc.f[i] * V[a * P + col], V[b * P + col], acc);
        }
        out[a * P + b] = acc;
    }
}

// out = X Y, the inner index ascending; no barrier
__device__ inline void matmul(double *out, const double *X, const double *Y, int d, int P) {
    for (int e = threadIdx.x; e < d * d; e += ET) {
        const int a = e / d, b = e - a * d;
        double acc = 0.0;
        for (int k = 0; k < d; ++k) acc = fma(X[a * P + k], Y[k * P + b], acc);
        out[a * P + b] = acc;
    }
}

__global__ void __launch_bounds__(ET) k_sym_eig(const double *__restrict__ A, int d, double *__restrict__ w,
                                                double *__restrict__ V, int32_t *__restrict__ sweeps) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int P = pitch_of(d);
    double *const mA = lds, *const mV = mA + d * P, *const mX = mV + d * P;
    Scratch &sc = *(Scratch *)(mX + d * P);
    const int64_t b = blockIdx.x;
    load_sym(mA, A + b * d * d, d, P);
    const int n = jacobi(mA, mV, mX, d, P, sc);
    const int tid = threadIdx.x;
    if (tid < d) w[b * d + tid] = sc.w[tid];
    if (V)
        for (int e = tid; e < d * d; e += ET) {
            const int k = e / d, i = e - k * d;
            V[b * d * d + e] = mV[k * P + sc.order[i]];
        }
    if (sweeps && tid == 0) sweeps[b] = n;
}

__device__ inline double sqrt_clipped(double w) { return w != w ? w : (w > 0.0 ? sqrt(w) : 0.0); }   // sqrt(np.clip(w, 0, None))

// mean [2, d], cov [2, d, d]: the moments; G [2, d, d]: G[0] = dFD / dcov_f (route 0), G[1] = dFD / dcov_r (route 1), or NULL
__global__ void __launch_bounds__(ET) k_frechet_core(const double *__restrict__ mean, const double *__restrict__ cov, int d,
                                                     double rcond, double *__restrict__ G, double *__restrict__ value,
                                                     double *__restrict__ parts, double *__restrict__ eig,
                                                     int32_t *__restrict__ rank) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int P = pitch_of(d), tid = threadIdx.x, route = blockIdx.x;
    double *const m0 = lds, *const m1 = m0 + d * P, *const m2 = m1 + d * P, *const m3 = m2 + d * P;
    Scratch &sc = *(Scratch *)(m3 + d * P);
    const double *const covA = cov + (int64_t)route * d * d, *const covB = cov + (int64_t)(1 - route) * d * d;

    load_sym(m0, covA, d, P);
    jacobi(m0, m1, m3, d, P, sc);
    if (tid < d) sc.f[tid] = sqrt_clipped(sc.w[tid]);
    __syncthreads();
    spectral(m2, m1, d, P, sc);                  // m2 = S = A^(1/2)
    load_sym(m0, covB, d, P);                    // (its barrier completes S too)
    matmul(m3, m2, m0, d, P);                    // S B
    __syncthreads();
    matmul(m1, m3, m2, d, P);                    // S B S
    __syncthreads();
    for (int e = tid; e < d * d; e += ET) {
        const int i = e / d, j = e - i * d;
        m0[i * P + j] = (m1[i * P + j] + m1[j * P + i]) * 0.5;
    }
    __syncthreads();
    jacobi(m0, m1, m3, d, P, sc);                // m1 = V, sc.w = lambda

    if (tid == 0) {
        const double lmax = sc.w[d - 1];         // (NaN ranks last)
        const double thr = rcond * lmax;
        double trs = 0.0;
        int kept = 0;
        for (int i = 0; i < d; ++i) {
            const double l = sc.w[i];
            trs += sqrt_clipped(l);
            double c = 0.0;
            if (l != l || lmax != lmax) c = l + lmax;            // NaN in, NaN out
            else if (lmax > 0.0 && l > thr) { c = 1.0 / sqrt(l); ++kept; }
            sc.f[i] = c;
        }
        if (route == 0) {
            const double *mr = mean, *mf = mean + d;
            double dm2 = 0.0, tr_r = 0.0, tr_f = 0.0;
            for (int k = 0; k < d; ++k) {
                const double df = mr[k] - mf[k];
                dm2 = fma(df, df, dm2);
                tr_r += cov[(int64_t)k * d + k];
                tr_f += cov[(int64_t)d * d + (int64_t)k * d + k];
            }
            const double fd = ((dm2 + tr_r) + tr_f) - 2.0 * trs;
            value[0] = fd;
            if (parts) { parts[0] = fd; parts[1] = dm2; parts[2] = tr_r; parts[3] = tr_f; parts[4] = trs; }
            if (eig)
                for (int i = 0; i < d; ++i) eig[i] = sc.w[i];
            if (rank) {
                rank[0] = kept;
                if (gridDim.x == 1) rank[1] = -1;
            }
        } else if (rank) {
            rank[1] = kept;
        }
    }
    if (!G) return;
    __syncthreads();
    spectral(m3, m1, d, P, sc);                  // M^(-1/2)_cut
    __syncthreads();
    matmul(m0, m2, m3, d, P);                    // S M^(-1/2)_cut
    __syncthreads();
    double *const Gout = G + (int64_t)route * d * d;
    for (int e = tid; e < d * d; e += ET) {
        const int a = e / d, b = e - a * d;
        double acc = 0.0;
        for (int k = 0; k < d; ++k) acc = fma(m0[a * P + k], m2[k * P + b], acc);
        Gout[e] = (a == b ? 1.0 : 0.0) - acc;
    }
}

// grad[a, :] = (2 / n_s) (mu_s - mu_o) + (2 / (n_s - 1)) G_s (z_a - mu_s) for 64 rows of one sample; zeros for a sample not asked for
__global__ void __launch_bounds__(NT) k_frechet_rows(const double *__restrict__ Z, int64_t n, int d, int64_t nr, int sides,
                                                     const double *__restrict__ mean, const double *__restrict__ G,
                                                     double *__restrict__ grad) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int P = pitch_of(d), tid = threadIdx.x;
    double *const g = lds, *const x = g + d * P, *const mu = x + ROWS * P, *const mt = mu + d;
    const int64_t blocks_r = (nr + ROWS - 1) / ROWS;
    const int side = (int64_t)blockIdx.x < blocks_r ? 0 : 1;
    const int64_t first = side == 0 ? 0 : nr, ns = side == 0 ? nr : n - nr;
    const int64_t r0 = first + ((int64_t)blockIdx.x - (side == 0 ? 0 : blocks_r)) * ROWS;
    const int64_t left = first + ns - r0;
    const int rc = (int)(left < ROWS ? left : ROWS);
    double *const out = grad + r0 * d;
    if (!((sides >> side) & 1)) {
        for (int e = tid; e < rc * d; e += NT) out[e] = 0.0;
        return;
    }
    const double *const Gs = G + (int64_t)(1 - side) * d * d;      // G[1] belongs to the real rows, G[0] to the fake ones
    const double *const ms = mean + side * d, *const mo = mean + (1 - side) * d;
    const double cm = 2.0 / (double)ns, cg = 2.0 / (double)(ns - 1);
    for (int e = tid; e < d * d; e += NT) {
        const int i = e / d, j = e - i * d;
        g[i * P + j] = Gs[e];
    }
    for (int k = tid; k < d; k += NT) {
        mu[k] = ms[k];
        mt[k] = cm * (ms[k] - mo[k]);
    }
    const double *const zin = Z + r0 * d;
    for (int e = tid; e < rc * d; e += NT) {
        const int i = e / d, k = e - i * d;
        x[i * P + k] = zin[e] - ms[k];
    }
    __syncthreads();
    for (int e = tid; e < rc * d; e += NT) {
        const int i = e / d, j = e - i * d;
        double acc = 0.0;
        for (int k = 0; k < d; ++k) acc = fma(g[j * P + k], x[i * P + k], acc);
        out[e] = fma(cg, acc, mt[j]);
    }
}

inline size_t rows_lds_bytes(int d) { return sizeof(double) * ((size_t)(d + ROWS) * pitch_of(d) + 2 * (size_t)d); }

bool frechet_sizes_ok(int64_t n, int64_t d, int64_t n_first) {
    return d >= 1 && n < ((int64_t)1 << 31) && n_first >= 2 && n - n_first >= 2;
}

struct Layout {                                  // of pfm_frechet_grad's workspace
    size_t mean, cov, G, partials, total;
};

Layout layout_of(int64_t n, int64_t d, int64_t n_first) {
    Layout l;
    l.mean = 0;
    l.cov = l.mean + align256(sizeof(double) * 2 * d);
    l.G = l.cov + align256(sizeof(double) * 2 * d * d);
    l.partials = l.G + align256(sizeof(double) * 2 * d * d);
    l.total = l.partials + pf_moments_partial_bytes(n_first, n - n_first, d, 1);
    return l;
}

template <typename K>
int raise_lds(K kernel, size_t bytes) {
    if (bytes > 64 * 1024) PFM_TRY(hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    return PFM_OK;
}

}  // namespace

extern "C" size_t pfm_sym_eig_workspace_bytes(int64_t batch, int64_t d) {
    if (batch < 1 || batch > 65535 || d < 1 || d > MAXD) return 0;
    return 256;
}

extern "C" int pfm_sym_eig(void *stream, const double *A, int64_t batch, int64_t d, double *w, double *V, int32_t *sweeps,
                           void *workspace, size_t workspace_bytes) {
    if (!A || !w || batch < 1 || batch > 65535 || d < 1) return PFM_EINVAL;
    if (d > MAXD) return PFM_EUNSUPPORTED;
    if (!workspace || workspace_bytes < pfm_sym_eig_workspace_bytes(batch, d)) return PFM_EWORKSPACE;
    const size_t lds = lds_bytes((int)d, 3);
    const int st = raise_lds(k_sym_eig, lds);
    if (st != PFM_OK) return st;
    hipLaunchKernelGGL(k_sym_eig, dim3((unsigned)batch), dim3(ET), lds, (hipStream_t)stream, A, (int)d, w, V, sweeps);
    PFM_TRY(hipGetLastError());
    return PFM_OK;
}

extern "C" size_t pfm_frechet_grad_workspace_bytes(int64_t n, int64_t d, int64_t n_first) {
    if (!frechet_sizes_ok(n, d, n_first) || d > MAXD) return 0;
    return layout_of(n, d, n_first).total;
}

extern "C" int pfm_frechet_grad(void *stream, const double *Z, int64_t n, int64_t d, int64_t n_first, double rcond, int sides,
                                double *value, double *grad, double *parts, double *eig, int32_t *rank, void *workspace,
                                size_t workspace_bytes) {
    if (!Z || !value || !frechet_sizes_ok(n, d, n_first) || !(rcond >= 0.0 && rcond < 1.0) || sides < 0 || sides > 3 ||
        (grad && sides == 0))
        return PFM_EINVAL;
    if (d > MAXD) return PFM_EUNSUPPORTED;
    const Layout l = layout_of(n, d, n_first);
    if (!workspace || workspace_bytes < l.total) return PFM_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    char *const base = (char *)workspace;
    double *const mean = (double *)(base + l.mean), *const cov = (double *)(base + l.cov);
    double *const G = grad ? (double *)(base + l.G) : nullptr;
    const int64_t nr = n_first, nf = n - n_first;
    const size_t core_lds = lds_bytes((int)d, 4), rows_lds = rows_lds_bytes((int)d);
    int s = raise_lds(k_frechet_core, core_lds);
    if (s != PFM_OK) return s;
    s = raise_lds(k_frechet_rows, rows_lds);
    if (s != PFM_OK) return s;

    PFM_TRY(pf_moments_enqueue(st, Z, nr, Z + nr * d, nf, d, nullptr, nullptr, 1, mean, cov, base + l.partials));
    const unsigned routes = (grad && (sides & 1)) ? 2u : 1u;
    hipLaunchKernelGGL(k_frechet_core, dim3(routes), dim3(ET), core_lds, st, mean, cov, (int)d, rcond, G, value, parts, eig, rank);
    PFM_TRY(hipGetLastError());
    if (grad) {
        const int64_t blocks = (nr + ROWS - 1) / ROWS + (nf + ROWS - 1) / ROWS;
        hipLaunchKernelGGL(k_frechet_rows, dim3((unsigned)blocks), dim3(NT), rows_lds, st, Z, n, (int)d, nr, sides, mean, G, grad);
        PFM_TRY(hipGetLastError());
    }
    return PFM_OK;
}
