// pf_metrics.hip -- bootstrapped MMD and Frechet-distance moments for gfx950 (C ABI: pf_metrics.h).
//
// Every kernel is batched over bootstrap replicates (grid.y) and gathers the resampled rows through the
// int32 index vectors, so no resampled copy is ever built.  All arithmetic is float64 (the reference runs
// numpy float64); partial sums are reduced in a fixed order with no float atomics, so a call is bitwise
// reproducible.
//
// MMD, per replicate, over the pooled rows Z = [X[idx_x]; Y[idx_y]] (m rows), in 2 + 2 * MMD_PASSES launches:
//   k_mmd_init     state and histograms zeroed; ranks (m*m - 1) / 2 and m*m / 2 of np.median
//   k_mmd_hist     (per digit) sweeps the upper-triangle 64 x 64 tiles of Z: d^2 of every pair i < j from
//                  chunk_d2 of pf_pairtile.h, over the gathered rows (tile_d2_pooled).  The f64 bit pattern of
//                  d^2 >= 0 orders like a uint64: each pair whose key matches the prefix found so far adds
//                  2 (it is (i, j) and (j, i)) to the LDS histogram of the key's next digit; workgroups
//                  flush their histograms with integer atomics (exact, order-free)
//   k_mmd_scan     (per digit) one workgroup per replicate: adds the m diagonal zeros to bucket 0, finds
//                  the bucket holding each of the two middle ranks, extends the prefixes, zeroes the
//                  histograms; after the last digit the prefixes ARE the two order statistics
//   k_mmd_rbf      the same tile sweep and the same tile_d2_pooled, summing exp(-gamma d^2) into XX / YY / XY
//   k_mmd_final    per replicate: the workgroups' partials in order, the three means, mmd
// Two prefixes are tracked because the two middle ranks may part at any digit; while they agree one
// histogram serves both.
//
// Moments (Frechet distance), jobs (replicate, sample), rows split into up to 64 parts per job:
//   k_mean_partial / k_mean_final   column sums per part, then the parts in order / n
//   k_cov_partial / k_cov_final     centred products over row tiles staged in LDS, then the parts in
//                                   order * 1 / (n - 1)  (np.cov multiplies by the reciprocal)
// A null index vector means "row r is row r" (pf_moments.h: the samples as given, for pf_frechet.hip).
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "pf_metrics.h"
#include "pf_moments.h"
#include "pf_pairtile.h"

namespace {

constexpr int MMD_PASSES = 6;      // radix digits of the 64-bit key, most significant first
constexpr int k_shift[MMD_PASSES] = {52, 41, 30, 19, 8, 0};
constexpr int k_width[MMD_PASSES] = {12, 11, 11, 11, 11, 8};
constexpr int MAX_BINS = 4096;     // 1 << max width
constexpr int64_t MMD_TARGET_WG = 3072;        // workgroups per launch worth aiming for (256 CUs, a few per CU)
constexpr int64_t MMD_MAX_TILES_PER_WG = 65536; // keeps a workgroup's LDS counts < 2^32 (65536 * 4096 pairs * 2)
constexpr int64_t ROWS_PER_PART = 2048;         // moments: rows per workgroup (at most MAX_PARTS parts)
constexpr int64_t MAX_PARTS = 64;
constexpr int LDS_ROW_DOUBLES = 4096;           // moments: the centred row tile, 32 KB

struct MmdState {
    uint64_t pref[2];    // key prefix of the rank (m*m-1)/2 and m*m/2 order statistics
    uint64_t rank[2];    // remaining rank inside the prefix
    double median, gamma;
    int32_t same;        // pref[0] == pref[1]: one histogram serves both
    int32_t pad[3];
};

inline int64_t mmd_wg_per_rep(int64_t m, int64_t reps) {
    int64_t T = triangle_tiles(m);
    int64_t w = (MMD_TARGET_WG + reps - 1) / reps;
    if (w > T) w = T;
    int64_t wmin = (T + MMD_MAX_TILES_PER_WG - 1) / MMD_MAX_TILES_PER_WG;
    if (w < wmin) w = wmin;
    return w < 1 ? 1 : w;
}

inline int64_t parts_of(int64_t n) {
    int64_t p = (n + ROWS_PER_PART - 1) / ROWS_PER_PART;
    return p < 1 ? 1 : (p > MAX_PARTS ? MAX_PARTS : p);
}

struct Pooled {                      // one replicate's pooled sample Z = [X[ix]; Y[iy]]: a row source of pf_pairtile.h
    const double *X, *Y;
    const int32_t *ix, *iy;
    int64_t nx, n, d;
    __device__ const double *row(int64_t r) const {
        return r < nx ? X + (int64_t)ix[r] * d : Y + (int64_t)iy[r - nx] * d;
    }
};

// tile_d2 of pf_pairtile.h for tile (bi, bj) of one pooled sample, with the two sides staged in ONE loop (both gathers of an
// element are in flight together).  As two stage() calls k_mmd_hist and k_mmd_rbf measured 6 % slower at 20 000 pooled rows,
// d = 16 (profiles/r19_pairtile_time.txt), so the MMD kernels keep this loop; the arithmetic is chunk_d2's, the same as everywhere.
__device__ inline void tile_d2_pooled(const Pooled &z, int64_t bi, int64_t bj, double (*sA)[TPAD], double (*sB)[TPAD],
                                      double acc[4][4]) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = 0.0;
    const int64_t I0 = bi * TILE, J0 = bj * TILE;
    for (int64_t k0 = 0; k0 < z.d; k0 += DC) {
        const int dc = (int)((z.d - k0) < DC ? (z.d - k0) : DC);
        __syncthreads();                               // the previous chunk's reads are done
        for (int e = tid; e < TILE * dc; e += NT) {
            const int row = e / dc, col = e - row * dc;
            const int64_t gi = I0 + row, gj = J0 + row;
            sA[col][row] = gi < z.n ? z.row(gi)[k0 + col] : 0.0;
            sB[col][row] = gj < z.n ? z.row(gj)[k0 + col] : 0.0;
        }
        __syncthreads();
        chunk_d2(sA, sB, dc, acc);
    }
}

__device__ inline Pooled pooled(const double *X, int64_t nx, const double *Y, int64_t ny, int64_t d,
                                const int32_t *idx_x, const int32_t *idx_y, int64_t rep) {
    Pooled z;
    z.X = X; z.Y = Y; z.ix = idx_x + rep * nx; z.iy = idx_y + rep * ny;
    z.nx = nx; z.n = nx + ny; z.d = d;
    return z;
}

__global__ void k_mmd_init(MmdState *st, unsigned long long *hist, int64_t reps, int64_t m) {
    const int64_t total = reps * 2 * MAX_BINS;
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < total; i += (int64_t)gridDim.x * NT) hist[i] = 0ull;
    const int64_t r = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (r < reps) {
        const uint64_t M = (uint64_t)m * (uint64_t)m;
        MmdState s = {};
        s.pref[0] = s.pref[1] = 0ull;
        s.rank[0] = (M - 1) / 2;
        s.rank[1] = M / 2;
        s.same = 1;
        st[r] = s;
    }
}

__global__ void __launch_bounds__(NT) k_mmd_hist(const double *X, int64_t nx, const double *Y, int64_t ny, int64_t d,
                                                 const int32_t *idx_x, const int32_t *idx_y, const MmdState *st,
                                                 unsigned long long *hist, int shift, int width) {
    __shared__ uint32_t hA[MAX_BINS], hB[MAX_BINS];
    __shared__ double sA[DC][TPAD], sB[DC][TPAD];
    const int64_t rep = blockIdx.y;
    const Pooled z = pooled(X, nx, Y, ny, d, idx_x, idx_y, rep);
    const int nbins = 1 << width, tid = threadIdx.x, ti = tid >> 4, tj = tid & 15;
    const uint64_t hi_mask = (shift + width >= 64) ? 0ull : (~0ull << (shift + width));
    const uint64_t bmask = (uint64_t)nbins - 1;
    const uint64_t pA = st[rep].pref[0], pB = st[rep].pref[1];
    const bool same = st[rep].same != 0;
    for (int b = tid; b < nbins; b += NT) { hA[b] = 0u; hB[b] = 0u; }
    // (tile_d2_pooled begins with a barrier, which also orders these zero stores before the first count)
    const int64_t T = triangle_tiles(z.n);
    for (int64_t t = blockIdx.x; t < T; t += gridDim.x) {
        int64_t bi, bj;
        tile_decode(t, bi, bj);
        double acc[4][4];
        tile_d2_pooled(z, bi, bj, sA, sB, acc);
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int64_t gi = bi * TILE + ti + 16 * a, gj = bj * TILE + tj + 16 * b;
                if (gi < z.n && gj < z.n && gi < gj) {
                    const uint64_t key = (uint64_t)__double_as_longlong(acc[a][b]);
                    const uint32_t dig = (uint32_t)((key >> shift) & bmask);
                    if ((key & hi_mask) == pA) atomicAdd(&hA[dig], 2u);
                    if (!same && (key & hi_mask) == pB) atomicAdd(&hB[dig], 2u);
                }
            }
    }
    __syncthreads();
    unsigned long long *gA = hist + (rep * 2) * MAX_BINS, *gB = gA + MAX_BINS;
    for (int b = tid; b < nbins; b += NT) {
        if (hA[b]) atomicAdd(&gA[b], (unsigned long long)hA[b]);
        if (hB[b]) atomicAdd(&gB[b], (unsigned long long)hB[b]);
    }
}

__global__ void __launch_bounds__(NT) k_mmd_scan(MmdState *st, unsigned long long *hist, int64_t m, int shift, int width,
                                                 int last) {
    __shared__ unsigned long long part[NT];
    __shared__ int64_t found_t;
    __shared__ unsigned long long found_before;
    const int64_t rep = blockIdx.x;
    const int tid = threadIdx.x, nbins = 1 << width, per = nbins / NT;   // width >= 8: per >= 1
    MmdState s = st[rep];
    unsigned long long *gA = hist + (rep * 2) * MAX_BINS;
    for (int w = 0; w < 2; ++w) {
        const unsigned long long *h = (w == 1 && !s.same) ? gA + MAX_BINS : gA;
        // the m diagonal zeros: key 0, counted where the prefix admits it (all-zero prefix)
        const unsigned long long diag = (s.pref[w] == 0ull) ? (unsigned long long)m : 0ull;
        unsigned long long sum = 0;
        for (int i = 0; i < per; ++i) sum += h[tid * per + i] + (tid == 0 && i == 0 ? diag : 0ull);
        part[tid] = sum;
        __syncthreads();
        if (tid == 0) {
            unsigned long long cum = 0;
            int64_t t = NT - 1;
            for (int i = 0; i < NT; ++i) {
                if (s.rank[w] < cum + part[i]) { t = i; break; }
                cum += part[i];
            }
            found_t = t;
            found_before = cum;
        }
        __syncthreads();
        if (tid == 0) {
            unsigned long long cum = found_before;
            const int64_t t = found_t;
            int bucket = (int)(t * per + per - 1);
            for (int i = 0; i < per; ++i) {
                const unsigned long long c = h[t * per + i] + (t == 0 && i == 0 ? diag : 0ull);
                if (s.rank[w] < cum + c) { bucket = (int)(t * per + i); break; }
                cum += c;
            }
            s.pref[w] |= (uint64_t)bucket << shift;
            s.rank[w] -= cum;
        }
        __syncthreads();
    }
    for (int b = tid; b < 2 * nbins; b += NT) gA[(b < nbins ? 0 : MAX_BINS) + (b % nbins)] = 0ull;
    if (tid == 0) {
        s.same = s.pref[0] == s.pref[1];
        if (last) {
            const double a = sqrt(__longlong_as_double((long long)s.pref[0]));
            const double b = sqrt(__longlong_as_double((long long)s.pref[1]));
            const uint64_t M = (uint64_t)m * (uint64_t)m;
            s.median = (M & 1ull) ? a : (a + b) / 2.0;       // np.median: the mean of the two middle values
            s.gamma = 1.0 / (2.0 * (s.median * s.median));
        }
        st[rep] = s;
    }
}

__global__ void __launch_bounds__(NT) k_mmd_rbf(const double *X, int64_t nx, const double *Y, int64_t ny, int64_t d,
                                                const int32_t *idx_x, const int32_t *idx_y, const MmdState *st,
                                                double *partials) {
    __shared__ double sA[DC][TPAD], sB[DC][TPAD];
    __shared__ double red[3][NT];
    const int64_t rep = blockIdx.y;
    const Pooled z = pooled(X, nx, Y, ny, d, idx_x, idx_y, rep);
    const int tid = threadIdx.x, ti = tid >> 4, tj = tid & 15;
    const double gamma = st[rep].gamma;
    const bool skip = !(st[rep].median > 0.0);              // median 0: the caller raises, no point in the sweep
    double sxx = 0.0, syy = 0.0, sxy = 0.0;
    const int64_t T = skip ? 0 : triangle_tiles(z.n);
    for (int64_t t = blockIdx.x; t < T; t += gridDim.x) {
        int64_t bi, bj;
        tile_decode(t, bi, bj);
        double acc[4][4];
        tile_d2_pooled(z, bi, bj, sA, sB, acc);
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int64_t gi = bi * TILE + ti + 16 * a, gj = bj * TILE + tj + 16 * b;
                if (gi < z.n && gj < z.n && gi < gj) {
                    const double k = exp(acc[a][b] * -gamma);   // rbf_kernel: K *= -gamma; np.exp(K)
                    if (gi >= nx) syy += k;                     // gi < gj: both in Y
                    else if (gj < nx) sxx += k;
                    else sxy += k;
                }
            }
    }
    red[0][tid] = sxx; red[1][tid] = syy; red[2][tid] = sxy;
    __syncthreads();
    for (int s = NT / 2; s > 0; s >>= 1) {
        if (tid < s) {
            red[0][tid] += red[0][tid + s];
            red[1][tid] += red[1][tid + s];
            red[2][tid] += red[2][tid + s];
        }
        __syncthreads();
    }
    if (tid < 3) partials[(rep * gridDim.x + blockIdx.x) * 3 + tid] = red[tid][0];
}

__global__ void k_mmd_final(const MmdState *st, const double *partials, int64_t wg, int64_t reps, int64_t nx, int64_t ny,
                            double *median, double *mmd) {
    const int64_t rep = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (rep >= reps) return;
    double sxx = 0.0, syy = 0.0, sxy = 0.0;
    for (int64_t w = 0; w < wg; ++w) {
        const double *p = partials + (rep * wg + w) * 3;
        sxx += p[0]; syy += p[1]; sxy += p[2];
    }
    const double fx = (double)nx, fy = (double)ny;
    // off-diagonal pairs were summed once per i < j: twice in the full matrix; the diagonal is exp(0) = 1
    const double mxx = ((double)nx + 2.0 * sxx) / (fx * fx);
    const double myy = ((double)ny + 2.0 * syy) / (fy * fy);
    const double mxy = sxy / (fx * fy);
    const double med = st[rep].median;
    median[rep] = med;
    mmd[rep] = med > 0.0 ? mxx + myy - 2.0 * mxy : __longlong_as_double(0x7ff8000000000000ll);
}

// ---- moments ------------------------------------------------------------------------------------------

struct Job {
    const double *X;
    const int32_t *idx;              // NULL: the rows as given
    int64_t n;
    __device__ int64_t src(int64_t r) const { return idx ? (int64_t)idx[r] : r; }
};

__device__ inline Job job_of(const double *Xr, int64_t nr, const double *Xf, int64_t nf, const int32_t *idx_r,
                             const int32_t *idx_f, int64_t j) {
    const int64_t rep = j >> 1;
    Job b;
    if ((j & 1) == 0) { b.X = Xr; b.idx = idx_r ? idx_r + rep * nr : nullptr; b.n = nr; }
    else { b.X = Xf; b.idx = idx_f ? idx_f + rep * nf : nullptr; b.n = nf; }
    return b;
}

__device__ inline int64_t dev_parts(int64_t n) {
    int64_t p = (n + ROWS_PER_PART - 1) / ROWS_PER_PART;
    return p < 1 ? 1 : (p > MAX_PARTS ? MAX_PARTS : p);
}

__global__ void __launch_bounds__(NT) k_mean_partial(const double *Xr, int64_t nr, const double *Xf, int64_t nf, int64_t d,
                                                     const int32_t *idx_r, const int32_t *idx_f, double *part,
                                                     int64_t pmax) {
    __shared__ double red[NT];
    const int64_t j = blockIdx.y, p = blockIdx.x;
    const Job b = job_of(Xr, nr, Xf, nf, idx_r, idx_f, j);
    const int64_t P = dev_parts(b.n);
    if (p >= P) return;
    const int64_t r0 = b.n * p / P, r1 = b.n * (p + 1) / P;
    const int tid = threadIdx.x;
    const int F = (int)(d < NT ? d : NT), lanes = NT / F;
    for (int64_t k0 = 0; k0 < d; k0 += F) {
        const int fk = (int)((d - k0) < F ? (d - k0) : F);
        const int kk = tid % F, lane = tid / F;
        double acc = 0.0;
        if (lane < lanes && kk < fk)
            for (int64_t r = r0 + lane; r < r1; r += lanes) acc += b.X[b.src(r) * d + k0 + kk];
        red[tid] = acc;
        __syncthreads();
        if (tid < fk) {
            double s = 0.0;
            for (int l = 0; l < lanes; ++l) s += red[l * F + tid];
            part[(j * pmax + p) * d + k0 + tid] = s;
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(NT) k_mean_final(const double *part, int64_t pmax, int64_t nr, int64_t nf, int64_t d,
                                                   double *mean) {
    const int64_t j = blockIdx.x;
    const int64_t n = (j & 1) ? nf : nr, P = dev_parts(n);
    for (int64_t k = threadIdx.x; k < d; k += NT) {
        double s = 0.0;
        for (int64_t p = 0; p < P; ++p) s += part[(j * pmax + p) * d + k];
        mean[j * d + k] = s / (double)n;
    }
}

__device__ inline void pair_decode(int64_t t, int64_t &k, int64_t &l) {   // t -> (k <= l), l-major
    int64_t r = (int64_t)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
    while (r * (r + 1) / 2 > t) --r;
    while ((r + 1) * (r + 2) / 2 <= t) ++r;
    l = r;
    k = t - r * (r + 1) / 2;
}

__global__ void __launch_bounds__(NT) k_cov_partial(const double *Xr, int64_t nr, const double *Xf, int64_t nf, int64_t d,
                                                    const int32_t *idx_r, const int32_t *idx_f, const double *mean,
                                                    double *cpart, int64_t pmax) {
    __shared__ double rows[LDS_ROW_DOUBLES];
    __shared__ double red[NT];
    const int64_t j = blockIdx.y, p = blockIdx.x;
    const Job b = job_of(Xr, nr, Xf, nf, idx_r, idx_f, j);
    const int64_t P = dev_parts(b.n);
    if (p >= P) return;
    const int64_t r0 = b.n * p / P, r1 = b.n * (p + 1) / P;
    const int tid = threadIdx.x;
    const int64_t npair = d * (d + 1) / 2;
    const int PG = (int)(npair < NT ? npair : NT), lanes = NT / PG;
    const int64_t RT = (LDS_ROW_DOUBLES / d) < 64 ? (LDS_ROW_DOUBLES / d) : 64;   // d <= 4096: RT >= 1
    const double *mu = mean + j * d;
    for (int64_t g0 = 0; g0 < npair; g0 += PG) {
        const int64_t pi = g0 + tid % PG;
        const int lane = tid / PG;
        const bool active = lane < lanes && pi < npair;
        int64_t k = 0, l = 0;
        if (active) pair_decode(pi, k, l);
        double acc = 0.0;
        for (int64_t c0 = r0; c0 < r1; c0 += RT) {
            const int64_t rc = (r1 - c0) < RT ? (r1 - c0) : RT;
            __syncthreads();
            for (int64_t e = tid; e < rc * d; e += NT) {
                const int64_t rr = e / d, kk = e - rr * d;
                rows[e] = b.X[b.src(c0 + rr) * d + kk] - mu[kk];
            }
            __syncthreads();
            if (active)
                for (int64_t rr = lane; rr < rc; rr += lanes) acc = fma(rows[rr * d + k], rows[rr * d + l], acc);
        }
        red[tid] = acc;
        __syncthreads();
        if (tid < PG && g0 + tid < npair) {
            double s = 0.0;
            for (int q = 0; q < lanes; ++q) s += red[q * PG + tid];
            cpart[(j * pmax + p) * npair + g0 + tid] = s;
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(NT) k_cov_final(const double *cpart, int64_t pmax, int64_t nr, int64_t nf, int64_t d,
                                                  double *cov) {
    const int64_t j = blockIdx.x;
    const int64_t n = (j & 1) ? nf : nr, P = dev_parts(n);
    const int64_t npair = d * (d + 1) / 2;
    const double inv = 1.0 / (double)(n - 1);             // np.cov: c *= np.true_divide(1, fact)
    double *c = cov + j * d * d;
    for (int64_t t = threadIdx.x; t < npair; t += NT) {
        double s = 0.0;
        for (int64_t p = 0; p < P; ++p) s += cpart[(j * pmax + p) * npair + t];
        int64_t k, l;
        pair_decode(t, k, l);
        const double v = s * inv;
        c[k * d + l] = v;
        c[l * d + k] = v;
    }
}

}  // namespace

// ---- C ABI --------------------------------------------------------------------------------------------

extern "C" int pfm_version(void) { return PFM_VERSION; }

extern "C" const char *pfm_status_string(int status) {
    switch (status) {
        case PFM_OK: return "ok";
        case PFM_EINVAL: return "invalid argument (NULL pointer or size)";
        case PFM_EUNSUPPORTED: return "more features than the moments kernels' LDS row tile holds";
        case PFM_EWORKSPACE: return "workspace missing or smaller than the *_workspace_bytes() query says";
        default: return status > 0 ? hipGetErrorString((hipError_t)status) : "unknown status";
    }
}

static bool mmd_args_ok(int64_t nx, int64_t ny, int64_t d, int64_t reps) {
    return nx >= 1 && ny >= 1 && d >= 1 && reps >= 1 && reps <= 65535 && nx + ny <= (int64_t)INT32_MAX;
}

extern "C" size_t pfm_mmd_workspace_bytes(int64_t nx, int64_t ny, int64_t d, int64_t reps) {
    if (!mmd_args_ok(nx, ny, d, reps)) return 0;
    const int64_t wg = mmd_wg_per_rep(nx + ny, reps);
    return align256(sizeof(MmdState) * reps) + align256(sizeof(unsigned long long) * 2 * MAX_BINS * reps) +
           align256(sizeof(double) * 3 * wg * reps);
}

extern "C" int pfm_mmd(void *stream, const double *X, int64_t nx, const double *Y, int64_t ny, int64_t d,
                       const int32_t *idx_x, const int32_t *idx_y, int64_t reps, double *median, double *mmd,
                       void *workspace, size_t workspace_bytes) {
    if (!X || !Y || !idx_x || !idx_y || !median || !mmd || !mmd_args_ok(nx, ny, d, reps)) return PFM_EINVAL;
    const size_t need = pfm_mmd_workspace_bytes(nx, ny, d, reps);
    if (!workspace || workspace_bytes < need) return PFM_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int64_t m = nx + ny, wg = mmd_wg_per_rep(m, reps);
    char *w = (char *)workspace;
    MmdState *state = (MmdState *)w;
    w += align256(sizeof(MmdState) * reps);
    unsigned long long *hist = (unsigned long long *)w;
    w += align256(sizeof(unsigned long long) * 2 * MAX_BINS * reps);
    double *partials = (double *)w;

    const int64_t init_blocks = (reps * 2 * MAX_BINS + NT - 1) / NT;
    hipLaunchKernelGGL(k_mmd_init, dim3((unsigned)init_blocks), dim3(NT), 0, st, state, hist, reps, m);
    PFM_TRY(hipGetLastError());
    const dim3 grid((unsigned)wg, (unsigned)reps);
    for (int p = 0; p < MMD_PASSES; ++p) {
        hipLaunchKernelGGL(k_mmd_hist, grid, dim3(NT), 0, st, X, nx, Y, ny, d, idx_x, idx_y, state, hist, k_shift[p],
                           k_width[p]);
        PFM_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_mmd_scan, dim3((unsigned)reps), dim3(NT), 0, st, state, hist, m, k_shift[p], k_width[p],
                           p == MMD_PASSES - 1 ? 1 : 0);
        PFM_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(k_mmd_rbf, grid, dim3(NT), 0, st, X, nx, Y, ny, d, idx_x, idx_y, state, partials);
    PFM_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_mmd_final, dim3((unsigned)((reps + 63) / 64)), dim3(64), 0, st, state, partials, wg, reps, nx, ny,
                       median, mmd);
    PFM_TRY(hipGetLastError());
    return PFM_OK;
}

static bool mom_args_ok(int64_t nr, int64_t nf, int64_t d, int64_t reps) {
    return nr >= 1 && nf >= 1 && d >= 1 && reps >= 1 && 2 * reps <= 65535;
}

size_t pf_moments_partial_bytes(int64_t nr, int64_t nf, int64_t d, int64_t reps) {
    const int64_t pmax = parts_of(nr > nf ? nr : nf), jobs = 2 * reps;
    return align256(sizeof(double) * jobs * pmax * d) + align256(sizeof(double) * jobs * pmax * (d * (d + 1) / 2));
}

hipError_t pf_moments_enqueue(hipStream_t st, const double *Xr, int64_t nr, const double *Xf, int64_t nf, int64_t d,
                              const int32_t *idx_r, const int32_t *idx_f, int64_t reps, double *mean, double *cov,
                              void *partials) {
    const int64_t pmax = parts_of(nr > nf ? nr : nf), jobs = 2 * reps;
    double *mpart = (double *)partials;
    double *cpart = (double *)((char *)partials + align256(sizeof(double) * jobs * pmax * d));
    const dim3 grid((unsigned)pmax, (unsigned)jobs);
    hipError_t e;
    hipLaunchKernelGGL(k_mean_partial, grid, dim3(NT), 0, st, Xr, nr, Xf, nf, d, idx_r, idx_f, mpart, pmax);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_mean_final, dim3((unsigned)jobs), dim3(NT), 0, st, mpart, pmax, nr, nf, d, mean);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_cov_partial, grid, dim3(NT), 0, st, Xr, nr, Xf, nf, d, idx_r, idx_f, mean, cpart, pmax);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_cov_final, dim3((unsigned)jobs), dim3(NT), 0, st, cpart, pmax, nr, nf, d, cov);
    return hipGetLastError();
}

extern "C" size_t pfm_moments_workspace_bytes(int64_t nr, int64_t nf, int64_t d, int64_t reps) {
    if (!mom_args_ok(nr, nf, d, reps) || d > PFM_MOMENTS_MAX_D) return 0;
    return pf_moments_partial_bytes(nr, nf, d, reps);
}

extern "C" int pfm_boot_moments(void *stream, const double *Xr, int64_t nr, const double *Xf, int64_t nf, int64_t d,
                                const int32_t *idx_r, const int32_t *idx_f, int64_t reps, double *mean, double *cov,
                                void *workspace, size_t workspace_bytes) {
    if (!Xr || !Xf || !idx_r || !idx_f || !mean || !cov || !mom_args_ok(nr, nf, d, reps)) return PFM_EINVAL;
    if (d > PFM_MOMENTS_MAX_D) return PFM_EUNSUPPORTED;
    const size_t need = pfm_moments_workspace_bytes(nr, nf, d, reps);
    if (!workspace || workspace_bytes < need) return PFM_EWORKSPACE;
    PFM_TRY(pf_moments_enqueue((hipStream_t)stream, Xr, nr, Xf, nf, d, idx_r, idx_f, reps, mean, cov, workspace));
    return PFM_OK;
}
