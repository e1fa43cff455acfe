// pf_slicegrad.hip -- the sliced Wasserstein distance of the samples as given TOGETHER WITH its derivative by every row, for
// training on it, for gfx950 (C ABI: pf_metrics.h, pfm_slice_grad).
//
// Pool Z = [first sample; second sample] (n = nr + nf rows), directions theta_k, k < P.  Per direction the two samples' projections
// are sorted by (value, pooled row index) and coupled by quantiles: on the integer grid of nr nf cells sorted real element i covers
// [i nf, (i + 1) nf) and sorted fake element j covers [j nr, (j + 1) nr); the weights are uniform, so the breakpoints are arithmetic
// and nobody searches (k_wp of pf_wasserstein.hip, whose replicates are weighted, must).  Four kernels and a sort:
//   k_slice_project  the projections of every pooled row on every direction, into the workspace: a kernel of its own, so that all
//                    CUs read the rows, staged through LDS.
//   k_slice_sort     grid (P, 2), one workgroup per direction and sample: the sample's projections go into LDS as (float64 value,
//                    int32 row) and are sorted there by a bitonic network in the form whose compare-exchanges all point the same
//                    way (the first step of a merge pairs i with i ^ (2 m - 1), the others i with i ^ m).  Positions >= n then
//                    behave as +infinity without being stored: a pair whose upper position is >= n is skipped, so n need not be a
//                    power of two.  The network is data-oblivious: NaN cannot make it loop or index out of range.  12 bytes per
//                    entry in 160 KiB of LDS: PFM_SLICE_LDS_ROWS rows per sample.
//   k_slice_given    the caller's order instead (perm_in): the projections of the rows in that order, any n.
//   k_slice_couple   one thread per sorted real element and one per sorted fake element; each walks its own range of partners in
//                    ascending order, so it writes the derivative by its row's projection exactly once, through the permutation.
//                    The real side also adds the value's terms; a workgroup's are summed by block_sum (pf_scan1d.h).
//   k_slice_finish   rows[a, :] = (1 / P) sum_k g_k[a] theta_k with k ascending, and the value from the workgroups' partials.
// No float atomics; every sum's order depends on (nr, nf, P) only and every workspace byte read was written by the same call, so
// the outputs are bitwise the same in any call.  The projection is k_project's: the sum starts at 0 and runs over the features in
// order, product and sum rounded separately (-ffp-contract=off, Makefile).
#include <hip/hip_runtime.h>

#include <atomic>
#include <math.h>
#include <stdint.h>

#include "pf_common.h"
#include "pf_metrics.h"
#include "pf_scan1d.h"

namespace {

constexpr int SORT_NT = 1024;                        // threads of a sort workgroup: a stage has up to 8192 compare-exchanges
constexpr int64_t LDS_ROWS = PFM_SLICE_LDS_ROWS;
static_assert(LDS_ROWS * 12 <= 160 * 1024, "a sample's (value, row) pairs must fit the LDS of one CU");
static_assert(LDS_ROWS % 2 == 0, "the rows follow the values: keep them 8-byte aligned");

// u = sum_j z[j] th[j] as k_project forms it; th == NULL: feature k itself, copied
__device__ inline double project_row(const double *z, const double *th, int64_t d, int64_t k) {
    if (!th) return z[k];
    double acc = 0.0;
    for (int64_t j = 0; j < d; ++j) {
        const double prod = z[j] * th[j];
        acc = acc + prod;
    }
    return acc;
}

// the sort route's projections, unsorted, into vals [P, N] (and cols_out): a workgroup takes NT pooled rows and KC directions.  The
// rows' features are staged through LDS in chunks of PDC, read coalesced and stored feature-major, so that thread a reads feature
// c of ITS row without a bank conflict; it carries KC sums, each over the features in order as project_row forms it.  theta is
// uniform over the workgroup.  (One thread per row and direction reading its row from global memory, as k_project does, was
// measured first: 90 us at 10 000 rows per sample, d = 16, P = 64, a third of the call.)
constexpr int KC = 8;            // directions per workgroup
constexpr int PDC = 16;          // features staged per chunk
__global__ void __launch_bounds__(NT) k_slice_project(const double *__restrict__ Z, int64_t N, int64_t d,
                                                      const double *__restrict__ theta, int64_t P, double *__restrict__ vals,
                                                      double *__restrict__ cols_out) {
    __shared__ double tile[PDC][NT + 1];
    const int tid = threadIdx.x;
    const int64_t a0 = (int64_t)blockIdx.x * NT, a = a0 + tid, k0 = (int64_t)blockIdx.y * KC;
    const int rows = (int)(N - a0 < NT ? N - a0 : NT);
    if (!theta) {                                     // the coordinate axes: column k is feature k, copied
        if (a < N)
            for (int64_t k = k0; k < k0 + KC && k < P; ++k) {
                const double u = Z[a * d + k];
                vals[k * N + a] = u;
                if (cols_out) cols_out[k * N + a] = u;
            }
        return;
    }
    double acc[KC];
#pragma unroll
    for (int q = 0; q < KC; ++q) acc[q] = 0.0;
    for (int64_t j0 = 0; j0 < d; j0 += PDC) {
        const int dc = (int)(d - j0 < PDC ? d - j0 : PDC);
        __syncthreads();                              // the previous chunk's reads are done
        for (int e = tid; e < rows * dc; e += NT) {
            const int r = e / dc, c = e - r * dc;
            tile[c][r] = Z[(a0 + r) * d + j0 + c];
        }
        __syncthreads();
        for (int c = 0; c < dc; ++c) {
            const double z = tile[c][tid];            // threads past the last row read what is there and store nothing
#pragma unroll
            for (int q = 0; q < KC; ++q) {
                const int64_t k = k0 + q < P ? k0 + q : P - 1;
                const double prod = z * theta[k * d + j0 + c];
                acc[q] = acc[q] + prod;
            }
        }
    }
    if (a < N)
#pragma unroll
        for (int q = 0; q < KC; ++q)
            if (k0 + q < P) {
                vals[(k0 + q) * N + a] = acc[q];
                if (cols_out) cols_out[(k0 + q) * N + a] = acc[q];
            }
}

// vals [P, N] holds the projections on the pooled rows; on return each sample's segment holds them sorted, perm their rows
__global__ void __launch_bounds__(SORT_NT) k_slice_sort(int64_t N, int64_t nr, int lds_rows, double *__restrict__ vals,
                                                        int32_t *__restrict__ perm, int32_t *__restrict__ perm_out) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    double *const sv = lds;                           // [lds_rows] values
    int32_t *const si = (int32_t *)(lds + lds_rows);  // [lds_rows] pooled rows
    const int64_t k = blockIdx.x;
    const int tid = threadIdx.x;
    const int off = blockIdx.y == 0 ? 0 : (int)nr;
    const int n = blockIdx.y == 0 ? (int)nr : (int)(N - nr);      // <= lds_rows: the host checked

    for (int a = tid; a < n; a += SORT_NT) {
        sv[a] = vals[k * N + off + a];
        si[a] = off + a;
    }
    __syncthreads();

    int npad = 1;
    while (npad < n) npad <<= 1;
    const int half = npad >> 1;
    for (int m = 2; m <= npad; m <<= 1) {
        for (int j = m >> 1; j > 0; j >>= 1) {
            const int flip = j == (m >> 1) ? m - 1 : j;           // the merge's first step mirrors, the others shift
            for (int t = tid; t < half; t += SORT_NT) {
                const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                const int hi = lo ^ flip;                          // hi > lo
                if (lo >= n) break;                                // lo grows with t
                if (hi < n) {                                      // hi >= n: +infinity stays above
                    const double a = sv[lo], b = sv[hi];
                    const int32_t ia = si[lo], ib = si[hi];
                    if (a > b || (a == b && ia > ib)) {
                        sv[lo] = b;
                        sv[hi] = a;
                        si[lo] = ib;
                        si[hi] = ia;
                    }
                }
            }
            __syncthreads();
        }
    }

    for (int a = tid; a < n; a += SORT_NT) {
        const int64_t e = k * N + off + a;
        vals[e] = sv[a];
        perm[e] = si[a];
        if (perm_out) perm_out[e] = si[a];
    }
}

// the caller's order: vals[k, pos] = the projection of row perm_in[k, pos] (entries are clamped to [0, N))
__global__ void __launch_bounds__(NT) k_slice_given(const double *__restrict__ Z, int64_t N, int64_t d,
                                                    const double *__restrict__ theta, const int32_t *__restrict__ perm_in,
                                                    double *__restrict__ vals, double *__restrict__ cols_out,
                                                    int32_t *__restrict__ perm_out) {
    const int64_t k = blockIdx.y, pos = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (pos >= N) return;
    const int64_t e = k * N + pos;
    int64_t row = perm_in[e];
    row = row < 0 ? 0 : row >= N ? N - 1 : row;       // a permutation is the caller's duty; no entry leaves the sample
    const double u = project_row(Z + row * d, theta ? theta + k * d : nullptr, d, k);
    vals[e] = u;
    if (cols_out) cols_out[k * N + row] = u;
    if (perm_out) perm_out[e] = (int32_t)row;
}

template <int P>
__device__ inline void pair_term(double diff, double ov, double &val, double &g) {
    if (P == 1) {
        val = val + ov * fabs(diff);
        g = g + ov * (double)((diff > 0.0) - (diff < 0.0));       // exactly 0 on a coincidence
    } else {
        val = val + ov * (diff * diff);
        g = g + ov * (2.0 * diff);
    }
}

// thread t < nr: sorted real element i = t against fake j = (i nf) div nr .. ((i + 1) nf - 1) div nr; thread t >= nr: sorted fake
// element j = t - nr against real i = (j nr) div nf .. ((j + 1) nr - 1) div nf.  All products fit int64: nr nf < 2^62.
template <int P>
__global__ void __launch_bounds__(NT) k_slice_couple(const double *__restrict__ vals, const int32_t *__restrict__ perm,
                                                     int64_t nr, int64_t nf, double inv_cells, double *__restrict__ g,
                                                     double *__restrict__ partial) {
    __shared__ double sd[NT];
    const int64_t N = nr + nf, k = blockIdx.y, t = (int64_t)blockIdx.x * NT + threadIdx.x;
    const double *us = vals + k * N, *vs = us + nr;
    double val = 0.0;
    if (t < N) {
        const bool real = t < nr;
        const int64_t e = real ? t : t - nr;
        const int64_t mine = real ? nf : nr, other = real ? nr : nf;      // my cells per element, the partner's
        const double *pv = real ? vs : us;
        const double x = real ? us[e] : vs[e];
        const int64_t lo = e * mine, hi = lo + mine;
        const int64_t q0 = lo / other, q1 = (hi - 1) / other;
        double acc = 0.0;
        for (int64_t q = q0; q <= q1; ++q) {
            const int64_t a = q * other, b = a + other;
            const int64_t ov = (b < hi ? b : hi) - (a > lo ? a : lo);
            pair_term<P>(real ? x - pv[q] : pv[q] - x, (double)ov, val, acc);
        }
        if (g) {
            int64_t row = perm[k * N + t];
            row = row < 0 ? 0 : row >= N ? N - 1 : row;                  // as k_slice_given
            g[k * N + row] = (real ? acc : -acc) * inv_cells;
        }
        if (!real) val = 0.0;                                            // every pair's value term is the real side's
    }
    const double s = block_sum(val, sd);
    if (threadIdx.x == 0) partial[k * gridDim.x + blockIdx.x] = s;
}

// workgroups 0 .. gridDim.x - 2 (none for the value alone): element e = a d + j of rows; the last one: the value
__global__ void __launch_bounds__(NT) k_slice_finish(const double *__restrict__ g, const double *__restrict__ theta, int64_t N,
                                                     int64_t d, int64_t P, const double *__restrict__ partial,
                                                     int64_t n_partial, double inv_cells, double *__restrict__ value,
                                                     double *__restrict__ rows) {
    __shared__ double sd[NT];
    const int tid = threadIdx.x;
    if (blockIdx.x + 1 < gridDim.x) {
        const int64_t e = (int64_t)blockIdx.x * NT + tid;
        if (e < N * d) {
            const int64_t a = e / d, j = e - a * d;
            double acc;
            if (!theta) {
                acc = g[j * N + a];
            } else {
                acc = 0.0;
#pragma unroll 8                                         // the loads of eight directions in flight; the sum's order is unchanged
                for (int64_t k = 0; k < P; ++k) acc = acc + g[k * N + a] * theta[k * d + j];
            }
            rows[e] = acc / (double)P;
        }
        return;
    }
    double v = 0.0;
    for (int64_t i = tid; i < n_partial; i += NT) v = v + partial[i];
    const double total = block_sum(v, sd);
    if (tid == 0) value[0] = total * inv_cells / (double)P;
}

struct Layout {                 // the workspace: sorted values [P, n], their rows [P, n], g [P, n], the value partials [P, blocks]
    int64_t blocks;             // coupling workgroups per direction
    size_t vals, perm, g, partial, total;
};

bool slice_args_ok(int64_t n, int64_t d, int64_t n_first, int64_t n_proj) {
    if (n < 2 || n > (int64_t)INT32_MAX || d < 1 || n_first < 1 || n_first >= n) return false;
    if (n_proj < 1 || n_proj > 65535) return false;
    if (d > INT64_MAX / n / (int64_t)sizeof(double)) return false;                  // the rows' bytes overflow
    if ((n * d + NT - 1) / NT + 1 > (int64_t)INT32_MAX) return false;               // the finish's grid.x
    return true;
}

Layout layout_of(int64_t n, int64_t n_proj) {
    Layout l;
    l.blocks = (n + NT - 1) / NT;
    l.vals = align256(sizeof(double) * (size_t)(n_proj * n));
    l.perm = align256(sizeof(int32_t) * (size_t)(n_proj * n));
    l.g = l.vals;
    l.partial = align256(sizeof(double) * (size_t)(n_proj * l.blocks));
    l.total = l.vals + l.perm + l.g + l.partial;
    return l;
}

// the sort kernel's dynamic LDS goes beyond the default limit: raised once per device (one bit per device id)
int allow_sort_lds() {
    static std::atomic<uint64_t> done{0};
    int dev = 0;
    PFM_TRY(hipGetDevice(&dev));
    const uint64_t bit = 1ull << (dev & 63);
    if (dev > 63 || !(done.load(std::memory_order_relaxed) & bit)) {
        PFM_TRY(hipFuncSetAttribute((const void *)k_slice_sort, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)(LDS_ROWS * 12)));
        done.fetch_or(bit, std::memory_order_relaxed);
    }
    return PFM_OK;
}

}  // namespace

// ---- C ABI --------------------------------------------------------------------------------------------

extern "C" size_t pfm_slice_grad_workspace_bytes(int64_t n, int64_t d, int64_t n_first, int64_t n_proj) {
    if (!slice_args_ok(n, d, n_first, n_proj)) return 0;
    return layout_of(n, n_proj).total;
}

extern "C" int pfm_slice_grad(void *stream, int p, const double *Z, int64_t n, int64_t d, int64_t n_first, const double *theta,
                              int64_t n_proj, const int32_t *perm_in, double *value, double *rows, double *cols_out,
                              int32_t *perm_out, void *workspace, size_t workspace_bytes) {
    if (!Z || !value || !slice_args_ok(n, d, n_first, n_proj)) return PFM_EINVAL;
    if (!theta && n_proj != d) return PFM_EINVAL;
    if (p != 1 && p != 2) return PFM_EUNSUPPORTED;
    const int64_t nr = n_first, nf = n - n_first, longer = nr > nf ? nr : nf;
    if (!perm_in && longer > LDS_ROWS) return PFM_EUNSUPPORTED;
    const Layout l = layout_of(n, n_proj);
    if (!workspace || workspace_bytes < l.total) return PFM_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    char *base = (char *)workspace;
    double *vals = (double *)base;
    int32_t *ws_perm = (int32_t *)(base + l.vals);
    double *g = (double *)(base + l.vals + l.perm);
    double *partial = (double *)(base + l.vals + l.perm + l.g);
    const dim3 per_dir((unsigned)l.blocks, (unsigned)n_proj);

    if (perm_in) {
        hipLaunchKernelGGL(k_slice_given, per_dir, dim3(NT), 0, st, Z, n, d, theta, perm_in, vals, cols_out, perm_out);
    } else {
        const int lds_rows = (int)((longer + 1) & ~(int64_t)1);
        const size_t lds_bytes = (size_t)lds_rows * 12;
        if (lds_bytes > 64 * 1024) {
            const int st_lds = allow_sort_lds();
            if (st_lds != PFM_OK) return st_lds;
        }
        hipLaunchKernelGGL(k_slice_project, dim3((unsigned)l.blocks, (unsigned)((n_proj + KC - 1) / KC)), dim3(NT), 0, st, Z, n,
                           d, theta, n_proj, vals, cols_out);
        PFM_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_slice_sort, dim3((unsigned)n_proj, 2), dim3(SORT_NT), lds_bytes, st, n, nr, lds_rows, vals, ws_perm,
                           perm_out);
    }
    PFM_TRY(hipGetLastError());

    const int32_t *perm = perm_in ? perm_in : ws_perm;
    const double inv_cells = 1.0 / ((double)nr * (double)nf);
    double *gk = rows ? g : nullptr;
    if (p == 1)
        hipLaunchKernelGGL(k_slice_couple<1>, per_dir, dim3(NT), 0, st, (const double *)vals, perm, nr, nf, inv_cells, gk, partial);
    else
        hipLaunchKernelGGL(k_slice_couple<2>, per_dir, dim3(NT), 0, st, (const double *)vals, perm, nr, nf, inv_cells, gk, partial);
    PFM_TRY(hipGetLastError());

    const int64_t rblocks = rows ? (n * d + NT - 1) / NT : 0;
    hipLaunchKernelGGL(k_slice_finish, dim3((unsigned)(rblocks + 1)), dim3(NT), 0, st, (const double *)g, theta, n, d, n_proj,
                       (const double *)partial, n_proj * l.blocks, inv_cells, value, rows);
    PFM_TRY(hipGetLastError());
    return PFM_OK;
}
