// pf_knn.hip -- k-nearest-neighbour precision, recall, density and coverage for gfx950 (C ABI: pf_metrics.h, pfm_prdc).
//
// Per bootstrap replicate (grid.y), with R = Xr[idx_r] (nr rows) and F = Xf[idx_f] (nf rows) gathered through the int32
// index vectors (no resampled copy is built) and k = nearest_k:
//   k_knn_radius<L>  jobs (replicate, sample, 64-row query tile): the workgroup sweeps every 64-row candidate tile of the
//                    same resampled sample and writes, per query row, the (k + 1)-th smallest squared distance of its row
//                    of D^2(S, S), the diagonal 0 and the zeros of duplicated rows included (np.partition(row, k)[k])
//   k_prdc_sweep     jobs (replicate, 64-row real tile): sweeps all fake tiles of D^2(R, F) against the radii.  cov[i] and
//                    rec[i] are complete inside the workgroup and leave it as two integers; c[j] is summed over the tile
//                    in LDS and added to an int32 array with one integer atomic per fake column and tile
//   k_prdc_final     one workgroup per replicate: P = #{c > 0}, Rc, Dn = sum c, Cv as int64
// Every distance is the squared Euclidean distance accumulated as fma(df, df, acc) over the features in order, in float64:
// tile_d2 of pf_pairtile.h, pfm_mmd's chunk_d2.  No square root is taken and no norm / dot-product identity is used: a
// duplicated row's distance is exactly 0 and the comparisons `d^2 < radius^2` are between values of one formula.  The outputs
// are order statistics (values) and integer counts (integer atomics are exact and order-free), so a call is bitwise
// reproducible and a replicate's result does not depend on the grid.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "pf_metrics.h"
#include "pf_nearest.h"

namespace {

struct Rows {                       // one replicate's resampled sample X[idx]: a row source of pf_pairtile.h
    const double *X;
    const int32_t *idx;
    int64_t n, d;
    __device__ const double *row(int64_t r) const { return X + (int64_t)idx[r] * d; }
};

// The sweep of pf_nearest.h over the candidate tiles of the same resampled sample, values only: every row in range counts, the
// query row itself included, so L >= k + 1 values are kept and round k of the merge gives the (k + 1)-th smallest of the row.
template <int L>
__global__ void __launch_bounds__(NT) k_knn_radius(const double *Xr, int64_t nr, const double *Xf, int64_t nf, int64_t d,
                                                   const int32_t *idx_r, const int32_t *idx_f, int k, double *rad_r,
                                                   double *rad_f) {
    __shared__ double sA[DC][TPAD], sB[DC][TPAD];
    __shared__ double heads[2][4][16][16];
    const int64_t rep = blockIdx.y, ntr = tiles_per_side(nr);
    const bool fake = (int64_t)blockIdx.x >= ntr;
    const int64_t bi = fake ? (int64_t)blockIdx.x - ntr : (int64_t)blockIdx.x;
    Rows S;
    S.X = fake ? Xf : Xr;
    S.n = fake ? nf : nr;
    S.idx = fake ? idx_f + rep * nf : idx_r + rep * nr;
    S.d = d;
    double *out = fake ? rad_f + rep * nf : rad_r + rep * nr;
    const int tid = threadIdx.x, ti = tid >> 4, tj = tid & 15;

    Nearest<L, false> near;
    near.init();
    const bool resident = d <= DC;
    if (resident) stage(S, bi * TILE, 0, (int)d, sA);     // (tile_d2 begins with a barrier)
    const int64_t nb = tiles_per_side(S.n);
    for (int64_t bj = 0; bj < nb; ++bj) {
        double acc[4][4];
        tile_d2(S, bi * TILE, S, bj * TILE, resident, sA, sB, acc);
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const bool in = bj * TILE + tj + 16 * b < S.n;
#pragma unroll
            for (int a = 0; a < 4; ++a) near.offer(a, in ? acc[a][b] : INFINITY, 0);
        }
        near.share();
    }
    double res[4] = {0.0, 0.0, 0.0, 0.0};
    for (int it = 0; it <= k; ++it) near.take(heads[it & 1], nullptr, [&](int a, double m, int32_t) { res[a] = m; });
    if (tj == 0) {
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const int64_t gi = bi * TILE + ti + 16 * a;
            if (gi < S.n) out[gi] = res[a];
        }
    }
}

__global__ void __launch_bounds__(NT) k_prdc_sweep(const double *Xr, int64_t nr, const double *Xf, int64_t nf, int64_t d,
                                                   const int32_t *idx_r, const int32_t *idx_f, const double *rad_r,
                                                   const double *rad_f, int32_t *c, int32_t *wg) {
    __shared__ double sA[DC][TPAD], sB[DC][TPAD];
    __shared__ int32_t colcnt[TILE], rowflag[2][TILE];
    const int64_t rep = blockIdx.y, bi = blockIdx.x;
    Rows R, F;
    R.X = Xr; R.idx = idx_r + rep * nr; R.n = nr; R.d = d;
    F.X = Xf; F.idx = idx_f + rep * nf; F.n = nf; F.d = d;
    const double *rr = rad_r + rep * nr, *ss = rad_f + rep * nf;
    int32_t *crep = c + rep * nf;
    const int tid = threadIdx.x, ti = tid >> 4, tj = tid & 15;

    double rr4[4];                  // a squared distance is never below -1: rows and columns past the end match nothing
    bool cov[4], rec[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const int64_t gi = bi * TILE + ti + 16 * a;
        rr4[a] = gi < nr ? rr[gi] : -1.0;
        cov[a] = rec[a] = false;
    }
    if (tid < TILE) { colcnt[tid] = 0; rowflag[0][tid] = 0; rowflag[1][tid] = 0; }
    const bool resident = d <= DC;
    if (resident) stage(R, bi * TILE, 0, (int)d, sA);     // (tile_d2 begins with a barrier, which also orders the zero stores)
    const int64_t nb = tiles_per_side(nf);
    for (int64_t bj = 0; bj < nb; ++bj) {
        double acc[4][4];
        tile_d2(R, bi * TILE, F, bj * TILE, resident, sA, sB, acc);
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int64_t gj = bj * TILE + tj + 16 * b;
            const bool in = gj < nf;
            const double s2 = in ? ss[gj] : -1.0;
            int32_t cnt = 0;
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                const bool inside = in && acc[a][b] < rr4[a];
                cnt += inside ? 1 : 0;
                cov[a] = cov[a] || inside;
                rec[a] = rec[a] || acc[a][b] < s2;
            }
            if (cnt) atomicAdd(&colcnt[tj + 16 * b], cnt);
        }
        __syncthreads();
        if (tid < TILE) {           // (only columns inside the sample were counted)
            const int32_t v = colcnt[tid];
            if (v) {
                atomicAdd(&crep[bj * TILE + tid], v);
                colcnt[tid] = 0;
            }
        }
    }
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        if (cov[a]) rowflag[0][ti + 16 * a] = 1;
        if (rec[a]) rowflag[1][ti + 16 * a] = 1;
    }
    __syncthreads();
    if (tid < 2) {
        const int64_t left = nr - bi * TILE;
        const int rows = (int)(left < TILE ? left : TILE);
        int32_t s = 0;
        for (int i = 0; i < rows; ++i) s += rowflag[tid][i];
        wg[(rep * gridDim.x + bi) * 2 + tid] = s;          // [0] covered rows, [1] recalled rows of this tile
    }
}

__global__ void __launch_bounds__(NT) k_prdc_final(const int32_t *c, const int32_t *wg, int64_t nf, int64_t ntr,
                                                   int64_t *counts) {
    __shared__ int64_t red[4][NT];
    const int64_t rep = blockIdx.x;
    const int tid = threadIdx.x;
    int64_t p = 0, rc = 0, dn = 0, cv = 0;
    for (int64_t j = tid; j < nf; j += NT) {
        const int32_t v = c[rep * nf + j];
        p += v > 0 ? 1 : 0;
        dn += v;
    }
    for (int64_t t = tid; t < ntr; t += NT) {
        cv += wg[(rep * ntr + t) * 2];
        rc += wg[(rep * ntr + t) * 2 + 1];
    }
    red[0][tid] = p; red[1][tid] = rc; red[2][tid] = dn; red[3][tid] = cv;
    __syncthreads();
    for (int s = NT / 2; s > 0; s >>= 1) {
        if (tid < s) {
#pragma unroll
            for (int q = 0; q < 4; ++q) red[q][tid] += red[q][tid + s];
        }
        __syncthreads();
    }
    if (tid < 4) counts[rep * 4 + tid] = red[tid][0];
}

bool prdc_args_ok(int64_t nr, int64_t nf, int64_t d, int64_t reps, int64_t k) {
    if (nr < 1 || nf < 1 || d < 1 || reps < 1 || reps > 65535 || k < 1) return false;
    if (nr > (int64_t)INT32_MAX || nf > (int64_t)INT32_MAX) return false;        // int32 indices
    const int64_t big = nr > nf ? nr : nf;
    if (d > INT64_MAX / big) return false;                                      // a row's offset overflows
    return k < (nr < nf ? nr : nf);
}

}  // namespace

// ---- C ABI --------------------------------------------------------------------------------------------

extern "C" size_t pfm_prdc_workspace_bytes(int64_t nr, int64_t nf, int64_t d, int64_t reps, int64_t k) {
    if (!prdc_args_ok(nr, nf, d, reps, k) || k > PFM_KNN_MAX_K) return 0;
    return align256(sizeof(int32_t) * (size_t)reps * (size_t)nf) +
           align256(sizeof(int32_t) * 2 * (size_t)reps * (size_t)tiles_per_side(nr));
}

extern "C" int pfm_prdc(void *stream, const double *Xr, int64_t nr, const double *Xf, int64_t nf, int64_t d,
                        const int32_t *idx_r, const int32_t *idx_f, int64_t reps, int64_t k, double *radius2_r,
                        double *radius2_f, int64_t *counts, void *workspace, size_t workspace_bytes) {
    if (!Xr || !Xf || !idx_r || !idx_f || !radius2_r || !radius2_f || !counts || !prdc_args_ok(nr, nf, d, reps, k))
        return PFM_EINVAL;
    if (k > PFM_KNN_MAX_K) return PFM_EUNSUPPORTED;
    const size_t need = pfm_prdc_workspace_bytes(nr, nf, d, reps, k);
    if (!workspace || workspace_bytes < need) return PFM_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int64_t ntr = tiles_per_side(nr), ntf = tiles_per_side(nf);
    const size_t cbytes = sizeof(int32_t) * (size_t)reps * (size_t)nf;
    int32_t *c = (int32_t *)workspace;
    int32_t *wg = (int32_t *)((char *)workspace + align256(cbytes));

    PFM_TRY(hipMemsetAsync(c, 0, cbytes, st));
    const dim3 grid_rad((unsigned)(ntr + ntf), (unsigned)reps);
#define PFM_RADIUS(L_)                                                                                                  \
    hipLaunchKernelGGL(k_knn_radius<L_>, grid_rad, dim3(NT), 0, st, Xr, nr, Xf, nf, d, idx_r, idx_f, (int)k, radius2_r, \
                       radius2_f)
    if (k + 1 <= 3) PFM_RADIUS(3);
    else if (k + 1 <= 6) PFM_RADIUS(6);
    else if (k + 1 <= 11) PFM_RADIUS(11);
    else PFM_RADIUS(PFM_KNN_MAX_K + 1);
#undef PFM_RADIUS
    PFM_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_prdc_sweep, dim3((unsigned)ntr, (unsigned)reps), dim3(NT), 0, st, Xr, nr, Xf, nf, d, idx_r, idx_f,
                       radius2_r, radius2_f, c, wg);
    PFM_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_prdc_final, dim3((unsigned)reps), dim3(NT), 0, st, c, wg, nf, ntr, counts);
    PFM_TRY(hipGetLastError());
    return PFM_OK;
}
