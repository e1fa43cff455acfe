// pf_scan1d.h -- what the per-column bootstrap kernels of libpf_metrics.so share (pf_metrics1d.hip, pf_wasserstein.hip): the
// draw counts of a replicate, a column's sorted order with its tie groups, and the workgroup's integer scan and fixed-order sum.
// The draw counts (launch_counts) also serve pf_energy.hip and pf_sinkhorn.hip, whose size check pair_sizes_ok is; the fixed-order
// sum and maximum (block_sum, block_max) serve every finish kernel that reduces one value per thread, and the two Sinkhorn
// finishes share their tail here (sinkhorn_value_drift).
#ifndef PF_SCAN1D_H
#define PF_SCAN1D_H

#include "pf_common.h"

namespace {

constexpr int IPT = 4;           // tie groups per thread per chunk of the scan

__global__ void __launch_bounds__(NT) k_counts(const int32_t *idx_r, const int32_t *idx_f, int64_t nr, int64_t nf,
                                               int32_t *cnt) {
    const int64_t rep = blockIdx.y, N = nr + nf;
    int32_t *c = cnt + rep * N;
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < N; i += (int64_t)gridDim.x * NT) {
        if (i < nr) {
            const int32_t j = idx_r[rep * nr + i];
            if ((uint32_t)j < (uint32_t)nr) atomicAdd(&c[j], 1);
        } else {
            const int32_t j = idx_f[rep * nf + (i - nr)];
            if ((uint32_t)j < (uint32_t)nf) atomicAdd(&c[nr + j], 1);
        }
    }
}

// cnt [reps, nr + nf] = the draw counts of every replicate: zeroed and counted on `stream`; the launch's status
inline hipError_t launch_counts(hipStream_t stream, const int32_t *idx_r, const int32_t *idx_f, int64_t nr, int64_t nf,
                                int64_t reps, int32_t *cnt) {
    const int64_t N = nr + nf;
    const hipError_t e = hipMemsetAsync(cnt, 0, sizeof(int32_t) * (size_t)reps * (size_t)N, stream);
    if (e != hipSuccess) return e;
    int64_t cb = (N + NT - 1) / NT;
    if (cb > 1024) cb = 1024;
    hipLaunchKernelGGL(k_counts, dim3((unsigned)cb, (unsigned)reps), dim3(NT), 0, stream, idx_r, idx_f, nr, nf, cnt);
    return hipGetLastError();
}

// the sizes pfm_energy and pfm_sinkhorn accept: two samples of d features gathered through int32 indices, reps in grid.y
inline bool pair_sizes_ok(int64_t nr, int64_t nf, int64_t d, int64_t reps) {
    if (nr < 1 || nf < 1 || d < 1 || reps < 1 || reps > 65535) return false;
    if (nr > (int64_t)INT32_MAX || nf > (int64_t)INT32_MAX) return false;        // int32 indices
    const int64_t big = nr > nf ? nr : nf;
    return d <= INT64_MAX / big / (int64_t)sizeof(double);                      // a row's byte offset overflows
}

struct Feature {                 // one (feature, replicate): the sorted order, its tie groups, the draw counts
    const double *col;           // pooled original column [N]
    const int32_t *perm, *gs;    // sorted position -> pooled row [N]; group g = positions gs[g] .. gs[g + 1] - 1
    const int32_t *cnt;          // draw count of each pooled row [N]
    int64_t nr, N;
    int G;
    __device__ void counts(int g, int64_t &l, int64_t &ar) const {
        l = 0;
        ar = 0;
        for (int32_t k = gs[g]; k < gs[g + 1]; ++k) {
            const int32_t row = perm[k];
            const int64_t v = cnt[row];
            l += v;
            if (row < nr) ar += v;
        }
    }
    __device__ double value(int g) const { return col[perm[gs[g]]]; }
};

// inclusive block scan of (a, b) over the workgroup's threads; returns the exclusive prefix, totals in ta / tb
__device__ void block_scan2(int64_t a, int64_t b, int64_t &ea, int64_t &eb, int64_t &ta, int64_t &tb, int64_t *sa,
                            int64_t *sb) {
    const int tid = threadIdx.x;
    sa[tid] = a;
    sb[tid] = b;
    __syncthreads();
    for (int off = 1; off < NT; off <<= 1) {
        const int64_t xa = tid >= off ? sa[tid - off] : 0, xb = tid >= off ? sb[tid - off] : 0;
        __syncthreads();
        sa[tid] += xa;
        sb[tid] += xb;
        __syncthreads();
    }
    ea = sa[tid] - a;
    eb = sb[tid] - b;
    ta = sa[NT - 1];
    tb = sb[NT - 1];
    __syncthreads();
}

// fixed-order tree sum of one double per thread; every thread gets the total
__device__ double block_sum(double v, double *sd) {
    const int tid = threadIdx.x;
    sd[tid] = v;
    __syncthreads();
    for (int off = NT / 2; off > 0; off >>= 1) {
        if (tid < off) sd[tid] = sd[tid] + sd[tid + off];
        __syncthreads();
    }
    const double s = sd[0];
    __syncthreads();
    return s;
}

// the same tree with fmax
__device__ double block_max(double v, double *sd) {
    const int tid = threadIdx.x;
    sd[tid] = v;
    __syncthreads();
    for (int off = NT / 2; off > 0; off >>= 1) {
        if (tid < off) sd[tid] = fmax(sd[tid], sd[tid + off]);
        __syncthreads();
    }
    const double s = sd[0];
    __syncthreads();
    return s;
}

// the tail of the two Sinkhorn finishes (pf_sinkhorn.hip, pf_sinkgrad.hip) for the four potentials of n pooled rows under one
// weighting: value = sum_i weight(i) (fin[0][i] - fin[1][i]), thread t taking i = t, t + NT, .. and then block_sum;
// drift = the largest |cur - prev| of a potential (0 without has_prev).  A row of weight 0 takes no part in either.
template <class Weight>
__device__ void sinkhorn_value_drift(const double *fin, const double *cur, const double *prev, int has_prev, int64_t n,
                                     Weight weight, double *sd, double &value, double &drift) {
    double v = 0.0, dr = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += NT) {
        const double w = weight(i);
        if (w > 0.0) {
            v = v + w * (fin[i] - fin[n + i]);
            if (has_prev) dr = fmax(dr, fmax(fabs(cur[i] - prev[i]), fabs(cur[n + i] - prev[n + i])));
        }
    }
    value = block_sum(v, sd);
    drift = block_max(dr, sd);
}

}  // namespace

#endif
