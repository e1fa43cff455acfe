// pf_nn.hip -- which rows are a row's nearest neighbours, and how many of them carry the row's own label, for gfx950
// (C ABI: pf_metrics.h, pfm_nn_index and pfm_nn_count; the nearest-neighbour two-sample test of metrics/twosample.py).
//
//   k_nn_index<L>   one workgroup per 64-row query tile of the pooled sample Z: it sweeps every 64-row candidate tile in
//                   ascending order and writes, per query row a, the k nearest OTHER rows in ascending order of
//                   (d^2, row index), as nbr[a, r] and d2[a, r].  Row a itself is left out by its index, not by its distance:
//                   a duplicate of a is a neighbour at distance exactly 0.  The sweep of pf_nearest.h with the index kept
//                   beside the value (which also says why its pruning is exact under that order).
//   k_nn_count      workgroups (labelling, slice of the n k slots): the labelling's bytes are packed into bits in LDS (while
//                   n <= PFM_NN_STAGE_MAX_N; read from global memory above that), nbr is read coalesced, and the slots whose
//                   row and neighbour are both labelled (counts[p, 0]) or both unlabelled (counts[p, 1]) are counted
//   k_nn_count_sum  adds the slices' counts of a labelling where there are several
// Every distance is tile_d2 of pf_pairtile.h on a Plain source: bitwise what pfm_prdc and the other kernels form for the pair.
// The counts are integers added in a fixed order.  Both calls are bitwise reproducible and keep no state.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "pf_metrics.h"
#include "pf_nearest.h"

namespace {

template <int L>
__global__ void __launch_bounds__(NT) k_nn_index(const double *Zp, int64_t n, int64_t d, int k, int32_t *nbr, double *d2) {
    __shared__ double sA[DC][TPAD], sB[DC][TPAD];
    __shared__ double heads[2][4][16][16];
    __shared__ int32_t headj[2][4][16][16];
    const int64_t bi = blockIdx.x;
    Plain Z;
    Z.X = Zp;
    Z.n = n;
    Z.d = d;
    const int tid = threadIdx.x, ti = tid >> 4, tj = tid & 15;

    Nearest<L, true> near;
    near.init();
    const bool resident = d <= DC;
    if (resident) stage(Z, bi * TILE, 0, (int)d, sA);     // (tile_d2 begins with a barrier)
    const int64_t nb = tiles_per_side(n);
    for (int64_t bj = 0; bj < nb; ++bj) {
        double acc[4][4];
        tile_d2(Z, bi * TILE, Z, bj * TILE, resident, sA, sB, acc);
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int64_t gj = bj * TILE + tj + 16 * b;
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                const bool take = gj < n && gj != bi * TILE + ti + 16 * a;      // a row is no neighbour of itself
                near.offer(a, take ? acc[a][b] : INFINITY, (int32_t)gj);
            }
        }
        near.share();
    }
    for (int it = 0; it < k; ++it) {            // round r of the merge gives the neighbour of rank r
        near.take(heads[it & 1], headj[it & 1], [&](int a, double m, int32_t mj) {
            const int64_t gi = bi * TILE + ti + 16 * a;
            if (tj == 0 && gi < n) {
                nbr[gi * k + it] = mj;
                d2[gi * k + it] = m;
            }
        });
    }
}

// ---- the counts ------------------------------------------------------------------------------------------

constexpr int64_t SLOTS_PER_WG = 1 << 16;      // slots (row, rank) of one workgroup, at least

// slots per workgroup: a staging workgroup reads the labelling's n bytes first, so it takes 4 n slots at least
__host__ __device__ inline int64_t slots_per_wg(int64_t n, int64_t k) {
    const int64_t slots = n * k;
    int64_t per = SLOTS_PER_WG;
    if (n <= PFM_NN_STAGE_MAX_N && 4 * n > per) per = 4 * n;
    const int64_t most = (slots + 65534) / 65535;             // grid.y
    return per > most ? per : most;
}

inline int64_t count_slices(int64_t n, int64_t k) {
    const int64_t per = slots_per_wg(n, k);
    return (n * k + per - 1) / per;
}

template <bool STAGED>
__global__ void __launch_bounds__(NT) k_nn_count(const int32_t *nbr, int64_t n, int64_t k, const uint8_t *labels, int64_t *out) {
    __shared__ uint64_t bits[STAGED ? PFM_NN_STAGE_MAX_N / 64 : 1];
    __shared__ int64_t red[2][NT];
    const int64_t rep = blockIdx.x, slice = blockIdx.y;
    const uint8_t *lab = labels + rep * n;
    const int tid = threadIdx.x;
    if (STAGED) {               // 64 label bytes -> one 64-bit word: bit (a & 63) of bits[a >> 6] is set iff lab[a] != 0
        for (int64_t w0 = tid & ~63; w0 < n; w0 += NT) {      // (the same trip count for the 64 lanes of a wave)
            const int64_t a = w0 + (tid & 63);
            const uint64_t m = __ballot(a < n && lab[a] != 0);
            if ((tid & 63) == 0) bits[w0 >> 6] = m;
        }
        __syncthreads();
    }
    const int64_t per = slots_per_wg(n, k), slots = n * k;
    const int64_t s0 = slice * per, s1 = s0 + per < slots ? s0 + per : slots;
    // slot s = a k + r: the thread's slots s0 + tid, + NT, ...; (a, r) advance without a division per slot
    const int64_t qa = NT / k, qr = NT - qa * k;
    int64_t a = (s0 + tid) / k, r = (s0 + tid) - a * k;
    int64_t both1 = 0, both0 = 0;
    for (int64_t s = s0 + tid; s < s1; s += NT) {
        const int64_t j = nbr[s];
        int la, lb;
        if (STAGED) {
            la = (int)(bits[a >> 6] >> (a & 63)) & 1;
            lb = (int)(bits[j >> 6] >> (j & 63)) & 1;
        } else {
            la = lab[a] != 0;
            lb = lab[j] != 0;
        }
        both1 += la & lb;
        both0 += (la | lb) ^ 1;
        a += qa;
        r += qr;
        if (r >= k) { r -= k; ++a; }
    }
    red[0][tid] = both1;
    red[1][tid] = both0;
    __syncthreads();
    for (int s = NT / 2; s > 0; s >>= 1) {
        if (tid < s) {
            red[0][tid] += red[0][tid + s];
            red[1][tid] += red[1][tid + s];
        }
        __syncthreads();
    }
    if (tid < 2) out[(rep * gridDim.y + slice) * 2 + tid] = red[tid][0];
}

__global__ void __launch_bounds__(NT) k_nn_count_sum(const int64_t *partial, int64_t reps, int64_t slices, int64_t *counts) {
    const int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x;          // (labelling, which count)
    if (e >= reps * 2) return;
    const int64_t rep = e >> 1, c = e & 1;
    int64_t s = 0;
    for (int64_t i = 0; i < slices; ++i) s += partial[(rep * slices + i) * 2 + c];
    counts[e] = s;
}

bool index_args_ok(int64_t n, int64_t d, int64_t k) {
    if (n < 2 || n > (int64_t)INT32_MAX || d < 1 || k < 1 || k > n - 1) return false;
    return d <= INT64_MAX / n / (int64_t)sizeof(double);                        // a row's byte offset overflows
}

bool count_args_ok(int64_t n, int64_t k, int64_t reps) {
    if (n < 1 || n > (int64_t)INT32_MAX || k < 1 || reps < 1 || reps > (int64_t)INT32_MAX) return false;   // reps is grid.x
    if (k > (INT64_MAX >> 4) / n) return false;                                 // the slots' byte offsets overflow
    return count_slices(n, k) <= (INT64_MAX >> 5) / reps;                       // and the partial counts'
}

}  // namespace

// ---- C ABI --------------------------------------------------------------------------------------------

extern "C" size_t pfm_nn_index_workspace_bytes(int64_t n, int64_t d, int64_t k) {
    if (!index_args_ok(n, d, k) || k > PFM_NN_MAX_K) return 0;
    return 256;                                    // nothing is kept between launches: the least a caller can allocate
}

extern "C" int pfm_nn_index(void *stream, const double *Z, int64_t n, int64_t d, int64_t k, int32_t *nbr, double *d2,
                            void *workspace, size_t workspace_bytes) {
    if (!Z || !nbr || !d2 || !index_args_ok(n, d, k)) return PFM_EINVAL;
    if (k > PFM_NN_MAX_K) return PFM_EUNSUPPORTED;
    if (!workspace || workspace_bytes < pfm_nn_index_workspace_bytes(n, d, k)) return PFM_EWORKSPACE;
    const dim3 grid((unsigned)tiles_per_side(n));
#define PFM_NN_INDEX(L_) \
    hipLaunchKernelGGL(k_nn_index<L_>, grid, dim3(NT), 0, (hipStream_t)stream, Z, n, d, (int)k, nbr, d2)
    if (k <= 2) PFM_NN_INDEX(2);
    else if (k <= 5) PFM_NN_INDEX(5);
    else if (k <= 10) PFM_NN_INDEX(10);
    else PFM_NN_INDEX(PFM_NN_MAX_K);
#undef PFM_NN_INDEX
    PFM_TRY(hipGetLastError());
    return PFM_OK;
}

extern "C" size_t pfm_nn_count_workspace_bytes(int64_t n, int64_t k, int64_t reps) {
    if (!count_args_ok(n, k, reps)) return 0;
    return align256(sizeof(int64_t) * 2 * (size_t)reps * (size_t)count_slices(n, k));
}

extern "C" int pfm_nn_count(void *stream, const int32_t *nbr, int64_t n, int64_t k, const uint8_t *labels, int64_t reps,
                            int64_t *counts, void *workspace, size_t workspace_bytes) {
    if (!nbr || !labels || !counts || !count_args_ok(n, k, reps)) return PFM_EINVAL;
    if (!workspace || workspace_bytes < pfm_nn_count_workspace_bytes(n, k, reps)) return PFM_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int64_t slices = count_slices(n, k);
    int64_t *out = slices == 1 ? counts : (int64_t *)workspace;      // one slice: its counts are the labelling's
    const dim3 grid((unsigned)reps, (unsigned)slices);
    if (n <= PFM_NN_STAGE_MAX_N) hipLaunchKernelGGL(k_nn_count<true>, grid, dim3(NT), 0, st, nbr, n, k, labels, out);
    else hipLaunchKernelGGL(k_nn_count<false>, grid, dim3(NT), 0, st, nbr, n, k, labels, out);
    PFM_TRY(hipGetLastError());
    if (slices > 1) {
        hipLaunchKernelGGL(k_nn_count_sum, dim3((unsigned)((reps * 2 + NT - 1) / NT)), dim3(NT), 0, st, out, reps, slices, counts);
        PFM_TRY(hipGetLastError());
    }
    return PFM_OK;
}
