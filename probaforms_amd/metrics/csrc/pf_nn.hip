// pf_nn.hip -- which rows are a row's nearest neighbours, and how many of them carry the row's own label, for gfx950
// (C ABI: pf_metrics.h, pfm_nn_index and pfm_nn_count; the nearest-neighbour two-sample test of metrics/twosample.py).
//
//   k_nn_index<L>   one workgroup per 64-row query tile of the pooled sample Z: it sweeps every 64-row candidate tile in
//                   ascending order and writes, per query row a, the k nearest OTHER rows in ascending order of
//                   (d^2, row index), as nbr[a, r] and d2[a, r].  Row a itself is left out by its index, not by its distance:
//                   a duplicate of a is a neighbour at distance exactly 0.  k_knn_radius<L> of pf_knn.hip with the index kept
//                   beside the value, in the lists and in the merge.
//   k_nn_count      workgroups (labelling, slice of the n k slots): the labelling's bytes are packed into bits in LDS (while
//                   n <= PFM_NN_STAGE_MAX_N; read from global memory above that), nbr is read coalesced, and the slots whose
//                   row and neighbour are both labelled (counts[p, 0]) or both unlabelled (counts[p, 1]) are counted
//   k_nn_count_sum  adds the slices' counts of a labelling where there are several
// Every distance is tile_d2 of pf_pairtile.h on a Plain source: bitwise what pfm_prdc and the other kernels form for the pair.
// The counts are integers added in a fixed order.  Both calls are bitwise reproducible and keep no state.
//
// Why `v < bound` stays exact under the (d^2, row index) order.  A lane keeps, per query row, the L >= k smallest candidates it
// has met, ascending.  It meets its candidates in ascending row index: the tiles are swept in ascending order and inside a tile
// the lane's columns tj + 16 b ascend with b.  The insertion moves a new entry past strictly larger values only, so among equal
// values the earlier, smaller index stays in front: a list is ascending in (d^2, index).  `bound` is never above the lane's own
// L-th value, and is lowered after every tile to the smallest L-th value among the row's 16 lanes.  So whatever the bound rests
// on is a list of L >= k candidates that were met before the candidate under test: by the lane itself (smaller indices, same
// or earlier tile) or by another lane in an EARLIER tile (smaller indices again).  A candidate with v >= bound therefore has at
// least k candidates in front of it in (d^2, index) order, all with values <= v and smaller indices; it is not among the k
// nearest and skipping it changes nothing, ties included.  The argument needs the ascending sweep: in another order a
// candidate equal to the bound could carry the smaller index and would have to be kept.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "pf_metrics.h"
#include "pf_pairtile.h"

namespace {

// (v, j) into the list (b, id), ascending in (value, index), of the L nearest candidates met so far (the caller has tested
// v < b[L - 1], and j is above every index in the list): it replaces the last entry and sinks past strictly larger values
// through an unrolled compare-exchange chain; every list index is a compile-time constant, so the lists stay in registers
template <int L>
__device__ inline void push(double (&b)[L], int32_t (&id)[L], double v, int32_t j) {
    b[L - 1] = v;
    id[L - 1] = j;
#pragma unroll
    for (int i = L - 1; i > 0; --i) {
        const double hi = b[i], lo = b[i - 1];
        const int32_t jh = id[i], jl = id[i - 1];
        const bool sw = hi < lo;
        b[i - 1] = sw ? hi : lo;
        b[i] = sw ? lo : hi;
        id[i - 1] = sw ? jh : jl;
        id[i] = sw ? jl : jh;
    }
}

template <int L>
__device__ inline void pop(double (&b)[L], int32_t (&id)[L]) {
#pragma unroll
    for (int i = 0; i + 1 < L; ++i) {
        b[i] = b[i + 1];
        id[i] = id[i + 1];
    }
    b[L - 1] = INFINITY;
    id[L - 1] = INT32_MAX;
}

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

    double best[4][L], bound[4];
    int32_t who[4][L];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        bound[a] = INFINITY;
#pragma unroll
        for (int i = 0; i < L; ++i) {
            best[a][i] = INFINITY;
            who[a][i] = INT32_MAX;
        }
    }
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
                const double v = take ? acc[a][b] : INFINITY;
                if (v < bound[a]) {
                    push<L>(best[a], who[a], v, (int32_t)gj);
                    bound[a] = best[a][L - 1] < bound[a] ? best[a][L - 1] : bound[a];
                }
            }
        }
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            double m = bound[a];
#pragma unroll
            for (int s = 1; s < 16; s <<= 1) {
                const double o = __shfl_xor(m, s, 16);
                m = o < m ? o : m;
            }
            bound[a] = m;
        }
    }

    // the 16 threads of a query row merge their lists through LDS: k rounds, each takes the smallest (d^2, index) of the 16
    // heads, and the thread that held it pops it (an index is in one list only); round r gives the neighbour of rank r
    for (int it = 0; it < k; ++it) {
        double (*h)[16][16] = heads[it & 1];
        int32_t (*hj)[16][16] = headj[it & 1];
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            h[a][ti][tj] = best[a][0];
            hj[a][ti][tj] = who[a][0];
        }
        __syncthreads();
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            double m = h[a][ti][0];
            int32_t mj = hj[a][ti][0];
#pragma unroll
            for (int t = 1; t < 16; ++t) {
                const double o = h[a][ti][t];
                const int32_t oj = hj[a][ti][t];
                if (o < m || (o == m && oj < mj)) { m = o; mj = oj; }
            }
            if (mj == who[a][0]) pop<L>(best[a], who[a]);
            const int64_t gi = bi * TILE + ti + 16 * a;
            if (tj == 0 && gi < n) {
                nbr[gi * k + it] = mj;
                d2[gi * k + it] = m;
            }
        }
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
