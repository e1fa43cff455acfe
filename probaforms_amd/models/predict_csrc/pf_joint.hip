// pf_joint.hip -- pfp_joint_scores / pfp_joint_tiling of libpf_predict.so (C ABI: pf_predict.h): the energy score and the
// variogram score of the K draws of every condition row against its observed target (gfx950).
//
// k_joint: one 256-thread workgroup works on one row at a time and grid-strides over the rows.  The row's draws are staged
// through LDS as float32 images [column][draw], draw-contiguous as in xt.  Every difference, square, sum and square root is
// float64 (the float32 values are widened when they are read from the image).
//
//   pairs      The K (K - 1) / 2 unordered pairs are walked in blocks of 64 x 64 draws (block row bi <= block column bj).  In a
//              block thread (g, a) = (tid / 64, tid % 64) owns draw a of the block row against the 16 draws 16 g .. 16 g + 15 of
//              the block column: per column it reads its own value once (consecutive lanes, consecutive words) and the 16
//              partners as broadcasts (g is the wave), into 16 float64 sums of squares held in registers.  A pair counts where
//              its first draw lies below its second, so a diagonal block counts its upper triangle; all 256 threads walk every
//              block together, so no thread is left with the long end of a triangle.
//   target     In the diagonal blocks wave 0 carries y as a 17th partner: sum_k |x_k - y|.
//   tiles      Plan (joint_plan, reported by pfp_joint_tiling): (a) d (K + 1) floats within the budget: the whole row is ONE
//              image, staged once; (b) otherwise tiles of T draws (a multiple of 64) with two images, d (2 T + 1) floats: tile
//              P stays while the tiles Q >= P pass through the second image; (c) d too wide even for T = 64: tiles of 64 draws
//              and chunks of columns, the 16 sums of squares staying in registers while the chunks pass through.
//   variogram  Wave w takes the column pairs i < j numbered w, w + 4, ...: its lanes stride over the K draws (from the image in
//              plan (a), else from xt itself, which this workgroup has just read), a fixed xor butterfly joins the 64 partials,
//              and the wave adds (|y_i - y_j|^p - mean)^2.  The sum over all (i, j) is twice the sum over i < j.
//   sums       Every thread adds its distances in the order it meets them; the 256 float64 partials are combined by the halving
//              tree of k_scores.  No atomics; the order depends on (d, K) alone: a row gives the same bits in any call and grid.
//   non-finite A pass over the row's words of xt and y sets three flags (a NaN, an infinite draw, an infinite target) and the
//              outputs follow pf_predict.h; in particular the pair sum's diagonal, which is not summed, is set explicitly.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "pf_predict.h"

namespace {

constexpr int kThreads = 256;
constexpr int kBlock = 64;                  // draws of a block row / column
constexpr int kPartners = 16;               // partners per thread in a block: kBlock * kBlock / kThreads
constexpr int kMaxGrid = 65536;
constexpr int kBudget = 40 * 1024;          // the images and y; with the scratch below one workgroup stays under 48 KiB
constexpr int kScratch = kThreads * (2 * (int)sizeof(double) + (int)sizeof(uint32_t));

struct Plan {
    int tile;        // draws per image (K in plan (a))
    int n_tiles;
    int cols;        // columns per chunk (d in plans (a), (b))
    int n_chunks;
    int img;         // floats of one image; plan (a) has one image, (b) and (c) two
    int n_img;
    int ycap;        // floats of y held at once
};

Plan joint_plan(int64_t d, int64_t K) {
    const int64_t cap = kBudget / (int64_t)sizeof(float);
    Plan p;
    if (d * (K + 1) <= cap) {
        p = Plan{(int)K, 1, (int)d, 1, (int)(d * K), 1, (int)d};
    } else if (d * (2 * kBlock + 1) <= cap) {
        const int64_t t = (cap / d - 1) / 2 / kBlock * kBlock;
        p = Plan{(int)t, (int)((K + t - 1) / t), (int)d, 1, (int)(d * t), 2, (int)d};
    } else {
        const int64_t c = cap / (2 * kBlock + 1);
        p = Plan{kBlock, (int)((K + kBlock - 1) / kBlock), (int)c, (int)((d + c - 1) / c), (int)(c * kBlock), 2, (int)c};
    }
    return p;
}

size_t plan_lds(const Plan &p) { return (size_t)kScratch + sizeof(float) * ((size_t)p.img * p.n_img + p.ycap); }

// img[j][k] = src[col0 + j][k0 + k] for ncols columns and nk draws; img has row stride ld, src row stride K
__device__ __forceinline__ void stage(float *img, int ld, const float *__restrict__ src, int64_t K, int col0, int ncols,
                                      int64_t k0, int nk, int tid) {
    for (int e = tid; e < ncols * nk; e += kThreads) {
        const int j = e / nk, k = e - j * nk;
        img[j * ld + k] = src[(int64_t)(col0 + j) * K + k0 + k];
    }
}

// acc[u] += sum_j (A[j][ia] - B[j][ib[u]])^2 over ncols columns; WITHY: accy += sum_j (A[j][ia] - Y[j])^2
template <bool WITHY>
__device__ __forceinline__ void block_sums(const float *A, const float *B, int ld, int ia, const int (&ib)[kPartners], int ncols,
                                           const float *Y, double (&acc)[kPartners], double &accy) {
    for (int j = 0; j < ncols; ++j) {
        const double xa = (double)A[j * ld + ia];
        const float *bj = B + j * ld;
#pragma unroll
        for (int u = 0; u < kPartners; ++u) {
            const double df = xa - (double)bj[ib[u]];
            acc[u] = fma(df, df, acc[u]);
        }
        if (WITHY) {
            const double dy = xa - (double)Y[j];
            accy = fma(dy, dy, accy);
        }
    }
}

template <int MODE> __device__ __forceinline__ double vpow(double a) {      // |a|^p as sqrt, identity or square, never pow
    const double m = fabs(a);
    return MODE == 0 ? sqrt(m) : (MODE == 1 ? m : m * m);
}

// this wave's share of sum_{i < j} (|y_i - y_j|^p - 1/K sum_k |x_ki - x_kj|^p)^2; X [d][ld] holds the K draws of every column
template <int MODE>
__device__ __forceinline__ double variogram_share(const float *X, int64_t ld, const float *__restrict__ yr, int d, int K, int wave,
                                                  int lane) {
    double total = 0.0;
    int64_t cnt = 0;
    for (int i = 0; i < d; ++i) {
        for (int j = i + 1; j < d; ++j, ++cnt) {
            if ((int)(cnt & 3) != wave) continue;
            const float *xi = X + (int64_t)i * ld, *xj = X + (int64_t)j * ld;
            double s = 0.0;
            for (int k = lane; k < K; k += 64) s += vpow<MODE>((double)xi[k] - (double)xj[k]);
#pragma unroll
            for (int w = 32; w >= 1; w >>= 1) s += __shfl_xor(s, w);
            const double t = vpow<MODE>((double)yr[i] - (double)yr[j]) - s / (double)K;
            total += t * t;
        }
    }
    return total;
}

__device__ __forceinline__ double variogram_of(int mode, const float *X, int64_t ld, const float *__restrict__ yr, int d, int K,
                                               int wave, int lane) {
    if (mode == 0) return variogram_share<0>(X, ld, yr, d, K, wave, lane);
    if (mode == 1) return variogram_share<1>(X, ld, yr, d, K, wave, lane);
    return variogram_share<2>(X, ld, yr, d, K, wave, lane);
}

__global__ void __launch_bounds__(kThreads)
k_joint(const float *__restrict__ xt, const float *__restrict__ y, int64_t n_rows, int d, int K, Plan p, int fair, int vmode,
        float *__restrict__ energy, float *__restrict__ spread, float *__restrict__ variogram) {
    extern __shared__ __attribute__((aligned(16))) unsigned char joint_lds[];
    double *r1 = reinterpret_cast<double *>(joint_lds), *r2 = r1 + kThreads;
    uint32_t *rf = reinterpret_cast<uint32_t *>(r2 + kThreads);
    float *Y = reinterpret_cast<float *>(rf + kThreads), *A = Y + p.ycap, *B = A + (p.n_img > 1 ? p.img : 0);
    const int tid = threadIdx.x, g = tid >> 6, a = tid & 63, ld = p.tile;
    const bool want_pairs = energy || spread;
    for (int64_t row = blockIdx.x; row < n_rows; row += gridDim.x) {
        const float *__restrict__ xr = xt + row * (int64_t)d * K;
        const float *__restrict__ yr = y + row * (int64_t)d;
        // 1 = a NaN among the draws or in y, 2 = an infinite draw, 4 = an infinite target
        uint32_t flags = 0;
        for (int64_t e = tid; e < (int64_t)d * K; e += kThreads) {
            const float v = xr[e];
            flags |= (v != v ? 1u : 0u) | (isinf(v) ? 2u : 0u);
        }
        for (int j = tid; j < d; j += kThreads) {
            const float v = yr[j];
            flags |= (v != v ? 1u : 0u) | (isinf(v) ? 4u : 0u);
        }
        double s1 = 0.0, s2 = 0.0;           // this thread's share of sum_k |x_k - y| and of sum_{k < l} |x_k - x_l|
        if (want_pairs || (variogram && p.n_img == 1)) {
            // (the image of plan (a) also feeds the variogram)
            for (int P = 0; P < p.n_tiles; ++P) {
                const int64_t k0P = (int64_t)P * p.tile;
                const int nkP = (int)(K - k0P < p.tile ? K - k0P : p.tile);
                for (int Q = P; Q < p.n_tiles; ++Q) {
                    const int64_t k0Q = (int64_t)Q * p.tile;
                    const int nkQ = (int)(K - k0Q < p.tile ? K - k0Q : p.tile);
                    const float *Bi = Q == P ? A : B;
                    const int nbP = (nkP + kBlock - 1) / kBlock, nbQ = (nkQ + kBlock - 1) / kBlock;
                    if (p.n_chunks == 1) {
                        // plans (a), (b): whole columns; tile P and y are staged when Q == P, tile Q > P into the second image
                        __syncthreads();
                        if (Q == P) {
                            stage(A, ld, xr, K, 0, d, k0P, nkP, tid);
                            if (P == 0)
                                for (int j = tid; j < d; j += kThreads) Y[j] = yr[j];
                        } else {
                            stage(B, ld, xr, K, 0, d, k0Q, nkQ, tid);
                        }
                        __syncthreads();
                        if (!want_pairs) continue;
                    }
                    for (int bi = 0; bi < nbP; ++bi) {
                        for (int bj = Q == P ? bi : 0; bj < nbQ; ++bj) {
                            const int a0 = bi * kBlock, b0 = bj * kBlock;
                            const int nav = nkP - a0 < kBlock ? nkP - a0 : kBlock, nbv = nkQ - b0 < kBlock ? nkQ - b0 : kBlock;
                            const bool withy = Q == P && bi == bj && g == 0;
                            const bool live = kPartners * g < nbv;               // (per wave) any partner of this wave in the block
                            // draws past the end are clamped onto the block's last one and left out below
                            const int ia = a0 + (a < nav ? a : nav - 1);
                            int ib[kPartners];
#pragma unroll
                            for (int u = 0; u < kPartners; ++u) {
                                const int b = kPartners * g + u;
                                ib[u] = b0 + (b < nbv ? b : nbv - 1);
                            }
                            double acc[kPartners], accy = 0.0;
#pragma unroll
                            for (int u = 0; u < kPartners; ++u) acc[u] = 0.0;
                            if (p.n_chunks == 1) {
                                if (withy) block_sums<true>(A, Bi, ld, ia, ib, d, Y, acc, accy);
                                else if (live) block_sums<false>(A, Bi, ld, ia, ib, d, Y, acc, accy);
                            } else {
                                // plan (c): one block per tile pair, the columns pass through in chunks
                                for (int ch = 0; ch < p.n_chunks; ++ch) {
                                    const int c0 = ch * p.cols, nc = d - c0 < p.cols ? d - c0 : p.cols;
                                    __syncthreads();
                                    stage(A, ld, xr, K, c0, nc, k0P, nkP, tid);
                                    if (Q != P) stage(B, ld, xr, K, c0, nc, k0Q, nkQ, tid);
                                    else
                                        for (int j = tid; j < nc; j += kThreads) Y[j] = yr[c0 + j];
                                    __syncthreads();
                                    if (withy) block_sums<true>(A, Bi, ld, ia, ib, nc, Y, acc, accy);
                                    else if (live) block_sums<false>(A, Bi, ld, ia, ib, nc, Y, acc, accy);
                                }
                            }
                            if (live && a < nav) {
                                const int64_t ka = k0P + a0 + a;
#pragma unroll
                                for (int u = 0; u < kPartners; ++u) {
                                    const int b = kPartners * g + u;
                                    if (b < nbv && ka < k0Q + b0 + b) s2 += sqrt(acc[u]);
                                }
                                if (withy) s1 += sqrt(accy);
                            }
                        }
                    }
                }
            }
        }
        r1[tid] = s1; r2[tid] = s2; rf[tid] = flags;
        __syncthreads();
        for (int s = kThreads / 2; s > 0; s >>= 1) {
            if (tid < s) { r1[tid] += r1[tid + s]; r2[tid] += r2[tid + s]; rf[tid] |= rf[tid + s]; }
            __syncthreads();
        }
        const uint32_t f = rf[0];
        if (tid == 0 && want_pairs) {
            const double kd = (double)K, dd = fair ? kd - 1.0 : kd;
            double sp = r2[0] / (kd * dd);                            // K = 1 and fair: 0 / 0
            double en = r1[0] / kd - sp;                              // an infinite target: +inf
            if (f & 3u) { sp = NAN; en = NAN; }                       // (the diagonal of the pair sum would form inf - inf)
            if (energy) energy[row] = (float)en;
            if (spread) spread[row] = (float)sp;
        }
        if (variogram) {
            __syncthreads();                                          // r1[0] has been read
            double v = 0.0;
            if (d > 1 && f == 0) {
                v = p.n_img == 1 ? variogram_of(vmode, A, ld, yr, d, K, g, a) : variogram_of(vmode, xr, K, yr, d, K, g, a);
            }
            if (a == 0) r1[g] = v;
            __syncthreads();
            if (tid == 0) {
                double tot = 2.0 * ((r1[0] + r1[1]) + (r1[2] + r1[3]));
                if (f) tot = NAN;                                     // the (i, i) terms form inf - inf; a NaN makes the row NaN
                variogram[row] = (float)tot;
            }
        }
        __syncthreads();
    }
}

int mode_of(double order) { return order == 0.5 ? 0 : (order == 1.0 ? 1 : (order == 2.0 ? 2 : -1)); }

}  // namespace

extern "C" {

int pfp_joint_tiling(int32_t d, int64_t k_total, pfp_joint_tile *out) {
    if (!out || d < 1 || k_total < 1) return PFP_EINVAL;
    if (k_total > PFP_MAX_QUANTILE_DRAWS) return PFP_EUNSUPPORTED;
    const Plan p = joint_plan(d, k_total);
    out->tile_draws = p.tile;
    out->n_tiles = p.n_tiles;
    out->chunk_cols = p.cols;
    out->n_chunks = p.n_chunks;
    out->budget_bytes = kBudget;
    out->lds_bytes = (int32_t)plan_lds(p);
    out->threads = kThreads;
    out->max_grid = kMaxGrid;
    return PFP_OK;
}

int pfp_joint_scores(void *stream, const float *xt, const float *y, int64_t n_rows, int32_t d, int64_t k_total,
                     int32_t fair, double variogram_order, float *energy, float *spread, float *variogram) {
    if (!xt || !y || n_rows < 0 || d < 1 || k_total < 1) return PFP_EINVAL;
    const int mode = variogram ? mode_of(variogram_order) : 0;
    if (mode < 0) return PFP_EINVAL;
    if (k_total > PFP_MAX_QUANTILE_DRAWS) return PFP_EUNSUPPORTED;
    if (n_rows == 0 || (!energy && !spread && !variogram)) return PFP_OK;
    const Plan p = joint_plan(d, k_total);
    const int grid = (int)(n_rows < kMaxGrid ? n_rows : kMaxGrid);
    hipLaunchKernelGGL(k_joint, dim3(grid), dim3(kThreads), plan_lds(p), (hipStream_t)stream, xt, y, n_rows, (int)d, (int)k_total,
                       p, (int)(fair != 0), mode, energy, spread, variogram);
    return (int)hipGetLastError();
}

}  // extern "C"
