// pf_sortscore.hip -- per (row, feature) series the CRPS of the series' K draws against its target TOGETHER WITH its derivative by
// every draw and by the target, and the pinball scores of the draws' empirical quantiles with what their derivative needs, from the
// SORTED series, for gfx950 (C ABI: pf_metrics.h, pfm_sort_score, pfm_sort_score_plan, pfm_pinball_grad).  pfm_score_grad at d = 1
// walks the K (K - 1) / 2 pairs of a series; here a series costs one sort and one pass.
//
// Per series s, with the shifted draws t_k = X[k, s] - Y[s] sorted by (value, draw index), t_(i) the i-th of them, lo_i / hi_i the
// first / last sorted position of the run of values equal to t_(i), c_i = lo_i + hi_i - K + 1 (the draws strictly below minus the
// draws strictly above; 2 i - K + 1 without ties) and D = K - 1 if fair else K:
//   crps = (1 / K) sum_i |t_(i)| - (1 / (K D)) sum_i c_i t_(i)
//   d crps / d x_k = (sgn(t_k) D - c_k) / (K D),   d crps / d y = -(sum_k sgn(t_k)) / K          sgn(0) = 0
// sum_i c_i = 0, so the shift by y changes nothing but the rounding: draws centred at 1e6 with unit spread lose nothing, as in the
// pair route.  Both numerators are integers formed exactly; one division per element.
//
// k_sort_score.  A workgroup takes G consecutive series (pfm_sort_score_plan).  For every draw their values are ONE contiguous run of
// G doubles of X: the runs are staged series-major into LDS as (float64 t, int32 draw), `pitch` = K | 1 entries apart, so that the
// staging (stride = pitch) and a lane per series meet every bank once.  Then
//   the sort    all G segments at once by seg_sort (pf_segsort.h): data-oblivious, no padding.
//   the runs    lo = max-scan of the run starts (i where t_(i - 1) != t_(i), else 0), hi = min-scan of the run ends, both over the
//               whole segment by doubling steps, log2 K of them whatever the values are: an all-equal series costs what a distinct
//               one costs.  A step updates in place: max and min are idempotent, so an entry that reads a neighbour already updated
//               in this step only takes in positions it would take in later.
//   the sums    a series is shared by L lanes (L the power of two >= K / 4, at most 256; 256 / L series in flight): lane j sums the
//               positions j, j + L, .. in order, the L partials are folded by a halving tree.  Every order depends on K only and a
//               series never meets another: its outputs are the same bits at any position, for any M, in any call.
//   the levels  Q_p - y = numpy's lerp of t_(i), t_(i + 1); pinball, side = p - [y < Q_p] and the two draws' indices.
//   grad_x      (sgn D - c) is left beside the entry as an int16 (at most 2 K - 1 = 16383); after the last read of the sorted
//               values the quotient goes THROUGH THE INDEX into the series' own segment, and the image leaves as the runs it came in.
// A series whose sum of |t| is NaN (a NaN among its draws or in y) gets NaN for its score and for all its gradient elements: the
// integer formula alone would hide it.  No float atomics, no workspace traffic.
//
// k_pinball_grad.  One thread per series adds, for q ascending, -g side (1 - frac) and -g side frac to the two draws pfm_sort_score
// named for level q in the zero-filled grad_x, and sums g side into grad_y.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "pf_common.h"
#include "pf_metrics.h"
#include "pf_segsort.h"

namespace {

constexpr int64_t LDS_MAX = 160 * 1024;              // one CU's LDS: what a single workgroup may take
constexpr int64_t ENTRY_BYTES = 16;                  // float64 value, int32 draw, int16 lo, int16 hi
constexpr int64_t SCRATCH_BYTES = NT * (8 + 8 + 4);  // a lane's two float64 partial sums and its count
constexpr int64_t ENTRIES = (64 * 1024 - SCRATCH_BYTES) / ENTRY_BYTES;   // entries a workgroup sorts at once while more than one
                                                     // series fits, 3776: 64 KiB of LDS with the scratch, two workgroups per CU
constexpr int SB = 8;                                // global loads a lane keeps in flight while it stages the draws
constexpr int MAXQ = PFM_SORT_MAX_Q;
constexpr size_t WS_BYTES = 256;                     // nothing is kept in the workspace: the least a caller can allocate
static_assert(ENTRY_BYTES * (PFM_SORT_MAX_K | 1) + SCRATCH_BYTES <= LDS_MAX, "a series at the limit must fit the LDS");
static_assert(2 * PFM_SORT_MAX_K - 1 <= INT16_MAX, "sgn D - c must fit an int16");

struct Plan {
    int64_t G, pitch, L, lds, wgs;                   // L: the lanes that share a series
};

int sizes_status(int64_t M, int64_t K, int64_t Q) {
    if (M < 1 || K < 1 || Q < 0 || M > (int64_t)INT32_MAX) return PFM_EINVAL;
    if (K > PFM_SORT_MAX_K || Q > MAXQ) return PFM_EUNSUPPORTED;
    return PFM_OK;                                   // M K 8 < 2^31 2^13 2^3: no size overflows
}

Plan plan_of(int64_t M, int64_t K) {
    Plan p;
    p.pitch = K | 1;
    p.G = ENTRIES / p.pitch;
    if (p.G < 1) p.G = 1;
    p.L = 1;
    while (p.L < NT && 4 * p.L < K) p.L <<= 1;
    p.lds = ENTRY_BYTES * p.G * p.pitch + SCRATCH_BYTES;
    p.wgs = (M + p.G - 1) / p.G;
    return p;
}

// the levels as the kernels take them: p, the lower order statistic i and frac of h = p (K - 1)
struct Levels {
    int Q;
    int i0[MAXQ];
    double p[MAXQ], frac[MAXQ];
};

int levels_of(const double *levels, int Q, int64_t K, Levels &l) {
    l.Q = Q;
    for (int q = 0; q < MAXQ; ++q) l.i0[q] = 0, l.p[q] = 0.0, l.frac[q] = 0.0;
    for (int q = 0; q < Q; ++q) {
        const double p = levels[q];
        if (!(p >= 0.0 && p <= 1.0)) return PFM_EINVAL;
        const double h = p * (double)(K - 1);
        double i = floor(h);
        if (i > (double)(K - 2)) i = (double)(K - 2);
        if (i < 0.0) i = 0.0;
        l.p[q] = p, l.i0[q] = (int)i, l.frac[q] = h - i;
    }
    return PFM_OK;
}

struct Args {
    const double *X, *Y;
    int64_t M;
    int K, G, pitch, L, D;
    double inv_k, inv_kd, k, kd;                     // 1 / K, 1 / (K D), K, K D
    double *crps, *gx, *gy, *pin, *side;
    int32_t *idx;
    Levels lv;
};

// a / b for 0 <= a < 2^24, inv_b = 1 / (float)b: the float quotient is off by one at the most
__device__ __forceinline__ int div_small(int a, int b, float inv_b) {
    int q = (int)((float)a * inv_b);
    if (q * b > a) --q;
    else if ((q + 1) * b <= a) ++q;
    return q;
}

__global__ void __launch_bounds__(NT) k_sort_score(Args a) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int K = a.K, G = a.G, pitch = a.pitch, L = a.L;
    double *const sv = lds;                                      // [G][pitch] t, sorted; at the end the gradients by draw
    int32_t *const si = (int32_t *)(sv + G * pitch);             // [G][pitch] the draws
    uint16_t *const lo = (uint16_t *)(si + G * pitch);           // [G][pitch] run starts, then sgn D - c as int16
    uint16_t *const hi = lo + G * pitch;                         // [G][pitch] run ends
    double *const r1 = (double *)(hi + G * pitch);               // [NT] partial sums of |t| (16 G pitch bytes in: aligned)
    double *const r2 = r1 + NT;                                  // [NT] of c t
    int *const rn = (int *)(r2 + NT);                            // [NT] of sgn t
    const int tid = threadIdx.x;
    const int64_t s0 = (int64_t)blockIdx.x * G;
    const int g = (int)(a.M - s0 < G ? a.M - s0 : G);            // the series of this workgroup
    const int total = K * g;                                     // <= max(ENTRIES, K): far below 2^24
    const float inv_g = 1.0f / (float)g, inv_K = 1.0f / (float)K;

    // ---- staging: entry e = k g + r is draw k of series s0 + r; SB loads in flight per lane, then their stores ----
    for (int e0 = tid; e0 < total; e0 += SB * NT) {
        double v[SB];
        int at[SB], kk[SB];
#pragma unroll
        for (int b = 0; b < SB; ++b) {
            const int e = e0 + b * NT;
            at[b] = -1;
            if (e < total) {
                const int k = div_small(e, g, inv_g), r = e - k * g;
                at[b] = r * pitch + k;
                kk[b] = k;
                v[b] = a.X[(int64_t)k * a.M + s0 + r] - a.Y[s0 + r];
            }
        }
#pragma unroll
        for (int b = 0; b < SB; ++b)
            if (at[b] >= 0) {
                sv[at[b]] = v[b];
                si[at[b]] = kk[b];
            }
    }
    __syncthreads();

    seg_sort(sv, si, g, K, pitch, tid, NT);

    // ---- the runs of equal values: entry e = r K + i is sorted position i of series r ----
    for (int e = tid; e < total; e += NT) {
        const int r = div_small(e, K, inv_K), i = e - r * K;
        const double *v = sv + r * pitch;
        lo[r * pitch + i] = (uint16_t)(i > 0 && v[i - 1] == v[i] ? 0 : i);
        hi[r * pitch + i] = (uint16_t)(i + 1 < K && v[i] == v[i + 1] ? K - 1 : i);
    }
    __syncthreads();
    for (int off = 1; off < K; off <<= 1) {
        for (int e = tid; e < total; e += NT) {
            const int r = div_small(e, K, inv_K), i = e - r * K, at = r * pitch + i;
            if (i >= off) {
                const uint16_t m = lo[at - off];
                if (m > lo[at]) lo[at] = m;
            }
            if (i + off < K) {
                const uint16_t m = hi[at + off];
                if (m < hi[at]) hi[at] = m;
            }
        }
        __syncthreads();
    }

    // ---- the sums, the levels and the gradients: 256 / L series in flight, L lanes each ----
    int16_t *const num = (int16_t *)lo;
    const int r_in = tid / L, j = tid - r_in * L, first = r_in * L;
    for (int r0 = 0; r0 < g; r0 += NT / L) {          // (uniform: every barrier below is met by the whole workgroup)
        const int r = r0 + r_in;
        const bool ok = r < g;
        const int base = (ok ? r : 0) * pitch;
        const int64_t s = s0 + (ok ? r : 0);
        double a1 = 0.0, a2 = 0.0;
        int ns = 0;
        if (ok)
            for (int i = j; i < K; i += L) {
                const double t = sv[base + i];
                const int c = (int)lo[base + i] + (int)hi[base + i] - K + 1;
                const int sg = (t > 0.0) - (t < 0.0);
                const double ct = (double)c * t;
                a1 = a1 + fabs(t);
                a2 = a2 + ct;
                ns += sg;
                num[base + i] = (int16_t)(sg * a.D - c);
            }
        r1[tid] = a1, r2[tid] = a2, rn[tid] = ns;
        __syncthreads();
        for (int h = L >> 1; h > 0; h >>= 1) {
            if (j < h) {
                r1[tid] = r1[tid] + r1[tid + h];
                r2[tid] = r2[tid] + r2[tid + h];
                rn[tid] = rn[tid] + rn[tid + h];
            }
            __syncthreads();
        }
        const double S1 = r1[first], S2 = r2[first];
        const bool bad = S1 != S1;                    // a NaN among the draws or in y
        if (ok && j == 0) {
            if (a.crps) a.crps[s] = a.inv_k * S1 - a.inv_kd * S2;
            if (a.gy) a.gy[s] = bad ? NAN : -((double)rn[first] / a.k);
        }
        if (ok)
            for (int q = 0; q < a.lv.Q; ++q) {        // level q on lane q mod L
                if ((q & (L - 1)) != j) continue;
                const int i0 = a.lv.i0[q], i1 = K > 1 ? i0 + 1 : i0;
                const double p = a.lv.p[q], fr = a.lv.frac[q];
                const double ta = sv[base + i0], tb = sv[base + i1], diff = tb - ta;
                double qt = ta + diff * fr;           // Q_p - y
                if (fr >= 0.5) qt = tb - diff * (1.0 - fr);
                if (diff == 0.0) qt = ta;
                const double sd = bad ? NAN : p - (0.0 < qt ? 1.0 : 0.0);
                const int64_t o = (int64_t)q * a.M + s;
                if (a.pin) a.pin[o] = bad ? NAN : -qt * sd;
                if (a.side) a.side[o] = sd;
                if (a.idx) {
                    a.idx[2 * o] = si[base + i0];
                    a.idx[2 * o + 1] = si[base + i1];
                }
            }
        __syncthreads();                              // nobody reads this pass's sorted values or sums any more
        if (a.gx && ok)
            for (int i = j; i < K; i += L) sv[base + si[base + i]] = bad ? NAN : (double)num[base + i] / a.kd;
    }

    if (a.gx) {
        __syncthreads();
        for (int e = tid; e < total; e += NT) {
            const int k = div_small(e, g, inv_g), r = e - k * g;
            a.gx[(int64_t)k * a.M + s0 + r] = sv[r * pitch + k];
        }
    }
}

struct GradArgs {
    const int32_t *idx;
    const double *side, *g;
    int64_t M;
    int K, Q;
    double frac[MAXQ];
    double *gx, *gy;
};

__global__ void __launch_bounds__(NT) k_pinball_grad(GradArgs a) {
    const int64_t s = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (s >= a.M) return;
    double acc = 0.0;
    for (int q = 0; q < a.Q; ++q) {
        const int64_t o = (int64_t)q * a.M + s;
        const double w = a.g[o] * a.side[o];
        acc = acc + w;
        if (a.gx) {
            int i0 = a.idx[2 * o], i1 = a.idx[2 * o + 1];
            i0 = i0 < 0 ? 0 : i0 >= a.K ? a.K - 1 : i0;          // what pfm_sort_score wrote is in range; nothing else leaves grad_x
            i1 = i1 < 0 ? 0 : i1 >= a.K ? a.K - 1 : i1;
            const double fr = a.frac[q], wa = -w * (1.0 - fr), wb = -w * fr;
            double *const pa = a.gx + (int64_t)i0 * a.M + s, *const pb = a.gx + (int64_t)i1 * a.M + s;
            *pa = *pa + wa;
            *pb = *pb + wb;
        }
    }
    if (a.gy) a.gy[s] = acc;
}

}  // namespace

// ---- C ABI --------------------------------------------------------------------------------------------

extern "C" size_t pfm_sort_score_workspace_bytes(int64_t M, int64_t K, int64_t n_levels) {
    return sizes_status(M, K, n_levels) == PFM_OK ? WS_BYTES : 0;
}

extern "C" int pfm_sort_score_plan(int64_t M, int64_t K, int64_t *plan) {
    if (!plan) return PFM_EINVAL;
    const int st = sizes_status(M, K, 0);
    if (st != PFM_OK) return st;
    const Plan p = plan_of(M, K);
    plan[0] = p.G;
    plan[1] = p.pitch;
    plan[2] = p.lds;
    plan[3] = p.wgs;
    return PFM_OK;
}

extern "C" int pfm_sort_score(void *stream, const double *X, const double *Y, int64_t M, int64_t K, int fair, const double *levels,
                              int n_levels, double *crps, double *grad_x, double *grad_y, double *pinball, double *side,
                              int32_t *idx, void *workspace, size_t workspace_bytes) {
    if (!X || !Y) return PFM_EINVAL;
    const int st = sizes_status(M, K, n_levels);
    if (st == PFM_EINVAL || (fair && K == 1)) return PFM_EINVAL;
    if (n_levels > 0 ? !levels : (pinball || side || idx)) return PFM_EINVAL;
    if (!crps && !grad_x && !grad_y && !pinball && !side && !idx) return PFM_EINVAL;
    if (st != PFM_OK) return st;
    Args a;
    const int lst = levels_of(levels, n_levels, K, a.lv);
    if (lst != PFM_OK) return lst;
    if (!workspace || workspace_bytes < WS_BYTES) return PFM_EWORKSPACE;
    const Plan p = plan_of(M, K);
    a.X = X, a.Y = Y, a.M = M;
    a.K = (int)K, a.G = (int)p.G, a.pitch = (int)p.pitch, a.L = (int)p.L, a.D = (int)(fair ? K - 1 : K);
    a.k = (double)K;
    a.kd = (double)K * (double)a.D;
    a.inv_k = 1.0 / a.k;
    a.inv_kd = 1.0 / a.kd;
    a.crps = crps, a.gx = grad_x, a.gy = grad_y, a.pin = pinball, a.side = side, a.idx = idx;
    if (p.lds > 64 * 1024)
        PFM_TRY(hipFuncSetAttribute((const void *)k_sort_score, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds));
    hipLaunchKernelGGL(k_sort_score, dim3((unsigned)p.wgs), dim3(NT), (size_t)p.lds, (hipStream_t)stream, a);
    PFM_TRY(hipGetLastError());
    return PFM_OK;
}

extern "C" int pfm_pinball_grad(void *stream, const int32_t *idx, const double *side, const double *g, const double *levels,
                                int n_levels, int64_t M, int64_t K, double *grad_x, double *grad_y, void *workspace,
                                size_t workspace_bytes) {
    if (!idx || !side || !g || !levels || n_levels < 1 || (!grad_x && !grad_y)) return PFM_EINVAL;
    const int st = sizes_status(M, K, n_levels);
    if (st != PFM_OK) return st;
    Levels lv;
    const int lst = levels_of(levels, n_levels, K, lv);
    if (lst != PFM_OK) return lst;
    if (!workspace || workspace_bytes < WS_BYTES) return PFM_EWORKSPACE;
    GradArgs a;
    a.idx = idx, a.side = side, a.g = g, a.M = M, a.K = (int)K, a.Q = n_levels;
    for (int q = 0; q < MAXQ; ++q) a.frac[q] = lv.frac[q];
    a.gx = grad_x, a.gy = grad_y;
    hipStream_t s = (hipStream_t)stream;
    if (grad_x) PFM_TRY(hipMemsetAsync(grad_x, 0, sizeof(double) * (size_t)K * (size_t)M, s));
    hipLaunchKernelGGL(k_pinball_grad, dim3((unsigned)((M + NT - 1) / NT)), dim3(NT), 0, s, a);
    PFM_TRY(hipGetLastError());
    return PFM_OK;
}
