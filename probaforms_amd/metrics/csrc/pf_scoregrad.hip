// pf_scoregrad.hip -- the per-row energy score of K draws against the row's target TOGETHER WITH its derivative by every draw and
// by the target, for training a conditional sampler on it, for gfx950 (C ABI: pf_metrics.h, pfm_score_grad, pfm_score_plan).
//
// Per row i, with draws x_k = X[k, i, :] (k < K), target y = Y[i, :] and D = K - 1 if fair else K:
//   T1 = (1 / K) sum_k |x_k - y|,  spread = 1 / (K D) sum_{k < l} |x_k - x_l|,  score = T1 - spread
//   d score / d x_k = (1 / K) c_k (x_k - y) - (1 / (K D)) sum_l c_kl (x_k - x_l),  d score / d y = -(1 / K) sum_k c_k (x_k - y)
// c = 1 / distance, and exactly 0 where the squared distance is 0.  Differences are taken on the values themselves and the squared
// distance is fma(df, df, acc) over the features in order, as pf_pairgrad.hip does; no norm / dot-product identity.
//
// One kernel, k_score.  A workgroup owns R consecutive rows.  For every draw k its R rows are ONE contiguous run of R d doubles of
// X: the runs are staged into LDS (a row's draws side by side, pitches odd where they fit: a lane per draw then reads conflict-free)
// and, for d <= 16, the gradients leave through the same image as the same runs.  Of the R rows, G are in flight at a time, each
// on S lanes (S the power of two >= K, at most 256; G = 256 / S unless LDS holds fewer): lane (row, s) owns the draws s, s + S, ..
// (U = ceil(K / S) <= 4 of them), so K = 4 packs 64 rows into a workgroup and K = 1024 gives every lane four draws of one row.
// pfm_score_plan says what a shape gets.
//   the pairs   offset o = 1 .. K / 2: the owner of draw k forms the distance to draw (k + o) mod K, ONCE per unordered pair (at
//               2 o = K only the lower half does), adds it to its spread sum and c (x_k - x_l) to its gradient, and leaves c in
//               LDS; after the barrier the owner of draw (k + o) mod K reads c and adds c (x_l - x_k) to its own.  A lane's
//               gradient of d <= 16 features stays in registers for the whole walk (forms for 1, 4 and 16 features); the value
//               alone needs no exchange and no barrier.  Wider rows walk the pairs once per chunk of
//               16 features (the distance is then re-formed per chunk, as pfm_pair_grad's feature chunks do) and store the chunk
//               to grad_x themselves.
//   the sums    a lane's terms in the order of o, forward before backward; the row's S lane sums of T1 and of the spread in lane
//               order by one lane; grad_y[j] over k in order by lane j mod S.  Every order depends on (K, d) only and a row never
//               meets another row: its outputs are the same bits at any position, for any n, in any call.
// No float atomics, no workspace traffic, nothing of size K^2 anywhere.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "pf_common.h"
#include "pf_metrics.h"

namespace {

constexpr int DC = 16;                               // features of a gradient chunk: a lane's registers
constexpr int64_t LDS_MAX = 160 * 1024;              // one CU's LDS: what a single workgroup may take
constexpr int64_t LDS_SOFT = 64 * 1024;              // what a workgroup takes while more rows would still fit: two per CU
constexpr int64_t MIN_WGS = 256;                     // R shrinks (down to G) while n rows make fewer workgroups than this
constexpr int SB = 8;                                // global loads a lane keeps in flight while it stages the draws
constexpr size_t WS_BYTES = 256;                     // nothing is kept in the workspace: the least a caller can allocate
static_assert(PFM_SCORE_MAX_K <= 4 * NT, "a lane owns at most four draws");
static_assert(8 * (PFM_SCORE_MAX_KD + 3 * PFM_SCORE_MAX_K + 2 * NT) <= LDS_MAX, "a row at the limits must fit the LDS");

struct Plan {
    int64_t R, S, G, U, dp, rp, wgs, lds;            // dp: doubles between a row's draws in LDS; rp: between rows
    int y_lds;                                       // the targets are staged too (else read from global memory)
};

// LDS doubles: the rows' draws, their targets, per row in flight c_k [K], the pair exchange [2][K] and the lane sums [2][S]
int64_t lds_bytes(int64_t rows, int64_t G, int64_t K, int64_t d, int64_t S, int64_t rp, int y_lds) {
    return 8 * (rows * rp + (y_lds ? rows * d : 0) + 3 * G * K + 2 * G * S);
}

int sizes_status(int64_t n, int64_t K, int64_t d) {
    if (n < 1 || K < 1 || d < 1 || n > (int64_t)INT32_MAX) return PFM_EINVAL;
    if (K > PFM_SCORE_MAX_K || d > PFM_SCORE_MAX_KD / K) return PFM_EUNSUPPORTED;
    return PFM_OK;                                   // n K d 8 < 2^31 2^14 2^3: no size overflows
}

Plan plan_of(int64_t n, int64_t K, int64_t d) {
    Plan p;
    p.S = 1;
    while (p.S < K && p.S < NT) p.S <<= 1;
    p.U = (K + p.S - 1) / p.S;
    p.dp = d | 1;
    p.rp = (K * p.dp) | 1;
    p.y_lds = 1;
    if (lds_bytes(1, 1, K, d, p.S, p.rp, 1) > LDS_MAX) {            // no room for odd pitches
        p.dp = d;
        p.rp = K * d;
    }
    if (lds_bytes(1, 1, K, d, p.S, p.rp, 1) > LDS_MAX) p.y_lds = 0; // nor for the target (K small, d in the thousands)
    p.G = NT / p.S;
    while (p.G > 1 && lds_bytes(p.G, p.G, K, d, p.S, p.rp, p.y_lds) > LDS_MAX) p.G >>= 1;
    const int64_t limit = lds_bytes(p.G, p.G, K, d, p.S, p.rp, p.y_lds) <= LDS_SOFT ? LDS_SOFT : LDS_MAX;
    const int64_t per_pass = lds_bytes(p.G, 0, K, d, p.S, p.rp, p.y_lds), aux = lds_bytes(0, p.G, K, d, p.S, p.rp, p.y_lds);
    int64_t passes = (limit - aux) / per_pass;
    const int64_t by_n = n / (MIN_WGS * p.G);
    if (passes > by_n) passes = by_n;
    if (passes < 1) passes = 1;
    p.R = p.G * passes;
    p.wgs = (n + p.R - 1) / p.R;
    p.lds = lds_bytes(p.R, p.G, K, d, p.S, p.rp, p.y_lds);
    return p;
}

struct Args {
    const double *X, *Y;
    int64_t n;
    int K, d, R, S, G, dp, rp, y_lds;
    double inv_k, inv_kd;                            // 1 / K, 1 / (K D)
    double *scores, *spread, *gx, *gy;
};

// a / b for 0 <= a < 2^24, inv_b = 1 / (float)b: the float quotient is off by one at the most
__device__ __forceinline__ int div_small(int a, int b, float inv_b) {
    int q = (int)((float)a * inv_b);
    if (q * b > a) --q;
    else if ((q + 1) * b <= a) ++q;
    return q;
}

// MODE 0: the value alone; 1: gradients, d <= QF <= DC (a draw's features and gradient in registers, grad_x leaves through LDS);
// 2: gradients, d > DC (one pair walk per chunk of QF = DC features).  QF: the features that get registers, 1, 4 or DC
template <int U, int MODE, int QF>
__global__ void __launch_bounds__(NT) k_score(Args a) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int K = a.K, d = a.d, G = a.G, S = a.S, dp = a.dp, rp = a.rp;
    double *const xs = lds;
    double *const ys = xs + (int64_t)a.R * rp;
    double *const c0 = ys + (a.y_lds ? a.R * d : 0);
    double *const cs = c0 + G * K;
    double *const red = cs + 2 * G * K;
    const int tid = threadIdx.x;
    const int64_t i0 = (int64_t)blockIdx.x * a.R;
    const int rows = (int)(a.n - i0 < a.R ? a.n - i0 : a.R);
    const int run = rows * d;                        // doubles of one draw's rows: contiguous in X and in grad_x

    const float inv_run = 1.0f / (float)run, inv_d = 1.0f / (float)d;   // K run < 2^15 (the image fits the LDS)
    for (int e0 = tid; e0 < K * run; e0 += SB * NT) {   // SB loads in flight per lane, then their stores
        double v[SB];
        int at[SB];
#pragma unroll
        for (int b = 0; b < SB; ++b) {
            const int e = e0 + b * NT;
            at[b] = -1;
            if (e < K * run) {
                const int k = div_small(e, run, inv_run), rem = e - k * run, r = div_small(rem, d, inv_d), j = rem - r * d;
                at[b] = r * rp + k * dp + j;
                v[b] = a.X[((int64_t)k * a.n + i0) * d + rem];
            }
        }
#pragma unroll
        for (int b = 0; b < SB; ++b)
            if (at[b] >= 0) xs[at[b]] = v[b];
    }
    if (a.y_lds)
        for (int e = tid; e < run; e += NT) ys[e] = a.Y[i0 * d + e];
    __syncthreads();

    const int r_in = tid % G, s = tid / G;
    double *const c0r = c0 + r_in * K;
    for (int r0 = 0; r0 < rows; r0 += G) {           // (uniform: every barrier below is met by the whole workgroup)
        const int r = r0 + r_in;
        const bool row_ok = r < rows && s < S;
        const int64_t i = i0 + (row_ok ? r : 0);
        double *const xr = xs + (row_ok ? r : 0) * rp;
        const double *const yr = a.y_lds ? ys + (row_ok ? r : 0) * d : a.Y + i * d;

        // ---- the target: c_k, T1's terms ----
        bool ok[U];
        double c0k[U], xk[U][MODE == 1 ? QF : 1];
        double t1 = 0.0, sp = 0.0;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int k = s + u * S;
            ok[u] = row_ok && k < K;
            c0k[u] = 0.0;
            if (ok[u]) {
                const double *x = xr + k * dp;
                double dd = 0.0;
                if (MODE == 1) {
#pragma unroll
                    for (int q = 0; q < QF; ++q)
                        if (q < d) {
                            xk[u][q] = x[q];
                            const double df = xk[u][q] - yr[q];
                            dd = fma(df, df, dd);
                        }
                } else {
                    for (int j = 0; j < d; ++j) {
                        const double df = x[j] - yr[j];
                        dd = fma(df, df, dd);
                    }
                }
                const double sq = sqrt(dd);
                c0k[u] = dd == 0.0 ? 0.0 : 1.0 / sq;
                t1 = t1 + sq;
                c0r[k] = c0k[u];
            }
        }
        __syncthreads();

        // ---- grad_y[j] = -(1 / K) sum_k c_k (x_k[j] - y[j]), k in order ----
        if (MODE != 0 && a.gy && row_ok)
            for (int j = s; j < d; j += S) {
                const double yj = yr[j];
                double acc = 0.0;
                for (int k = 0; k < K; ++k) acc = fma(c0r[k], xr[k * dp + j] - yj, acc);
                a.gy[i * d + j] = -(a.inv_k * acc);
            }

        // ---- the pairs ----
        double g[U][MODE == 0 ? 1 : QF];
        for (int jc = 0; jc < (MODE == 2 && a.gx ? d : 1); jc += QF) {   // (grad_y alone: one walk, for the spread)
            if (MODE != 0) {
#pragma unroll
                for (int u = 0; u < U; ++u)
#pragma unroll
                    for (int q = 0; q < QF; ++q) g[u][q] = 0.0;
            }
            for (int o = 1; 2 * o <= K; ++o) {
                double *const cb = cs + ((o & 1) * G + r_in) * K;
                const bool half = 2 * o == K;        // each pair at this offset is met from both ends: the lower end forms it
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int k = s + u * S;
                    if (ok[u] && (!half || 2 * k < K)) {
                        const int l = k + o < K ? k + o : k + o - K;
                        const double *x = xr + k * dp, *z = xr + l * dp;
                        double dd = 0.0, c;
                        if (MODE == 1) {
                            double df[QF];
#pragma unroll
                            for (int q = 0; q < QF; ++q)
                                if (q < d) {
                                    df[q] = xk[u][q] - z[q];
                                    dd = fma(df[q], df[q], dd);
                                }
                            const double sq = sqrt(dd);
                            c = dd == 0.0 ? 0.0 : 1.0 / sq;
                            sp = sp + sq;
#pragma unroll
                            for (int q = 0; q < QF; ++q)
                                if (q < d) g[u][q] = fma(c, df[q], g[u][q]);
                        } else {
                            for (int j = 0; j < d; ++j) {
                                const double df = x[j] - z[j];
                                dd = fma(df, df, dd);
                            }
                            const double sq = sqrt(dd);
                            c = dd == 0.0 ? 0.0 : 1.0 / sq;
                            if (jc == 0) sp = sp + sq;
                            if (MODE == 2) {
#pragma unroll
                                for (int q = 0; q < QF; ++q)
                                    if (jc + q < d) g[u][q] = fma(c, x[jc + q] - z[jc + q], g[u][q]);
                            }
                        }
                        if (MODE != 0) cb[k] = c;
                    }
                }
                if (MODE != 0) {
                    __syncthreads();
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const int k = s + u * S;
                        if (ok[u] && (!half || 2 * k >= K)) {
                            const int m = k - o >= 0 ? k - o : k - o + K;
                            const double *x = xr + k * dp, *z = xr + m * dp;
                            const double c = cb[m];
#pragma unroll
                            for (int q = 0; q < QF; ++q) {
                                if (MODE == 1) {
                                    if (q < d) g[u][q] = fma(c, xk[u][q] - z[q], g[u][q]);
                                } else {
                                    if (jc + q < d) g[u][q] = fma(c, x[jc + q] - z[jc + q], g[u][q]);
                                }
                            }
                        }
                    }
                }
            }
            // ---- d score / d x_k of this chunk; d > DC: stored by the lane, 16 consecutive doubles ----
            if (MODE == 2) {
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int k = s + u * S;
                    if (ok[u] && a.gx) {
                        const double *x = xr + k * dp;
                        double *out = a.gx + ((int64_t)k * a.n + i) * d;
#pragma unroll
                        for (int q = 0; q < QF; ++q)
                            if (jc + q < d)
                                out[jc + q] = a.inv_k * (c0k[u] * (x[jc + q] - yr[jc + q])) - a.inv_kd * g[u][q];
                    }
                }
                __syncthreads();                     // the next chunk's first step takes the exchange buffer of this one's last
            }
        }

        // ---- the row's sums, lane by lane in order ----
        if (s < S) {
            red[r_in * S + s] = t1;
            red[(G + r_in) * S + s] = sp;
        }
        __syncthreads();                             // and nobody reads this pass's draws any more
        if (row_ok && s == 0) {
            double T = 0.0, P = 0.0;
            for (int q = 0; q < S; ++q) {
                T = T + red[r_in * S + q];
                P = P + red[(G + r_in) * S + q];
            }
            const double t = a.inv_k * T, v = a.inv_kd * P;
            a.scores[i] = t - v;
            if (a.spread) a.spread[i] = v;
        }
        if (MODE == 1 && a.gx) {                     // the gradient takes the draw's place in the image
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (ok[u]) {
                    double *x = xr + (s + u * S) * dp;
#pragma unroll
                    for (int q = 0; q < QF; ++q)
                        if (q < d) x[q] = a.inv_k * (c0k[u] * (xk[u][q] - yr[q])) - a.inv_kd * g[u][q];
                }
        }
    }

    if (MODE == 1 && a.gx) {
        __syncthreads();
        for (int e = tid; e < K * run; e += NT) {
            const int k = div_small(e, run, inv_run), rem = e - k * run, r = div_small(rem, d, inv_d), j = rem - r * d;
            a.gx[((int64_t)k * a.n + i0) * d + rem] = xs[r * rp + k * dp + j];
        }
    }
}

template <int U, int MODE, int QF>
int launch(hipStream_t st, const Plan &p, const Args &a) {
    if (p.lds > LDS_SOFT)
        PFM_TRY(hipFuncSetAttribute((const void *)k_score<U, MODE, QF>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds));
    hipLaunchKernelGGL((k_score<U, MODE, QF>), dim3((unsigned)p.wgs), dim3(NT), (size_t)p.lds, st, a);
    PFM_TRY(hipGetLastError());
    return PFM_OK;
}

template <int U>
int launch_mode(hipStream_t st, bool grad, const Plan &p, const Args &a) {
    if (!grad) return launch<U, 0, 1>(st, p, a);
    if (a.d == 1) return launch<U, 1, 1>(st, p, a);
    if (a.d <= 4) return launch<U, 1, 4>(st, p, a);
    if (a.d <= DC) return launch<U, 1, DC>(st, p, a);
    return launch<U, 2, DC>(st, p, a);
}

}  // namespace

// ---- C ABI --------------------------------------------------------------------------------------------

extern "C" size_t pfm_score_grad_workspace_bytes(int64_t n, int64_t K, int64_t d) {
    return sizes_status(n, K, d) == PFM_OK ? WS_BYTES : 0;
}

extern "C" int pfm_score_plan(int64_t n, int64_t K, int64_t d, int64_t *plan) {
    if (!plan) return PFM_EINVAL;
    const int st = sizes_status(n, K, d);
    if (st != PFM_OK) return st;
    const Plan p = plan_of(n, K, d);
    plan[0] = p.R;
    plan[1] = p.S;
    plan[2] = p.lds;
    plan[3] = p.wgs;
    return PFM_OK;
}

extern "C" int pfm_score_grad(void *stream, const double *X, const double *Y, int64_t n, int64_t K, int64_t d, int fair,
                              double *scores, double *spread, double *grad_x, double *grad_y, void *workspace,
                              size_t workspace_bytes) {
    if (!X || !Y || !scores) return PFM_EINVAL;
    const int st = sizes_status(n, K, d);
    if (st == PFM_EINVAL || (fair && K == 1)) return PFM_EINVAL;
    if (st != PFM_OK) return st;
    if (!workspace || workspace_bytes < WS_BYTES) return PFM_EWORKSPACE;
    const Plan p = plan_of(n, K, d);
    if (p.lds > LDS_MAX) return PFM_EUNSUPPORTED;
    Args a;
    a.X = X, a.Y = Y, a.n = n;
    a.K = (int)K, a.d = (int)d, a.R = (int)p.R, a.S = (int)p.S, a.G = (int)p.G, a.dp = (int)p.dp, a.rp = (int)p.rp, a.y_lds = p.y_lds;
    a.inv_k = 1.0 / (double)K;
    a.inv_kd = 1.0 / ((double)K * (double)(fair ? K - 1 : K));
    a.scores = scores, a.spread = spread, a.gx = grad_x, a.gy = grad_y;
    const bool grad = grad_x || grad_y;
    hipStream_t s = (hipStream_t)stream;
    return p.U == 1 ? launch_mode<1>(s, grad, p, a) : p.U == 2 ? launch_mode<2>(s, grad, p, a) : launch_mode<4>(s, grad, p, a);
}
