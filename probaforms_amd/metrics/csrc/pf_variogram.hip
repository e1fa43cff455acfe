// pf_variogram.hip -- the per-row variogram score (Scheuerer & Hamill 2015) of K draws against the row's target TOGETHER WITH its
// derivative by every draw and by the target, for gfx950 (C ABI: pf_metrics.h, pfm_variogram_grad, pfm_variogram_plan).
//
// Per row, with draws x_k = X[k, row, :] (k < K), target y = Y[row, :], order p in {0.5, 1, 2} and weights w [d, d] (NULL: all 1):
//   v_ij = |y_i - y_j|^p,  m_ij = (1 / K) sum_k |x_ki - x_kj|^p,  r_ij = v_ij - m_ij,  t_ij = (w_ij + w_ji) r_ij
//   VS            = sum_{i < j} t_ij r_ij             (= sum_i sum_j w_ij r_ij^2: r is symmetric and its diagonal is 0)
//   d VS / d x_ki = -(2 / K) sum_j t_ij h(x_ki - x_kj),   d VS / d y_i = 2 sum_j t_ij h(y_i - y_j)
//   h(t) = 2 t (p = 2);  sgn t (p = 1);  sgn t / (2 sqrt|t|) (p = 0.5);  for p = 1 and 0.5 exactly 0 at t = 0 (the subgradient)
// |.|^p is a square root, the identity or a square, never pow; differences are taken on the values themselves.
//
// One kernel, k_vario, laid out as k_score (pf_scoregrad.hip).  A workgroup owns R consecutive rows: for every draw they are ONE
// contiguous run of R d doubles of X, staged into LDS with several loads in flight (a row's draws side by side, odd pitches), and
// for d <= 16 the gradients leave through the same image as the same runs.  Of the R rows, G are in flight at a time, each on S lanes
// (S the power of two >= K, at most 256; G = 256 / S unless LDS holds fewer).  The pair (i < j) has the index j (j - 1) / 2 + i.
//   pass A   the P = d (d - 1) / 2 pairs of a row go round its S lanes; where P < S the K draws are cut into T slices of ceil(K / T),
//            T = S / P, so that the lanes of a row of many draws and few features all work.  A lane sums |x_ki - x_kj|^p over its
//            slice in the order of k; the slices are summed in their order, divided by K, and t_ij is left in the row's table in LDS.
//            The value: a lane's t_ij r_ij in the order of its pairs, then the row's S lane sums in lane order by one lane.
//   grad_y   lane i mod S: sum over j != i in the order of j.
//   pass B   a lane owns one (row, draw) at a time.  d <= 16: the draw's features sit in registers and the pairs are walked ONCE,
//            j = 1 .. d - 1 and i < j: t h is added to feature i in its register and subtracted from feature j, whose sum takes the
//            place of x_kj in the image (nobody reads it after step j); the table reads are broadcasts.  d > 16: chunks of 16
//            features in registers, each summed over all j != i (a pair is then formed from both ends) and stored by the lane.
// Every order depends on (K, d) only and a row never meets another row: its outputs are the same bits at any position, for any n,
// in any call, whichever outputs are asked for.  d = 1 has no pair: k_vario_d1 writes the zeros (NaN where the row holds a NaN or
// an infinity, as the diagonal x - x of the definition gives).  No float atomics, no workspace traffic, nothing of size K d^2.
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
static_assert(PFM_VARIO_MAX_D == 64, "the LDS budget below is worked out for 64 features");
// a row at the limits: its draws at odd pitches (K d + K + 1 at the most), the target, the table, the lane sums
static_assert(8 * (PFM_SCORE_MAX_KD + PFM_SCORE_MAX_K + 1 + 64 + 2016 + 2 * NT) <= LDS_MAX, "a row at the limits must fit the LDS");

struct Plan {
    int64_t R, S, G, T, P, dp, rp, tp, pp, wgs, lds; // dp, rp: doubles between a row's draws, between rows; tp, pp: the pitches of
};                                                   // a row's table and of its slice sums (pp = 0: one slice, no slice sums)

// LDS doubles: the rows' draws and targets; per row in flight the table [P], the slice sums [T][P] and the lane sums [S]
int64_t lds_bytes(int64_t rows, int64_t G, int64_t d, int64_t S, int64_t rp, int64_t tp, int64_t pp) {
    return 8 * (rows * (rp + d) + G * (tp + pp + S));
}

int sizes_status(int64_t n, int64_t K, int64_t d) {
    if (n < 1 || K < 1 || d < 1 || n > (int64_t)INT32_MAX) return PFM_EINVAL;
    if (d > PFM_VARIO_MAX_D || K > PFM_SCORE_MAX_K || d > PFM_SCORE_MAX_KD / K) return PFM_EUNSUPPORTED;
    return PFM_OK;                                   // n K d 8 < 2^31 2^14 2^3: no size overflows
}

Plan plan_of(int64_t n, int64_t K, int64_t d) {
    Plan p;
    if (d == 1) {                                    // k_vario_d1: a lane per row, no LDS
        p.R = p.G = NT, p.S = p.T = 1, p.P = p.dp = p.rp = p.tp = p.pp = p.lds = 0;
        p.wgs = (n + NT - 1) / NT;
        return p;
    }
    p.S = 1;
    while (p.S < K && p.S < NT) p.S <<= 1;
    p.P = d * (d - 1) / 2;
    p.T = p.P < p.S ? p.S / p.P : 1;
    if (p.T > K) p.T = K;
    const int64_t per_slice = (K + p.T - 1) / p.T;
    p.T = (K + per_slice - 1) / per_slice;           // no empty slice
    p.dp = d | 1;
    p.rp = (K * p.dp) | 1;
    p.tp = p.P | 1;
    p.pp = p.T > 1 ? (p.T * p.P) | 1 : 0;
    p.G = NT / p.S;
    while (p.G > 1 && lds_bytes(p.G, p.G, d, p.S, p.rp, p.tp, p.pp) > LDS_MAX) p.G >>= 1;
    const int64_t limit = lds_bytes(p.G, p.G, d, p.S, p.rp, p.tp, p.pp) <= LDS_SOFT ? LDS_SOFT : LDS_MAX;
    const int64_t per_pass = lds_bytes(p.G, 0, d, p.S, p.rp, p.tp, p.pp), aux = lds_bytes(0, p.G, d, p.S, p.rp, p.tp, p.pp);
    int64_t passes = (limit - aux) / per_pass;
    const int64_t by_n = n / (MIN_WGS * p.G);
    if (passes > by_n) passes = by_n;
    if (passes < 1) passes = 1;
    p.R = p.G * passes;
    p.wgs = (n + p.R - 1) / p.R;
    p.lds = lds_bytes(p.R, p.G, d, p.S, p.rp, p.tp, p.pp);
    return p;
}

struct Args {
    const double *X, *Y, *W;
    int64_t n;
    int K, d, R, S, G, T, P, dp, rp, tp, pp;
    double k, scale_x;                               // K; -2 / K
    double *scores, *gx, *gy;
};

// a / b for 0 <= a < 2^24, inv_b = 1 / (float)b: the float quotient is off by one at the most
__device__ __forceinline__ int div_small(int a, int b, float inv_b) {
    int q = (int)((float)a * inv_b);
    if (q * b > a) --q;
    else if ((q + 1) * b <= a) ++q;
    return q;
}

// ORDER 0: p = 0.5; 1: p = 1; 2: p = 2
template <int ORDER>
__device__ __forceinline__ double power(double t) {  // |t|^p
    const double a = fabs(t);
    return ORDER == 0 ? sqrt(a) : ORDER == 1 ? a : a * a;
}

template <int ORDER>
__device__ __forceinline__ double slope(double t) {  // d |t|^p / d t, the subgradient 0 at t = 0; NaN for a NaN
    if (ORDER == 2) return 2.0 * t;
    if (ORDER == 1) return t > 0.0 ? 1.0 : t < 0.0 ? -1.0 : t;     // (t itself: 0, or the NaN)
    const double s = 0.5 / sqrt(fabs(t));
    return t > 0.0 ? s : t < 0.0 ? -s : t;           // no 0 times infinity: at t = 0 the quotient is not used
}

__device__ __forceinline__ int pair_index(int i, int j) {          // of the unordered pair, i != j
    return i < j ? j * (j - 1) / 2 + i : i * (i - 1) / 2 + j;
}

// MODE 0: the value alone (and grad_y, had it been asked for alone); 1: grad_x for d <= DC, through the LDS image; 2: grad_x for
// d > DC, chunk by chunk
template <int ORDER, int MODE>
__global__ void __launch_bounds__(NT) k_vario(Args a) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int K = a.K, d = a.d, G = a.G, S = a.S, T = a.T, P = a.P, dp = a.dp, rp = a.rp;
    double *const xs = lds;
    double *const ys = xs + (int64_t)a.R * rp;
    double *const tabs = ys + a.R * d;
    double *const parts = tabs + G * a.tp;
    double *const red = parts + G * a.pp;
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
    for (int e = tid; e < run; e += NT) ys[e] = a.Y[i0 * d + e];
    __syncthreads();

    const int r_in = tid % G, s = tid / G;
    double *const tab = tabs + r_in * a.tp;
    double *const part = parts + r_in * a.pp;
    const int per_slice = (K + T - 1) / T;
    for (int r0 = 0; r0 < rows; r0 += G) {           // (uniform: every barrier below is met by the whole workgroup)
        const int r = r0 + r_in;
        const bool row_ok = r < rows && s < S;
        const int64_t row = i0 + (row_ok ? r : 0);
        double *const xr = xs + (row_ok ? r : 0) * rp;
        const double *const yr = ys + (row_ok ? r : 0) * d;

        // ---- pass A: the slice sums of |x_ki - x_kj|^p; with one slice the pair is finished by the lane that summed it ----
        double vs = 0.0;
        for (int item = s; item < P * T; item += S) {
            if (!row_ok) break;
            const int t = item / P, p = item - t * P;
            int j = (int)(0.5f * (1.0f + sqrtf(8.0f * (float)p + 1.0f)));
            while (j * (j - 1) / 2 > p) --j;
            while ((j + 1) * j / 2 <= p) ++j;
            const int i = p - j * (j - 1) / 2;
            const int k1 = (t + 1) * per_slice < K ? (t + 1) * per_slice : K;
            double acc = 0.0;
            for (int k = t * per_slice; k < k1; ++k) acc = acc + power<ORDER>(xr[k * dp + i] - xr[k * dp + j]);
            if (T > 1) {
                part[item] = acc;
            } else {
                const double rij = power<ORDER>(yr[i] - yr[j]) - acc / a.k;
                const double tij = (a.W ? a.W[i * d + j] + a.W[j * d + i] : 2.0) * rij;
                tab[p] = tij;
                vs = vs + tij * rij;
            }
        }
        if (T > 1) {
            __syncthreads();
            for (int p = s; p < P; p += S) {
                if (!row_ok) break;
                int j = (int)(0.5f * (1.0f + sqrtf(8.0f * (float)p + 1.0f)));
                while (j * (j - 1) / 2 > p) --j;
                while ((j + 1) * j / 2 <= p) ++j;
                const int i = p - j * (j - 1) / 2;
                double acc = 0.0;
                for (int t = 0; t < T; ++t) acc = acc + part[t * P + p];
                const double rij = power<ORDER>(yr[i] - yr[j]) - acc / a.k;
                const double tij = (a.W ? a.W[i * d + j] + a.W[j * d + i] : 2.0) * rij;
                tab[p] = tij;
                vs = vs + tij * rij;
            }
        }
        if (s < S) red[s * G + r_in] = vs;
        __syncthreads();                             // the table and the lane sums are complete
        if (row_ok && s == 0) {
            double V = 0.0;
            for (int q = 0; q < S; ++q) V = V + red[q * G + r_in];
            a.scores[row] = V;
        }

        // ---- grad_y[i] = 2 sum_{j != i} t_ij h(y_i - y_j), j in order ----
        if (a.gy && row_ok)
            for (int i = s; i < d; i += S) {
                const double yi = yr[i];
                double acc = 0.0;
                for (int j = 0; j < d; ++j)
                    if (j != i) acc = acc + tab[pair_index(i, j)] * slope<ORDER>(yi - yr[j]);
                a.gy[row * d + i] = 2.0 * acc;
            }

        // ---- pass B: grad_x[k, row, :] = -(2 / K) sum_j t_ij h(x_ki - x_kj) ----
        if (MODE == 1 && row_ok)
            for (int k = s; k < K; k += S) {
                double *const x = xr + k * dp;
                double xi[DC], g[DC];
#pragma unroll
                for (int q = 0; q < DC; ++q) {
                    xi[q] = q < d ? x[q] : 0.0;
                    g[q] = 0.0;
                }
                for (int j = 1; j < d; ++j) {
                    const double xj = x[j];
                    const double *const tj = tab + j * (j - 1) / 2;
                    double back = 0.0;
#pragma unroll
                    for (int q = 0; q < DC - 1; ++q)
                        if (q < j) {
                            const double th = tj[q] * slope<ORDER>(xi[q] - xj);
                            g[q] = g[q] + th;
                            back = back - th;
                        }
                    x[j] = back;                     // feature j's sum over i < j takes the place of x_kj: nobody reads it again
                }
                x[0] = a.scale_x * g[0];
#pragma unroll
                for (int q = 1; q < DC; ++q)
                    if (q < d) x[q] = a.scale_x * (g[q] + x[q]);
            }
        if (MODE == 2 && row_ok)
            for (int k = s; k < K; k += S) {
                const double *const x = xr + k * dp;
                double *const out = a.gx + ((int64_t)k * a.n + row) * d;
                for (int c0 = 0; c0 < d; c0 += DC) {
                    double xi[DC], g[DC];
#pragma unroll
                    for (int q = 0; q < DC; ++q) {
                        xi[q] = c0 + q < d ? x[c0 + q] : 0.0;
                        g[q] = 0.0;
                    }
                    for (int j = 0; j < d; ++j) {
                        const double xj = x[j];
#pragma unroll
                        for (int q = 0; q < DC; ++q) {
                            const int i = c0 + q;
                            if (i < d && i != j) g[q] = g[q] + tab[pair_index(i, j)] * slope<ORDER>(xi[q] - xj);
                        }
                    }
#pragma unroll
                    for (int q = 0; q < DC; ++q)
                        if (c0 + q < d) out[c0 + q] = a.scale_x * g[q];
                }
            }
        __syncthreads();                             // the next pass takes the table, the slice sums and the lane sums
    }

    if (MODE == 1) {                                 // (the barrier that ends the last pass stands before this)
        for (int e = tid; e < K * run; e += NT) {
            const int k = div_small(e, run, inv_run), rem = e - k * run, r = div_small(rem, d, inv_d), j = rem - r * d;
            a.gx[((int64_t)k * a.n + i0) * d + rem] = xs[r * rp + k * dp + j];
        }
    }
}

// d = 1: every |x - x|^p of the diagonal is 0, or NaN where the row holds a NaN or an infinity; a lane per row, k in order
__global__ void __launch_bounds__(NT) k_vario_d1(const double *X, const double *Y, int64_t n, int K, double *scores, double *gx,
                                                 double *gy) {
    const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (i >= n) return;
    double z = Y[i] - Y[i];
    for (int k = 0; k < K; ++k) z = z + (X[(int64_t)k * n + i] - X[(int64_t)k * n + i]);
    scores[i] = z;
    if (gy) gy[i] = z;
    if (gx)
        for (int k = 0; k < K; ++k) gx[(int64_t)k * n + i] = z;
}

template <int ORDER, int MODE>
int launch(hipStream_t st, const Plan &p, const Args &a) {
    if (p.lds > LDS_SOFT)
        PFM_TRY(hipFuncSetAttribute((const void *)k_vario<ORDER, MODE>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds));
    hipLaunchKernelGGL((k_vario<ORDER, MODE>), dim3((unsigned)p.wgs), dim3(NT), (size_t)p.lds, st, a);
    PFM_TRY(hipGetLastError());
    return PFM_OK;
}

template <int ORDER>
int launch_mode(hipStream_t st, const Plan &p, const Args &a) {
    if (!a.gx) return launch<ORDER, 0>(st, p, a);
    return a.d <= DC ? launch<ORDER, 1>(st, p, a) : launch<ORDER, 2>(st, p, a);
}

}  // namespace

// ---- C ABI --------------------------------------------------------------------------------------------

extern "C" size_t pfm_variogram_grad_workspace_bytes(int64_t n, int64_t K, int64_t d) {
    return sizes_status(n, K, d) == PFM_OK ? WS_BYTES : 0;
}

extern "C" int pfm_variogram_plan(int64_t n, int64_t K, int64_t d, int64_t *plan) {
    if (!plan) return PFM_EINVAL;
    const int st = sizes_status(n, K, d);
    if (st != PFM_OK) return st;
    const Plan p = plan_of(n, K, d);
    plan[0] = p.R;
    plan[1] = p.S;
    plan[2] = p.lds;
    plan[3] = p.wgs;
    plan[4] = p.G;
    plan[5] = p.T;
    return PFM_OK;
}

extern "C" int pfm_variogram_grad(void *stream, const double *X, const double *Y, const double *W, int64_t n, int64_t K, int64_t d,
                                  double order, double *scores, double *grad_x, double *grad_y, void *workspace,
                                  size_t workspace_bytes) {
    if (!X || !Y || !scores) return PFM_EINVAL;
    const int st = sizes_status(n, K, d);
    if (st == PFM_EINVAL || !(order == 0.5 || order == 1.0 || order == 2.0)) return PFM_EINVAL;
    if (st != PFM_OK) return st;
    if (!workspace || workspace_bytes < WS_BYTES) return PFM_EWORKSPACE;
    const Plan p = plan_of(n, K, d);
    if (p.lds > LDS_MAX) return PFM_EUNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    if (d == 1) {
        hipLaunchKernelGGL(k_vario_d1, dim3((unsigned)p.wgs), dim3(NT), 0, s, X, Y, n, (int)K, scores, grad_x, grad_y);
        PFM_TRY(hipGetLastError());
        return PFM_OK;
    }
    Args a;
    a.X = X, a.Y = Y, a.W = W, a.n = n;
    a.K = (int)K, a.d = (int)d, a.R = (int)p.R, a.S = (int)p.S, a.G = (int)p.G, a.T = (int)p.T, a.P = (int)p.P;
    a.dp = (int)p.dp, a.rp = (int)p.rp, a.tp = (int)p.tp, a.pp = (int)p.pp;
    a.k = (double)K;
    a.scale_x = -2.0 / (double)K;
    a.scores = scores, a.gx = grad_x, a.gy = grad_y;
    return order == 0.5 ? launch_mode<0>(s, p, a) : order == 1.0 ? launch_mode<1>(s, p, a) : launch_mode<2>(s, p, a);
}
