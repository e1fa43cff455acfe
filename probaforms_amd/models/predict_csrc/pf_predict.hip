// pf_predict.hip -- libpf_predict.so (C ABI: pf_predict.h): K prior draws per condition row through the inverse
// RealNVP flow, reduced across the draws on the device (gfx950).
//
// k_draw: one WAVE (a 64-thread workgroup) owns one condition row for the whole launch, so every (row, column) of
// `state` has exactly one owner and nothing is summed with atomics.
//   * the 16 columns of an MFMA tile are 16 DRAWS of that row; a pass pushes NT = 1, 2 or 4 such tiles (16 .. 64
//     draws) through the stack at once so that a weight fragment loaded once feeds NT MFMAs;
//   * every Linear is computed transposed, out^T[out x draws] = W[out x in] . act^T[in x draws], as
//     v_mfma_f32_16x16x4_f32: A = weights read from the flat parameter buffer as they lie (lane (q, i) holds
//     W[16m + i][4ks + q]), B = the activations' LDS image [feature][RS], the accumulator (bias, activation) goes back
//     to the image of the next Linear;
//   * the row's condition enters every net only through its first Linear, and is the same for all K draws: the wave
//     forms cb = b1 + W1[:, d:] . c[r] once per (layer, net) when it picks the row up, keeps the 2 L vectors in LDS
//     and uses them as the first Linear's bias -- the MFMA contraction of that Linear runs over the d data columns
//     only, and c[r] is read once instead of K times;
//   * z is drawn per (draw, global row, 4 columns) with the counter-based Philox / Box-Muller of rnvp_prior.h straight
//     into the image (never written to memory), or read from a caller's z[k][global row][:];
//   * after the last layer the lanes reduce each column's 16 draws with a fixed xor butterfly (float64 sums of
//     x - shift and its square, float32 min / max) and one lane folds the tile into the row's running state in LDS;
//     the state is read once when the row is picked up and written once when it is done.
// A draw's value depends on nothing but its own column of the image, and the order of the float64 sums is fixed by
// (k_lo, k_cnt) alone: rows split over calls reproduce one call bit for bit.
//
// k_quantiles / k_scores: one 256-thread workgroup per (row, column) series of the transposed draws sorts it in LDS; quantiles,
// and the CRPS / PIT / pinball scores against an observed target, are one pass over the sorted series (see the kernels).
//
// k_joint (pfp_joint_scores, pfp_joint_tiling): pf_joint.hip, the second object of this library.
#include "../../csrc/rnvp_common.h"
#include "../../csrc/rnvp_generic_net.h"
#include "../../csrc/rnvp_prior.h"
#include "pf_drawfold.h"

#include <math.h>

namespace {

using rnvp::KShape;
using namespace drawfold;          // State, f4, mfma16, min_nan / max_nan, row_stride, load_state, emit_fold, store_state

constexpr int kLdsWide = 40 * 1024;        // a pass of more than 16 draws only while four waves still fit a CU

// float offsets of one wave's LDS images
struct Geo {
    int oX, oXM, oT, oS, oH0, oH1, oCB, oST, floats;
};

Geo make_geo(const KShape &s, int RS) {
    const int dp = (s.d + 3) / 4 * 4, hp = (s.hmax + 3) / 4 * 4;
    Geo g;
    int o = 0;
    g.oX = o;  o += dp * RS;
    g.oXM = o; o += dp * RS;
    g.oT = o;  o += dp * RS;
    g.oS = o;  o += dp * RS;
    g.oH0 = o; o += hp * RS;
    g.oH1 = o; o += (s.nh > 1 ? hp : 0) * RS;
    g.oCB = o; o += s.L * 2 * s.nout[0];
    o = (o + 3) / 4 * 4;
    g.oST = o; o += s.d * kStateFloats;
    g.floats = o;
    return g;
}

__device__ __forceinline__ float mask_of(const KShape &s, const uint8_t *__restrict__ masks, int l, int j) {
    if (masks) return (float)masks[l * s.d + j];
    return (float)((j + l + (s.alt == 2 ? 1 : 0)) & 1);
}

// out^T[nout x 16 NT draws] = act(W[:, :nin] . in^T + bias); `in` / `out` are LDS images [feature][RS], W has row stride ldw.
// act: -1 none, RNVP_ACT_*.  Out-of-range k: both operands are forced to zero (a stale image row may hold anything).
template <int NT>
__device__ __forceinline__ void linear(const float *__restrict__ W, int ldw, int nin, int nout, const float *bias,
                                       const float *in, float *out, int act, int lane) {
    constexpr int RS = row_stride(NT);
    const int q = lane >> 4, r = lane & 15;
    const int MT = (nout + 15) >> 4, KS = (nin + 3) >> 2;
    for (int m = 0; m < MT; ++m) {
        f4 acc[NT];
        {
            f4 b0;
#pragma unroll
            for (int e = 0; e < 4; ++e) { const int o = 16 * m + 4 * q + e; b0[e] = o < nout ? bias[o] : 0.f; }
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[t] = b0;
        }
        const int arow = 16 * m + r;
        const bool rok = arow < nout;
        const float *__restrict__ wp = W + (size_t)(rok ? arow : nout - 1) * ldw;
        // groups of four k-steps: the group's operand loads are issued together, then its MFMAs
        for (int ks0 = 0; ks0 < KS; ks0 += 4) {
            float a[4], b[4][NT];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int k = 4 * (ks0 + u) + q;
                const bool ok = k < nin;
                const int kk = ok ? k : 0;
                const float wv = wp[kk];
                a[u] = (rok && ok) ? wv : 0.f;
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    const float bv = in[kk * RS + 16 * t + r];
                    b[u][t] = ok ? bv : 0.f;
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (ks0 + u < KS) {
#pragma unroll
                    for (int t = 0; t < NT; ++t) acc[t] = mfma16(a[u], b[u][t], acc[t]);
                }
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int o = 16 * m + 4 * q + e;
            if (o < nout) {
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    float v = acc[t][e];
                    if (act >= 0) v = rnvp::act_fwd(v, act);
                    out[o * RS + 16 * t + r] = v;
                }
            }
        }
    }
}

template <int NT>
__global__ void __launch_bounds__(64)
k_draw(KShape s, Geo g, const float *__restrict__ params, const uint8_t *__restrict__ masks, const float *__restrict__ c,
       int64_t n_rows, int64_t row_offset, const uint64_t *__restrict__ seeds, const float *__restrict__ z, int64_t n_total,
       int64_t k_lo, int64_t k_cnt, int64_t k_total, State *state, float *x_out, float *xt_out) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int RS = row_stride(NT), NC = 16 * NT;
    const int lane = threadIdx.x, d = s.d, cd = s.c, h0 = s.nout[0];
    float *X = lds + g.oX, *XM = lds + g.oXM, *T = lds + g.oT, *S = lds + g.oS, *H0 = lds + g.oH0, *H1 = lds + g.oH1;
    float *CB = lds + g.oCB;
    State *ST = reinterpret_cast<State *>(lds + g.oST);
    for (int e = lane; e < g.floats; e += 64) lds[e] = 0.f;
    __syncthreads();
    for (int64_t row = blockIdx.x; row < n_rows; row += gridDim.x) {
        const int64_t grow = row_offset + row;
        // the condition's share of every net's first Linear, once per row
        for (int e = lane; e < s.L * 2 * h0; e += 64) {
            const int ln = e / h0, o = e - ln * h0;
            const float *pn = params + (size_t)ln * s.npn;
            const float *w = pn + s.woff[0] + (size_t)o * s.nin[0] + d;
            float a = pn[s.boff[0] + o];
            for (int i = 0; i < cd; ++i) a = fmaf(w[i], c[row * cd + i], a);
            CB[e] = a;
        }
        load_state(ST, state, row, d, lane);
        __syncthreads();
        for (int64_t k0 = 0; k0 < k_cnt; k0 += NC) {
            const int ncols = (int)(k_cnt - k0 < NC ? k_cnt - k0 : NC);
            if (seeds) {
                const int nblk = (d + 3) >> 2;
                for (int e = lane; e < NC * nblk; e += 64) {
                    const int col = e % NC, blk = e / NC;
                    float zz[4] = {0.f, 0.f, 0.f, 0.f};
                    if (col < ncols) rnvp::prior_normal4(seeds[k0 + col], grow, blk, zz);
#pragma unroll
                    for (int u = 0; u < 4; ++u)
                        if (4 * blk + u < d) X[(4 * blk + u) * RS + col] = zz[u];
                }
            } else {
                for (int e = lane; e < NC * d; e += 64) {
                    const int col = e / d, j = e - col * d;
                    X[j * RS + col] = col < ncols ? z[((k0 + col) * n_total + grow) * d + j] : 0.f;
                }
            }
            __syncthreads();
            for (int l = s.L - 1; l >= 0; --l) {
                for (int e = lane; e < NC * d; e += 64) {
                    const int j = e / NC, col = e - j * NC;
                    XM[j * RS + col] = X[j * RS + col] * mask_of(s, masks, l, j);
                }
                __syncthreads();
                for (int net = 0; net < 2; ++net) {
                    const float *pn = params + (size_t)(l * 2 + net) * s.npn;
                    const float *cur = XM;
                    float *dst = H0;
                    for (int k = 0; k <= s.nh; ++k) {
                        const bool last = k == s.nh;
                        float *ob = last ? (net == 0 ? T : S) : dst;
                        linear<NT>(pn + s.woff[k], s.nin[k], k == 0 ? d : s.nin[k], s.nout[k],
                                   k == 0 ? CB + (l * 2 + net) * h0 : pn + s.boff[k], cur, ob, last ? -1 : s.act, lane);
                        __syncthreads();
                        cur = ob;
                        if (!last) dst = dst == H0 ? H1 : H0;
                    }
                }
                // realnvp.py:128  ((X - T) * exp(-S)) * (1 - mask) + X * mask
                for (int e = lane; e < NC * d; e += 64) {
                    const int j = e / NC, col = e - j * NC;
                    if (mask_of(s, masks, l, j) == 0.f) {
                        const int a = j * RS + col;
                        X[a] = (X[a] - T[a]) * expf(-S[a]);
                    }
                }
                __syncthreads();
            }
            emit_fold<NT>(X, RS, d, ncols, row, n_rows, k0, k_lo, k_total, ST, state != nullptr, x_out, xt_out, lane);
            __syncthreads();
        }
        store_state(state, ST, row, d, lane);
        __syncthreads();
    }
}

__global__ void __launch_bounds__(256)
k_finalize(const State *__restrict__ state, int64_t total, int ddof, float *mean, float *sd, float *mn, float *mx) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const State st = state[i];
    const double n = (double)st.count;
    double m = NAN, v = NAN;
    if (st.count > 0) {
        m = (double)st.shift + st.sum / n;
        double ss = st.sumsq - st.sum * st.sum / n;
        if (ss < 0.0) ss = 0.0;
        v = sqrt(ss / (n - (double)ddof));            // count <= ddof: NaN (0 / 0, x / negative) or inf, as numpy
        if ((double)ddof >= n) v = NAN;
    }
    if (mean) mean[i] = (float)m;
    if (sd) sd[i] = (float)v;
    if (mn) mn[i] = st.count ? st.mn : NAN;
    if (mx) mx[i] = st.count ? st.mx : NAN;
}

// float <-> a uint32 key whose unsigned order is the float order (-0 below +0, NaNs at the two ends)
__device__ __forceinline__ uint32_t key_of(float v) {
    const uint32_t b = __float_as_uint(v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float val_of(uint32_t k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// the workgroup's 256 threads load one series into `keys` (P = 2^ceil(log2 K) entries, the P - K pad keys are 0xffffffff,
// at or above every float's key) and sort it ascending with a bitonic network; ends on a barrier
__device__ __forceinline__ void sort_series(uint32_t *keys, const float *__restrict__ x, int K, int P, int tid) {
    for (int i = tid; i < P; i += 256) keys[i] = i < K ? key_of(x[i]) : 0xffffffffu;
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < P; i += 256) {
                const int p = i ^ j;
                if (p > i) {
                    const uint32_t a = keys[i], b = keys[p];
                    const bool asc = (i & k) == 0;
                    if ((a > b) == asc) { keys[i] = b; keys[p] = a; }
                }
            }
            __syncthreads();
        }
    }
}

// numpy's 'linear' quantile of the sorted series in float64 (before its rounding): virtual index p (K - 1), then
// _lerp(a, b, t)
__device__ __forceinline__ double quantile_of(const uint32_t *keys, int K, double prob, bool has_nan) {
    const double pos = prob * (double)(K - 1);
    double fl = floor(pos);
    if (fl < 0.0) fl = 0.0;
    if (fl > (double)(K - 1)) fl = (double)(K - 1);
    const int lo = (int)fl, hi = lo + 1 < K ? lo + 1 : K - 1;
    const double t = pos - fl;
    const double a = (double)val_of(keys[lo]), b = (double)val_of(keys[hi]);
    const double diff = b - a;
    double res = a + diff * t;
    if (t >= 0.5) res = b - diff * (1.0 - t);
    if (diff == 0.0) res = a;
    if (has_nan) res = NAN;
    return res;
}

// one workgroup per (row, column) series: bitonic sort of P = 2^ceil(log2 K) keys in LDS, the P - K pad keys are
// 0xffffffff (at or above every float's key) and only indices below K are read afterwards.  NaNs sort to the two ends
// (by sign), so a series holds one iff keys[0] or keys[K - 1] decodes to NaN: every quantile of it is then NaN, as
// numpy.quantile gives
__global__ void __launch_bounds__(256)
k_quantiles(const float *__restrict__ xt, int64_t n_series, int K, int P, const double *__restrict__ probs, int nq,
            float *__restrict__ q_out) {
    extern __shared__ __attribute__((aligned(16))) uint32_t keys[];
    const int tid = threadIdx.x;
    for (int64_t sr = blockIdx.x; sr < n_series; sr += gridDim.x) {
        sort_series(keys, xt + sr * K, K, P, tid);
        const float v_lo = val_of(keys[0]), v_hi = val_of(keys[K - 1]);
        const bool has_nan = v_lo != v_lo || v_hi != v_hi;
        for (int i = tid; i < nq; i += 256)
            q_out[(int64_t)i * n_series + sr] = (float)quantile_of(keys, K, probs[i], has_nan);
        __syncthreads();
    }
}

// k_scores: k_quantiles' layout (one workgroup per series, the same sort), then ONE pass over the sorted series x_(0..K-1)
// against the series' target y:
//   S1 = sum_i |x_(i) - y|                       (K times the CRPS' first term)
//   S2 = sum_i (2 i - K + 1) (x_(i) - c)         (= 1/2 sum_k sum_l |x_k - x_l|: every pair counts its larger member with +,
//                                                 its smaller with -; the weights sum to zero, so any shift c cancels.  c is
//                                                 the middle order statistic x_(K/2): the terms are then bounded by K times the
//                                                 series' RANGE, wherever y lies)
//   lt, eq = #{x_(i) < y}, #{x_(i) == y}         (on the float values: -0 == +0 although their keys differ)
// Thread t sums i = t, t + 256, ... in that order in float64; the 256 partials are combined by a halving tree in LDS (t += t +
// s for s = 128 .. 1).  The order depends on K alone: no atomics, the same series gives the same bits in any grid.
// Non-finite: a NaN in the series (it sorts to an end) or in y makes crps, pit and every pinball NaN; a series holding an
// infinity has crps NaN (the pair sum's diagonal forms inf - inf); y = +-inf with a finite series gives S1 = inf, S2 finite.
// LDS in front of the keys: two float64 and two count partials per thread
constexpr size_t kScoreScratch = 256 * (2 * sizeof(double) + 2 * sizeof(uint32_t));

__global__ void __launch_bounds__(256)
k_scores(const float *__restrict__ xt, const float *__restrict__ y, int64_t n_series, int K, int P, int fair,
         const double *__restrict__ probs, int nq, float *__restrict__ crps, float *__restrict__ pit,
         float *__restrict__ q_out, float *__restrict__ pinball) {
    extern __shared__ __attribute__((aligned(16))) unsigned char score_lds[];
    double *r1 = reinterpret_cast<double *>(score_lds), *r2 = r1 + 256;        // the reduction scratch, then the keys
    uint32_t *rl = reinterpret_cast<uint32_t *>(r2 + 256), *re = rl + 256, *keys = re + 256;
    const int tid = threadIdx.x;
    for (int64_t sr = blockIdx.x; sr < n_series; sr += gridDim.x) {
        sort_series(keys, xt + sr * K, K, P, tid);
        const float v_lo = val_of(keys[0]), v_hi = val_of(keys[K - 1]);
        const bool has_nan = v_lo != v_lo || v_hi != v_hi;
        const bool has_inf = isinf(v_lo) || isinf(v_hi);
        const float yf = y[sr];
        const bool bad = has_nan || yf != yf;
        if (crps || pit) {
            const float cf = val_of(keys[K >> 1]);
            const double yd = (double)yf, c = isfinite(cf) ? (double)cf : 0.0;
            double s1 = 0.0, s2 = 0.0;
            uint32_t lt = 0, eq = 0;
            for (int i = tid; i < K; i += 256) {
                const float v = val_of(keys[i]);
                s1 += fabs((double)v - yd);
                s2 += (double)(2 * i - K + 1) * ((double)v - c);
                lt += v < yf ? 1u : 0u;
                eq += v == yf ? 1u : 0u;
            }
            r1[tid] = s1; r2[tid] = s2; rl[tid] = lt; re[tid] = eq;
            __syncthreads();
            for (int s = 128; s > 0; s >>= 1) {
                if (tid < s) { r1[tid] += r1[tid + s]; r2[tid] += r2[tid + s]; rl[tid] += rl[tid + s]; re[tid] += re[tid + s]; }
                __syncthreads();
            }
            if (tid == 0) {
                const double kd = (double)K, dd = fair ? kd - 1.0 : kd;
                double cr = r1[0] / kd - r2[0] / (kd * dd);             // K = 1 and fair: 0 / 0
                if (bad || has_inf) cr = NAN;
                const double pt = bad ? (double)NAN : ((double)rl[0] + 0.5 * (double)re[0]) / kd;
                if (crps) crps[sr] = (float)cr;
                if (pit) pit[sr] = (float)pt;
            }
        }
        for (int i = tid; i < nq; i += 256) {
            const double p = probs[i], q = quantile_of(keys, K, p, has_nan), yd = (double)yf;
            if (q_out) q_out[(int64_t)i * n_series + sr] = (float)q;
            if (pinball) {
                double pb = (yd - q) * (p - (yd < q ? 1.0 : 0.0));
                if (bad) pb = NAN;
                pinball[(int64_t)i * n_series + sr] = (float)pb;
            }
        }
        __syncthreads();
    }
}

// the draws per pass (NT tiles of 16) and the LDS bytes of one wave; 0 when not even one tile fits
int pick_tiles(const KShape &s, int64_t k_cnt, size_t *bytes) {
    const int want = k_cnt > 32 ? 4 : (k_cnt > 16 ? 2 : 1);
    for (int nt = want; nt >= 1; nt >>= 1) {
        const size_t b = (size_t)make_geo(s, row_stride(nt)).floats * sizeof(float);
        if (b <= (size_t)(nt > 1 ? kLdsWide : kLdsLimit)) { *bytes = b; return nt; }
    }
    return 0;
}

int shape_of(const rnvp_shape *shape, KShape *k) {
    if (!shape) return PFP_EINVAL;
    rnvp_shape s = *shape;
    s.precision = RNVP_PREC_AUTO; s.small_calls = RNVP_SMALL_INVARIANT; s.family = RNVP_FAMILY_AUTO;
    return rnvp::make_kshape(&s, k) == RNVP_OK ? PFP_OK : PFP_EINVAL;
}

std::atomic<uint64_t> g_big[3];

template <int NT>
int launch_draw(hipStream_t st, const KShape &k, size_t lds, int grid, const float *params, const uint8_t *masks, const float *c,
                int64_t n_rows, int64_t row_offset, const uint64_t *seeds, const float *z, int64_t n_total, int64_t k_lo,
                int64_t k_cnt, int64_t k_total, State *state, float *x_out, float *xt_out) {
    constexpr int slot = NT == 4 ? 2 : NT - 1;
    const Geo g = make_geo(k, row_stride(NT));
    if (lds > 48 * 1024) {
        const int e = rnvp::allow_big_lds(reinterpret_cast<const void *>(&k_draw<NT>), (int)lds, g_big[slot]);
        if (e != RNVP_OK) return e;
    }
    hipLaunchKernelGGL(k_draw<NT>, dim3(grid), dim3(64), lds, st, k, g, params, masks, c, n_rows, row_offset, seeds, z, n_total,
                       k_lo, k_cnt, k_total, state, x_out, xt_out);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" {

int pfp_version(void) { return PFP_VERSION; }

const char *pfp_status_string(int status) {
    switch (status) {
        case PFP_OK: return "ok";
        case PFP_EINVAL: return "invalid argument";
        case PFP_EUNSUPPORTED: return "shape not supported by the predictive-statistics kernels";
        case PFP_EWORKSPACE: return "workspace too small";
        default: return status > 0 ? hipGetErrorString((hipError_t)status) : "unknown status";
    }
}

size_t pfp_workspace_bytes(const rnvp_shape *shape, int64_t k_cnt) {
    KShape k;
    size_t lds = 0;
    if (k_cnt < 1 || shape_of(shape, &k) != PFP_OK || pick_tiles(k, k_cnt, &lds) == 0) return 0;
    return rnvp::align_up((size_t)k_cnt * sizeof(uint64_t), 256);
}

int pfp_draw_accumulate(void *stream, const rnvp_shape *shape, const float *params, const uint8_t *masks,
                        const float *c, int64_t n_rows, int64_t row_offset,
                        const uint64_t *seeds, const float *z, int64_t n_total,
                        int64_t k_lo, int64_t k_cnt, int64_t k_total,
                        void *state, float *x_out, float *xt_out,
                        void *workspace, size_t workspace_bytes) {
    KShape k;
    if (shape_of(shape, &k) != PFP_OK || !params) return PFP_EINVAL;
    if (n_rows < 0 || row_offset < 0 || k_cnt < 1 || k_lo < 0) return PFP_EINVAL;
    if ((seeds == nullptr) == (z == nullptr)) return PFP_EINVAL;
    if (k.c > 0 && !c && n_rows > 0) return PFP_EINVAL;
    if (!masks && k.alt == 0) return PFP_EINVAL;
    if (row_offset + n_rows > n_total) return PFP_EINVAL;
    if (k_lo + k_cnt > k_total) return PFP_EINVAL;
    size_t lds = 0;
    const int nt = pick_tiles(k, k_cnt, &lds);
    if (nt == 0) return PFP_EUNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    const uint64_t *dseeds = nullptr;
    if (seeds) {
        const size_t need = (size_t)k_cnt * sizeof(uint64_t);
        if (!workspace || workspace_bytes < need) return PFP_EWORKSPACE;
        if (n_rows > 0) RNVP_HIP_TRY(hipMemcpyAsync(workspace, seeds, need, hipMemcpyHostToDevice, st));
        dseeds = static_cast<const uint64_t *>(workspace);
    }
    if (n_rows == 0) return PFP_OK;
    const int grid = (int)(n_rows < kMaxGrid ? n_rows : kMaxGrid);
    State *sp = static_cast<State *>(state);
    if (nt == 4) return launch_draw<4>(st, k, lds, grid, params, masks, c, n_rows, row_offset, dseeds, z, n_total, k_lo, k_cnt, k_total, sp, x_out, xt_out);
    if (nt == 2) return launch_draw<2>(st, k, lds, grid, params, masks, c, n_rows, row_offset, dseeds, z, n_total, k_lo, k_cnt, k_total, sp, x_out, xt_out);
    return launch_draw<1>(st, k, lds, grid, params, masks, c, n_rows, row_offset, dseeds, z, n_total, k_lo, k_cnt, k_total, sp, x_out, xt_out);
}

int pfp_finalize(void *stream, const void *state, int64_t n_rows, int32_t d, int32_t ddof,
                 float *mean, float *std, float *min, float *max) {
    if (!state || n_rows < 0 || d < 1 || ddof < 0) return PFP_EINVAL;
    const int64_t total = n_rows * d;
    if (total == 0) return PFP_OK;
    hipLaunchKernelGGL(k_finalize, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       static_cast<const State *>(state), total, (int)ddof, mean, std, min, max);
    return (int)hipGetLastError();
}

int pfp_quantiles(void *stream, const float *xt, int64_t n_rows, int32_t d, int64_t k_total,
                  const double *probs, int32_t n_probs, float *q_out) {
    if (!xt || !probs || !q_out || n_rows < 0 || d < 1 || k_total < 1 || n_probs < 1) return PFP_EINVAL;
    if (k_total > PFP_MAX_QUANTILE_DRAWS) return PFP_EUNSUPPORTED;
    const int64_t n_series = n_rows * d;
    if (n_series == 0) return PFP_OK;
    int P = 1;
    while (P < k_total) P <<= 1;
    const int grid = (int)(n_series < kMaxGrid ? n_series : kMaxGrid);
    hipLaunchKernelGGL(k_quantiles, dim3(grid), dim3(256), (size_t)P * sizeof(uint32_t), (hipStream_t)stream, xt, n_series,
                       (int)k_total, P, probs, (int)n_probs, q_out);
    return (int)hipGetLastError();
}

int pfp_scores(void *stream, const float *xt, const float *y, int64_t n_rows, int32_t d, int64_t k_total,
               int32_t fair, const double *probs, int32_t n_probs,
               float *crps, float *pit, float *q_out, float *pinball) {
    if (!xt || !y || n_rows < 0 || d < 1 || k_total < 1 || n_probs < 0 || (n_probs > 0 && !probs)) return PFP_EINVAL;
    if (k_total > PFP_MAX_QUANTILE_DRAWS) return PFP_EUNSUPPORTED;
    const int64_t n_series = n_rows * d;
    if (n_series == 0) return PFP_OK;
    int P = 1;
    while (P < k_total) P <<= 1;
    const int grid = (int)(n_series < kMaxGrid ? n_series : kMaxGrid);
    hipLaunchKernelGGL(k_scores, dim3(grid), dim3(256), kScoreScratch + (size_t)P * sizeof(uint32_t), (hipStream_t)stream, xt, y,
                       n_series, (int)k_total, P, (int)(fair != 0), n_probs > 0 ? probs : nullptr, (int)n_probs, crps, pit, q_out,
                       pinball);
    return (int)hipGetLastError();
}

}  // extern "C"
