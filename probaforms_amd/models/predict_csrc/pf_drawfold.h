// pf_drawfold.h -- what the draw kernels of libpf_predict.so (k_draw) and libpf_gendraw.so (k_mlp_draw, k_affine_draw) share:
// the running-moment state of pf_predict.h and its pick-up, fold and write-back by ONE wave, the LDS image's row stride and
// the MFMA / NaN-aware min and max helpers.  Everything here is a wave's own work: no barrier, no atomics; the
// caller synchronises (a workgroup barrier in k_draw, whose workgroup is one wave; wave_sync in pf_gendraw.hip).
// The fold's NaN rule (min_nan / max_nan), its shift rule (the tile's first draw, 0 when that is not finite) and its fixed
// summation order are what lets rows and draws split over calls reproduce one call bit for bit: they exist here only.
#pragma once
#include "pf_predict.h"

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace drawfold {

using f4 = __attribute__((ext_vector_type(4))) float;

constexpr int kMaxGrid = 65536;
constexpr int kLdsLimit = 160 * 1024;      // one CU's LDS on gfx950

struct State {
    double sum, sumsq;
    float shift, mn, mx;
    uint32_t count;
};
static_assert(sizeof(State) == PFP_STATE_BYTES, "state layout of pf_predict.h");
constexpr int kStateFloats = (int)(sizeof(State) / sizeof(float));

// row stride of an image [feature][RS] holding 16 nt draws: the four k rows a B read touches fall on distinct banks
__host__ __device__ constexpr int row_stride(int nt) { return nt == 4 ? 80 : 16 * nt + 1; }

__device__ __forceinline__ f4 mfma16(float a, float b, f4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// numpy's min / max: NaN when either operand is NaN (fminf / fmaxf return the other operand)
__device__ __forceinline__ float min_nan(float a, float b) { return (a != a || b != b) ? NAN : fminf(a, b); }
__device__ __forceinline__ float max_nan(float a, float b) { return (a != a || b != b) ? NAN : fmaxf(a, b); }

// the state of the row's d columns into ST (LDS) when the wave picks the row up; no state, or a column that has seen no
// draw yet: the empty state
__device__ __forceinline__ void load_state(State *ST, const State *state, int64_t row, int d, int lane) {
    for (int j = lane; j < d; j += 64) {
        State st = State{0.0, 0.0, 0.f, 0.f, 0.f, 0u};
        if (state) st = state[row * d + j];
        if (st.count == 0) { st.sum = 0.0; st.sumsq = 0.0; st.mn = INFINITY; st.mx = -INFINITY; }
        ST[j] = st;
    }
}

// and back when the row is done
__device__ __forceinline__ void store_state(State *state, const State *ST, int64_t row, int d, int lane) {
    if (state)
        for (int j = lane; j < d; j += 64) state[row * d + j] = ST[j];
}

// One wave: the pass's draws X [d][RS] (ncols valid columns) to x_out / xt_out, and folded into the row's state ST (LDS).
// Fold: lane (q, r) takes column 4 jj + q and draw 16 t + r; the 16 draws of a tile are reduced by a fixed xor butterfly
// (float64 sums of x - shift and its square, float32 min / max), the tiles are added in draw order.
template <int NT>
__device__ __forceinline__ void emit_fold(const float *X, int RS, int d, int ncols, int64_t row, int64_t n_rows, int64_t k0,
                                          int64_t k_lo, int64_t k_total, State *ST, bool fold, float *__restrict__ x_out,
                                          float *__restrict__ xt_out, int lane) {
    constexpr int NC = 16 * NT;
    const int q = lane >> 4, r = lane & 15;
    if (x_out) {
        for (int e = lane; e < ncols * d; e += 64) {
            const int col = e / d, j = e - col * d;
            x_out[((k0 + col) * n_rows + row) * d + j] = X[j * RS + col];
        }
    }
    if (xt_out) {
        for (int e = lane; e < NC * d; e += 64) {
            const int j = e / NC, col = e - j * NC;
            if (col < ncols) xt_out[(row * d + j) * k_total + k_lo + k0 + col] = X[j * RS + col];
        }
    }
    if (!fold) return;
    for (int jj = 0; jj < d; jj += 4) {
        const int j = jj + q;
        const bool jok = j < d;
        State st = ST[jok ? j : 0];
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int col = 16 * t + r;
            const bool ok = jok && col < ncols;
            const float v = X[(jok ? j : 0) * RS + col];
            const float first = __shfl(v, lane & 48);           // the tile's first draw of this column
            if (st.count == 0) st.shift = isfinite(first) ? first : 0.f;
            const double dv = ok ? (double)v - (double)st.shift : 0.0;
            double s1 = dv, s2 = dv * dv;
            float mn = ok ? v : INFINITY, mx = ok ? v : -INFINITY;
#pragma unroll
            for (int w = 8; w >= 1; w >>= 1) {
                s1 += __shfl_xor(s1, w);
                s2 += __shfl_xor(s2, w);
                mn = min_nan(mn, __shfl_xor(mn, w));
                mx = max_nan(mx, __shfl_xor(mx, w));
            }
            const int nv = ncols - 16 * t;
            if (nv > 0) {
                st.sum += s1; st.sumsq += s2;
                st.mn = min_nan(st.mn, mn); st.mx = max_nan(st.mx, mx);
                st.count += (uint32_t)(nv < 16 ? nv : 16);
            }
        }
        if (jok && r == 0) ST[j] = st;
    }
}

}  // namespace drawfold
