// pf_pairgrad.hip -- value and row gradients of the two closed-form two-sample statistics, for gfx950 (C ABI: pf_metrics.h,
// pfm_pair_grad).
//
// With the pooled rows z_0 .. z_{n-1} (n_first rows of the first sample, then the second's), the weights w[a] = +1 / n_first
// on a first row and -1 / (n - n_first) otherwise, and d^2_ab the squared distance of pf_pairtile.h,
//   L        = sum_ab w_a w_b g(d^2_ab)
//   dL/dz_a  = 2 w_a sum_b w_b c(d^2_ab) (z_a - z_b)
//   energy:  g = -sqrt(d^2),  c = -1 / sqrt(d^2), and exactly 0 where d^2 == 0
//   Gauss:   g = sum_m exp(-(gamma_m d^2)),  c = -2 sum_m gamma_m exp(-(gamma_m d^2))
// L is the energy distance's D^2 (V-statistic) or the biased MMD^2.  The difference z_a - z_b is taken feature by feature, as
// chunk_d2 takes it; the expansion z_a sum_b c - sum_b c z_b is NOT used (it cancels catastrophically for samples far from
// the origin), so a row that copies another gets a finite gradient and duplicated rows add exactly 0 to each other.
//   k_pair_sweep   workgroup (I, s, fc) runs row_grad_sweep of pf_gradsweep.h over its row block, column slice and feature chunk
//                  with coef_ab = w_b c(d^2), adding the value's terms w_a w_b g(d^2) on the way; the value of the workgroup
//                  (fc == 0 only) goes through a wave tree and the waves in index order to vpart[I, s].
//   k_pair_finish  grad[a, k] = 2 w_a (the slices' partials in index order); its last workgroup sums vpart in a fixed order.
// The slices depend on (n, d) only, never on the device, and there are no float atomics: the same inputs give the same bits,
// and every element the finish reads was written by the sweep of the same call.
// Rows and columns past n take no part: their terms are selected to 0, not multiplied by a zero weight (a finite row far from
// the origin is at an infinite d^2 from the all-zero row that pads a tile).
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "pf_metrics.h"
#include "pf_gradsweep.h"
#include "pf_scan1d.h"

namespace {

struct Gammas {
    double g[PFM_PAIR_MAX_GAMMAS];
};

// g(d^2) and c(d^2) of one pair
template <int KIND>
__device__ __forceinline__ void pair_terms(double dd, const Gammas &gm, int ng, double &g, double &c) {
    if (KIND == PFM_PERM_ENERGY) {
        const double s = sqrt(dd);
        g = -s;
        c = dd == 0.0 ? 0.0 : -1.0 / s;
    } else {
        __builtin_assume(ng >= 1);                 // pfm_pair_grad checked: the loop needs no guard
        double sg = 0.0, sc = 0.0;
#pragma unroll 1
        for (int m = 0; m < ng; ++m) {             // (uniform; the gammas are read from the kernel's arguments)
            const double e = exp(-(gm.g[m] * dd));
            sg += e;
            sc = fma(gm.g[m], e, sc);
        }
        g = sg;
        c = -2.0 * sc;
    }
}

// row_grad_sweep's Coef: coef_ab = w_b c(d^2); val gathers the thread's terms of the value
template <int KIND>
struct PairCoef {
    const Gammas &gm;
    int ng;
    double w_first, w_second;
    double val;
    __device__ __forceinline__ void columns(int64_t) {}
    __device__ __forceinline__ double pair(int, int, double d2, bool row_first, bool col_first, bool ok) {
        const double wb = col_first ? w_first : w_second;
        double g, c;
        pair_terms<KIND>(d2, gm, ng, g, c);
        val += ok ? (row_first ? w_first : w_second) * (wb * g) : 0.0;
        return ok ? wb * c : 0.0;
    }
};

// GF: the features of a gradient chunk that get registers (4 for d <= 4, else DC).  4 x 16 float64 accumulators are 128 of a
// lane's registers: two waves per SIMD fit beside them but for the Gaussian kind, which would spill to scratch at that bound and
// runs one wave per SIMD instead
template <int KIND, bool GRAD, int GF>
__global__ void __launch_bounds__(NT, (KIND == PFM_PERM_GAUSS && GF == DC) ? 1 : 2)
    k_pair_sweep(Gammas gm, int ng, const double *Z, int64_t n, int64_t d, int64_t n_first, Slices sl, double *vpart,
                 double *partial) {
    __shared__ double red[NT / 64];
    const int tid = threadIdx.x;
    PairCoef<KIND> coef = {gm, ng, 1.0 / (double)n_first, -1.0 / (double)(n - n_first), 0.0};
    row_grad_sweep<GRAD, GF>(Z, n, d, n_first, sl, coef, partial);

    // ---- the value: the wave's 64 lanes, then the waves in index order ----
    if (blockIdx.z == 0) {
        double val = coef.val;
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) val = val + __shfl_xor(val, m, 64);
        if ((tid & 63) == 0) red[tid >> 6] = val;
        __syncthreads();
        if (tid == 0) {
            double v = red[0];
#pragma unroll
            for (int w = 1; w < NT / 64; ++w) v = v + red[w];
            vpart[(int64_t)blockIdx.x * sl.count + blockIdx.y] = v;
        }
    }
}

// grad[a, k] = 2 w_a sum_s partial[s, a, k] (finish_rows); the last workgroup sums the nv value partials: thread t takes
// t, t + NT, .. in order, then block_sum's fixed tree over the threads
__global__ void __launch_bounds__(NT) k_pair_finish(const double *vpart, int64_t nv, const double *partial, int64_t n,
                                                    int64_t d, int64_t n_first, int64_t slices, double *value, double *grad) {
    __shared__ double red[NT];
    const int tid = threadIdx.x;
    if (blockIdx.x + 1 < gridDim.x) {
        finish_rows(partial, n, d, slices, [=](int64_t a) {
            const double w = a < n_first ? 1.0 / (double)n_first : -1.0 / (double)(n - n_first);
            return 2.0 * w;
        }, grad);
        return;
    }
    double v = 0.0;
    for (int64_t i = tid; i < nv; i += NT) v = v + vpart[i];
    const double total = block_sum(v, red);
    if (tid == 0) value[0] = total;
}

template <int KIND>
void launch_sweep(hipStream_t st, bool want_grad, const Gammas &gm, int ng, const double *Z, int64_t n, int64_t d,
                  int64_t n_first, const Slices &sl, double *vpart, double *partial) {
    const dim3 grid((unsigned)sl.nb, (unsigned)sl.count, want_grad ? (unsigned)sl.fc : 1u);
    if (!want_grad)
        hipLaunchKernelGGL((k_pair_sweep<KIND, false, 1>), grid, dim3(NT), 0, st, gm, ng, Z, n, d, n_first, sl, vpart, partial);
    else if (d <= 4)
        hipLaunchKernelGGL((k_pair_sweep<KIND, true, 4>), grid, dim3(NT), 0, st, gm, ng, Z, n, d, n_first, sl, vpart, partial);
    else
        hipLaunchKernelGGL((k_pair_sweep<KIND, true, DC>), grid, dim3(NT), 0, st, gm, ng, Z, n, d, n_first, sl, vpart, partial);
}

}  // namespace

// ---- C ABI --------------------------------------------------------------------------------------------

extern "C" size_t pfm_pair_grad_workspace_bytes(int64_t n, int64_t d, int64_t n_first) {
    if (!pair_args_ok(n, d, n_first)) return 0;
    const Slices sl = slices_of(n, d);
    return align256(sizeof(double) * (size_t)(sl.nb * sl.count)) + partial_bytes(sl, n, d);
}

extern "C" int pfm_pair_grad(void *stream, int kind, const double *gammas, int n_gamma, const double *Z, int64_t n, int64_t d,
                             int64_t n_first, double *value, double *grad, void *workspace, size_t workspace_bytes) {
    if (!Z || !value || !pair_args_ok(n, d, n_first)) return PFM_EINVAL;
    if (kind != PFM_PERM_ENERGY && kind != PFM_PERM_GAUSS) return PFM_EUNSUPPORTED;
    Gammas gm;
    for (int m = 0; m < PFM_PAIR_MAX_GAMMAS; ++m) gm.g[m] = 0.0;
    if (kind == PFM_PERM_GAUSS) {
        if (!gammas || n_gamma < 1 || n_gamma > PFM_PAIR_MAX_GAMMAS) return PFM_EINVAL;
        for (int m = 0; m < n_gamma; ++m) {
            if (!(gammas[m] > 0.0 && gammas[m] <= 1.79769313486231570815e308)) return PFM_EINVAL;
            gm.g[m] = gammas[m];
        }
    } else {
        n_gamma = 0;
    }
    if (!workspace || workspace_bytes < pfm_pair_grad_workspace_bytes(n, d, n_first)) return PFM_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const Slices sl = slices_of(n, d);
    double *vpart = (double *)workspace;
    double *partial = (double *)((char *)workspace + align256(sizeof(double) * (size_t)(sl.nb * sl.count)));

    const bool want_grad = grad != nullptr;
    if (kind == PFM_PERM_ENERGY) launch_sweep<PFM_PERM_ENERGY>(st, want_grad, gm, n_gamma, Z, n, d, n_first, sl, vpart, partial);
    else launch_sweep<PFM_PERM_GAUSS>(st, want_grad, gm, n_gamma, Z, n, d, n_first, sl, vpart, partial);
    PFM_TRY(hipGetLastError());
    const int64_t gblocks = grad ? (n * d + NT - 1) / NT : 0;
    hipLaunchKernelGGL(k_pair_finish, dim3((unsigned)(gblocks + 1)), dim3(NT), 0, st, (const double *)vpart, sl.nb * sl.count,
                       (const double *)partial, n, d, n_first, sl.count, value, grad);
    PFM_TRY(hipGetLastError());
    return PFM_OK;
}
