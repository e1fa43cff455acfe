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
//   k_pair_sweep   workgroup (I, s, fc) owns the 64 rows a of row block I, the column tiles J of slice s and the features
//                  16 fc .. 16 fc + 15 of the gradient.  Per tile it forms d^2 (tile_d2), turns the 4 x 4 values a thread owns
//                  into w_b c(d^2) and, for the value, into w_a w_b g(d^2), and accumulates sum_b coef_ab (z_a[k] - z_b[k]) per
//                  owned row and feature in registers (4 rows x 16 features) across its whole slice.  For d <= 16 the row
//                  block's features stay staged in LDS for the sweep (tile_d2's a_resident) and the column tile tile_d2 staged
//                  is read again for the differences; for wider rows the gradient's chunk of both sides is staged beside the
//                  chunks tile_d2 walks, and every feature chunk's workgroup re-forms d^2 over all d features.  At the end of
//                  the slice the 16 lanes that share a row are summed (xor tree) and written to partial[s, a, k]; the value
//                  of the workgroup (fc == 0 only) goes through a wave tree and the waves in index order to vpart[I, s].
//   k_pair_finish  grad[a, k] = 2 w_a (the slices' partials in index order); its last workgroup sums vpart in a fixed order.
// The slices depend on (n, d) only, never on the device, and there are no float atomics: the same inputs give the same bits,
// and every element the finish reads was written by the sweep of the same call.
// Rows and columns past n take no part: their terms are selected to 0, not multiplied by a zero weight (a finite row far from
// the origin is at an infinite d^2 from the all-zero row that pads a tile).
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "pf_metrics.h"
#include "pf_pairtile.h"

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

// GF: the features of a gradient chunk that get registers (4 for d <= 4, else DC).  4 x 16 float64 accumulators are 128 of a
// lane's registers: two waves per SIMD fit beside them but for the Gaussian kind, which would spill to scratch at that bound and
// runs one wave per SIMD instead
template <int KIND, bool GRAD, int GF>
__global__ void __launch_bounds__(NT, (KIND == PFM_PERM_GAUSS && GF == DC) ? 1 : 2)
    k_pair_sweep(Gammas gm, int ng, const double *Z, int64_t n, int64_t d, int64_t n_first, Slices sl, double *vpart,
                 double *partial) {
    __shared__ double sA[DC][TPAD], sB[DC][TPAD];          // the chunks tile_d2 walks
    __shared__ double xA[DC][TPAD], xB[DC][TPAD];          // d > DC: the gradient's chunk of the rows and of the column tile
    __shared__ double red[NT / 64];
    const int tid = threadIdx.x, ti = tid >> 4, tj = tid & 15;
    const int64_t I0 = (int64_t)blockIdx.x * TILE;
    const int64_t s = blockIdx.y;
    const int64_t k0 = (int64_t)blockIdx.z * DC;           // first feature of this workgroup's gradient chunk
    const int dcg = (int)((d - k0) < DC ? (d - k0) : DC);
    const bool resident = d <= DC;
    const Plain pooled = {Z, n, d};
    const double w_first = 1.0 / (double)n_first, w_second = -1.0 / (double)(n - n_first);

    int64_t J = s * sl.per, J_end = J + sl.per;
    if (J_end > sl.nb) J_end = sl.nb;

    double (*gA)[TPAD] = resident ? sA : xA;
    double (*gB)[TPAD] = resident ? sB : xB;
    if (resident) stage(pooled, I0, 0, (int)d, sA);        // visible after tile_d2's first barrier
    else if (GRAD) stage(pooled, I0, k0, dcg, xA);

    // row ti + 16 a of the block exists while 16 a < rows_left and is of the first sample while 16 a < first_left
    const int rows_left = (int)(n - I0 - ti < TILE ? n - I0 - ti : TILE);
    const int first_left = (int)(n_first - I0 - ti < TILE ? (n_first - I0 - ti > -TILE ? n_first - I0 - ti : -TILE) : TILE);

    double G[4][GF];
    double val = 0.0;
    if (GRAD) {
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int k = 0; k < GF; ++k) G[a][k] = 0.0;
    }

    for (; J < J_end; ++J) {
        const int64_t J0 = J * TILE;
        if (GRAD && !resident) {
            __syncthreads();                               // the previous tile's reads of xB are done
            stage(pooled, J0, k0, dcg, xB);
        }
        double dd[4][4];
        tile_d2(pooled, I0, pooled, J0, resident, sA, sB, dd);

        // ---- dd <- w_b c(d^2); the value's terms on the way ----
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int64_t cb = J0 + tj + 16 * b;
            const bool col_ok = cb < n;
            const double wb = cb < n_first ? w_first : w_second;
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                double g, c;
                pair_terms<KIND>(dd[a][b], gm, ng, g, c);
                const bool ok = col_ok && 16 * a < rows_left;
                val += ok ? (16 * a < first_left ? w_first : w_second) * (wb * g) : 0.0;
                dd[a][b] = ok ? wb * c : 0.0;
            }
        }

        // ---- the differences, feature by feature ----
        if (GRAD) {
#pragma unroll
            for (int k = 0; k < GF; ++k)
                if (k < dcg) {                             // (uniform)
                    double xa[4], yb[4];
#pragma unroll
                    for (int a = 0; a < 4; ++a) xa[a] = gA[k][ti + 16 * a];
#pragma unroll
                    for (int b = 0; b < 4; ++b) yb[b] = gB[k][tj + 16 * b];
#pragma unroll
                    for (int a = 0; a < 4; ++a)
#pragma unroll
                        for (int b = 0; b < 4; ++b) G[a][k] = fma(dd[a][b], xa[a] - yb[b], G[a][k]);
                }
        }
    }

    // ---- a row's 16 lanes: xor tree; lane tj then writes feature tj ----
    if (GRAD) {
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            double out = 0.0;
#pragma unroll
            for (int k = 0; k < GF; ++k) {
                double v = G[a][k];
#pragma unroll
                for (int m = 1; m < 16; m <<= 1) v = v + __shfl_xor(v, m, 16);
                if (tj == k) out = v;
            }
            const int64_t r = I0 + ti + 16 * a;
            if (r < n && tj < dcg) partial[(s * n + r) * d + k0 + tj] = out;
        }
    }

    // ---- the value: the wave's 64 lanes, then the waves in index order ----
    if (blockIdx.z == 0) {
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) val = val + __shfl_xor(val, m, 64);
        if ((tid & 63) == 0) red[tid >> 6] = val;
        __syncthreads();
        if (tid == 0) {
            double v = red[0];
#pragma unroll
            for (int w = 1; w < NT / 64; ++w) v = v + red[w];
            vpart[(int64_t)blockIdx.x * sl.count + s] = v;
        }
    }
}

// grad[a, k] = 2 w_a sum_s partial[s, a, k], element e = a d + k of workgroups 0 .. gridDim.x - 2; the last workgroup sums
// the nv value partials: thread t takes t, t + NT, .. in order, then a fixed tree over the threads
__global__ void __launch_bounds__(NT) k_pair_finish(const double *vpart, int64_t nv, const double *partial, int64_t n,
                                                    int64_t d, int64_t n_first, int64_t slices, double *value, double *grad) {
    __shared__ double red[NT];
    const int tid = threadIdx.x;
    if (blockIdx.x + 1 < gridDim.x) {
        const int64_t e = (int64_t)blockIdx.x * NT + tid;
        if (e < n * d) {
            const int64_t a = e / d;
            double v = partial[e];
            for (int64_t s = 1; s < slices; ++s) v = v + partial[s * n * d + e];
            const double w = a < n_first ? 1.0 / (double)n_first : -1.0 / (double)(n - n_first);
            grad[e] = (2.0 * w) * v;
        }
        return;
    }
    double v = 0.0;
    for (int64_t i = tid; i < nv; i += NT) v = v + vpart[i];
    red[tid] = v;
    __syncthreads();
    for (int m = NT / 2; m > 0; m >>= 1) {
        if (tid < m) red[tid] = red[tid] + red[tid + m];
        __syncthreads();
    }
    if (tid == 0) value[0] = red[0];
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
    return align256(sizeof(double) * (size_t)(sl.nb * sl.count)) + align256(sizeof(double) * (size_t)(sl.count * n * d));
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
