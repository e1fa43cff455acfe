// pf_sinkgrad.hip -- the debiased Sinkhorn divergence of the samples as given TOGETHER WITH its derivative by every row, for
// gfx950 (C ABI: pf_metrics.h, pfm_sinkhorn_grad).
//
// The value is the scheme of pf_sinkhorn.hip with the uniform weights 1 / nr, 1 / nf: four potentials on the pooled rows
// z = [R; F] (pot[slot][n], slot 0 the cross potential, slot 1 the self potential), n_sinkhorn averaged symmetrised Jacobi steps
// from old values, one last plain step.  With `old` the buffer the last step read and `fin` the one it wrote, every row's final
// softmin is differentiated by that row's own coordinates only (the columns and the incoming potentials held fixed: the
// envelope-theorem gradient, exact at the fixed point):
//   P_ab     = exp((fin_a[slot] + old_b[slot] - C_ab) / eps - log n_side(b)),   slot = self if side(a) == side(b), else cross
//   dS/dz_a  = w_a sum_b sgn_ab P_ab c_p(d^2_ab) (z_a - z_b),   sgn = +1 cross, -1 self;  c_2 = 2;  c_1 = 1 / sqrt(d^2), 0 at d^2 = 0
// sum_b P_ab over one side is 1 by the definition of fin_a, so no exp overflows.  The difference z_a - z_b is taken feature by
// feature on the rows themselves, as pf_pairgrad.hip takes it.
//   k_sinkhorn_step1   one step for all four potentials of ONE weighting.  A workgroup owns a strip of TILE rows of one sample and
//                      walks the column tiles of R, then those of F; per tile it forms the TILE x TILE costs / eps once (tile_d2)
//                      and keeps them in LDS.  Thread (row = lane, wave w) folds the columns 16 w .. 16 w + 15 of every tile into
//                      its own running (max, sum): all four waves work on the strip.  After a sample's last tile the four
//                      partial (max, sum) pairs of a row are merged through LDS in wave order, -log n of the columns' sample is
//                      added once, and the softmin is averaged with the old potential (or, in the last step, stored as it is)
//                      into the other buffer.  Columns past the end carry h = -inf and add exp(-inf) = 0; a wave whose 16
//                      columns are such alone skips the tile.
//   k_sinkhorn_sweep   workgroup (I, s, fc) runs row_grad_sweep of pf_gradsweep.h over its row block of the pooled sample, column
//                      slice and feature chunk with coef_ab = sgn P c_p, one exp per pair.
//   k_sinkhorn_grad_finish  grad[a, k] = w_a (the slices' partials in index order); its last workgroup forms value and drift as
//                      k_sinkhorn_finish does (sinkhorn_value_drift of pf_scan1d.h) and copies the potentials out.
// k_sinkhorn_step1 is NOT k_sinkhorn_step of pf_sinkhorn.hip with one replicate: that kernel shares the replicates out over the
// waves, this one the columns of a tile, and the one-replicate form measured 1.5 to 2.1 times faster for it
// (profiles/r23_sinkhorn_loss_time.txt).  The two are kept apart on purpose.
// A row's softmin is folded per wave over the columns in index order and the waves are merged in wave order; the slices depend
// on (n, d) only: the order of every sum depends on (n, n_first, d) only, and two calls give the same bytes.  No float atomics.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "pf_metrics.h"
#include "pf_gradsweep.h"
#include "pf_scan1d.h"

namespace {

constexpr int NW = NT / 64;                // waves of a workgroup
constexpr int CPW = TILE / NW;             // columns of a tile a wave folds
constexpr int64_t MAX_SINKHORN = 1000000;  // launches per call, at most

struct Sk1Shared {
    double G[TILE][TPAD];               // the tile's costs / eps
    double A[DC][TPAD], B[DC][TPAD];    // staged feature chunks: the strip's rows (resident for d <= DC), the tile's columns
    double h[TILE];                     // h / eps of the tile's columns, -inf past the end
    double pm[NW][TILE], ps[NW][TILE];  // the waves' partial (max, sum) of every row of the strip
};

__global__ void __launch_bounds__(NT) k_sinkhorn_step1(const double *Z, int64_t nr, int64_t nf, int64_t d, int p, double eps,
                                                       double inv_eps, const double *__restrict__ src,
                                                       double *__restrict__ dst, int averaged) {
    __shared__ Sk1Shared sh;
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    const int ti = tid >> 4, tj = tid & 15;
    const int64_t N = nr + nf, ta = tiles_per_side(nr), tb = tiles_per_side(nf);
    const int64_t strip = blockIdx.x;
    const int rside = strip >= ta ? 1 : 0;
    const int64_t I0 = (rside ? strip - ta : strip) * TILE, roff = rside ? nr : 0;
    const Plain A = {Z + roff * d, rside ? nf : nr, d};
    const bool resident = d <= DC;
    if (resident) stage(A, I0, 0, (int)d, sh.A);     // visible after tile_d2's barriers

    for (int cside = 0; cside < 2; ++cside) {
        const int64_t coff = cside ? nr : 0, ntc = cside ? tb : ta;
        const Plain B = {Z + coff * d, cside ? nf : nr, d};
        const int slot = rside == cside ? 1 : 0;
        double m = -INFINITY, s = 0.0;

        for (int64_t J = 0; J < ntc; ++J) {
            const int64_t J0 = J * TILE;
            double hv = -INFINITY;                                // in flight under tile_d2
            if (tid < TILE && J0 + tid < B.n) hv = src[slot * N + coff + J0 + tid] * inv_eps;

            double dd[4][4];
            tile_d2(A, I0, B, J0, resident, sh.A, sh.B, dd);      // begins with a barrier: the previous tile's folds are done
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) sh.G[ti + 16 * a][tj + 16 * b] = (p == 1 ? sqrt(dd[a][b]) : dd[a][b]) * inv_eps;
            if (tid < TILE) sh.h[tid] = hv;
            __syncthreads();

            double tm = -INFINITY;
#pragma unroll
            for (int k = 0; k < CPW; ++k) tm = fmax(tm, sh.h[CPW * w + k] - sh.G[lane][CPW * w + k]);
            if (tm > -INFINITY) {                                 // (uniform over the wave: G is finite)
                const double M = fmax(m, tm);
                double acc = s * exp(m - M);
#pragma unroll 4
                for (int k = 0; k < CPW; ++k) acc = acc + exp((sh.h[CPW * w + k] - sh.G[lane][CPW * w + k]) - M);
                s = acc;
                m = M;
            }
        }

        // the softmin of the strip's rows against this sample's columns: the waves' partials in wave order
        sh.pm[w][lane] = m;
        sh.ps[w][lane] = s;
        __syncthreads();       // the next sample's first write to pm / ps lies behind tile_d2's barriers, which wave 0 joins
        const int64_t g = I0 + lane;
        if (w == 0 && g < A.n) {
            double M = sh.pm[0][lane];
#pragma unroll
            for (int q = 1; q < NW; ++q) M = fmax(M, sh.pm[q][lane]);
            double S = 0.0;
#pragma unroll
            for (int q = 0; q < NW; ++q)
                if (sh.pm[q][lane] > -INFINITY) S = S + sh.ps[q][lane] * exp(sh.pm[q][lane] - M);
            const double sm = -eps * ((M + log(S)) - log((double)B.n));
            const int64_t at = slot * N + roff + g;
            dst[at] = averaged ? 0.5 * (src[at] + sm) : sm;
        }
    }
}

// row_grad_sweep's Coef: coef_ab = sgn P c_p(d^2) from the rows' final potentials and the columns' old ones
struct SinkCoef {
    int64_t n, n_first;
    int p;
    double inv_eps, lw_first, lw_second;
    const double *__restrict__ old;
    double fa[4][2];                                       // the rows' final potentials / eps: cross, self
    double ob[4][2];                                       // the columns' old potentials / eps - log n: in flight under tile_d2
    __device__ __forceinline__ void rows(const double *__restrict__ fin) {
        const int64_t r0 = (int64_t)blockIdx.x * TILE + (threadIdx.x >> 4);
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const int64_t r = r0 + 16 * a;
            fa[a][0] = r < n ? fin[r] * inv_eps : 0.0;
            fa[a][1] = r < n ? fin[n + r] * inv_eps : 0.0;
        }
    }
    __device__ __forceinline__ void columns(int64_t J0) {
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int64_t cb = J0 + (threadIdx.x & 15) + 16 * b;
            const double lw = cb < n_first ? lw_first : lw_second;
            ob[b][0] = cb < n ? fma(old[cb], inv_eps, lw) : 0.0;
            ob[b][1] = cb < n ? fma(old[n + cb], inv_eps, lw) : 0.0;
        }
    }
    __device__ __forceinline__ double pair(int a, int b, double d2, bool row_first, bool col_first, bool ok) const {
        const bool same = row_first == col_first;
        const double C = p == 1 ? sqrt(d2) : d2;
        const double e = exp((same ? fa[a][1] + ob[b][1] : fa[a][0] + ob[b][0]) - C * inv_eps);
        const double c = p == 1 ? (d2 == 0.0 ? 0.0 : 1.0 / C) : 2.0;
        return ok ? (same ? -e : e) * c : 0.0;
    }
};

// GF: the features of a gradient chunk that get registers (4 for d <= 4, else DC), as k_pair_sweep's; the 4 x 16 float64
// accumulators beside the exp run one wave per SIMD
template <int GF>
__global__ void __launch_bounds__(NT, GF == DC ? 1 : 2)
    k_sinkhorn_sweep(const double *Z, int64_t n, int64_t d, int64_t n_first, int p, double inv_eps,
                     const double *__restrict__ fin, const double *__restrict__ old, Slices sl, double *partial) {
    SinkCoef coef = {n, n_first, p, inv_eps, -log((double)n_first), -log((double)(n - n_first)), old};
    coef.rows(fin);
    row_grad_sweep<true, GF>(Z, n, d, n_first, sl, coef, partial);
}

// grad[a, k] = w_a sum_s partial[s, a, k] (finish_rows; there are no such workgroups for the value alone); the last workgroup:
// value = sum_i w_i (fin[0][i] - fin[1][i]) and drift = the largest |cur - prev| of a potential (the last averaged step's
// change), and the potentials, fin then cur
__global__ void __launch_bounds__(NT) k_sinkhorn_grad_finish(const double *partial, int64_t n, int64_t d, int64_t n_first,
                                                             int64_t slices, const double *__restrict__ fin,
                                                             const double *__restrict__ cur, const double *__restrict__ prev,
                                                             int has_prev, double *__restrict__ value,
                                                             double *__restrict__ drift, double *__restrict__ grad,
                                                             double *__restrict__ potentials) {
    __shared__ double sd[NT];
    const int tid = threadIdx.x;
    const double w_first = 1.0 / (double)n_first, w_second = 1.0 / (double)(n - n_first);
    const auto weight = [=](int64_t i) { return i < n_first ? w_first : w_second; };
    if (blockIdx.x + 1 < gridDim.x) {
        finish_rows(partial, n, d, slices, weight, grad);
        return;
    }
    double total, dr;
    sinkhorn_value_drift(fin, cur, prev, has_prev, n, weight, sd, total, dr);
    if (tid == 0) {
        value[0] = total;
        drift[0] = dr;
    }
    if (potentials)
        for (int64_t i = tid; i < 2 * n; i += NT) {
            potentials[i] = fin[i];
            potentials[2 * n + i] = cur[i];
        }
}

struct Layout {                     // the workspace: three potential buffers, the slices' gradient partials
    size_t pot, partial, total;     // bytes of ONE potential buffer, of the partials, of everything
};

Layout layout_of(int64_t n, int64_t d) {
    const Slices sl = slices_of(n, d);
    Layout l;
    l.pot = align256(sizeof(double) * 2 * (size_t)n);
    l.partial = partial_bytes(sl, n, d);
    l.total = 3 * l.pot + l.partial;
    return l;
}

}  // namespace

// ---- C ABI --------------------------------------------------------------------------------------------

extern "C" size_t pfm_sinkhorn_grad_workspace_bytes(int64_t n, int64_t d, int64_t n_first) {
    if (!pair_args_ok(n, d, n_first)) return 0;
    return layout_of(n, d).total;
}

extern "C" int pfm_sinkhorn_grad(void *stream, const double *Z, int64_t n, int64_t d, int64_t n_first, int p, double eps,
                                 int64_t n_sinkhorn, double *value, double *drift, double *grad, double *potentials,
                                 void *workspace, size_t workspace_bytes) {
    if (!Z || !value || !drift || !pair_args_ok(n, d, n_first)) return PFM_EINVAL;
    if (!(eps > 0.0) || !isfinite(eps) || !isfinite(1.0 / eps) || n_sinkhorn < 0 || n_sinkhorn > MAX_SINKHORN)
        return PFM_EINVAL;
    if (p != 1 && p != 2) return PFM_EUNSUPPORTED;
    const Layout l = layout_of(n, d);
    if (!workspace || workspace_bytes < l.total) return PFM_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int64_t nr = n_first, nf = n - n_first;
    char *base = (char *)workspace;
    double *pot[3];
    for (int k = 0; k < 3; ++k) pot[k] = (double *)(base + k * l.pot);
    double *partial = (double *)(base + 3 * l.pot);

    PFM_TRY(hipMemsetAsync(pot[0], 0, sizeof(double) * 2 * (size_t)n, st));      // every potential starts at 0
    const dim3 strips((unsigned)(tiles_per_side(nr) + tiles_per_side(nf)));
    const double inv_eps = 1.0 / eps;
    for (int64_t it = 0; it <= n_sinkhorn; ++it) {
        const bool last = it == n_sinkhorn;
        hipLaunchKernelGGL(k_sinkhorn_step1, strips, dim3(NT), 0, st, Z, nr, nf, d, p, eps, inv_eps,
                           (const double *)pot[it & 1], last ? pot[2] : pot[(it + 1) & 1], last ? 0 : 1);
        PFM_TRY(hipGetLastError());
    }
    const double *fin = pot[2], *old = pot[n_sinkhorn & 1], *prev = pot[(n_sinkhorn + 1) & 1];
    const Slices sl = slices_of(n, d);
    if (grad) {
        const dim3 grid((unsigned)sl.nb, (unsigned)sl.count, (unsigned)sl.fc);
        if (d <= 4)
            hipLaunchKernelGGL((k_sinkhorn_sweep<4>), grid, dim3(NT), 0, st, Z, n, d, n_first, p, inv_eps, fin, old, sl, partial);
        else
            hipLaunchKernelGGL((k_sinkhorn_sweep<DC>), grid, dim3(NT), 0, st, Z, n, d, n_first, p, inv_eps, fin, old, sl, partial);
        PFM_TRY(hipGetLastError());
    }
    const int64_t gblocks = grad ? (n * d + NT - 1) / NT : 0;
    hipLaunchKernelGGL(k_sinkhorn_grad_finish, dim3((unsigned)(gblocks + 1)), dim3(NT), 0, st, (const double *)partial, n, d,
                       n_first, sl.count, fin, old, prev, n_sinkhorn > 0 ? 1 : 0, value, drift, grad, potentials);
    PFM_TRY(hipGetLastError());
    return PFM_OK;
}
