// pf_sinkhorn.hip -- the debiased Sinkhorn divergence of every bootstrap replicate, for gfx950 (C ABI: pf_metrics.h,
// pfm_sinkhorn).
//
// A bootstrap replicate is the original sample with marginal weights count / n (k_counts of pf_scan1d.h), and the cost matrix
// C(x, y) = |x - y|^p does not depend on the replicate.  So nothing is gathered and nothing of the size of the pair matrix is
// stored: every iteration re-forms the costs tile by tile on the ORIGINAL rows (tile_d2 of pf_pairtile.h), once per block of RB
// replicates, and what a replicate costs per pair and iteration is one float64 exp.
//
// The pooled rows z = [R; F] (N = nr + nf) carry two potentials each, pot[rep][slot][N]:
//   slot 0  the cross potential: f on a real row (against F), g on a fake row (against R)
//   slot 1  the self potential:  u on a real row (against R), v on a fake row (against F)
// so a row's softmin against the columns of one sample reads and writes slot (row's sample == columns' sample).
//   k_logw           lw[rep][i] = log(count / n) of a pooled row, -inf (the constant, no log is taken) for count 0
//   k_sinkhorn_step  one symmetrised Jacobi step for all four potentials.  A workgroup owns a strip of TILE rows of one sample
//                    (grid.x) and a block of RB replicates (grid.y).  It walks the column tiles of R, then those of F.  Per tile
//                    it forms the TILE x TILE costs once, scaled by 1 / eps, and keeps them in LDS as G, next to
//                    hl[column][replicate] = h / eps + lw of the tile's columns.  Then thread (row = lane, wave w) folds the
//                    tile into the running (max, sum) of its row for the replicates 4 w .. 4 w + 3, flash-attention style: the
//                    tile's row maximum without an exp, one rescaling exp per row and tile, one exp per pair.  After the
//                    last tile of a sample the softmin -eps (max + log sum) is averaged with the old potential (or, in the
//                    last step, stored as it is) into the other buffer: potentials ping-pong, every step reads old values only.
//   k_sinkhorn_finish  value = sum_i w_i (pot[0][i] - pot[1][i]) over the rows of non-zero count, a strided sum per thread and
//                    a tree over the threads; drift = the largest |change| of such a row's potentials in the last averaged step
//                    (sinkhorn_value_drift of pf_scan1d.h, which pf_sinkgrad.hip's finish uses with the weights 1 / n).
// A (row, replicate) pair is folded by one thread over the columns in index order: the order of every sum depends on
// (nr, nf, d) only, and a replicate's value, drift and potentials are bitwise the same alone, in any group, in any call.  A
// column of count 0 (or past the end of its sample) carries hl = -inf and adds exp(-inf) = 0; a tile of such columns alone is
// skipped, so no (-inf) - (-inf) is formed.  No float atomics; the only atomics are k_counts' integer ones.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "pf_metrics.h"
#include "pf_pairtile.h"
#include "pf_scan1d.h"

namespace {

constexpr int RB = PFM_ENERGY_REP_BLOCK;   // replicates per workgroup: 4 per wave
constexpr int RBP = RB + 1;
constexpr int RPW = RB / (NT / 64);        // replicates a wave folds
constexpr int64_t MAX_SINKHORN = 1000000;  // launches per call, at most
static_assert(RPW == 4 && TILE == 64, "a lane owns a row of the strip, a wave 4 replicates");

struct SkShared {
    double G[TILE][TPAD];               // the tile's costs / eps
    double A[DC][TPAD], B[DC][TPAD];    // staged feature chunks: the strip's rows (resident for d <= DC), the tile's columns
    double hl[TILE][RBP];               // h / eps + log w of the tile's columns, per replicate of the block
};

__global__ void __launch_bounds__(NT) k_logw(const int32_t *__restrict__ cnt, int64_t nr, int64_t nf, int64_t reps,
                                             double *__restrict__ lw) {
    const int64_t N = nr + nf, total = reps * N;
    for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < total; e += (int64_t)gridDim.x * NT) {
        const int64_t i = e % N;
        const int32_t c = cnt[e];
        lw[e] = c > 0 ? log((double)c / (double)(i < nr ? nr : nf)) : -INFINITY;
    }
}

__global__ void __launch_bounds__(NT) k_sinkhorn_step(const double *Xr, int64_t nr, const double *Xf, int64_t nf, int64_t d,
                                                      const double *__restrict__ lw, int64_t reps, int p, double eps,
                                                      double inv_eps, const double *__restrict__ src,
                                                      double *__restrict__ dst, int averaged) {
    __shared__ SkShared sh;
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    const int ti = tid >> 4, tj = tid & 15;
    const int64_t N = nr + nf, ta = tiles_per_side(nr), tb = tiles_per_side(nf);
    const int64_t strip = blockIdx.x;
    const int rside = strip >= ta ? 1 : 0;
    const int64_t I0 = (rside ? strip - ta : strip) * TILE, roff = rside ? nr : 0;
    const int64_t rep0 = (int64_t)blockIdx.y * RB;
    const Plain A = {rside ? Xf : Xr, rside ? nf : nr, d};
    const bool resident = d <= DC;
    if (resident) stage(A, I0, 0, (int)d, sh.A);     // visible after tile_d2's barriers

    for (int cside = 0; cside < 2; ++cside) {
        const Plain B = {cside ? Xf : Xr, cside ? nf : nr, d};
        const int64_t coff = cside ? nr : 0, ntc = cside ? tb : ta;
        const int slot = rside == cside ? 1 : 0;
        double m[RPW], s[RPW];
#pragma unroll
        for (int j = 0; j < RPW; ++j) {
            m[j] = -INFINITY;
            s[j] = 0.0;
        }

        for (int64_t J = 0; J < ntc; ++J) {
            const int64_t J0 = J * TILE;
            // the tile's column terms, element e = tid + NT q -> (replicate e >> 6, column e & 63): in flight under tile_d2
            double hv[TILE * RB / NT];
#pragma unroll
            for (int q = 0; q < TILE * RB / NT; ++q) {
                const int e = tid + NT * q;
                const int64_t g = J0 + (e & (TILE - 1)), rep = rep0 + (e >> 6);
                hv[q] = -INFINITY;
                if (g < B.n && rep < reps) {
                    const double l = lw[rep * N + coff + g];
                    if (l > -INFINITY) hv[q] = fma(src[(rep * 2 + slot) * N + coff + g], inv_eps, l);
                }
            }

            double dd[4][4];
            tile_d2(A, I0, B, J0, resident, sh.A, sh.B, dd);      // begins with a barrier: the previous tile's folds are done
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) sh.G[ti + 16 * a][tj + 16 * b] = (p == 1 ? sqrt(dd[a][b]) : dd[a][b]) * inv_eps;
#pragma unroll
            for (int q = 0; q < TILE * RB / NT; ++q) {
                const int e = tid + NT * q;
                sh.hl[e & (TILE - 1)][e >> 6] = hv[q];
            }
            __syncthreads();

#pragma unroll
            for (int j = 0; j < RPW; ++j) {
                const int r = RPW * w + j;
                if (rep0 + r < reps) {                             // (uniform over the wave)
                    double tm = -INFINITY;
#pragma unroll 8
                    for (int k = 0; k < TILE; ++k) tm = fmax(tm, sh.hl[k][r] - sh.G[lane][k]);
                    if (tm > -INFINITY) {                          // (uniform over the wave: G is finite)
                        const double M = fmax(m[j], tm);
                        double acc = s[j] * exp(m[j] - M);
#pragma unroll 4
                        for (int k = 0; k < TILE; ++k) acc = acc + exp((sh.hl[k][r] - sh.G[lane][k]) - M);
                        s[j] = acc;
                        m[j] = M;
                    }
                }
            }
        }

        // the softmin of the strip's rows against this sample's columns
        const int64_t g = I0 + lane;
        if (g < A.n) {
#pragma unroll
            for (int j = 0; j < RPW; ++j) {
                const int64_t rep = rep0 + RPW * w + j;
                if (rep < reps) {
                    const double sm = -eps * (m[j] + log(s[j]));
                    const int64_t at = (rep * 2 + slot) * N + roff + g;
                    dst[at] = averaged ? 0.5 * (src[at] + sm) : sm;
                }
            }
        }
    }
}

// one workgroup per replicate
__global__ void __launch_bounds__(NT) k_sinkhorn_finish(const int32_t *__restrict__ cnt, int64_t nr, int64_t nf,
                                                        const double *__restrict__ fin, const double *__restrict__ cur,
                                                        const double *__restrict__ prev, int has_prev,
                                                        double *__restrict__ value, double *__restrict__ drift,
                                                        double *__restrict__ potentials) {
    __shared__ double sd[NT];
    const int tid = threadIdx.x;
    const int64_t rep = blockIdx.x, N = nr + nf;
    const int32_t *c = cnt + rep * N;
    const double *f = fin + rep * 2 * N;
    double total, dr;
    sinkhorn_value_drift(f, cur + rep * 2 * N, prev + rep * 2 * N, has_prev, N, [=](int64_t i) {
        const int32_t ci = c[i];
        return ci > 0 ? (double)ci / (double)(i < nr ? nr : nf) : 0.0;
    }, sd, total, dr);
    if (tid == 0) {
        value[rep] = total;
        drift[rep] = dr;
    }
    if (potentials)
        for (int64_t i = tid; i < 2 * N; i += NT) potentials[rep * 2 * N + i] = f[i];
}

struct Layout {                     // the workspace: draw counts, log-weights, three potential buffers
    size_t cnt, lw, pot, total;     // bytes of the counts, of the log-weights, of ONE potential buffer, of everything
};

Layout layout_of(int64_t nr, int64_t nf, int64_t reps) {
    const size_t rows = (size_t)reps * (size_t)(nr + nf);
    Layout l;
    l.cnt = align256(sizeof(int32_t) * rows);
    l.lw = align256(sizeof(double) * rows);
    l.pot = align256(sizeof(double) * 2 * rows);
    l.total = l.cnt + l.lw + 3 * l.pot;
    return l;
}

}  // namespace

// ---- C ABI --------------------------------------------------------------------------------------------

extern "C" size_t pfm_sinkhorn_workspace_bytes(int64_t nr, int64_t nf, int64_t d, int64_t reps) {
    if (!pair_sizes_ok(nr, nf, d, reps)) return 0;
    return layout_of(nr, nf, reps).total;
}

extern "C" int pfm_sinkhorn(void *stream, const double *Xr, int64_t nr, const double *Xf, int64_t nf, int64_t d,
                            const int32_t *idx_r, const int32_t *idx_f, int64_t reps, int p, double eps, int64_t n_sinkhorn,
                            double *value, double *drift, double *potentials, void *workspace, size_t workspace_bytes) {
    if (!Xr || !Xf || !idx_r || !idx_f || !value || !drift || !pair_sizes_ok(nr, nf, d, reps)) return PFM_EINVAL;
    if (!(eps > 0.0) || !isfinite(eps) || !isfinite(1.0 / eps) || n_sinkhorn < 0 || n_sinkhorn > MAX_SINKHORN)
        return PFM_EINVAL;
    if (p != 1 && p != 2) return PFM_EUNSUPPORTED;
    const Layout l = layout_of(nr, nf, reps);
    if (!workspace || workspace_bytes < l.total) return PFM_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int64_t N = nr + nf;
    char *base = (char *)workspace;
    int32_t *cnt = (int32_t *)base;
    double *lw = (double *)(base + l.cnt);
    double *pot[3];
    for (int k = 0; k < 3; ++k) pot[k] = (double *)(base + l.cnt + l.lw + k * l.pot);

    PFM_TRY(hipMemsetAsync(pot[0], 0, sizeof(double) * 2 * (size_t)reps * (size_t)N, st));   // every potential starts at 0
    PFM_TRY(launch_counts(st, idx_r, idx_f, nr, nf, reps, cnt));
    int64_t lb = (reps * N + NT - 1) / NT;
    if (lb > 4096) lb = 4096;
    hipLaunchKernelGGL(k_logw, dim3((unsigned)lb), dim3(NT), 0, st, (const int32_t *)cnt, nr, nf, reps, lw);
    PFM_TRY(hipGetLastError());

    const dim3 grid((unsigned)(tiles_per_side(nr) + tiles_per_side(nf)), (unsigned)((reps + RB - 1) / RB));
    const double inv_eps = 1.0 / eps;
    for (int64_t it = 0; it <= n_sinkhorn; ++it) {
        const bool last = it == n_sinkhorn;
        hipLaunchKernelGGL(k_sinkhorn_step, grid, dim3(NT), 0, st, Xr, nr, Xf, nf, d, (const double *)lw, reps, p, eps,
                           inv_eps, (const double *)pot[it & 1], last ? pot[2] : pot[(it + 1) & 1], last ? 0 : 1);
        PFM_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(k_sinkhorn_finish, dim3((unsigned)reps), dim3(NT), 0, st, (const int32_t *)cnt, nr, nf,
                       (const double *)pot[2], (const double *)pot[n_sinkhorn & 1], (const double *)pot[(n_sinkhorn + 1) & 1],
                       n_sinkhorn > 0 ? 1 : 0, value, drift, potentials);
    PFM_TRY(hipGetLastError());
    return PFM_OK;
}
