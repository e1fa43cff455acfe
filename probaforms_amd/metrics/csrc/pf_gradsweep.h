// pf_gradsweep.h -- the row-gradient sweep over the pairs of the pooled rows that pf_pairgrad.hip and pf_sinkgrad.hip share:
//   dL/dz_a = scale(a) sum_b coef_ab (z_a - z_b)
// A workgroup (I, s, fc) owns the 64 rows of row block I, the column tiles of slice s and the features 16 fc .. 16 fc + 15 of
// the gradient (row_grad_sweep); a finish kernel sums the slices' partials [slices, n, d] in index order (finish_rows).  What a
// pair's coefficient is, the kernel says with its Coef.  The slices depend on (n, d) only and there are no float atomics.
#ifndef PF_GRADSWEEP_H
#define PF_GRADSWEEP_H

#include "pf_pairtile.h"

namespace {

struct Slices {             // how the column tiles of a row block are shared out; a function of (n, d) only
    int64_t nb;             // tiles per side
    int64_t fc;             // feature chunks of the gradient
    int64_t per;            // column tiles per slice
    int64_t count;          // slices
};

constexpr int64_t TARGET_WORKGROUPS = 1024;    // about four per CU of the device the library is written for

__host__ inline Slices slices_of(int64_t n, int64_t d) {
    Slices s;
    s.nb = tiles_per_side(n);
    s.fc = (d + DC - 1) / DC;
    int64_t want = (TARGET_WORKGROUPS + s.nb * s.fc - 1) / (s.nb * s.fc);
    if (want < 1) want = 1;
    if (want > s.nb) want = s.nb;
    s.per = (s.nb + want - 1) / want;
    s.count = (s.nb + s.per - 1) / s.per;
    return s;
}

// the sizes such a sweep and its finish accept: n pooled rows of d features, the first n_first of the first sample
inline bool pair_args_ok(int64_t n, int64_t d, int64_t n_first) {
    if (n < 2 || n > (int64_t)INT32_MAX || d < 1 || d > 65535 * (int64_t)DC) return false;      // feature chunks are grid.z
    if (n_first < 1 || n_first >= n) return false;
    const Slices sl = slices_of(n, d);
    if (sl.count > 65535) return false;                                                           // slices are grid.y
    if (d > INT64_MAX / n / sl.count / (int64_t)sizeof(double) / 2) return false;                 // the partials' bytes overflow
    if ((n * d + NT - 1) / NT + 1 > (int64_t)INT32_MAX) return false;                             // the finish's grid.x
    return true;
}

// the workspace bytes of partial [slices, n, d]
inline size_t partial_bytes(const Slices &sl, int64_t n, int64_t d) { return align256(sizeof(double) * (size_t)(sl.count * n * d)); }

// The sweep of workgroup (blockIdx.x, .y, .z) = (I, s, fc) over the pooled rows Z [n, d].  Per column tile it forms d^2
// (tile_d2), has coef turn the 4 x 4 values a thread owns into coef_ab, and accumulates sum_b coef_ab (z_a[k] - z_b[k]) per owned
// row and feature in registers (4 rows x GF features: 4 for d <= 4, else DC) across its whole slice.  For d <= DC the row block's
// features stay staged in LDS for the sweep (tile_d2's a_resident) and the column tile tile_d2 staged is read again for the
// differences; for wider rows the gradient's chunk of both sides is staged beside the chunks tile_d2 walks, and every feature
// chunk's workgroup re-forms d^2 over all d features.  At the end of the slice the 16 lanes that share a row are summed (xor
// tree) and written to partial[s, a, k].  The difference z_a - z_b is taken feature by feature, as chunk_d2 takes it.
//   coef.columns(J0)   before a tile's staging: whatever the tile's columns J0 + tj + 16 b need, its loads in flight under tile_d2
//   coef.pair(a, b, d2, row_first, col_first, ok) -> coef_ab of owned pair (a, b); row_first / col_first: the row / the column
//                      is of the first sample; !ok: the row or the column lies past n, and the pair's terms are SELECTED to 0
//                      (a finite row far from the origin is at an infinite d^2 from the all-zero row that pads a tile)
// GRAD false: coef.pair is called for what it accumulates itself, and nothing else is formed or stored.
template <bool GRAD, int GF, class Coef>
__device__ __forceinline__ void row_grad_sweep(const double *Z, int64_t n, int64_t d, int64_t n_first, const Slices &sl,
                                               Coef &coef, double *partial) {
    __shared__ double sA[DC][TPAD], sB[DC][TPAD];          // the chunks tile_d2 walks
    __shared__ double xA[DC][TPAD], xB[DC][TPAD];          // d > DC: the gradient's chunk of the rows and of the column tile
    const int tid = threadIdx.x, ti = tid >> 4, tj = tid & 15;
    const int64_t I0 = (int64_t)blockIdx.x * TILE;
    const int64_t s = blockIdx.y;
    const int64_t k0 = (int64_t)blockIdx.z * DC;           // first feature of this workgroup's gradient chunk
    const int dcg = (int)((d - k0) < DC ? (d - k0) : DC);
    const bool resident = d <= DC;
    const Plain pooled = {Z, n, d};

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
    if (GRAD) {
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int k = 0; k < GF; ++k) G[a][k] = 0.0;
    }

    for (; J < J_end; ++J) {
        const int64_t J0 = J * TILE;
        coef.columns(J0);
        if (GRAD && !resident) {
            __syncthreads();                               // the previous tile's reads of xB are done
            stage(pooled, J0, k0, dcg, xB);
        }
        double dd[4][4];
        tile_d2(pooled, I0, pooled, J0, resident, sA, sB, dd);

        // ---- dd <- coef_ab ----
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int64_t cb = J0 + tj + 16 * b;
            const bool col_ok = cb < n, col_first = cb < n_first;
#pragma unroll
            for (int a = 0; a < 4; ++a)
                dd[a][b] = coef.pair(a, b, dd[a][b], 16 * a < first_left, col_first, col_ok && 16 * a < rows_left);
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
}

// the row part of a finish kernel, workgroups 0 .. gridDim.x - 2: grad[e] = scale(a) (the slices' partials of element
// e = a d + k in index order)
template <class Scale>
__device__ inline void finish_rows(const double *partial, int64_t n, int64_t d, int64_t slices, Scale scale, double *grad) {
    const int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (e < n * d) {
        double v = partial[e];
        for (int64_t s = 1; s < slices; ++s) v = v + partial[s * n * d + e];
        grad[e] = scale(e / d) * v;
    }
}

}  // namespace

#endif
