// pf_pairtile.h -- the ONE place a squared distance is formed in libpf_metrics.so, and how the pair matrix is cut into tiles.
//
// The pair matrix of two row sets is cut into TILE x TILE tiles.  A workgroup of NT = 256 threads forms one tile at a time:
// thread (ti, tj) = (tid >> 4, tid & 15) owns the 4 x 4 pairs of rows ti + 16 a and columns tj + 16 b.  The two row sets are
// staged through LDS in chunks of DC features, and d^2 is accumulated as fma(df, df, acc) over the features in order, in
// float64 (chunk_d2).  No square root is taken and no norm / dot-product identity is used.  Every kernel that needs a
// distance gets it from chunk_d2: pf_knn.hip, pf_nn.hip, pf_energy.hip, pf_perm.hip, pf_sinkhorn.hip and the row-gradient sweep of
// pf_gradsweep.h through tile_d2, pf_metrics.hip through its tile_d2_pooled, which differs in how it stages only.  So across
// kernels a duplicated row is at distance exactly 0, `d^2 < radius^2` compares values of one formula, and a statistic recomputed
// by another entry point has the same bits.  Only the distance and the tiles live here; how a sweep's column tiles are shared out
// over workgroups (Slices) is pf_gradsweep.h's.
#ifndef PF_PAIRTILE_H
#define PF_PAIRTILE_H

#include <math.h>

#include "pf_common.h"
#include "pf_metrics.h"

namespace {

constexpr int TILE = PFM_ENERGY_TILE;   // rows per side of a pair tile
constexpr int TPAD = TILE + 1;          // LDS row of one feature of a tile, and of a row of a tile kept in LDS (odd stride:
                                        // staging writes spread over the banks)
constexpr int DC = 16;                  // features staged per chunk
static_assert(TILE == 64 && NT == 256, "16 x 16 threads own 4 x 4 pairs each");

// ---- tiles ---------------------------------------------------------------------------------------------

__host__ __device__ inline int64_t tiles_per_side(int64_t n) { return (n + TILE - 1) / TILE; }
__host__ __device__ inline int64_t triangle_tiles(int64_t n) {      // tiles (I <= J) of the n x n matrix
    const int64_t nb = tiles_per_side(n);
    return nb * (nb + 1) / 2;
}

// random access: linear upper-triangle tile t -> block pair (bi <= bj), column-major (bj outer)
__device__ inline void tile_decode(int64_t t, int64_t &bi, int64_t &bj) {
    int64_t r = (int64_t)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
    while (r * (r + 1) / 2 > t) --r;
    while ((r + 1) * (r + 2) / 2 <= t) ++r;
    bj = r;
    bi = t - r * (r + 1) / 2;
}

// sequential access: the tiles (I, J) row by row, J < ntb; of the upper triangle (row I holds the ntb - I tiles (I, I) ..
// (I, ntb - 1)) or of the whole rectangle
struct TileWalk {
    int64_t I, J;
    __device__ void start(int64_t t, int64_t ntb, bool triangle) {
        if (triangle) {
            I = 0;
            while (t >= ntb - I) {
                t -= ntb - I;
                ++I;
            }
            J = I + t;
        } else {
            I = t / ntb;
            J = t - I * ntb;
        }
    }
    __device__ void advance(int64_t ntb, bool triangle) {
        if (++J == ntb) {
            ++I;
            J = triangle ? I : 0;
        }
    }
};

// ---- rows ----------------------------------------------------------------------------------------------
// A row source has n rows of d features and row(r), the first feature of row r < n.  Plain is a sample as it lies in memory;
// pf_metrics.hip (Pooled) and pf_knn.hip (Rows) gather resampled rows through index vectors.

struct Plain {
    const double *X;
    int64_t n, d;
    __device__ const double *row(int64_t r) const { return X + r * d; }
};

// features k0 .. k0 + dc - 1 of rows r0 .. r0 + TILE - 1 into sm[feature][row]; rows past the end are zeros
template <class Src>
__device__ inline void stage(const Src &s, int64_t r0, int64_t k0, int dc, double (*sm)[TPAD]) {
    for (int e = threadIdx.x; e < TILE * dc; e += NT) {
        const int row = e / dc, col = e - row * dc;
        const int64_t g = r0 + row;
        sm[col][row] = g < s.n ? s.row(g)[k0 + col] : 0.0;
    }
}

// acc += the squared differences over the dc features staged in sA / sB, for the 4 x 4 pairs a thread owns
__device__ inline void chunk_d2(const double (*sA)[TPAD], const double (*sB)[TPAD], int dc, double acc[4][4]) {
    const int tid = threadIdx.x, ti = tid >> 4, tj = tid & 15;
    for (int k = 0; k < dc; ++k) {
        double xa[4], yb[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) xa[a] = sA[k][ti + 16 * a];
#pragma unroll
        for (int b = 0; b < 4; ++b) yb[b] = sB[k][tj + 16 * b];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const double df = xa[a] - yb[b];
                acc[a][b] = fma(df, df, acc[a][b]);
            }
    }
}

// d^2 of the 4 x 4 pairs a thread owns: rows I0 + ti + 16 a of A against rows J0 + tj + 16 b of B (A.d == B.d).  Begins with
// a barrier: the previous tile's reads of sA / sB are done, and whatever the caller stored to LDS before the call is visible
// after it.  a_resident: A has one feature chunk (d <= DC) and the caller staged it in sA once for a whole sweep.
template <class SrcA, class SrcB>
__device__ inline void tile_d2(const SrcA &A, int64_t I0, const SrcB &B, int64_t J0, bool a_resident, double (*sA)[TPAD],
                               double (*sB)[TPAD], double acc[4][4]) {
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = 0.0;
    for (int64_t k0 = 0; k0 < A.d; k0 += DC) {
        const int dc = (int)((A.d - k0) < DC ? (A.d - k0) : DC);
        __syncthreads();                               // the previous chunk's (or tile's) reads are done
        if (!a_resident) stage(A, I0, k0, dc, sA);
        stage(B, J0, k0, dc, sB);
        __syncthreads();
        chunk_d2(sA, sB, dc, acc);
    }
}

}  // namespace

#endif
