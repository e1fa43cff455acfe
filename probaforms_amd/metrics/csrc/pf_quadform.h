// pf_quadform.h -- what k_energy_tiles (pf_energy.hip) and k_perm_tiles (pf_perm.hip) share.  Both sum, for every replicate r
// of a group, quadratic forms sum_ab w[a, r] w[b, r] G(a, b) over blocks of a pair matrix whose G does not depend on r:
//   * the blocks are cut into lists of TILE x TILE tiles, one list per workgroup (Plan, and TileWalk of pf_pairtile.h); a
//     workgroup serves up to SUPER replicates (grid.y) in blocks of RB;
//   * per tile G is formed once and kept in LDS (Shared); per block of RB replicates the two weight tiles w[a, r], w[b, r]
//     are prefetched in registers and stored to LDS as float64 (WeightTiles); how a fetched element becomes a weight is the
//     kernel's policy W: the draw count for the energy distance, +n_second / -n_first / 0 for a labelling;
//   * T = G w and its fold into the lane's accumulators is the kernel's own, and so is the sum over the lanes of a wave that
//     share a replicate: both are tied to where the T phase leaves its values, and a shared form would reorder float64
//     additions.  What follows is shared: the waves in index order into partial[wg, r] (waves_to_partial), then the
//     workgroups of a block in index order (k_quad_finish).
// The lists and their order depend on the blocks' sizes only, and a replicate's place in the call decides which lanes hold it,
// never in which order its terms are added.  No float atomics.
#ifndef PF_QUADFORM_H
#define PF_QUADFORM_H

#include "pf_pairtile.h"

namespace {

constexpr int RB = PFM_ENERGY_REP_BLOCK;   // replicates per weight tile
constexpr int RBP = RB + 1;                // LDS stride of a weight-tile row
constexpr int SUPER = 128;                 // replicates per workgroup (grid.y): SUPER / RB accumulator sets in registers
constexpr int NRB = SUPER / RB;
constexpr int WPT = 2 * TILE * RB / NT;    // elements of the two weight tiles per thread
constexpr int64_t MIN_LIST = 4;            // tiles per workgroup, at least
constexpr int64_t TARGET_WGS = 2048;       // workgroups per call, about (beyond it the lists grow instead)
static_assert(RB == 16 && WPT == 8, "the lane layouts are written for 64 x 64 tiles and 16 replicates");

struct Plan {                       // the decomposition: a function of (na, nb) only
    int64_t ta, tb;                 // tiles per side of sample a and of sample b
    int64_t nt[3];                  // tiles of block AA (upper triangle), BB (upper triangle), AB
    int64_t list;                   // tiles per workgroup (the last workgroup of a block may have fewer)
    int64_t first[4];               // workgroups of block q: first[q] .. first[q + 1] - 1
};

// nb = 0: one pooled block, the upper triangle of sample a, in workgroups 0 .. first[1] - 1
__host__ inline Plan plan_of(int64_t na, int64_t nb) {
    Plan p;
    p.ta = tiles_per_side(na);
    p.tb = tiles_per_side(nb);
    p.nt[0] = triangle_tiles(na);
    p.nt[1] = triangle_tiles(nb);
    p.nt[2] = p.ta * p.tb;
    const int64_t total = p.nt[0] + p.nt[1] + p.nt[2];
    p.list = (total + TARGET_WGS - 1) / TARGET_WGS;
    if (p.list < MIN_LIST) p.list = MIN_LIST;
    p.first[0] = 0;
    for (int q = 0; q < 3; ++q) p.first[q + 1] = p.first[q] + (p.nt[q] + p.list - 1) / p.list;
    return p;
}

struct Shared {
    double G[TILE][TPAD];                          // the tile's pair values
    union {
        struct { double A[DC][TPAD], B[DC][TPAD]; } st;   // staged feature chunks (while G is formed)
        double C[2][TILE][RBP];                    // weight tiles of the a rows and the b rows (while T is formed)
        double red[NT / 64][SUPER];                // the waves' sums per replicate (after the last tile)
    } u;
};

// The two weight tiles of the tile at rows I0, columns J0, as this thread stages them: element e = tid + NT s of a block of RB
// replicates is (side, replicate, row).  fetch(rb) loads block rb's elements into registers, store() puts the fetched block into
// C[side][row][replicate] as float64.  A policy W has raw_t, rows(side), load(side, row, replicate) and weight(raw); a row past
// the end of its sample, or a replicate past the end of the call, is raw_t 0.  (A struct with member functions, like the
// closures it replaces: as free functions taking `pre` the same code left k_energy_tiles ten registers over its 256.)
template <class W>
struct WeightTiles {
    const W w;
    int tid;
    int64_t I0, J0, rep0, reps;
    typename W::raw_t pre[WPT];
    __device__ void fetch(int rb) {
#pragma unroll
        for (int s = 0; s < WPT; ++s) {
            const int e = tid + NT * s;
            const int side = e >> 10, r = (e >> 6) & (RB - 1), row = e & (TILE - 1);
            const int64_t g = (side ? J0 : I0) + row, rep = rep0 + rb * RB + r;
            const bool in = g < w.rows(side) && rep < reps;
            pre[s] = in ? w.load(side, g, rep) : (typename W::raw_t)0;
        }
    }
    __device__ void store(double (*C)[TILE][RBP]) const {
#pragma unroll
        for (int s = 0; s < WPT; ++s) {
            const int e = tid + NT * s;
            C[e >> 10][e & (TILE - 1)][(e >> 6) & (RB - 1)] = w.weight(pre[s]);
        }
    }
};

// red[wave][replicate] holds the waves' sums: the waves in index order, to out[replicate]
__device__ inline void waves_to_partial(const double (*red)[SUPER], int nrep, double *out) {
    const int tid = threadIdx.x;
    __syncthreads();
    if (tid < nrep) {
        double s = red[0][tid];
#pragma unroll
        for (int v = 1; v < NT / 64; ++v) s = s + red[v][tid];
        out[tid] = s;
    }
}

// sums[r, q] = the partials of block q's workgroups in index order, q < NB
template <int NB>
__global__ void __launch_bounds__(NT) k_quad_finish(const double *__restrict__ partial, int64_t reps, Plan p,
                                                    double *__restrict__ sums) {
    const int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x;      // q-major, so that a wave reads neighbouring replicates
    if (e >= NB * reps) return;
    const int64_t q = NB == 1 ? 0 : e / reps, r = e - q * reps;
    double s = 0.0;
#pragma unroll 8
    for (int64_t wg = p.first[q]; wg < p.first[q + 1]; ++wg) s = s + partial[wg * reps + r];
    sums[r * NB + q] = s;
}

}  // namespace

#endif
