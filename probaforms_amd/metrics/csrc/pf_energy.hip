// pf_energy.hip -- the energy distance's three pair sums for every bootstrap replicate, for gfx950 (C ABI: pf_metrics.h,
// pfm_energy).
//
// A bootstrap replicate is the original sample with integer draw counts c (k_counts of pf_scan1d.h), and its pair sum over
// a block of the pooled distance matrix is the quadratic form sum_ab c[a] c[b] |z_a - z_b|.  The distances do not depend on
// the replicate, so every distance is formed ONCE per group of replicates, on the ORIGINAL rows (nothing is gathered), and
// what is left per replicate and pair is one float64 multiply-add.  The decomposition, the count tiles and the last two
// reduction steps are pf_quadform.h's, the distances pf_pairtile.h's:
//   k_energy_tiles   a workgroup walks a list of TILE x TILE pair tiles of one block (RR, FF or RF; RR and FF walk the
//                    upper triangle of tiles, an off-diagonal tile weighs 2).  Per tile it forms the 64 x 64 distances
//                    (tile_d2, one sqrt) and keeps them in LDS as G.  Then, per block of RB replicates, it loads the two
//                    count tiles Ca[a, r] and Cb[b, r] as float64 (exact) and forms T[a, r] = sum_b G[a, b] Cb[b, r]: a
//                    wave owns a quarter of the b's, a lane a 4 x 4 micro-tile of T (rows ta + 16 i, replicates tr + 4 j)
//                    in registers, so 4 LDS reads of G and 4 of Cb feed 16 fmas.  The partial T (over the wave's b's) is
//                    multiplied by w Ca[a, r] and folded over a into the lane's accumulator of that replicate, which lives
//                    in a register across all the workgroup's tiles.  At the end of the list the 64 lanes that share a
//                    replicate (16 ta x 4 waves) are summed: an xor tree over the 16 lanes, then the 4 waves in index
//                    order through LDS, and the sum goes to partial[wg, r].
//   k_quad_finish<3> sums[r, q] = the partials of block q's workgroups in index order.
// Rows past a sample's end carry count 0 and the finite distance of an all-zero row; replicates past `reps` carry count 0
// and are not written.  The lists of tiles and their order depend on (nr, nf) only, and a replicate's place in the call
// decides which lanes hold it, never in which order its terms are added: a replicate's three sums are bitwise the same
// in any call.  No float atomics; the only atomics are k_counts' integer ones.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "pf_metrics.h"
#include "pf_quadform.h"
#include "pf_scan1d.h"

namespace {

struct Counts {                     // the weights of a block: the draw counts cnt [reps, N] of its two samples, exact in float64
    typedef int32_t raw_t;
    const int32_t *cnt;
    int64_t N, na, nb, offa, offb;  // rows of the a and the b sample, and their first columns in cnt
    __device__ int64_t rows(int side) const { return side ? nb : na; }
    __device__ raw_t load(int side, int64_t g, int64_t rep) const { return cnt[rep * N + (side ? offb : offa) + g]; }
    __device__ double weight(raw_t c) const { return (double)c; }
};

__global__ void __launch_bounds__(NT) k_energy_tiles(const double *Xr, int64_t nr, const double *Xf, int64_t nf, int64_t d,
                                                     const int32_t *cnt, int64_t reps, Plan p, double *partial) {
    __shared__ Shared sh;
    const int tid = threadIdx.x;
    const int64_t wg = blockIdx.x;
    const int64_t rep0 = (int64_t)blockIdx.y * SUPER;
    const int64_t left = reps - rep0;
    const int nrep = (int)(left < SUPER ? left : SUPER);          // replicates of this workgroup
    const int nrb = (nrep + RB - 1) / RB;

    const int q = wg >= p.first[2] ? 2 : (wg >= p.first[1] ? 1 : 0);
    const Plain A = {q == 1 ? Xf : Xr, q == 1 ? nf : nr, d}, B = {q == 0 ? Xr : Xf, q == 0 ? nr : nf, d};
    const Counts C = {cnt, nr + nf, A.n, B.n, q == 1 ? nr : 0, q == 0 ? 0 : nr};
    const bool triangle = q != 2;
    const int64_t ntb = q == 0 ? p.ta : p.tb;                       // tiles along b
    int64_t t = (wg - p.first[q]) * p.list;
    int64_t t_end = t + p.list;
    if (t_end > p.nt[q]) t_end = p.nt[q];
    TileWalk at;
    at.start(t, ntb, triangle);

    // G phase: thread (ti, tj) owns rows ti + 16 a, columns tj + 16 b.  T phase: wave w owns b = 16 w .. 16 w + 15, lane
    // (ta, tr) rows ta + 16 i and replicates tr + 4 j of the block
    const int ti = tid >> 4, tj = tid & 15;
    const int w = tid >> 6, ta = tid & 15, tr = (tid >> 4) & 3;

    double acc[NRB][4];
#pragma unroll
    for (int rb = 0; rb < NRB; ++rb)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[rb][j] = 0.0;

    for (; t < t_end; ++t) {
        const int64_t I0 = at.I * TILE, J0 = at.J * TILE;
        const double wgt = (triangle && at.I != at.J) ? 2.0 : 1.0;

        WeightTiles<Counts> wt = {C, tid, I0, J0, rep0, reps};
        wt.fetch(0);

        // ---- the tile's distances, once ----
        double dd[4][4];
        tile_d2(A, I0, B, J0, false, sh.u.st.A, sh.u.st.B, dd);
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) sh.G[ti + 16 * a][tj + 16 * b] = sqrt(dd[a][b]);

        // ---- T = G C per block of replicates, folded into the accumulators ----
#pragma unroll
        for (int rb = 0; rb < NRB; ++rb) {
            if (rb < nrb) {                        // (uniform over the workgroup)
                __syncthreads();                   // G is written; the staged chunks / the previous count tiles are read
                wt.store(sh.u.C);
                __syncthreads();
                if (rb + 1 < nrb) wt.fetch(rb + 1);   // in flight under the fmas below

                double T[4][4];
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) T[i][j] = 0.0;
#pragma unroll 4
                for (int k = 0; k < TILE / 4; ++k) {
                    const int b = 16 * w + k;
                    double dv[4], cv[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) dv[i] = sh.G[ta + 16 * i][b];
#pragma unroll
                    for (int j = 0; j < 4; ++j) cv[j] = sh.u.C[1][b][tr + 4 * j];
#pragma unroll
                    for (int i = 0; i < 4; ++i)
#pragma unroll
                        for (int j = 0; j < 4; ++j) T[i][j] = fma(dv[i], cv[j], T[i][j]);
                }
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        acc[rb][j] = fma(wgt * sh.u.C[0][ta + 16 * i][tr + 4 * j], T[i][j], acc[rb][j]);
            }
        }
        at.advance(ntb, triangle);
    }

    // ---- the 64 lanes of a replicate: xor tree over ta, then the waves in index order ----
#pragma unroll
    for (int rb = 0; rb < NRB; ++rb)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            double v = acc[rb][j];
#pragma unroll
            for (int s = 1; s < 16; s <<= 1) v = v + __shfl_xor(v, s, 16);
            acc[rb][j] = v;
        }
    __syncthreads();                               // the last tile's count tiles are read
    if (ta == 0) {
#pragma unroll
        for (int rb = 0; rb < NRB; ++rb)
#pragma unroll
            for (int j = 0; j < 4; ++j) sh.u.red[w][rb * RB + tr + 4 * j] = acc[rb][j];
    }
    waves_to_partial(sh.u.red, nrep, partial + wg * reps + rep0);
}

}  // namespace

// ---- C ABI --------------------------------------------------------------------------------------------

extern "C" size_t pfm_energy_workspace_bytes(int64_t nr, int64_t nf, int64_t d, int64_t reps) {
    if (!pair_sizes_ok(nr, nf, d, reps)) return 0;
    const Plan p = plan_of(nr, nf);
    return align256(sizeof(int32_t) * (size_t)reps * (size_t)(nr + nf)) +
           align256(sizeof(double) * (size_t)reps * (size_t)p.first[3]);
}

extern "C" int pfm_energy(void *stream, const double *Xr, int64_t nr, const double *Xf, int64_t nf, int64_t d,
                          const int32_t *idx_r, const int32_t *idx_f, int64_t reps, double *sums, void *workspace,
                          size_t workspace_bytes) {
    if (!Xr || !Xf || !idx_r || !idx_f || !sums || !pair_sizes_ok(nr, nf, d, reps)) return PFM_EINVAL;
    const size_t need = pfm_energy_workspace_bytes(nr, nf, d, reps);
    if (!workspace || workspace_bytes < need) return PFM_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const Plan p = plan_of(nr, nf);
    int32_t *cnt = (int32_t *)workspace;
    double *partial = (double *)((char *)workspace + align256(sizeof(int32_t) * (size_t)reps * (size_t)(nr + nf)));

    PFM_TRY(launch_counts(st, idx_r, idx_f, nr, nf, reps, cnt));
    const dim3 grid((unsigned)p.first[3], (unsigned)((reps + SUPER - 1) / SUPER));
    hipLaunchKernelGGL(k_energy_tiles, grid, dim3(NT), 0, st, Xr, nr, Xf, nf, d, (const int32_t *)cnt, reps, p, partial);
    PFM_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_quad_finish<3>, dim3((unsigned)((3 * reps + NT - 1) / NT)), dim3(NT), 0, st,
                       (const double *)partial, reps, p, sums);
    PFM_TRY(hipGetLastError());
    return PFM_OK;
}
