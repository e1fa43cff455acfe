// pf_energy.hip -- the energy distance's three pair sums for every bootstrap replicate, for gfx950 (C ABI: pf_metrics.h,
// pfm_energy).
//
// A bootstrap replicate is the original sample with integer draw counts c (k_counts of pf_scan1d.h), and its pair sum over
// a block of the pooled distance matrix is the quadratic form sum_ab c[a] c[b] |z_a - z_b|.  The distances do not depend on
// the replicate, so every distance is formed ONCE per group of replicates, on the ORIGINAL rows (nothing is gathered), and
// what is left per replicate and pair is one float64 multiply-add:
//   k_energy_tiles   a workgroup walks a list of TILE x TILE pair tiles of one block (RR, FF or RF; RR and FF walk the
//                    upper triangle of tiles, an off-diagonal tile weighs 2).  Per tile it stages the two row sets through
//                    LDS in chunks of 16 features, forms the 64 x 64 distances (fma(df, df, acc) over the features in
//                    order, one sqrt) and keeps them in LDS as D.  Then, per block of REP_BLOCK replicates, it loads the two
//                    count tiles Ca[a, r] and Cb[b, r] as float64 (exact) and forms T[a, r] = sum_b D[a, b] Cb[b, r]: a
//                    wave owns a quarter of the b's, a lane a 4 x 4 micro-tile of T (rows ta + 16 i, replicates tr + 4 j)
//                    in registers, so 4 LDS reads of D and 4 of Cb feed 16 fmas.  The partial T (over the wave's b's) is
//                    multiplied by w Ca[a, r] and folded over a into the lane's accumulator of that replicate, which lives
//                    in a register across all the workgroup's tiles.  At the end of the list the 64 lanes that share a
//                    replicate (16 ta x 4 waves) are summed: an xor tree over the 16 lanes, then the 4 waves in index
//                    order through LDS, and the sum goes to partial[wg, r].
//   k_energy_finish  sums[r, q] = the partials of block q's workgroups in index order.
// Rows past a sample's end carry count 0 and the finite distance of an all-zero row; replicates past `reps` carry count 0
// and are not written.  The lists of tiles and their order depend on (nr, nf) only, and a replicate's place in the call
// decides which lanes hold it, never in which order its terms are added: a replicate's three sums are bitwise the same
// in any call.  No float atomics; the only atomics are k_counts' integer ones.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "pf_metrics.h"
#include "pf_scan1d.h"

namespace {

constexpr int TILE = PFM_ENERGY_TILE;      // rows per side of a pair tile
constexpr int TPAD = TILE + 1;             // odd LDS stride of a staged feature and of a row of D
constexpr int DC = 16;                     // features staged per chunk
constexpr int RB = PFM_ENERGY_REP_BLOCK;   // replicates per count tile
constexpr int RBP = RB + 1;                // LDS stride of a count-tile row
constexpr int SUPER = 128;                 // replicates per workgroup (grid.y): SUPER / RB accumulator sets in registers
constexpr int NRB = SUPER / RB;
constexpr int64_t MIN_LIST = 4;            // tiles per workgroup, at least
constexpr int64_t TARGET_WGS = 2048;       // workgroups per call, about (beyond it the lists grow instead)
static_assert(TILE == 64 && RB == 16 && NT == 256, "the lane layout below is written for 64 x 64 tiles and 16 replicates");

__host__ __device__ inline int64_t tiles_of(int64_t n) { return (n + TILE - 1) / TILE; }

struct Plan {                       // the decomposition: a function of (nr, nf) only
    int64_t tr, tf;                 // tiles per side
    int64_t nt[3];                  // tiles of RR (upper triangle), FF (upper triangle), RF
    int64_t list;                   // tiles per workgroup (the last workgroup of a block may have fewer)
    int64_t first[4];               // workgroups of block q: first[q] .. first[q + 1] - 1
};

__host__ inline Plan plan_of(int64_t nr, int64_t nf) {
    Plan p;
    p.tr = tiles_of(nr);
    p.tf = tiles_of(nf);
    p.nt[0] = p.tr * (p.tr + 1) / 2;
    p.nt[1] = p.tf * (p.tf + 1) / 2;
    p.nt[2] = p.tr * p.tf;
    const int64_t total = p.nt[0] + p.nt[1] + p.nt[2];
    p.list = (total + TARGET_WGS - 1) / TARGET_WGS;
    if (p.list < MIN_LIST) p.list = MIN_LIST;
    p.first[0] = 0;
    for (int q = 0; q < 3; ++q) p.first[q + 1] = p.first[q] + (p.nt[q] + p.list - 1) / p.list;
    return p;
}

// features k0 .. k0 + dc - 1 of rows r0 .. r0 + 63 of X [n, d] into sm[feature][row]; rows past the end are zeros
__device__ inline void stage(const double *X, int64_t n, int64_t d, int64_t r0, int64_t k0, int dc, double (*sm)[TPAD]) {
    for (int e = threadIdx.x; e < TILE * dc; e += NT) {
        const int row = e / dc, col = e - row * dc;
        const int64_t g = r0 + row;
        sm[col][row] = g < n ? X[g * d + k0 + col] : 0.0;
    }
}

struct Shared {
    double D[TILE][TPAD];                          // the tile's distances
    union {
        struct { double A[DC][TPAD], B[DC][TPAD]; } st;   // staged feature chunks (while D is formed)
        double C[2][TILE][RBP];                    // count tiles of the a rows and the b rows (while T is formed)
        double red[NT / 64][SUPER];                // the waves' sums per replicate (after the last tile)
    } u;
};

__global__ void __launch_bounds__(NT) k_energy_tiles(const double *Xr, int64_t nr, const double *Xf, int64_t nf, int64_t d,
                                                     const int32_t *cnt, int64_t reps, Plan p, double *partial) {
    __shared__ Shared sh;
    const int tid = threadIdx.x;
    const int64_t wg = blockIdx.x, N = nr + nf;
    const int64_t rep0 = (int64_t)blockIdx.y * SUPER;
    const int64_t left = reps - rep0;
    const int nrep = (int)(left < SUPER ? left : SUPER);          // replicates of this workgroup
    const int nrb = (nrep + RB - 1) / RB;

    const int q = wg >= p.first[2] ? 2 : (wg >= p.first[1] ? 1 : 0);
    const double *XA = q == 1 ? Xf : Xr, *XB = q == 0 ? Xr : Xf;
    const int64_t na = q == 1 ? nf : nr, nb = q == 0 ? nr : nf;
    const int64_t offa = q == 1 ? nr : 0, offb = q == 0 ? 0 : nr;  // the samples' first columns in cnt [reps, N]
    const int64_t ntb = q == 0 ? p.tr : p.tf;                       // tiles along b
    int64_t t = (wg - p.first[q]) * p.list;
    int64_t t_end = t + p.list;
    if (t_end > p.nt[q]) t_end = p.nt[q];
    int64_t I, J;
    if (q == 2) {
        I = t / ntb;
        J = t - I * ntb;
    } else {                        // row I of the upper triangle holds the ntb - I tiles (I, I) .. (I, ntb - 1)
        int64_t rest = t;
        I = 0;
        while (rest >= ntb - I) {
            rest -= ntb - I;
            ++I;
        }
        J = I + rest;
    }

    // D phase: thread (ti, tj) owns rows ti + 16 a, columns tj + 16 b.  T phase: wave w owns b = 16 w .. 16 w + 15, lane
    // (ta, tr) rows ta + 16 i and replicates tr + 4 j of the block
    const int ti = tid >> 4, tj = tid & 15;
    const int w = tid >> 6, ta = tid & 15, tr = (tid >> 4) & 3;

    double acc[NRB][4];
#pragma unroll
    for (int rb = 0; rb < NRB; ++rb)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[rb][j] = 0.0;

    for (; t < t_end; ++t) {
        const int64_t I0 = I * TILE, J0 = J * TILE;
        const double wgt = (q != 2 && I != J) ? 2.0 : 1.0;

        // the counts of replicate block rb as this thread stages them: element e = tid + 256 s is (side, replicate, row)
        int32_t pre[8];
        auto fetch = [&](int rb) {
#pragma unroll
            for (int s = 0; s < 8; ++s) {
                const int e = tid + NT * s;
                const int side = e >> 10, r = (e >> 6) & (RB - 1), row = e & (TILE - 1);
                const int64_t g = (side ? J0 : I0) + row, rep = rep0 + rb * RB + r;
                const bool in = g < (side ? nb : na) && rep < reps;
                pre[s] = in ? cnt[rep * N + (side ? offb : offa) + g] : 0;
            }
        };
        fetch(0);

        // ---- the tile's distances, once ----
        double dd[4][4];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) dd[a][b] = 0.0;
        for (int64_t k0 = 0; k0 < d; k0 += DC) {
            const int dc = (int)((d - k0) < DC ? (d - k0) : DC);
            __syncthreads();                       // the previous chunk's (or tile's) reads are done
            stage(XA, na, d, I0, k0, dc, sh.u.st.A);
            stage(XB, nb, d, J0, k0, dc, sh.u.st.B);
            __syncthreads();
            for (int k = 0; k < dc; ++k) {
                double xa[4], yb[4];
#pragma unroll
                for (int a = 0; a < 4; ++a) xa[a] = sh.u.st.A[k][ti + 16 * a];
#pragma unroll
                for (int b = 0; b < 4; ++b) yb[b] = sh.u.st.B[k][tj + 16 * b];
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int b = 0; b < 4; ++b) {
                        const double df = xa[a] - yb[b];
                        dd[a][b] = fma(df, df, dd[a][b]);
                    }
            }
        }
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) sh.D[ti + 16 * a][tj + 16 * b] = sqrt(dd[a][b]);

        // ---- T = D C per block of replicates, folded into the accumulators ----
#pragma unroll
        for (int rb = 0; rb < NRB; ++rb) {
            if (rb < nrb) {                        // (uniform over the workgroup)
                __syncthreads();                   // D is written; the staged chunks / the previous count tiles are read
#pragma unroll
                for (int s = 0; s < 8; ++s) {
                    const int e = tid + NT * s;
                    sh.u.C[e >> 10][e & (TILE - 1)][(e >> 6) & (RB - 1)] = (double)pre[s];
                }
                __syncthreads();
                if (rb + 1 < nrb) fetch(rb + 1);   // in flight under the fmas below

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
                    for (int i = 0; i < 4; ++i) dv[i] = sh.D[ta + 16 * i][b];
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

        if (++J == ntb) {
            ++I;
            J = q == 2 ? 0 : I;
        }
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
    __syncthreads();
    if (tid < nrep) {
        double s = sh.u.red[0][tid];
#pragma unroll
        for (int v = 1; v < NT / 64; ++v) s = s + sh.u.red[v][tid];
        partial[wg * reps + rep0 + tid] = s;
    }
}

__global__ void __launch_bounds__(NT) k_energy_finish(const double *__restrict__ partial, int64_t reps, Plan p,
                                                      double *__restrict__ sums) {
    const int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x;      // q-major, so that a wave reads neighbouring replicates
    if (e >= 3 * reps) return;
    const int64_t q = e / reps, r = e - q * reps;
    double s = 0.0;
#pragma unroll 8
    for (int64_t wg = p.first[q]; wg < p.first[q + 1]; ++wg) s = s + partial[wg * reps + r];
    sums[r * 3 + q] = s;
}

bool energy_args_ok(int64_t nr, int64_t nf, int64_t d, int64_t reps) {
    if (nr < 1 || nf < 1 || d < 1 || reps < 1 || reps > 65535) return false;
    if (nr > (int64_t)INT32_MAX || nf > (int64_t)INT32_MAX) return false;        // int32 indices
    const int64_t big = nr > nf ? nr : nf;
    if (d > INT64_MAX / big / (int64_t)sizeof(double)) return false;            // a row's byte offset overflows
    return true;
}

}  // namespace

// ---- C ABI --------------------------------------------------------------------------------------------

extern "C" size_t pfm_energy_workspace_bytes(int64_t nr, int64_t nf, int64_t d, int64_t reps) {
    if (!energy_args_ok(nr, nf, d, reps)) return 0;
    const Plan p = plan_of(nr, nf);
    return align256(sizeof(int32_t) * (size_t)reps * (size_t)(nr + nf)) +
           align256(sizeof(double) * (size_t)reps * (size_t)p.first[3]);
}

extern "C" int pfm_energy(void *stream, const double *Xr, int64_t nr, const double *Xf, int64_t nf, int64_t d,
                          const int32_t *idx_r, const int32_t *idx_f, int64_t reps, double *sums, void *workspace,
                          size_t workspace_bytes) {
    if (!Xr || !Xf || !idx_r || !idx_f || !sums || !energy_args_ok(nr, nf, d, reps)) return PFM_EINVAL;
    const size_t need = pfm_energy_workspace_bytes(nr, nf, d, reps);
    if (!workspace || workspace_bytes < need) return PFM_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const Plan p = plan_of(nr, nf);
    const int64_t N = nr + nf;
    const size_t cbytes = sizeof(int32_t) * (size_t)reps * (size_t)N;
    int32_t *cnt = (int32_t *)workspace;
    double *partial = (double *)((char *)workspace + align256(cbytes));

    PFM_TRY(hipMemsetAsync(cnt, 0, cbytes, st));
    int64_t cb = (N + NT - 1) / NT;
    if (cb > 1024) cb = 1024;
    hipLaunchKernelGGL(k_counts, dim3((unsigned)cb, (unsigned)reps), dim3(NT), 0, st, idx_r, idx_f, nr, nf, cnt);
    PFM_TRY(hipGetLastError());
    const dim3 grid((unsigned)p.first[3], (unsigned)((reps + SUPER - 1) / SUPER));
    hipLaunchKernelGGL(k_energy_tiles, grid, dim3(NT), 0, st, Xr, nr, Xf, nf, d, (const int32_t *)cnt, reps, p, partial);
    PFM_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_energy_finish, dim3((unsigned)((3 * reps + NT - 1) / NT)), dim3(NT), 0, st,
                       (const double *)partial, reps, p, sums);
    PFM_TRY(hipGetLastError());
    return PFM_OK;
}
