// pf_perm.hip -- the permutation two-sample tests' two halves, for gfx950 (C ABI: pf_metrics.h, pfm_perm_labels and
// pfm_perm_form).
//
// A relabelling of the pooled sample z_0 .. z_{n-1} (n_first "first" rows, n - n_first "second" rows) is a byte per row, and
// the statistic of a relabelling is the signed quadratic form S = sum_ab s[a] s[b] G(a, b) with s = +n_second on a row
// labelled 1 and -n_first otherwise: G does not depend on the labelling, so every G(a, b) is formed ONCE per group of
// labellings and what is left per labelling and pair is one float64 multiply-add, as in pf_energy.hip.
//   k_perm_labels    one workgroup per labelling p.  Row a's sort key is 64 bits of Philox4x32-10 at counter (a, 0, p, 0),
//                    and the n_first rows of smallest (key, a) get label 1.  The n_first-th smallest key is found by an
//                    MSB-first radix select: 8 passes, each a 256-bin histogram in LDS (integer LDS atomics) of the next
//                    byte of the keys that match the bytes chosen so far.  The keys are recomputed in every pass: nothing of
//                    the size reps x n x 8 is stored.  A last pass in index order writes every label: 1 below the
//                    threshold key; the rows equal to it take the places that are left in index order, with a running count
//                    carried from chunk to chunk (a ballot inside a wave, the waves in index order).
//   k_perm_tiles     k_energy_tiles' decomposition over the ONE pooled block: a workgroup walks a list of 64 x 64 tiles of
//                    the upper triangle (an off-diagonal tile weighs 2), forms the tile's G once -- fma(df, df, acc) over the
//                    features in order, then sqrt (energy) or exp(-(gamma d^2)) (Gauss) -- and keeps it in LDS.  A wave owns 16
//                    rows a of the tile and holds their G[a, 0..63] in registers.  Per block of 16 labellings the workgroup
//                    stages the two label tiles as float64 weights (a row past the end weighs 0) and the wave forms
//                    T[a, r] = sum_b G[a, b] s[b, r] with 16 v_mfma_f64_16x16x4_f64 in one chain (it measured 1.36 times as
//                    fast as the 4 x 4 register micro-tiles of VALU fmas that k_energy_tiles uses), then folds T with
//                    w s[a, r] into the lane's accumulator of that block, which lives in a register across all the
//                    workgroup's tiles.
//   k_perm_finish    S[r] = the workgroups' partials in index order.
// The lists of tiles and their order depend on n only, the chunks of features on d, and a labelling's place in the call
// decides which lanes hold it, never in which order its terms are added: a labelling's S is bitwise the same alone, in any
// group, in any call.  No float atomics.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "pf_metrics.h"

#define PFM_TRY(x)                                              \
    do {                                                        \
        hipError_t e_ = (x);                                    \
        if (e_ != hipSuccess) return (int)e_;                   \
    } while (0)

namespace {

constexpr int NT = 256;                    // threads per workgroup, every kernel
constexpr int TILE = PFM_ENERGY_TILE;      // rows per side of a pair tile
constexpr int TPAD = TILE + 1;             // odd LDS stride of a staged feature and of a row of G
constexpr int DC = 16;                     // features staged per chunk
constexpr int RB = PFM_ENERGY_REP_BLOCK;   // labellings per weight tile
constexpr int RBP = RB + 1;                // LDS stride of a weight-tile row
constexpr int SUPER = 128;                 // labellings per workgroup (grid.y): SUPER / RB accumulators in registers
constexpr int NRB = SUPER / RB;
constexpr int64_t MIN_LIST = 4;            // tiles per workgroup, at least
constexpr int64_t TARGET_WGS = 2048;       // workgroups per call, about (beyond it the lists grow instead)
static_assert(TILE == 64 && RB == 16 && NT == 256, "the lane layout below is written for 64 x 64 tiles and 16 labellings");

inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// ---- the labellings --------------------------------------------------------------------------------------

// Philox4x32-10 (Salmon et al. 2011), as probaforms_amd/csrc/rnvp_prior.h states it
__device__ __forceinline__ void philox4x32_10(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c[0]), lo0 = 0xD2511F53u * c[0];
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c[2]), lo1 = 0xCD9E8D57u * c[2];
        const uint32_t n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
        c[0] = n0; c[1] = lo1; c[2] = n2; c[3] = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
}

__device__ __forceinline__ uint64_t sort_key(uint64_t seed, uint64_t key_mask, uint32_t p, int64_t a) {
    uint32_t c[4] = {(uint32_t)a, 0u, p, 0u};
    philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    return ((uint64_t)c[0] | (uint64_t)c[1] << 32) & key_mask;
}

__global__ void __launch_bounds__(NT) k_perm_labels(uint64_t seed, uint64_t key_mask, int64_t first_perm, int64_t n,
                                                    int64_t n_first, uint8_t *labels) {
    __shared__ uint32_t hist[256];
    __shared__ uint32_t wave_eq[NT / 64];
    __shared__ int s_bin;
    __shared__ int64_t s_rank;
    const int tid = threadIdx.x;
    const uint32_t p = (uint32_t)(first_perm + blockIdx.x);
    uint8_t *out = labels + (int64_t)blockIdx.x * n;

    // ---- the key of rank n_first - 1 (0-based) among the n keys, byte by byte from the top ----
    uint64_t prefix = 0;
    int64_t rank = n_first - 1;                    // its rank among the keys that match `prefix` so far
    for (int pass = 0; pass < 8; ++pass) {
        const int shift = 56 - 8 * pass;
        const uint64_t chosen = pass == 0 ? 0 : ~(uint64_t)0 << (shift + 8);      // the bytes chosen so far
        hist[tid] = 0;
        __syncthreads();
        for (int64_t a = tid; a < n; a += NT) {
            const uint64_t key = sort_key(seed, key_mask, p, a);
            if ((key & chosen) == prefix) atomicAdd(&hist[(key >> shift) & 255], 1u);
        }
        __syncthreads();
        if (tid == 0) {
            int64_t cum = 0;
            int b = 0;
            for (; b < 255; ++b) {                 // (the rank lies inside the matching keys, so bin 255 needs no test)
                const int64_t c = hist[b];
                if (rank < cum + c) break;
                cum += c;
            }
            s_bin = b;
            s_rank = rank - cum;
        }
        __syncthreads();
        prefix |= (uint64_t)s_bin << shift;
        rank = s_rank;
        __syncthreads();                           // s_bin / s_rank are read before the next pass writes them
    }
    const uint64_t thr = prefix;
    const int64_t take = rank + 1;                 // rows with key == thr that get label 1, in index order

    // ---- every label, in index order ----
    const int lane = tid & 63, w = tid >> 6;
    int64_t taken = 0;                             // rows with key == thr before this chunk (uniform)
    for (int64_t base = 0; base < n; base += NT) {
        const int64_t a = base + tid;
        const bool in = a < n;
        const uint64_t key = in ? sort_key(seed, key_mask, p, a) : 0;
        const bool eq = in && key == thr;
        const uint64_t bal = __ballot(eq);
        if (lane == 0) wave_eq[w] = (uint32_t)__popcll(bal);
        __syncthreads();
        int64_t before = taken + __popcll(bal & (((uint64_t)1 << lane) - 1));
        int64_t total = 0;
#pragma unroll
        for (int v = 0; v < NT / 64; ++v) {
            if (v < w) before += wave_eq[v];
            total += wave_eq[v];
        }
        if (in) out[a] = (uint8_t)((key < thr || (eq && before < take)) ? 1 : 0);
        taken += total;
        __syncthreads();                           // wave_eq is read before the next chunk writes it
    }
}

// ---- the quadratic forms ---------------------------------------------------------------------------------

__host__ __device__ inline int64_t tiles_of(int64_t n) { return (n + TILE - 1) / TILE; }

struct Plan {                       // the decomposition: a function of n only
    int64_t tn;                     // tiles per side
    int64_t nt;                     // tiles of the upper triangle
    int64_t list;                   // tiles per workgroup (the last workgroup may have fewer)
    int64_t wgs;                    // workgroups
};

__host__ inline Plan plan_of(int64_t n) {
    Plan p;
    p.tn = tiles_of(n);
    p.nt = p.tn * (p.tn + 1) / 2;
    p.list = (p.nt + TARGET_WGS - 1) / TARGET_WGS;
    if (p.list < MIN_LIST) p.list = MIN_LIST;
    p.wgs = (p.nt + p.list - 1) / p.list;
    return p;
}

// features k0 .. k0 + dc - 1 of rows r0 .. r0 + 63 of Z [n, d] into sm[feature][row]; rows past the end are zeros
__device__ inline void stage(const double *Z, int64_t n, int64_t d, int64_t r0, int64_t k0, int dc, double (*sm)[TPAD]) {
    for (int e = threadIdx.x; e < TILE * dc; e += NT) {
        const int row = e / dc, col = e - row * dc;
        const int64_t g = r0 + row;
        sm[col][row] = g < n ? Z[g * d + k0 + col] : 0.0;
    }
}

struct Shared {
    double G[TILE][TPAD];                          // the tile's pair values
    union {
        struct { double A[DC][TPAD], B[DC][TPAD]; } st;   // staged feature chunks (while G is formed)
        double C[2][TILE][RBP];                    // weight tiles of the a rows and the b rows (while T is formed)
        double red[NT / 64][SUPER];                // the waves' sums per labelling (after the last tile)
    } u;
};

typedef double v4d __attribute__((ext_vector_type(4)));

// T = G s on v_mfma_f64_16x16x4_f64.  Wave w owns the a rows 16 w .. 16 w + 15 and all 64 b; lane (ln, lk) feeds
// A[m = ln][k = lk] = G[16 w + ln][4 kk + lk] (held in registers for the whole tile) and B[k = lk][n = ln] = s[4 kk + lk][ln]
// and gets T[m = lk + 4 i][n = ln] in result i.
__global__ void __launch_bounds__(NT) k_perm_tiles(int kind, double gamma, const double *Z, int64_t n, int64_t d,
                                                   int64_t n_first, const uint8_t *labels, int64_t reps, Plan p,
                                                   double *partial) {
    __shared__ Shared sh;
    const int tid = threadIdx.x;
    const int64_t wg = blockIdx.x;
    const int64_t rep0 = (int64_t)blockIdx.y * SUPER;
    const int64_t left = reps - rep0;
    const int nrep = (int)(left < SUPER ? left : SUPER);          // labellings of this workgroup
    const int nrb = (nrep + RB - 1) / RB;
    const double w_one = (double)(n - n_first), w_zero = -(double)n_first;       // s of label 1 / label 0: exact integers

    int64_t t = wg * p.list;
    int64_t t_end = t + p.list;
    if (t_end > p.nt) t_end = p.nt;
    int64_t I = 0, J;
    {
        int64_t rest = t;
        while (rest >= p.tn - I) {
            rest -= p.tn - I;
            ++I;
        }
        J = I + rest;
    }

    // G phase: thread (ti, tj) owns rows ti + 16 a, columns tj + 16 b.  T phase: wave w owns a = 16 w .. 16 w + 15; lane
    // (ln, lk) holds labelling ln of the block and the rows lk + 4 i
    const int ti = tid >> 4, tj = tid & 15;
    const int w = tid >> 6, ln = tid & 15, lk = (tid >> 4) & 3;

    double acc[NRB];                               // one per block of labellings, across all the workgroup's tiles
#pragma unroll
    for (int rb = 0; rb < NRB; ++rb) acc[rb] = 0.0;

    for (; t < t_end; ++t) {
        const int64_t I0 = I * TILE, J0 = J * TILE;
        const double wgt = I != J ? 2.0 : 1.0;

        // the labels of block rb as this thread stages them: element e = tid + 256 s is (side, labelling, row); 0 = no row
        // (past the end of the sample or of the call), 1 = label 1, 2 = label 0
        uint8_t pre[8];
        auto fetch = [&](int rb) {
#pragma unroll
            for (int s = 0; s < 8; ++s) {
                const int e = tid + NT * s;
                const int side = e >> 10, r = (e >> 6) & (RB - 1), row = e & (TILE - 1);
                const int64_t g = (side ? J0 : I0) + row, rep = rep0 + rb * RB + r;
                const bool in = g < n && rep < reps;
                pre[s] = in ? (labels[rep * n + g] ? 1 : 2) : 0;
            }
        };
        fetch(0);

        // ---- the tile's pair values, once ----
        double dd[4][4];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) dd[a][b] = 0.0;
        for (int64_t k0 = 0; k0 < d; k0 += DC) {
            const int dc = (int)((d - k0) < DC ? (d - k0) : DC);
            __syncthreads();                       // the previous chunk's (or tile's) reads are done
            stage(Z, n, d, I0, k0, dc, sh.u.st.A);
            stage(Z, n, d, J0, k0, dc, sh.u.st.B);
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
        if (kind == PFM_PERM_ENERGY) {
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) sh.G[ti + 16 * a][tj + 16 * b] = sqrt(dd[a][b]);
        } else {
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) sh.G[ti + 16 * a][tj + 16 * b] = exp(-(gamma * dd[a][b]));
        }
        __syncthreads();                           // G is written; the staged chunks are read
        double gv[TILE / 4];                       // the wave's slab of G, for every block of labellings
#pragma unroll
        for (int kk = 0; kk < TILE / 4; ++kk) gv[kk] = sh.G[16 * w + ln][4 * kk + lk];

        // ---- T = G s per block of labellings, folded into the accumulators ----
#pragma unroll
        for (int rb = 0; rb < NRB; ++rb) {
            if (rb < nrb) {                        // (uniform over the workgroup)
                if (rb > 0) __syncthreads();       // the previous weight tiles are read
#pragma unroll
                for (int s = 0; s < 8; ++s) {
                    const int e = tid + NT * s;
                    sh.u.C[e >> 10][e & (TILE - 1)][(e >> 6) & (RB - 1)] = pre[s] == 1 ? w_one : (pre[s] == 2 ? w_zero : 0.0);
                }
                __syncthreads();
                if (rb + 1 < nrb) fetch(rb + 1);   // in flight under the MFMAs below

                v4d T = {0.0, 0.0, 0.0, 0.0};      // one chain: two and four independent ones were no faster
#pragma unroll
                for (int kk = 0; kk < TILE / 4; ++kk)
                    T = __builtin_amdgcn_mfma_f64_16x16x4f64(gv[kk], sh.u.C[1][4 * kk + lk][ln], T, 0, 0, 0);
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[rb] = fma(wgt * sh.u.C[0][16 * w + lk + 4 * i][ln], T[i], acc[rb]);
            }
        }

        if (++J == p.tn) {
            ++I;
            J = I;
        }
    }

    // ---- the 16 lanes of a labelling: xor tree over lk, then the waves in index order ----
#pragma unroll
    for (int rb = 0; rb < NRB; ++rb) {
        double v = acc[rb];
        v = v + __shfl_xor(v, 16, 64);
        v = v + __shfl_xor(v, 32, 64);
        acc[rb] = v;
    }
    __syncthreads();                               // the last tile's weight tiles are read
    if (lk == 0) {
#pragma unroll
        for (int rb = 0; rb < NRB; ++rb) sh.u.red[w][rb * RB + ln] = acc[rb];
    }
    __syncthreads();
    if (tid < nrep) {
        double s = sh.u.red[0][tid];
#pragma unroll
        for (int v = 1; v < NT / 64; ++v) s = s + sh.u.red[v][tid];
        partial[wg * reps + rep0 + tid] = s;
    }
}

__global__ void __launch_bounds__(NT) k_perm_finish(const double *__restrict__ partial, int64_t reps, int64_t wgs,
                                                    double *__restrict__ S) {
    const int64_t r = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (r >= reps) return;
    double s = 0.0;
#pragma unroll 8
    for (int64_t wg = 0; wg < wgs; ++wg) s = s + partial[wg * reps + r];
    S[r] = s;
}

bool labels_args_ok(int64_t first_perm, int64_t reps, int64_t n, int64_t n_first) {
    if (reps < 1 || reps > (int64_t)INT32_MAX || n < 2 || n > (int64_t)INT32_MAX) return false;      // reps is grid.x
    if (n_first < 1 || n_first >= n) return false;
    if (first_perm < 0 || first_perm > ((int64_t)1 << 32) - reps) return false;       // p is a 32-bit counter word
    if (reps > INT64_MAX / n) return false;
    return true;
}

bool form_args_ok(int64_t n, int64_t d, int64_t n_first, int64_t reps) {
    if (n < 2 || n > (int64_t)INT32_MAX || d < 1 || reps < 1 || reps > 65535 * (int64_t)SUPER) return false;
    if (n_first < 1 || n_first >= n) return false;
    if (d > INT64_MAX / n / (int64_t)sizeof(double)) return false;              // a row's byte offset overflows
    return true;
}

}  // namespace

// ---- C ABI --------------------------------------------------------------------------------------------

extern "C" size_t pfm_perm_labels_workspace_bytes(int64_t reps, int64_t n, int64_t n_first) {
    if (!labels_args_ok(0, reps, n, n_first)) return 0;
    return 256;                                    // nothing is kept between launches: the least a caller can allocate
}

extern "C" int pfm_perm_labels(void *stream, uint64_t seed, uint64_t key_mask, int64_t first_perm, int64_t reps, int64_t n,
                               int64_t n_first, uint8_t *labels, void *workspace, size_t workspace_bytes) {
    if (!labels || !labels_args_ok(first_perm, reps, n, n_first)) return PFM_EINVAL;
    if (!workspace || workspace_bytes < pfm_perm_labels_workspace_bytes(reps, n, n_first)) return PFM_EWORKSPACE;
    hipLaunchKernelGGL(k_perm_labels, dim3((unsigned)reps), dim3(NT), 0, (hipStream_t)stream, seed, key_mask, first_perm, n,
                       n_first, labels);
    PFM_TRY(hipGetLastError());
    return PFM_OK;
}

extern "C" size_t pfm_perm_form_workspace_bytes(int64_t n, int64_t d, int64_t n_first, int64_t reps) {
    if (!form_args_ok(n, d, n_first, reps)) return 0;
    return align256(sizeof(double) * (size_t)reps * (size_t)plan_of(n).wgs);
}

extern "C" int pfm_perm_form(void *stream, int kind, double gamma, const double *Z, int64_t n, int64_t d, int64_t n_first,
                             const uint8_t *labels, int64_t reps, double *S, void *workspace, size_t workspace_bytes) {
    if (!Z || !labels || !S || !form_args_ok(n, d, n_first, reps)) return PFM_EINVAL;
    if (kind != PFM_PERM_ENERGY && kind != PFM_PERM_GAUSS) return PFM_EUNSUPPORTED;
    if (kind == PFM_PERM_GAUSS && !(gamma > 0.0 && gamma <= 1.79769313486231570815e308)) return PFM_EINVAL;
    if (!workspace || workspace_bytes < pfm_perm_form_workspace_bytes(n, d, n_first, reps)) return PFM_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const Plan p = plan_of(n);
    double *partial = (double *)workspace;
    const dim3 grid((unsigned)p.wgs, (unsigned)((reps + SUPER - 1) / SUPER));
    hipLaunchKernelGGL(k_perm_tiles, grid, dim3(NT), 0, st, kind, gamma, Z, n, d, n_first, labels, reps, p, partial);
    PFM_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_perm_finish, dim3((unsigned)((reps + NT - 1) / NT)), dim3(NT), 0, st, (const double *)partial, reps,
                       p.wgs, S);
    PFM_TRY(hipGetLastError());
    return PFM_OK;
}
