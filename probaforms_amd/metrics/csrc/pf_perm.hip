// pf_perm.hip -- the permutation two-sample tests' two halves, for gfx950 (C ABI: pf_metrics.h, pfm_perm_labels and
// pfm_perm_form).
//
// A relabelling of the pooled sample z_0 .. z_{n-1} (n_first "first" rows, n - n_first "second" rows) is a byte per row, and
// the statistic of a relabelling is the signed quadratic form S = sum_ab s[a] s[b] G(a, b) with s = +n_second on a row
// labelled 1 and -n_first otherwise: G does not depend on the labelling, so every G(a, b) is formed ONCE per group of
// labellings and what is left per labelling and pair is one float64 multiply-add: the scaffold of pf_quadform.h, which
// pf_energy.hip shares.
//   k_perm_labels    one workgroup per labelling p.  Row a's sort key is 64 bits of Philox4x32-10 at counter (a, 0, p, 0),
//                    and the n_first rows of smallest (key, a) get label 1.  The n_first-th smallest key is found by an
//                    MSB-first radix select: 8 passes, each a 256-bin histogram in LDS (integer LDS atomics) of the next
//                    byte of the keys that match the bytes chosen so far.  The keys are recomputed in every pass: nothing of
//                    the size reps x n x 8 is stored.  A last pass in index order writes every label: 1 below the
//                    threshold key; the rows equal to it take the places that are left in index order, with a running count
//                    carried from chunk to chunk (a ballot inside a wave, the waves in index order).
//   k_perm_tiles     k_energy_tiles' decomposition over the ONE pooled block: a workgroup walks a list of 64 x 64 tiles of
//                    the upper triangle (an off-diagonal tile weighs 2), forms the tile's G once -- tile_d2 of
//                    pf_pairtile.h, then sqrt (energy) or exp(-(gamma d^2)) (Gauss) -- and keeps it in LDS.  A wave owns 16
//                    rows a of the tile and holds their G[a, 0..63] in registers.  Per block of 16 labellings the workgroup
//                    stages the two label tiles as float64 weights (a row past the end weighs 0) and the wave forms
//                    T[a, r] = sum_b G[a, b] s[b, r] with 16 v_mfma_f64_16x16x4_f64 in one chain (it measured 1.36 times as
//                    fast as the 4 x 4 register micro-tiles of VALU fmas that k_energy_tiles uses), then folds T with
//                    w s[a, r] into the lane's accumulator of that block, which lives in a register across all the
//                    workgroup's tiles.
//   k_quad_finish<1> S[r] = the workgroups' partials in index order.
// The lists of tiles and their order depend on n only, the chunks of features on d, and a labelling's place in the call
// decides which lanes hold it, never in which order its terms are added: a labelling's S is bitwise the same alone, in any
// group, in any call.  No float atomics.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "../../csrc/rnvp_prior.h"   // philox4x32_10, the one statement of it (pf_predict.hip draws through the same header)
#include "pf_metrics.h"
#include "pf_quadform.h"

namespace {

// ---- the labellings --------------------------------------------------------------------------------------

__device__ __forceinline__ uint64_t sort_key(uint64_t seed, uint64_t key_mask, uint32_t p, int64_t a) {
    uint32_t c[4] = {(uint32_t)a, 0u, p, 0u};
    rnvp::philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
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

struct Labels {                     // the weights of a labelling: s = +n_second on a row labelled 1, -n_first otherwise
    typedef int32_t raw_t;          // 0 = no row (past the end of the sample or of the call), 1 = label 1, 2 = label 0
    const uint8_t *labels;          // [reps, n]
    int64_t n;
    double w_one, w_zero;           // exact integers
    __device__ int64_t rows(int) const { return n; }
    __device__ raw_t load(int, int64_t g, int64_t rep) const { return labels[rep * n + g] ? 1 : 2; }
    __device__ double weight(raw_t v) const {
        const double one = w_one, zero = w_zero;   // read before the selection, so that it stays two selects
        return v == 1 ? one : (v == 2 ? zero : 0.0);
    }
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
    const Plain pooled = {Z, n, d};
    const Labels S = {labels, n, (double)(n - n_first), -(double)n_first};

    int64_t t = wg * p.list;
    int64_t t_end = t + p.list;
    if (t_end > p.nt[0]) t_end = p.nt[0];
    TileWalk at;
    at.start(t, p.ta, true);

    // G phase: thread (ti, tj) owns rows ti + 16 a, columns tj + 16 b.  T phase: wave w owns a = 16 w .. 16 w + 15; lane
    // (ln, lk) holds labelling ln of the block and the rows lk + 4 i
    const int ti = tid >> 4, tj = tid & 15;
    const int w = tid >> 6, ln = tid & 15, lk = (tid >> 4) & 3;

    double acc[NRB];                               // one per block of labellings, across all the workgroup's tiles
#pragma unroll
    for (int rb = 0; rb < NRB; ++rb) acc[rb] = 0.0;

    for (; t < t_end; ++t) {
        const int64_t I0 = at.I * TILE, J0 = at.J * TILE;
        const double wgt = at.I != at.J ? 2.0 : 1.0;

        WeightTiles<Labels> wt = {S, tid, I0, J0, rep0, reps};
        wt.fetch(0);

        // ---- the tile's pair values, once ----
        double dd[4][4];
        tile_d2(pooled, I0, pooled, J0, false, sh.u.st.A, sh.u.st.B, dd);
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
                wt.store(sh.u.C);
                __syncthreads();
                if (rb + 1 < nrb) wt.fetch(rb + 1);   // in flight under the MFMAs below

                v4d T = {0.0, 0.0, 0.0, 0.0};      // one chain: two and four independent ones were no faster
#pragma unroll
                for (int kk = 0; kk < TILE / 4; ++kk)
                    T = __builtin_amdgcn_mfma_f64_16x16x4f64(gv[kk], sh.u.C[1][4 * kk + lk][ln], T, 0, 0, 0);
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[rb] = fma(wgt * sh.u.C[0][16 * w + lk + 4 * i][ln], T[i], acc[rb]);
            }
        }

        at.advance(p.ta, true);
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
    waves_to_partial(sh.u.red, nrep, partial + wg * reps + rep0);
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
    return align256(sizeof(double) * (size_t)reps * (size_t)plan_of(n, 0).first[1]);
}

extern "C" int pfm_perm_form(void *stream, int kind, double gamma, const double *Z, int64_t n, int64_t d, int64_t n_first,
                             const uint8_t *labels, int64_t reps, double *S, void *workspace, size_t workspace_bytes) {
    if (!Z || !labels || !S || !form_args_ok(n, d, n_first, reps)) return PFM_EINVAL;
    if (kind != PFM_PERM_ENERGY && kind != PFM_PERM_GAUSS) return PFM_EUNSUPPORTED;
    if (kind == PFM_PERM_GAUSS && !(gamma > 0.0 && gamma <= 1.79769313486231570815e308)) return PFM_EINVAL;
    if (!workspace || workspace_bytes < pfm_perm_form_workspace_bytes(n, d, n_first, reps)) return PFM_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const Plan p = plan_of(n, 0);                  // one pooled block
    double *partial = (double *)workspace;
    const dim3 grid((unsigned)p.first[1], (unsigned)((reps + SUPER - 1) / SUPER));
    hipLaunchKernelGGL(k_perm_tiles, grid, dim3(NT), 0, st, kind, gamma, Z, n, d, n_first, labels, reps, p, partial);
    PFM_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_quad_finish<1>, dim3((unsigned)((reps + NT - 1) / NT)), dim3(NT), 0, st, (const double *)partial,
                       reps, p, S);
    PFM_TRY(hipGetLastError());
    return PFM_OK;
}
