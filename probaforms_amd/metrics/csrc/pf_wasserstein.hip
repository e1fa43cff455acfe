// pf_wasserstein.hip -- the 1-D Wasserstein distance W_p^p (p = 1, 2) of every bootstrap replicate's columns, and the
// projection that turns a multivariate sample into such columns (sliced Wasserstein), for gfx950
// (C ABI: pf_metrics.h, pfm_project / pfm_wasserstein1d).
//
// As in pf_metrics1d.hip the caller sorts each POOLED ORIGINAL column once per call; a replicate's two resampled columns
// are that order with every original row repeated by its draw count (k_counts), so no replicate is sorted or gathered.
// One workgroup per (column, replicate).  With the tie groups g in value order, A_g / B_g the real / fake draw counts
// and CR_g / CF_g their running sums after group g:
//   k_w1       W_1 = sum_g |CR_g / nr - CF_g / nf| (v_{g+1} - v_g) over all groups but the last (scipy's
//              wasserstein_distance; empty groups leave the cdfs unchanged and their gaps still count), on the chunked
//              integer scan of k_scan1d.  The cdf difference is the exact integer |CR_g nf - CF_g nr| over nr nf.
//   k_wp<P>    W_p^p = int_0^1 |Q_r(u) - Q_f(u)|^p du on the integer grid of nr nf cells: a non-empty real group covers
//              [CR_before nf, CR nf), a non-empty fake group [CF_before nr, CF nr), and every overlap of a real with a
//              fake group adds overlap |v_g - v_h|^p / (nr nf).  Two steps:
//              1. the same scan compacts each sample's non-empty groups into a table of (value, inclusive cumulative
//                 count): the real sample's from the front of the table, the fake sample's from its back;
//              2. the two tables' breakpoints CR nf and CF nr are two ascending lists whose merge has Mr + Mf steps;
//                 thread t takes steps [t S, (t + 1) S): a binary search (merge path) finds how many real breakpoints
//                 lie before step t S, then a walk of S steps adds the segments' terms.  The walk moves through the
//                 compacted tables only, so it costs the same wherever the samples lie relative to each other
//                 (disjoint supports, long runs of groups one sample never drew).
//              The table lives in LDS while min(G, nr) + min(G, nf) <= WP_LDS entries.  Beyond that it is written to
//              the workspace and merged in tiles of WP_LDS / 2 steps: a tile's entries of either list are staged in
//              LDS with coalesced loads, so the threads' searches and walks never wait on global memory.
// Float sums run per thread in group / segment order and then through the fixed LDS tree of block_sum; there are no
// float atomics and every table entry read was written by the same launch, so a call is bitwise reproducible whatever
// the workspace held.  -ffp-contract=off (Makefile): k_project's multiply and add are rounded separately, as numpy's.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "pf_metrics.h"
#include "pf_scan1d.h"

namespace {

constexpr int WP_LDS = 2048;     // table entries (both samples) held in LDS: 12 bytes each

__global__ void __launch_bounds__(NT) k_project(const double *Xr, const double *Xf, int64_t nr, int64_t nf, int64_t d,
                                                const double *theta, int64_t P, double *cols) {
    const int64_t N = nr + nf, total = P * N;
    for (int64_t t = (int64_t)blockIdx.x * NT + threadIdx.x; t < total; t += (int64_t)gridDim.x * NT) {
        const int64_t k = t / N, i = t - k * N;
        const double *x = i < nr ? Xr + i * d : Xf + (i - nr) * d;
        const double *th = theta + k * d;
        double acc = 0.0;
        for (int64_t j = 0; j < d; ++j) {
            const double prod = x[j] * th[j];
            acc = acc + prod;
        }
        cols[t] = acc;
    }
}

__device__ inline Feature feature_of(const double *cols, const int32_t *perm, const int32_t *gstart,
                                     const int32_t *ngroups, const int32_t *cnt, int64_t nr, int64_t nf) {
    const int64_t f = blockIdx.x, rep = blockIdx.y, N = nr + nf;
    Feature z;
    z.col = cols + f * N;
    z.perm = perm + f * N;
    z.gs = gstart + f * (N + 1);
    z.cnt = cnt + rep * N;
    z.nr = nr;
    z.N = N;
    z.G = ngroups[f];
    return z;
}

__global__ void __launch_bounds__(NT) k_w1(const double *cols, const int32_t *perm, const int32_t *gstart,
                                           const int32_t *ngroups, const int32_t *cnt, int64_t nr, int64_t nf,
                                           int64_t d, double *out) {
    __shared__ int64_t sa[NT], sb[NT];
    __shared__ double sd[NT];
    const int tid = threadIdx.x;
    const Feature z = feature_of(cols, perm, gstart, ngroups, cnt, nr, nf);
    double acc = 0.0;
    int64_t carryR = 0, carryF = 0;
    for (int base = 0; base < z.G; base += NT * IPT) {
        int64_t ar[IPT], af[IPT], tr = 0, tf = 0;
#pragma unroll
        for (int i = 0; i < IPT; ++i) {
            const int g = base + tid * IPT + i;
            int64_t l = 0;
            ar[i] = 0;
            if (g < z.G) z.counts(g, l, ar[i]);
            af[i] = l - ar[i];
            tr += ar[i];
            tf += af[i];
        }
        int64_t Cr, Cf, TR, TF;
        block_scan2(tr, tf, Cr, Cf, TR, TF, sa, sb);
        Cr += carryR;
        Cf += carryF;
        carryR += TR;
        carryF += TF;
#pragma unroll
        for (int i = 0; i < IPT; ++i) {
            const int g = base + tid * IPT + i;
            Cr += ar[i];
            Cf += af[i];
            if (g < z.G - 1) {
                const int64_t num = Cr * nf - Cf * nr;           // (CR / nr - CF / nf) nr nf, |.| <= nr nf < 2^62
                if (num != 0) acc = acc + (double)(num < 0 ? -num : num) * (z.value(g + 1) - z.value(g));
            }
        }
    }
    const double s = block_sum(acc, sd);
    if (tid == 0) out[(int64_t)blockIdx.y * d + blockIdx.x] = s / ((double)nr * (double)nf);
}

template <int P>
__device__ inline double pow_abs(double a) {
    a = fabs(a);
    return P == 1 ? a : a * a;
}

// Steps [k0, k1) of the merge of the breakpoints A_i = tc[i] nf (i < Mr) and B_j = tc[b0 + BS j] nr (j < Mf), A first on a tie.
// Step k, with i real and j fake breakpoints before it (i + j = k), is the segment [previous breakpoint, min(A_i, B_j)) of real
// entry i and fake entry j; prevA / prevB are the breakpoints before entry 0 of either list.  A binary search (merge path) finds
// i at k0, then the steps are walked.  Returns the sum of the segments' terms in step order, and (i, j) after step k1 - 1.
template <int P, int BS>
__device__ double merge_steps(const int32_t *tc, const double *tv, int64_t b0, int64_t Mr, int64_t Mf, int64_t nr,
                              int64_t nf, int64_t prevA, int64_t prevB, int64_t k0, int64_t k1, int64_t &i, int64_t &j) {
    // the smallest i with A_i > B_{k0 - i - 1}
    int64_t lo = k0 > Mf ? k0 - Mf : 0, hi = k0 < Mr ? k0 : Mr;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((int64_t)tc[mid] * nf <= (int64_t)tc[b0 + BS * (k0 - mid - 1)] * nr) lo = mid + 1;
        else hi = mid;
    }
    i = lo;
    j = k0 - lo;
    if (i > 0) prevA = (int64_t)tc[i - 1] * nf;
    if (j > 0) prevB = (int64_t)tc[b0 + BS * (j - 1)] * nr;
    int64_t prev = prevA > prevB ? prevA : prevB;
    double acc = 0.0;
    for (int64_t k = k0; k < k1; ++k) {
        if (i < Mr && j < Mf) {
            const int64_t a = (int64_t)tc[i] * nf, b = (int64_t)tc[b0 + BS * j] * nr;
            const int64_t end = a <= b ? a : b;
            if (end > prev) acc = acc + (double)(end - prev) * pow_abs<P>(tv[i] - tv[b0 + BS * j]);
            prev = end;
            if (a <= b) ++i;
            else ++j;
        } else if (i < Mr) {     // both lists end at nr nf: what is left after one ran out are empty segments
            ++i;
        } else {
            ++j;
        }
    }
    return acc;
}

template <int P>
__global__ void __launch_bounds__(NT) k_wp(const double *cols, const int32_t *perm, const int32_t *gstart,
                                           const int32_t *ngroups, const int32_t *cnt, int64_t nr, int64_t nf,
                                           int64_t d, double *ws_val, int32_t *ws_cum, double *out) {
    __shared__ int64_t sa[NT], sb[NT];
    __shared__ double sd[NT];
    __shared__ double lval[WP_LDS];
    __shared__ int32_t lcum[WP_LDS];
    __shared__ int64_t next[4];
    const int tid = threadIdx.x;
    const Feature z = feature_of(cols, perm, gstart, ngroups, cnt, nr, nf);
    const int64_t N = nr + nf, rf = (int64_t)blockIdx.y * d + blockIdx.x;

    // the table: real entry i at [i], fake entry j at [cap - 1 - j]; Mr + Mf <= min(G, nr) + min(G, nf) <= cap
    const int64_t bound = (z.G < nr ? z.G : nr) + (z.G < nf ? z.G : nf);
    const bool in_lds = bound <= WP_LDS;
    double *const tv = in_lds ? lval : ws_val + rf * N;
    int32_t *const tc = in_lds ? lcum : ws_cum + rf * N;
    const int64_t cap = in_lds ? WP_LDS : N;

    // 1. compact the non-empty groups of each sample.  One scan carries a sample's draw count in the low and its
    //    number of non-empty groups in the high 32 bits (both < 2^31: no carry between the halves)
    int64_t carryR = 0, carryF = 0;
    for (int base = 0; base < z.G; base += NT * IPT) {
        int64_t ar[IPT], af[IPT], tr = 0, tf = 0;
#pragma unroll
        for (int i = 0; i < IPT; ++i) {
            const int g = base + tid * IPT + i;
            int64_t l = 0;
            ar[i] = 0;
            if (g < z.G) z.counts(g, l, ar[i]);
            af[i] = l - ar[i];
            tr += ar[i] + ((int64_t)(ar[i] > 0) << 32);
            tf += af[i] + ((int64_t)(af[i] > 0) << 32);
        }
        int64_t er, ef, TR, TF;
        block_scan2(tr, tf, er, ef, TR, TF, sa, sb);
        er += carryR;
        ef += carryF;
        carryR += TR;
        carryF += TF;
        int64_t Cr = er & 0xffffffff, Cf = ef & 0xffffffff, ir = er >> 32, jf = ef >> 32;
#pragma unroll
        for (int i = 0; i < IPT; ++i) {
            const int g = base + tid * IPT + i;
            if (ar[i] > 0 || af[i] > 0) {
                const double v = z.value(g);
                if (ar[i] > 0) {
                    Cr += ar[i];
                    if (ir < cap) {
                        tv[ir] = v;
                        tc[ir] = (int32_t)Cr;
                    }
                    ++ir;
                }
                if (af[i] > 0) {
                    Cf += af[i];
                    if (jf < cap) {
                        tv[cap - 1 - jf] = v;
                        tc[cap - 1 - jf] = (int32_t)Cf;
                    }
                    ++jf;
                }
            }
        }
    }
    if (tid == 0) next[0] = next[1] = next[2] = next[3] = 0;
    __syncthreads();
    int64_t Mr = carryR >> 32, Mf = carryF >> 32;
    if (Mr + Mf > cap) {         // unreachable for draw counts that sum to nr and nf: keep every index inside the table
        Mr = 0;
        Mf = 0;
    }

    // 2. the Mr + Mf steps of the merge, the same number for every thread
    const int64_t T = Mr + Mf;
    double acc = 0.0;
    int64_t i, j;
    if (in_lds) {                // the whole table is in LDS: thread t takes steps [t S, (t + 1) S)
        const int64_t S = (T + NT - 1) / NT;
        int64_t k0 = (int64_t)tid * S, k1 = k0 + S;
        if (k0 > T) k0 = T;
        if (k1 > T) k1 = T;
        if (k0 < k1) acc = merge_steps<P, -1>(tc, tv, cap - 1, Mr, Mf, nr, nf, 0, 0, k0, k1, i, j);
    } else {
        // the table is in the workspace: tiles of TILE steps.  A tile that starts with ti real and tj fake breakpoints
        // consumed needs at most the next TILE entries of either list; they are staged in LDS (coalesced), and thread t takes
        // steps [t TILE / NT, (t + 1) TILE / NT) of the tile.  Whoever takes the tile's last step hands (i, j) and the two
        // breakpoints before them to the next tile
        constexpr int64_t TILE = WP_LDS / 2, PER = TILE / NT;
        for (int64_t kt = 0; kt < T; kt += TILE) {
            const int64_t ti = next[0], tj = next[1], pA = next[2], pB = next[3];
            const int64_t mr = Mr - ti < TILE ? Mr - ti : TILE, mf = Mf - tj < TILE ? Mf - tj : TILE;
            const int64_t steps = T - kt < TILE ? T - kt : TILE;
            for (int64_t e = tid; e < TILE; e += NT) {
                if (e < mr) {
                    lcum[e] = tc[ti + e];
                    lval[e] = tv[ti + e];
                }
                if (e < mf) {
                    lcum[TILE + e] = tc[cap - 1 - (tj + e)];
                    lval[TILE + e] = tv[cap - 1 - (tj + e)];
                }
            }
            __syncthreads();
            int64_t k0 = (int64_t)tid * PER, k1 = k0 + PER;
            if (k0 > steps) k0 = steps;
            if (k1 > steps) k1 = steps;
            if (k0 < k1) {
                acc = acc + merge_steps<P, 1>(lcum, lval, TILE, mr, mf, nr, nf, pA, pB, k0, k1, i, j);
                if (k1 == steps) {
                    next[0] = ti + i;
                    next[1] = tj + j;
                    next[2] = i > 0 ? (int64_t)lcum[i - 1] * nf : pA;
                    next[3] = j > 0 ? (int64_t)lcum[TILE + j - 1] * nr : pB;
                }
            }
            __syncthreads();
        }
    }
    const double s = block_sum(acc, sd);
    if (tid == 0) out[rf] = s / ((double)nr * (double)nf);
}

bool w1d_sizes_ok(int64_t nr, int64_t nf, int64_t d, int64_t reps) {
    if (nr < 1 || nf < 1 || d < 1 || reps < 1 || reps > 65535) return false;
    if (nr + nf >= (int64_t)INT32_MAX || d > (int64_t)INT32_MAX) return false;
    return true;
}

}  // namespace

extern "C" int pfm_project(void *stream, const double *Xr, int64_t nr, const double *Xf, int64_t nf, int64_t d,
                           const double *theta, int64_t n_proj, double *cols) {
    if (!Xr || !Xf || !theta || !cols) return PFM_EINVAL;
    if (nr < 1 || nf < 1 || d < 1 || n_proj < 1 || nr + nf >= (int64_t)INT32_MAX || d > (int64_t)INT32_MAX ||
        n_proj > (int64_t)INT32_MAX)
        return PFM_EINVAL;
    const int64_t total = n_proj * (nr + nf);
    int64_t blocks = (total + NT - 1) / NT;
    if (blocks > 65536) blocks = 65536;
    hipLaunchKernelGGL(k_project, dim3((unsigned)blocks), dim3(NT), 0, (hipStream_t)stream, Xr, Xf, nr, nf, d, theta,
                       n_proj, cols);
    PFM_TRY(hipGetLastError());
    return PFM_OK;
}

extern "C" size_t pfm_wasserstein1d_workspace_bytes(int64_t nr, int64_t nf, int64_t d, int64_t reps, int p) {
    if (!w1d_sizes_ok(nr, nf, d, reps) || (p != 1 && p != 2)) return 0;
    const int64_t N = nr + nf;
    size_t b = align256(sizeof(int32_t) * reps * N);
    if (p != 1 && N > WP_LDS) b += align256(sizeof(double) * reps * d * N) + align256(sizeof(int32_t) * reps * d * N);
    return b;
}

extern "C" int pfm_wasserstein1d(void *stream, int p, const double *cols, const int32_t *perm, const int32_t *gstart,
                                 const int32_t *ngroups, int64_t nr, int64_t nf, int64_t d, const int32_t *idx_r,
                                 const int32_t *idx_f, int64_t reps, double *out, void *workspace,
                                 size_t workspace_bytes) {
    if (!cols || !perm || !gstart || !ngroups || !idx_r || !idx_f || !out) return PFM_EINVAL;
    if (!w1d_sizes_ok(nr, nf, d, reps)) return PFM_EINVAL;
    if (p != 1 && p != 2) return PFM_EUNSUPPORTED;
    const size_t need = pfm_wasserstein1d_workspace_bytes(nr, nf, d, reps, p);
    if (!workspace || workspace_bytes < need) return PFM_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int64_t N = nr + nf;
    int32_t *cnt = (int32_t *)workspace;
    char *tables = (char *)workspace + align256(sizeof(int32_t) * reps * N);
    double *ws_val = (double *)tables;
    int32_t *ws_cum = (int32_t *)(tables + align256(sizeof(double) * reps * d * N));

    PFM_TRY(launch_counts(st, idx_r, idx_f, nr, nf, reps, cnt));

    const dim3 grid((unsigned)d, (unsigned)reps);
    if (p == 1)
        hipLaunchKernelGGL(k_w1, grid, dim3(NT), 0, st, cols, perm, gstart, ngroups, cnt, nr, nf, d, out);
    else
        hipLaunchKernelGGL(k_wp<2>, grid, dim3(NT), 0, st, cols, perm, gstart, ngroups, cnt, nr, nf, d, ws_val, ws_cum,
                           out);
    PFM_TRY(hipGetLastError());
    return PFM_OK;
}
