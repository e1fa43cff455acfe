// pf_metrics1d.hip -- the per-feature two-sample statistics of probaforms.metrics (ks1d.py, div1d.py) for gfx950
// (C ABI: pf_metrics.h, pfm_metric1d).
//
// Every statistic of a replicate's feature f depends on the resampled values only through their sorted order and
// ties.  The caller sorts each feature's POOLED ORIGINAL column [X_real[:, f]; X_fake[:, f]] once per call and passes
// the permutation and its tie groups (runs of equal values, a CSR of sorted positions).  A bootstrap replicate's
// sorted column is that order with every original row repeated by its draw count, so no replicate is ever sorted
// or gathered:
//   k_counts     per replicate, the int32 draw count of every pooled original row (integer atomics: exact)
//   k_scan1d<M>  one workgroup per (feature, replicate) walks the tie groups in order.  Per group it sums the draw
//                counts of its members into l (pooled rows in the group) and a_r (real rows), a block-wide integer
//                prefix scan gives C (pooled rows before the group) and C_r (real rows before), and these four
//                integers give every rank statistic in closed form (see pf_metrics.h for what each M writes).
//                Empty groups (no draw) are skipped: they are not values of the replicate.
//   k_kde        per (replicate, feature, sample, 8 grid points): the max-shifted log-sum-exp of the Gaussian log
//                kernel over the sample's original rows, each weighted by its draw count, in row order
// Float sums run in a fixed order (per thread in group order, then a fixed LDS tree); there are no float atomics,
// so a call is bitwise reproducible.  -ffp-contract=off (Makefile): every product and sum is rounded as written,
// which the histogram edges and the Anderson-Darling terms rely on to follow numpy's operation order.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "pf_metrics.h"
#include "pf_scan1d.h"

namespace {

constexpr int GP = 8;            // grid points per KDE workgroup
constexpr int HIST_LDS = 2048;   // bins counted in LDS (more go straight to global memory)
constexpr int64_t CVM_MAX_N = int64_t(1) << 20;   // sum (2R - 2i)^2 <= n (2N)^2 < 2^63: exact in 64 bits

// numpy.linspace(start, stop, num)[k] (endpoint=True): k * step + start with step = (stop - start) / (num - 1), or
// (k / div) * delta + start where step underflows to 0; the last point is `stop` itself
__device__ inline double linspace_at(int64_t k, int64_t num, double start, double stop) {
    const int64_t div = num - 1;
    const double delta = stop - start;
    double y;
    if (div > 0) {
        const double step = delta / (double)div;
        y = step == 0.0 ? ((double)k / (double)div) * delta : (double)k * step;
    } else {
        y = (double)k * delta;
    }
    y = y + start;
    if (num > 1 && k == num - 1) y = stop;
    return y;
}

// value of the first (last = false) or last non-empty group: the replicate's pooled minimum / maximum
__device__ double extreme(const Feature &z, bool last, int *sh) {
    const int tid = threadIdx.x;
    for (int base = 0; base < z.G; base += NT) {
        if (tid == 0) *sh = last ? -1 : z.G;
        __syncthreads();
        const int i = base + tid;
        if (i < z.G) {
            const int g = last ? z.G - 1 - i : i;
            int64_t l, ar;
            z.counts(g, l, ar);
            if (l > 0) {
                if (last) atomicMax(sh, g);
                else atomicMin(sh, g);
            }
        }
        __syncthreads();
        const int g = *sh;
        __syncthreads();
        if (last ? g >= 0 : g < z.G) return z.value(g);
    }
    return 0.0;                  // unreachable: every replicate draws rows
}

template <int M>
__global__ void __launch_bounds__(NT) k_scan1d(const double *cols, const int32_t *perm, const int32_t *gstart,
                                               const int32_t *ngroups, const int32_t *cnt, int64_t nr, int64_t nf,
                                               int64_t d, int64_t bins, double *ext, void *out) {
    __shared__ int64_t sa[NT], sb[NT];
    __shared__ double sd[NT];
    __shared__ int sh;
    __shared__ int32_t lhist[M == PFM_M1D_HIST ? 2 * HIST_LDS : 1];
    const int64_t f = blockIdx.x, rep = blockIdx.y, N = nr + nf;
    const int tid = threadIdx.x;
    Feature z;
    z.col = cols + f * N;
    z.perm = perm + f * N;
    z.gs = gstart + f * (N + 1);
    z.cnt = cnt + rep * N;
    z.nr = nr;
    z.N = N;
    z.G = ngroups[f];
    const int64_t rf = rep * d + f;

    double lo = 0.0, hi = 0.0;
    if (M == PFM_M1D_HIST || M == PFM_M1D_KDE) {
        lo = extreme(z, false, &sh);
        hi = extreme(z, true, &sh);
        if (M == PFM_M1D_KDE) {
            if (tid == 0) {
                ext[2 * rf] = lo;
                ext[2 * rf + 1] = hi;
            }
            return;
        }
        if (lo == hi) {          // np.histogram's range of a constant sample
            lo = lo - 0.5;
            hi = hi + 0.5;
        }
    }

    double dmax = -INFINITY, dmin = INFINITY;    // KS
    uint64_t sx = 0, sy = 0;                      // CvM: sum (2R - 2i)^2 of the real / fake rows
    double adr = 0.0, adf = 0.0;                  // AD: scipy's `inner` summed per sample
    int64_t distinct = 0;                         // AD: non-empty groups
    int64_t u2 = 0;                               // AUC: 2 U
    int32_t *const ghist = (int32_t *)out + rf * 2 * bins;       // zeroed by pfm_metric1d
    const bool in_lds = bins <= HIST_LDS;
    int32_t *hist = in_lds ? lhist : ghist;
    if (M == PFM_M1D_HIST && in_lds) {
        for (int64_t k = tid; k < 2 * bins; k += NT) lhist[k] = 0;
        __syncthreads();
    }
    const double Nd = (double)N;

    int64_t carryC = 0, carryR = 0;
    for (int base = 0; base < z.G; base += NT * IPT) {
        int64_t l[IPT], ar[IPT], tl = 0, tr = 0;
#pragma unroll
        for (int i = 0; i < IPT; ++i) {
            const int g = base + tid * IPT + i;
            l[i] = 0;
            ar[i] = 0;
            if (g < z.G) z.counts(g, l[i], ar[i]);
            tl += l[i];
            tr += ar[i];
        }
        int64_t C, Cr, TC, TR;
        block_scan2(tl, tr, C, Cr, TC, TR, sa, sb);
        C += carryC;
        Cr += carryR;
        carryC += TC;
        carryR += TR;
#pragma unroll
        for (int i = 0; i < IPT; ++i) {
            const int g = base + tid * IPT + i;
            const int64_t L = l[i], A = ar[i], Af = L - A, Cf = C - Cr;
            if (L > 0) {
                if (M == PFM_M1D_KS) {
                    // ks_2samp: cdf1 = searchsorted(data1, v, 'right') / n1 at every pooled value v
                    const double diff = (double)(Cr + A) / (double)nr - (double)(Cf + Af) / (double)nf;
                    dmax = fmax(dmax, diff);
                    dmin = fmin(dmin, diff);
                } else if (M == PFM_M1D_CVM) {
                    // the group's average rank R = C + (L + 1) / 2; its real rows are the sorted x's
                    // i = Cr + 1 .. Cr + A: sum_j (B - 2j)^2 = A B^2 - 2 B A (A + 1) + 4 A (A + 1) (2A + 1) / 6 with
                    // B = 2R - 2 Cr.  Wrapping uint64 arithmetic: the true sum is < 2^63, so the residue is exact
                    const uint64_t twoR = (uint64_t)(2 * C + L + 1);
                    const uint64_t br = twoR - 2 * (uint64_t)Cr, bf = twoR - 2 * (uint64_t)Cf;
                    const uint64_t a = (uint64_t)A, b = (uint64_t)Af;
                    const uint64_t qa = a * (a + 1) / 2 * (2 * a + 1) / 3, qb = b * (b + 1) / 2 * (2 * b + 1) / 3;
                    sx += a * br * br - 2 * br * a * (a + 1) + 4 * qa;
                    sy += b * bf * bf - 2 * bf * b * (b + 1) + 4 * qb;
                } else if (M == PFM_M1D_AD) {
                    // scipy _anderson_ksamp_midrank, one Zstar: lj = L, Bj = C + lj / 2., Mij = (C_i + a_i) - a_i / 2.,
                    // inner = lj / float(N) * (N*Mij - Bj*n[i])**2 / (Bj*(N - Bj) - N*lj/4.)
                    const double lj = (double)L;
                    const double Bj = (double)C + lj / 2.0;
                    const double den = Bj * (Nd - Bj) - (double)(N * L) / 4.0;
                    const double w = lj / Nd;
                    double Mr = (double)(Cr + A);
                    Mr = Mr - (double)A / 2.0;
                    double Mf = (double)(Cf + Af);
                    Mf = Mf - (double)Af / 2.0;
                    const double er = Nd * Mr - Bj * (double)nr, ef = Nd * Mf - Bj * (double)nf;
                    adr += w * (er * er) / den;
                    adf += w * (ef * ef) / den;
                    ++distinct;
                } else if (M == PFM_M1D_AUC) {
                    // Mann-Whitney U of the fake (positive) rows: each beats the Cr real rows below, ties count 1/2
                    u2 += Af * (2 * Cr + A);
                } else if (M == PFM_M1D_HIST) {
                    // np.histogram(x, edges): bin k holds e[k] <= v < e[k + 1], the last bin is closed.  The edges
                    // are nondecreasing, so the bin is the largest k <= bins - 1 with e[k] <= v (e[0] = min <= v)
                    const double v = z.value(g);
                    int64_t a = 0, b = bins - 1;
                    while (a < b) {
                        const int64_t mid = (a + b + 1) >> 1;
                        if (linspace_at(mid, bins + 1, lo, hi) <= v) a = mid;
                        else b = mid - 1;
                    }
                    if (A) atomicAdd(&hist[a], (int32_t)A);
                    if (Af) atomicAdd(&hist[bins + a], (int32_t)Af);
                }
            }
            C += L;
            Cr += A;
        }
    }

    if (M == PFM_M1D_KS) {
        sd[tid] = dmax;
        __syncthreads();
        for (int off = NT / 2; off > 0; off >>= 1) {
            if (tid < off) sd[tid] = fmax(sd[tid], sd[tid + off]);
            __syncthreads();
        }
        const double mx = sd[0];
        __syncthreads();
        sd[tid] = dmin;
        __syncthreads();
        for (int off = NT / 2; off > 0; off >>= 1) {
            if (tid < off) sd[tid] = fmin(sd[tid], sd[tid + off]);
            __syncthreads();
        }
        if (tid == 0) {
            // d = max(minS, maxS), minS = clip(-min(cddiffs), 0, 1)
            const double minS = fmin(fmax(-sd[0], 0.0), 1.0);
            ((double *)out)[rf] = minS > mx ? minS : mx;
        }
    } else if (M == PFM_M1D_CVM) {
        int64_t ex, ey, tx, ty;
        block_scan2((int64_t)sx, (int64_t)sy, ex, ey, tx, ty, sa, sb);
        if (tid == 0) {
            ((int64_t *)out)[2 * rf] = tx;
            ((int64_t *)out)[2 * rf + 1] = ty;
        }
    } else if (M == PFM_M1D_AD) {
        const double tr = block_sum(adr, sd);
        const double tf = block_sum(adf, sd);
        int64_t e0, e1, td, t1;
        block_scan2(distinct, 0, e0, e1, td, t1, sa, sb);
        if (tid == 0) {
            double *o = (double *)out + 3 * rf;
            o[0] = tr;
            o[1] = tf;
            o[2] = (double)td;
        }
    } else if (M == PFM_M1D_HIST) {
        if (in_lds) {
            __syncthreads();
            for (int64_t k = tid; k < 2 * bins; k += NT) ghist[k] = lhist[k];
        }
    } else if (M == PFM_M1D_AUC) {
        int64_t e0, e1, tu, t1;
        block_scan2(u2, 0, e0, e1, tu, t1, sa, sb);
        if (tid == 0) ((int64_t *)out)[rf] = tu;
    }
}

// log sum_i c_i exp(-0.5 * (x - v_i)^2 / (h * h)) over one sample's original rows (c_i its draw count), at the
// replicate's grid linspace(min, max, bins): shifted by the largest term, so a density the reference underflows
// to 0 after exp() is a finite log here too
__global__ void __launch_bounds__(NT) k_kde(const double *cols, const int32_t *cnt, const double *ext, int64_t nr,
                                            int64_t nf, int64_t d, int64_t bins, double h_r, double h_f, double *out) {
    __shared__ double red[GP][NT];
    const int64_t nchunk = (bins + GP - 1) / GP;
    const int64_t chunk = blockIdx.x % nchunk, js = blockIdx.x / nchunk;
    const int64_t s = js & 1, f = js >> 1, rep = blockIdx.y, N = nr + nf;
    const int tid = threadIdx.x;
    const int64_t rf = rep * d + f;
    const int64_t off = s ? nr : 0, n = s ? nf : nr;
    const double *v = cols + f * N + off;
    const int32_t *c = cnt + rep * N + off;
    const double lo = ext[2 * rf], hi = ext[2 * rf + 1];
    const double h = s ? h_f : h_r, hh = h * h;
    double x[GP], m[GP], acc[GP];
#pragma unroll
    for (int j = 0; j < GP; ++j) {
        const int64_t k = chunk * GP + j;
        x[j] = linspace_at(k < bins ? k : bins - 1, bins, lo, hi);
        m[j] = -INFINITY;
        acc[j] = 0.0;
    }
    for (int64_t i = tid; i < n; i += NT) {
        if (c[i] == 0) continue;
        const double vi = v[i];
#pragma unroll
        for (int j = 0; j < GP; ++j) {
            const double dx = x[j] - vi;
            m[j] = fmax(m[j], -0.5 * (dx * dx) / hh);
        }
    }
#pragma unroll
    for (int j = 0; j < GP; ++j) red[j][tid] = m[j];
    __syncthreads();
    for (int o = NT / 2; o > 0; o >>= 1) {
        if (tid < o) {
#pragma unroll
            for (int j = 0; j < GP; ++j) red[j][tid] = fmax(red[j][tid], red[j][tid + o]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < GP; ++j) m[j] = red[j][0];
    __syncthreads();
    for (int64_t i = tid; i < n; i += NT) {
        const int32_t ci = c[i];
        if (ci == 0) continue;
        const double vi = v[i], w = (double)ci;
#pragma unroll
        for (int j = 0; j < GP; ++j) {
            const double dx = x[j] - vi;
            acc[j] = acc[j] + w * exp(-0.5 * (dx * dx) / hh - m[j]);
        }
    }
#pragma unroll
    for (int j = 0; j < GP; ++j) red[j][tid] = acc[j];
    __syncthreads();
    for (int o = NT / 2; o > 0; o >>= 1) {
        if (tid < o) {
#pragma unroll
            for (int j = 0; j < GP; ++j) red[j][tid] = red[j][tid] + red[j][tid + o];
        }
        __syncthreads();
    }
    if (tid < GP) {
        const int64_t k = chunk * GP + tid;
        if (k < bins) out[(rf * 2 + s) * bins + k] = m[tid] + log(red[tid][0]);
    }
}

bool m1d_args_ok(int metric, int64_t nr, int64_t nf, int64_t d, int64_t reps, int64_t bins) {
    if (metric < PFM_M1D_KS || metric > PFM_M1D_KDE) return false;
    if (nr < 1 || nf < 1 || d < 1 || reps < 1 || reps > 65535) return false;
    if (nr + nf >= (int64_t)INT32_MAX || d > (int64_t)INT32_MAX) return false;
    if (metric == PFM_M1D_HIST || metric == PFM_M1D_KDE) {
        if (bins < 1 || bins >= (int64_t)INT32_MAX) return false;
        if (metric == PFM_M1D_KDE && ((bins + GP - 1) / GP) * 2 * d > (int64_t)INT32_MAX) return false;
    }
    return true;
}

}  // namespace

extern "C" size_t pfm_metric1d_workspace_bytes(int metric, int64_t nr, int64_t nf, int64_t d, int64_t reps,
                                               int64_t bins) {
    if (!m1d_args_ok(metric, nr, nf, d, reps, bins)) return 0;
    return align256(sizeof(int32_t) * reps * (nr + nf)) + align256(sizeof(double) * 2 * reps * d);
}

extern "C" int pfm_metric1d(void *stream, int metric, const double *cols, const int32_t *perm, const int32_t *gstart,
                            const int32_t *ngroups, int64_t nr, int64_t nf, int64_t d, const int32_t *idx_r,
                            const int32_t *idx_f, int64_t reps, int64_t bins, double h_r, double h_f, void *out,
                            void *workspace, size_t workspace_bytes) {
    if (!cols || !perm || !gstart || !ngroups || !idx_r || !idx_f || !out) return PFM_EINVAL;
    if (!m1d_args_ok(metric, nr, nf, d, reps, bins)) return PFM_EINVAL;
    if (metric == PFM_M1D_CVM && nr + nf > CVM_MAX_N) return PFM_EUNSUPPORTED;
    const size_t need = pfm_metric1d_workspace_bytes(metric, nr, nf, d, reps, bins);
    if (!workspace || workspace_bytes < need) return PFM_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int64_t N = nr + nf;
    int32_t *cnt = (int32_t *)workspace;
    double *ext = (double *)((char *)workspace + align256(sizeof(int32_t) * reps * N));

    PFM_TRY(launch_counts(st, idx_r, idx_f, nr, nf, reps, cnt));

    const dim3 grid((unsigned)d, (unsigned)reps);
    switch (metric) {
        case PFM_M1D_KS:
            hipLaunchKernelGGL(k_scan1d<PFM_M1D_KS>, grid, dim3(NT), 0, st, cols, perm, gstart, ngroups, cnt, nr, nf, d,
                               bins, ext, out);
            break;
        case PFM_M1D_CVM:
            hipLaunchKernelGGL(k_scan1d<PFM_M1D_CVM>, grid, dim3(NT), 0, st, cols, perm, gstart, ngroups, cnt, nr, nf,
                               d, bins, ext, out);
            break;
        case PFM_M1D_AD:
            hipLaunchKernelGGL(k_scan1d<PFM_M1D_AD>, grid, dim3(NT), 0, st, cols, perm, gstart, ngroups, cnt, nr, nf, d,
                               bins, ext, out);
            break;
        case PFM_M1D_AUC:
            hipLaunchKernelGGL(k_scan1d<PFM_M1D_AUC>, grid, dim3(NT), 0, st, cols, perm, gstart, ngroups, cnt, nr, nf,
                               d, bins, ext, out);
            break;
        case PFM_M1D_HIST:
            PFM_TRY(hipMemsetAsync(out, 0, sizeof(int32_t) * reps * d * 2 * bins, st));
            hipLaunchKernelGGL(k_scan1d<PFM_M1D_HIST>, grid, dim3(NT), 0, st, cols, perm, gstart, ngroups, cnt, nr, nf,
                               d, bins, ext, out);
            break;
        case PFM_M1D_KDE:
            hipLaunchKernelGGL(k_scan1d<PFM_M1D_KDE>, grid, dim3(NT), 0, st, cols, perm, gstart, ngroups, cnt, nr, nf,
                               d, bins, ext, out);
            PFM_TRY(hipGetLastError());
            hipLaunchKernelGGL(k_kde, dim3((unsigned)(((bins + GP - 1) / GP) * 2 * d), (unsigned)reps), dim3(NT), 0, st,
                               cols, cnt, ext, nr, nf, d, bins, h_r, h_f, (double *)out);
            break;
    }
    PFM_TRY(hipGetLastError());
    return PFM_OK;
}
