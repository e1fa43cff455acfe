// pf_cnormal.hip -- ConditionalNormal training and sampling for gfx950 (C ABI: pf_cnormal.h).
//
// The net is the reference's: a trunk of activated Linears over the conditions, two heads (mu, log_sigma) and the d x d
// Linear `out`.  Rows are evaluated "one thread = one row" with the row state in LDS [feature][S], as the WGAN kernels do;
// the weights are read with wave-uniform addresses.  Sigmoid and the d x d inverse are new here and live in this file.
//
// One training iteration = 2 launches:
//   k_step    row tiles of R batch rows.  In full-covariance mode every workgroup first inverts out.weight (Gauss-Jordan,
//             partial pivoting, float64, [d, 2d] in LDS: the same arithmetic in every workgroup, so the same bits).  Then
//             each thread runs its row: trunk, heads, t = x or M (x - b), the row's loss, dL/dmu and dL/dlog_sigma.  The
//             backward sweeps ("thread = parameter") sum over the tile's rows in row order and write the workgroup's partial
//             gradient; the `out` block of the partial holds sum_r G_r inv_r^T and sum_r G_r.
//   k_finish  one thread per parameter: the workgroups' partials summed in workgroup order, then Adam.  One extra workgroup
//             owns the `out` block: it reduces the d x d sums, applies -M^T and runs Adam on out.weight / out.bias.
// A singular out.weight sets an error word; k_finish then leaves parameters and optimizer state alone.
// Inference (pfn_forward): one launch, thread = row; the inverse is computed only when inv is asked for.
//
// No float atomics anywhere: a call is bitwise reproducible, and pfn_fit_epoch is the same launches as the loop of
// pfn_train_step calls.
#include "../../csrc/rnvp_common.h"
#include "../pf_rowtile.h"

#include <math.h>

#include "pf_cnormal.h"

using pf_rowtile::big_lds;
using pf_rowtile::kLds;
using pf_rowtile::Plan;

namespace {

constexpr int NT = 256;                   // threads of every workgroup here
constexpr int kInvPer = (2 * PFN_MAX_D * PFN_MAX_D + NT - 1) / NT;   // elements of the [d, 2d] system per thread

struct NShape {
    int d, c, nh, act, indep;
    int nin[PFN_MAX_HIDDEN], nout[PFN_MAX_HIDDEN], woff[PFN_MAX_HIDDEN], boff[PFN_MAX_HIDDEN];   // the trunk's Linears
    int muW, muB, lsW, lsB, outW, outB;
    int hl;           // width of the last hidden layer
    int hs, hmax;     // sum / max of the hidden widths
    int P, Pmain;     // all parameters / all but out's (out is the tail: outW == Pmain)
    int step_unit;    // floats of k_step LDS per LDS row
    int fwd_unit;     // floats of k_forward LDS per LDS row
    int shared;       // bytes in front of the rows: the [d, 2d] float64 system, M = W^-1 as float32, a flag word
};

int make_nshape(const pfn_shape *s, NShape &w) {
    if (!s || s->d < 1 || s->c < 1 || s->n_hidden < 1 || s->n_hidden > PFN_MAX_HIDDEN) return PFN_EINVAL;
    if (s->act != PFN_ACT_TANH && s->act != PFN_ACT_RELU && s->act != PFN_ACT_SIGMOID) return PFN_EINVAL;
    if (s->independent != 0 && s->independent != 1) return PFN_EINVAL;
    memset(&w, 0, sizeof(w));
    w.d = s->d; w.c = s->c; w.nh = s->n_hidden; w.act = s->act; w.indep = s->independent;
    int64_t off = 0, in = s->c, hs = 0;
    for (int i = 0; i < s->n_hidden; ++i) {
        const int64_t out = s->hidden[i];
        if (out < 1) return PFN_EINVAL;
        if (out > (1 << 20) || off > (1 << 28)) return PFN_EUNSUPPORTED;
        w.nin[i] = (int)in; w.nout[i] = (int)out;
        w.woff[i] = (int)off; w.boff[i] = (int)(off + out * in);
        off += out * in + out;
        hs += out;
        w.hmax = out > w.hmax ? (int)out : w.hmax;
        in = out;
    }
    if (s->d > (1 << 12) || off > (1 << 28)) return PFN_EUNSUPPORTED;
    const int64_t d = s->d;
    w.hl = (int)in; w.hs = (int)hs;
    w.muW = (int)off; w.muB = (int)(off + d * in); off += d * in + d;
    w.lsW = (int)off; w.lsB = (int)(off + d * in); off += d * in + d;
    w.Pmain = (int)off;
    w.outW = (int)off; w.outB = (int)(off + d * d); off += d * d + d;
    w.P = (int)off;
    // k_step rows: conditions, every hidden activation, mu -> dL/dmu, log_sigma -> dL/dlog_sigma, t, two gradient buffers,
    // the row's loss
    w.step_unit = w.c + w.hs + 3 * w.d + 2 * w.hmax + 1;
    // k_forward rows: conditions, every hidden activation, mu, sigma, mu + eps sigma
    w.fwd_unit = w.c + w.hs + 3 * w.d;
    const int dd = w.d <= PFN_MAX_D ? w.d : PFN_MAX_D;
    w.shared = (int)rnvp::align_up((size_t)2 * dd * dd * sizeof(double) + (size_t)dd * dd * sizeof(float) + 16, 16);
    return PFN_OK;
}

// LDS rows (S = tile + 1) that fit behind the shared region, capped so that tile <= NT
int tile_cap(const NShape &w, int unit) {
    if (w.d > PFN_MAX_D) return 0;
    const int64_t S = (int64_t)((kLds - w.shared) / ((size_t)unit * sizeof(float)));
    const int64_t R = S - 1;
    return (int)(R > NT ? NT : (R < 0 ? 0 : R));
}

// the launches (pf_rowtile::Plan): enqueue_step / pfn_forward launch from these and pfn_tiling reports them
Plan step_plan(const NShape &w, int64_t rows) {
    return pf_rowtile::make_plan(pf_rowtile::step_tile(tile_cap(w, w.step_unit), rows), w.shared, 1, w.step_unit, rows);
}

Plan fwd_plan(const NShape &w, int64_t n) {
    return pf_rowtile::make_plan(tile_cap(w, w.fwd_unit), w.shared, 1, w.fwd_unit, n);
}

struct Ws {
    float *gpart;    // [G][P]
    float *lpart;    // [G]
    float *minv;     // [PFN_MAX_D^2]: M = out.weight^-1 of the step (workgroup 0 writes it, k_finish reads it)
    int32_t *err;    // [0] the step's error word, [1] the call's sticky word when the caller passes no status
};

size_t ws_bytes(const NShape &w, int64_t batch_rows, Ws *out, void *base) {
    const int64_t G = pf_rowtile::step_wg_bound(tile_cap(w, w.step_unit), batch_rows);
    const size_t a = rnvp::align_up((size_t)G * w.P * sizeof(float), 256);
    const size_t b = rnvp::align_up((size_t)G * sizeof(float), 256);
    const size_t c = rnvp::align_up((size_t)PFN_MAX_D * PFN_MAX_D * sizeof(float), 256);
    if (out) {
        char *p = (char *)base;
        out->gpart = (float *)p; out->lpart = (float *)(p + a); out->minv = (float *)(p + a + b);
        out->err = (int32_t *)(p + a + b + c);
    }
    return a + b + c + 256;
}

// torch.optim.Adam's scalars (bias corrections in double, like torch); the arithmetic is rnvp::adam_one
rnvp::AdamK make_adam_k(const pfn_adam *o, int64_t step) {
    rnvp::AdamK a;
    const double bc1 = 1.0 - pow(o->beta1, (double)step);
    const double bc2 = 1.0 - pow(o->beta2, (double)step);
    a.step_size = (float)(o->lr / bc1);
    a.bc2_sqrt = (float)sqrt(bc2);
    a.w1 = (float)(1.0 - o->beta1);
    a.beta2 = (float)o->beta2;
    a.w2 = (float)(1.0 - o->beta2);
    a.wd = (float)o->weight_decay;
    a.eps = (float)o->eps;
    a.use_wd = o->weight_decay != 0.0;
    return a;
}

// ---- device code -------------------------------------------------------------------------------------------------

__device__ __forceinline__ float act_fwd(float v, int act) {
    if (act == PFN_ACT_TANH) return tanhf(v);
    if (act == PFN_ACT_SIGMOID) return 1.0f / (1.0f + expf(-v));
    return fmaxf(v, 0.f);
}

// d act / d v from the activation's OUTPUT a
__device__ __forceinline__ float act_bwd(float a, int act) {
    if (act == PFN_ACT_TANH) return 1.f - a * a;
    if (act == PFN_ACT_SIGMOID) return a * (1.f - a);
    return a > 0.f ? 1.f : 0.f;
}

// M = W^-1 (W: d x d float32, row-major) by Gauss-Jordan elimination with partial pivoting in float64 on the augmented
// system A = [W | I] ([d, 2d] in LDS); Mf receives M as float32.  Every thread of the workgroup calls it (barriers inside)
// and gets the same result: nonzero when a pivot is zero or not finite, or an entry of Mf is not finite.  Each column
// step computes all new elements from the old system, then a barrier, then stores them: 2 barriers per column.
__device__ int invert_out(const float *__restrict__ W, int d, double *A, float *Mf, int *flag, int t) {
    const int w2 = 2 * d, ne = d * w2;
    for (int idx = t; idx < ne; idx += NT) {
        const int r = idx / w2, j = idx - r * w2;
        A[idx] = j < d ? (double)W[r * d + j] : (j - d == r ? 1.0 : 0.0);
    }
    if (t == 0) *flag = 0;
    __syncthreads();
    int bad = 0;
    for (int col = 0; col < d; ++col) {
        int p = col;
        double pv = A[col * w2 + col];
        for (int r = col + 1; r < d; ++r) {
            const double v = A[r * w2 + col];
            if (fabs(v) > fabs(pv)) { pv = v; p = r; }
        }
        if (pv == 0.0 || !isfinite(pv)) bad = 1;
        const double acc = A[col * w2 + col];
        double nv[kInvPer];
#pragma unroll
        for (int k = 0; k < kInvPer; ++k) {
            const int idx = t + k * NT;
            nv[k] = 0.0;
            if (idx < ne) {
                const int r = idx / w2, j = idx - r * w2;
                const double prow = A[p * w2 + j] / pv;              // the scaled pivot row
                if (r == col) nv[k] = prow;
                else {                                               // row p receives the old row `col`
                    const double f = (r == p) ? acc : A[r * w2 + col];
                    const double base = (r == p) ? A[col * w2 + j] : A[idx];
                    nv[k] = base - f * prow;
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kInvPer; ++k) {
            const int idx = t + k * NT;
            if (idx < ne) A[idx] = nv[k];
        }
        __syncthreads();
    }
    for (int idx = t; idx < ne; idx += NT) {
        const int r = idx / w2, j = idx - r * w2;
        if (j >= d) {
            const float m = (float)A[idx];
            Mf[r * d + (j - d)] = m;
            if (!isfinite(m)) *flag = 1;
        }
    }
    __syncthreads();
    return bad | *flag;
}

// the trunk for row t: every hidden activation vector kept, consecutively, in acts [hs][S]
__device__ void trunk_forward(const float *__restrict__ p, const NShape &w, const float *cin, float *acts, int S, int t) {
    const float *cur = cin;
    float *dst = acts;
    for (int k = 0; k < w.nh; ++k) {
        const int nin = w.nin[k], nout = w.nout[k];
        const float *__restrict__ Wk = p + w.woff[k];
        const float *__restrict__ b = p + w.boff[k];
        for (int o = 0; o < nout; o += 4) {
            const int o1 = min(o + 1, nout - 1), o2 = min(o + 2, nout - 1), o3 = min(o + 3, nout - 1);
            const float *w0 = Wk + o * nin, *w1 = Wk + o1 * nin, *w2 = Wk + o2 * nin, *w3 = Wk + o3 * nin;
            float a0 = b[o], a1 = b[o1], a2 = b[o2], a3 = b[o3];
            for (int i = 0; i < nin; ++i) {
                const float v = cur[i * S + t];
                a0 = fmaf(v, w0[i], a0);
                a1 = fmaf(v, w1[i], a1);
                a2 = fmaf(v, w2[i], a2);
                a3 = fmaf(v, w3[i], a3);
            }
            dst[o * S + t] = act_fwd(a0, w.act);
            if (o + 1 < nout) dst[(o + 1) * S + t] = act_fwd(a1, w.act);
            if (o + 2 < nout) dst[(o + 2) * S + t] = act_fwd(a2, w.act);
            if (o + 3 < nout) dst[(o + 3) * S + t] = act_fwd(a3, w.act);
        }
        cur = dst;
        dst += nout * S;
    }
}

// the two heads for row t: mu and log_sigma [d][S] from the last hidden layer h [hl][S]
__device__ void heads_forward(const float *__restrict__ p, const NShape &w, const float *h, float *mu, float *ls, int S,
                              int t) {
    const float *__restrict__ Wm = p + w.muW, *__restrict__ Wl = p + w.lsW;
    for (int j = 0; j < w.d; ++j) {
        float a = p[w.muB + j], b = p[w.lsB + j];
        for (int i = 0; i < w.hl; ++i) {
            const float v = h[i * S + t];
            a = fmaf(v, Wm[j * w.hl + i], a);
            b = fmaf(v, Wl[j * w.hl + i], b);
        }
        mu[j * S + t] = a;
        ls[j * S + t] = b;
    }
}

__global__ __launch_bounds__(NT) void k_step(NShape w, int R, const float *__restrict__ params,
                                             const float *__restrict__ x, const float *__restrict__ c,
                                             const int64_t *__restrict__ row_index, int64_t rows, float inv_Bd,
                                             float *__restrict__ gpart, float *__restrict__ lpart,
                                             float *__restrict__ minv, int32_t *__restrict__ err_step) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int t = threadIdx.x, d = w.d;
    const int S = R + 1;
    const int64_t r0 = (int64_t)blockIdx.x * R;
    const int TB = (int)(rows - r0 < R ? rows - r0 : R);
    double *A = (double *)smem;
    float *Mf = (float *)(smem + (size_t)2 * d * d * sizeof(double));
    int *flag = (int *)(Mf + d * d);
    float *cin = (float *)(smem + w.shared);
    float *acts = cin + w.c * S;
    float *gmu = acts + w.hs * S;        // mu, then dL/dmu
    float *gls = gmu + d * S;            // log_sigma, then dL/dlog_sigma
    float *tt = gls + d * S;             // t = x (independent) or inv (full)
    float *bufA = tt + d * S;
    float *bufB = bufA + w.hmax * S;
    float *lrow = bufB + w.hmax * S;
    const float *h = acts + (w.hs - w.hl) * S;
    float *gp = gpart + (int64_t)blockIdx.x * w.P;

    int bad = 0;
    if (!w.indep) {
        bad = invert_out(params + w.outW, d, A, Mf, flag, t);
        if (blockIdx.x == 0)
            for (int idx = t; idx < d * d; idx += NT) minv[idx] = Mf[idx];
    }
    if (blockIdx.x == 0 && t == 0) err_step[0] = bad;

    if (t < TB) {
        const int64_t brow = r0 + t;
        const int64_t row = row_index ? row_index[brow] : brow;
        for (int j = 0; j < w.c; ++j) cin[j * S + t] = c[row * w.c + j];
        trunk_forward(params, w, cin, acts, S, t);
        heads_forward(params, w, h, gmu, gls, S, t);
        const float *xr = x + row * d;
        const float *bo = params + w.outB;
        float loss = 0.f;
        for (int j = 0; j < d; ++j) {
            float tv;
            if (w.indep) tv = xr[j];
            else {
                tv = 0.f;
                for (int k = 0; k < d; ++k) tv = fmaf(Mf[j * d + k], xr[k] - bo[k], tv);
            }
            const float m = gmu[j * S + t], l = gls[j * S + t];
            const float sg = expf(l), s2 = sg * sg, df = tv - m;
            const float q = df * df / s2;
            loss += df * df / (2.f * s2) + l;                // (t - mu)^2 / (2 sigma^2) + log(sigma)
            tt[j * S + t] = tv;
            gmu[j * S + t] = -(df / s2) * inv_Bd;
            gls[j * S + t] = (1.f - q) * inv_Bd;
        }
        lrow[t] = loss;
    }
    __syncthreads();
    if (t == 0) {
        float a = 0.f;
        for (int r = 0; r < TB; ++r) a += lrow[r];
        lpart[blockIdx.x] = a;
    }
    // the heads' parameter gradients: thread = (q, i), rows in row order
    for (int idx = t; idx < d * w.hl; idx += NT) {
        const int q = idx / w.hl, i = idx - q * w.hl;
        const float *gm = gmu + q * S, *gl = gls + q * S, *hi = h + i * S;
        float a = 0.f, b = 0.f;
        for (int r = 0; r < TB; ++r) { a = fmaf(gm[r], hi[r], a); b = fmaf(gl[r], hi[r], b); }
        gp[w.muW + idx] = a;
        gp[w.lsW + idx] = b;
    }
    for (int q = t; q < d; q += NT) {
        const float *gm = gmu + q * S, *gl = gls + q * S;
        float a = 0.f, b = 0.f;
        for (int r = 0; r < TB; ++r) { a += gm[r]; b += gl[r]; }
        gp[w.muB + q] = a;
        gp[w.lsB + q] = b;
    }
    if (!w.indep) {
        // G_r = dL/dinv_r = -dL/dmu_r: the tile's sum_r G_r inv_r^T and sum_r G_r (k_finish applies -M^T)
        for (int idx = t; idx < d * d; idx += NT) {
            const int k = idx / d, j = idx - k * d;
            const float *gm = gmu + k * S, *iv = tt + j * S;
            float a = 0.f;
            for (int r = 0; r < TB; ++r) a = fmaf(-gm[r], iv[r], a);
            gp[w.outW + idx] = a;
        }
        for (int k = t; k < d; k += NT) {
            const float *gm = gmu + k * S;
            float a = 0.f;
            for (int r = 0; r < TB; ++r) a -= gm[r];
            gp[w.outB + k] = a;
        }
    }
    // d loss / d h_last: thread = row
    if (t < TB) {
        const float *__restrict__ Wm = params + w.muW, *__restrict__ Wl = params + w.lsW;
        for (int i = 0; i < w.hl; ++i) {
            float a = 0.f;
            for (int q = 0; q < d; ++q) {
                a = fmaf(gmu[q * S + t], Wm[q * w.hl + i], a);
                a = fmaf(gls[q * S + t], Wl[q * w.hl + i], a);
            }
            bufA[i * S + t] = a;
        }
    }
    // the trunk, last Linear first
    float *gcur = bufA, *gprev = bufB;
    int aoff = w.hs;
    for (int k = w.nh - 1; k >= 0; --k) {
        const int nin = w.nin[k], nout = w.nout[k];
        aoff -= nout;
        const float *ak = acts + aoff * S;
        const float *inp = (k == 0) ? cin : acts + (aoff - nin) * S;
        if (t < TB)
            for (int q = 0; q < nout; ++q) gcur[q * S + t] *= act_bwd(ak[q * S + t], w.act);
        __syncthreads();
        for (int idx = t; idx < nout * nin; idx += NT) {
            const int q = idx / nin, i = idx - q * nin;
            const float *gq = gcur + q * S, *xi = inp + i * S;
            float a = 0.f;
            for (int r = 0; r < TB; ++r) a = fmaf(gq[r], xi[r], a);
            gp[w.woff[k] + idx] = a;
        }
        for (int q = t; q < nout; q += NT) {
            const float *gq = gcur + q * S;
            float a = 0.f;
            for (int r = 0; r < TB; ++r) a += gq[r];
            gp[w.boff[k] + q] = a;
        }
        if (k > 0 && t < TB) {
            const float *__restrict__ Wk = params + w.woff[k];
            for (int i = 0; i < nin; ++i) {
                float a = 0.f;
                for (int q = 0; q < nout; ++q) a = fmaf(gcur[q * S + t], Wk[q * nin + i], a);
                gprev[i * S + t] = a;
            }
        }
        float *tmp = gcur; gcur = gprev; gprev = tmp;
    }
}

__global__ __launch_bounds__(NT) void k_finish(NShape w, int G, const float *__restrict__ gpart,
                                               const float *__restrict__ lpart, const float *__restrict__ minv,
                                               const int32_t *__restrict__ err_step, float Bd, float *params,
                                               float *exp_avg, float *exp_avg_sq, float *grad_out, float *loss_out,
                                               rnvp::AdamK adam, int update, int32_t *status, int first) {
    __shared__ float sums[PFN_MAX_D * PFN_MAX_D + PFN_MAX_D];
    const int t = threadIdx.x, d = w.d;
    const int err = err_step[0];
    const bool step = update && !err;
    const int nbm = (w.Pmain + NT - 1) / NT;
    if (blockIdx.x == 0 && t == 0) {
        if (loss_out) {
            float a = 0.f;
            for (int k = 0; k < G; ++k) a += lpart[k];
            loss_out[0] = a / Bd;
        }
        if (first || err) status[0] = err;       // sticky over the batches of one call
    }
    if ((int)blockIdx.x < nbm) {
        const int i = blockIdx.x * NT + t;
        if (i < w.Pmain) {
            float g = 0.f;
            for (int k = 0; k < G; ++k) g += gpart[(int64_t)k * w.P + i];
            if (grad_out) grad_out[i] = g;
            if (step) rnvp::adam_one(params[i], g, exp_avg[i], exp_avg_sq[i], adam);
        }
        return;
    }
    // the workgroup of the `out` block
    const int no = d * d + d;
    if (w.indep) {     // no gradient: Adam skips it entirely (no update, no weight decay, no state)
        if (grad_out)
            for (int idx = t; idx < no; idx += NT) grad_out[w.outW + idx] = 0.f;
        return;
    }
    for (int idx = t; idx < no; idx += NT) {
        float a = 0.f;
        for (int k = 0; k < G; ++k) a += gpart[(int64_t)k * w.P + w.outW + idx];
        sums[idx] = a;
    }
    __syncthreads();
    for (int idx = t; idx < no; idx += NT) {
        float g = 0.f;
        if (idx < d * d) {                       // dL/dW = -M^T (sum_r G_r inv_r^T)
            const int i = idx / d, j = idx - i * d;
            for (int k = 0; k < d; ++k) g = fmaf(minv[k * d + i], sums[k * d + j], g);
        } else {                                 // dL/db = -M^T (sum_r G_r)
            const int i = idx - d * d;
            for (int k = 0; k < d; ++k) g = fmaf(minv[k * d + i], sums[d * d + k], g);
        }
        g = -g;
        const int pi = w.outW + idx;
        if (grad_out) grad_out[pi] = g;
        if (step) rnvp::adam_one(params[pi], g, exp_avg[pi], exp_avg_sq[pi], adam);
    }
}

// inference: thread = row, T rows per workgroup
__global__ __launch_bounds__(NT) void k_forward(NShape w, int T, const float *__restrict__ params,
                                                const float *__restrict__ c, const float *__restrict__ eps,
                                                const float *__restrict__ x, int64_t n, float *__restrict__ mu_out,
                                                float *__restrict__ sigma_out, float *__restrict__ xt_out,
                                                float *__restrict__ inv_out, int32_t *__restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int t = threadIdx.x, d = w.d, S = T + 1;
    double *A = (double *)smem;
    float *Mf = (float *)(smem + (size_t)2 * d * d * sizeof(double));
    int *flag = (int *)(Mf + d * d);
    float *cin = (float *)(smem + w.shared);
    float *acts = cin + w.c * S;
    float *mu = acts + w.hs * S;
    float *sg = mu + d * S;
    float *y = sg + d * S;
    int bad = 0;
    if (inv_out) bad = invert_out(params + w.outW, d, A, Mf, flag, t);
    if (status && blockIdx.x == 0 && t == 0) status[0] = bad;
    const int64_t row = (int64_t)blockIdx.x * T + t;
    if (t >= T || row >= n) return;      // no barriers below
    for (int j = 0; j < w.c; ++j) cin[j * S + t] = c[row * w.c + j];
    trunk_forward(params, w, cin, acts, S, t);
    heads_forward(params, w, acts + (w.hs - w.hl) * S, mu, sg, S, t);
    for (int j = 0; j < d; ++j) {
        const float s = expf(sg[j * S + t]);
        sg[j * S + t] = s;
        if (mu_out) mu_out[row * d + j] = mu[j * S + t];
        if (sigma_out) sigma_out[row * d + j] = s;
    }
    const float *__restrict__ Wo = params + w.outW, *__restrict__ bo = params + w.outB;
    if (xt_out) {
        for (int j = 0; j < d; ++j) {
            const float v = mu[j * S + t] + eps[row * d + j] * sg[j * S + t];     // two roundings, as the reference
            if (w.indep) xt_out[row * d + j] = v;
            else y[j * S + t] = v;
        }
        if (!w.indep)
            for (int j = 0; j < d; ++j) {
                float a = bo[j];
                for (int k = 0; k < d; ++k) a = fmaf(y[k * S + t], Wo[j * d + k], a);
                xt_out[row * d + j] = a;
            }
    }
    if (inv_out)
        for (int j = 0; j < d; ++j) {
            float a = 0.f;
            for (int k = 0; k < d; ++k) a = fmaf(Mf[j * d + k], x[row * d + k] - bo[k], a);
            inv_out[row * d + j] = a;
        }
}

std::atomic<uint64_t> g_lds_step{0}, g_lds_fwd{0};

int enqueue_step(hipStream_t st, const NShape &w, float *params, float *m, float *v, const float *x, const float *c,
                 const int64_t *ri, int64_t rows, const rnvp::AdamK *adam, float *grad_out, float *loss_out,
                 int32_t *status, int first, const Ws &ws) {
    const Plan pl = step_plan(w, rows);
    const int R = pl.tile;
    const int64_t G = pl.wgs;
    const size_t lds = pl.lds;
    if (int e = big_lds(k_step, lds, g_lds_step)) return e;
    const float Bd = (float)rows * (float)w.d;
    hipLaunchKernelGGL(k_step, dim3((unsigned)G), dim3(NT), lds, st, w, R, params, x, c, ri, rows, 1.0f / Bd, ws.gpart,
                       ws.lpart, ws.minv, ws.err);
    RNVP_HIP_TRY(hipGetLastError());
    const int blocks = (w.Pmain + NT - 1) / NT + 1;
    const rnvp::AdamK a = adam ? *adam : rnvp::AdamK{};
    hipLaunchKernelGGL(k_finish, dim3((unsigned)blocks), dim3(NT), 0, st, w, (int)G, ws.gpart, ws.lpart, ws.minv, ws.err,
                       Bd, params, m, v, grad_out, loss_out, a, adam ? 1 : 0, status ? status : ws.err + 1, first);
    RNVP_HIP_TRY(hipGetLastError());
    return PFN_OK;
}

int check_train(const NShape &w, int64_t batch_rows, void *ws, size_t wsb, Ws &out) {
    if (tile_cap(w, w.step_unit) < 1) return PFN_EUNSUPPORTED;
    if (!ws || wsb < ws_bytes(w, batch_rows, &out, ws)) return PFN_EWORKSPACE;
    return PFN_OK;
}

bool bad_adam(const pfn_adam *o, int64_t step) { return !o || step < 1; }

}  // namespace

extern "C" {

int pfn_version(void) { return PFN_VERSION; }

const char *pfn_status_string(int status) {
    switch (status) {
    case PFN_OK: return "ok";
    case PFN_EINVAL: return "invalid argument";
    case PFN_EUNSUPPORTED: return "shape unsupported: d exceeds PFN_MAX_D (32) or one row of the network does not fit the 160 KiB of LDS";
    case PFN_EWORKSPACE: return "workspace too small";
    default: return status > 0 ? hipGetErrorString((hipError_t)status) : "unknown status";
    }
}

int64_t pfn_param_count(const pfn_shape *s) {
    if (!s || s->d < 1 || s->c < 1 || s->n_hidden < 1 || s->n_hidden > PFN_MAX_HIDDEN) return -1;
    int64_t off = 0, in = s->c;
    for (int i = 0; i < s->n_hidden; ++i) {
        if (s->hidden[i] < 1) return -1;
        off += (int64_t)s->hidden[i] * in + s->hidden[i];
        in = s->hidden[i];
    }
    const int64_t d = s->d;
    return off + 2 * (d * in + d) + d * d + d;
}

size_t pfn_workspace_bytes(const pfn_shape *s, int64_t batch_rows) {
    NShape w;
    if (make_nshape(s, w) || batch_rows < 1 || tile_cap(w, w.step_unit) < 1) return 0;
    return ws_bytes(w, batch_rows, nullptr, nullptr);
}

int pfn_tiling(const pfn_shape *s, int64_t rows, pfn_tiling_info *out) {
    NShape w;
    const int e = make_nshape(s, w);
    if (e == PFN_EINVAL || !out || rows < 1) return PFN_EINVAL;
    memset(out, 0, sizeof(*out));
    if (e) return e;
    const Plan fw = fwd_plan(w, rows);
    out->fwd_tile = fw.tile; out->fwd_lds_bytes = (int64_t)fw.lds;
    out->step_cap = tile_cap(w, w.step_unit);
    if (out->step_cap < 1) return PFN_EUNSUPPORTED;
    const Plan st = step_plan(w, rows);
    out->step_tile = st.tile; out->step_wgs = st.wgs; out->step_lds_bytes = (int64_t)st.lds;
    out->step_wg_bound = pf_rowtile::step_wg_bound(out->step_cap, rows);
    return PFN_OK;
}

int pfn_forward(void *stream, const pfn_shape *s, const float *params, const float *c, const float *eps,
                const float *x, int64_t n, float *mu, float *sigma, float *x_tilde, float *inv, int32_t *status) {
    NShape w;
    if (int e = make_nshape(s, w)) return e;
    if (tile_cap(w, w.fwd_unit) < 1) return PFN_EUNSUPPORTED;
    if (!params || !c || n < 1 || (x_tilde && !eps) || (inv && !x)) return PFN_EINVAL;
    const Plan pl = fwd_plan(w, n);
    const int T = pl.tile;
    const size_t lds = pl.lds;
    if (int e = big_lds(k_forward, lds, g_lds_fwd)) return e;
    hipLaunchKernelGGL(k_forward, dim3((unsigned)pl.wgs), dim3(NT), lds, (hipStream_t)stream, w, T, params, c,
                       eps, x, n, mu, sigma, x_tilde, inv, status);
    RNVP_HIP_TRY(hipGetLastError());
    return PFN_OK;
}

int pfn_loss_grad(void *stream, const pfn_shape *s, const float *params, const float *x, const float *c,
                  const int64_t *row_index, int64_t rows, float *grad_out, float *loss_out, int32_t *status,
                  void *workspace, size_t workspace_bytes) {
    NShape w;
    if (int e = make_nshape(s, w)) return e;
    if (tile_cap(w, w.step_unit) < 1) return PFN_EUNSUPPORTED;
    if (!params || !x || !c || rows < 1) return PFN_EINVAL;
    Ws ws;
    if (int e = check_train(w, rows, workspace, workspace_bytes, ws)) return e;
    return enqueue_step((hipStream_t)stream, w, const_cast<float *>(params), nullptr, nullptr, x, c, row_index, rows,
                        nullptr, grad_out, loss_out, status, 1, ws);
}

int pfn_train_step(void *stream, const pfn_shape *s, float *params, float *exp_avg, float *exp_avg_sq,
                   const float *x, const float *c, const int64_t *row_index, int64_t rows, const pfn_adam *opt,
                   int64_t step, float *grad_out, float *loss_out, int32_t *status, void *workspace,
                   size_t workspace_bytes) {
    NShape w;
    if (int e = make_nshape(s, w)) return e;
    if (tile_cap(w, w.step_unit) < 1) return PFN_EUNSUPPORTED;
    if (!params || !exp_avg || !exp_avg_sq || !x || !c || rows < 1 || bad_adam(opt, step)) return PFN_EINVAL;
    Ws ws;
    if (int e = check_train(w, rows, workspace, workspace_bytes, ws)) return e;
    const rnvp::AdamK a = make_adam_k(opt, step);
    return enqueue_step((hipStream_t)stream, w, params, exp_avg, exp_avg_sq, x, c, row_index, rows, &a, grad_out,
                        loss_out, status, 1, ws);
}

int pfn_fit_epoch(void *stream, const pfn_shape *s, float *params, float *exp_avg, float *exp_avg_sq,
                  const float *x, const float *c, const int64_t *perm, int64_t n, int64_t batch_size,
                  const pfn_adam *opt, int64_t first_step, float *losses, int32_t *status, void *workspace,
                  size_t workspace_bytes) {
    NShape w;
    if (int e = make_nshape(s, w)) return e;
    if (tile_cap(w, w.step_unit) < 1) return PFN_EUNSUPPORTED;
    if (!params || !exp_avg || !exp_avg_sq || !x || !c || !perm || !losses || n < 1 || batch_size < 1 ||
        bad_adam(opt, first_step))
        return PFN_EINVAL;
    const int64_t B = batch_size < n ? batch_size : n;
    Ws ws;
    if (int e = check_train(w, B, workspace, workspace_bytes, ws)) return e;
    const int64_t nb = (n + batch_size - 1) / batch_size;
    for (int64_t b = 0; b < nb; ++b) {
        const int64_t s0 = b * batch_size, rows = (n - s0 < batch_size) ? n - s0 : batch_size;
        const rnvp::AdamK a = make_adam_k(opt, first_step + b);
        if (int e = enqueue_step((hipStream_t)stream, w, params, exp_avg, exp_avg_sq, x, c, perm + s0, rows, &a, nullptr,
                                 losses + b, status, b == 0, ws))
            return e;
    }
    return PFN_OK;
}

}  // extern "C"
