// pf_wgan.hip -- ConditionalWGAN training and sampling for gfx950 (C ABI: pf_wgan.h).
//
// Both nets are the reference's (Linear, act, ..., Linear) MLPs, evaluated "one thread = one row" with the row state in
// LDS [feature][S]: the backward is net_backward of ../../csrc/rnvp_generic_net.h (included unchanged), the forward
// its net_forward with an exact tanh (mlp_forward below).
//
// One training iteration = 2 launches:
//   k_step    row tiles of R batch rows; each workgroup gathers its rows through row_index, runs
//             G([z || c]) -> fake, then D on the fake rows (LDS rows 0..TB-1) and, on critic steps, on the real rows
//             (rows TB..2TB-1).  The backward is seeded with +-1/B per row of D's output: critic steps take D's parameter
//             gradient over all 2TB rows; generator steps take D's input gradient of the x columns, then G's parameter
//             gradient.  Each workgroup writes its partial gradient and partial loss (row order).
//   k_finish  one thread per parameter of the stepped net: the workgroups' partials summed in workgroup order, weight
//             decay, RMSprop (torch.optim.RMSprop's order of separately rounded ops) and, on critic steps, the clamp.
// Epoch-end losses = 2 launches:
//   k_eloss         row tiles: G over z_full, D on the fake and the real rows, per-workgroup sums (row order)
//   k_eloss_finish  one workgroup: the partials in a fixed order (float64), the two means
// Inference (pfw_generate / pfw_critic): one launch each, thread = row.
//
// No float atomics anywhere: a call is bitwise reproducible, and pfw_fit_epoch is the same launches as the loop of
// pfw_train_step calls.
#include "../../csrc/rnvp_generic_net.h"
#include "../pf_rowtile.h"

#include <math.h>

#include "pf_wgan.h"

using rnvp::KShape;
using pf_rowtile::big_lds;
using pf_rowtile::kLds;
using pf_rowtile::Plan;

namespace {

constexpr int NT = 256;                   // threads of a k_step workgroup (the parameter sweeps use all of them)
constexpr int FWD_T = 64;                 // rows of an inference / epoch-loss tile (one wave)
constexpr int kFinishT = 256;

// the nets of one shape, as rnvp::KShape (L = 1; KShape::d = leading input columns whose gradient the backward produces)
struct WShape {
    KShape g;         // (latent + c) -> g_hidden.. -> d, no input gradient
    KShape dc;        // (d + c) -> d_hidden.. -> 1, critic step: no input gradient
    KShape dg;        // the same net, generator step: input gradient of the d x columns
    int d, c, lat, PG, PD, wmax;
    int step_unit;    // floats of k_step LDS per LDS row
    int fwd_unit;     // floats of k_eloss LDS per LDS row
};

int make_net(KShape &k, int nin0, const int32_t *hidden, int nh, int act, int nout_last) {
    if (nh < 1 || nh > PFW_MAX_HIDDEN || nin0 < 1 || nout_last < 1) return PFW_EINVAL;
    memset(&k, 0, sizeof(k));
    k.L = 1; k.nh = nh; k.act = act == PFW_ACT_TANH ? RNVP_ACT_TANH : RNVP_ACT_RELU;
    int in = nin0, off = 0;
    k.wmax = in;
    for (int i = 0; i <= nh; ++i) {
        const int out = i < nh ? hidden[i] : nout_last;
        if (out < 1) return PFW_EINVAL;
        k.nin[i] = in; k.nout[i] = out;
        k.woff[i] = off; k.boff[i] = off + out * in;
        off += out * in + out;
        if (i < nh) { k.hs += out; k.hmax = out > k.hmax ? out : k.hmax; }
        k.wmax = out > k.wmax ? out : k.wmax;
        in = out;
    }
    k.npn = off;
    return PFW_OK;
}

int make_wshape(const pfw_shape *s, WShape &w) {
    if (!s || s->d < 1 || s->c < 0 || s->latent < 1) return PFW_EINVAL;
    if (s->g_act != PFW_ACT_TANH && s->g_act != PFW_ACT_RELU) return PFW_EINVAL;
    if (s->d_act != PFW_ACT_TANH && s->d_act != PFW_ACT_RELU) return PFW_EINVAL;
    int st = make_net(w.g, s->latent + s->c, s->g_hidden, s->g_n_hidden, s->g_act, s->d);
    if (st) return st;
    st = make_net(w.dc, s->d + s->c, s->d_hidden, s->d_n_hidden, s->d_act, 1);
    if (st) return st;
    w.g.d = 0; w.g.c = s->latent + s->c;
    w.dg = w.dc;
    w.dc.d = 0; w.dc.c = s->d + s->c;
    w.dg.d = s->d; w.dg.c = s->c;
    w.d = s->d; w.c = s->c; w.lat = s->latent;
    w.PG = w.g.npn; w.PD = w.dc.npn;
    int wm = w.g.hmax > w.dc.hmax ? w.g.hmax : w.dc.hmax;
    w.wmax = wm > s->d ? wm : s->d;
    // k_step: gIn, gActs, dIn, dActs, dOut, bufA, bufB, gx (the x-column gradient, later G's ping-pong buffer)
    w.step_unit = (w.lat + w.c) + w.g.hs + (w.d + w.c) + w.dc.hs + 1 + 3 * w.wmax;
    // k_eloss (ping-pong, no backward): gIn, G's two buffers, dIn, D's two buffers, dOut
    w.fwd_unit = (w.lat + w.c) + 2 * w.g.hmax + (w.d + w.c) + 2 * w.dc.hmax + 1;
    return PFW_OK;
}

// batch rows per k_step workgroup that fit LDS (S = 2R + 1 LDS rows), capped so that 2R <= NT
int step_tile_cap(const WShape &w) {
    const size_t per = (size_t)w.step_unit * sizeof(float);
    const int64_t S = (int64_t)(kLds / per);
    int64_t R = (S - 1) / 2;
    if (R > NT / 2) R = NT / 2;
    return (int)(R < 0 ? 0 : R);
}

// rows of an epoch-loss tile (2T + 1 LDS rows) / of an inference tile (T + 1 LDS rows)
int eloss_tile(const WShape &w) {
    int64_t S = (int64_t)(kLds / ((size_t)w.fwd_unit * sizeof(float)));
    int64_t T = (S - 1) / 2;
    return (int)(T > FWD_T ? FWD_T : (T < 0 ? 0 : T));
}

int gen_unit(const WShape &w) { return (w.lat + w.c) + 2 * w.g.hmax + w.d; }
int crit_unit(const WShape &w) { return (w.d + w.c) + 2 * w.dc.hmax + 1; }

int fwd_tile(int unit) {
    int64_t T = (int64_t)(kLds / ((size_t)unit * sizeof(float))) - 1;
    return (int)(T > FWD_T ? FWD_T : (T < 0 ? 0 : T));
}

// the launches (pf_rowtile::Plan): enqueue_* / pfw_generate / pfw_critic launch from these and pfw_tiling reports them
Plan step_plan(const WShape &w, int64_t rows) {
    return pf_rowtile::make_plan(pf_rowtile::step_tile(step_tile_cap(w), rows), 0, 2, w.step_unit, rows);
}

Plan eloss_plan(const WShape &w, int64_t n) { return pf_rowtile::make_plan(eloss_tile(w), 0, 2, w.fwd_unit, n); }

// pfw_generate (unit = gen_unit) / pfw_critic (unit = crit_unit)
Plan fwd_plan(int unit, int64_t n) { return pf_rowtile::make_plan(fwd_tile(unit), 0, 1, unit, n); }

struct Ws {
    float *gpart;   // [G][PG + PD]
    float *lpart;   // [G]
    float *epart;   // [E][2]
};

size_t ws_bytes(const WShape &w, int64_t batch_rows, int64_t loss_rows, Ws *out, void *base) {
    const int64_t G = batch_rows > 0 ? pf_rowtile::step_wg_bound(step_tile_cap(w), batch_rows) : 0;
    const int T = eloss_tile(w);
    const int64_t E = (loss_rows > 0 && T > 0) ? (loss_rows + T - 1) / T : 0;
    const size_t a = rnvp::align_up((size_t)G * (w.PG + w.PD) * sizeof(float), 256);
    const size_t b = rnvp::align_up((size_t)G * sizeof(float), 256);
    const size_t c = rnvp::align_up((size_t)E * 2 * sizeof(float), 256);
    if (out) {
        char *p = (char *)base;
        out->gpart = (float *)p; out->lpart = (float *)(p + a); out->epart = (float *)(p + a + b);
    }
    return a + b + c;
}

struct Rms {
    float alpha, w1, eps, neg_lr, wd, lo, hi;
    int use_wd, clamp;
};

Rms make_rms(const pfw_rmsprop *o, bool critic) {
    Rms r;
    // the scalars as torch's CPU kernels see them: Python floats rounded to float32 once
    r.alpha = (float)o->alpha;
    r.w1 = (float)(1.0 - o->alpha);
    r.eps = (float)o->eps;
    r.neg_lr = (float)(-o->lr);
    r.wd = (float)o->weight_decay;
    r.use_wd = o->weight_decay != 0.0;
    r.clamp = critic && o->clamp > 0.0;
    r.lo = (float)(-o->clamp); r.hi = (float)o->clamp;
    return r;
}

// net_forward of rnvp_generic_net.h with ocml's tanhf in place of act_fwd's exp2 / rcp form.  That form has an
// ABSOLUTE error of ~1e-7; a clamped critic (every weight in [-0.01, 0.01]) works on activations of ~1e-2, where it is
// a relative error of ~1e-5 -- measured as 6e-5 of max |grad| on the tanh fixture.  tanhf is accurate to ~1 ulp at
// every magnitude, as the reference's torch.tanh is.  ReLU is the same code as net_forward.
__device__ __forceinline__ float act_exact(float v, int act) { return act == RNVP_ACT_TANH ? tanhf(v) : fmaxf(v, 0.f); }

template <bool KEEP>
__device__ void mlp_forward(const float *__restrict__ p, const KShape &s, const float *in, float *buf0, float *buf1,
                            float *out, int TBP, int t) {
    const float *cur = in;
    float *dst = buf0;
    for (int k = 0; k <= s.nh; ++k) {
        const int nin = s.nin[k], nout = s.nout[k];
        const float *__restrict__ Wk = p + s.woff[k];
        const float *__restrict__ b = p + s.boff[k];
        float *ob = (k < s.nh) ? dst : out;
        for (int o = 0; o < nout; o += 4) {
            const int o1 = min(o + 1, nout - 1), o2 = min(o + 2, nout - 1), o3 = min(o + 3, nout - 1);
            const float *w0 = Wk + o * nin, *w1 = Wk + o1 * nin, *w2 = Wk + o2 * nin, *w3 = Wk + o3 * nin;
            float a0 = b[o], a1 = b[o1], a2 = b[o2], a3 = b[o3];
            for (int i = 0; i < nin; ++i) {
                const float v = cur[i * TBP + t];
                a0 = fmaf(v, w0[i], a0);
                a1 = fmaf(v, w1[i], a1);
                a2 = fmaf(v, w2[i], a2);
                a3 = fmaf(v, w3[i], a3);
            }
            if (k < s.nh) {
                a0 = act_exact(a0, s.act); a1 = act_exact(a1, s.act);
                a2 = act_exact(a2, s.act); a3 = act_exact(a3, s.act);
            }
            ob[o * TBP + t] = a0;
            if (o + 1 < nout) ob[(o + 1) * TBP + t] = a1;
            if (o + 2 < nout) ob[(o + 2) * TBP + t] = a2;
            if (o + 3 < nout) ob[(o + 3) * TBP + t] = a3;
        }
        cur = ob;
        if (k < s.nh) {
            if (KEEP) dst += nout * TBP;
            else dst = (dst == buf0) ? buf1 : buf0;
        }
    }
}

// ---- kernels -----------------------------------------------------------------------------------------------------

// stage row t of a tile: G input [z || c] into gIn row t, the condition columns of D's fake row t and (real != nullptr)
// the whole real row into D's row `rrow`
__device__ inline void stage_row(const WShape &w, int S, int t, int64_t brow, int64_t row, const float *z,
                                 const float *x, const float *c, float *gIn, float *dIn, int rrow, bool real) {
    for (int j = 0; j < w.lat; ++j) gIn[j * S + t] = z[brow * w.lat + j];
    for (int j = 0; j < w.c; ++j) {
        const float cv = c[row * w.c + j];
        gIn[(w.lat + j) * S + t] = cv;
        dIn[(w.d + j) * S + t] = cv;
        if (real) dIn[(w.d + j) * S + rrow] = cv;
    }
    if (real)
        for (int j = 0; j < w.d; ++j) dIn[j * S + rrow] = x[row * w.d + j];
}

__global__ __launch_bounds__(NT) void k_step(WShape w, int critic, int R, const float *__restrict__ params,
                                             const float *__restrict__ x, const float *__restrict__ c,
                                             const int64_t *__restrict__ row_index, const float *__restrict__ z,
                                             int64_t rows, float inv_B, float *__restrict__ gpart,
                                             float *__restrict__ lpart) {
    extern __shared__ float lds[];
    const int t = threadIdx.x;
    const int S = 2 * R + 1;
    const int64_t r0 = (int64_t)blockIdx.x * R;
    const int TB = (int)(rows - r0 < R ? rows - r0 : R);
    const int TBD = critic ? 2 * TB : TB;
    float *gIn = lds;
    float *gActs = gIn + (w.lat + w.c) * S;
    float *dIn = gActs + w.g.hs * S;
    float *dActs = dIn + (w.d + w.c) * S;
    float *dOut = dActs + w.dc.hs * S;
    float *bufA = dOut + S;
    float *bufB = bufA + w.wmax * S;
    float *gx = bufB + w.wmax * S;
    const float *pG = params, *pD = params + w.PG;
    float *gp = gpart + (int64_t)blockIdx.x * (w.PG + w.PD);

    if (t < TB) {
        const int64_t brow = r0 + t;
        const int64_t row = row_index ? row_index[brow] : brow;
        stage_row(w, S, t, brow, row, z, x, c, gIn, dIn, TB + t, critic != 0);
        mlp_forward<true>(pG, w.g, gIn, gActs, nullptr, dIn, S, t);     // fake -> D's rows 0..TB-1
    }
    __syncthreads();
    if (t < TBD) {
        mlp_forward<true>(pD, w.dc, dIn, dActs, nullptr, dOut, S, t);
        bufA[t] = (critic && t >= TB) ? -inv_B : (critic ? inv_B : -inv_B);    // d loss / d D(row)
        if (!critic)
            for (int j = 0; j < w.d; ++j) gx[j * S + t] = 0.f;
    }
    __syncthreads();
    // D backward: parameter gradient (critic steps: the partial that counts; generator steps: unused) and, on generator
    // steps, d loss / d fake into gx
    rnvp::net_backward(pD, gp + w.PG, critic ? w.dc : w.dg, dIn, dActs, bufA, bufB, gx, TBD, S, t, NT, true);
    if (!critic)   // G backward seeded with gx (it serves as G's gradient ping-pong buffer; G needs no input gradient)
        rnvp::net_backward(pG, gp, w.g, gIn, gActs, gx, bufB, bufA, TB, S, t, NT, true);
    if (t == 0) {
        float a = 0.f;
        for (int r = 0; r < TBD; ++r) a += (critic && r >= TB) ? -dOut[r] : (critic ? dOut[r] : -dOut[r]);
        lpart[blockIdx.x] = a;
    }
}

__global__ __launch_bounds__(kFinishT) void k_finish(int off, int P, int stride, int G, const float *__restrict__ gpart,
                                                     const float *__restrict__ lpart, float B, float *params, float *sq,
                                                     float *grad_out, float *loss_out, Rms r, int update) {
    const int64_t i = (int64_t)blockIdx.x * kFinishT + threadIdx.x;
    if (i < P) {
        float g = 0.f;
        for (int k = 0; k < G; ++k) g += gpart[(int64_t)k * stride + off + i];
        if (grad_out) grad_out[i] = g;
        if (update) {
            float p = params[off + i], v = sq[off + i];
            if (r.use_wd) g = rnvp::add_rn(g, rnvp::mul_rn(r.wd, p));                          // grad.add(param, alpha=wd)
            v = rnvp::add_rn(rnvp::mul_rn(v, r.alpha), rnvp::mul_rn(rnvp::mul_rn(r.w1, g), g));  // mul_(a).addcmul_(g, g, 1-a)
            const float avg = rnvp::add_rn(sqrtf(v), r.eps);                                   // sqrt().add_(eps)
            p = rnvp::add_rn(p, rnvp::mul_rn(r.neg_lr, g / avg));                               // addcdiv_(g, avg, -lr)
            if (r.clamp) p = fminf(fmaxf(p, r.lo), r.hi);                                       // clamp_(-0.01, 0.01)
            params[off + i] = p;
            sq[off + i] = v;
        }
    }
    if (loss_out && blockIdx.x == 0 && threadIdx.x == 0) {
        float a = 0.f;
        for (int k = 0; k < G; ++k) a += lpart[k];
        loss_out[0] = a / B;
    }
}

__global__ __launch_bounds__(2 * FWD_T) void k_eloss(WShape w, int T, const float *__restrict__ params,
                                                     const float *__restrict__ x, const float *__restrict__ c,
                                                     const float *__restrict__ z, int64_t n, float *__restrict__ epart) {
    extern __shared__ float lds[];
    const int t = threadIdx.x;
    const int S = 2 * T + 1;
    const int64_t r0 = (int64_t)blockIdx.x * T;
    const int TB = (int)(n - r0 < T ? n - r0 : T);
    float *gIn = lds;
    float *g0 = gIn + (w.lat + w.c) * S, *g1 = g0 + w.g.hmax * S;
    float *dIn = g1 + w.g.hmax * S;
    float *d0 = dIn + (w.d + w.c) * S, *d1 = d0 + w.dc.hmax * S;
    float *dOut = d1 + w.dc.hmax * S;
    if (t < TB) {
        const int64_t row = r0 + t;
        stage_row(w, S, t, row, row, z, x, c, gIn, dIn, TB + t, true);
        mlp_forward<false>(params, w.g, gIn, g0, g1, dIn, S, t);
    }
    __syncthreads();
    if (t < 2 * TB) mlp_forward<false>(params + w.PG, w.dc, dIn, d0, d1, dOut, S, t);
    __syncthreads();
    if (t == 0) {
        float f = 0.f, r = 0.f;
        for (int k = 0; k < TB; ++k) f += dOut[k];
        for (int k = 0; k < TB; ++k) r += dOut[TB + k];
        epart[2 * blockIdx.x] = f;
        epart[2 * blockIdx.x + 1] = r;
    }
}

__global__ __launch_bounds__(kFinishT) void k_eloss_finish(const float *__restrict__ epart, int64_t E, int64_t n,
                                                           float *out) {
    __shared__ double sf[kFinishT], sr[kFinishT];
    const int t = threadIdx.x;
    double f = 0.0, r = 0.0;
    for (int64_t k = t; k < E; k += kFinishT) { f += epart[2 * k]; r += epart[2 * k + 1]; }
    sf[t] = f; sr[t] = r;
    __syncthreads();
    if (t == 0) {
        double F = 0.0, Rr = 0.0;
        for (int k = 0; k < kFinishT; ++k) { F += sf[k]; Rr += sr[k]; }
        const float gen = -(float)(F / (double)n);
        const float real = (float)(Rr / (double)n);
        out[0] = gen;              // gen_loss_epoch  = -mean D(fake)
        out[1] = real + gen;       // disc_loss_epoch = mean D(real) + gen_loss_epoch
    }
}

// inference: thread = row, ping-pong buffers; G writes [n, d], D writes [n]
__global__ __launch_bounds__(FWD_T) void k_generate(WShape w, int T, const float *__restrict__ params,
                                                    const float *__restrict__ z, const float *__restrict__ c, int64_t n,
                                                    float *__restrict__ out) {
    extern __shared__ float lds[];
    const int t = threadIdx.x, S = T + 1;
    const int64_t row = (int64_t)blockIdx.x * T + t;
    float *in = lds, *b0 = in + (w.lat + w.c) * S, *b1 = b0 + w.g.hmax * S, *o = b1 + w.g.hmax * S;
    if (t >= T || row >= n) return;   // no barriers below
    for (int j = 0; j < w.lat; ++j) in[j * S + t] = z[row * w.lat + j];
    for (int j = 0; j < w.c; ++j) in[(w.lat + j) * S + t] = c[row * w.c + j];
    mlp_forward<false>(params, w.g, in, b0, b1, o, S, t);
    for (int j = 0; j < w.d; ++j) out[row * w.d + j] = o[j * S + t];
}

__global__ __launch_bounds__(FWD_T) void k_critic(WShape w, int T, const float *__restrict__ params,
                                                  const float *__restrict__ x, const float *__restrict__ c, int64_t n,
                                                  float *__restrict__ out) {
    extern __shared__ float lds[];
    const int t = threadIdx.x, S = T + 1;
    const int64_t row = (int64_t)blockIdx.x * T + t;
    float *in = lds, *b0 = in + (w.d + w.c) * S, *b1 = b0 + w.dc.hmax * S, *o = b1 + w.dc.hmax * S;
    if (t >= T || row >= n) return;
    for (int j = 0; j < w.d; ++j) in[j * S + t] = x[row * w.d + j];
    for (int j = 0; j < w.c; ++j) in[(w.d + j) * S + t] = c[row * w.c + j];
    mlp_forward<false>(params + w.PG, w.dc, in, b0, b1, o, S, t);
    out[row] = o[t];
}

std::atomic<uint64_t> g_lds_step{0}, g_lds_eloss{0}, g_lds_gen{0}, g_lds_crit{0};

int enqueue_step(hipStream_t st, const WShape &w, int kind, float *params, float *sq, const float *x, const float *c,
                 const int64_t *ri, const float *z, int64_t rows, const Rms *rms, float *grad_out, float *loss_out,
                 const Ws &ws) {
    const Plan pl = step_plan(w, rows);
    const int R = pl.tile;
    const int64_t G = pl.wgs;
    const size_t lds = pl.lds;
    const bool critic = kind == PFW_STEP_CRITIC;
    if (int e = big_lds(k_step, lds, g_lds_step)) return e;
    hipLaunchKernelGGL(k_step, dim3((unsigned)G), dim3(NT), lds, st, w, critic ? 1 : 0, R, params, x, c, ri, z, rows,
                       1.0f / (float)rows, ws.gpart, ws.lpart);
    RNVP_HIP_TRY(hipGetLastError());
    const int off = critic ? w.PG : 0, P = critic ? w.PD : w.PG;
    Rms r = rms ? *rms : Rms{};
    hipLaunchKernelGGL(k_finish, dim3((unsigned)((P + kFinishT - 1) / kFinishT)), dim3(kFinishT), 0, st, off, P,
                       w.PG + w.PD, (int)G, ws.gpart, ws.lpart, (float)rows, params, sq, grad_out, loss_out, r,
                       rms ? 1 : 0);
    RNVP_HIP_TRY(hipGetLastError());
    return PFW_OK;
}

int enqueue_eloss(hipStream_t st, const WShape &w, const float *params, const float *x, const float *c, const float *z,
                  int64_t n, float *out, const Ws &ws) {
    const Plan pl = eloss_plan(w, n);
    const int T = pl.tile;
    const size_t lds = pl.lds;
    const int64_t E = pl.wgs;
    if (int e = big_lds(k_eloss, lds, g_lds_eloss)) return e;
    hipLaunchKernelGGL(k_eloss, dim3((unsigned)E), dim3(2 * FWD_T), lds, st, w, T, params, x, c, z, n, ws.epart);
    RNVP_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_eloss_finish, dim3(1), dim3(kFinishT), 0, st, ws.epart, E, n, out);
    RNVP_HIP_TRY(hipGetLastError());
    return PFW_OK;
}

int check_train(const WShape &w, int64_t batch_rows, int64_t loss_rows, void *ws, size_t wsb, Ws &out) {
    if (step_tile_cap(w) < 1 || (loss_rows > 0 && eloss_tile(w) < 1)) return PFW_EUNSUPPORTED;
    if (!ws || wsb < ws_bytes(w, batch_rows, loss_rows, &out, ws)) return PFW_EWORKSPACE;
    return PFW_OK;
}

}  // namespace

extern "C" {

int pfw_version(void) { return PFW_VERSION; }

const char *pfw_status_string(int status) {
    switch (status) {
    case PFW_OK: return "ok";
    case PFW_EINVAL: return "invalid argument";
    case PFW_EUNSUPPORTED: return "shape unsupported: one row of the networks does not fit the 160 KiB of LDS";
    case PFW_EWORKSPACE: return "workspace too small";
    default: return status > 0 ? hipGetErrorString((hipError_t)status) : "unknown status";
    }
}

int64_t pfw_param_count(const pfw_shape *s, int net) {
    WShape w;
    if (make_wshape(s, w)) return -1;
    return net == PFW_NET_G ? w.PG : (net == PFW_NET_D ? w.PD : -1);
}

size_t pfw_workspace_bytes(const pfw_shape *s, int64_t batch_rows, int64_t loss_rows) {
    WShape w;
    if (make_wshape(s, w) || batch_rows < 0 || loss_rows < 0) return 0;
    return ws_bytes(w, batch_rows, loss_rows, nullptr, nullptr);
}

int pfw_tiling(const pfw_shape *s, int64_t rows, pfw_tiling_info *out) {
    WShape w;
    if (int e = make_wshape(s, w)) return e;
    if (!out || rows < 1) return PFW_EINVAL;
    memset(out, 0, sizeof(*out));
    const Plan el = eloss_plan(w, rows), ge = fwd_plan(gen_unit(w), rows), cr = fwd_plan(crit_unit(w), rows);
    out->eloss_tile = el.tile; out->eloss_lds_bytes = (int64_t)el.lds;
    out->gen_tile = ge.tile; out->gen_lds_bytes = (int64_t)ge.lds;
    out->crit_tile = cr.tile; out->crit_lds_bytes = (int64_t)cr.lds;
    out->step_cap = step_tile_cap(w);
    if (out->step_cap < 1) return PFW_EUNSUPPORTED;
    const Plan st = step_plan(w, rows);
    out->step_tile = st.tile; out->step_wgs = st.wgs; out->step_lds_bytes = (int64_t)st.lds;
    out->step_wg_bound = pf_rowtile::step_wg_bound(out->step_cap, rows);
    return PFW_OK;
}

int pfw_generate(void *stream, const pfw_shape *s, const float *params, const float *z, const float *c, int64_t n,
                 float *out) {
    WShape w;
    if (int e = make_wshape(s, w)) return e;
    if (!params || !z || !out || n < 1 || (w.c > 0 && !c)) return PFW_EINVAL;
    const Plan pl = fwd_plan(gen_unit(w), n);
    const int T = pl.tile;
    if (T < 1) return PFW_EUNSUPPORTED;
    const size_t lds = pl.lds;
    if (int e = big_lds(k_generate, lds, g_lds_gen)) return e;
    hipLaunchKernelGGL(k_generate, dim3((unsigned)pl.wgs), dim3(FWD_T), lds, (hipStream_t)stream, w, T, params,
                       z, c, n, out);
    RNVP_HIP_TRY(hipGetLastError());
    return PFW_OK;
}

int pfw_critic(void *stream, const pfw_shape *s, const float *params, const float *x, const float *c, int64_t n,
               float *out) {
    WShape w;
    if (int e = make_wshape(s, w)) return e;
    if (!params || !x || !out || n < 1 || (w.c > 0 && !c)) return PFW_EINVAL;
    const Plan pl = fwd_plan(crit_unit(w), n);
    const int T = pl.tile;
    if (T < 1) return PFW_EUNSUPPORTED;
    const size_t lds = pl.lds;
    if (int e = big_lds(k_critic, lds, g_lds_crit)) return e;
    hipLaunchKernelGGL(k_critic, dim3((unsigned)pl.wgs), dim3(FWD_T), lds, (hipStream_t)stream, w, T, params,
                       x, c, n, out);
    RNVP_HIP_TRY(hipGetLastError());
    return PFW_OK;
}

int pfw_loss_grad(void *stream, const pfw_shape *s, int kind, const float *params, const float *x, const float *c,
                  const int64_t *row_index, const float *z, int64_t rows, float *grad_out, float *loss_out,
                  void *workspace, size_t workspace_bytes) {
    WShape w;
    if (int e = make_wshape(s, w)) return e;
    if ((kind != PFW_STEP_GEN && kind != PFW_STEP_CRITIC) || !params || !x || !z || rows < 1 || (w.c > 0 && !c))
        return PFW_EINVAL;
    Ws ws;
    if (int e = check_train(w, rows, 0, workspace, workspace_bytes, ws)) return e;
    return enqueue_step((hipStream_t)stream, w, kind, const_cast<float *>(params), nullptr, x, c, row_index, z, rows,
                        nullptr, grad_out, loss_out, ws);
}

int pfw_train_step(void *stream, const pfw_shape *s, int kind, float *params, float *square_avg, const float *x,
                   const float *c, const int64_t *row_index, const float *z, int64_t rows, const pfw_rmsprop *opt,
                   float *grad_out, float *loss_out, void *workspace, size_t workspace_bytes) {
    WShape w;
    if (int e = make_wshape(s, w)) return e;
    if ((kind != PFW_STEP_GEN && kind != PFW_STEP_CRITIC) || !params || !square_avg || !x || !z || !opt || rows < 1 ||
        (w.c > 0 && !c))
        return PFW_EINVAL;
    Ws ws;
    if (int e = check_train(w, rows, 0, workspace, workspace_bytes, ws)) return e;
    const Rms r = make_rms(opt, kind == PFW_STEP_CRITIC);
    return enqueue_step((hipStream_t)stream, w, kind, params, square_avg, x, c, row_index, z, rows, &r, grad_out,
                        loss_out, ws);
}

int pfw_epoch_losses(void *stream, const pfw_shape *s, const float *params, const float *x, const float *c,
                     const float *z_full, int64_t n, float *epoch_losses, void *workspace, size_t workspace_bytes) {
    WShape w;
    if (int e = make_wshape(s, w)) return e;
    if (!params || !x || !z_full || !epoch_losses || n < 1 || (w.c > 0 && !c)) return PFW_EINVAL;
    Ws ws;
    if (int e = check_train(w, 0, n, workspace, workspace_bytes, ws)) return e;
    return enqueue_eloss((hipStream_t)stream, w, params, x, c, z_full, n, epoch_losses, ws);
}

int pfw_fit_epoch(void *stream, const pfw_shape *s, float *params, float *square_avg, const float *x, const float *c,
                  const int64_t *perm, const float *z_batches, const float *z_full, int64_t n, int64_t batch_size,
                  const int8_t *kinds_host, const pfw_rmsprop *opt, float *epoch_losses, void *workspace,
                  size_t workspace_bytes) {
    WShape w;
    if (int e = make_wshape(s, w)) return e;
    if (!params || !square_avg || !x || !perm || !z_batches || !kinds_host || !opt || n < 1 || batch_size < 1 ||
        (w.c > 0 && !c) || (z_full && !epoch_losses))
        return PFW_EINVAL;
    const int64_t B = batch_size < n ? batch_size : n;
    Ws ws;
    if (int e = check_train(w, B, z_full ? n : 0, workspace, workspace_bytes, ws)) return e;
    const int64_t nb = (n + batch_size - 1) / batch_size;
    for (int64_t b = 0; b < nb; ++b)
        if (kinds_host[b] != PFW_STEP_GEN && kinds_host[b] != PFW_STEP_CRITIC) return PFW_EINVAL;
    const Rms rc = make_rms(opt, true), rg = make_rms(opt, false);
    hipStream_t st = (hipStream_t)stream;
    for (int64_t b = 0; b < nb; ++b) {
        const int64_t s0 = b * batch_size, rows = (n - s0 < batch_size) ? n - s0 : batch_size;
        const int kind = kinds_host[b];
        if (int e = enqueue_step(st, w, kind, params, square_avg, x, c, perm + s0, z_batches + s0 * w.lat, rows,
                                 kind == PFW_STEP_CRITIC ? &rc : &rg, nullptr, nullptr, ws))
            return e;
    }
    if (z_full) return enqueue_eloss(st, w, params, x, c, z_full, n, epoch_losses, ws);
    return PFW_OK;
}

}  // extern "C"
