// pf_gendraw.hip -- libpf_gendraw.so (C ABI: pf_gendraw.h): K draws per condition row of an MLP generator (CVAE's
// Decoder, ConditionalWGAN's Generator) or of ConditionalNormal's affine map, reduced across the draws on the device
// (gfx950) into the running-moment state of pf_predict.h.
//
// k_mlp_draw: a workgroup of PFG_WAVES = 4 waves; every WAVE owns one condition row at a time (row = 4 * workgroup + wave,
// then a grid stride), so every (row, column) of `state` has exactly one owner, nothing is summed with atomics and,
// after the one barrier behind the weight staging, no wave ever waits for another: inside the row loop a wave
// synchronises only with itself.
//   * k_pack writes the parameters at the head of every call into the workspace in MFMA fragment order: per Linear
//     [out tile m][group of 4 k-steps][lane][k-step in group], zero where the out row or the k column does not exist,
//     then the biases of every Linear but the first.  A lane's A operands of four k-steps are ONE 16-byte load.
//   * the four waves share one copy of that blob in LDS when it fits beside their four activation images
//     (weights_in_lds); otherwise every wave reads the same fragments from the workspace (L2).
//   * the 16 columns of an MFMA tile are 16 DRAWS of the wave's row, NT = 1, 2 or 4 tiles per pass; every Linear is
//     out^T[out x draws] = W . act^T as v_mfma_f32_16x16x4_f32, B = the LDS image [feature][RS] of the previous Linear.
//   * the row's condition enters through the first Linear only and is the same for all K draws: cb = b0 + W0[:, latent:] . c[r]
//     is formed once per row and used as that Linear's bias; its contraction runs over the `latent` z columns alone.
//   * B operands of a k column at or past the Linear's input width are forced to zero (the image row there is stale),
//     A operands there and in out rows past the width are zeros of the pack.
// A draw's value depends on its own image column only, in a k order fixed by the shape; the fold order is fixed by
// (k_lo, k_cnt) alone.
#include "../../csrc/rnvp_common.h"
#include "pf_gendraw.h"
#include "../predict_csrc/pf_drawfold.h"

#include <math.h>

namespace {

using namespace drawfold;          // State, f4, mfma16, min_nan / max_nan, row_stride, load_state, emit_fold, store_state

constexpr int kW = PFG_WAVES;
constexpr int kThreads = 64 * kW;
constexpr int kLdsWide = 80 * 1024;        // a pass of more than 16 draws only while two workgroups still fit a CU
constexpr int kMaxLin = PFG_MAX_HIDDEN + 1;

// the net as the kernels see it; offsets in floats
struct Net {
    int nlin, n_out, c, latent, act, hmax;
    int nin[kMaxLin], nout[kMaxLin];       // nin[0] = latent: the first Linear contracts over the z columns only
    int ldw[kMaxLin];                      // row stride of W_k in params (latent + c for k = 0)
    int woff[kMaxLin], boff[kMaxLin];      // in params
    int MT[kMaxLin], KS[kMaxLin], KG[kMaxLin];
    int foff[kMaxLin];                     // fragments of Linear k in the packed blob
    int pboff[kMaxLin];                    // bias of Linear k >= 1 in the packed blob
    int packed_floats;                     // a multiple of 4
};

// one workgroup's LDS in floats: [packed blob when resident][image of wave 0] .. [image of wave 3]; the o* are offsets
// inside a wave's image
struct Geo {
    int RS, resident, oImg, img, oZ, oA, oB, oCB, oST, floats;
};

int make_net(const pfg_mlp *m, Net *n) {
    if (!m) return PFG_EINVAL;
    if (m->n_out < 1 || m->c < 0 || m->latent < 1 || m->n_hidden < 1 || m->n_hidden > PFG_MAX_HIDDEN) return PFG_EINVAL;
    if (m->act != RNVP_ACT_TANH && m->act != RNVP_ACT_RELU) return PFG_EINVAL;
    if (m->n_out > (1 << 20) || m->c > (1 << 20) || m->latent > (1 << 20)) return PFG_EINVAL;
    *n = Net{};
    n->nlin = m->n_hidden + 1; n->n_out = m->n_out; n->c = m->c; n->latent = m->latent; n->act = m->act;
    int64_t po = 0, fo = 0;
    int prev = m->latent + m->c;
    for (int k = 0; k < n->nlin; ++k) {
        const int out = k < m->n_hidden ? m->hidden[k] : m->n_out;
        if (out < 1 || out > (1 << 20)) return PFG_EINVAL;
        n->ldw[k] = prev;
        n->nin[k] = k == 0 ? m->latent : prev;
        n->nout[k] = out;
        if (po + (int64_t)prev * out + out > (int64_t)1 << 30) return PFG_EINVAL;
        n->woff[k] = (int)po; po += (int64_t)prev * out;
        n->boff[k] = (int)po; po += out;
        n->MT[k] = (out + 15) / 16;
        n->KS[k] = (n->nin[k] + 3) / 4;
        n->KG[k] = (n->KS[k] + 3) / 4;
        n->foff[k] = (int)fo;
        fo += (int64_t)n->MT[k] * n->KG[k] * 256;
        if (fo > (int64_t)1 << 29) return PFG_EINVAL;
        if (k < m->n_hidden && out > n->hmax) n->hmax = out;
        prev = out;
    }
    for (int k = 1; k < n->nlin; ++k) {
        n->pboff[k] = (int)fo;
        fo += (n->nout[k] + 3) / 4 * 4;
    }
    n->packed_floats = (int)fo;
    return PFG_OK;
}

// The LDS budget.  One wave's image: z [latent up to 4][RS], two ping-pong buffers [max(hmax, n_out) up to 4][RS] (a Linear
// reads one and writes the other; the last one's output is what the fold reads), cb [hidden[0]], the row's state.
int64_t image_floats(const Net &n, int RS, Geo *g) {
    const int lp = (n.latent + 3) / 4 * 4;
    const int rows = ((n.hmax > n.n_out ? n.hmax : n.n_out) + 3) / 4 * 4;
    int64_t o = 0;
    g->oZ = (int)o;  o += (int64_t)lp * RS;
    g->oA = (int)o;  o += (int64_t)rows * RS;
    g->oB = (int)o;  o += (int64_t)rows * RS;
    g->oCB = (int)o; o += n.nout[0];
    o = (o + 3) / 4 * 4;
    g->oST = (int)o; o += (int64_t)n.n_out * kStateFloats;
    return (o + 3) / 4 * 4;
}

// The draws per pass (NT tiles of 16), whether the packed weights are staged in LDS, and the geometry; 0 when not even one
// tile per wave fits.  The weights in LDS come first: a narrower pass with resident weights before a wider one without.
int pick_plan(const Net &n, int64_t k_cnt, Geo *g) {
    const int want = k_cnt > 32 ? 4 : (k_cnt > 16 ? 2 : 1);
    for (int resident = 1; resident >= 0; --resident) {
        for (int nt = want; nt >= 1; nt >>= 1) {
            Geo t{};
            t.RS = row_stride(nt);
            t.resident = resident;
            const int64_t img = image_floats(n, t.RS, &t);
            const int64_t total = (resident ? (int64_t)n.packed_floats : 0) + kW * img;
            if (total * 4 > (nt > 1 ? kLdsWide : kLdsLimit)) continue;
            t.oImg = resident ? n.packed_floats : 0;
            t.img = (int)img;
            t.floats = (int)total;
            *g = t;
            return nt;
        }
    }
    return 0;
}

// as pf_wgan.hip's act_exact: what the models' own sample computes
__device__ __forceinline__ float act_exact(float v, int act) { return act == RNVP_ACT_TANH ? tanhf(v) : fmaxf(v, 0.f); }

// the lanes of ONE wave agree on what they wrote to LDS (the LDS serves a wave's accesses in order)
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__global__ void __launch_bounds__(256)
k_pack(Net n, const float *__restrict__ params, float *__restrict__ packed) {
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < n.packed_floats; t += gridDim.x * blockDim.x) {
        float v = 0.f;
        for (int k = 0; k < n.nlin; ++k) {
            const int per = n.KG[k] * 256, fl = n.MT[k] * per;
            if (t >= n.foff[k] && t < n.foff[k] + fl) {
                const int idx = t - n.foff[k];
                const int m = idx / per, rem = idx - m * per;
                const int g = rem >> 8, lane = (rem & 255) >> 2, u = rem & 3;
                const int row = 16 * m + (lane & 15), col = 4 * (4 * g + u) + (lane >> 4);
                if (row < n.nout[k] && col < n.nin[k]) v = params[n.woff[k] + (size_t)row * n.ldw[k] + col];
                break;
            }
            if (k >= 1 && t >= n.pboff[k] && t < n.pboff[k] + n.nout[k]) {
                v = params[n.boff[k] + (t - n.pboff[k])];
                break;
            }
        }
        packed[t] = v;
    }
}

// out^T[nout x 16 NT draws] = act(W . in^T + bias) for one wave.  frag: the Linear's packed fragments (LDS or workspace),
// bias: nout floats, in / out: the wave's LDS images [feature][RS].  act < 0: none.
template <int NT>
__device__ __forceinline__ void linear(const float *frag, int MT, int KS, int KG, int nin, int nout, const float *bias,
                                       const float *in, float *out, int RS, int act, int lane) {
    const int q = lane >> 4, r = lane & 15;
    for (int m = 0; m < MT; ++m) {
        f4 acc[NT];
        {
            f4 b0;
#pragma unroll
            for (int e = 0; e < 4; ++e) { const int o = 16 * m + 4 * q + e; b0[e] = o < nout ? bias[o] : 0.f; }
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[t] = b0;
        }
        const float *fa = frag + ((size_t)m * KG * 64 + lane) * 4;
        for (int g = 0; g < KG; ++g) {
            const f4 a = *reinterpret_cast<const f4 *>(fa + (size_t)g * 256);
            float b[4][NT];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int k = 4 * (4 * g + u) + q;
                const bool ok = k < nin;
                const float *ip = in + (ok ? k : 0) * RS + r;
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    const float bv = ip[16 * t];
                    b[u][t] = ok ? bv : 0.f;
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (4 * g + u < KS) {
#pragma unroll
                    for (int t = 0; t < NT; ++t) acc[t] = mfma16(a[u], b[u][t], acc[t]);
                }
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int o = 16 * m + 4 * q + e;
            if (o < nout) {
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    float v = acc[t][e];
                    if (act >= 0) v = act_exact(v, act);
                    out[o * RS + 16 * t + r] = v;
                }
            }
        }
    }
}

template <int NT, bool RESIDENT>
__global__ void __launch_bounds__(kThreads)
k_mlp_draw(Net n, Geo g, const float *__restrict__ params, const float *__restrict__ packed, const float *__restrict__ c,
           int64_t n_rows, int64_t row_offset, const float *__restrict__ z, int64_t n_total, int64_t k_lo, int64_t k_cnt,
           int64_t k_total, State *state, float *x_out, float *xt_out) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int NC = 16 * NT;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, RS = g.RS, d = n.n_out, lat = n.latent, h0 = n.nout[0];
    if (RESIDENT) {
        const f4 *src = reinterpret_cast<const f4 *>(packed);
        f4 *dst = reinterpret_cast<f4 *>(lds);
        for (int e = tid; e < n.packed_floats / 4; e += kThreads) dst[e] = src[e];
    }
    float *img = lds + g.oImg + wave * g.img;
    for (int e = lane; e < g.img; e += 64) img[e] = 0.f;
    __syncthreads();                                   // the only workgroup barrier: the staged weights
    const float *wts = RESIDENT ? lds : packed;
    float *Z = img + g.oZ, *A = img + g.oA, *B = img + g.oB, *CB = img + g.oCB;
    State *ST = reinterpret_cast<State *>(img + g.oST);
    for (int64_t row = (int64_t)blockIdx.x * kW + wave; row < n_rows; row += (int64_t)gridDim.x * kW) {
        const int64_t grow = row_offset + row;
        // the condition's share of the first Linear, once per row
        for (int o = lane; o < h0; o += 64) {
            const float *w = params + n.woff[0] + (size_t)o * n.ldw[0] + lat;
            float a = params[n.boff[0] + o];
            for (int i = 0; i < n.c; ++i) a = fmaf(w[i], c[row * n.c + i], a);
            CB[o] = a;
        }
        load_state(ST, state, row, d, lane);
        wave_sync();
        for (int64_t k0 = 0; k0 < k_cnt; k0 += NC) {
            const int ncols = (int)(k_cnt - k0 < NC ? k_cnt - k0 : NC);
            for (int e = lane; e < NC * lat; e += 64) {
                const int col = e / lat, j = e - col * lat;
                Z[j * RS + col] = col < ncols ? z[((k0 + col) * n_total + grow) * lat + j] : 0.f;
            }
            wave_sync();
            const float *cur = Z;
            float *dst = A;
            for (int k = 0; k < n.nlin; ++k) {
                const bool last = k == n.nlin - 1;
                linear<NT>(wts + n.foff[k], n.MT[k], n.KS[k], n.KG[k], n.nin[k], n.nout[k], k == 0 ? CB : wts + n.pboff[k],
                           cur, dst, RS, last ? -1 : n.act, lane);
                wave_sync();
                cur = dst;
                dst = dst == A ? B : A;
            }
            emit_fold<NT>(cur, RS, d, ncols, row, n_rows, k0, k_lo, k_total, ST, state != nullptr, x_out, xt_out, lane);
            wave_sync();
        }
        store_state(state, ST, row, d, lane);
        wave_sync();
    }
}

// ConditionalNormal: one wave per row at a time, 16 draws per pass.  out (d x d, d <= 32) is staged once per workgroup;
// mu and sigma of the wave's row sit in LDS; y = mu + eps * sigma is rounded twice, then one fmaf chain per output, as
// pf_cnormal.hip's k_forward.
constexpr int kARS = 17;
__global__ void __launch_bounds__(kThreads)
k_affine_draw(int d, const float *__restrict__ mu, const float *__restrict__ sigma, const float *__restrict__ out_w,
              const float *__restrict__ out_b, const float *__restrict__ eps, int64_t n_rows, int64_t row_offset,
              int64_t n_total, int64_t k_lo, int64_t k_cnt, int64_t k_total, State *state, float *x_out, float *xt_out) {
    __shared__ __attribute__((aligned(16))) float sW[PFG_MAX_D * PFG_MAX_D + PFG_MAX_D];
    __shared__ __attribute__((aligned(16))) float sMS[kW][2 * PFG_MAX_D];
    __shared__ __attribute__((aligned(16))) float sY[kW][PFG_MAX_D * kARS];
    __shared__ __attribute__((aligned(16))) float sX[kW][PFG_MAX_D * kARS];
    __shared__ __attribute__((aligned(16))) State sST[kW][PFG_MAX_D];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, q = lane >> 4, r = lane & 15;
    float *Wo = sW, *bo = sW + PFG_MAX_D * PFG_MAX_D;
    if (out_w) {
        for (int e = tid; e < d * d; e += kThreads) Wo[e] = out_w[e];
        for (int e = tid; e < d; e += kThreads) bo[e] = out_b[e];
    }
    for (int e = lane; e < PFG_MAX_D * kARS; e += 64) { sY[wave][e] = 0.f; sX[wave][e] = 0.f; }
    __syncthreads();                                   // the only workgroup barrier
    float *M = sMS[wave], *S = sMS[wave] + PFG_MAX_D, *Y = sY[wave], *X = sX[wave];
    State *ST = sST[wave];
    for (int64_t row = (int64_t)blockIdx.x * kW + wave; row < n_rows; row += (int64_t)gridDim.x * kW) {
        const int64_t grow = row_offset + row;
        for (int j = lane; j < d; j += 64) { M[j] = mu[row * d + j]; S[j] = sigma[row * d + j]; }
        load_state(ST, state, row, d, lane);
        wave_sync();
        for (int64_t k0 = 0; k0 < k_cnt; k0 += 16) {
            const int ncols = (int)(k_cnt - k0 < 16 ? k_cnt - k0 : 16);
            float *yb = out_w ? Y : X;
            for (int e = lane; e < 16 * d; e += 64) {
                const int col = e / d, j = e - col * d;
                float v = 0.f;
                if (col < ncols) {
                    const float p = eps[((k0 + col) * n_total + grow) * d + j] * S[j];
                    v = M[j] + p;
                }
                yb[j * kARS + col] = v;
            }
            wave_sync();
            if (out_w) {
                for (int jj = 0; jj < d; jj += 4) {
                    const int j = jj + q;
                    if (j < d) {
                        float a = bo[j];
                        for (int k = 0; k < d; ++k) a = fmaf(Y[k * kARS + r], Wo[j * d + k], a);
                        X[j * kARS + r] = a;
                    }
                }
                wave_sync();
            }
            emit_fold<1>(X, kARS, d, ncols, row, n_rows, k0, k_lo, k_total, ST, state != nullptr, x_out, xt_out, lane);
            wave_sync();
        }
        store_state(state, ST, row, d, lane);
        wave_sync();
    }
}

std::atomic<uint64_t> g_big[6];

template <int NT, bool RESIDENT>
int launch_mlp(hipStream_t st, const Net &n, const Geo &g, int grid, const float *params, const float *packed, const float *c,
               int64_t n_rows, int64_t row_offset, const float *z, int64_t n_total, int64_t k_lo, int64_t k_cnt, int64_t k_total,
               State *state, float *x_out, float *xt_out) {
    constexpr int slot = (NT == 4 ? 2 : NT - 1) * 2 + (RESIDENT ? 1 : 0);
    const size_t lds = (size_t)g.floats * sizeof(float);
    if (lds > 48 * 1024) {
        const int e = rnvp::allow_big_lds(reinterpret_cast<const void *>(&k_mlp_draw<NT, RESIDENT>), (int)lds, g_big[slot]);
        if (e != RNVP_OK) return e;
    }
    hipLaunchKernelGGL((k_mlp_draw<NT, RESIDENT>), dim3(grid), dim3(kThreads), lds, st, n, g, params, packed, c, n_rows,
                       row_offset, z, n_total, k_lo, k_cnt, k_total, state, x_out, xt_out);
    return (int)hipGetLastError();
}

int grid_of(int64_t n_rows) {
    const int64_t wgs = (n_rows + kW - 1) / kW;
    return (int)(wgs < kMaxGrid ? wgs : kMaxGrid);
}

}  // namespace

extern "C" {

int pfg_version(void) { return PFG_VERSION; }

const char *pfg_status_string(int status) {
    switch (status) {
        case PFG_OK: return "ok";
        case PFG_EINVAL: return "invalid argument";
        case PFG_EUNSUPPORTED: return "shape not supported by the generator draw kernels";
        case PFG_EWORKSPACE: return "workspace too small";
        default: return status > 0 ? hipGetErrorString((hipError_t)status) : "unknown status";
    }
}

size_t pfg_workspace_bytes(const pfg_mlp *net, int64_t k_cnt) {
    Net n;
    Geo g;
    if (k_cnt < 1 || make_net(net, &n) != PFG_OK || pick_plan(n, k_cnt, &g) == 0) return 0;
    return rnvp::align_up((size_t)n.packed_floats * sizeof(float), 256);
}

int pfg_plan(const pfg_mlp *net, int64_t k_cnt, pfg_plan_info *out) {
    Net n;
    Geo g;
    if (!out || k_cnt < 1 || make_net(net, &n) != PFG_OK) return PFG_EINVAL;
    *out = pfg_plan_info{};
    const int nt = pick_plan(n, k_cnt, &g);
    if (nt == 0) return PFG_EUNSUPPORTED;
    out->draw_tiles = nt;
    out->waves = kW;
    out->weights_in_lds = g.resident;
    out->lds_bytes = (int64_t)g.floats * (int64_t)sizeof(float);
    out->packed_bytes = (int64_t)n.packed_floats * (int64_t)sizeof(float);
    return PFG_OK;
}

int pfg_mlp_draw_accumulate(void *stream, const pfg_mlp *net, const float *params, const float *c,
                            int64_t n_rows, int64_t row_offset, const float *z, int64_t n_total,
                            int64_t k_lo, int64_t k_cnt, int64_t k_total,
                            void *state, float *x_out, float *xt_out, void *workspace, size_t workspace_bytes) {
    Net n;
    if (make_net(net, &n) != PFG_OK || !params || !z) return PFG_EINVAL;
    if (n_rows < 0 || row_offset < 0 || k_cnt < 1 || k_lo < 0) return PFG_EINVAL;
    if (n.c > 0 && !c && n_rows > 0) return PFG_EINVAL;
    if (row_offset + n_rows > n_total) return PFG_EINVAL;
    if (k_lo + k_cnt > k_total) return PFG_EINVAL;
    Geo g;
    const int nt = pick_plan(n, k_cnt, &g);
    if (nt == 0) return PFG_EUNSUPPORTED;
    if (!workspace || workspace_bytes < (size_t)n.packed_floats * sizeof(float)) return PFG_EWORKSPACE;
    if (n_rows == 0) return PFG_OK;
    hipStream_t st = (hipStream_t)stream;
    float *packed = static_cast<float *>(workspace);
    const int pblocks = (n.packed_floats + 255) / 256;
    hipLaunchKernelGGL(k_pack, dim3(pblocks < 1024 ? pblocks : 1024), dim3(256), 0, st, n, params, packed);
    RNVP_HIP_TRY(hipGetLastError());
    const int grid = grid_of(n_rows);
    State *sp = static_cast<State *>(state);
#define PFG_LAUNCH(NT_, RES_) \
    return launch_mlp<NT_, RES_>(st, n, g, grid, params, packed, c, n_rows, row_offset, z, n_total, k_lo, k_cnt, k_total, sp, x_out, xt_out)
    if (g.resident) {
        if (nt == 4) PFG_LAUNCH(4, true);
        if (nt == 2) PFG_LAUNCH(2, true);
        PFG_LAUNCH(1, true);
    }
    if (nt == 4) PFG_LAUNCH(4, false);
    if (nt == 2) PFG_LAUNCH(2, false);
    PFG_LAUNCH(1, false);
#undef PFG_LAUNCH
}

int pfg_affine_draw_accumulate(void *stream, int32_t d, const float *mu, const float *sigma, const float *out_w,
                               const float *out_b, const float *eps, int64_t n_rows, int64_t row_offset, int64_t n_total,
                               int64_t k_lo, int64_t k_cnt, int64_t k_total, void *state, float *x_out, float *xt_out) {
    if (d < 1 || !mu || !sigma || !eps) return PFG_EINVAL;
    if ((out_w == nullptr) != (out_b == nullptr)) return PFG_EINVAL;
    if (n_rows < 0 || row_offset < 0 || k_cnt < 1 || k_lo < 0) return PFG_EINVAL;
    if (row_offset + n_rows > n_total) return PFG_EINVAL;
    if (k_lo + k_cnt > k_total) return PFG_EINVAL;
    if (d > PFG_MAX_D) return PFG_EUNSUPPORTED;
    if (n_rows == 0) return PFG_OK;
    hipLaunchKernelGGL(k_affine_draw, dim3(grid_of(n_rows)), dim3(kThreads), 0, (hipStream_t)stream, (int)d, mu, sigma, out_w,
                       out_b, eps, n_rows, row_offset, n_total, k_lo, k_cnt, k_total, static_cast<State *>(state), x_out, xt_out);
    return (int)hipGetLastError();
}

}  // extern "C"
