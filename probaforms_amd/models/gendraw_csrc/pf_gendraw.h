/*
 * pf_gendraw.h -- C ABI of libpf_gendraw.so: multi-draw predictive statistics of the three generators that are not
 * flows (CVAE, ConditionalWGAN, ConditionalNormal) on the MI355X (gfx950).  For every condition row it evaluates K
 * draws and reduces across them on the device, writing the running-moment state pf_predict.h documents, so that the
 * caller finishes with pfp_finalize / pfp_quantiles of libpf_predict.so.
 *
 *   pfg_mlp_draw_accumulate      x[k][r] = MLP([z[k][r] || c[r]]): CVAE's Decoder, ConditionalWGAN's Generator
 *   pfg_affine_draw_accumulate   x[k][r] = out(mu[r] + eps[k][r] * sigma[r]): ConditionalNormal
 *
 * Conventions (as pf_predict.h)
 *   - every array is a DEVICE pointer; sizes are plain integers;
 *   - the caller owns all device memory including the workspace (no hidden hipMalloc);
 *   - kernels are enqueued on `stream` (a hipStream_t passed as void*) and the call returns without synchronising;
 *   - return value: 0 ok; <0 argument error (PFG_E*); >0 a hipError_t;
 *   - no global mutable state other than the one-time kernel attribute setup; no float atomics: the same inputs
 *     give bitwise the same outputs.  No kernel waits on another workgroup.
 *
 * Rows and draws: exactly the contract of pfp_draw_accumulate.  A call handles the condition rows row_offset ..
 * row_offset + n_rows of a larger job of n_total rows and the draws k_lo .. k_lo + k_cnt of k_total.  A draw's value
 * depends only on (z[k] / eps[k] of the GLOBAL row, the row's own inputs): not on the draw-tile width, the wave that
 * computed it, the window or the row split.  Any split of the rows over calls gives bitwise the result of one call,
 * state included; a split of the draws into windows changes the order of the float64 sums, so the moments of windows
 * agree to rounding only (draws, min and max stay bitwise).
 *
 *   state   [n_rows, n_out] x PFP_STATE_BYTES   (nullable) read, updated with this call's draws, written back
 *   x_out   [k_cnt, n_rows, n_out]              (nullable) the draws
 *   xt_out  [n_rows, n_out, k_total]            (nullable) the draws transposed, written at columns k_lo .. k_lo + k_cnt
 */
#ifndef PF_GENDRAW_H
#define PF_GENDRAW_H

#include <stddef.h>
#include <stdint.h>

#include "../predict_csrc/pf_predict.h"   /* PFP_STATE_BYTES and the state's layout; RNVP_ACT_* */

#ifdef __cplusplus
extern "C" {
#endif

#define PFG_OK            0
#define PFG_EINVAL       (-1)   /* NULL pointer, negative size, bad shape                              */
#define PFG_EUNSUPPORTED (-2)   /* one draw tile's activations do not fit the LDS; d > PFG_MAX_D       */
#define PFG_EWORKSPACE   (-3)   /* workspace smaller than pfg_workspace_bytes() says                   */

#define PFG_VERSION 100         /* pfg_version(): bumped whenever an argument list or a struct changes */

#define PFG_MAX_HIDDEN 8
#define PFG_MAX_D 32            /* pfg_affine_draw_accumulate: PFN_MAX_D of pf_cnormal.h               */
#define PFG_WAVES 4             /* waves of a workgroup; each owns one condition row at a time         */

/* a plain MLP: Linear(latent + c, hidden[0]), act, ..., Linear(hidden[n_hidden - 1], n_out) */
typedef struct pfg_mlp {
    int32_t n_out;                      /* output columns (d), >= 1                        */
    int32_t c;                          /* condition columns, >= 0                         */
    int32_t latent;                     /* z columns, >= 1                                 */
    int32_t n_hidden;                   /* hidden layers, 1..PFG_MAX_HIDDEN                */
    int32_t hidden[PFG_MAX_HIDDEN];
    int32_t act;                        /* RNVP_ACT_TANH / RNVP_ACT_RELU                   */
} pfg_mlp;

/* what a launch of pfg_mlp_draw_accumulate with k_cnt draws does, from the functions the launch itself uses */
typedef struct pfg_plan_info {
    int32_t draw_tiles;                 /* tiles of 16 draws a wave pushes through the net per pass: 1, 2 or 4 */
    int32_t waves;                      /* waves per workgroup (PFG_WAVES)                                     */
    int32_t weights_in_lds;             /* 1: the workgroup stages the packed weights in LDS; 0: read from the workspace */
    int32_t reserved;
    int64_t lds_bytes;                  /* dynamic LDS of one workgroup                                        */
    int64_t packed_bytes;               /* the packed weights and biases in the workspace                      */
} pfg_plan_info;

int         pfg_version(void);
const char *pfg_status_string(int status);

/* bytes of device workspace pfg_mlp_draw_accumulate needs; 0 for an invalid or unsupported shape or k_cnt < 1 */
size_t pfg_workspace_bytes(const pfg_mlp *net, int64_t k_cnt);

/* Host only, launches nothing.  PFG_EINVAL for a bad shape, k_cnt < 1 or a NULL out; PFG_EUNSUPPORTED when not even
 * one tile of 16 draws per wave fits the LDS. */
int pfg_plan(const pfg_mlp *net, int64_t k_cnt, pfg_plan_info *out);

/*
 * x[k][r] = MLP([z[k][row_offset + r] || c[r]]).
 *   params  W0, b0, ..., W_last, b_last; every W row-major [out, in]; W0's first `latent` columns take z
 *   c       [n_rows, c]               conditions of this call's rows (NULL iff c == 0)
 *   z       [k_cnt, n_total, latent]  the latent draws of this window, indexed by GLOBAL row
 * The activation is tanhf / fmaxf(v, 0.f), so a ReLU net maps a NaN pre-activation to 0 as the models' own sample
 * does.  row_offset + n_rows <= n_total and k_lo + k_cnt <= k_total (PFG_EINVAL otherwise).
 */
int pfg_mlp_draw_accumulate(void *stream, const pfg_mlp *net, const float *params, const float *c,
                            int64_t n_rows, int64_t row_offset, const float *z, int64_t n_total,
                            int64_t k_lo, int64_t k_cnt, int64_t k_total,
                            void *state, float *x_out, float *xt_out, void *workspace, size_t workspace_bytes);

/*
 * x[k][r] = out_w . (mu[r] + eps[k][row_offset + r] * sigma[r]) + out_b, rounded as pfn_forward rounds x_tilde
 * (product and sum separately, then one fmaf chain per output over the d inputs in order).
 *   mu, sigma     [n_rows, d]          of this call's rows
 *   out_w, out_b  [d, d] row-major, [d]; both NULL: independent covariance, x = mu + eps * sigma
 *   eps           [k_cnt, n_total, d]  indexed by GLOBAL row
 * 1 <= d <= PFG_MAX_D (PFG_EUNSUPPORTED above).
 */
int pfg_affine_draw_accumulate(void *stream, int32_t d, const float *mu, const float *sigma, const float *out_w,
                               const float *out_b, const float *eps, int64_t n_rows, int64_t row_offset, int64_t n_total,
                               int64_t k_lo, int64_t k_cnt, int64_t k_total, void *state, float *x_out, float *xt_out);

#ifdef __cplusplus
}
#endif
#endif
