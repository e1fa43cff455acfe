/*
 * pf_predict.h -- C ABI of libpf_predict.so: multi-draw predictive statistics of a conditional RealNVP flow on
 * the MI355X (gfx950).  For every condition row it pushes K prior draws through the inverse flow
 * (RealNVPLayer.g, realnvp.py:104-129; NormalizingFlow.sample, nflow.py:142-143) and reduces across the draws
 * on the device: what the reference's notebooks do with a Python loop of `model.sample(X)` calls followed by
 * numpy's mean / std / quantile over the stacked results.
 *
 *   pfp_draw_accumulate   K draws per row through the inverse flow; running moments, the draws, their transpose
 *   pfp_finalize          running moments -> mean, std, min, max
 *   pfp_quantiles         exact quantiles (numpy's default 'linear') of the transposed draws
 *   pfp_scores            CRPS, PIT, quantiles and pinball losses of the transposed draws against observed targets
 *   pfp_joint_scores      energy score and variogram score of each row's draws as vectors in R^d (pf_joint.hip)
 *   pfp_joint_tiling      how pfp_joint_scores walks a row of (d, K): host only
 *
 * Conventions (as pf_cnormal.h)
 *   - every array is a DEVICE pointer unless it says HOST; sizes are plain integers;
 *   - the caller owns all device memory including the workspace (no hidden hipMalloc);
 *   - kernels are enqueued on `stream` (a hipStream_t passed as void*) and the call returns without synchronising;
 *   - return value: 0 ok; <0 argument error (PFP_E*); >0 a hipError_t;
 *   - no global mutable state other than the one-time kernel attribute setup; no float atomics: the same inputs
 *     give bitwise the same outputs.
 *
 * Data layout: `shape`, `params` and `masks` are those of include/rnvp_hip.h (flat float32 parameters in
 * nf.parameters() order; masks [L, d] uint8, 1 = pass-through; masks may be NULL when shape->alt_masks is 1 or 2).
 * Of rnvp_shape only L, d, c, n_hidden, hidden, act and alt_masks are read.
 *
 * Rows and draws.  A call handles the condition rows row_offset .. row_offset + n_rows of a larger job and the
 * draws k_lo .. k_lo + k_cnt of K_total.  Row r's results depend only on (seeds / z, the GLOBAL row, c[r]): any
 * split of the rows over calls gives bitwise the result of one call.  A split of the draws into windows changes
 * the order of the float64 sums, so windows agree to rounding only.
 */
#ifndef PF_PREDICT_H
#define PF_PREDICT_H

#include <stddef.h>
#include <stdint.h>

#include "../../../include/rnvp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PFP_OK            0
#define PFP_EINVAL       (-1)   /* NULL pointer, negative size, bad shape                                    */
#define PFP_EUNSUPPORTED (-2)   /* one draw tile's image does not fit the LDS, or K_total > PFP_MAX_QUANTILE_DRAWS */
#define PFP_EWORKSPACE   (-3)   /* workspace smaller than pfp_workspace_bytes() says                         */

#define PFP_VERSION 101         /* pfp_version(): bumped whenever an argument list or the state's layout or meaning changes */

#define PFP_MAX_QUANTILE_DRAWS 8192   /* pfp_quantiles / pfp_scores sort one (row, column) series inside one workgroup's LDS;
                                         pfp_joint_scores bounds one workgroup's O(K^2) pair loop by the same number */

/*
 * Running moments of one (row, column): PFP_STATE_BYTES bytes, all zero = nothing seen yet.
 *   float64 sum, sumsq   of (x - shift) and its square over the draws seen
 *   float32 shift        the first draw seen, or 0 when that draw is not finite (inf - shift then stays inf)
 *   float32 min, max     NaN once a NaN has been seen (numpy's min / max, not fminf / fmaxf)
 *   uint32  count
 * The values accumulated are the float32 values x_out receives.
 *
 * Non-finite draws follow numpy over the stacked draws.  A series holding a NaN: mean, std, min, max and every quantile
 * are NaN.  A series holding +inf (or -inf) and no NaN: mean +inf (-inf), std NaN, min / max exact; both infinities:
 * mean NaN.  A quantile that interpolates from or to an infinity is what numpy's lerp gives (NaN where it forms
 * inf * 0 or inf - inf).  Each (row, column) series is reduced on its own: a NaN never leaves its series.
 */
#define PFP_STATE_BYTES 32

int         pfp_version(void);
const char *pfp_status_string(int status);

/* bytes of device workspace pfp_draw_accumulate needs for k_cnt draws per call; 0 for an invalid or unsupported shape */
size_t pfp_workspace_bytes(const rnvp_shape *shape, int64_t k_cnt);

/*
 * x[k][r] = g(z[k][r], c[r]) for the n_rows rows and k_cnt draws of this call, in ONE launch.
 *   c       [n_rows, cdim]            conditions of this call's rows (NULL iff cdim == 0)
 *   seeds   HOST [k_cnt] uint64       draw k_lo + i uses z[r][j] = the counter-based prior value of
 *                                     (seeds[i], row_offset + r, j): the numbers rnvp_sample(seed = seeds[i],
 *                                     row_offset) uses, drawn in registers and never written; or NULL and
 *   z       [k_cnt, n_total, d]       the prior draws themselves, indexed by GLOBAL row (row_offset + r < n_total)
 *   state   [n_rows, d] x PFP_STATE_BYTES   (nullable) read, updated with this call's draws, written back
 *   x_out   [k_cnt, n_rows, d]        (nullable) the draws
 *   xt_out  [n_rows, d, k_total]      (nullable) the draws transposed, written at columns k_lo .. k_lo + k_cnt
 * Exactly one of seeds / z is given.  With seeds the call is the one exception to "returns without synchronising": the HOST array
 * is copied into the workspace by a stream-ordered host-to-device copy (hipMemcpyAsync), so it must stay alive until `stream`
 * has passed the call; from pageable memory that copy may make the call wait for the work enqueued on `stream` before it, and a
 * capture would record the host address, not the values.  Given z the call enqueues one launch and nothing else.  On either path row_offset + n_rows <= n_total (the rows of the whole job) and
 * k_lo + k_cnt <= k_total, whichever outputs are asked for (PFP_EINVAL otherwise).  PFP_EUNSUPPORTED when the shape's per-tile image exceeds a CU's LDS.
 */
int pfp_draw_accumulate(void *stream, const rnvp_shape *shape, const float *params, const uint8_t *masks,
                        const float *c, int64_t n_rows, int64_t row_offset,
                        const uint64_t *seeds, const float *z, int64_t n_total,
                        int64_t k_lo, int64_t k_cnt, int64_t k_total,
                        void *state, float *x_out, float *xt_out,
                        void *workspace, size_t workspace_bytes);

/*
 * state -> mean, std (divisor count - ddof), min, max, each [n_rows, d] float32 and nullable.  float64 arithmetic,
 * one rounding to float32 at the end.  A series with count <= ddof gives std = NaN, as numpy does; count == 0
 * gives NaN everywhere.  Non-finite draws: see the state comment above.
 */
int pfp_finalize(void *stream, const void *state, int64_t n_rows, int32_t d, int32_t ddof,
                 float *mean, float *std, float *min, float *max);

/*
 * q_out[i][r][j] = numpy.quantile(xt[r][j][:], probs[i]) (method 'linear'), evaluated in float64 on the sorted
 * series and rounded once.  xt [n_rows, d, k_total] (pfp_draw_accumulate's xt_out; not modified),
 * probs [n_probs] float64 in [0, 1], 1 <= k_total <= PFP_MAX_QUANTILE_DRAWS.  Any k_total: the sort pads to a
 * power of two with keys above every float, which are never selected.  A series holding a NaN of either sign gives
 * NaN for every probability.
 */
int pfp_quantiles(void *stream, const float *xt, int64_t n_rows, int32_t d, int64_t k_total,
                  const double *probs, int32_t n_probs, float *q_out);

/*
 * Scores of every (row, column) series x_1 .. x_K = xt[r][j][:] against its observed target y[r][j], in float64 on the
 * sorted series with one rounding to float32 (D = K, or K - 1 when fair != 0):
 *   crps[r][j]       = 1/K sum_k |x_k - y|  -  1/(2 K D) sum_k sum_l |x_k - x_l|      (fair and K = 1: NaN, 0 / 0)
 *   pit[r][j]        = (#{x_k < y} + 0.5 #{x_k == y}) / K                             (float comparisons: -0 == +0)
 *   q_out[i][r][j]   = what pfp_quantiles returns for the same series and probs[i], bitwise
 *   pinball[i][r][j] = (y - Q_i) (probs[i] - [y < Q_i]),  Q_i the float64 quantile before its rounding
 * xt [n_rows, d, k_total] and y [n_rows, d] are not modified; crps, pit [n_rows, d] and q_out, pinball
 * [n_probs, n_rows, d] are each nullable; probs [n_probs] float64 in [0, 1], NULL iff n_probs == 0;
 * 1 <= k_total <= PFP_MAX_QUANTILE_DRAWS.  The pair sum is evaluated as 2 sum_i (2 i - K + 1) x_(i) over the sorted series,
 * the sums in an order fixed by k_total alone (no atomics): a series' results are bitwise the same in any call.
 * Non-finite values: a NaN in the series or in y makes crps, pit and every pinball of that (row, column) NaN (q_out
 * only for a NaN in the series); otherwise the outputs are what numpy gives for the definitions above, pair sum included:
 * a series holding an infinity has crps NaN (inf - inf), y = +-inf with a finite series has crps +inf.  Nothing leaves its
 * (row, column).
 */
int pfp_scores(void *stream, const float *xt, const float *y, int64_t n_rows, int32_t d, int64_t k_total,
               int32_t fair, const double *probs, int32_t n_probs,
               float *crps, float *pit, float *q_out, float *pinball);

/*
 * Joint scores of every row's draws x_1 .. x_K = xt[r][:][k] in R^d against its target y[r][:], in float64 from the float32
 * values (every difference, square, sum and square root; the sums of squares over the d columns included) with one rounding
 * to float32 (D = K, or K - 1 when fair != 0):
 *   spread[r]    = 1/(2 K D) sum_k sum_l |x_k - x_l|_2                                   (fair and K = 1: NaN, 0 / 0)
 *   energy[r]    = 1/K sum_k |x_k - y|_2  -  spread[r]            (Gneiting & Raftery 2007; at d = 1 the crps of pfp_scores)
 *   variogram[r] = sum_i sum_j ( |y_i - y_j|^p - 1/K sum_k |x_ki - x_kj|^p )^2           (Scheuerer & Hamill 2015, unit
 *                  weights, p = variogram_order; 0 when d = 1)
 * xt [n_rows, d, k_total] (pfp_draw_accumulate's xt_out) and y [n_rows, d] are not modified; energy, spread and variogram
 * [n_rows] are each nullable, and what is not asked for is not computed (no variogram: no O(K d^2) pass; neither energy nor
 * spread: no pair loop).  variogram_order is 0.5, 1 or 2, evaluated as sqrt, identity or square; it is ignored when variogram
 * is NULL and PFP_EINVAL otherwise.  1 <= k_total <= PFP_MAX_QUANTILE_DRAWS (PFP_EUNSUPPORTED above); every d >= 1 is served.
 * One workgroup per row, the draws staged through LDS as pfp_joint_tiling reports; each unordered pair of draws is visited
 * once; per-thread float64 partials are combined by a fixed halving tree, no atomics: the order of every sum depends on
 * (d, k_total) alone, so a row's results are bitwise the same in any call, any grid and any split of the rows over calls.
 * Non-finite values: a NaN among the row's draws or in its y makes all three outputs NaN.  A row whose draws hold an infinity
 * has energy and spread NaN (the pair sum's diagonal forms inf - inf; it is not summed, so this is set explicitly); a finite
 * row with an infinity in y has energy +inf.  The variogram's (i, i) terms form inf - inf as soon as the row's draws or its y
 * hold an infinity: it is then NaN (set explicitly, the diagonal is not summed either).  Nothing leaves its row.
 */
int pfp_joint_scores(void *stream, const float *xt, const float *y, int64_t n_rows, int32_t d, int64_t k_total,
                     int32_t fair, double variogram_order, float *energy, float *spread, float *variogram);

/*
 * How pfp_joint_scores walks one row of (d, k_total).  The draws' images [column][draw] and y share budget_bytes of LDS:
 *   n_tiles == 1                  d (K + 1) floats fit: the whole row is one image, tile_draws == k_total
 *   n_tiles  > 1, n_chunks == 1   tiles of tile_draws draws (a multiple of 64), two images of all d columns
 *   n_chunks > 1                  even two 64-draw images of all columns do not fit: tile_draws == 64 and the columns pass
 *                                 through in n_chunks chunks of chunk_cols
 * lds_bytes is one workgroup's dynamic LDS (the reduction scratch included), threads its size, max_grid the largest grid: more
 * rows than that are served by the grid stride.
 */
typedef struct {
    int32_t tile_draws, n_tiles;
    int32_t chunk_cols, n_chunks;
    int32_t budget_bytes, lds_bytes;
    int32_t threads, max_grid;
} pfp_joint_tile;

/* host only, no GPU.  PFP_EINVAL for NULL out, d < 1 or k_total < 1; PFP_EUNSUPPORTED for k_total > PFP_MAX_QUANTILE_DRAWS */
int pfp_joint_tiling(int32_t d, int64_t k_total, pfp_joint_tile *out);

#ifdef __cplusplus
}
#endif
#endif
