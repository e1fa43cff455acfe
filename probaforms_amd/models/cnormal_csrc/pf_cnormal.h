/*
 * pf_cnormal.h -- C ABI of libpf_cnormal.so: the conditional normal model of
 * probaforms.models.cnormal (ConditionalNormal / Net) trained and sampled on the MI355X (gfx950).
 *
 *   pfn_forward      Net.forward and sample: mu, sigma, x_tilde, inv   (inference only, no autograd)
 *   pfn_loss_grad    one batch's loss and the gradient of every parameter
 *   pfn_train_step   pfn_loss_grad, then torch.optim.Adam on the parameters
 *   pfn_fit_epoch    one epoch: every batch's pfn_train_step
 *
 * Conventions (as pf_wgan.h)
 *   - every array is a DEVICE pointer; sizes are plain integers;
 *   - the caller owns all device memory including the workspace (no hidden hipMalloc);
 *     pfn_workspace_bytes() says how much a call needs;
 *   - kernels are enqueued on `stream` (a hipStream_t passed as void*) and the call returns
 *     without synchronising;
 *   - return value: 0 ok; <0 argument error (PFN_E*); >0 a hipError_t;
 *   - no global mutable state.  Partial gradients are summed in a fixed order with no float
 *     atomics: the same inputs give bitwise the same outputs, and pfn_fit_epoch equals the
 *     loop of pfn_train_step calls it replaces bit for bit.
 *
 * The model (cnormal.py:18-91)
 *   h = model(C)  (n_hidden Linears, each followed by the activation),  mu = mu(h),
 *   sigma = exp(log_sigma(h)),  x_tilde = mu + eps * sigma,  and in full-covariance mode
 *   x_tilde = out(x_tilde);  inv_r = W^-1 (x_r - b) with (W, b) = out's weight and bias.
 *   loss = mean over rows x d of (t - mu)^2 / (2 sigma^2) + log(sigma), t = x (independent) or inv (full).
 *
 * Data layout
 *   params [P] float32: every nn.Linear's weight (row-major [out, in]) then bias, in module order:
 *   model.0, model.2, ..., mu, log_sigma, out.  `out` (d*d + d floats, the tail of the buffer) exists in
 *   both modes; in independent mode it has no gradient and the optimizer never touches it.
 *   exp_avg / exp_avg_sq have the same layout.  x [n, d], c [n, c], eps [n, d]: float32 row-major.
 *   row_index [rows] int64 (nullable = identity): batch row r is row row_index[r] of x and c.
 *
 * Errors of the d x d inverse (full-covariance mode only): W is inverted on the device by Gauss-Jordan
 * elimination with partial pivoting in float64.  A zero pivot or a non-finite entry of the inverse sets
 * status[0] = 1 (it is 0 otherwise); the step's Adam update is then skipped (parameters and optimizer
 * state keep their bits), the loss and gradient written are not meaningful.  Within pfn_fit_epoch the
 * word is sticky: 1 if any batch failed.  `status` is nullable.
 */
#ifndef PF_CNORMAL_H
#define PF_CNORMAL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PFN_OK            0
#define PFN_EINVAL       (-1)   /* NULL pointer, non-positive size, bad shape                        */
#define PFN_EUNSUPPORTED (-2)   /* d > PFN_MAX_D, or one row's working set does not fit the LDS      */
#define PFN_EWORKSPACE   (-3)   /* workspace smaller than pfn_workspace_bytes() says                 */

#define PFN_VERSION 101         /* pfn_version(): bumped whenever the ABI changes (101: pfn_tiling)  */

#define PFN_MAX_HIDDEN 8
#define PFN_MAX_D 32            /* the d x d system is inverted by ONE workgroup: [d, 2d] float64 in LDS */
#define PFN_ACT_TANH    0
#define PFN_ACT_RELU    1       /* the reference maps every activation it does not know to ReLU      */
#define PFN_ACT_SIGMOID 2

typedef struct pfn_shape {
    int32_t d;                          /* data columns (var_size), 1..PFN_MAX_D      */
    int32_t c;                          /* condition columns (cond_size), >= 1        */
    int32_t n_hidden;                   /* hidden layers, 1..PFN_MAX_HIDDEN           */
    int32_t hidden[PFN_MAX_HIDDEN];
    int32_t act;                        /* PFN_ACT_*                                  */
    int32_t independent;                /* 1: independent_covariance (t = x, out unused) */
} pfn_shape;

/* torch.optim.Adam(lr, betas, eps, weight_decay): L2 weight decay, no amsgrad */
typedef struct pfn_adam {
    double lr, beta1, beta2, eps, weight_decay;
} pfn_adam;

/* pfn_tiling(): how the host tiles a batch / a pfn_forward call of `rows` rows.  A tile is the rows one workgroup
 * stages in LDS; *_lds_bytes is the dynamic LDS its launch requests (above 65 536 the launch first raises the
 * kernel's limit).  A tile of 0: that kernel cannot run this shape. */
typedef struct pfn_tiling_info {
    int32_t step_tile;                  /* R: batch rows per k_step workgroup                                    */
    int32_t step_cap;                   /* the largest R that LDS and the 256 threads allow                      */
    int32_t fwd_tile;                   /* pfn_forward                                                           */
    int32_t reserved;
    int64_t step_wgs;                   /* G = ceil(rows / R): workgroups, and partial-gradient slabs summed     */
    int64_t step_wg_bound;              /* the G that pfn_workspace_bytes(rows) provides for: >= G of any batch
                                           of at most `rows` rows                                               */
    int64_t step_lds_bytes;
    int64_t fwd_lds_bytes;
} pfn_tiling_info;

int         pfn_version(void);
const char *pfn_status_string(int status);

/* parameters of the net (out included); -1 for an invalid shape */
int64_t pfn_param_count(const pfn_shape *s);

/* workspace of a training call whose batches have at most batch_rows rows; 0 for an invalid shape */
size_t pfn_workspace_bytes(const pfn_shape *s, int64_t batch_rows);

/* Host only, launches nothing: the tiling of a training step on `rows` batch rows and of pfn_forward on `rows` rows,
 * from the same functions the launches use.  PFN_EINVAL for a bad shape, rows < 1 or a NULL out; PFN_EUNSUPPORTED
 * where the step cannot run (the step fields are then 0; fwd_* is still filled where pfn_forward can run). */
int pfn_tiling(const pfn_shape *s, int64_t rows, pfn_tiling_info *out);

/*
 * Net.forward over n rows.  Outputs (each [n, d], each nullable): mu, sigma, x_tilde, inv.
 * x_tilde needs eps [n, d]; inv needs x [n, d] (PFN_EINVAL otherwise).  inv is computed in both modes,
 * as the reference does; status (see above) is written whenever it is given.
 */
int pfn_forward(void *stream, const pfn_shape *s, const float *params, const float *c, const float *eps,
                const float *x, int64_t n, float *mu, float *sigma, float *x_tilde, float *inv, int32_t *status);

/* loss_out [1] (nullable) and grad_out [P] (nullable) of the batch rows; in independent mode the `out`
 * block of grad_out is written as zeros */
int pfn_loss_grad(void *stream, const pfn_shape *s, const float *params, const float *x, const float *c,
                  const int64_t *row_index, int64_t rows, float *grad_out, float *loss_out, int32_t *status,
                  void *workspace, size_t workspace_bytes);

/* pfn_loss_grad, then Adam step number `step` (>= 1) in torch's single-tensor order: g += wd * p;
 * m += (1 - b1) (g - m); v = b2 v + (1 - b2) g g; p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps).
 * grad_out receives the gradient before weight decay.  In independent mode the `out` block of params,
 * exp_avg and exp_avg_sq is left bit for bit untouched. */
int pfn_train_step(void *stream, const pfn_shape *s, float *params, float *exp_avg, float *exp_avg_sq,
                   const float *x, const float *c, const int64_t *row_index, int64_t rows, const pfn_adam *opt,
                   int64_t step, float *grad_out, float *loss_out, int32_t *status, void *workspace,
                   size_t workspace_bytes);

/* One epoch: batch b covers perm[b * batch_size, min(n, (b + 1) * batch_size)) and is Adam step
 * first_step + b; losses [ceil(n / batch_size)] receives every batch's loss. */
int pfn_fit_epoch(void *stream, const pfn_shape *s, float *params, float *exp_avg, float *exp_avg_sq,
                  const float *x, const float *c, const int64_t *perm, int64_t n, int64_t batch_size,
                  const pfn_adam *opt, int64_t first_step, float *losses, int32_t *status, void *workspace,
                  size_t workspace_bytes);

#ifdef __cplusplus
}
#endif
#endif
