/*
 * pf_wgan.h -- C ABI of libpf_wgan.so: the conditional Wasserstein GAN of
 * probaforms.models.wgan (ConditionalWGAN) trained and sampled on the MI355X (gfx950).
 *
 *   pfw_generate     G([z || c])                       inference only, no autograd
 *   pfw_critic       D([x || c])                       inference only, no autograd
 *   pfw_loss_grad    one iteration's loss and the gradient of the net that steps
 *   pfw_train_step   pfw_loss_grad, then RMSprop on that net (plus the clamp on critic steps)
 *   pfw_fit_epoch    one epoch: every batch's pfw_train_step, then the two epoch-end losses
 *
 * Conventions (as include/rnvp_hip.h)
 *   - every array is a DEVICE pointer unless its name ends in _host; sizes are plain integers;
 *   - the caller owns all device memory including the workspace (no hidden hipMalloc);
 *     pfw_workspace_bytes() says how much a call needs;
 *   - kernels are enqueued on `stream` (a hipStream_t passed as void*) and the call returns
 *     without synchronising;
 *   - return value: 0 ok; <0 argument error (PFW_E*); >0 a hipError_t;
 *   - no global mutable state.  Partial gradients are summed in a fixed order with no float
 *     atomics: the same inputs give bitwise the same outputs, and pfw_fit_epoch equals the
 *     loop of pfw_train_step calls it replaces bit for bit.
 *
 * Data layout
 *   params [P_G + P_D] float32: the generator's nn.Linear weights and biases in module order
 *   (W0, b0, W1, b1, ..., row-major [out, in]), then the discriminator's in the same form.
 *   square_avg has the same layout (RMSprop state of both nets).
 *   x [n, d], c [n, c] (c may be NULL when c == 0), z [rows, latent]: float32 row-major.
 *   row_index [rows] int64 (nullable = identity): batch row r is row row_index[r] of x and c;
 *   z is indexed by the batch row itself.
 *   The generator maps latent + c inputs to d outputs, the discriminator d + c inputs to 1.
 */
#ifndef PF_WGAN_H
#define PF_WGAN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PFW_OK            0
#define PFW_EINVAL       (-1)   /* NULL pointer, non-positive size, bad shape or kind         */
#define PFW_EUNSUPPORTED (-2)   /* one row's working set does not fit the 160 KiB of LDS        */
#define PFW_EWORKSPACE   (-3)   /* workspace smaller than pfw_workspace_bytes() says            */

#define PFW_VERSION 101         /* pfw_version(): bumped whenever the ABI changes (101: pfw_tiling) */

#define PFW_MAX_HIDDEN 8
#define PFW_ACT_TANH 0          /* the values of RNVP_ACT_* (include/rnvp_hip.h)                  */
#define PFW_ACT_RELU 1          /* the reference maps every activation other than 'tanh' to ReLU */

#define PFW_NET_G 0
#define PFW_NET_D 1

/* step kinds: iter_i % n_critic != 0 -> critic step, else generator step (wgan.py:233) */
#define PFW_STEP_GEN    0
#define PFW_STEP_CRITIC 1

typedef struct pfw_shape {
    int32_t d;                          /* data columns                               */
    int32_t c;                          /* condition columns (0: no conditions)       */
    int32_t latent;                     /* latent_dim                                 */
    int32_t g_n_hidden;                 /* generator: hidden layers, 1..PFW_MAX_HIDDEN */
    int32_t g_hidden[PFW_MAX_HIDDEN];
    int32_t g_act;                      /* PFW_ACT_*                                  */
    int32_t d_n_hidden;                 /* discriminator                              */
    int32_t d_hidden[PFW_MAX_HIDDEN];
    int32_t d_act;
} pfw_shape;

/* RMSprop(alpha, eps, weight_decay, lr), no momentum, not centred; clamp > 0 clips the critic's
 * parameters to [-clamp, clamp] after its step (wgan.py:248) */
typedef struct pfw_rmsprop {
    double lr, alpha, eps, weight_decay, clamp;
} pfw_rmsprop;

/* pfw_tiling(): how the host tiles a batch / an inference call of `rows` rows.  A tile is the rows one workgroup
 * stages in LDS; *_lds_bytes is the dynamic LDS its launch requests (above 65 536 the launch first raises the
 * kernel's limit).  A tile of 0: that kernel cannot run this shape. */
typedef struct pfw_tiling_info {
    int32_t step_tile;                  /* R: batch rows per k_step workgroup (a critic step stages 2R LDS rows) */
    int32_t step_cap;                   /* the largest R that LDS and the 256 threads allow                      */
    int32_t eloss_tile;                 /* pfw_epoch_losses                                                      */
    int32_t gen_tile;                   /* pfw_generate                                                          */
    int32_t crit_tile;                  /* pfw_critic                                                            */
    int32_t reserved;
    int64_t step_wgs;                   /* G = ceil(rows / R): workgroups, and partial-gradient slabs summed     */
    int64_t step_wg_bound;              /* the G that pfw_workspace_bytes(rows) provides for: >= G of any batch
                                           of at most `rows` rows                                               */
    int64_t step_lds_bytes;
    int64_t eloss_lds_bytes;
    int64_t gen_lds_bytes;
    int64_t crit_lds_bytes;
} pfw_tiling_info;

int         pfw_version(void);
const char *pfw_status_string(int status);

/* parameters of one net (PFW_NET_G / PFW_NET_D); -1 for an invalid shape */
int64_t pfw_param_count(const pfw_shape *s, int net);

/* workspace of a training call whose batches have at most batch_rows rows and whose epoch-end
 * losses run over loss_rows rows (0 when none are computed) */
size_t pfw_workspace_bytes(const pfw_shape *s, int64_t batch_rows, int64_t loss_rows);

/* Host only, launches nothing: the tiling of a training step on `rows` batch rows and of the inference calls on
 * `rows` rows, from the same functions the launches use.  PFW_EINVAL for a bad shape, rows < 1 or a NULL out;
 * PFW_EUNSUPPORTED where the step cannot run (the step fields are then 0; the inference fields are still filled). */
int pfw_tiling(const pfw_shape *s, int64_t rows, pfw_tiling_info *out);

/* out [n, d] = G([z || c]) */
int pfw_generate(void *stream, const pfw_shape *s, const float *params, const float *z, const float *c,
                 int64_t n, float *out);

/* out [n] = D([x || c]) */
int pfw_critic(void *stream, const pfw_shape *s, const float *params, const float *x, const float *c,
               int64_t n, float *out);

/*
 * One iteration on the batch rows (row_index) with noise z [rows, latent]; fake = G([z || c]).
 *   kind PFW_STEP_CRITIC: loss = -mean D([x || c]) + mean D([fake || c]), gradient w.r.t. D's parameters
 *   kind PFW_STEP_GEN:    loss = -mean D([fake || c]),                    gradient w.r.t. G's parameters
 * grad_out [P of the stepped net] (nullable), loss_out [1] (nullable).
 */
int pfw_loss_grad(void *stream, const pfw_shape *s, int kind, const float *params, const float *x, const float *c,
                  const int64_t *row_index, const float *z, int64_t rows, float *grad_out, float *loss_out,
                  void *workspace, size_t workspace_bytes);

/* pfw_loss_grad, then (torch.optim.RMSprop order) g += wd * p; v = alpha * v + (1 - alpha) * g * g;
 * p += -lr * (g / (sqrt(v) + eps)) on the stepped net, and on critic steps p = clamp(p, -clamp, clamp).
 * grad_out receives the gradient before weight decay. */
int pfw_train_step(void *stream, const pfw_shape *s, int kind, float *params, float *square_avg, const float *x,
                   const float *c, const int64_t *row_index, const float *z, int64_t rows, const pfw_rmsprop *opt,
                   float *grad_out, float *loss_out, void *workspace, size_t workspace_bytes);

/*
 * One epoch.  Batch b covers perm[b * batch_size, min(n, (b + 1) * batch_size)) and its noise is the same
 * rows of z_batches [n, latent]; its step kind is kinds_host[b] (host memory).  Then, with
 * fake = G([z_full || c]) over all n rows:
 *   epoch_losses[0] = -mean D([fake || c])                  (gen_loss_history, wgan.py:289)
 *   epoch_losses[1] = mean D([x || c]) + epoch_losses[0]    (disc_loss_history, wgan.py:290)
 * z_full may be NULL: no epoch-end losses (epoch_losses untouched).
 */
int pfw_fit_epoch(void *stream, const pfw_shape *s, float *params, float *square_avg, const float *x, const float *c,
                  const int64_t *perm, const float *z_batches, const float *z_full, int64_t n, int64_t batch_size,
                  const int8_t *kinds_host, const pfw_rmsprop *opt, float *epoch_losses,
                  void *workspace, size_t workspace_bytes);

/* the epoch-end losses alone (the tail of pfw_fit_epoch) */
int pfw_epoch_losses(void *stream, const pfw_shape *s, const float *params, const float *x, const float *c,
                     const float *z_full, int64_t n, float *epoch_losses, void *workspace, size_t workspace_bytes);

#ifdef __cplusplus
}
#endif
#endif
