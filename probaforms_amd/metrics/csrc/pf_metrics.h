/*
 * pf_metrics.h -- C ABI of libpf_metrics.so: bootstrapped two-sample metrics of
 * probaforms.metrics on the MI355X (gfx950).
 *
 *   pfm_mmd           one maximum-mean-discrepancy replicate per bootstrap draw
 *                     (probaforms/metrics/mmd.py, mmd_calc): median pairwise distance by
 *                     radix select, then the RBF kernel means over XX, YY and XY
 *   pfm_boot_moments  mean and np.cov covariance (ddof 1) of each resampled set
 *                     (probaforms/metrics/fd.py); the trace of the matrix square root is
 *                     left to the caller (pfm_frechet_grad forms it on the device)
 *   pfm_metric1d      the per-feature rank and density statistics behind the eight 1-D
 *                     metrics (probaforms/metrics/ks1d.py, div1d.py), from the pooled
 *                     column's sorted order and the replicate's draw counts
 *   pfm_wasserstein1d the 1-D Wasserstein distance W_p^p (p = 1, 2) of every replicate's columns, from the
 *                     same sorted order and draw counts; pfm_project makes such columns of a
 *                     multivariate sample's projections (sliced Wasserstein distance)
 *   pfm_prdc          k-nearest-neighbour precision, recall, density and coverage: every row's k-th-neighbour
 *                     radius inside its own resampled set, then the real x fake squared distances against
 *                     those radii, as four integer counts per replicate
 *   pfm_energy        the energy distance's three pair sums (real x real, fake x fake, real x fake Euclidean
 *                     distances) of every replicate: each distance is formed once per call on the original rows
 *                     and weighted by the replicates' draw counts, one float64 multiply-add per replicate and pair
 *   pfm_sinkhorn      the debiased Sinkhorn divergence (entropic optimal transport, cost |x - y|^p) of every replicate: the
 *                     costs are re-formed tile by tile on the original rows in every iteration, the replicates' draw counts
 *                     are the marginal weights, one float64 exp per replicate, pair and iteration
 *   pfm_perm_labels   random relabellings of the pooled sample for a permutation test, drawn on the device from a
 *                     counter-based generator, and
 *   pfm_perm_form     the signed pair sum of every relabelling (energy or Gaussian kernel): each pair value is formed once
 *                     per call, one float64 multiply-add per relabelling and pair
 *   pfm_nn_index      every pooled row's k nearest other rows, which rows they are and their squared distances, ordered by
 *                     (distance, row index), and
 *   pfm_nn_count      per labelling, how many (row, neighbour) slots carry the same label on both sides: the
 *                     nearest-neighbour two-sample test, whose neighbour table does not depend on the labelling
 *   pfm_pair_grad     the energy distance's D^2 or the biased MMD^2 of the samples as given TOGETHER WITH its derivative by
 *                     every row, for training on it: one more sweep over the same pair tiles, an [n, d] result
 *   pfm_sinkhorn_grad the debiased Sinkhorn divergence of the samples as given TOGETHER WITH its envelope-theorem derivative
 *                     by every row: a step kernel for the one weighting whose four waves share a strip, then one sweep over
 *                     the pair tiles with one float64 exp per pair
 *   pfm_slice_grad    the sliced Wasserstein distance of the samples as given TOGETHER WITH its derivative by every row: per
 *                     direction a (value, row) sort of each sample in LDS, the quantile coupling of the two sorted samples and
 *                     its gradient, O(P n log n) where the three above walk n^2 pairs
 *   pfm_score_grad    per row, the energy score of the row's K draws against the row's target TOGETHER WITH its derivative by
 *                     every draw and by the target: the loss a conditional sampler is trained on, one sweep over each row's
 *                     K (K - 1) / 2 pairs in LDS; pfm_score_plan says how a shape is tiled
 *   pfm_variogram_grad per row, the variogram score of the row's K draws against the row's target TOGETHER WITH its derivative by
 *                     every draw and by the target: the score that reacts to the dependence between the features; a row's
 *                     d (d - 1) / 2 pair terms stay in LDS; pfm_variogram_plan says how a shape is tiled
 *   pfm_sort_score    per (row, feature) series, the CRPS of the series' K draws against its target TOGETHER WITH its derivative
 *                     by every draw and by the target, and the pinball scores of the draws' empirical quantiles: a (value, draw)
 *                     sort of the series in LDS and one pass, O(K log^2 K) where pfm_score_grad walks K^2 / 2 pairs;
 *                     pfm_sort_score_plan says how a shape is tiled
 *   pfm_pinball_grad  the derivative of those pinball scores by every draw and by the target, from the two order statistics
 *                     pfm_sort_score names per level
 *   pfm_sym_eig       eigenvalues and eigenvectors of a batch of real symmetric matrices of up to 64 rows: cyclic Jacobi in a
 *                     parallel order, one workgroup per matrix, the matrix and its eigenvectors in LDS
 *   pfm_frechet_grad  the Frechet distance of the samples as given, the trace of the matrix square root included, TOGETHER WITH
 *                     its derivative by every row: the moments of pfm_boot_moments, two eigen-decompositions per route in one
 *                     workgroup, and one row kernel, O(n d^2); the gradient of a spectral function needs no eigenvector derivative
 *
 * Conventions (as include/rnvp_hip.h)
 *   - every pointer is a DEVICE pointer (but pfm_pair_grad's `gammas` and the `levels` of pfm_sort_score and
 *     pfm_pinball_grad); sizes are plain integers;
 *   - the caller owns all device memory including the workspace (no hidden hipMalloc);
 *     *_workspace_bytes() says how much a call needs;
 *   - kernels are enqueued on `stream` (a hipStream_t passed as void*) and the call
 *     returns without synchronising;
 *   - return value: 0 ok; <0 argument error (PFM_E*); >0 a hipError_t;
 *   - no global mutable state.  Reductions run in a fixed order with no float atomics:
 *     the same inputs give bitwise the same outputs.
 *
 * Data layout
 *   X [nx, d], Y [ny, d]: float64 row-major.
 *   idx_x [reps, nx], idx_y [reps, ny]: int32 bootstrap indices, replicate r resamples row
 *   idx_x[r * nx + i] of X as its row i (sklearn.utils.resample; never materialised).
 */
#ifndef PF_METRICS_H
#define PF_METRICS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PFM_OK            0
#define PFM_EINVAL       (-1)   /* NULL pointer, non-positive size, index range       */
#define PFM_EUNSUPPORTED (-2)   /* d too large for the moments kernels' LDS row tile;
                                   a Wasserstein order or Sinkhorn cost power p other than 1 or 2;
                                   nearest_k above PFM_KNN_MAX_K; k above PFM_NN_MAX_K;
                                   a sample above PFM_SLICE_LDS_ROWS without perm_in;
                                   d above PFM_FRECHET_MAX_D in pfm_sym_eig, pfm_frechet_grad */
#define PFM_EWORKSPACE   (-3)   /* workspace smaller than *_workspace_bytes() says      */

#define PFM_VERSION 101         /* pfm_version(): bumped whenever an argument list changes */

#define PFM_MOMENTS_MAX_D 4096  /* one centred row must fit the 32 KB LDS row tile      */

int         pfm_version(void);
const char *pfm_status_string(int status);

/* bytes of workspace pfm_mmd needs for `reps` replicates of an nx + ny row pooled sample */
size_t pfm_mmd_workspace_bytes(int64_t nx, int64_t ny, int64_t d, int64_t reps);

/*
 * `reps` MMD replicates.  For replicate r, with Z = [X[idx_x[r]]; Y[idx_y[r]]] (m = nx + ny rows):
 *   median[r] = np.median of the m x m Euclidean distance matrix of Z (its m diagonal zeros
 *               and every pair i < j twice included): the mean of the order statistics of rank
 *               (m*m - 1) / 2 and m*m / 2, selected exactly among the kernel's own d^2 values;
 *   mmd[r]    = mean K_XX + mean K_YY - 2 mean K_XY,  K = exp(-gamma d^2), gamma = 1 / (2 median^2),
 *               diagonals of K_XX and K_YY included.
 * A replicate whose median is 0 gets mmd = NaN (the reference raises; the caller checks `median`).
 */
int pfm_mmd(void *stream, const double *X, int64_t nx, const double *Y, int64_t ny, int64_t d,
            const int32_t *idx_x, const int32_t *idx_y, int64_t reps,
            double *median, double *mmd, void *workspace, size_t workspace_bytes);

/* bytes of workspace pfm_boot_moments needs */
size_t pfm_moments_workspace_bytes(int64_t nr, int64_t nf, int64_t d, int64_t reps);

/*
 * Mean and covariance (np.cov(rowvar=False), ddof 1, two passes: the mean, then the centred
 * products) of each resampled set: job j = 2 r + s, s = 0 for Xr[idx_r[r]], 1 for Xf[idx_f[r]].
 *   mean [reps, 2, d]      cov [reps, 2, d, d] (symmetric, both triangles written)
 */
int pfm_boot_moments(void *stream, const double *Xr, int64_t nr, const double *Xf, int64_t nf, int64_t d,
                     const int32_t *idx_r, const int32_t *idx_f, int64_t reps,
                     double *mean, double *cov, void *workspace, size_t workspace_bytes);

/* ---- 1-D metrics (pf_metrics1d.hip) ------------------------------------------------------ */

/* what pfm_metric1d writes per (replicate r, feature f); rf = r * d + f */
#define PFM_M1D_KS    0   /* double  out[rf]: the ks_2samp statistic                              */
#define PFM_M1D_CVM   1   /* int64   out[2 rf + s]: sum_i (2 R_i - 2 i)^2 over sample s's sorted
                             rows (R the pooled average rank, i = 1..n_s); pooled N <= 2^20        */
#define PFM_M1D_AD    2   /* double  out[3 rf + s]: scipy's midrank `inner` summed over the distinct
                             pooled values for sample s; out[3 rf + 2]: the number of those values */
#define PFM_M1D_AUC   3   /* int64   out[rf]: 2 U, U = pairs (real, fake) with fake > real, ties 1/2 */
#define PFM_M1D_HIST  4   /* int32   out[(2 rf + s) bins + k]: np.histogram counts of sample s in
                             the bins of np.histogram(pooled, bins)                               */
#define PFM_M1D_KDE   5   /* double  out[(2 rf + s) bins + k]: log sum_i exp(-(x_k - v_i)^2 / (2 h_s^2))
                             over sample s's resampled values v_i, x = linspace(min, max, bins) of
                             the pooled replicate; the caller adds the kernel norm and -log n_s   */

/* bytes of workspace pfm_metric1d needs (0: the arguments are invalid) */
size_t pfm_metric1d_workspace_bytes(int metric, int64_t nr, int64_t nf, int64_t d, int64_t reps, int64_t bins);

/*
 * `reps` replicates of one 1-D statistic, every feature.  N = nr + nf pooled rows: real rows
 * 0 .. nr-1, fake rows nr .. N-1.  Per call (not per replicate) the caller provides, per feature f:
 *   cols    [d, N] float64   the pooled original column f
 *   perm    [d, N] int32     pooled rows in ascending order of cols[f]
 *   gstart  [d, N + 1] int32 tie groups (runs of equal values) of that order: group g is sorted
 *                            positions gstart[f, g] .. gstart[f, g + 1] - 1, g < ngroups[f];
 *                            gstart[f, ngroups[f]] = N
 *   ngroups [d] int32
 * idx_r [reps, nr] / idx_f [reps, nf] are the bootstrap indices (as pfm_boot_moments); `bins`
 * matters for HIST / KDE, h_r / h_f (the samples' bandwidths) for KDE only.  `out` is laid out
 * as the PFM_M1D_* comment says; HIST zeroes its counts itself.
 * Returns PFM_EUNSUPPORTED for CVM with N > 2^20.
 */
int pfm_metric1d(void *stream, int metric, const double *cols, const int32_t *perm, const int32_t *gstart,
                 const int32_t *ngroups, int64_t nr, int64_t nf, int64_t d, const int32_t *idx_r,
                 const int32_t *idx_f, int64_t reps, int64_t bins, double h_r, double h_f, void *out,
                 void *workspace, size_t workspace_bytes);

/* ---- Wasserstein distances (pf_wasserstein.hip) ------------------------------------------- */

/*
 * The pooled columns of n_proj projections: cols[k, i] = sum_j Z[i, j] theta[k, j] with Z = [Xr; Xf]
 * (real rows first), cols [n_proj, nr + nf], theta [n_proj, d], all float64 row-major.  The sum
 * starts at 0 and runs over j in order, the product and the sum rounded separately (no fma).
 */
int pfm_project(void *stream, const double *Xr, int64_t nr, const double *Xf, int64_t nf, int64_t d,
                const double *theta, int64_t n_proj, double *cols);

/* bytes of workspace pfm_wasserstein1d needs (0: the arguments are invalid, p not 1 or 2 included) */
size_t pfm_wasserstein1d_workspace_bytes(int64_t nr, int64_t nf, int64_t d, int64_t reps, int p);

/*
 * `reps` replicates, every column: out[r * d + f] = W_p^p = int_0^1 |Q_r(u) - Q_f(u)|^p du between the
 * empirical distributions of the two resampled columns (for p = 1 scipy.stats.wasserstein_distance);
 * the caller takes the p-th root.  cols / perm / gstart / ngroups, idx_r / idx_f as pfm_metric1d.
 * Returns PFM_EUNSUPPORTED for a p other than 1 or 2.
 */
int pfm_wasserstein1d(void *stream, int p, const double *cols, const int32_t *perm, const int32_t *gstart,
                      const int32_t *ngroups, int64_t nr, int64_t nf, int64_t d, const int32_t *idx_r,
                      const int32_t *idx_f, int64_t reps, double *out, void *workspace, size_t workspace_bytes);

/* ---- k-NN precision, recall, density, coverage (pf_knn.hip) ---------------------------------- */

#define PFM_KNN_MAX_K 16        /* nearest_k: the per-thread candidate lists live in registers */

/* bytes of workspace pfm_prdc needs (0: the arguments are invalid, k above PFM_KNN_MAX_K included, or a size overflows) */
size_t pfm_prdc_workspace_bytes(int64_t nr, int64_t nf, int64_t d, int64_t reps, int64_t k);

/*
 * `reps` replicates of the k-nearest-neighbour counts behind improved precision / recall (Kynkaanniemi et al. 2019) and
 * density / coverage (Naeem et al. 2020).  With R = Xr[idx_r[r]], F = Xf[idx_f[r]] and D2 the SQUARED Euclidean distance
 * accumulated as fma(df, df, acc) over the features in order (no square root anywhere, no norm / dot-product identity):
 *   radius2_r[r, i] = the (k + 1)-th smallest value of row i of D2(R, R), the diagonal 0 and the zeros of duplicated
 *                     rows included (np.partition(row, k)[k]); radius2_f[r, j] the same inside F
 *   c[j] = #{i : D2(R_i, F_j) < radius2_r[i]},  cov[i] = any_j D2(R_i, F_j) < radius2_r[i],
 *   rec[i] = any_j D2(R_i, F_j) < radius2_f[j]                                  (strict <, as the prdc package)
 *   counts[r] = { P = #{j : c[j] > 0}, Rc = #{i : rec[i]}, Dn = sum_j c[j], Cv = #{i : cov[i]} }
 * precision = P / nf, recall = Rc / nr, density = Dn / (k nf), coverage = Cv / nr are left to the caller.
 * radius2_r [reps, nr], radius2_f [reps, nf], counts [reps, 4].  PFM_EINVAL for k < 1 or k >= min(nr, nf),
 * PFM_EUNSUPPORTED for k > PFM_KNN_MAX_K.
 */
int pfm_prdc(void *stream, const double *Xr, int64_t nr, const double *Xf, int64_t nf, int64_t d,
             const int32_t *idx_r, const int32_t *idx_f, int64_t reps, int64_t k,
             double *radius2_r, double *radius2_f, int64_t *counts, void *workspace, size_t workspace_bytes);

/* ---- energy distance (pf_energy.hip) ----------------------------------------------------------- */

#define PFM_ENERGY_TILE 64      /* rows per side of a pair tile: a tile lies inside one of the blocks RR, FF, RF */
#define PFM_ENERGY_REP_BLOCK 16 /* replicates whose draw counts are staged and multiplied at a time */

/* bytes of workspace pfm_energy needs: the draw counts and the workgroups' partial sums (0: the arguments are invalid or a
   size overflows) */
size_t pfm_energy_workspace_bytes(int64_t nr, int64_t nf, int64_t d, int64_t reps);

/*
 * `reps` replicates of the three raw pair sums of the energy distance (Szekely & Rizzo), V-statistic: with R = Xr[idx_r[r]],
 * F = Xf[idx_f[r]] and |.| the Euclidean norm, the squared distance accumulated as fma(df, df, acc) over the features in
 * order and one sqrt (no norm / dot-product identity: duplicated rows are at distance exactly 0),
 *   sums[r] = { Srr = sum_a sum_b |R_a - R_b|,  Sff = sum_a sum_b |F_a - F_b|,  Srf = sum_a sum_b |R_a - F_b| }
 * over all ordered pairs, the zero diagonals of Srr and Sff included.  D^2 = 2 Srf / (nr nf) - Srr / nr^2 - Sff / nf^2 is
 * left to the caller.  Computed as sum_ab c[a] c[b] |z_a - z_b| over the ORIGINAL rows with the replicate's draw counts c;
 * the order of summation depends on (nr, nf) only, so a replicate's sums are bitwise the same in any call.  Every element
 * of sums [reps, 3] is written.
 */
int pfm_energy(void *stream, const double *Xr, int64_t nr, const double *Xf, int64_t nf, int64_t d,
               const int32_t *idx_r, const int32_t *idx_f, int64_t reps, double *sums, void *workspace,
               size_t workspace_bytes);

/* ---- Sinkhorn divergence (pf_sinkhorn.hip) --------------------------------------------------------- */

/* bytes of workspace pfm_sinkhorn needs: the draw counts, their logarithms and three buffers of potentials, 60 bytes per
   replicate and pooled row; nothing of the size of the pair matrix (0: the arguments are invalid or a size overflows) */
size_t pfm_sinkhorn_workspace_bytes(int64_t nr, int64_t nf, int64_t d, int64_t reps);

/*
 * `reps` replicates of the debiased Sinkhorn divergence (Genevay et al. 2018; Feydy et al. 2019) between the resampled sets,
 * taken as the ORIGINAL rows with weights a = count_r / nr, b = count_f / nf.  Cost C(x, y) = |x - y|^p, p = 1 or 2, from the
 * squared distance of pfm_energy (fma(df, df, acc) over the features in order; one sqrt for p = 1: a duplicated row costs
 * exactly 0).  With
 *   softmin(h, C, w)[i] = -eps log sum_j w_j exp((h_j - C_ij) / eps)      over the columns of non-zero weight, evaluated with
 * the row's running maximum subtracted, four potentials start at 0: f (on R, against F), g (on F, against R), u (on R, against
 * R), v (on F, against F).  Each of n_sinkhorn iterations replaces all four from the previous iteration's values,
 *   f <- (f + softmin(g, C_RF, b)) / 2     g <- (g + softmin(f, C_FR, a)) / 2
 *   u <- (u + softmin(u, C_RR, a)) / 2     v <- (v + softmin(v, C_FF, b)) / 2
 * and one last step takes the same four softmins without the averaging, again from the old values.  Then
 *   value[r] = sum_i a_i (f_i - u_i) + sum_j b_j (g_j - v_j)            over the rows of non-zero count
 *   drift[r] = the largest |change| of a potential of such a row in the last averaged step (0 for n_sinkhorn = 0)
 *   potentials[r, 0] = (f, g), potentials[r, 1] = (u, v) after the last step, on the pooled rows (real rows first), the finite
 *                      potentials of rows of count 0 included; potentials may be NULL.
 * One launch per step, n_sinkhorn + 1 in all; a step costs one float64 exp per replicate and pooled pair.  The order of every sum
 * depends on (nr, nf, d) only, so a replicate's outputs are bitwise the same alone, in any group, in any call.  value [reps],
 * drift [reps], potentials [reps, 2, nr + nf]; every element is written.
 * PFM_EINVAL for bad sizes, reps > 65535, an eps that is not positive and finite (or whose reciprocal is not), n_sinkhorn < 0 or
 * above 1000000; PFM_EUNSUPPORTED for a p other than 1 or 2; on any error nothing is written.
 */
int pfm_sinkhorn(void *stream, const double *Xr, int64_t nr, const double *Xf, int64_t nf, int64_t d,
                 const int32_t *idx_r, const int32_t *idx_f, int64_t reps, int p, double eps, int64_t n_sinkhorn,
                 double *value, double *drift, double *potentials, void *workspace, size_t workspace_bytes);

/* ---- permutation two-sample tests (pf_perm.hip) -------------------------------------------------- */

#define PFM_PERM_ENERGY 0       /* G(a, b) = |z_a - z_b|, formed as pfm_energy forms it */
#define PFM_PERM_GAUSS  1       /* G(a, b) = exp(-(gamma |z_a - z_b|^2)) of the same squared distance */

/* bytes of workspace pfm_perm_labels needs: nothing is kept there, the figure is the least a caller can allocate (0: the
   arguments are invalid) */
size_t pfm_perm_labels_workspace_bytes(int64_t reps, int64_t n, int64_t n_first);

/*
 * `reps` random labellings of n pooled rows with exactly n_first ones each, labels [reps, n] (every byte written, 0 or 1).
 * Labelling r of the call has the global index p = first_perm + r, and depends on (seed, key_mask, p, n, n_first) only: it is
 * the same bytes whatever call or group makes it.  Row a's sort key is
 *   (w0 | w1 << 32) & key_mask,   (w0, w1, w2, w3) = Philox4x32-10(counter (a, 0, p, 0), key (seed & 0xffffffff, seed >> 32)),
 * and row a gets label 1 iff its rank in ascending lexicographic order of (key, a) is below n_first.  key_mask is all ones in
 * use; a narrow mask forces ties (3: n / 4-fold), and 0 orders by index alone: rows 0 .. n_first - 1 get the ones.
 * 1 <= n_first < n <= 2^31 - 1, 0 <= first_perm, first_perm + reps <= 2^32.
 */
int pfm_perm_labels(void *stream, uint64_t seed, uint64_t key_mask, int64_t first_perm, int64_t reps,
                    int64_t n, int64_t n_first, uint8_t *labels, void *workspace, size_t workspace_bytes);

/* bytes of workspace pfm_perm_form needs: the workgroups' partial sums (0: the arguments are invalid or a size overflows) */
size_t pfm_perm_form_workspace_bytes(int64_t n, int64_t d, int64_t n_first, int64_t reps);

/*
 * The signed quadratic form of `reps` labellings of the pooled sample Z [n, d] (the first sample's n_first rows, then the
 * second's n - n_first): with s[r, a] = +(n - n_first) where labels[r, a] is non-zero and -n_first otherwise (integers, exact
 * in float64),
 *   S[r] = sum_a sum_b s[r, a] s[r, b] G(a, b)   over all ordered pairs, the diagonal included,
 * G as `kind` says (gamma matters for PFM_PERM_GAUSS only and must then be positive and finite).  With the observed labelling
 * (a < n_first) the caller gets the energy distance's D^2 = -S / (n_first (n - n_first))^2 and the biased
 * MMD^2 = +S / (n_first (n - n_first))^2 of the samples as given.  The order of summation depends on (n, d) only, so a
 * labelling's S is bitwise the same alone, in any group, in any call.  Every element of S [reps] is written.
 * PFM_EUNSUPPORTED for another kind.
 */
int pfm_perm_form(void *stream, int kind, double gamma, const double *Z, int64_t n, int64_t d, int64_t n_first,
                  const uint8_t *labels, int64_t reps, double *S, void *workspace, size_t workspace_bytes);

/* ---- differentiable two-sample losses (pf_pairgrad.hip) ------------------------------------------- */

#define PFM_PAIR_MAX_GAMMAS 8   /* Gaussians in the kernel sum of PFM_PERM_GAUSS */

/* bytes of workspace pfm_pair_grad needs: the workgroups' value partials and the column slices' gradient partials
   [slices, n, d]; the number of slices depends on (n, d) only and nothing of the size of the pair matrix is kept (0: the
   arguments are invalid or a size overflows) */
size_t pfm_pair_grad_workspace_bytes(int64_t n, int64_t d, int64_t n_first);

/*
 * The value and the row gradients of a two-sample statistic of the pooled sample Z [n, d] (the first sample's n_first rows,
 * then the second's n - n_first): with w[a] = +1 / n_first on a first row and -1 / (n - n_first) otherwise, and d2(a, b) the
 * squared distance of the other entry points (fma(df, df, acc) over the features in order),
 *   value[0]   = sum_a sum_b w[a] w[b] g(d2(a, b))                       over all ordered pairs, the diagonal included
 *   grad[a, k] = 2 w[a] sum_b w[b] c(d2(a, b)) (Z[a, k] - Z[b, k])       = d value / d Z[a, k]
 *   PFM_PERM_ENERGY  g = -sqrt(d2),  c = -1 / sqrt(d2), and exactly 0 where d2 == 0 (a coincident pair adds nothing)
 *   PFM_PERM_GAUSS   g = sum_m exp(-(gammas[m] d2)),  c = -2 sum_m gammas[m] exp(-(gammas[m] d2)),  m < n_gamma
 * so value is the energy distance's D^2 (V-statistic) or the biased MMD^2 of a sum of Gaussians.  The differences are taken
 * feature by feature on the rows themselves: duplicated rows add exactly 0 to each other's gradient, at any offset of the data.
 * gammas is the one HOST pointer of this header: n_gamma <= PFM_PAIR_MAX_GAMMAS positive finite values, read before the call
 * returns and handed to the kernel by value (ignored for PFM_PERM_ENERGY, where it may be NULL).  grad [n, d] may be NULL:
 * then only the value is formed.  Nothing is checked for NaN or infinity: they propagate.  The order of every sum depends on
 * (n, d) only, so the outputs are bitwise the same in any call.  value [1] and every element of grad are written.
 * PFM_EINVAL for n < 2, d < 1, n_first outside 1 .. n - 1, a bad n_gamma or gamma; PFM_EUNSUPPORTED for another kind; on any
 * error nothing is written.
 */
int pfm_pair_grad(void *stream, int kind, const double *gammas, int n_gamma, const double *Z, int64_t n, int64_t d,
                  int64_t n_first, double *value, double *grad, void *workspace, size_t workspace_bytes);

/* ---- differentiable Sinkhorn divergence (pf_sinkgrad.hip) ------------------------------------------- */

/* bytes of workspace pfm_sinkhorn_grad needs: three buffers of potentials and the column slices' gradient partials
   [slices, n, d]; a function of (n, d) only, nothing of the size of the pair matrix (0: the arguments are invalid or a size
   overflows) */
size_t pfm_sinkhorn_grad_workspace_bytes(int64_t n, int64_t d, int64_t n_first);

/*
 * The debiased Sinkhorn divergence of the pooled sample Z [n, d] (the first sample's nr = n_first rows, then the second's
 * nf = n - n_first) with the uniform weights a_i = 1 / nr, b_j = 1 / nf, and its row gradients.  Cost, softmin and iteration are
 * pfm_sinkhorn's: four potentials start at 0, n_sinkhorn averaged steps from old values, one last plain step, n_sinkhorn + 1
 * launches; the weights enter as the constants -log nr, -log nf, added once per softmin.  With `old` the potentials the last
 * step read and `fin` the ones it wrote, slot = self where rows a and b are of one sample and cross otherwise,
 *   value[0]   = sum_i a_i (f_i - u_i) + sum_j b_j (g_j - v_j)         of fin: pfm_sinkhorn's value of the identity replicate (not
 *                bitwise: the sums run in another order)
 *   drift[0]   = the largest |change| of a potential in the last averaged step (0 for n_sinkhorn = 0)
 *   P_ab       = exp((fin_a[slot] + old_b[slot] - C_ab) / eps) / n_side(b)        (sum_b over one side = 1: no overflow)
 *   grad[a, k] = w_a sum_b sgn_ab P_ab c_p(d2_ab) (Z[a, k] - Z[b, k]),   sgn = +1 cross, -1 self,  w_a = 1 / n_side(a),
 *                c_2 = 2,  c_1 = 1 / sqrt(d2) and exactly 0 where d2 == 0
 * grad differentiates every row's final softmin by that row's own coordinates only, the columns and the incoming potentials
 * held fixed (the envelope theorem): it is the exact derivative of the value at the fixed point of the iteration, NOT the
 * derivative of the n_sinkhorn unrolled steps; drift says how far from the fixed point the call stopped.  The differences are
 * taken feature by feature on the rows themselves, as pfm_pair_grad takes them.
 * grad [n, d] may be NULL: then only value and drift are formed.  potentials [2, 2, n] may be NULL: fin (cross, then self, on the
 * pooled rows), then old.  Nothing is checked for NaN or infinity: they propagate.  The order of every sum depends on
 * (n, n_first, d) only, so the outputs are bitwise the same in any call.  On success every element of every output given is
 * written.
 * PFM_EINVAL for n < 2, d < 1, n_first outside 1 .. n - 1, an eps that is not positive and finite (or whose reciprocal is not),
 * n_sinkhorn < 0 or above 1000000; PFM_EUNSUPPORTED for a p other than 1 or 2; on any error nothing is written.
 */
int pfm_sinkhorn_grad(void *stream, const double *Z, int64_t n, int64_t d, int64_t n_first, int p, double eps,
                      int64_t n_sinkhorn, double *value, double *drift, double *grad, double *potentials, void *workspace,
                      size_t workspace_bytes);

/* ---- differentiable sliced Wasserstein distance (pf_slicegrad.hip) ---------------------------------- */

#define PFM_SLICE_LDS_ROWS 13312    /* rows per SAMPLE that pfm_slice_grad sorts itself: (float64 value, int32 row) pairs of one
                                       sample and direction in the 160 KiB of LDS of one CU, 12 bytes each (156 KiB) */

/* bytes of workspace pfm_slice_grad needs: per direction the sorted projections, their rows and the derivatives by the
   projections, 20 bytes per direction and pooled row, and the workgroups' value partials (0: the arguments are invalid or a size
   overflows) */
size_t pfm_slice_grad_workspace_bytes(int64_t n, int64_t d, int64_t n_first, int64_t n_proj);

/*
 * The sliced Wasserstein distance (without the p-th root) of the pooled sample Z [n, d] (the first sample's nr = n_first rows, then
 * the second's nf = n - n_first) over the directions theta [n_proj, d], and its row gradients.  Per direction k:
 *   u_k[a]  = sum_j Z[a, j] theta[k, j] as pfm_project forms it (the sum starts at 0 and runs over j in order, product and sum
 *             rounded separately).  theta may be NULL: the coordinate axes, n_proj must equal d and u_k[a] = Z[a, k], copied, so
 *             an infinity in another feature does not reach column k;
 *   order   each sample's rows ascending by (u_k, pooled row index): what a stable ascending sort gives;
 *   W_k     = sum_ij ov_ij / (nr nf) |us_i - vs_j|^p over the sorted values us, vs: on a grid of nr nf cells sorted real element i
 *             covers [i nf, (i + 1) nf), sorted fake element j covers [j nr, (j + 1) nr) and ov_ij is their overlap, positive for
 *             nr + nf - gcd(nr, nf) pairs;
 *   g_k     the derivative of W_k by u_k: sum_j ov_ij / (nr nf) c_ij on sorted real element i's row and -sum_i of the same on sorted
 *             fake element j's, c = sign(us_i - vs_j) for p = 1 (exactly 0 on a coincidence), 2 (us_i - vs_j) for p = 2.  Among tied
 *             projections the (value, index) order decides who meets whom: a valid subgradient, and deterministic.
 *   value[0]   = (1 / n_proj) sum_k W_k
 *   rows[a, :] = (1 / n_proj) sum_k g_k[a] theta[k, :], k ascending                = d value / d Z[a, :]
 * perm_in NULL: the call sorts, in LDS; both samples must have at most PFM_SLICE_LDS_ROWS rows, else PFM_EUNSUPPORTED.  perm_in
 * [n_proj, n] given: per direction the real rows in order, then the fake rows in order, as pooled row indices; it is taken as given
 * (that it is such a permutation is the caller's duty; an entry outside [0, n) is read as the nearest row inside), for any n.
 * rows [n, d] may be NULL: then only the value is formed.  cols_out [n_proj, n] (the projections u_k, on the pooled rows) and
 * perm_out [n_proj, n] (the order used, laid out as perm_in) may be NULL.  theta is a constant: no derivative by it is formed.
 * Nothing is checked for NaN or infinity: they propagate into the value, and the sort's network does not depend on the data.  No
 * float atomics; the order of every sum depends on (n, n_first, n_proj) only, so the outputs are bitwise the same in any call.  On
 * success every element of every output given is written.
 * PFM_EINVAL for n < 2, d < 1, n_first outside 1 .. n - 1, n_proj outside 1 .. 65535, n >= 2^31, theta NULL with n_proj != d, a
 * NULL Z or value; PFM_EUNSUPPORTED for a p other than 1 or 2; on any error nothing is written.
 */
int pfm_slice_grad(void *stream, int p, const double *Z, int64_t n, int64_t d, int64_t n_first, const double *theta,
                   int64_t n_proj, const int32_t *perm_in, double *value, double *rows, double *cols_out, int32_t *perm_out,
                   void *workspace, size_t workspace_bytes);

/* ---- differentiable per-row scoring rule: the energy score of K draws (pf_scoregrad.hip) ------------ */

#define PFM_SCORE_MAX_K 1024        /* draws per row of pfm_score_grad: a lane owns at most four of them */
#define PFM_SCORE_MAX_KD 16384      /* K d of pfm_score_grad: a row's draws as float64 in 128 KiB of the 160 KiB of LDS of one CU */

/* bytes of workspace pfm_score_grad needs: nothing is kept there, the figure is the least a caller can allocate (0: the arguments
   are invalid or outside the limits) */
size_t pfm_score_grad_workspace_bytes(int64_t n, int64_t K, int64_t d);

/*
 * How pfm_score_grad tiles a call of n rows, K draws and d features; needs no device.  plan is a HOST array of 4:
 *   plan[0]  R: the consecutive rows of a workgroup (for every draw, one contiguous run of R d doubles of X and of grad_x)
 *   plan[1]  S: the lanes that share one row, a power of two, min(256, the least >= K); 256 / S rows are in flight at a time
 *            (fewer where LDS holds fewer), and a lane owns ceil(K / S) draws.  S < 256: rows packed into the waves (the
 *            streaming regime of a few draws); S = 256: a workgroup per row at a time (the pair walk of many draws)
 *   plan[2]  the dynamic LDS bytes of a workgroup, at most 163840
 *   plan[3]  the workgroups, ceil(n / R)
 * R depends on n (fewer rows per workgroup while the workgroups are few); no output of pfm_score_grad does.
 * The statuses are pfm_score_grad's for the sizes; PFM_EINVAL for a NULL plan.
 */
int pfm_score_plan(int64_t n, int64_t K, int64_t d, int64_t *plan);

/*
 * The energy score (Gneiting & Raftery 2007) of every row's K draws against the row's target, and its derivatives.  X [K, n, d]
 * holds draw k of row i at X[k, i, :], Y [n, d] the targets.  Per row, with x_k = X[k, i, :], y = Y[i, :] and D = K - 1 if fair
 * else K:
 *   T1        = (1 / K) sum_k |x_k - y|_2
 *   spread[i] = 1 / (2 K D) sum_k sum_l |x_k - x_l|_2           (every unordered pair's distance is formed once)
 *   scores[i] = T1 - spread[i]
 *   grad_x[k, i, :] = (1 / K) c_k (x_k - y) - (1 / (K D)) sum_l c_kl (x_k - x_l)        = d scores[i] / d X[k, i, :]
 *   grad_y[i, :]    = -(1 / K) sum_k c_k (x_k - y)                                      = d scores[i] / d Y[i, :]
 * c = 1 / distance and exactly 0 where the squared distance is exactly 0 (the subgradient); the squared distance is
 * fma(df, df, acc) over the features in order, df the difference of the values themselves: no norm / dot-product identity, so
 * draws centred far from the origin lose nothing and duplicated draws add exactly 0 to each other.
 * spread [n], grad_x [K, n, d] and grad_y [n, d] may each be NULL; with both gradients NULL only the values are formed.
 * Nothing is checked for NaN or infinity: they propagate inside their row and reach no other row.  No float atomics, and nothing is
 * kept in the workspace; the order of every sum depends on (K, d) only, so a row's outputs are bitwise the same at any position of
 * the row, for any n, in any call.  On success every element of every output given is written.
 * PFM_EINVAL for n, K or d < 1, n >= 2^31, fair != 0 with K = 1, a NULL X, Y or scores; PFM_EUNSUPPORTED for K > PFM_SCORE_MAX_K
 * or K d > PFM_SCORE_MAX_KD; PFM_EWORKSPACE for a missing or short workspace; on any error nothing is written.
 */
int pfm_score_grad(void *stream, const double *X, const double *Y, int64_t n, int64_t K, int64_t d, int fair, double *scores,
                   double *spread, double *grad_x, double *grad_y, void *workspace, size_t workspace_bytes);

/* ---- differentiable per-row scoring rule: the variogram score of K draws (pf_variogram.hip) -------- */

#define PFM_VARIO_MAX_D 64          /* features of pfm_variogram_grad: a row's d (d - 1) / 2 pair terms stay in LDS beside its draws */

/* bytes of workspace pfm_variogram_grad needs: nothing is kept there, the figure is the least a caller can allocate (0: the
   arguments are invalid or outside the limits) */
size_t pfm_variogram_grad_workspace_bytes(int64_t n, int64_t K, int64_t d);

/*
 * How pfm_variogram_grad tiles a call of n rows, K draws and d features; needs no device.  plan is a HOST array of 6:
 *   plan[0]  R: the consecutive rows of a workgroup (for every draw, one contiguous run of R d doubles of X and of grad_x)
 *   plan[1]  S: the lanes that share one row, a power of two, min(256, the least >= K); a lane owns ceil(K / S) draws
 *   plan[2]  the dynamic LDS bytes of a workgroup, at most 163840
 *   plan[3]  the workgroups, ceil(n / R)
 *   plan[4]  G: the rows in flight at a time, 256 / S or fewer where LDS holds fewer (every one keeps its pair table there)
 *   plan[5]  T: the slices the draws are cut into while a row's pair sums are formed, S / (d (d - 1) / 2) where that is above 1
 * d = 1 has no pair: a lane per row, R = G = 256, S = T = 1, no LDS.
 * R depends on n (fewer rows per workgroup while the workgroups are few); no output of pfm_variogram_grad does.
 * The statuses are pfm_variogram_grad's for the sizes; PFM_EINVAL for a NULL plan.
 */
int pfm_variogram_plan(int64_t n, int64_t K, int64_t d, int64_t *plan);

/*
 * The variogram score (Scheuerer & Hamill 2015) of every row's K draws against the row's target, and its derivatives.  X [K, n, d]
 * holds draw k of row r at X[k, r, :], Y [n, d] the targets, W [d, d] the weights (NULL: all 1; used as given, symmetric or not,
 * of either sign).  Per row, with x_k = X[k, r, :], y = Y[r, :] and order p = 0.5, 1 or 2:
 *   v_ij = |y_i - y_j|^p,   m_ij = (1 / K) sum_k |x_ki - x_kj|^p,   r_ij = v_ij - m_ij
 *   scores[r]       = sum_i sum_j W_ij r_ij^2                                            (formed as sum_{i < j} (W_ij + W_ji) r_ij r_ij)
 *   grad_x[k, r, i] = -(2 / K) sum_j (W_ij + W_ji) r_ij h(x_ki - x_kj)                   = d scores[r] / d X[k, r, i]
 *   grad_y[r, i]    =  2       sum_j (W_ij + W_ji) r_ij h(y_i - y_j)                     = d scores[r] / d Y[r, i]
 *   h(t) = 2 t (p = 2);  sgn t (p = 1);  sgn t / (2 sqrt|t|) (p = 0.5);  for p = 1 and 0.5 exactly 0 at t = 0 (the subgradient: no
 *   0 times infinity is formed).  For p = 0.5 h grows without bound as two coordinates of a draw approach each other.
 * |.|^p is a square root, the identity or a square, never pow, and every difference is taken on the values themselves.
 * grad_x [K, n, d] and grad_y [n, d] may each be NULL; with both NULL only the values are formed.
 * Nothing is checked for NaN or infinity: a NaN in a row's draws or target makes that row's score and all its gradients NaN and
 * reaches no other row.  No float atomics, and nothing is kept in the workspace; the order of every sum depends on (K, d) only, so a
 * row's outputs are bitwise the same at any position of the row, for any n, in any call, whichever outputs are asked for.  On
 * success every element of every output given is written.
 * PFM_EINVAL for n, K or d < 1, n >= 2^31, an order other than 0.5, 1 or 2, a NULL X, Y or scores; PFM_EUNSUPPORTED for
 * d > PFM_VARIO_MAX_D, K > PFM_SCORE_MAX_K or K d > PFM_SCORE_MAX_KD; PFM_EWORKSPACE for a missing or short workspace; on any error
 * nothing is written.
 */
int pfm_variogram_grad(void *stream, const double *X, const double *Y, const double *W, int64_t n, int64_t K, int64_t d,
                       double order, double *scores, double *grad_x, double *grad_y, void *workspace, size_t workspace_bytes);

/* ---- differentiable per-series scoring rules from the sorted draws: CRPS and pinball (pf_sortscore.hip) ---- */

#define PFM_SORT_MAX_K 8192         /* draws per series of pfm_sort_score: a series' (value, draw) pairs and ranks in the LDS of one CU */
#define PFM_SORT_MAX_Q 16           /* quantile levels of pfm_sort_score and pfm_pinball_grad: they travel as kernel arguments */

/* bytes of workspace pfm_sort_score and pfm_pinball_grad need: nothing is kept there, the figure is the least a caller can
   allocate (0: the arguments are invalid or outside the limits) */
size_t pfm_sort_score_workspace_bytes(int64_t M, int64_t K, int64_t n_levels);

/*
 * How pfm_sort_score tiles a call of M series of K draws; needs no device.  plan is a HOST array of 4:
 *   plan[0]  G: the consecutive series a workgroup stages and sorts at once (for every draw, one contiguous run of G doubles
 *            of X and of grad_x): 3776 / pitch, at least 1
 *   plan[1]  the pitch: doubles between two series in LDS, K | 1: odd, so that staging a draw's run (stride = pitch) and a
 *            lane per series meet every bank once
 *   plan[2]  the dynamic LDS bytes of a workgroup, at most 163840: 16 per entry (float64 value, int32 draw, two int16 ranks)
 *            and the sums' scratch
 *   plan[3]  the workgroups, ceil(M / G)
 * Only plan[3] depends on M; no output of pfm_sort_score depends on any of them.
 * The statuses are pfm_sort_score's for the sizes; PFM_EINVAL for a NULL plan.
 */
int pfm_sort_score_plan(int64_t M, int64_t K, int64_t *plan);

/*
 * The CRPS of every series' K draws against the series' target with its derivatives, and the pinball scores of the draws'
 * empirical quantiles, from the sorted series.  X [K, M] holds draw k of series s at X[k, s] (a [K, n, d] array of draws is M = n d
 * series as it lies), Y [M] the targets.  Per series the shifted draws t_k = x_k - y are sorted by (value, draw index); t_(i) is
 * the i-th of them, lo_i and hi_i the first and the last sorted position of the run of values equal (==) to t_(i), and
 *   c_i = lo_i + hi_i - K + 1 = #{draws below t_(i)} - #{draws above it}                 (2 i - K + 1 without ties)
 * With D = K - 1 if fair else K:
 *   crps[s]      = (1 / K) sum_i |t_(i)| - (1 / (K D)) sum_i c_i t_(i)
 *   grad_x[k, s] = (sgn(t_k) D - c_k) / (K D)          = d crps[s] / d X[k, s]: an integer over an integer, one division
 *   grad_y[s]    = -(sum_k sgn(t_k)) / K               = d crps[s] / d Y[s]
 * sgn(0) = 0: tied draws and a draw on its target get the subgradient pfm_score_grad gives them at d = 1.  The two routes agree to
 * rounding, not bitwise: their sums run in different orders.  A series whose sum of |t| is NaN (a NaN among its draws or in its
 * target) gets NaN for its score and for every element of its gradients; infinities are not treated, they stay in their series.
 * levels is a HOST array of n_levels probabilities in [0, 1] (n_levels <= PFM_SORT_MAX_Q; 0: no quantile output), read before the
 * call returns.  Per level p: h = p (K - 1), i = floor(h) clipped to K - 2 (0 at K = 1), frac = h - i, and
 *   Q_p - y         = lerp(t_(i), t_(i + 1), frac)     numpy's: a + (b - a) frac; b - (b - a) (1 - frac) for frac >= 0.5; a if b == a
 *   side[q, s]      = p - [y < Q_p]
 *   pinball[q, s]   = (y - Q_p) side[q, s]
 *   idx[q, s, 0..1] = the draws (their k) that are t_(i) and t_(i + 1); the same draw twice at K = 1
 * pinball and side are NaN for a series that holds a NaN; its idx are two of its draws.
 * crps [M], grad_x [K, M], grad_y [M], pinball [n_levels, M], side [n_levels, M] and idx [n_levels, M, 2] (int32) may each be NULL.
 * No float atomics, and nothing is kept in the workspace; the order of every sum depends on K only and a series never meets
 * another: its outputs are bitwise the same at any position, for any M, in any call, whichever outputs are asked for.  On success
 * every element of every output given is written.
 * PFM_EINVAL for M or K < 1, M >= 2^31, fair != 0 with K = 1, n_levels < 0, a level outside [0, 1] or NaN, a NULL X or Y, NULL levels
 * with n_levels > 0, pinball, side or idx given with n_levels = 0, or no output at all; PFM_EUNSUPPORTED for K > PFM_SORT_MAX_K or
 * n_levels > PFM_SORT_MAX_Q; PFM_EWORKSPACE for a missing or short workspace; on any error nothing is written.
 */
int pfm_sort_score(void *stream, const double *X, const double *Y, int64_t M, int64_t K, int fair, const double *levels,
                   int n_levels, double *crps, double *grad_x, double *grad_y, double *pinball, double *side, int32_t *idx,
                   void *workspace, size_t workspace_bytes);

/*
 * The derivatives of sum_q sum_s g[q, s] pinball[q, s] by the draws and by the targets, from what pfm_sort_score left: idx
 * [n_levels, M, 2] and side [n_levels, M]; g [n_levels, M] is the incoming weight, levels the HOST array of that call (frac is
 * formed from it as there), read before the call returns.  With w = g[q, s] side[q, s]:
 *   grad_x[idx[q, s, 0], s] += (-w) (1 - frac_q),   grad_x[idx[q, s, 1], s] += (-w) frac_q       for q ascending
 *   grad_y[s]                = sum_q w                                                          for q ascending
 * grad_x [K, M] is zero-filled on `stream` first; one thread owns a series, so two levels that meet on one order statistic add in a
 * fixed order.  An idx outside [0, K) is clamped into it.  grad_x and grad_y may each be NULL, not both; every element of every
 * output given is written.  A series that holds a NaN has a NaN side: its grad_y and the two draws named per level get NaN.
 * PFM_EINVAL for M or K < 1, M >= 2^31, n_levels < 1, a level outside [0, 1] or NaN, a NULL idx, side, g or levels, or no output at
 * all; PFM_EUNSUPPORTED for K > PFM_SORT_MAX_K or n_levels > PFM_SORT_MAX_Q; PFM_EWORKSPACE for a missing or short workspace; on any
 * error nothing is written.
 */
int pfm_pinball_grad(void *stream, const int32_t *idx, const double *side, const double *g, const double *levels, int n_levels,
                     int64_t M, int64_t K, double *grad_x, double *grad_y, void *workspace, size_t workspace_bytes);

/* ---- nearest-neighbour two-sample test (pf_nn.hip) ------------------------------------------------ */

#define PFM_NN_MAX_K 16         /* k of pfm_nn_index: the per-thread lists of (d^2, row) live in registers */
#define PFM_NN_STAGE_MAX_N 262144   /* rows up to which pfm_nn_count keeps a labelling in LDS, one bit per row (32 KB);
                                       above it the label bytes are read from global memory */

/* bytes of workspace pfm_nn_index needs: nothing is kept there, the figure is the least a caller can allocate (0: the
   arguments are invalid, k above PFM_NN_MAX_K included, or a size overflows) */
size_t pfm_nn_index_workspace_bytes(int64_t n, int64_t d, int64_t k);

/*
 * The k nearest OTHER rows of every row of Z [n, d]: nbr[a, r] is the row of rank r < k in ascending order of
 * (d^2, row index), so among equal squared distances the smaller row index comes first, and d2[a, r] its squared distance, the
 * D2 of pfm_prdc: fma(df, df, acc) over the features in order, no square root, no norm / dot-product identity, bitwise what
 * the other entry points form for the pair.  Row a is left out by its index, not by its distance: a duplicate of row a is a
 * neighbour at distance exactly 0.  nbr [n, k] int32, d2 [n, k]; every element is written.
 * PFM_EINVAL for n < 2, d < 1, k < 1, k > n - 1 or n > 2^31 - 1, PFM_EUNSUPPORTED for k > PFM_NN_MAX_K; on any error nothing is
 * written.
 */
int pfm_nn_index(void *stream, const double *Z, int64_t n, int64_t d, int64_t k, int32_t *nbr, double *d2,
                 void *workspace, size_t workspace_bytes);

/* bytes of workspace pfm_nn_count needs: the counts of the slices a labelling's slots are cut into (0: the arguments are
   invalid or a size overflows) */
size_t pfm_nn_count_workspace_bytes(int64_t n, int64_t k, int64_t reps);

/*
 * For each of `reps` labellings of the n rows (labels [reps, n], as pfm_perm_labels writes them), over the n k slots (a, r)
 * of a neighbour table nbr [n, k] (entries in [0, n): the caller's duty):
 *   counts[p, 0] = #{(a, r) : labels[p, a] != 0 and labels[p, nbr[a, r]] != 0}
 *   counts[p, 1] = #{(a, r) : labels[p, a] == 0 and labels[p, nbr[a, r]] == 0}
 * Integer work in a fixed order: a labelling's counts are the same alone, in any group, in any call.  counts [reps, 2] int64,
 * every element written.  n, k, reps >= 1, n <= 2^31 - 1, reps <= 2^31 - 1.
 */
int pfm_nn_count(void *stream, const int32_t *nbr, int64_t n, int64_t k, const uint8_t *labels, int64_t reps,
                 int64_t *counts, void *workspace, size_t workspace_bytes);

/* ---- symmetric eigensolver and the differentiable Frechet distance (pf_frechet.hip) ------------------ */

#define PFM_FRECHET_MAX_D 64        /* rows of a matrix of pfm_sym_eig, features of pfm_frechet_grad: four d x d float64 matrices at a
                                       row pitch of d | 1 fit the 160 KiB of LDS of one CU */
#define PFM_EIG_MAX_SWEEPS 30       /* sweeps after which pfm_sym_eig stops whatever the matrix holds */

/* bytes of workspace pfm_sym_eig needs: nothing is kept there, the figure is the least a caller can allocate (0: the arguments
   are invalid or outside the limits) */
size_t pfm_sym_eig_workspace_bytes(int64_t batch, int64_t d);

/*
 * Eigenvalues and eigenvectors of `batch` real symmetric matrices A [batch, d, d], 1 <= d <= PFM_FRECHET_MAX_D, batch <= 65535.
 * Only the lower triangle and the diagonal of each matrix are read (as np.linalg.eigh does); the matrices need not be positive
 * semi-definite.  w [batch, d]: the eigenvalues, ascending.  V [batch, d, d] (may be NULL): the eigenvectors, V[b, :, i] belongs to
 * w[b, i]; their sign is unspecified.  sweeps [batch] (int32, may be NULL): the sweeps that rotated something.
 * Method: cyclic Jacobi in a parallel (round-robin) order, one workgroup per matrix, A and V in LDS at a row pitch of d | 1 doubles.
 * With m = d rounded up to even a sweep is m - 1 rounds of m / 2 disjoint index pairs (for odd d one index has a bye).  The rotation
 * of the pair p < q is SKIPPED where
 *   |a_pq| <= 2^-53 sqrt|a_pp| sqrt|a_qq|                      (the relative criterion of Demmel & Veselic 1992)
 * and else taken from tau = (a_qq - a_pp) / (2 a_pq), t = sgn(tau) / (|tau| + sqrt(1 + tau^2)), c = 1 / sqrt(1 + t^2), s = t c; the
 * pair's new diagonal is a_pp - t a_pq, a_qq + t a_pq and its a_pq exactly 0.  The loop ends after a sweep in which every rotation
 * was skipped and after PFM_EIG_MAX_SWEEPS sweeps at the latest, so the call terminates on any input: a diagonal matrix takes 0
 * sweeps; a NaN compares false with the threshold, so a matrix that holds one in the triangle read (d >= 2) runs PFM_EIG_MAX_SWEEPS
 * sweeps and gets NaN for every eigenvalue and every element of V, and touches no other matrix.  Eigenvalues are ranked with NaN
 * last and ties by index.  No float atomics; a matrix's outputs are the same bits alone, in any batch, in any call.  On success every
 * element of every output given is written.
 * PFM_EINVAL for a NULL A or w, batch outside 1 .. 65535, d < 1; PFM_EUNSUPPORTED for d > PFM_FRECHET_MAX_D; PFM_EWORKSPACE for a
 * missing or short workspace; on any error nothing is written.
 */
int pfm_sym_eig(void *stream, const double *A, int64_t batch, int64_t d, double *w, double *V, int32_t *sweeps,
                void *workspace, size_t workspace_bytes);

/* bytes of workspace pfm_frechet_grad needs: the moments (mean [2, d] at offset 0, cov [2, d, d] at the next multiple of 256 bytes),
   the two covariance factors [2, d, d] and the moments' partial sums; nothing of size n d^2 (0: the arguments are invalid or
   outside the limits) */
size_t pfm_frechet_grad_workspace_bytes(int64_t n, int64_t d, int64_t n_first);

/*
 * The Frechet distance of the pooled sample Z [n, d] (the real sample's nr = n_first rows, then the fake sample's nf = n - n_first)
 * and its row gradients.  Per sample s the mean mu_s and the covariance C_s are pfm_boot_moments' for identity indices, bitwise
 * (np.cov(rowvar=False), ddof 1, two passes); both samples need at least 2 rows.
 *   FD = |mu_r - mu_f|^2 + tr C_r + tr C_f - 2 tr (C_r C_f)^(1/2)
 * The trace term (probaforms_amd/metrics/fd.py, trace_sqrtm): S = C_r^(1/2) from the eigen-decomposition of C_r with the eigenvalues
 * clipped at 0, M = sym(S C_f S) = V diag(lambda) V^T, tr (C_r C_f)^(1/2) = sum_i sqrt(max(lambda_i, 0)), summed ascending.  The
 * value always comes from this real-side route.  Both decompositions are pfm_sym_eig's device code.
 * The gradient: tr f(M) is a spectral function, d tr f(M) = tr(f'(M) dM): no eigenvector derivative appears and repeated
 * eigenvalues are no special case.  With M^(-1/2)_cut = V diag(c_i) V^T, c_i = lambda_i^(-1/2) where lambda_i > rcond lambda_max
 * and EXACTLY 0 otherwise (a cut eigenvalue adds the subgradient 0; lambda_max <= 0: nothing is kept),
 *   G_f = dFD / dC_f = I - S M^(-1/2)_cut S
 *   G_r = dFD / dC_r = I - T (sym(T C_r T))^(-1/2)_cut T,  T = C_f^(1/2)         (the same route with the samples swapped)
 *   grad[a, :] = (2 / n_s) (mu_s - mu_o) + (2 / (n_s - 1)) G_s (z_a - mu_s)      for row a of sample s, o the other sample;
 * the features are summed in ascending order.  An eigenvalue of rounding noise just above the cut gives gradient elements of order
 * 1 / sqrt(rcond lambda_max): with n <= d or collinear features pass a larger rcond and look at rank.
 * sides: bit 0 asks for the real rows' gradient, bit 1 for the fake rows'; rows of a sample not asked for are written as 0.  The
 * swapped route runs only where bit 0 is set and grad is given.  grad [n, d] may be NULL: then only the value is formed.
 * parts [5] (may be NULL) = { FD, |mu_r - mu_f|^2, tr C_r, tr C_f, tr (C_r C_f)^(1/2) }; eig [d] (may be NULL): lambda of the
 * real-side M, ascending; rank [2] (int32, may be NULL): the eigenvalues kept by the cut in the real-side route and in the swapped
 * route, the latter -1 where that route was not run.  On return the workspace holds the moments where
 * pfm_frechet_grad_workspace_bytes says.
 * Nothing is checked for NaN or infinity: a NaN anywhere in Z makes the value and every gradient element asked for NaN.  No float
 * atomics; the order of every sum depends on (n, n_first, d) only, so the outputs are bitwise the same in any call.  On success
 * every element of every output given is written.
 * PFM_EINVAL for n_first < 2, n - n_first < 2, d < 1, n >= 2^31, an rcond outside [0, 1) or NaN, sides outside 0 .. 3, sides == 0 with
 * grad given, a NULL Z or value; PFM_EUNSUPPORTED for d > PFM_FRECHET_MAX_D; PFM_EWORKSPACE for a missing or short workspace; on any
 * error nothing is written.
 */
int pfm_frechet_grad(void *stream, const double *Z, int64_t n, int64_t d, int64_t n_first, double rcond, int sides,
                     double *value, double *grad, double *parts, double *eig, int32_t *rank, void *workspace,
                     size_t workspace_bytes);

#ifdef __cplusplus
}
#endif
#endif
