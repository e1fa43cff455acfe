// pf_moments.h -- the moments kernels of pf_metrics.hip (k_mean_* / k_cov_*) for the library's other translation units: the
// launches behind pfm_boot_moments, without its argument checks.  pf_frechet.hip forms the moments of the samples as given with
// them, so that they are bitwise pfm_boot_moments' for identity indices.  Not part of the C ABI.
#ifndef PF_MOMENTS_H
#define PF_MOMENTS_H

#include <hip/hip_runtime.h>

#include <stddef.h>
#include <stdint.h>

// bytes of the two partial-sum buffers for `reps` replicates (what pfm_moments_workspace_bytes returns for valid sizes)
size_t pf_moments_partial_bytes(int64_t nr, int64_t nf, int64_t d, int64_t reps);

// enqueue mean [reps, 2, d] and cov [reps, 2, d, d] on `st`.  idx_r / idx_f NULL (both): row r is row r, reps must be 1.
// partials: pf_moments_partial_bytes() bytes.  -> hipSuccess or the launch error
hipError_t pf_moments_enqueue(hipStream_t st, const double *Xr, int64_t nr, const double *Xf, int64_t nf, int64_t d,
                              const int32_t *idx_r, const int32_t *idx_f, int64_t reps, double *mean, double *cov,
                              void *partials);

#endif
