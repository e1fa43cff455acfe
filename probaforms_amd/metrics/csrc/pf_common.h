// pf_common.h -- what every translation unit of libpf_metrics.so shares: the workgroup size, the status macro of the C entry
// points and the workspace alignment.
#ifndef PF_COMMON_H
#define PF_COMMON_H

#include <hip/hip_runtime.h>

#include <stddef.h>
#include <stdint.h>

#define PFM_TRY(x)                                              \
    do {                                                        \
        hipError_t e_ = (x);                                    \
        if (e_ != hipSuccess) return (int)e_;                   \
    } while (0)

namespace {

constexpr int NT = 256;          // threads per workgroup, every kernel

inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

}  // namespace

#endif
