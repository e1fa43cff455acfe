// pf_rowtile.h -- host-side row-tile policy of the "one thread = one row" models (pf_wgan.hip, pf_cnormal.hip).
//
// A training step runs row tiles of R batch rows per workgroup, with the tile's state in LDS.  How many rows LDS holds (the
// "cap") is the model's own formula; everything that follows from the cap is here.  Host code only: no kernel and no kernel
// parameter type lives in this header.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <atomic>

#include "../csrc/rnvp_common.h"

namespace pf_rowtile {

constexpr size_t kLds = 160 * 1024;       // LDS of one CU on gfx950
constexpr int kTargetWg = 256;            // a step kernel aims at one workgroup per CU
constexpr int kMinTile = 8;               // ... with at least 8 batch rows per workgroup

// rows per step workgroup for a batch of `rows`: at least kMinTile (latency: more workgroups only add partials), enough
// that ~kTargetWg workgroups cover the batch, at most `cap`, what LDS holds
inline int step_tile(int cap, int64_t rows) {
    int R = kMinTile;
    while ((int64_t)R * kTargetWg < rows) R *= 2;
    return R < cap ? R : cap;
}

// upper bound of the step's workgroups over every batch of at most `batch_rows` rows (sizes the partials' workspace)
inline int64_t step_wg_bound(int cap, int64_t batch_rows) {
    if (cap < 1) return 0;
    const int lo = cap < kMinTile ? cap : kMinTile;
    const int64_t a = (batch_rows + lo - 1) / lo;
    int64_t b = (batch_rows + cap - 1) / cap;
    if (b < kTargetWg) b = kTargetWg;
    return a < b ? a : b;
}

// what one launch is made of: rows per workgroup, LDS bytes, workgroups; tile == 0: the shape does not fit
struct Plan {
    int tile;
    size_t lds;
    int64_t wgs;
};

// `rows` rows in tiles of `tile`: `fixed` bytes of LDS, then per_tile * tile + 1 LDS rows of `unit` floats
inline Plan make_plan(int tile, size_t fixed, int per_tile, int unit, int64_t rows) {
    if (tile < 1) return Plan{0, 0, 0};
    return Plan{tile, fixed + (size_t)(per_tile * tile + 1) * unit * sizeof(float), (rows + tile - 1) / tile};
}

// a launch with more than 64 KiB of dynamic LDS needs the kernel's limit raised, once per process and device; 0 = ok
template <typename K>
int big_lds(K kernel, size_t bytes, std::atomic<uint64_t> &done) {
    if (bytes <= 64 * 1024) return 0;
    return rnvp::allow_big_lds(reinterpret_cast<const void *>(kernel), (int)kLds, done);
}

}  // namespace pf_rowtile
