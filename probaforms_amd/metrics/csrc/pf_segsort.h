// pf_segsort.h -- a segmented sort in LDS: `segs` segments of n entries (float64 value, int32 index) each, all sorted at once by one
// workgroup, ascending by (value, index).  The network is k_slice_sort's (pf_slicegrad.hip): a bitonic network in the form whose
// compare-exchanges all point the same way, the first step of a merge pairing i with i ^ (2 m - 1) and the others i with i ^ m.
// Positions >= n behave as +infinity without being stored: a compare-exchange whose upper position is >= n is skipped, so n need not
// be a power of two and nothing is padded.  The network is data-oblivious: which entries meet depends on n alone, so a NaN (every
// comparison with it is false: the pair stays as it lies) can neither make it loop nor make it index outside its segment; -0.0 and
// +0.0 are equal and ordered by their indices.
#ifndef PF_SEGSORT_H
#define PF_SEGSORT_H

#include <hip/hip_runtime.h>

#include <stdint.h>

namespace {

// segment r lies at sv + r * pitch and si + r * pitch, pitch >= n; threads: the workgroup's size, tid the thread's index in it.
// The whole workgroup calls it with the same arguments, after a barrier behind the last write of the entries; it ends on a barrier.
__device__ inline void seg_sort(double *sv, int32_t *si, int segs, int n, int pitch, int tid, int threads) {
    int npad = 1, lg = 0;
    while (npad < n) {
        npad <<= 1;
        ++lg;
    }
    const int half = npad >> 1;                       // compare-exchanges of a segment per step: 2^(lg - 1)
    const int total = segs * half;
    for (int m = 2; m <= npad; m <<= 1) {
        for (int j = m >> 1; j > 0; j >>= 1) {
            const int flip = j == (m >> 1) ? m - 1 : j;           // the merge's first step mirrors, the others shift
            for (int t = tid; t < total; t += threads) {
                const int r = t >> (lg - 1), q = t & (half - 1);
                const int lo = ((q & ~(j - 1)) << 1) | (q & (j - 1));
                const int hi = lo ^ flip;                          // hi > lo
                if (hi < n) {                                      // hi >= n: +infinity stays above
                    double *const v = sv + r * pitch;
                    int32_t *const x = si + r * pitch;
                    const double a = v[lo], b = v[hi];
                    const int32_t ia = x[lo], ib = x[hi];
                    const bool swap = a > b || (a == b && ia > ib);
                    v[lo] = swap ? b : a;                          // stored either way: the cost depends on n alone, too
                    v[hi] = swap ? a : b;
                    x[lo] = swap ? ib : ia;
                    x[hi] = swap ? ia : ib;
                }
            }
            __syncthreads();
        }
    }
}

}  // namespace

#endif
