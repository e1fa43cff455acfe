// pf_nearest.h -- the ONE k-nearest sweep of libpf_metrics.so: the per-lane lists of the nearest candidates of a query row,
// the pruning bound, and the merge of a row's 16 lists (k_knn_radius<L> of pf_knn.hip, k_nn_index<L> of pf_nn.hip).
//
// A workgroup owns a 64-row query tile and sweeps the candidate tiles with tile_d2 (pf_pairtile.h): thread (ti, tj) meets, for
// each of its 4 query rows ti + 16 a, the candidates tj + 16 b of every tile.  Nearest<L, IDX> is a thread's state: per query
// row an ascending list of the L nearest candidates it has met, with their row indices beside the values where IDX is set,
// and `bound`, an upper bound of the row's L-th nearest value.  The caller decides which candidates count (in range; the
// row itself or not), offers them with offer(), calls share() after every tile, and then takes the row's nearest candidates in
// ascending order, one per take(), which hands them to the caller's emit().  L is at least the number of take() rounds.
//
// Why `v < bound` stays exact under the (d^2, row index) order.  A lane keeps, per query row, the L >= k smallest candidates it
// has met, ascending.  It meets its candidates in ascending row index: the tiles are swept in ascending order and inside a tile
// the lane's columns tj + 16 b ascend with b.  The insertion moves a new entry past strictly larger values only, so among equal
// values the earlier, smaller index stays in front: a list is ascending in (d^2, index).  `bound` is never above the lane's own
// L-th value, and is lowered after every tile to the smallest L-th value among the row's 16 lanes.  So whatever the bound rests
// on is a list of L >= k candidates that were met before the candidate under test: by the lane itself (smaller indices, same
// or earlier tile) or by another lane in an EARLIER tile (smaller indices again).  A candidate with v >= bound therefore has at
// least k candidates in front of it in (d^2, index) order, all with values <= v and smaller indices; it is not among the k
// nearest and skipping it changes nothing, ties included.  The argument needs the ascending sweep: in another order a
// candidate equal to the bound could carry the smaller index and would have to be kept.
// The value-only variant needs no tie rule: it reports values alone, and which of several equal values is skipped or popped
// does not change the multiset of the k smallest values.
#ifndef PF_NEAREST_H
#define PF_NEAREST_H

#include "pf_pairtile.h"

namespace {

template <int L, bool IDX>
struct Nearest {
    double best[4][L], bound[4];
    int32_t who[4][IDX ? L : 1];        // (unused without IDX)

    __device__ void init() {
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            bound[a] = INFINITY;
#pragma unroll
            for (int i = 0; i < L; ++i) {
                best[a][i] = INFINITY;
                if constexpr (IDX) who[a][i] = INT32_MAX;
            }
        }
    }

    // candidate (v, j) of query row a (j is above every index the lane has met for the row; pass INFINITY for a candidate
    // that does not count).  Below the bound it replaces the list's last entry and sinks past strictly larger values through an
    // unrolled compare-exchange chain; every list index is a compile-time constant, so the lists stay in registers.  The
    // bound is rarely met, so the chain is rarely entered.
    __device__ void offer(int a, double v, int32_t j) {
        if (!(v < bound[a])) return;
        double (&b)[L] = best[a];
        b[L - 1] = v;
        if constexpr (IDX) who[a][L - 1] = j;
#pragma unroll
        for (int i = L - 1; i > 0; --i) {
            const double hi = b[i], lo = b[i - 1];
            const bool sw = hi < lo;
            b[i - 1] = sw ? hi : lo;
            b[i] = sw ? lo : hi;
            if constexpr (IDX) {
                const int32_t jh = who[a][i], jl = who[a][i - 1];
                who[a][i - 1] = sw ? jh : jl;
                who[a][i] = sw ? jl : jh;
            }
        }
        bound[a] = b[L - 1] < bound[a] ? b[L - 1] : bound[a];
    }

    // after a tile: the smallest bound of a query row's 16 lanes becomes the bound of all of them
    __device__ void share() {
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            double m = bound[a];
#pragma unroll
            for (int s = 1; s < 16; s <<= 1) {
                const double o = __shfl_xor(m, s, 16);
                m = o < m ? o : m;
            }
            bound[a] = m;
        }
    }

    __device__ void pop(int a) {
#pragma unroll
        for (int i = 0; i + 1 < L; ++i) {
            best[a][i] = best[a][i + 1];
            if constexpr (IDX) who[a][i] = who[a][i + 1];
        }
        best[a][L - 1] = INFINITY;
        if constexpr (IDX) who[a][L - 1] = INT32_MAX;
    }

    // one merge round of the 16 lists of each query row through LDS (h, hj: one of two alternating buffers, so that a round
    // needs one barrier; hj is not read without IDX): the smallest of the 16 heads is found by every lane of the row, the lane
    // that held it pops it, and every lane calls emit(a, value, index) for its query row a (the index is 0 without IDX).  With
    // IDX the smallest (d^2, index) wins and its holder is known by the index (an index is in one list only); without, the
    // lowest lane among equal values pops.
    template <class Emit>
    __device__ void take(double (*h)[16][16], int32_t (*hj)[16][16], Emit emit) {
        const int ti = threadIdx.x >> 4, tj = threadIdx.x & 15;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            h[a][ti][tj] = best[a][0];
            if constexpr (IDX) hj[a][ti][tj] = who[a][0];
        }
        __syncthreads();
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            double m = h[a][ti][0];
            if constexpr (IDX) {
                int32_t mj = hj[a][ti][0];
#pragma unroll
                for (int t = 1; t < 16; ++t) {
                    const double o = h[a][ti][t];
                    const int32_t oj = hj[a][ti][t];
                    if (o < m || (o == m && oj < mj)) { m = o; mj = oj; }
                }
                if (mj == who[a][0]) pop(a);
                emit(a, m, mj);
            } else {
                int w = 0;
#pragma unroll
                for (int t = 1; t < 16; ++t) {
                    const double o = h[a][ti][t];
                    if (o < m) { m = o; w = t; }
                }
                if (w == tj) pop(a);
                emit(a, m, 0);
            }
        }
    }
};

}  // namespace

#endif
