// exact_arith.h -- the device functions every kernel that restates the reference arithmetic shares: the 8-element row load, the
// finish of a float32 chain and the (query,row) distance built from the two. exact.hip (the exact path, the re-rank kernels),
// mmr.hip (the candidate Gram) and group.hip (the members of a group) include it, so that a pair distance, a member's distance
// and a query distance cannot drift apart.
#pragma once
#include "common.h"

namespace ak {

// Stored row elements in chunks of 8 (16 B for 16-bit dtypes, 2 x 16 B for f32): the reference
// arithmetic is a strictly sequential chain, so the only thing to vectorise is the LOAD.
template <int DT>
__device__ inline void load8(const typename Store<DT>::T *row, int i, float (&v)[8]) {
    if constexpr (DT == AK_DTYPE_F32) {
        float4 a = *(const float4 *)(row + i), b = *(const float4 *)(row + i + 4);
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    } else {
        uint4 u = *(const uint4 *)(row + i);
        const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
        for (int j = 0; j < 4; j++) {
            uint16_t lo = (uint16_t)(w[j] & 0xffffu), hi = (uint16_t)(w[j] >> 16);
            v[2 * j] = DT == AK_DTYPE_BF16 ? bf16_to_f32(lo) : f16_to_f32(lo);
            v[2 * j + 1] = DT == AK_DTYPE_BF16 ? bf16_to_f32(hi) : f16_to_f32(hi);
        }
    }
}

// The finish of one (query,row) distance: the float32 accumulator of the sequential chain -> float8 distance. One function for
// exact_distance, the panel re-rank and the MMR pair distances, so that the kernels cannot drift apart.
__device__ inline double exact_finish(float acc, int metric, float na, float nb) {
    if (metric == AK_METRIC_L2) return sqrt((double)acc);
    if (metric == AK_METRIC_IP) return (double)(-acc);
    double sim = (double)acc / sqrt((double)na * (double)nb);
    if (sim > 1.0) sim = 1.0;
    else if (sim < -1.0) sim = -1.0;
    return 1.0 - sim;
}

// One (query,row) distance in the oracle's arithmetic. `na` is the row's
// precomputed pgvector-order sum of squares, `nb` the query's. exact.hip (the exact path, the thread-per-candidate re-rank) and
// group.hip (the members of a group) call it.
template <int DT>
__device__ inline double exact_distance(const typename Store<DT>::T *row, const float *q, int dim,
                                        int metric, float na, float nb) {
    using S = Store<DT>;
    const bool vec = (dim % 8 == 0) && (((uintptr_t)row & 15) == 0);
    float acc = 0.0f;
    if (metric == AK_METRIC_L2) {
        int i = 0;
        if (vec)
            for (; i < dim; i += 8) {
                float v[8];
                load8<DT>(row, i, v);
#pragma unroll
                for (int j = 0; j < 8; j++) {
                    float diff = __fsub_rn(v[j], q[i + j]);
                    acc = __fadd_rn(acc, __fmul_rn(diff, diff));
                }
            }
        for (; i < dim; i++) {
            float diff = __fsub_rn(S::load(row, i), q[i]);
            acc = __fadd_rn(acc, __fmul_rn(diff, diff));
        }
        return exact_finish(acc, metric, na, nb);
    }
    int i = 0;
    if (vec)
        for (; i < dim; i += 8) {
            float v[8];
            load8<DT>(row, i, v);
#pragma unroll
            for (int j = 0; j < 8; j++) acc = __fadd_rn(acc, __fmul_rn(v[j], q[i + j]));
        }
    for (; i < dim; i++) acc = __fadd_rn(acc, __fmul_rn(S::load(row, i), q[i]));
    return exact_finish(acc, metric, na, nb);
}

}  // namespace ak
