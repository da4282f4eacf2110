// Row helpers of the CTC head's kernels, shared by ctc_loss.hip (loss, greedy decoder) and ctc_decode.hip (prefix beam
// search): one wave64 per row of raw head logits.
#pragma once

#include "common.hpp"

// Online max / exp-sum of one row over the wave, as rnnt_lse_gather forms it.  ARGMAX also tracks the largest logit's
// LOWEST index: a lane sees its columns in ascending order and replaces its best on a strictly larger value only, the
// wave reduction prefers the larger value and, on a tie, the lower index.
template <typename T, bool ARGMAX>
__device__ __forceinline__ float row_lse(const T* __restrict__ z, int V, int vec_ok, int lane, float* best_v, int* best_i) {
    constexpr int VEC = ElemIO<T>::VEC;
    float m = -INFINITY, s = 0.f;
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    if (vec_ok) {
        for (int v = lane * VEC; v < V; v += 64 * VEC) {
            float x[VEC];
            ElemIO<T>::load_vec(z + v, x);
            float mx = x[0];
#pragma unroll
            for (int i = 1; i < VEC; ++i) mx = fmaxf(mx, x[i]);
            if (ARGMAX) {
#pragma unroll
                for (int i = 0; i < VEC; ++i)
                    if (x[i] > bv || bi == 0x7fffffff) { bv = x[i]; bi = v + i; }
            }
            const float mn = fmaxf(m, mx);
            float acc = 0.f;
#pragma unroll
            for (int i = 0; i < VEC; ++i) acc += __expf(x[i] - mn);
            s = s * __expf(m - mn) + acc;
            m = mn;
        }
    } else {
        for (int v = lane; v < V; v += 64) {
            const float x = ElemIO<T>::load(z + v);
            if (ARGMAX && (x > bv || bi == 0x7fffffff)) { bv = x; bi = v; }
            const float mn = fmaxf(m, x);
            s = s * __expf(m - mn) + __expf(x - mn);
            m = mn;
        }
    }
    const float M = wave_max(m);
    const float part = (m == -INFINITY) ? 0.f : s * __expf(m - M);
    const float S = wave_sum(part);
    if (ARGMAX) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float ov = __shfl_xor(bv, off, 64);
            const int oi = __shfl_xor(bi, off, 64);
            if (oi != 0x7fffffff && (bi == 0x7fffffff || ov > bv || (ov == bv && oi < bi))) { bv = ov; bi = oi; }
        }
        *best_v = bv;
        *best_i = bi;
    }
    return M + logf(S);
}
