// Row-wise softmax negative log-likelihood on raw logits [M, V] (the LM's loss: log_softmax + NLLLoss(ignore_index) of
// cli/train_lm.py:60,89 in two passes over the logits instead of four over an fp32 [M, V] log-prob matrix and its
// gradient).  DESIGN.md section 4.43.
//
//   forward : one wave per row, ROWS rows per workgroup.  Each lane keeps an online (max, sum exp(x - max)) over its
//             16-byte vectors - ONE read of the row -, the 64 lane pairs are merged by a butterfly (fixed order), and
//             lane 0 writes lse = max + log(sum) and nll = log(sum) - (z[target] - max) (0 for an ignored row).
//             exp is the hardware's (v_exp_f32, ~1 ulp after the argument's scaling: 1e-6 relative at |x - max| = 100,
//             on terms of size e^-100); libm's expf made the forward VALU-bound at 2.4 TB/s.
//   reduce  : ONE workgroup adds nll over the valid rows in fp64 in a fixed order (strided partials, a butterfly per
//             wave, the 16 wave sums in order; no atomics) and writes {sum, count} and the reduced loss; 'mean' over
//             zero valid rows is 0, not NaN.
//   backward: one wave per row again: z <- g_m * (exp(z - lse) - onehot) in place in the logits' dtype (second read,
//             the only write); an ignored row is never read and gets exact zeros.  g_m comes from device memory (the
//             incoming gradient, divided by the device count for 'mean').
//
// A row is ignored when its target equals ignore_index or lies outside [0, V).  Rows whose base pointer, leading
// dimension and V allow 16-byte accesses take the vector path, everything else a scalar path with the same arithmetic
// order per lane (the two paths are NOT bit-identical to each other: the lane <-> column assignment differs).
#include "common.hpp"

namespace {

constexpr int LM_ROWS = 4;  // rows (waves) per workgroup

__device__ __forceinline__ bool lm_valid(int t, int V, int ignore_index) {
    return t != ignore_index && t >= 0 && t < V;
}

// (m, s) <- (m, s) merged with the values x[0..n): s = sum exp(. - m), m the running max; -inf entries add nothing
template <int N>
__device__ __forceinline__ void lm_online(float& m, float& s, const float (&x)[N]) {
    float vm = x[0];
#pragma unroll
    for (int k = 1; k < N; ++k) vm = fmaxf(vm, x[k]);
    if (vm > m) {
        s *= __expf(m - vm);  // m = -inf: s is 0 and stays 0
        m = vm;
    }
    if (m != -INFINITY) {
#pragma unroll
        for (int k = 0; k < N; ++k) s += __expf(x[k] - m);
    }
}

template <typename T, bool VECP>
__global__ __launch_bounds__(64 * LM_ROWS) void softmax_nll_fwd_kernel(const T* __restrict__ z, long long ldx,
                                                                       const int32_t* __restrict__ tgt, int M, int V,
                                                                       int ignore_index, float* __restrict__ lse,
                                                                       float* __restrict__ nll) {
    const int lane = threadIdx.x & 63;
    const long long r = (long long)blockIdx.x * LM_ROWS + (threadIdx.x >> 6);
    if (r >= M) return;  // the whole wave leaves: no workgroup barrier below
    const T* zr = z + r * ldx;
    float m = -INFINITY, s = 0.f;
    if (VECP) {
        constexpr int VEC = ElemIO<T>::VEC;
        const int nv = V / VEC;
#pragma unroll 2
        for (int i = lane; i < nv; i += 64) {
            float x[VEC];
            ElemIO<T>::load_vec(zr + (long long)i * VEC, x);
            lm_online(m, s, x);
        }
    } else {
        for (int i = lane; i < V; i += 64) {
            const float x[1] = {ElemIO<T>::load(zr + i)};
            lm_online(m, s, x);
        }
    }
    const float mx = wave_max(m);
    const float sum = wave_sum(m == -INFINITY ? 0.f : s * __expf(m - mx));
    if (lane == 0) {
        const float ls = logf(sum);
        if (lse) lse[r] = mx + ls;
        const int t = tgt[r];
        nll[r] = lm_valid(t, V, ignore_index) ? ls - (ElemIO<T>::load(zr + t) - mx) : 0.f;
    }
}

// stats = {sum of nll over the valid rows (fp64), number of valid rows}; reduced = sum, or sum / count ('mean'; 0
// when no row is valid).  One workgroup: thread k adds rows k, k + 1024, ... in order (8 loads in flight at a time:
// the chain of dependent load latencies was most of this kernel), a butterfly per wave, then lane 0 of wave 0 adds the
// 16 wave sums in order.
__device__ __forceinline__ double lm_wave_sum64(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
__global__ __launch_bounds__(1024) void softmax_nll_reduce_kernel(const float* __restrict__ nll,
                                                                  const int32_t* __restrict__ tgt, int M, int V,
                                                                  int ignore_index, int mean,
                                                                  double* __restrict__ stats,
                                                                  float* __restrict__ reduced) {
    __shared__ double psum[16];
    __shared__ double pcnt[16];
    const int tid = threadIdx.x;
    double a = 0.0, c = 0.0;
    for (long long base = 0; base < M; base += 8 * 1024) {
        float v[8];
        int t[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const long long r = base + j * 1024 + tid;
            v[j] = r < M ? nll[r] : 0.f;
            t[j] = r < M ? tgt[r] : -1;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const bool ok = base + j * 1024 + tid < M && lm_valid(t[j], V, ignore_index);
            a += ok ? (double)v[j] : 0.0;
            c += ok ? 1.0 : 0.0;
        }
    }
    a = lm_wave_sum64(a);
    c = lm_wave_sum64(c);
    if ((tid & 63) == 0) {
        psum[tid >> 6] = a;
        pcnt[tid >> 6] = c;
    }
    __syncthreads();
    if (tid == 0) {
        double sum = 0.0, cnt = 0.0;
        for (int w = 0; w < 16; ++w) {
            sum += psum[w];
            cnt += pcnt[w];
        }
        stats[0] = sum;
        stats[1] = cnt;
        if (reduced) *reduced = (float)(mean ? (cnt > 0.0 ? sum / cnt : 0.0) : sum);
    }
}

template <typename T, bool VECP>
__global__ __launch_bounds__(64 * LM_ROWS) void softmax_nll_bwd_kernel(T* __restrict__ z, long long ldx,
                                                                       const int32_t* __restrict__ tgt, int M, int V,
                                                                       int ignore_index,
                                                                       const float* __restrict__ lse,
                                                                       const float* __restrict__ grad,
                                                                       int grad_stride,
                                                                       const double* __restrict__ stats, int mean) {
    const int lane = threadIdx.x & 63;
    const long long r = (long long)blockIdx.x * LM_ROWS + (threadIdx.x >> 6);
    if (r >= M) return;
    T* zr = z + r * ldx;
    const int t = tgt[r];
    const bool valid = lm_valid(t, V, ignore_index);  // wave-uniform
    float g = 0.f, l = 0.f;
    if (valid) {
        g = grad[r * grad_stride];
        if (mean) {
            const double cnt = stats[1];
            g = cnt > 0.0 ? (float)((double)g / cnt) : 0.f;
        }
        l = lse[r];
    }
    if (VECP) {
        constexpr int VEC = ElemIO<T>::VEC;
        const int nv = V / VEC;
#pragma unroll 2
        for (int i = lane; i < nv; i += 64) {
            float x[VEC];
            if (valid) {
                ElemIO<T>::load_vec(zr + (long long)i * VEC, x);
#pragma unroll
                for (int k = 0; k < VEC; ++k) x[k] = g * (__expf(x[k] - l) - (i * VEC + k == t ? 1.f : 0.f));
            } else {
#pragma unroll
                for (int k = 0; k < VEC; ++k) x[k] = 0.f;
            }
            ElemIO<T>::store_vec(zr + (long long)i * VEC, x);
        }
    } else {
        for (int i = lane; i < V; i += 64) {
            float x = 0.f;
            if (valid) x = g * (__expf(ElemIO<T>::load(zr + i) - l) - (i == t ? 1.f : 0.f));
            ElemIO<T>::store(zr + i, x);
        }
    }
}

template <typename T>
bool lm_vec_ok(const void* z, long long ldx, int V) {
    constexpr int VEC = ElemIO<T>::VEC;
    return V % VEC == 0 && ldx % VEC == 0 && ((uintptr_t)z & 15) == 0;
}

}  // namespace

extern "C" int edgedict_softmax_nll_forward(int dtype, const void* logits, long long ldx, const int32_t* targets,
                                            int M, int V, int ignore_index, float* lse, float* nll, double* stats,
                                            float* reduced, int mean, void* stream_) {
    ED_CHECK_ARG(dtype == ED_F32 || dtype == ED_BF16, "softmax_nll_forward: bad dtype");
    ED_CHECK_ARG(M >= 0 && V > 0 && ldx >= V, "softmax_nll_forward: bad shape (M %d, V %d, ldx %lld)", M, V, ldx);
    ED_CHECK_ARG(stats || !reduced, "softmax_nll_forward: a reduced loss needs the stats buffer");
    ED_CHECK_ARG(M == 0 || (logits && targets && nll), "softmax_nll_forward: null pointer");
    hipStream_t s = (hipStream_t)stream_;
    if (M > 0) {
        const dim3 grid((M + LM_ROWS - 1) / LM_ROWS), block(64 * LM_ROWS);
#define ED_LM_FWD(T, VECP) \
    hipLaunchKernelGGL((softmax_nll_fwd_kernel<T, VECP>), grid, block, 0, s, (const T*)logits, ldx, targets, M, V, \
                       ignore_index, lse, nll)
        if (dtype == ED_F32) {
            if (lm_vec_ok<float>(logits, ldx, V)) ED_LM_FWD(float, true);
            else ED_LM_FWD(float, false);
        } else {
            if (lm_vec_ok<bf16_t>(logits, ldx, V)) ED_LM_FWD(bf16_t, true);
            else ED_LM_FWD(bf16_t, false);
        }
#undef ED_LM_FWD
        ED_CHECK_LAUNCH("softmax_nll_forward");
    }
    if (stats) {
        hipLaunchKernelGGL(softmax_nll_reduce_kernel, dim3(1), dim3(1024), 0, s, nll, targets, M, V, ignore_index,
                           mean != 0, stats, reduced);
        ED_CHECK_LAUNCH("softmax_nll_forward (reduce)");
    }
    return ED_OK;
}

extern "C" int edgedict_softmax_nll_backward(int dtype, void* logits, long long ldx, const int32_t* targets, int M,
                                             int V, int ignore_index, const float* lse, const float* grad,
                                             int grad_stride, const double* stats, int mean, void* stream_) {
    ED_CHECK_ARG(dtype == ED_F32 || dtype == ED_BF16, "softmax_nll_backward: bad dtype");
    ED_CHECK_ARG(M >= 0 && V > 0 && ldx >= V, "softmax_nll_backward: bad shape (M %d, V %d, ldx %lld)", M, V, ldx);
    ED_CHECK_ARG(grad_stride == 0 || grad_stride == 1, "softmax_nll_backward: grad_stride must be 0 or 1");
    ED_CHECK_ARG(!mean || stats, "softmax_nll_backward: 'mean' needs the forward's stats buffer");
    if (M == 0) return ED_OK;
    ED_CHECK_ARG(logits && targets && lse && grad, "softmax_nll_backward: null pointer");
    hipStream_t s = (hipStream_t)stream_;
    const dim3 grid((M + LM_ROWS - 1) / LM_ROWS), block(64 * LM_ROWS);
#define ED_LM_BWD(T, VECP) \
    hipLaunchKernelGGL((softmax_nll_bwd_kernel<T, VECP>), grid, block, 0, s, (T*)logits, ldx, targets, M, V, \
                       ignore_index, lse, grad, grad_stride, stats, mean != 0)
    if (dtype == ED_F32) {
        if (lm_vec_ok<float>(logits, ldx, V)) ED_LM_BWD(float, true);
        else ED_LM_BWD(float, false);
    } else {
        if (lm_vec_ok<bf16_t>(logits, ldx, V)) ED_LM_BWD(bf16_t, true);
        else ED_LM_BWD(bf16_t, false);
    }
#undef ED_LM_BWD
    ED_CHECK_LAUNCH("softmax_nll_backward");
    return ED_OK;
}
