// The risk layer of minimum word error rate (MWER) training for gfx950: from the negative log-likelihoods and the error
// counts of an utterance's N-best list, the expected number of errors under the list's renormalised posterior and its
// derivative with respect to every hypothesis' cost (Prabhavalkar et al. 2018; Guo et al. 2020 for RNN-T).  The errors
// come from edit_distance.hip, the costs from the packed joint + loss (models._JointRowCostsFn); loss.MWERLoss is the
// operator on top.
//
// costs [B, N] float32 (finite or +inf), errs int32 with an element stride (1: a [B, N] array; 4: `dist` of
// edit_distance's [B, N, 4]), n_hyp [B] live slots (null: all N).  Slot n of utterance b is LIVE iff n < n_hyp[b] and
// costs[b, n] < +inf.  Over the live slots, in fp64:
//     m = min c_n,  w_n = exp(-(c_n - m)),  p_n = w_n / sum w          the posterior (the cheapest hypothesis has w = 1)
//     e_min = min errs_n,  d_n = errs_n - e_min                         an integer difference
//     dbar = sum p_n d_n,  risk_b = e_min + dbar
//     coef_n = scale p_n (dbar - d_n) = d(scale risk_b) / d c_n         (the hypothesis' log-probability is -c_n)
// Taking d relative to e_min makes dbar, and with it every coefficient, exactly 0 when all live hypotheses have the
// same error count.  Dead slots: post = coef = 0; an utterance without a live slot: risk = 0.
//
//   mwer_risk_wave : ONE WAVE per utterance, lane n owns hypothesis n (lanes >= N are dead slots).  The two minima and
//                    the two sums are xor butterflies over the 64 lanes (offsets 32 .. 1): every lane forms the same
//                    operands in the same order, so all lanes hold the same bits and the result does not depend on the
//                    launch.                                                                          latency-bound.
//   mwer_reduce    : one wave; reduced = scale * sum_b (risk[b] + nll_weight * ref_costs[b]) from the risk values as
//                    they were stored, lane l adding b = l, l + 64, ... in fp64, then the same butterfly.
// No LDS, no atomics, no workspace; vector stores only; bit-identical from run to run.
#include "common.hpp"

#include <limits.h>

namespace {

constexpr int MWER_MAX_N = 32;

__device__ __forceinline__ double mwer_wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
__device__ __forceinline__ double mwer_wave_min(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmin(v, __shfl_xor(v, off, 64));
    return v;
}
__device__ __forceinline__ int mwer_wave_min(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = min(v, __shfl_xor(v, off, 64));
    return v;
}

// blockIdx.x = b, 64 threads, all of them active in every shuffle.
__global__ __launch_bounds__(64) void mwer_risk_wave(const float* __restrict__ costs, const int32_t* __restrict__ errs,
                                                     int err_stride, const int32_t* __restrict__ n_hyp, int N,
                                                     double scale, float* __restrict__ risk, float* __restrict__ post,
                                                     float* __restrict__ coef) {
    const int b = blockIdx.x, n = threadIdx.x;
    const long long slot = (long long)b * N + n;
    const int nh = n_hyp ? max(0, min(n_hyp[b], N)) : N;
    const double INF = (double)INFINITY;
    double c = INF;
    if (n < nh) {
        const float cf = costs[slot];
        if (cf < INFINITY) c = (double)cf;           // (a NaN is a dead slot too)
    }
    const bool live = c < INF;
    const int e = live ? errs[slot * err_stride] : INT_MAX;
    const double m = mwer_wave_min(c);
    const int e_min = mwer_wave_min(e);
    if (!(m < INF)) {                                // no live slot (wave-uniform: every lane holds the same m)
        if (n < N) post[slot] = coef[slot] = 0.f;
        if (n == 0) risk[b] = 0.f;
        return;
    }
    const double w = live ? exp(-(c - m)) : 0.0;
    const double p = w / mwer_wave_sum(w);
    const double d = live ? (double)(e - e_min) : 0.0;
    const double dbar = mwer_wave_sum(p * d);
    if (n < N) {
        post[slot] = (float)p;
        coef[slot] = (float)(scale * p * (dbar - d));
    }
    if (n == 0) risk[b] = (float)((double)e_min + dbar);
}

__global__ __launch_bounds__(64) void mwer_reduce(const float* __restrict__ risk, const float* __restrict__ ref_costs,
                                                  int B, double nll_weight, double scale, float* __restrict__ reduced) {
    double acc = 0.0;
    for (int b = threadIdx.x; b < B; b += 64) {
        double v = (double)risk[b];
        if (ref_costs) v += nll_weight * (double)ref_costs[b];
        acc += v;
    }
    acc = mwer_wave_sum(acc);
    if (threadIdx.x == 0) reduced[0] = (float)(scale * acc);
}

}  // namespace

extern "C" int edgedict_mwer_risk(const float* costs, const int32_t* errs, int err_stride, const int32_t* n_hyp,
                                  const float* ref_costs, int B, int N, double nll_weight, double scale, float* risk,
                                  float* post, float* coef, float* reduced, void* stream_) {
    ED_CHECK_ARG(B >= 1, "mwer_risk: B must be positive (got %d)", B);
    ED_CHECK_ARG(N >= 1 && N <= MWER_MAX_N, "mwer_risk: N = %d outside [1, %d] hypotheses per utterance", N, MWER_MAX_N);
    ED_CHECK_ARG(err_stride == 1 || err_stride == 4, "mwer_risk: err_stride = %d is neither 1 ([B, N]) nor 4 ([B, N, 4])",
                 err_stride);
    ED_CHECK_ARG((long long)B * N <= 0x7fffffffLL, "mwer_risk: B * N = %lld exceeds the grid", (long long)B * N);
    ED_CHECK_ARG(costs && errs && risk && post && coef, "mwer_risk: null pointer argument");
    hipStream_t stream = (hipStream_t)stream_;
    hipLaunchKernelGGL(mwer_risk_wave, dim3(B), dim3(64), 0, stream, costs, errs, err_stride, n_hyp, N, scale, risk, post,
                       coef);
    ED_CHECK_LAUNCH("mwer_risk_wave");
    if (reduced) {                                   // (null: the caller wants the per-utterance values only)
        hipLaunchKernelGGL(mwer_reduce, dim3(1), dim3(64), 0, stream, risk, ref_costs, B, nll_weight, scale, reduced);
        ED_CHECK_LAUNCH("mwer_reduce");
    }
    return ED_OK;
}
