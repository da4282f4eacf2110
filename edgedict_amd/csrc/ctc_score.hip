// CTC scorer of N-best lists for gfx950: the CTC log-likelihood of up to 32 hypotheses per utterance on the head's
// logits - the second pass that rescores the transducer's N-best lists with the auxiliary head (decode.ctc_rescore).
//
// Raw head logits z [B, T, V], per utterance N slots of token sequences hyps [B, N, U] (no blanks) with hyp_lens [B, N]
// and n_hyp [B] live slots.  scores[b, n] = ll of hyps[b, n, :hyp_lens[b, n]] over the frames t < act_lens[b], the
// quantity the header of ctc_loss.hip defines (the extended sequence, the alpha recursion, the last two states); -inf
// for a hypothesis without a path (T_b = 0, fewer frames than tokens plus adjacent repeats, a token outside [0, V)) and
// for the slots n >= n_hyp[b].
//
// A score needs the alpha walk only, and what depends on the frame alone is shared by an utterance's hypotheses:
//   ctc_score_rows : one wave64 per row (b, t < T_b): lse[b,t] (row_lse of ctc_rows.hpp, the vectorised / scalar choice
//                    of ctc_lse_gather) and lp_blank[b,t] = z[blank] - lse.  ONCE per utterance.        HBM-bound.
//   ctc_score_walk : ONE WAVE per (b, n), blockIdx.x = b N + n, so an utterance's hypotheses - which share the two row
//                    arrays and mostly share prefixes, hence logits - sit in adjacent workgroups.  The recursion, the
//                    lane ownership and the arithmetic are those of ctc_alpha_beta<C, false> in direction 0, restated
//                    here (ctc_loss.hip is not touched): a lane owns C consecutive states, lane l - 1's last two values
//                    arrive by wave_shr:1 DPP moves, log_add64 chained in the same order, fp64 carry, the final
//                    log_add64 over the last two states.  Two differences: a label's log-probability is read straight
//                    from the logits as (float)z[b,t,y_k] - lse[b,t] - the float expression ctc_lse_gather forms - and
//                    requested D rows ahead through the same register ring (the raw element and the row's lse wait in
//                    the ring, the subtraction happens at use); and NOTHING is stored per state: no alpha plane, no
//                    label gather [B,T,U], no label chain.                                              latency-bound.
// No LDS, no atomics, no MFMA.  The workspace is the two [B, T] float row arrays.
#include "common.hpp"
#include "ctc_rows.hpp"

namespace {

constexpr int CTC_SCORE_MAX_N = 32;

inline size_t score_up256(size_t n) { return ((n + 255) / 256) * 256; }

// a raw element of the ring as the float ElemIO<T>::load gives
__device__ __forceinline__ float score_elem(float v) { return v; }
__device__ __forceinline__ float score_elem(bf16_t v) { return bf16_to_f32(v); }

// grid (x, B), 4 waves per block, one row per wave per iteration; rows behind T_b are never read
template <typename T>
__global__ __launch_bounds__(256) void ctc_score_rows(const T* __restrict__ logits,
                                                      const int32_t* __restrict__ act_lens, int Tm, int V, int blank,
                                                      float* __restrict__ lse, float* __restrict__ lpb, int vec_ok) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.y;
    const int Tb = max(0, min(act_lens[b], Tm));
    for (int t = blockIdx.x * 4 + wave; t < Tb; t += gridDim.x * 4) {
        const long long row = (long long)b * Tm + t;
        const T* z = logits + row * (long long)V;
        const float l = row_lse<T, false>(z, V, vec_ok, lane, nullptr, nullptr);
        if (lane == 0) {
            lse[row] = l;
            lpb[row] = ElemIO<T>::load(z + blank) - l;
        }
    }
}

// blockIdx.x = b N + n, 64 threads.  Lane l owns the states m in [C l, C l + C) of the hypothesis' 2 U_n + 1; all lanes
// walk the frames in lock step (see ctc_alpha_beta in ctc_loss.hip, whose direction 0 this restates operation by
// operation).  The lane's C / 2 labels stay in registers; a label outside [0, V) reads nothing and has log-probability
// -inf (as ctc_lse_gather treats it), which the recursion carries to the score.  No sum has +inf as an operand, so no
// -inf - (-inf) is formed.  Tokens behind hyp_lens[b, n], the slots behind n_hyp[b] (n_hyp may be null: all N live)
// and the rows behind T_b are never read.
template <typename T, int C>
__global__ __launch_bounds__(64) void ctc_score_walk(const T* __restrict__ logits, const float* __restrict__ lse,
                                                     const float* __restrict__ lpb,
                                                     const int32_t* __restrict__ act_lens,
                                                     const int32_t* __restrict__ hyps,
                                                     const int32_t* __restrict__ hyp_lens,
                                                     const int32_t* __restrict__ n_hyp, int Tm, int N, int U, int V,
                                                     double* __restrict__ scores) {
    static_assert(C >= 2 && (C & 1) == 0, "a lane owns an even number of states");
    constexpr int H = C / 2;                         // label states per lane (the odd slots)
    constexpr int D = C <= 2 ? 8 : (C <= 4 ? 4 : (C <= 8 ? 2 : 1));
    const int b = blockIdx.x / N, n = blockIdx.x - b * N;
    const int lane = threadIdx.x;
    const double NEG = -(double)INFINITY;
    const int Tb = max(0, min(act_lens[b], Tm));
    const int live = n_hyp ? max(0, min(n_hyp[b], N)) : N;
    if (n >= live || Tb == 0) {
        if (lane == 0) scores[blockIdx.x] = NEG;
        return;
    }
    const int Ub = max(0, min(hyp_lens[blockIdx.x], U));
    const int S = 2 * Ub + 1;
    const long long row0 = (long long)b * Tm;
    const int32_t* y = hyps + (long long)blockIdx.x * U;
    int yk[H];                                       // the lane's labels; -1: none / outside [0, V)
    unsigned skip = 0;                               // bit c: state C lane + c may be entered from two states back
#pragma unroll
    for (int h = 0; h < H; ++h) {
        const int k = H * lane + h;                  // state m = 2 k + 1
        int v = -1;
        if (k < Ub) {
            v = y[k];
            if (k >= 1 && v != y[k - 1]) skip |= 1u << (2 * h + 1);
            if (v < 0 || v >= V) v = -1;
        }
        yk[h] = v;
    }
    double prev[C];
#pragma unroll
    for (int c = 0; c < C; ++c) prev[c] = NEG;
    float qb[D], qs[D];                              // ring by row: lp_blank, lse, the labels' raw logits
    T qz[D][H];
    auto request = [&](int j, int r) {               // (static j)
        float vb = 0.f, vs = 0.f;
        if (r < Tb) {
            vb = lpb[row0 + r];
            vs = lse[row0 + r];
        }
        qb[j] = vb;
        qs[j] = vs;
#pragma unroll
        for (int h = 0; h < H; ++h) {
            T vz = T(0);
            if (r < Tb && yk[h] >= 0) vz = logits[(row0 + r) * (long long)V + yk[h]];
            qz[j][h] = vz;
        }
    };
#pragma unroll
    for (int j = 0; j < D; ++j) request(j, j);
    for (int r0 = 0; r0 < Tb; r0 += D) {
#pragma unroll
        for (int j = 0; j < D; ++j) {
            const int r = r0 + j;
            if (r >= Tb) break;
            // lane l - 1's last two values of the previous row: a whole-wave shift by one lane (wave_shr:1)
            double s1 = __hiloint2double(__builtin_amdgcn_update_dpp(0, __double2hiint(prev[C - 1]), 0x138, 0xf, 0xf, false),
                                         __builtin_amdgcn_update_dpp(0, __double2loint(prev[C - 1]), 0x138, 0xf, 0xf, false));
            double s2 = __hiloint2double(__builtin_amdgcn_update_dpp(0, __double2hiint(prev[C - 2]), 0x138, 0xf, 0xf, false),
                                         __builtin_amdgcn_update_dpp(0, __double2loint(prev[C - 2]), 0x138, 0xf, 0xf, false));
            if (lane == 0) { s1 = NEG; s2 = NEG; }
            const float cb = qb[j];
            float cl[H];
#pragma unroll
            for (int h = 0; h < H; ++h) cl[h] = yk[h] >= 0 ? score_elem(qz[j][h]) - qs[j] : -INFINITY;
            request(j, r + D);
#pragma unroll
            for (int c = C - 1; c >= 0; --c) {
                const int m = C * lane + c;
                if (m >= S) continue;
                double p;
                if (r == 0) {
                    p = m <= 1 ? 0.0 : NEG;
                } else {
                    const double a1 = c >= 1 ? prev[c >= 1 ? c - 1 : 0] : s1;
                    const double a2 = c >= 2 ? prev[c >= 2 ? c - 2 : 0] : (c == 1 ? s1 : s2);
                    p = log_add64(prev[c], a1);
                    if ((c & 1) && ((skip >> c) & 1)) p = log_add64(p, a2);
                }
                prev[c] = p + (double)((c & 1) ? cl[c >> 1] : cb);
            }
        }
    }
    // ll = lse(last state, last label state) of the last row; the two may sit in different lanes
    double v1 = NEG, v2 = NEG;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        if (C * lane + c == S - 1) v1 = prev[c];
        if (C * lane + c == S - 2) v2 = prev[c];
    }
    v1 = __shfl(v1, (S - 1) / C, 64);
    v2 = __shfl(v2, S >= 2 ? (S - 2) / C : 0, 64);
    if (lane == 0) scores[blockIdx.x] = S >= 2 ? log_add64(v1, v2) : v1;
}

template <typename T>
inline int ctc_score_launch(const T* logits, const int32_t* act_lens, const int32_t* hyps, const int32_t* hyp_lens,
                            const int32_t* n_hyp, int B, int T_, int N, int U, int V, int blank, float* lse, float* lpb,
                            double* scores, int vec_ok, hipStream_t stream) {
    const dim3 grid1(ed_grid_for(T_, 4, max(1, 256 * 16 / B)), B);
    hipLaunchKernelGGL(ctc_score_rows<T>, grid1, dim3(256), 0, stream, logits, act_lens, T_, V, blank, lse, lpb, vec_ok);
    ED_CHECK_LAUNCH("ctc_score_rows");
#define ED_CTC_SCORE(CC)                                                                                              \
    hipLaunchKernelGGL((ctc_score_walk<T, CC>), dim3(B * N), dim3(64), 0, stream, logits, (const float*)lse,          \
                       (const float*)lpb, act_lens, hyps, hyp_lens, n_hyp, T_, N, U, V, scores)
    // C = max(2, ceil(S / 64)) states per lane, rounded up to a power of two, from the call's U (as ctc_launch_walk)
    const int per_lane = (2 * U + 1 + 63) / 64;
    if (per_lane <= 2) ED_CTC_SCORE(2);
    else if (per_lane <= 4) ED_CTC_SCORE(4);
    else if (per_lane <= 8) ED_CTC_SCORE(8);
    else if (per_lane <= 16) ED_CTC_SCORE(16);
    else ED_CTC_SCORE(32);
#undef ED_CTC_SCORE
    ED_CHECK_LAUNCH("ctc_score_walk");
    return ED_OK;
}

}  // namespace

// the two [B, T] float row arrays (lse, lp_blank): no term in V, T U or T N
extern "C" size_t edgedict_ctc_score_workspace_bytes(int B, int T, int N, int U) {
    if (B <= 0 || T <= 0 || N < 1 || N > CTC_SCORE_MAX_N || U < 0 || U > 1023) return 0;
    return 2 * score_up256((size_t)B * T * sizeof(float));
}

extern "C" int edgedict_ctc_score_nbest(const void* logits, int dtype, const int32_t* act_lens, const int32_t* hyps,
                                        const int32_t* hyp_lens, const int32_t* n_hyp, int B, int T, int N, int U, int V,
                                        int blank, double* scores, void* workspace, void* stream_) {
    ED_CHECK_ARG(B > 0 && T > 0 && U >= 0, "ctc_score_nbest: B, T must be positive and U >= 0 (got %d, %d, %d)", B, T, U);
    ED_CHECK_ARG(N >= 1 && N <= CTC_SCORE_MAX_N, "ctc_score_nbest: N = %d outside [1, %d] hypotheses per utterance", N,
                 CTC_SCORE_MAX_N);
    ED_CHECK_ARG(U <= 1023, "ctc_score_nbest: U = %d exceeds the supported maximum of 1023 tokens per hypothesis", U);
    ED_CHECK_ARG((long long)B * N <= 0x7fffffffLL, "ctc_score_nbest: B * N = %lld exceeds the grid", (long long)B * N);
    ED_CHECK_ARG(V >= 2, "ctc_score_nbest: V = %d, need at least the blank and one symbol", V);
    ED_CHECK_ARG(blank >= 0 && blank < V, "ctc_score_nbest: blank %d outside [0,%d)", blank, V);
    ED_CHECK_ARG(dtype == ED_F32 || dtype == ED_BF16, "ctc_score_nbest: unsupported dtype code %d", dtype);
    ED_CHECK_ARG(logits && act_lens && (hyps || U == 0) && hyp_lens && scores && workspace,
                 "ctc_score_nbest: null pointer argument");
    ED_CHECK_ARG(((uintptr_t)workspace & 15) == 0, "ctc_score_nbest: workspace must be 16-byte aligned");
    hipStream_t stream = (hipStream_t)stream_;
    char* p = (char*)workspace;
    float* lse = (float*)p;
    float* lpb = (float*)(p + score_up256((size_t)B * T * sizeof(float)));
    const size_t esz = dtype == ED_F32 ? 4 : 2;
    const int vec_ok = ((V * esz) % 16 == 0) && (((uintptr_t)logits & 15) == 0);
    if (dtype == ED_F32)
        return ctc_score_launch<float>((const float*)logits, act_lens, hyps, hyp_lens, n_hyp, B, T, N, U, V, blank, lse,
                                       lpb, scores, vec_ok, stream);
    return ctc_score_launch<bf16_t>((const bf16_t*)logits, act_lens, hyps, hyp_lens, n_hyp, B, T, N, U, V, blank, lse, lpb,
                                    scores, vec_ok, stream);
}
