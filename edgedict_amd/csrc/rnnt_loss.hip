// RNN-T forward-backward loss for gfx950.
//
// Replaces the third-party warprnnt_pytorch.RNNTLoss operator used at
// rnnt/models.py:221,238 (reference).  Arithmetic = Graves 2012:
//   lp = log_softmax(z);  alpha/beta lattice recursions in log space;  cost = -alpha(T-1,U)-lp_blank
//   d cost / d z(t,u,v) = softmax(v)*exp(a+b-ll) - [v=blank]*exp(a+lp+beta(t+1,u)-ll)
//                                              - [v=y_{u+1}]*exp(a+lp+beta(t,u+1)-ll)
//
// Three HBM-/latency-shaped kernels, none of them GEMM-shaped (no MFMA here on purpose):
//   1. rnnt_lse_gather : one wave64 per lattice cell row (V logits), 16-byte coalesced loads,
//                        online max/sum, writes denominator + blank/label log-probs.   HBM-bound.
//   2. rnnt_alpha_beta : one WAVE per (utterance, direction); a lane owns ceil(U1/64) label columns and
//                        runs one row behind its left neighbour, whose hand-over arrives by a DPP
//                        shuffle (no LDS, no barrier), next row's log-probs requested a step ahead.
//                                                                              latency-bound.
//   3. rnnt_grad       : one wave64 per row again; reads logits once, writes grads once. HBM-bound.
#include "common.hpp"
#include <cfloat>

namespace {

struct WsLayout {
    size_t cells;  // B*T*U1
    size_t off_denom, off_lpb, off_lpl, off_alpha, off_beta, off_ll, total;
};

inline WsLayout ws_layout(int B, int T, int U1) {
    WsLayout w;
    w.cells = (size_t)B * T * U1;
    const size_t cell_bytes = ((w.cells * sizeof(float) + 255) / 256) * 256;
    // alpha / beta / log-likelihoods are float64: the lattice values reach |ll| ~ 1e3 and
    // the gradient needs exp(alpha+beta-ll), i.e. the difference of three such numbers
    w.off_denom = 0;
    w.off_lpb = cell_bytes;
    w.off_lpl = 2 * cell_bytes;
    w.off_alpha = 3 * cell_bytes;
    w.off_beta = 5 * cell_bytes;
    w.off_ll = 7 * cell_bytes;
    w.total = 7 * cell_bytes + (((size_t)2 * B * sizeof(double) + 255) / 256) * 256;
    return w;
}

// ------------------------------------------------------------------ kernel 1
// grid-stride over rows; 4 waves per block, one row per wave per iteration.
// AR = true (alignment-restricted loss): label u of utterance b may be emitted on frames win_lo[b][u] .. win_hi[b][u]
// only - the label log-probability of every other frame is written as -inf, and that plane of the workspace is all the
// lattice walks, the back-trace and the gradient see of the windows.  AR = false is the kernel as it was.
template <typename T, bool AR = false>
__global__ __launch_bounds__(256) void rnnt_lse_gather(
    const T* __restrict__ acts, const int32_t* __restrict__ labels,
    const int32_t* __restrict__ act_lens, const int32_t* __restrict__ label_lens, int B, int Tm,
    int U1, int V, int blank, float* __restrict__ denom, float* __restrict__ lpb,
    float* __restrict__ lpl, int vec_ok, const long long* __restrict__ pk_off,
    const int32_t* __restrict__ win_lo = nullptr, const int32_t* __restrict__ win_hi = nullptr) {
    constexpr int VEC = ElemIO<T>::VEC;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    // grid (x, B): the workgroups of column b walk the VALID cells r = t (U_b + 1) + u of utterance b
    // (cells outside the box are never read) with 32-bit index arithmetic - three 64-bit divisions
    // per row were as much VALU work as the row itself
    const int b = blockIdx.y;
    const int Tb = min(act_lens[b], Tm), Ub = min(label_lens[b], U1 - 1);
    const int Wb = Ub + 1, nvalid = Tb * Wb;
    for (int r = blockIdx.x * 4 + wave; r < nvalid; r += gridDim.x * 4) {
        const int t = r / Wb, u = r - t * Wb;
        const long long row = ((long long)b * Tm + t) * U1 + u;
        // packed lattice: only the valid cells exist, utterance b starts at row pk_off[b] and its
        // rows are (U_b + 1) apart in t
        const long long arow = pk_off ? pk_off[b] + r : row;
        const T* z = acts + arow * (long long)V;
        float m = -INFINITY, s = 0.f;
        if (vec_ok) {
            for (int v = lane * VEC; v < V; v += 64 * VEC) {
                float x[VEC];
                ElemIO<T>::load_vec(z + v, x);
                float mx = x[0];
#pragma unroll
                for (int i = 1; i < VEC; ++i) mx = fmaxf(mx, x[i]);
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
                const float mn = fmaxf(m, x);
                s = s * __expf(m - mn) + __expf(x - mn);
                m = mn;
            }
        }
        // combine the 64 (m, s) pairs
        const float M = wave_max(m);
        const float part = (m == -INFINITY) ? 0.f : s * __expf(m - M);
        const float S = wave_sum(part);
        const float lse = M + logf(S);
        if (lane == 0) {
            denom[row] = lse;
            lpb[row] = ElemIO<T>::load(z + blank) - lse;
            float l = 0.f;
            if (u < Ub) {
                const int y = labels[(long long)b * (U1 - 1) + u];
                l = ElemIO<T>::load(z + y) - lse;
                if (AR && (t < win_lo[(long long)b * (U1 - 1) + u] || t > win_hi[(long long)b * (U1 - 1) + u])) l = -INFINITY;
            }
            lpl[row] = l;
        }
    }
}

// kernel 1 with the row maxima / exp-sums already reduced per 64-column slot by the logits product's
// epilogue (gemm_nt256.hip): half a wave per lattice row combines the `slots` pairs, one lane picks the
// blank / label logits out of the stored row.  Reads 8 * slots + 4 bytes per row instead of 2 V.
// AR as in rnnt_lse_gather.
template <bool AR = false>
__global__ __launch_bounds__(256) void rnnt_lse_from_parts(
    const bf16_t* __restrict__ acts, const float2* __restrict__ parts, int slots,
    const int32_t* __restrict__ labels, const int32_t* __restrict__ act_lens,
    const int32_t* __restrict__ label_lens, int Tm, int U1, int V, int blank,
    float* __restrict__ denom, float* __restrict__ lpb, float* __restrict__ lpl,
    const long long* __restrict__ pk_off, const int32_t* __restrict__ win_lo = nullptr,
    const int32_t* __restrict__ win_hi = nullptr) {
    // ONE LANE per lattice row (no cross-lane reduction, the three outputs of consecutive rows leave as coalesced
    // stores), but the row's `slots` pairs (8 * slots contiguous bytes) reach the lane through LDS: a wave copies the
    // pairs of its next 64 (32) rows - one contiguous block of the packed lattice - with coalesced 16-byte loads and each
    // lane then reads its own row.  Read straight from global memory, lane by lane, the 64 lanes of a load touch 64
    // different lines of which 16 bytes are used; the line is gone from the CU's cache before the loop comes back for
    // the next 16: the PMC counters showed 1.08 GB fetched for 139 MB of pairs (0.20 ms at the HBM roof).
    // The arithmetic per row - pairs merged two at a time in slot order - is unchanged.
    constexpr int WAVE_F4 = 64 * 17;                       // float4 per wave: 64 rows x (16 + 1) or 32 rows x (33 + 1)
    __shared__ float4 stage[4][WAVE_F4];
    const int b = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int Tb = max(0, min(act_lens[b], Tm)), Ub = max(0, min(label_lens[b], U1 - 1));   // as rnnt_alpha_beta
    const int Wb = Ub + 1, nvalid = Tb * Wb;
    const int q4 = slots >> 1;                             // 16-byte pieces per row (slots even on this path)
    const int RP = (slots & 1) ? 0 : (q4 <= 16 ? 64 : (q4 <= 33 ? 32 : 0));   // rows per wave and pass (0: direct loads)
    const int stride = q4 + 1;
    float4* sp = stage[wave];
    const int step = RP ? RP : 64;
    for (int r0 = (blockIdx.x * 4 + wave) * step; r0 < nvalid; r0 += gridDim.x * 4 * step) {
        const int nrows = min(step, nvalid - r0);
        const long long arow0 = pk_off[b] + r0;
        if (RP) {
            const float4* p4 = reinterpret_cast<const float4*>(parts + arow0 * slots);       // slots even: 16-byte aligned
            __builtin_amdgcn_wave_barrier();               // (the previous pass's reads of the stage are done)
            for (int i = lane; i < nrows * q4; i += 64) {
                const int rr = i / q4;
                sp[rr * stride + (i - rr * q4)] = p4[i];
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_wave_barrier();
        }
        if (lane >= nrows) continue;
        const int r = r0 + lane;
        const int t = r / Wb, u = r - t * Wb;
        const long long row = ((long long)b * Tm + t) * U1 + u;
        const long long arow = arow0 + lane;
        float m = -INFINITY, sm = 0.f;
        int k = 0;
        if (RP) {
            for (; k + 1 < slots; k += 2) {
                const float4 p = sp[lane * stride + (k >> 1)];      // (max, sum) of slots k and k + 1
                const float nm = fmaxf(m, fmaxf(p.x, p.z));
                if (nm != -INFINITY) sm = sm * __expf(m - nm) + p.y * __expf(p.x - nm) + p.w * __expf(p.z - nm);
                m = nm;
            }
        } else {
            const float4* p4 = reinterpret_cast<const float4*>(parts + arow * slots);
            for (; (slots & 1) == 0 && k + 1 < slots; k += 2) {
                const float4 p = p4[k >> 1];
                const float nm = fmaxf(m, fmaxf(p.x, p.z));
                if (nm != -INFINITY) sm = sm * __expf(m - nm) + p.y * __expf(p.x - nm) + p.w * __expf(p.z - nm);
                m = nm;
            }
            for (; k < slots; ++k) {                   // odd slot counts: 8-byte loads
                const float2 p = parts[arow * slots + k];
                const float nm = fmaxf(m, p.x);
                if (nm != -INFINITY) sm = sm * __expf(m - nm) + p.y * __expf(p.x - nm);
                m = nm;
            }
        }
        const float lse = m + logf(sm);
        const bf16_t* z = acts + arow * (long long)V;
        denom[row] = lse;
        lpb[row] = bf16_to_f32(z[blank]) - lse;
        float l = 0.f;
        if (u < Ub) l = bf16_to_f32(z[labels[(long long)b * (U1 - 1) + u]]) - lse;
        if (AR && u < Ub && (t < win_lo[(long long)b * (U1 - 1) + u] || t > win_hi[(long long)b * (U1 - 1) + u])) l = -INFINITY;
        lpl[row] = l;
    }
}

// (log_add64 - the log-add with float64 carry every lattice walk below uses - lives in common.hpp: ctc_loss.hip shares it)

// ------------------------------------------------------------------ kernel 2
// ONE WAVE per (utterance, direction): blockIdx.x = 2*b + dir (dir 0: alpha, dir 1: beta), 64 threads.  Lane l owns
// the C = ceil(U1 / 64) consecutive label columns [C l, C l + C) (beta: counted from the right end) and walks them
// down the frames one row per step, one step behind lane l - 1: at step s it is in row s - l.  What a cell needs from
// the column to its left (alpha: a(t,u-1) + lp_label(t,u-1); beta: b(t,u+1)) was produced by the SAME lane one
// statement earlier or by lane l - 1 in the step before - a register handed up one lane with a DPP shuffle; what it
// needs from the row above is the lane's own value of the step before.  No LDS, no barrier: T + ceil(U1/C) - 1 steps
// of C dependent log-adds each (E6D2: 233 steps of 2, against 265 diagonals with a workgroup barrier and an LDS round
// trip each: 0.17 -> 0.03 ms).  Per cell the arithmetic and its operand order are those of the barrier kernel it
// replaces (fp64 carry, fp32 correction term of log_add64 above): alphas, betas and the likelihoods are bit-identical
// to that kernel built with the same log_add64 (the correction term itself changed in rounds 4 and 5).
// VIT = true is the Viterbi walk of the forced aligner: ONE wave per utterance (blockIdx.x = b, direction 0 only), max
// in place of the log-add, v(t,u) written where the alphas go and the best path's score into ll[2 b].  The VIT = false
// instantiation is the kernel as it was.
// Alignment-restricted loss: masked label log-probabilities arrive as -inf and need nothing here.  No sum below has
// +inf as an operand, so no -inf - (-inf) is ever formed; log_add64 returns -inf for two -inf operands and m + 0 for
// one (expf(-inf) = 0); a cell no window-respecting alignment passes through gets alpha = -inf or beta = -inf, and an
// utterance whose windows admit no alignment ll = -inf on both sides.
template <int C, bool VIT = false>
__global__ __launch_bounds__(64) void rnnt_alpha_beta(const float* __restrict__ lpb, const float* __restrict__ lpl,
                                                      const int32_t* __restrict__ act_lens,
                                                      const int32_t* __restrict__ label_lens, int Tm, int U1,
                                                      double* __restrict__ alphas, double* __restrict__ betas,
                                                      double* __restrict__ ll) {
    // log-probabilities are requested D steps ahead of their use (a step is ~0.3 us of dependent arithmetic, an L2
    // round trip ~1 us: one step ahead the recurrence waited for its loads on every row - 0.30 instead of 0.17 ms)
    constexpr int D = C <= 2 ? 8 : (C <= 4 ? 4 : (C <= 8 ? 2 : 1));
    const int b = VIT ? blockIdx.x : blockIdx.x >> 1;
    const int dir = VIT ? 0 : blockIdx.x & 1;
    const int lane = threadIdx.x;
    // clamped exactly as rnnt_lse_gather / rnnt_grad clamp them: malformed lengths (the Python shim
    // rejects them, a raw C-ABI caller may not) cannot index past the [Tm, U1] slab; an empty utterance
    // (Tb <= 0) has likelihood 0 => cost +inf, never garbage
    const int Tb = max(0, min(act_lens[b], Tm)), Ub = max(0, min(label_lens[b], U1 - 1));
    if (Tb == 0) {
        if (lane == 0) ll[2 * b + dir] = -(double)INFINITY;
        return;
    }
    const long long base = (long long)b * Tm * U1;
    const int nlanes = (Ub + C) / C;                 // lanes that own a column <= Ub
    const int nsteps = Tb + nlanes - 1;
    const double NEG = -(double)INFINITY;
    double keep[C];                                  // alpha: a(t-1,u) + lp_blank(t-1,u);  beta: b(t+1,u)
#pragma unroll
    for (int c = 0; c < C; ++c) keep[c] = NEG;
    double out_last = NEG;                           // what the lane to the right needs from this lane's last step
    // column of slot c: alpha u = C lane + c; beta u = Ub - (C lane + c); row number r of this lane -> frame
    auto col = [&](int c) { return dir == 0 ? C * lane + c : Ub - (C * lane + c); };
    auto frame = [&](int r) { return dir == 0 ? r : Tb - 1 - r; };
    float qb[D][C], ql[D][C];                        // ring by STEP: slot s % D holds the row this lane is in at step s
    auto request = [&](int j, int r) {               // (static j)
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const int u = col(c);
            float vb = 0.f, vl = 0.f;
            if (lane < nlanes && r >= 0 && r < Tb && u >= 0 && u <= Ub) {
                const long long idx = base + (long long)frame(r) * U1 + u;
                vb = lpb[idx];
                vl = lpl[idx];
            }
            qb[j][c] = vb;
            ql[j][c] = vl;
        }
    };
#pragma unroll
    for (int j = 0; j < D; ++j) request(j, j - lane);
    for (int s0 = 0; s0 < nsteps; s0 += D) {
#pragma unroll
        for (int j = 0; j < D; ++j) {
            const int s = s0 + j;
            if (s >= nsteps) break;
            const int r = s - lane;                  // rows done before this one
            const bool live = lane < nlanes && r >= 0 && r < Tb;
            // lane l - 1's hand-over of the step before (same row): a whole-wave shift by one lane as two DPP moves
            // (wave_shr:1 - __shfl_up goes through the LDS crossbar and waits for it on every step)
            double side = __hiloint2double(__builtin_amdgcn_update_dpp(0, __double2hiint(out_last), 0x138, 0xf, 0xf, false),
                                           __builtin_amdgcn_update_dpp(0, __double2loint(out_last), 0x138, 0xf, 0xf, false));
            if (lane == 0) side = NEG;
            float cb[C], cl[C];
#pragma unroll
            for (int c = 0; c < C; ++c) { cb[c] = qb[j][c]; cl[c] = ql[j][c]; }
            request(j, r + D);                       // the row of step s + D
            if (live) {
                const int t = frame(r);
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const int u = col(c);
                    if (u < 0 || u > Ub) continue;
                    const long long idx = base + (long long)t * U1 + u;
                    if (dir == 0) {
                        // a(t,u) = lse(a(t-1,u) + lpb(t-1,u), a(t,u-1) + lpl(t,u-1))
                        const double a = (t == 0 && u == 0) ? 0.0 : (VIT ? fmax(keep[c], side) : log_add64(keep[c], side));
                        alphas[idx] = a;
                        keep[c] = a + cb[c];
                        side = (u < Ub) ? a + cl[c] : NEG;
                        if (t == Tb - 1 && u == Ub) ll[2 * b] = a + cb[c];
                    } else {
                        // b(t,u) = lse(b(t+1,u) + lpb(t,u), b(t,u+1) + lpl(t,u))
                        double bv;
                        if (t == Tb - 1 && u == Ub) {
                            bv = cb[c];
                        } else {
                            const double via_label = (u < Ub) ? side + cl[c] : NEG;
                            const double via_blank = (t < Tb - 1) ? keep[c] + cb[c] : NEG;
                            bv = log_add64(via_blank, via_label);
                        }
                        betas[idx] = bv;
                        keep[c] = bv;
                        side = bv;
                        if (t == 0 && u == 0) ll[2 * b + 1] = bv;
                    }
                }
                out_last = side;
            } else {
                out_last = NEG;
            }
        }
    }
}

// single block: costs[b] = -ll_alpha[b]; optionally reduced[0] = reduce_scale * sum_b costs[b]
__global__ __launch_bounds__(256) void rnnt_costs(const double* __restrict__ ll,
                                                  float* __restrict__ costs, int B,
                                                  float* __restrict__ reduced, float reduce_scale) {
    __shared__ float part[4];
    float acc = 0.f;
    for (int b = threadIdx.x; b < B; b += blockDim.x) {
        const float c = (float)(-ll[2 * b]);
        costs[b] = c;
        acc += c;
    }
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0 && reduced) reduced[0] = reduce_scale * (part[0] + part[1] + part[2] + part[3]);
}

// Back-trace of the Viterbi walk (rnnt_alpha_beta<C, true>): one wave per utterance.  Lane 0 walks from (T_b - 1, U_b)
// to (0, 0) and re-forms, with the operations of the forward walk (double + (double)float), the two candidates of which
// v(t,u) is the maximum - one of them is v(t,u) bit for bit, no back-pointers are stored.  TIE RULE: equal candidates
// take the blank predecessor (come from t - 1).  frames[b][u] = frame on which label u is emitted (the step
// (t,u) -> (t,u+1)); the other lanes write the -1 padding behind U_b.  T_b + U_b - 1 dependent steps of four loads.
// AR = true (windows): an utterance whose windows admit no alignment (score -inf) gets a frames row of all -1; on any
// other the walk stays on cells with a finite v, where one candidate still reproduces v(t,u) bit for bit.
template <bool AR = false>
__global__ __launch_bounds__(64) void rnnt_viterbi_backtrace(const float* __restrict__ lpb, const float* __restrict__ lpl,
                                                             const double* __restrict__ v, const double* __restrict__ ll,
                                                             const int32_t* __restrict__ act_lens,
                                                             const int32_t* __restrict__ label_lens, int Tm, int U1,
                                                             int32_t* __restrict__ frames, float* __restrict__ scores) {
    const int b = blockIdx.x;
    const int lane = threadIdx.x;
    const int Tb = max(0, min(act_lens[b], Tm)), Ub = max(0, min(label_lens[b], U1 - 1));   // as rnnt_alpha_beta
    int32_t* fr = frames + (long long)b * (U1 - 1);
    const bool none = AR && ll[2 * b] == -(double)INFINITY;
    for (int u = (Tb > 0 && !none ? Ub : 0) + lane; u < U1 - 1; u += 64) fr[u] = -1;
    if (lane != 0) return;
    scores[b] = (float)ll[2 * b];                    // -inf for an empty utterance
    if (Tb == 0 || none) return;
    const long long base = (long long)b * Tm * U1;
    int t = Tb - 1, u = Ub;
    while (u > 0) {
        bool from_label = (t == 0);
        if (!from_label) {
            const long long up = base + (long long)(t - 1) * U1 + u, left = base + (long long)t * U1 + u - 1;
            const double via_blank = v[up] + (double)lpb[up];
            const double via_label = v[left] + (double)lpl[left];
            from_label = via_label > via_blank;
        }
        if (from_label) {
            fr[u - 1] = t;
            --u;
        } else {
            --t;
        }
    }
}

// log(1 + lambda exp(d)), d <= 0 up to rounding: FastEmit's correction of c_all, on the hardware transcendental units
// with the series of log_add64 below 1e-2 (the term lies in [0, log(1 + lambda)])
__device__ __forceinline__ float fastemit_log1p(float lambda, float d) {
    const float x = lambda * __expf(d);
    return x < 1e-2f ? x * (1.f - x * (0.5f - x * (1.f / 3.f))) : __logf(1.f + x);
}

// ------------------------------------------------------------------ kernel 3
// FastEmit (Yu et al. 2021), FE = true: the gradient through the label emissions is scaled by 1 + lambda,
//   grad(t,u,k) = softmax_k (wb + (1 + lambda) wl) - [k == blank] wb - [k == y] (1 + lambda) wl,
//   wb = exp(a + lpb + beta(t+1,u) - L), wl = exp(a + lpl + beta(t,u+1) - L), wb + wl = exp(a + beta(t,u) - L):
// c_label grows by log1p(lambda) (fe_log1p, formed on the host) and c_all by log(1 + lambda wl / (wb + wl)), the
// exponent lpl + beta(t,u+1) - beta(t,u) formed in fp64 - one read of the lpl plane per CELL.  FE = false is the
// kernel as it was: the three extra arguments are not touched.
// AR = true (alignment-restricted loss, windows masked into the lpl plane by the first stage): a cell with alpha = -inf
// or beta = -inf (no window-respecting alignment passes through it), or of an utterance with L = -inf, gets a zero row
// and its logits are NOT read - the test comes before any arithmetic, which would form -inf - (-inf); a live cell whose
// label is masked (lpl = -inf) has c_label = -inf (wl = 0).  Everything else - arithmetic and operand order per cell -
// is that of AR = false, which is the kernel as it was.
#ifndef ED_GRAD_OCC
#define ED_GRAD_OCC 1
#endif
template <typename T, bool FE, bool AR = false>
__global__ __launch_bounds__(256, ED_GRAD_OCC) void rnnt_grad(
    const T* __restrict__ acts, T* __restrict__ grads, const int32_t* __restrict__ labels,
    const int32_t* __restrict__ act_lens, const int32_t* __restrict__ label_lens, int B, int Tm,
    int U1, int V, int blank, const float* __restrict__ denom, const double* __restrict__ alphas,
    const double* __restrict__ betas, const double* __restrict__ ll, float scale_host,
    const float* __restrict__ scale_dev, int scale_stride, int vec_ok,
    const long long* __restrict__ pk_off, int b0, const float* __restrict__ lpl, float fe_lambda, float fe_log1p) {
    constexpr int VEC = ElemIO<T>::VEC;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    // grid (x, B), 32-bit index arithmetic (see rnnt_lse_gather).  Dense layout: every cell of the
    // [Tm, U1] slab of utterance b is written (zeros outside its box); packed: only the box exists.
    const int b = b0 + blockIdx.y;      // utterances [b0, b0 + gridDim.y) of the batch
    const int Tb = min(act_lens[b], Tm), Ub = min(label_lens[b], U1 - 1);
    const float scale = scale_host * (scale_dev ? scale_dev[(long long)b * scale_stride] : 1.f);
    const int Wb = pk_off ? Ub + 1 : U1, ncells = pk_off ? Tb * Wb : Tm * U1;
    for (int r = blockIdx.x * 4 + wave; r < ncells; r += gridDim.x * 4) {
        const int t = r / Wb, u = r - t * Wb;
        const long long row = ((long long)b * Tm + t) * U1 + u;
        bool inside = (t < Tb && u <= Ub);
        if (AR && inside) {
            const double NEG = -(double)INFINITY;
            inside = !(alphas[row] == NEG || betas[row] == NEG || ll[2 * b] == NEG);
        }
        const long long arow = pk_off ? pk_off[b] + r : row;
        const T* z = acts + arow * (long long)V;
        T* g = grads + arow * (long long)V;
        // the first (for V <= 64 * VEC * 4: the only) batch of logits is requested BEFORE the cell's alpha / beta /
        // denominator are: the row does not depend on them, and behind them it would start a second round trip
        constexpr int NB = 4;
        uint4 raw[NB];
        if (vec_ok && inside) {
#pragma unroll
            for (int j = 0; j < NB; ++j) {
                const int v = (lane + 64 * j) * VEC;
                if (v < V) raw[j] = *reinterpret_cast<const uint4*>(z + v);
            }
        }
        float c_all = 0.f, c_blank = -INFINITY, c_label = -INFINITY;
        int y = -1;
        if (inside) {
            const double a = alphas[row], bt_ = betas[row];
            const double L = ll[2 * b];
            const float lse = denom[row];
            c_all = (float)(a + bt_ - L) - lse;  // exp(z + c_all) = softmax * exp(a+b-L)
            if (t < Tb - 1)
                c_blank = (float)(a + betas[row + U1] - L) - lse;
            else if (u == Ub)
                c_blank = (float)(a - L) - lse;
            if (u < Ub) {
                y = labels[(long long)b * (U1 - 1) + u];
                const double bl = betas[row + 1];
                c_label = (float)(a + bl - L) - lse;
                if (FE) {
                    c_all = (float)((a + bt_ - L) + (double)fastemit_log1p(fe_lambda, (float)((double)lpl[row] + bl - bt_))) - lse;
                    c_label += fe_log1p;
                }
                if (AR && lpl[row] == -INFINITY) c_label = -INFINITY;
            }
        }
        if (vec_ok) {
            for (int v = lane * VEC, j = 0; v < V; v += 64 * VEC, ++j) {
                float o[VEC];
                if (inside) {
                    float x[VEC];
                    if (j < NB) {
                        // (static indices only: a run-time raw[j] would put the array in scratch)
                        const uint4 rv = j == 0 ? raw[0] : (j == 1 ? raw[1] : (j == 2 ? raw[2] : raw[3]));
                        ElemIO<T>::cvt_vec(rv, x);
                    } else {
                        ElemIO<T>::load_vec(z + v, x);
                    }
#pragma unroll
                    for (int i = 0; i < VEC; ++i) {
                        float gv = __expf(x[i] + c_all);
                        if (v + i == blank) gv -= __expf(x[i] + c_blank);
                        if (v + i == y) gv -= __expf(x[i] + c_label);
                        o[i] = gv * scale;
                    }
                } else {
#pragma unroll
                    for (int i = 0; i < VEC; ++i) o[i] = 0.f;
                }
                ElemIO<T>::store_vec(g + v, o);
            }
        } else {
            for (int v = lane; v < V; v += 64) {
                float gv = 0.f;
                if (inside) {
                    const float x = ElemIO<T>::load(z + v);
                    gv = __expf(x + c_all);
                    if (v == blank) gv -= __expf(x + c_blank);
                    if (v == y) gv -= __expf(x + c_label);
                    gv *= scale;
                }
                ElemIO<T>::store(g + v, gv);
            }
        }
    }
}

// rnnt_grad for the PACKED lattice that also leaves the column sums of the gradient matrix (fp32 values in front of the
// store's rounding) as one partial row per workgroup in colsum_parts[blockIdx.y * gridDim.x + blockIdx.x][V]: the joint's
// output-bias gradient is the column sum of this matrix, and a separate pass over its 2.2 GB (E6D2 bench batch) on the
// auxiliary stream beside the encoder's BPTT cost the step 0.4 ms (profiles/r6_colsum.txt).
// Work split: the workgroup's rows are those of rnnt_grad (groups of 4: r = 4 (blockIdx.x + k gridDim.x) + q), but wave w
// owns COLUMN SLICE w (64 * VEC columns: one 16-byte vector per lane) of all four rows of a group instead of one whole
// row - VEC accumulators per lane with static indices, four loads in flight as before.  (Tried first: one row per wave
// with 4 x VEC register accumulators, 1.09 instead of 0.88 ms; LDS ds_add_f32 accumulators, 5.8 ms.)
// Needs 16-byte aligned rows and V <= 4 * 64 * VEC (2048 in bf16, 1024 in f32); arithmetic per cell as in rnnt_grad.
// AR as in rnnt_grad: a dead cell's logits are not read, its row is zeros and adds nothing to the column sums.
template <typename T, bool FE, bool AR = false>
__global__ __launch_bounds__(256, ED_GRAD_OCC) void rnnt_grad_cs(
    const T* __restrict__ acts, T* __restrict__ grads, const int32_t* __restrict__ labels,
    const int32_t* __restrict__ act_lens, const int32_t* __restrict__ label_lens, int B, int Tm,
    int U1, int V, int blank, const float* __restrict__ denom, const double* __restrict__ alphas,
    const double* __restrict__ betas, const double* __restrict__ ll, float scale_host,
    const float* __restrict__ scale_dev, int scale_stride, const long long* __restrict__ pk_off,
    float* __restrict__ colsum_parts, const float* __restrict__ lpl, float fe_lambda, float fe_log1p) {
    constexpr int VEC = ElemIO<T>::VEC;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int b = blockIdx.y;
    const int Tb = min(act_lens[b], Tm), Ub = min(label_lens[b], U1 - 1);
    const float scale = scale_host * (scale_dev ? scale_dev[(long long)b * scale_stride] : 1.f);
    const int Wb = Ub + 1, ncells = Tb * Wb;
    const int v = (wave * 64 + lane) * VEC;          // this lane's columns v .. v + VEC - 1 of every row
    const bool col_live = v < V;
    const double L = ll[2 * b];
    float cs[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) cs[i] = 0.f;
    for (int r0 = blockIdx.x * 4; r0 < ncells; r0 += gridDim.x * 4) {
        uint4 raw[4];
        bool live[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            live[q] = r0 + q < ncells;
            if (AR && live[q]) {
                const int r = r0 + q;
                const int t = r / Wb, u = r - t * Wb;
                const long long row = ((long long)b * Tm + t) * U1 + u;
                const double NEG = -(double)INFINITY;
                live[q] = !(alphas[row] == NEG || betas[row] == NEG || L == NEG);
            }
            if (col_live && live[q]) raw[q] = *reinterpret_cast<const uint4*>(acts + (pk_off[b] + r0 + q) * (long long)V + v);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int r = r0 + q;
            if (r >= ncells) break;
            if (AR && !live[q]) {
                if (col_live) {
                    float o[VEC];
#pragma unroll
                    for (int i = 0; i < VEC; ++i) o[i] = 0.f;
                    ElemIO<T>::store_vec(grads + (pk_off[b] + r) * (long long)V + v, o);
                }
                continue;
            }
            const int t = r / Wb, u = r - t * Wb;
            const long long row = ((long long)b * Tm + t) * U1 + u;
            const double a = alphas[row], bt_ = betas[row];
            const float lse = denom[row];
            float c_all = (float)(a + bt_ - L) - lse;
            float c_blank = -INFINITY, c_label = -INFINITY;
            int y = -1;
            if (t < Tb - 1)
                c_blank = (float)(a + betas[row + U1] - L) - lse;
            else if (u == Ub)
                c_blank = (float)(a - L) - lse;
            if (u < Ub) {
                y = labels[(long long)b * (U1 - 1) + u];
                const double bl = betas[row + 1];
                c_label = (float)(a + bl - L) - lse;
                if (FE) {
                    c_all = (float)((a + bt_ - L) + (double)fastemit_log1p(fe_lambda, (float)((double)lpl[row] + bl - bt_))) - lse;
                    c_label += fe_log1p;
                }
                if (AR && lpl[row] == -INFINITY) c_label = -INFINITY;
            }
            if (col_live) {
                float x[VEC], o[VEC];
                ElemIO<T>::cvt_vec(raw[q], x);
#pragma unroll
                for (int i = 0; i < VEC; ++i) {
                    float gv = __expf(x[i] + c_all);
                    if (v + i == blank) gv -= __expf(x[i] + c_blank);
                    if (v + i == y) gv -= __expf(x[i] + c_label);
                    o[i] = gv * scale;
                    cs[i] += o[i];
                }
                ElemIO<T>::store_vec(grads + (pk_off[b] + r) * (long long)V + v, o);
            }
        }
    }
    if (col_live) {
        float* out = colsum_parts + ((long long)blockIdx.y * gridDim.x + blockIdx.x) * V + v;
#pragma unroll
        for (int i = 0; i < VEC; ++i) out[i] = cs[i];
    }
}

// ------------------------------------------------------------------ window helpers (not on the hot path)
// windows around the frames of an alignment (rnnt_viterbi_backtrace's output, or an outside aligner's): one thread per
// (b, u).  Label u of utterance b: lo = max(0, f - left), hi = min(T_b - 1, f + right); behind the labels the window
// covers every frame (lo = 0, hi = Tm - 1; the loss ignores those entries).  Tm == 0: the largest act_lens of the batch
// (a caller that has the lengths on the device only; B reads per thread).
__global__ __launch_bounds__(256) void rnnt_windows_from_frames(const int32_t* __restrict__ frames,
                                                                const int32_t* __restrict__ act_lens,
                                                                const int32_t* __restrict__ label_lens, int B, int Tm,
                                                                int U, int left, int right, int32_t* __restrict__ lo,
                                                                int32_t* __restrict__ hi) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)B * U) return;
    const int b = (int)(i / U), u = (int)(i - (long long)b * U);
    if (Tm == 0)
        for (int k = 0; k < B; ++k) Tm = max(Tm, act_lens[k]);
    const int Tb = max(0, min(act_lens[b], Tm)), Ub = max(0, min(label_lens[b], U));
    int l = 0, h = Tm - 1;
    if (u < Ub) {
        const long long f = frames[i];
        l = (int)max(0ll, f - left);
        h = (int)min((long long)Tb - 1, f + right);
    }
    lo[i] = l;
    hi[i] = h;
}

// The cells of the lattice a window-respecting alignment can pass through (finite alpha AND finite beta), from the
// windows alone: with elo_u = max(lo_0 .. lo_u) and ehi_u = min(hi_u .. hi_{U_b - 1}, T_b - 1), column u is alive on the
// frames [elo_{u-1}, ehi_u] (column 0 from frame 0, column U_b up to frame T_b - 1), and no alignment exists iff
// elo_u > ehi_u for some u.  Both ends are non-decreasing in u, so the live columns of frame t are the interval
// [#{u : end_u < t}, #{u : start_u <= t} - 1].  One workgroup per utterance: thread 0 forms the two running extremes
// in LDS (U1 <= 2048 steps), a thread per frame then counts.  band[b][t] = (ulo, uhi), (0, -1) where no cell of the
// frame is alive (frames behind T_b; every frame of an utterance without an alignment); cells[b] = live cells.
constexpr int BAND_MAX_U1 = 2048;
__global__ __launch_bounds__(256) void rnnt_band_table(const int32_t* __restrict__ win_lo, const int32_t* __restrict__ win_hi,
                                                       const int32_t* __restrict__ act_lens,
                                                       const int32_t* __restrict__ label_lens, int Tm, int U1,
                                                       int32_t* __restrict__ band, long long* __restrict__ cells) {
    __shared__ int col_start[BAND_MAX_U1], col_end[BAND_MAX_U1];
    __shared__ int feasible;
    __shared__ unsigned long long total;
    const int b = blockIdx.x;
    const int Tb = max(0, min(act_lens[b], Tm)), Ub = max(0, min(label_lens[b], U1 - 1));
    const int32_t* lo = win_lo + (long long)b * (U1 - 1);
    const int32_t* hi = win_hi + (long long)b * (U1 - 1);
    if (threadIdx.x == 0) {
        int ok = Tb > 0, m = 0;
        col_start[0] = 0;
        for (int u = 0; u < Ub; ++u) {
            m = max(m, lo[u]);
            col_start[u + 1] = m;                    // elo_u
        }
        m = Tb - 1;
        col_end[Ub] = m;
        for (int u = Ub - 1; u >= 0; --u) {
            m = min(m, hi[u]);
            col_end[u] = m;                          // ehi_u
            if (col_start[u + 1] > m) ok = 0;
        }
        feasible = ok;
        total = 0ull;
    }
    __syncthreads();
    const bool ok = feasible != 0;
    unsigned long long mine = 0;
    for (int t = threadIdx.x; t < Tm; t += 256) {
        int ulo = 0, uhi = -1;
        if (ok && t < Tb) {
            int below = 0, started = 0;
            for (int u = 0; u <= Ub; ++u) {
                below += col_end[u] < t;
                started += col_start[u] <= t;
            }
            if (below <= started - 1) {
                ulo = below;
                uhi = started - 1;
                mine += (unsigned long long)(uhi - ulo + 1);
            }
        }
        band[((long long)b * Tm + t) * 2] = ulo;
        band[((long long)b * Tm + t) * 2 + 1] = uhi;
    }
    if (mine) atomicAdd(&total, mine);
    __syncthreads();
    if (threadIdx.x == 0) cells[b] = (long long)total;
}

// ------------------------------------------------------------------ band-packed lattice (joint + loss on the live cells)
// Only the cells of the band table exist as rows: row(b,t,u) = row_off[b][t] + (u - ulo[b][t]), ulo <= u <= uhi.  Rows
// of a frame are contiguous, frames of an utterance are contiguous, utterances in batch order: utterance b owns the
// cells[b] rows from row_off[b][0] on; one whose windows admit no alignment owns none.
struct BandArgs {
    const int32_t* band;        // [B][T][2]
    const long long* row_off;   // [B][T]
    const int32_t* row_tu;      // [M_band]: t << 16 | u
    const long long* cells;     // [B]
};

// row_off = exclusive prefix sum of the frame widths in (b, t) order; total[0] = M_band.  One workgroup per utterance:
// its base is the sum of the cells of the utterances in front of it (B reads), the frames are scanned 256 at a time.
__global__ __launch_bounds__(256) void rnnt_band_scan(const int32_t* __restrict__ band, const long long* __restrict__ cells,
                                                      int B, int Tm, long long* __restrict__ row_off,
                                                      long long* __restrict__ total) {
    __shared__ int part[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    long long base = 0;
    for (int k = 0; k < b; ++k) base += cells[k];
    if (b == 0 && tid == 0) {
        long long all = 0;
        for (int k = 0; k < B; ++k) all += cells[k];
        total[0] = all;
    }
    for (int c0 = 0; c0 < Tm; c0 += 256) {
        const int t = c0 + tid;
        int w = 0;
        if (t < Tm) w = max(0, band[((long long)b * Tm + t) * 2 + 1] - band[((long long)b * Tm + t) * 2] + 1);
        part[tid] = w;
        __syncthreads();
        for (int d = 1; d < 256; d <<= 1) {              // inclusive scan of the chunk
            const int add = tid >= d ? part[tid - d] : 0;
            __syncthreads();
            part[tid] += add;
            __syncthreads();
        }
        if (t < Tm) row_off[(long long)b * Tm + t] = base + (part[tid] - w);
        base += part[255];
        __syncthreads();
    }
}

// row_tu[row] = t << 16 | u of every band row: one thread per frame walks the frame's interval
__global__ __launch_bounds__(256) void rnnt_band_fill(const int32_t* __restrict__ band, const long long* __restrict__ row_off,
                                                      int B, int Tm, long long rows, int32_t* __restrict__ row_tu) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)B * Tm) return;
    const int t = (int)(i % Tm);
    const int ulo = band[i * 2], uhi = band[i * 2 + 1];
    const long long r0 = row_off[i];
    for (int u = ulo; u <= uhi; ++u) {
        const long long r = r0 + (u - ulo);
        if (r >= 0 && r < rows) row_tu[r] = (int32_t)(((unsigned)t << 16) | (unsigned)u);
    }
}

// first loss stage on band rows, part 1: the cells of the boxes that are NOT in the band get lp_blank = lp_label = -inf
// and a denominator of 0 - what the lattice walks see of a dead cell on the box path is an alpha or a beta of -inf, and
// log_add64 treats every -inf operand alike, so alpha and beta of the live cells, L and the costs are the box path's.
__global__ __launch_bounds__(256) void rnnt_band_dead_cells(const int32_t* __restrict__ band,
                                                            const int32_t* __restrict__ act_lens,
                                                            const int32_t* __restrict__ label_lens, int Tm, int U1,
                                                            float* __restrict__ denom, float* __restrict__ lpb,
                                                            float* __restrict__ lpl) {
    const int b = blockIdx.y;
    const int Tb = max(0, min(act_lens[b], Tm)), Ub = max(0, min(label_lens[b], U1 - 1));
    const int Wb = Ub + 1, nvalid = Tb * Wb;
    for (int r = blockIdx.x * 256 + threadIdx.x; r < nvalid; r += gridDim.x * 256) {
        const int t = r / Wb, u = r - t * Wb;
        const long long f = (long long)b * Tm + t;
        if (u >= band[f * 2] && u <= band[f * 2 + 1]) continue;
        const long long row = f * U1 + u;
        denom[row] = 0.f;
        lpb[row] = -INFINITY;
        lpl[row] = -INFINITY;
    }
}

// ... part 2: rnnt_lse_gather<T, true> over the band rows of utterance b - the cell comes from row_tu, the logits row is
// the band row; arithmetic, window mask and operand order are that kernel's.
template <typename T>
__global__ __launch_bounds__(256) void rnnt_lse_gather_band(
    const T* __restrict__ acts, const int32_t* __restrict__ labels, const int32_t* __restrict__ act_lens,
    const int32_t* __restrict__ label_lens, int Tm, int U1, int V, int blank, float* __restrict__ denom,
    float* __restrict__ lpb, float* __restrict__ lpl, int vec_ok, const int32_t* __restrict__ win_lo,
    const int32_t* __restrict__ win_hi, BandArgs bd) {
    constexpr int VEC = ElemIO<T>::VEC;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int b = blockIdx.y;
    const int Tb = min(act_lens[b], Tm), Ub = min(label_lens[b], U1 - 1);
    const int nrows = (int)bd.cells[b];
    const long long base = bd.row_off[(long long)b * Tm];
    for (int r = blockIdx.x * 4 + wave; r < nrows; r += gridDim.x * 4) {
        const long long arow = base + r;
        const unsigned tu = (unsigned)bd.row_tu[arow];
        const int t = (int)(tu >> 16), u = (int)(tu & 0xffffu);
        if (t >= Tb || u > Ub) continue;                 // (a table that does not belong to these lengths)
        const long long row = ((long long)b * Tm + t) * U1 + u;
        const T* z = acts + arow * (long long)V;
        float m = -INFINITY, s = 0.f;
        if (vec_ok) {
            for (int v = lane * VEC; v < V; v += 64 * VEC) {
                float x[VEC];
                ElemIO<T>::load_vec(z + v, x);
                float mx = x[0];
#pragma unroll
                for (int i = 1; i < VEC; ++i) mx = fmaxf(mx, x[i]);
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
                const float mn = fmaxf(m, x);
                s = s * __expf(m - mn) + __expf(x - mn);
                m = mn;
            }
        }
        const float M = wave_max(m);
        const float part = (m == -INFINITY) ? 0.f : s * __expf(m - M);
        const float S = wave_sum(part);
        const float lse = M + logf(S);
        if (lane == 0) {
            denom[row] = lse;
            lpb[row] = ElemIO<T>::load(z + blank) - lse;
            float l = 0.f;
            if (u < Ub) {
                const int y = labels[(long long)b * (U1 - 1) + u];
                l = ElemIO<T>::load(z + y) - lse;
                if (t < win_lo[(long long)b * (U1 - 1) + u] || t > win_hi[(long long)b * (U1 - 1) + u]) l = -INFINITY;
            }
            lpl[row] = l;
        }
    }
}

// ... and rnnt_lse_from_parts<true> over the band rows: one lane per row, the rows' pairs staged through LDS a wave's
// block of consecutive band rows at a time; the pairs are merged in that kernel's order.
__global__ __launch_bounds__(256) void rnnt_lse_from_parts_band(
    const bf16_t* __restrict__ acts, const float2* __restrict__ parts, int slots, const int32_t* __restrict__ labels,
    const int32_t* __restrict__ act_lens, const int32_t* __restrict__ label_lens, int Tm, int U1, int V, int blank,
    float* __restrict__ denom, float* __restrict__ lpb, float* __restrict__ lpl, const int32_t* __restrict__ win_lo,
    const int32_t* __restrict__ win_hi, BandArgs bd) {
    constexpr int WAVE_F4 = 64 * 17;
    __shared__ float4 stage[4][WAVE_F4];
    const int b = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int Tb = max(0, min(act_lens[b], Tm)), Ub = max(0, min(label_lens[b], U1 - 1));
    const int nvalid = (int)bd.cells[b];
    const long long base = bd.row_off[(long long)b * Tm];
    const int q4 = slots >> 1;
    const int RP = (slots & 1) ? 0 : (q4 <= 16 ? 64 : (q4 <= 33 ? 32 : 0));
    const int stride = q4 + 1;
    float4* sp = stage[wave];
    const int step = RP ? RP : 64;
    for (int r0 = (blockIdx.x * 4 + wave) * step; r0 < nvalid; r0 += gridDim.x * 4 * step) {
        const int nrows = min(step, nvalid - r0);
        const long long arow0 = base + r0;
        if (RP) {
            const float4* p4 = reinterpret_cast<const float4*>(parts + arow0 * slots);
            __builtin_amdgcn_wave_barrier();
            for (int i = lane; i < nrows * q4; i += 64) {
                const int rr = i / q4;
                sp[rr * stride + (i - rr * q4)] = p4[i];
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_wave_barrier();
        }
        if (lane >= nrows) continue;
        const long long arow = arow0 + lane;
        const unsigned tu = (unsigned)bd.row_tu[arow];
        const int t = (int)(tu >> 16), u = (int)(tu & 0xffffu);
        if (t >= Tb || u > Ub) continue;                 // (a table that does not belong to these lengths)
        const long long row = ((long long)b * Tm + t) * U1 + u;
        float m = -INFINITY, sm = 0.f;
        int k = 0;
        if (RP) {
            for (; k + 1 < slots; k += 2) {
                const float4 p = sp[lane * stride + (k >> 1)];
                const float nm = fmaxf(m, fmaxf(p.x, p.z));
                if (nm != -INFINITY) sm = sm * __expf(m - nm) + p.y * __expf(p.x - nm) + p.w * __expf(p.z - nm);
                m = nm;
            }
        } else {
            const float4* p4 = reinterpret_cast<const float4*>(parts + arow * slots);
            for (; (slots & 1) == 0 && k + 1 < slots; k += 2) {
                const float4 p = p4[k >> 1];
                const float nm = fmaxf(m, fmaxf(p.x, p.z));
                if (nm != -INFINITY) sm = sm * __expf(m - nm) + p.y * __expf(p.x - nm) + p.w * __expf(p.z - nm);
                m = nm;
            }
            for (; k < slots; ++k) {
                const float2 p = parts[arow * slots + k];
                const float nm = fmaxf(m, p.x);
                if (nm != -INFINITY) sm = sm * __expf(m - nm) + p.y * __expf(p.x - nm);
                m = nm;
            }
        }
        const float lse = m + logf(sm);
        const bf16_t* z = acts + arow * (long long)V;
        denom[row] = lse;
        lpb[row] = bf16_to_f32(z[blank]) - lse;
        float l = 0.f;
        if (u < Ub) l = bf16_to_f32(z[labels[(long long)b * (U1 - 1) + u]]) - lse;
        if (u < Ub && (t < win_lo[(long long)b * (U1 - 1) + u] || t > win_hi[(long long)b * (U1 - 1) + u])) l = -INFINITY;
        lpl[row] = l;
    }
}

// rnnt_grad<T, FE, true> over the band rows of utterance b: every row is a live cell, so there is no dead-cell test and
// no zero row; per cell the arithmetic and its operand order are the live-cell code of that kernel.
template <typename T, bool FE>
__global__ __launch_bounds__(256, ED_GRAD_OCC) void rnnt_grad_band(
    const T* __restrict__ acts, T* __restrict__ grads, const int32_t* __restrict__ labels,
    const int32_t* __restrict__ act_lens, const int32_t* __restrict__ label_lens, int Tm, int U1, int V, int blank,
    const float* __restrict__ denom, const double* __restrict__ alphas, const double* __restrict__ betas,
    const double* __restrict__ ll, float scale_host, const float* __restrict__ scale_dev, int scale_stride, int vec_ok,
    const float* __restrict__ lpl, float fe_lambda, float fe_log1p, BandArgs bd) {
    constexpr int VEC = ElemIO<T>::VEC;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int b = blockIdx.y;
    const int Tb = min(act_lens[b], Tm), Ub = min(label_lens[b], U1 - 1);
    const float scale = scale_host * (scale_dev ? scale_dev[(long long)b * scale_stride] : 1.f);
    const int nrows = (int)bd.cells[b];
    const long long base = bd.row_off[(long long)b * Tm];
    for (int r = blockIdx.x * 4 + wave; r < nrows; r += gridDim.x * 4) {
        const long long arow = base + r;
        const unsigned tu = (unsigned)bd.row_tu[arow];
        const int t = (int)(tu >> 16), u = (int)(tu & 0xffffu);
        if (t >= Tb || u > Ub) continue;                 // (a table that does not belong to these lengths)
        const long long row = ((long long)b * Tm + t) * U1 + u;
        const T* z = acts + arow * (long long)V;
        T* g = grads + arow * (long long)V;
        constexpr int NB = 4;
        uint4 raw[NB];
        if (vec_ok) {
#pragma unroll
            for (int j = 0; j < NB; ++j) {
                const int v = (lane + 64 * j) * VEC;
                if (v < V) raw[j] = *reinterpret_cast<const uint4*>(z + v);
            }
        }
        float c_all, c_blank = -INFINITY, c_label = -INFINITY;
        int y = -1;
        {
            const double a = alphas[row], bt_ = betas[row];
            const double L = ll[2 * b];
            const float lse = denom[row];
            c_all = (float)(a + bt_ - L) - lse;
            if (t < Tb - 1)
                c_blank = (float)(a + betas[row + U1] - L) - lse;
            else if (u == Ub)
                c_blank = (float)(a - L) - lse;
            if (u < Ub) {
                y = labels[(long long)b * (U1 - 1) + u];
                const double bl = betas[row + 1];
                c_label = (float)(a + bl - L) - lse;
                if (FE) {
                    c_all = (float)((a + bt_ - L) + (double)fastemit_log1p(fe_lambda, (float)((double)lpl[row] + bl - bt_))) - lse;
                    c_label += fe_log1p;
                }
                if (lpl[row] == -INFINITY) c_label = -INFINITY;
            }
        }
        if (vec_ok) {
            for (int v = lane * VEC, j = 0; v < V; v += 64 * VEC, ++j) {
                float o[VEC], x[VEC];
                if (j < NB) {
                    const uint4 rv = j == 0 ? raw[0] : (j == 1 ? raw[1] : (j == 2 ? raw[2] : raw[3]));
                    ElemIO<T>::cvt_vec(rv, x);
                } else {
                    ElemIO<T>::load_vec(z + v, x);
                }
#pragma unroll
                for (int i = 0; i < VEC; ++i) {
                    float gv = __expf(x[i] + c_all);
                    if (v + i == blank) gv -= __expf(x[i] + c_blank);
                    if (v + i == y) gv -= __expf(x[i] + c_label);
                    o[i] = gv * scale;
                }
                ElemIO<T>::store_vec(g + v, o);
            }
        } else {
            for (int v = lane; v < V; v += 64) {
                const float x = ElemIO<T>::load(z + v);
                float gv = __expf(x + c_all);
                if (v == blank) gv -= __expf(x + c_blank);
                if (v == y) gv -= __expf(x + c_label);
                gv *= scale;
                ElemIO<T>::store(g + v, gv);
            }
        }
    }
}

// rnnt_grad_cs<T, FE, true> over the band rows: work split, limits and arithmetic as there.  Every workgroup writes its
// partial row of column sums, zeros where it had no rows.
template <typename T, bool FE>
__global__ __launch_bounds__(256, ED_GRAD_OCC) void rnnt_grad_cs_band(
    const T* __restrict__ acts, T* __restrict__ grads, const int32_t* __restrict__ labels,
    const int32_t* __restrict__ act_lens, const int32_t* __restrict__ label_lens, int Tm, int U1, int V, int blank,
    const float* __restrict__ denom, const double* __restrict__ alphas, const double* __restrict__ betas,
    const double* __restrict__ ll, float scale_host, const float* __restrict__ scale_dev, int scale_stride,
    float* __restrict__ colsum_parts, const float* __restrict__ lpl, float fe_lambda, float fe_log1p, BandArgs bd) {
    constexpr int VEC = ElemIO<T>::VEC;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int b = blockIdx.y;
    const int Tb = min(act_lens[b], Tm), Ub = min(label_lens[b], U1 - 1);
    const float scale = scale_host * (scale_dev ? scale_dev[(long long)b * scale_stride] : 1.f);
    const int ncells = (int)bd.cells[b];
    const long long base = bd.row_off[(long long)b * Tm];
    const int v = (wave * 64 + lane) * VEC;
    const bool col_live = v < V;
    const double L = ll[2 * b];
    float cs[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) cs[i] = 0.f;
    for (int r0 = blockIdx.x * 4; r0 < ncells; r0 += gridDim.x * 4) {
        uint4 raw[4];
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (col_live && r0 + q < ncells) raw[q] = *reinterpret_cast<const uint4*>(acts + (base + r0 + q) * (long long)V + v);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int r = r0 + q;
            if (r >= ncells) break;
            const unsigned tu = (unsigned)bd.row_tu[base + r];
            const int t = (int)(tu >> 16), u = (int)(tu & 0xffffu);
            if (t >= Tb || u > Ub) continue;             // (a table that does not belong to these lengths)
            const long long row = ((long long)b * Tm + t) * U1 + u;
            const double a = alphas[row], bt_ = betas[row];
            const float lse = denom[row];
            float c_all = (float)(a + bt_ - L) - lse;
            float c_blank = -INFINITY, c_label = -INFINITY;
            int y = -1;
            if (t < Tb - 1)
                c_blank = (float)(a + betas[row + U1] - L) - lse;
            else if (u == Ub)
                c_blank = (float)(a - L) - lse;
            if (u < Ub) {
                y = labels[(long long)b * (U1 - 1) + u];
                const double bl = betas[row + 1];
                c_label = (float)(a + bl - L) - lse;
                if (FE) {
                    c_all = (float)((a + bt_ - L) + (double)fastemit_log1p(fe_lambda, (float)((double)lpl[row] + bl - bt_))) - lse;
                    c_label += fe_log1p;
                }
                if (lpl[row] == -INFINITY) c_label = -INFINITY;
            }
            if (col_live) {
                float x[VEC], o[VEC];
                ElemIO<T>::cvt_vec(raw[q], x);
#pragma unroll
                for (int i = 0; i < VEC; ++i) {
                    float gv = __expf(x[i] + c_all);
                    if (v + i == blank) gv -= __expf(x[i] + c_blank);
                    if (v + i == y) gv -= __expf(x[i] + c_label);
                    o[i] = gv * scale;
                    cs[i] += o[i];
                }
                ElemIO<T>::store_vec(grads + (base + r) * (long long)V + v, o);
            }
        }
    }
    if (col_live) {
        float* out = colsum_parts + ((long long)blockIdx.y * gridDim.x + blockIdx.x) * V + v;
#pragma unroll
        for (int i = 0; i < VEC; ++i) out[i] = cs[i];
    }
}

inline int check_common(int B, int T, int U1, int V, int blank, int dtype) {
    ED_CHECK_ARG(B > 0 && T > 0 && U1 > 0 && V > 0, "rnnt_loss: B,T,U1,V must be positive (got %d,%d,%d,%d)", B, T, U1, V);
    ED_CHECK_ARG(U1 <= 1024, "rnnt_loss: U+1 = %d exceeds the supported maximum of 1024", U1);
    ED_CHECK_ARG(blank >= 0 && blank < V, "rnnt_loss: blank %d outside [0,%d)", blank, V);
    ED_CHECK_ARG(dtype == ED_F32 || dtype == ED_BF16, "rnnt_loss: unsupported dtype code %d", dtype);
    return ED_OK;
}

}  // namespace

extern "C" size_t edgedict_rnnt_workspace_bytes(int B, int T, int U1) {
    if (B <= 0 || T <= 0 || U1 <= 0) return 0;
    return ws_layout(B, T, U1).total;
}

extern "C" const void* edgedict_rnnt_workspace_view(const void* workspace, int B, int T, int U1,
                                                     int which) {
    const WsLayout w = ws_layout(B, T, U1);
    const char* p = (const char*)workspace;
    switch (which) {
        case 0: return p + w.off_denom;
        case 1: return p + w.off_alpha;
        case 2: return p + w.off_beta;
        case 3: return p + w.off_ll;
        case 4: return p + w.off_lpb;
        case 5: return p + w.off_lpl;
    }
    return nullptr;
}

static int loss_forward(const void* acts, int acts_dtype, const int32_t* labels,
                        const int32_t* act_lens, const int32_t* label_lens, int B, int T, int U1,
                        int V, int blank, float* costs, float* reduced, float reduce_scale,
                        void* workspace, const long long* pk_off, void* stream_,
                        const float* lse_parts = nullptr, int lse_slots = 0,
                        int32_t* al_frames = nullptr, float* al_scores = nullptr,
                        const int32_t* win_lo = nullptr, const int32_t* win_hi = nullptr,
                        const BandArgs* band = nullptr) {
    // al_scores set: the forced aligner (edgedict_rnnt_align*): same first stage, then the Viterbi walk and its
    // back-trace in place of the two lattice walks and the costs.  win_lo set: the alignment-restricted entry points
    // (*_ar) - the first stage masks the label log-probabilities, the back-trace knows about impossible windows
    if (int rc = check_common(B, T, U1, V, blank, acts_dtype)) return rc;
    ED_CHECK_ARG(acts && (labels || U1 == 1) && act_lens && label_lens && (costs || al_scores) && workspace,
                 "rnnt_loss_forward: null pointer argument");
    ED_CHECK_ARG(!al_scores || al_frames || U1 == 1, "rnnt_align: null frames");
    ED_CHECK_ARG(((uintptr_t)workspace & 15) == 0, "rnnt_loss_forward: workspace must be 16-byte aligned");
    hipStream_t stream = (hipStream_t)stream_;
    const WsLayout w = ws_layout(B, T, U1);
    char* p = (char*)workspace;
    float* denom = (float*)(p + w.off_denom);
    float* lpb = (float*)(p + w.off_lpb);
    float* lpl = (float*)(p + w.off_lpl);
    double* alphas = (double*)(p + w.off_alpha);
    double* betas = (double*)(p + w.off_beta);
    double* ll = (double*)(p + w.off_ll);

    const size_t esz = acts_dtype == ED_F32 ? 4 : 2;
    const int vec_ok = ((V * esz) % 16 == 0) && (((uintptr_t)acts & 15) == 0);
    const dim3 grid1(ed_grid_for((long long)T * U1, 4, max(1, 256 * 16 / B)), B);
    if (band) {
        // band rows (band != null: *_band entry points): the dead cells of the boxes, then the live rows
        const dim3 gridp(ed_grid_for((long long)T * U1, 256, max(1, 256 * 16 / B)), B);
        hipLaunchKernelGGL(rnnt_band_dead_cells, gridp, dim3(256), 0, stream, band->band, act_lens, label_lens, T, U1,
                           denom, lpb, lpl);
        ED_CHECK_LAUNCH("rnnt_band_dead_cells");
        if (lse_parts) {
            ED_CHECK_ARG(((uintptr_t)lse_parts & 15) == 0, "rnnt_loss_forward_band_parts: lse_parts must be 16-byte aligned");
            hipLaunchKernelGGL(rnnt_lse_from_parts_band, gridp, dim3(256), 0, stream, (const bf16_t*)acts,
                               (const float2*)lse_parts, lse_slots, labels, act_lens, label_lens, T, U1, V, blank, denom,
                               lpb, lpl, win_lo, win_hi, *band);
        } else if (acts_dtype == ED_F32)
            hipLaunchKernelGGL(rnnt_lse_gather_band<float>, grid1, dim3(256), 0, stream, (const float*)acts, labels,
                               act_lens, label_lens, T, U1, V, blank, denom, lpb, lpl, vec_ok, win_lo, win_hi, *band);
        else
            hipLaunchKernelGGL(rnnt_lse_gather_band<bf16_t>, grid1, dim3(256), 0, stream, (const bf16_t*)acts, labels,
                               act_lens, label_lens, T, U1, V, blank, denom, lpb, lpl, vec_ok, win_lo, win_hi, *band);
    } else if (lse_parts) {
        ED_CHECK_ARG(((uintptr_t)lse_parts & 15) == 0, "rnnt_loss_forward: lse_parts must be 16-byte aligned");
        ED_CHECK_ARG(acts_dtype == ED_BF16 && pk_off && lse_slots > 0,
                     "rnnt_loss_forward: log-sum-exp partials need bf16 logits on the packed lattice");
        const dim3 gridp(ed_grid_for((long long)T * U1, 256, max(1, 256 * 16 / B)), B);
        if (win_lo)
            hipLaunchKernelGGL(rnnt_lse_from_parts<true>, gridp, dim3(256), 0, stream, (const bf16_t*)acts,
                               (const float2*)lse_parts, lse_slots, labels, act_lens, label_lens, T, U1, V,
                               blank, denom, lpb, lpl, pk_off, win_lo, win_hi);
        else
            hipLaunchKernelGGL(rnnt_lse_from_parts<false>, gridp, dim3(256), 0, stream, (const bf16_t*)acts,
                               (const float2*)lse_parts, lse_slots, labels, act_lens, label_lens, T, U1, V,
                               blank, denom, lpb, lpl, pk_off, nullptr, nullptr);
    } else if (win_lo) {
        if (acts_dtype == ED_F32)
            hipLaunchKernelGGL((rnnt_lse_gather<float, true>), grid1, dim3(256), 0, stream,
                               (const float*)acts, labels, act_lens, label_lens, B, T, U1, V, blank,
                               denom, lpb, lpl, vec_ok, pk_off, win_lo, win_hi);
        else
            hipLaunchKernelGGL((rnnt_lse_gather<bf16_t, true>), grid1, dim3(256), 0, stream,
                               (const bf16_t*)acts, labels, act_lens, label_lens, B, T, U1, V, blank,
                               denom, lpb, lpl, vec_ok, pk_off, win_lo, win_hi);
    } else if (acts_dtype == ED_F32)
        hipLaunchKernelGGL((rnnt_lse_gather<float, false>), grid1, dim3(256), 0, stream,
                           (const float*)acts, labels, act_lens, label_lens, B, T, U1, V, blank,
                           denom, lpb, lpl, vec_ok, pk_off, nullptr, nullptr);
    else
        hipLaunchKernelGGL((rnnt_lse_gather<bf16_t, false>), grid1, dim3(256), 0, stream,
                           (const bf16_t*)acts, labels, act_lens, label_lens, B, T, U1, V, blank,
                           denom, lpb, lpl, vec_ok, pk_off, nullptr, nullptr);
    ED_CHECK_LAUNCH("rnnt_lse_gather");

    // one wave per (utterance, direction), C = ceil(U1 / 64) label columns per lane (rounded up to a power of two).
    // The one limit is check_common's U1 <= 1024, the same for the loss and the aligner: C = 16 is the widest walk
#define ED_AB_LAUNCH(CC)                                                                                              \
    do {                                                                                                              \
        if (al_scores)                                                                                                \
            hipLaunchKernelGGL((rnnt_alpha_beta<CC, true>), dim3(B), dim3(64), 0, stream, lpb, lpl, act_lens,         \
                               label_lens, T, U1, alphas, betas, ll);                                                 \
        else                                                                                                          \
            hipLaunchKernelGGL(rnnt_alpha_beta<CC>, dim3(2 * B), dim3(64), 0, stream, lpb, lpl, act_lens, label_lens, \
                               T, U1, alphas, betas, ll);                                                             \
    } while (0)
    const int cols = (U1 + 63) / 64;
    if (cols <= 1) ED_AB_LAUNCH(1);
    else if (cols <= 2) ED_AB_LAUNCH(2);
    else if (cols <= 4) ED_AB_LAUNCH(4);
    else if (cols <= 8) ED_AB_LAUNCH(8);
    else ED_AB_LAUNCH(16);
#undef ED_AB_LAUNCH
    ED_CHECK_LAUNCH("rnnt_alpha_beta");
    if (al_scores) {
        if (win_lo)
            hipLaunchKernelGGL(rnnt_viterbi_backtrace<true>, dim3(B), dim3(64), 0, stream, lpb, lpl, alphas, ll, act_lens,
                               label_lens, T, U1, al_frames, al_scores);
        else
            hipLaunchKernelGGL(rnnt_viterbi_backtrace<false>, dim3(B), dim3(64), 0, stream, lpb, lpl, alphas, ll, act_lens,
                               label_lens, T, U1, al_frames, al_scores);
        ED_CHECK_LAUNCH("rnnt_viterbi_backtrace");
        return ED_OK;
    }
    hipLaunchKernelGGL(rnnt_costs, dim3(1), dim3(256), 0, stream, ll, costs, B, reduced,
                       reduce_scale);
    ED_CHECK_LAUNCH("rnnt_costs");
    return ED_OK;
}

extern "C" int edgedict_rnnt_loss_forward(const void* acts, int acts_dtype, const int32_t* labels,
                                          const int32_t* act_lens, const int32_t* label_lens,
                                          int B, int T, int U1, int V, int blank, float* costs,
                                          float* reduced, float reduce_scale, void* workspace,
                                          void* stream_) {
    return loss_forward(acts, acts_dtype, labels, act_lens, label_lens, B, T, U1, V, blank, costs,
                        reduced, reduce_scale, workspace, nullptr, stream_);
}

extern "C" int edgedict_rnnt_loss_forward_packed(const void* acts, int acts_dtype,
                                                 const int32_t* labels, const int32_t* act_lens,
                                                 const int32_t* label_lens,
                                                 const long long* row_offsets, int B, int T, int U1,
                                                 int V, int blank, float* costs, float* reduced,
                                                 float reduce_scale, void* workspace, void* stream_) {
    ED_CHECK_ARG(row_offsets, "rnnt_loss_forward_packed: null row_offsets");
    return loss_forward(acts, acts_dtype, labels, act_lens, label_lens, B, T, U1, V, blank, costs,
                        reduced, reduce_scale, workspace, row_offsets, stream_);
}

extern "C" int edgedict_rnnt_loss_forward_packed_parts(const void* acts, const int32_t* labels,
                                                       const int32_t* act_lens,
                                                       const int32_t* label_lens,
                                                       const long long* row_offsets, int B, int T,
                                                       int U1, int V, int blank, float* costs,
                                                       float* reduced, float reduce_scale,
                                                       void* workspace, const float* lse_parts,
                                                       int lse_slots, void* stream_) {
    ED_CHECK_ARG(row_offsets && lse_parts, "rnnt_loss_forward_packed_parts: null pointer");
    ED_CHECK_ARG(lse_slots == (V + 63) / 64, "rnnt_loss_forward_packed_parts: lse_slots must be ceil(V / 64)");
    return loss_forward(acts, ED_BF16, labels, act_lens, label_lens, B, T, U1, V, blank, costs,
                        reduced, reduce_scale, workspace, row_offsets, stream_, lse_parts, lse_slots);
}

// workgroups per utterance of rnnt_grad (grid.x; grid.y = utterances)
static int grad_grid_x(int B, int T, int U1) { return ed_grid_for((long long)T * U1, 4, max(1, 256 * 16 / B)); }

static int loss_backward(const void* acts, int acts_dtype, void* grads, const int32_t* labels,
                         const int32_t* act_lens, const int32_t* label_lens, int B, int T, int U1,
                         int V, int blank, const void* workspace, float grad_scale_host,
                         const float* grad_scale_dev, int grad_scale_stride,
                         const long long* pk_off, void* stream_, int b0 = 0, int nb = -1,
                         float* colsum_parts = nullptr, float fe_lambda = 0.f, bool ar = false,
                         const BandArgs* band = nullptr) {
    // (first: a bad lambda is refused whatever else the call holds, before any launch)
    ED_CHECK_ARG(fe_lambda >= 0.f && fe_lambda <= FLT_MAX, "rnnt_loss_backward: fastemit_lambda must be finite and >= 0 (got %g)",
                 (double)fe_lambda);
    if (int rc = check_common(B, T, U1, V, blank, acts_dtype)) return rc;
    if (nb < 0) nb = B - b0;
    ED_CHECK_ARG(b0 >= 0 && nb >= 0 && b0 + nb <= B, "rnnt_loss_backward: utterance range [%d, %d) outside the batch of %d", b0, b0 + nb, B);
    if (nb == 0) return ED_OK;
    ED_CHECK_ARG(acts && grads && (labels || U1 == 1) && act_lens && label_lens && workspace,
                 "rnnt_loss_backward: null pointer argument");
    hipStream_t stream = (hipStream_t)stream_;
    const WsLayout w = ws_layout(B, T, U1);
    const char* p = (const char*)workspace;
    const float* denom = (const float*)(p + w.off_denom);
    const double* alphas = (const double*)(p + w.off_alpha);
    const double* betas = (const double*)(p + w.off_beta);
    const double* ll = (const double*)(p + w.off_ll);
    const float* lpl = (const float*)(p + w.off_lpl);
    // FastEmit is a template parameter of the gradient kernels: lambda == 0 launches the instantiation without it
    const bool fe = fe_lambda > 0.f;
    const float fe_log1p = log1pf(fe_lambda);
    const size_t esz = acts_dtype == ED_F32 ? 4 : 2;
    const int vec_ok = ((V * esz) % 16 == 0) && (((uintptr_t)acts & 15) == 0) &&
                       (((uintptr_t)grads & 15) == 0);
    const dim3 grid(grad_grid_x(B, T, U1), nb);
    if (band) {
        // band rows (*_band entry points): the whole batch in one pass, no dead rows to zero
        const int cs_width = 4 * 64 * (acts_dtype == ED_F32 ? 4 : 8);
        ED_CHECK_ARG(b0 == 0 && nb == B, "rnnt_loss_backward_band: no utterance ranges");
        ED_CHECK_ARG(!colsum_parts || (vec_ok && V <= cs_width),
                     "rnnt_loss_backward_band_colsum: fused column sums need 16-byte aligned rows and V <= %d (got V = %d)",
                     cs_width, V);
#define ED_BAND_LAUNCH(TT, FE)                                                                                         \
    do {                                                                                                               \
        if (colsum_parts)                                                                                              \
            hipLaunchKernelGGL((rnnt_grad_cs_band<TT, FE>), grid, dim3(256), 0, stream, (const TT*)acts, (TT*)grads,   \
                               labels, act_lens, label_lens, T, U1, V, blank, denom, alphas, betas, ll,                \
                               grad_scale_host, grad_scale_dev, grad_scale_stride, colsum_parts, lpl, fe_lambda,       \
                               fe_log1p, *band);                                                                       \
        else                                                                                                           \
            hipLaunchKernelGGL((rnnt_grad_band<TT, FE>), grid, dim3(256), 0, stream, (const TT*)acts, (TT*)grads,      \
                               labels, act_lens, label_lens, T, U1, V, blank, denom, alphas, betas, ll,                \
                               grad_scale_host, grad_scale_dev, grad_scale_stride, vec_ok, lpl, fe_lambda, fe_log1p,   \
                               *band);                                                                                 \
    } while (0)
        if (acts_dtype == ED_F32) {
            if (fe) ED_BAND_LAUNCH(float, true);
            else ED_BAND_LAUNCH(float, false);
        } else {
            if (fe) ED_BAND_LAUNCH(bf16_t, true);
            else ED_BAND_LAUNCH(bf16_t, false);
        }
#undef ED_BAND_LAUNCH
        ED_CHECK_LAUNCH("rnnt_grad_band");
        return ED_OK;
    }
    if (colsum_parts) {
        const int cs_width = 4 * 64 * (acts_dtype == ED_F32 ? 4 : 8);      // four column slices of 64 lanes x 16 bytes
        ED_CHECK_ARG(vec_ok && V <= cs_width && pk_off && b0 == 0 && nb == B,
                     "rnnt_loss_backward: fused column sums need the packed lattice, 16-byte aligned rows and V <= %d (got V = %d)",
                     cs_width, V);
#define ED_CS_LAUNCH(TT, FE)                                                                                           \
    hipLaunchKernelGGL((rnnt_grad_cs<TT, FE, AR>), grid, dim3(256), 0, stream, (const TT*)acts, (TT*)grads, labels, act_lens, \
                       label_lens, B, T, U1, V, blank, denom, alphas, betas, ll, grad_scale_host, grad_scale_dev,        \
                       grad_scale_stride, pk_off, colsum_parts, lpl, fe_lambda, fe_log1p)
#define ED_CS_PICK(AR_)                                  \
    do {                                                 \
        constexpr bool AR = AR_;                         \
        if (acts_dtype == ED_F32) {                      \
            if (fe) ED_CS_LAUNCH(float, true);           \
            else ED_CS_LAUNCH(float, false);             \
        } else {                                         \
            if (fe) ED_CS_LAUNCH(bf16_t, true);          \
            else ED_CS_LAUNCH(bf16_t, false);            \
        }                                                \
    } while (0)
        if (ar) ED_CS_PICK(true);
        else ED_CS_PICK(false);
#undef ED_CS_PICK
#undef ED_CS_LAUNCH
        ED_CHECK_LAUNCH("rnnt_grad_cs");
        return ED_OK;
    }
#define ED_GRAD_LAUNCH(TT, FE)                                                                                         \
    hipLaunchKernelGGL((rnnt_grad<TT, FE, AR>), grid, dim3(256), 0, stream, (const TT*)acts, (TT*)grads, labels, act_lens, \
                       label_lens, B, T, U1, V, blank, denom, alphas, betas, ll, grad_scale_host, grad_scale_dev,     \
                       grad_scale_stride, vec_ok, pk_off, b0, lpl, fe_lambda, fe_log1p)
#define ED_GRAD_PICK(AR_)                                \
    do {                                                 \
        constexpr bool AR = AR_;                         \
        if (acts_dtype == ED_F32) {                      \
            if (fe) ED_GRAD_LAUNCH(float, true);         \
            else ED_GRAD_LAUNCH(float, false);           \
        } else {                                         \
            if (fe) ED_GRAD_LAUNCH(bf16_t, true);        \
            else ED_GRAD_LAUNCH(bf16_t, false);          \
        }                                                \
    } while (0)
    if (ar) ED_GRAD_PICK(true);
    else ED_GRAD_PICK(false);
#undef ED_GRAD_PICK
#undef ED_GRAD_LAUNCH
    ED_CHECK_LAUNCH("rnnt_grad");
    return ED_OK;
}

extern "C" int edgedict_rnnt_loss_backward(const void* acts, int acts_dtype, void* grads,
                                           const int32_t* labels, const int32_t* act_lens,
                                           const int32_t* label_lens, int B, int T, int U1, int V,
                                           int blank, const void* workspace, float grad_scale_host,
                                           const float* grad_scale_dev, int grad_scale_stride,
                                           void* stream_) {
    return loss_backward(acts, acts_dtype, grads, labels, act_lens, label_lens, B, T, U1, V, blank,
                         workspace, grad_scale_host, grad_scale_dev, grad_scale_stride, nullptr, stream_);
}

extern "C" int edgedict_rnnt_loss_backward_packed(const void* acts, int acts_dtype, void* grads,
                                                  const int32_t* labels, const int32_t* act_lens,
                                                  const int32_t* label_lens,
                                                  const long long* row_offsets, int B, int T, int U1,
                                                  int V, int blank, const void* workspace,
                                                  float grad_scale_host, const float* grad_scale_dev,
                                                  int grad_scale_stride, void* stream_) {
    ED_CHECK_ARG(row_offsets, "rnnt_loss_backward_packed: null row_offsets");
    return loss_backward(acts, acts_dtype, grads, labels, act_lens, label_lens, B, T, U1, V, blank,
                         workspace, grad_scale_host, grad_scale_dev, grad_scale_stride, row_offsets,
                         stream_);
}

extern "C" int edgedict_rnnt_grad_colsum_rows(int acts_dtype, int B, int T, int U1, int V) {
    if (B <= 0 || T <= 0 || U1 <= 0 || V <= 0 || (acts_dtype != ED_F32 && acts_dtype != ED_BF16)) return 0;
    const int esz = acts_dtype == ED_F32 ? 4 : 2;
    if ((V * esz) % 16 != 0 || V > 4 * 64 * (16 / esz)) return 0;
    return grad_grid_x(B, T, U1) * B;
}

extern "C" int edgedict_rnnt_loss_backward_packed_colsum(const void* acts, int acts_dtype, void* grads,
                                                         const int32_t* labels, const int32_t* act_lens,
                                                         const int32_t* label_lens,
                                                         const long long* row_offsets, int B, int T, int U1,
                                                         int V, int blank, const void* workspace,
                                                         float grad_scale_host, const float* grad_scale_dev,
                                                         int grad_scale_stride, float* colsum_parts, void* stream_) {
    ED_CHECK_ARG(row_offsets && colsum_parts, "rnnt_loss_backward_packed_colsum: null pointer");
    return loss_backward(acts, acts_dtype, grads, labels, act_lens, label_lens, B, T, U1, V, blank,
                         workspace, grad_scale_host, grad_scale_dev, grad_scale_stride, row_offsets,
                         stream_, 0, -1, colsum_parts);
}

extern "C" int edgedict_rnnt_loss_backward_packed_range(const void* acts, int acts_dtype, void* grads,
                                                        const int32_t* labels, const int32_t* act_lens,
                                                        const int32_t* label_lens,
                                                        const long long* row_offsets, int B, int T, int U1,
                                                        int V, int blank, const void* workspace,
                                                        float grad_scale_host, const float* grad_scale_dev,
                                                        int grad_scale_stride, int b0, int nb, void* stream_) {
    ED_CHECK_ARG(row_offsets, "rnnt_loss_backward_packed_range: null row_offsets");
    return loss_backward(acts, acts_dtype, grads, labels, act_lens, label_lens, B, T, U1, V, blank,
                         workspace, grad_scale_host, grad_scale_dev, grad_scale_stride, row_offsets,
                         stream_, b0, nb);
}

// ---------------------------------------------------------------------------------------------- FastEmit entry points
// the plain entry points above with `fastemit_lambda` (>= 0, finite): only the gradient changes, the costs the forward
// call returned stay the plain negative log-likelihood.  lambda == 0 runs the kernels of the plain entry points.
extern "C" int edgedict_rnnt_loss_backward_fe(const void* acts, int acts_dtype, void* grads, const int32_t* labels,
                                              const int32_t* act_lens, const int32_t* label_lens, int B, int T, int U1,
                                              int V, int blank, const void* workspace, float grad_scale_host,
                                              const float* grad_scale_dev, int grad_scale_stride,
                                              float fastemit_lambda, void* stream_) {
    return loss_backward(acts, acts_dtype, grads, labels, act_lens, label_lens, B, T, U1, V, blank, workspace,
                         grad_scale_host, grad_scale_dev, grad_scale_stride, nullptr, stream_, 0, -1, nullptr,
                         fastemit_lambda);
}

extern "C" int edgedict_rnnt_loss_backward_packed_fe(const void* acts, int acts_dtype, void* grads,
                                                     const int32_t* labels, const int32_t* act_lens,
                                                     const int32_t* label_lens, const long long* row_offsets, int B,
                                                     int T, int U1, int V, int blank, const void* workspace,
                                                     float grad_scale_host, const float* grad_scale_dev,
                                                     int grad_scale_stride, float fastemit_lambda, void* stream_) {
    ED_CHECK_ARG(fastemit_lambda >= 0.f && fastemit_lambda <= FLT_MAX,
                 "rnnt_loss_backward_packed_fe: fastemit_lambda must be finite and >= 0 (got %g)", (double)fastemit_lambda);
    ED_CHECK_ARG(row_offsets, "rnnt_loss_backward_packed_fe: null row_offsets");
    return loss_backward(acts, acts_dtype, grads, labels, act_lens, label_lens, B, T, U1, V, blank, workspace,
                         grad_scale_host, grad_scale_dev, grad_scale_stride, row_offsets, stream_, 0, -1, nullptr,
                         fastemit_lambda);
}

extern "C" int edgedict_rnnt_loss_backward_packed_colsum_fe(const void* acts, int acts_dtype, void* grads,
                                                            const int32_t* labels, const int32_t* act_lens,
                                                            const int32_t* label_lens, const long long* row_offsets,
                                                            int B, int T, int U1, int V, int blank,
                                                            const void* workspace, float grad_scale_host,
                                                            const float* grad_scale_dev, int grad_scale_stride,
                                                            float* colsum_parts, float fastemit_lambda, void* stream_) {
    ED_CHECK_ARG(fastemit_lambda >= 0.f && fastemit_lambda <= FLT_MAX,
                 "rnnt_loss_backward_packed_colsum_fe: fastemit_lambda must be finite and >= 0 (got %g)", (double)fastemit_lambda);
    ED_CHECK_ARG(row_offsets && colsum_parts, "rnnt_loss_backward_packed_colsum_fe: null pointer");
    return loss_backward(acts, acts_dtype, grads, labels, act_lens, label_lens, B, T, U1, V, blank, workspace,
                         grad_scale_host, grad_scale_dev, grad_scale_stride, row_offsets, stream_, 0, -1, colsum_parts,
                         fastemit_lambda);
}

extern "C" int edgedict_rnnt_loss_backward_packed_range_fe(const void* acts, int acts_dtype, void* grads,
                                                           const int32_t* labels, const int32_t* act_lens,
                                                           const int32_t* label_lens, const long long* row_offsets,
                                                           int B, int T, int U1, int V, int blank,
                                                           const void* workspace, float grad_scale_host,
                                                           const float* grad_scale_dev, int grad_scale_stride, int b0,
                                                           int nb, float fastemit_lambda, void* stream_) {
    ED_CHECK_ARG(fastemit_lambda >= 0.f && fastemit_lambda <= FLT_MAX,
                 "rnnt_loss_backward_packed_range_fe: fastemit_lambda must be finite and >= 0 (got %g)", (double)fastemit_lambda);
    ED_CHECK_ARG(row_offsets, "rnnt_loss_backward_packed_range_fe: null row_offsets");
    return loss_backward(acts, acts_dtype, grads, labels, act_lens, label_lens, B, T, U1, V, blank, workspace,
                         grad_scale_host, grad_scale_dev, grad_scale_stride, row_offsets, stream_, b0, nb, nullptr,
                         fastemit_lambda);
}

// ---------------------------------------------------------------------------------------------------- forced alignment
// Viterbi over the lattice of the loss: v(t,u) = max(v(t-1,u) + lpb(t-1,u), v(t,u-1) + lpl(t,u-1)),
// score = v(T_b-1,U_b) + lpb(T_b-1,U_b).  Arguments as the forward entry points', frames [B][U1-1] (frame on which
// label u is emitted, -1 behind U_b) and scores [B] in place of costs / reduced.  Ties take the blank predecessor.
extern "C" int edgedict_rnnt_align(const void* acts, int acts_dtype, const int32_t* labels, const int32_t* act_lens,
                                   const int32_t* label_lens, int B, int T, int U1, int V, int blank, int32_t* frames,
                                   float* scores, void* workspace, void* stream_) {
    ED_CHECK_ARG(scores, "rnnt_align: null scores");
    return loss_forward(acts, acts_dtype, labels, act_lens, label_lens, B, T, U1, V, blank, nullptr, nullptr, 0.f,
                        workspace, nullptr, stream_, nullptr, 0, frames, scores);
}

extern "C" int edgedict_rnnt_align_packed(const void* acts, int acts_dtype, const int32_t* labels,
                                          const int32_t* act_lens, const int32_t* label_lens,
                                          const long long* row_offsets, int B, int T, int U1, int V, int blank,
                                          int32_t* frames, float* scores, void* workspace, void* stream_) {
    ED_CHECK_ARG(row_offsets && scores, "rnnt_align_packed: null pointer");
    return loss_forward(acts, acts_dtype, labels, act_lens, label_lens, B, T, U1, V, blank, nullptr, nullptr, 0.f,
                        workspace, row_offsets, stream_, nullptr, 0, frames, scores);
}

extern "C" int edgedict_rnnt_align_packed_parts(const void* acts, const int32_t* labels, const int32_t* act_lens,
                                                const int32_t* label_lens, const long long* row_offsets, int B, int T,
                                                int U1, int V, int blank, int32_t* frames, float* scores,
                                                void* workspace, const float* lse_parts, int lse_slots, void* stream_) {
    ED_CHECK_ARG(row_offsets && lse_parts && scores, "rnnt_align_packed_parts: null pointer");
    ED_CHECK_ARG(lse_slots == (V + 63) / 64, "rnnt_align_packed_parts: lse_slots must be ceil(V / 64)");
    return loss_forward(acts, ED_BF16, labels, act_lens, label_lens, B, T, U1, V, blank, nullptr, nullptr, 0.f,
                        workspace, row_offsets, stream_, lse_parts, lse_slots, frames, scores);
}

// ------------------------------------------------------------------------------- alignment-restricted loss (Ar-RNN-T)
// Mahadeokar et al. 2021: label u of utterance b may be emitted (the lattice step (t,u) -> (t,u+1)) on the frames
// win_lo[b][u] <= t <= win_hi[b][u] only; cost_b = -log of the probability summed over the alignments that respect every
// window.  win_lo / win_hi: int32 [B][U1-1] on the device, entries behind label_lens[b] ignored, values outside
// [0, T_b) match no frame.  The forward entry points are the plain ones with the windows behind label_lens; windows
// that admit no alignment give cost +inf (aligner: score -inf, frames all -1), decided on the device.  Null windows
// are refused before anything is launched.
#define ED_CHECK_WINDOWS(name) \
    ED_CHECK_ARG((win_lo && win_hi) || U1 == 1, name ": null windows (win_lo / win_hi); the plain entry point takes none")

extern "C" int edgedict_rnnt_loss_forward_ar(const void* acts, int acts_dtype, const int32_t* labels,
                                             const int32_t* act_lens, const int32_t* label_lens, const int32_t* win_lo,
                                             const int32_t* win_hi, int B, int T, int U1, int V, int blank, float* costs,
                                             float* reduced, float reduce_scale, void* workspace, void* stream_) {
    ED_CHECK_WINDOWS("rnnt_loss_forward_ar");
    return loss_forward(acts, acts_dtype, labels, act_lens, label_lens, B, T, U1, V, blank, costs, reduced,
                        reduce_scale, workspace, nullptr, stream_, nullptr, 0, nullptr, nullptr, win_lo, win_hi);
}

extern "C" int edgedict_rnnt_loss_forward_packed_ar(const void* acts, int acts_dtype, const int32_t* labels,
                                                    const int32_t* act_lens, const int32_t* label_lens,
                                                    const int32_t* win_lo, const int32_t* win_hi,
                                                    const long long* row_offsets, int B, int T, int U1, int V, int blank,
                                                    float* costs, float* reduced, float reduce_scale, void* workspace,
                                                    void* stream_) {
    ED_CHECK_WINDOWS("rnnt_loss_forward_packed_ar");
    ED_CHECK_ARG(row_offsets, "rnnt_loss_forward_packed_ar: null row_offsets");
    return loss_forward(acts, acts_dtype, labels, act_lens, label_lens, B, T, U1, V, blank, costs, reduced,
                        reduce_scale, workspace, row_offsets, stream_, nullptr, 0, nullptr, nullptr, win_lo, win_hi);
}

extern "C" int edgedict_rnnt_loss_forward_packed_parts_ar(const void* acts, const int32_t* labels,
                                                          const int32_t* act_lens, const int32_t* label_lens,
                                                          const int32_t* win_lo, const int32_t* win_hi,
                                                          const long long* row_offsets, int B, int T, int U1, int V,
                                                          int blank, float* costs, float* reduced, float reduce_scale,
                                                          void* workspace, const float* lse_parts, int lse_slots,
                                                          void* stream_) {
    ED_CHECK_WINDOWS("rnnt_loss_forward_packed_parts_ar");
    ED_CHECK_ARG(row_offsets && lse_parts, "rnnt_loss_forward_packed_parts_ar: null pointer");
    ED_CHECK_ARG(lse_slots == (V + 63) / 64, "rnnt_loss_forward_packed_parts_ar: lse_slots must be ceil(V / 64)");
    return loss_forward(acts, ED_BF16, labels, act_lens, label_lens, B, T, U1, V, blank, costs, reduced,
                        reduce_scale, workspace, row_offsets, stream_, lse_parts, lse_slots, nullptr, nullptr, win_lo,
                        win_hi);
}

// Backward of a workspace an *_ar forward entry point filled: the *_fe entry points' arguments (fastemit_lambda >= 0,
// 0 = none), the gradient kernels built with the dead-cell test.  The windows themselves are not needed: they are in
// the workspace (lp_label = -inf).  On a workspace of a plain forward call the result is the plain gradient.
extern "C" int edgedict_rnnt_loss_backward_ar(const void* acts, int acts_dtype, void* grads, const int32_t* labels,
                                              const int32_t* act_lens, const int32_t* label_lens, int B, int T, int U1,
                                              int V, int blank, const void* workspace, float grad_scale_host,
                                              const float* grad_scale_dev, int grad_scale_stride,
                                              float fastemit_lambda, void* stream_) {
    return loss_backward(acts, acts_dtype, grads, labels, act_lens, label_lens, B, T, U1, V, blank, workspace,
                         grad_scale_host, grad_scale_dev, grad_scale_stride, nullptr, stream_, 0, -1, nullptr,
                         fastemit_lambda, true);
}

extern "C" int edgedict_rnnt_loss_backward_packed_ar(const void* acts, int acts_dtype, void* grads,
                                                     const int32_t* labels, const int32_t* act_lens,
                                                     const int32_t* label_lens, const long long* row_offsets, int B,
                                                     int T, int U1, int V, int blank, const void* workspace,
                                                     float grad_scale_host, const float* grad_scale_dev,
                                                     int grad_scale_stride, float fastemit_lambda, void* stream_) {
    ED_CHECK_ARG(fastemit_lambda >= 0.f && fastemit_lambda <= FLT_MAX,
                 "rnnt_loss_backward_packed_ar: fastemit_lambda must be finite and >= 0 (got %g)", (double)fastemit_lambda);
    ED_CHECK_ARG(row_offsets, "rnnt_loss_backward_packed_ar: null row_offsets");
    return loss_backward(acts, acts_dtype, grads, labels, act_lens, label_lens, B, T, U1, V, blank, workspace,
                         grad_scale_host, grad_scale_dev, grad_scale_stride, row_offsets, stream_, 0, -1, nullptr,
                         fastemit_lambda, true);
}

extern "C" int edgedict_rnnt_loss_backward_packed_colsum_ar(const void* acts, int acts_dtype, void* grads,
                                                            const int32_t* labels, const int32_t* act_lens,
                                                            const int32_t* label_lens, const long long* row_offsets,
                                                            int B, int T, int U1, int V, int blank,
                                                            const void* workspace, float grad_scale_host,
                                                            const float* grad_scale_dev, int grad_scale_stride,
                                                            float* colsum_parts, float fastemit_lambda, void* stream_) {
    ED_CHECK_ARG(fastemit_lambda >= 0.f && fastemit_lambda <= FLT_MAX,
                 "rnnt_loss_backward_packed_colsum_ar: fastemit_lambda must be finite and >= 0 (got %g)", (double)fastemit_lambda);
    ED_CHECK_ARG(row_offsets && colsum_parts, "rnnt_loss_backward_packed_colsum_ar: null pointer");
    return loss_backward(acts, acts_dtype, grads, labels, act_lens, label_lens, B, T, U1, V, blank, workspace,
                         grad_scale_host, grad_scale_dev, grad_scale_stride, row_offsets, stream_, 0, -1, colsum_parts,
                         fastemit_lambda, true);
}

extern "C" int edgedict_rnnt_loss_backward_packed_range_ar(const void* acts, int acts_dtype, void* grads,
                                                           const int32_t* labels, const int32_t* act_lens,
                                                           const int32_t* label_lens, const long long* row_offsets,
                                                           int B, int T, int U1, int V, int blank,
                                                           const void* workspace, float grad_scale_host,
                                                           const float* grad_scale_dev, int grad_scale_stride, int b0,
                                                           int nb, float fastemit_lambda, void* stream_) {
    ED_CHECK_ARG(fastemit_lambda >= 0.f && fastemit_lambda <= FLT_MAX,
                 "rnnt_loss_backward_packed_range_ar: fastemit_lambda must be finite and >= 0 (got %g)", (double)fastemit_lambda);
    ED_CHECK_ARG(row_offsets, "rnnt_loss_backward_packed_range_ar: null row_offsets");
    return loss_backward(acts, acts_dtype, grads, labels, act_lens, label_lens, B, T, U1, V, blank, workspace,
                         grad_scale_host, grad_scale_dev, grad_scale_stride, row_offsets, stream_, b0, nb, nullptr,
                         fastemit_lambda, true);
}

extern "C" int edgedict_rnnt_align_ar(const void* acts, int acts_dtype, const int32_t* labels, const int32_t* act_lens,
                                      const int32_t* label_lens, const int32_t* win_lo, const int32_t* win_hi, int B,
                                      int T, int U1, int V, int blank, int32_t* frames, float* scores, void* workspace,
                                      void* stream_) {
    ED_CHECK_WINDOWS("rnnt_align_ar");
    ED_CHECK_ARG(scores, "rnnt_align_ar: null scores");
    return loss_forward(acts, acts_dtype, labels, act_lens, label_lens, B, T, U1, V, blank, nullptr, nullptr, 0.f,
                        workspace, nullptr, stream_, nullptr, 0, frames, scores, win_lo, win_hi);
}

extern "C" int edgedict_rnnt_align_packed_ar(const void* acts, int acts_dtype, const int32_t* labels,
                                             const int32_t* act_lens, const int32_t* label_lens, const int32_t* win_lo,
                                             const int32_t* win_hi, const long long* row_offsets, int B, int T, int U1,
                                             int V, int blank, int32_t* frames, float* scores, void* workspace,
                                             void* stream_) {
    ED_CHECK_WINDOWS("rnnt_align_packed_ar");
    ED_CHECK_ARG(row_offsets && scores, "rnnt_align_packed_ar: null pointer");
    return loss_forward(acts, acts_dtype, labels, act_lens, label_lens, B, T, U1, V, blank, nullptr, nullptr, 0.f,
                        workspace, row_offsets, stream_, nullptr, 0, frames, scores, win_lo, win_hi);
}

extern "C" int edgedict_rnnt_align_packed_parts_ar(const void* acts, const int32_t* labels, const int32_t* act_lens,
                                                   const int32_t* label_lens, const int32_t* win_lo,
                                                   const int32_t* win_hi, const long long* row_offsets, int B, int T,
                                                   int U1, int V, int blank, int32_t* frames, float* scores,
                                                   void* workspace, const float* lse_parts, int lse_slots,
                                                   void* stream_) {
    ED_CHECK_WINDOWS("rnnt_align_packed_parts_ar");
    ED_CHECK_ARG(row_offsets && lse_parts && scores, "rnnt_align_packed_parts_ar: null pointer");
    ED_CHECK_ARG(lse_slots == (V + 63) / 64, "rnnt_align_packed_parts_ar: lse_slots must be ceil(V / 64)");
    return loss_forward(acts, ED_BF16, labels, act_lens, label_lens, B, T, U1, V, blank, nullptr, nullptr, 0.f,
                        workspace, row_offsets, stream_, lse_parts, lse_slots, frames, scores, win_lo, win_hi);
}
#undef ED_CHECK_WINDOWS

// windows of `left` frames before and `right` frames after the frames of an alignment (frames [B][U] as the aligner
// writes them): lo = max(0, f - left), hi = min(T_b - 1, f + right); behind label_lens[b]: lo = 0, hi = T - 1.
// T = 0: the largest act_lens of the batch, found on the device.
extern "C" int edgedict_rnnt_alignment_windows(const int32_t* frames, const int32_t* act_lens, const int32_t* label_lens,
                                               int B, int T, int U, int left, int right, int32_t* win_lo,
                                               int32_t* win_hi, void* stream_) {
    ED_CHECK_ARG(B > 0 && T >= 0 && U >= 0, "rnnt_alignment_windows: B must be positive, T and U >= 0 (got %d,%d,%d)", B, T, U);
    ED_CHECK_ARG(left >= 0 && right >= 0, "rnnt_alignment_windows: left and right must be >= 0 (got %d, %d)", left, right);
    if (U == 0) return ED_OK;
    ED_CHECK_ARG(frames && act_lens && label_lens && win_lo && win_hi, "rnnt_alignment_windows: null pointer argument");
    const long long n = (long long)B * U;
    hipLaunchKernelGGL(rnnt_windows_from_frames, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream_,
                       frames, act_lens, label_lens, B, T, U, left, right, win_lo, win_hi);
    ED_CHECK_LAUNCH("rnnt_windows_from_frames");
    return ED_OK;
}

// the live cells of the restricted lattice from the windows alone: band [B][T][2] int32 = (first, last) live label
// column of every frame, (0, -1) where the frame has none; cells [B] int64 = live cells of the utterance (0 where the
// windows admit no alignment).  Equals isfinite(alpha) & isfinite(beta) of the *_ar forward call's workspace.
extern "C" int edgedict_rnnt_band(const int32_t* win_lo, const int32_t* win_hi, const int32_t* act_lens,
                                  const int32_t* label_lens, int B, int T, int U1, int32_t* band, long long* cells,
                                  void* stream_) {
    ED_CHECK_ARG(B > 0 && T > 0 && U1 > 0, "rnnt_band: B, T, U1 must be positive (got %d,%d,%d)", B, T, U1);
    ED_CHECK_ARG(U1 <= BAND_MAX_U1, "rnnt_band: U+1 = %d exceeds the supported maximum of %d", U1, BAND_MAX_U1);
    ED_CHECK_ARG(((win_lo && win_hi) || U1 == 1) && act_lens && label_lens && band && cells, "rnnt_band: null pointer argument");
    hipLaunchKernelGGL(rnnt_band_table, dim3(B), dim3(256), 0, (hipStream_t)stream_, win_lo, win_hi, act_lens, label_lens,
                       T, U1, band, cells);
    ED_CHECK_LAUNCH("rnnt_band_table");
    return ED_OK;
}

// ------------------------------------------------------------------------------------------- band-packed joint + loss
// The plan's device work: row_off [B][T] int64 = exclusive prefix sum of the widths max(0, uhi - ulo + 1) of the band
// table in (b, t) order, total [1] int64 = M_band (= the sum of cells) ...
extern "C" int edgedict_rnnt_band_offsets(const int32_t* band, const long long* cells, int B, int T, long long* row_off,
                                          long long* total, void* stream_) {
    ED_CHECK_ARG(B > 0 && T > 0, "rnnt_band_offsets: B, T must be positive (got %d,%d)", B, T);
    ED_CHECK_ARG(band && cells && row_off && total, "rnnt_band_offsets: null pointer argument");
    hipLaunchKernelGGL(rnnt_band_scan, dim3(B), dim3(256), 0, (hipStream_t)stream_, band, cells, B, T, row_off, total);
    ED_CHECK_LAUNCH("rnnt_band_scan");
    return ED_OK;
}

// ... and, once the host knows M_band: row_tu [rows] int32 = t << 16 | u of every band row (T, U1 < 65536).
extern "C" int edgedict_rnnt_band_rows(const int32_t* band, const long long* row_off, int B, int T, int U1, long long rows,
                                       int32_t* row_tu, void* stream_) {
    ED_CHECK_ARG(B > 0 && T > 0 && U1 > 0 && rows >= 0, "rnnt_band_rows: bad shape (got %d,%d,%d, %lld rows)", B, T, U1, rows);
    ED_CHECK_ARG(T < 65536 && U1 < 65536, "rnnt_band_rows: T and U+1 must be below 65536 (got %d, %d)", T, U1);
    if (rows == 0) return ED_OK;
    ED_CHECK_ARG(band && row_off && row_tu, "rnnt_band_rows: null pointer argument");
    const long long n = (long long)B * T;
    hipLaunchKernelGGL(rnnt_band_fill, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream_, band, row_off,
                       B, T, rows, row_tu);
    ED_CHECK_LAUNCH("rnnt_band_fill");
    return ED_OK;
}

#define ED_CHECK_BAND(name)                                                                                   \
    ED_CHECK_ARG(row_off && row_tu && cells, name ": null band rows (row_off / row_tu / cells)");              \
    ED_CHECK_ARG(T < 65536 && U1 < 65536, name ": T and U+1 must be below 65536 (got %d, %d)", T, U1)

// The *_packed_ar forward entry points with the logits (and the log-sum-exp partials) on BAND rows: every cell of the
// boxes gets its workspace planes - a live cell from its band row exactly as the *_ar kernels form them, a dead cell
// lp_blank = lp_label = -inf and denominator 0 - and the lattice walks and the costs run unchanged behind that.
extern "C" int edgedict_rnnt_loss_forward_band(const void* acts, int acts_dtype, const int32_t* labels,
                                               const int32_t* act_lens, const int32_t* label_lens, const int32_t* win_lo,
                                               const int32_t* win_hi, const int32_t* band, const long long* row_off,
                                               const int32_t* row_tu, const long long* cells, int B, int T, int U1, int V,
                                               int blank, float* costs, float* reduced, float reduce_scale,
                                               void* workspace, void* stream_) {
    ED_CHECK_ARG((win_lo && win_hi) || U1 == 1, "rnnt_loss_forward_band: null windows (win_lo / win_hi)");
    ED_CHECK_ARG(band, "rnnt_loss_forward_band: null band table");
    ED_CHECK_BAND("rnnt_loss_forward_band");
    const BandArgs bd{band, row_off, row_tu, cells};
    return loss_forward(acts, acts_dtype, labels, act_lens, label_lens, B, T, U1, V, blank, costs, reduced,
                        reduce_scale, workspace, nullptr, stream_, nullptr, 0, nullptr, nullptr, win_lo, win_hi, &bd);
}

extern "C" int edgedict_rnnt_loss_forward_band_parts(const void* acts, const int32_t* labels, const int32_t* act_lens,
                                                     const int32_t* label_lens, const int32_t* win_lo,
                                                     const int32_t* win_hi, const int32_t* band, const long long* row_off,
                                                     const int32_t* row_tu, const long long* cells, int B, int T, int U1,
                                                     int V, int blank, float* costs, float* reduced, float reduce_scale,
                                                     void* workspace, const float* lse_parts, int lse_slots,
                                                     void* stream_) {
    ED_CHECK_ARG((win_lo && win_hi) || U1 == 1, "rnnt_loss_forward_band_parts: null windows (win_lo / win_hi)");
    ED_CHECK_BAND("rnnt_loss_forward_band_parts");
    ED_CHECK_ARG(band && lse_parts, "rnnt_loss_forward_band_parts: null pointer");
    ED_CHECK_ARG(lse_slots == (V + 63) / 64, "rnnt_loss_forward_band_parts: lse_slots must be ceil(V / 64)");
    const BandArgs bd{band, row_off, row_tu, cells};
    return loss_forward(acts, ED_BF16, labels, act_lens, label_lens, B, T, U1, V, blank, costs, reduced, reduce_scale,
                        workspace, nullptr, stream_, lse_parts, lse_slots, nullptr, nullptr, win_lo, win_hi, &bd);
}

// Backward of a workspace a *_band forward call filled: logits and gradient on band rows, every row a live cell (no
// zero rows are written: there are none).  fastemit_lambda as the *_ar entry points'.  The colsum form writes
// edgedict_rnnt_grad_colsum_rows(...) partial rows, all of them (zeros where a workgroup had no rows).
extern "C" int edgedict_rnnt_loss_backward_band(const void* acts, int acts_dtype, void* grads, const int32_t* labels,
                                                const int32_t* act_lens, const int32_t* label_lens,
                                                const long long* row_off, const int32_t* row_tu, const long long* cells,
                                                int B, int T, int U1, int V, int blank, const void* workspace,
                                                float grad_scale_host, const float* grad_scale_dev,
                                                int grad_scale_stride, float fastemit_lambda, void* stream_) {
    ED_CHECK_ARG(fastemit_lambda >= 0.f && fastemit_lambda <= FLT_MAX,
                 "rnnt_loss_backward_band: fastemit_lambda must be finite and >= 0 (got %g)", (double)fastemit_lambda);
    ED_CHECK_BAND("rnnt_loss_backward_band");
    const BandArgs bd{nullptr, row_off, row_tu, cells};
    return loss_backward(acts, acts_dtype, grads, labels, act_lens, label_lens, B, T, U1, V, blank, workspace,
                         grad_scale_host, grad_scale_dev, grad_scale_stride, nullptr, stream_, 0, -1, nullptr,
                         fastemit_lambda, true, &bd);
}

extern "C" int edgedict_rnnt_loss_backward_band_colsum(const void* acts, int acts_dtype, void* grads,
                                                       const int32_t* labels, const int32_t* act_lens,
                                                       const int32_t* label_lens, const long long* row_off,
                                                       const int32_t* row_tu, const long long* cells, int B, int T,
                                                       int U1, int V, int blank, const void* workspace,
                                                       float grad_scale_host, const float* grad_scale_dev,
                                                       int grad_scale_stride, float* colsum_parts,
                                                       float fastemit_lambda, void* stream_) {
    ED_CHECK_ARG(fastemit_lambda >= 0.f && fastemit_lambda <= FLT_MAX,
                 "rnnt_loss_backward_band_colsum: fastemit_lambda must be finite and >= 0 (got %g)", (double)fastemit_lambda);
    ED_CHECK_BAND("rnnt_loss_backward_band_colsum");
    ED_CHECK_ARG(colsum_parts, "rnnt_loss_backward_band_colsum: null pointer");
    const BandArgs bd{nullptr, row_off, row_tu, cells};
    return loss_backward(acts, acts_dtype, grads, labels, act_lens, label_lens, B, T, U1, V, blank, workspace,
                         grad_scale_host, grad_scale_dev, grad_scale_stride, nullptr, stream_, 0, -1, colsum_parts,
                         fastemit_lambda, true, &bd);
}
#undef ED_CHECK_BAND
