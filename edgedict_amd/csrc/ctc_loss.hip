// CTC loss, its gradient and the CTC greedy decoder for gfx950 (Graves et al. 2006).
//
// The auxiliary head of the transducer's encoder: raw head logits z [B, T, V], a transcript y_0 .. y_{U_b-1} per
// utterance, and the extended sequence of S_b = 2 U_b + 1 states  blank, y_0, blank, y_1, ..., blank  (state s is a
// label iff s is odd, label (s - 1) / 2).  With lp(t,s) = log_softmax(z_t)[symbol of state s]:
//   alpha(0,0) = lp(0,0), alpha(0,1) = lp(0,1), alpha(0,s>1) = -inf
//   alpha(t,s) = lp(t,s) + lse(alpha(t-1,s), alpha(t-1,s-1), [skip(s)] alpha(t-1,s-2))
//   skip(s)    = s is a label, s >= 3 and it differs from the label two states back
//   ll         = lse(alpha(T_b-1,S_b-1), alpha(T_b-1,S_b-2))          (U_b = 0: the first term only)
// BETA CONVENTION: beta(t,s) is the log-probability of finishing the transcript from state s AFTER frame t's symbol has
// been emitted - it does NOT contain lp(t,s):
//   beta(T_b-1,s) = 0 for s in {S_b-1, S_b-2}, -inf otherwise
//   beta(t,s)     = lse over s' in {s, s+1, [skip(s+2)] s+2} of beta(t+1,s') + lp(t+1,s')
// so the occupancy of a state is exp(alpha + beta - ll) with nothing to subtract, and
//   d cost / d z(t,v) = softmax(z_t)[v] - sum over states s carrying v of exp(alpha(t,s) + beta(t,s) - ll).
//
// Kernels (none of them GEMM-shaped, no MFMA here on purpose - as rnnt_loss.hip):
//   ctc_lse_gather  : one wave64 per row (b, t < T_b): log-sum-exp of V logits with 16-byte loads, then the blank's and
//                     the U_b labels' log-probabilities.                                              HBM-bound.
//   ctc_label_chain : per utterance, for every label position the next position with the same label and whether it is
//                     the first one - what lets ctc_grad sum a repeated label's occupancies in a FIXED order.
//   ctc_alpha_beta  : ONE WAVE per (utterance, direction), a lane owns C consecutive states, all lanes walk the frames
//                     in lock step; the two values a lane needs from its left neighbour arrive by DPP moves (no LDS,
//                     no barrier).  fp64 carry, log_add64 of common.hpp.                              latency-bound.
//                     <C, VIT = true>: the forced aligner's Viterbi walk, one wave per utterance, max for the log-add.
//   ctc_viterbi_backtrace : one wave per utterance, one lane walks the best path back: each label's first / last frame.
//   ctc_costs       : costs, the zero_infinity rule, the dead-utterance flags, the reduction.
//   ctc_grad        : one wave64 per row again; reads the logits once, writes the gradient once.      HBM-bound.
//   ctc_argmax / ctc_collapse : the greedy decoder (arg max per frame, then drop repeats and blanks).
#include "common.hpp"
#include "ctc_rows.hpp"

namespace {

struct CtcWs {
    size_t off_lse, off_lpb, off_lpl, off_alpha, off_beta, off_ll, off_flag, off_chain, total;
};

inline size_t up256(size_t n) { return ((n + 255) / 256) * 256; }

inline CtcWs ctc_ws(int B, int T, int U) {
    CtcWs w;
    const size_t rows = (size_t)B * T, S = 2 * (size_t)U + 1;
    size_t o = 0;
    w.off_lse = o;   o += up256(rows * sizeof(float));
    w.off_lpb = o;   o += up256(rows * sizeof(float));
    w.off_lpl = o;   o += up256(rows * U * sizeof(float));
    // alpha / beta / log-likelihoods are float64 for the reason rnnt_loss.hip gives: the gradient needs
    // exp(alpha + beta - ll), the difference of three numbers of size |ll|
    w.off_alpha = o; o += up256(rows * S * sizeof(double));
    w.off_beta = o;  o += up256(rows * S * sizeof(double));
    w.off_ll = o;    o += up256((size_t)2 * B * sizeof(double));
    w.off_flag = o;  o += up256((size_t)B * sizeof(int32_t));
    w.off_chain = o; o += up256((size_t)2 * B * U * sizeof(int32_t));   // [B][2][U]: next, first
    w.total = o;
    return w;
}

// ------------------------------------------------------------------ rows: row_lse (log-sum-exp, + arg max) is in
// ctc_rows.hpp, shared with ctc_decode.hip

// grid (x, B): the workgroups of column b walk the frames t < T_b of utterance b (rows behind T_b are never read),
// 4 waves per block, one row per wave per iteration.  A label outside [0, V) (the Python shim never passes one, a raw
// C-ABI caller may) reads nothing and gets log-probability -inf.
template <typename T>
__global__ __launch_bounds__(256) void ctc_lse_gather(const T* __restrict__ logits, const int32_t* __restrict__ labels,
                                                      const int32_t* __restrict__ act_lens,
                                                      const int32_t* __restrict__ label_lens, int Tm, int U, int V,
                                                      int blank, float* __restrict__ lse, float* __restrict__ lpb,
                                                      float* __restrict__ lpl, int vec_ok) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.y;
    const int Tb = max(0, min(act_lens[b], Tm)), Ub = max(0, min(label_lens[b], U));
    for (int t = blockIdx.x * 4 + wave; t < Tb; t += gridDim.x * 4) {
        const long long row = (long long)b * Tm + t;
        const T* z = logits + row * (long long)V;
        const float l = row_lse<T, false>(z, V, vec_ok, lane, nullptr, nullptr);
        if (lane == 0) {
            lse[row] = l;
            lpb[row] = ElemIO<T>::load(z + blank) - l;
        }
        for (int u = lane; u < Ub; u += 64) {
            const int y = labels[(long long)b * U + u];
            lpl[row * U + u] = (y >= 0 && y < V) ? ElemIO<T>::load(z + y) - l : -INFINITY;
        }
    }
}

// chain[b][0][u] = the next position u' > u with y_u' == y_u (-1: none), chain[b][1][u] = 1 iff no position before u
// carries y_u.  One workgroup per utterance, one thread per position; depends on the labels only.
__global__ __launch_bounds__(256) void ctc_label_chain(const int32_t* __restrict__ labels,
                                                       const int32_t* __restrict__ label_lens, int U,
                                                       int32_t* __restrict__ chain) {
    const int b = blockIdx.x;
    const int Ub = max(0, min(label_lens[b], U));
    const int32_t* y = labels + (long long)b * U;
    int32_t* nxt = chain + (long long)b * 2 * U;
    int32_t* first = nxt + U;
    for (int u = threadIdx.x; u < Ub; u += blockDim.x) {
        const int me = y[u];
        int n = -1, f = 1;
        for (int k = u + 1; k < Ub; ++k)
            if (y[k] == me) { n = k; break; }
        for (int k = u - 1; k >= 0; --k)
            if (y[k] == me) { f = 0; break; }
        nxt[u] = n;
        first[u] = f;
    }
}

// ------------------------------------------------------------------ the lattice walks
// ONE WAVE per (utterance, direction): blockIdx.x = 2 b + dir, 64 threads.  Both directions run the SAME recursion: the
// beta walk is the alpha walk of the reversed transcript over the reversed frames (S_b is odd, so reversing the states
// keeps blanks on even and labels on odd positions, and the skip rule is symmetric).  In walk coordinates lane l owns
// the C consecutive states m in [C l, C l + C) (beta: m counts from the right end, s = S_b - 1 - m), row r is frame r
// (beta: T_b - 1 - r).  A row depends on the row before it only, so all lanes are in the same row: per row a lane needs
// its own C values of the previous row and lane l - 1's last two, handed up with wave_shr:1 DPP moves (two doubles =
// four moves) as rnnt_alpha_beta hands its one.  The slots are updated from the highest down, so the lower ones still
// hold the previous row.  What is carried is  p(r,m) + lp(r,m)  with  p = lse(three predecessors)  (row 0: p = 0 for
// m <= 1); the alpha plane receives the carry, the beta plane p itself - the beta convention at the top of the file.
// T_b rows of C two- or three-way log-adds (log_add64 chained: fp64 add / max, fp32 correction term); the row's
// log-probabilities (the blank's, and the lane's C / 2 labels') are requested D rows ahead.
// No sum below has +inf as an operand, so no -inf - (-inf) is ever formed; an utterance with T_b < U_b + repeats never
// reaches its last two states and gets ll = -inf from the recursion itself.
// VIT = true is the Viterbi walk of the forced aligner (edgedict_ctc_align): ONE wave per utterance (blockIdx.x = b,
// direction 0 only), ONE fmax per predecessor in place of the log-add, then the same add:
//   v(t,s) = max(v(t-1,s), v(t-1,s-1), [skip(s)] v(t-1,s-2)) + (double)lp(t,s)       (row 0: 0.0 + lp for s <= 1)
// written where the alphas go, and the best path's score max(v(T_b-1,S_b-1), v(T_b-1,S_b-2)) into ll[2 b]; the beta
// plane and ll[2 b + 1] are not written.  The VIT = false instantiation is the kernel as it was.
template <int C, bool VIT = false>
__global__ __launch_bounds__(64) void ctc_alpha_beta(const float* __restrict__ lpb, const float* __restrict__ lpl,
                                                     const int32_t* __restrict__ labels,
                                                     const int32_t* __restrict__ act_lens,
                                                     const int32_t* __restrict__ label_lens, int Tm, int U,
                                                     double* __restrict__ alphas, double* __restrict__ betas,
                                                     double* __restrict__ ll) {
    static_assert(C >= 2 && (C & 1) == 0, "a lane owns an even number of states");
    constexpr int H = C / 2;                         // label states per lane (the odd slots)
    constexpr int D = C <= 2 ? 8 : (C <= 4 ? 4 : (C <= 8 ? 2 : 1));
    const int b = VIT ? blockIdx.x : blockIdx.x >> 1;
    const int dir = VIT ? 0 : blockIdx.x & 1;
    const int lane = threadIdx.x;
    // clamped as rnnt_alpha_beta clamps them; an empty utterance has likelihood 0
    const int Tb = max(0, min(act_lens[b], Tm)), Ub = max(0, min(label_lens[b], U));
    if (Tb == 0) {
        if (lane == 0) ll[2 * b + dir] = -(double)INFINITY;
        return;
    }
    const int S = 2 * Ub + 1, Sm = 2 * U + 1;
    const double NEG = -(double)INFINITY;
    const long long row0 = (long long)b * Tm;
    const int32_t* y = labels + (long long)b * U;
    // walk position k of the transcript -> label index
    auto pos = [&](int k) { return dir == 0 ? k : Ub - 1 - k; };
    auto frame = [&](int r) { return dir == 0 ? r : Tb - 1 - r; };
    unsigned skip = 0;                               // bit c: state C lane + c may be entered from two states back
#pragma unroll
    for (int h = 0; h < H; ++h) {
        const int k = H * lane + h;                  // state m = 2 k + 1
        if (k >= 1 && k < Ub && y[pos(k)] != y[pos(k - 1)]) skip |= 1u << (2 * h + 1);
    }
    double prev[C];
#pragma unroll
    for (int c = 0; c < C; ++c) prev[c] = NEG;
    float qb[D], ql[D][H];                           // ring by row
    auto request = [&](int j, int r) {               // (static j)
        float vb = 0.f;
        if (r < Tb) vb = lpb[row0 + frame(r)];
        qb[j] = vb;
#pragma unroll
        for (int h = 0; h < H; ++h) {
            const int k = H * lane + h;
            float vl = 0.f;
            if (r < Tb && k < Ub) vl = lpl[(row0 + frame(r)) * U + pos(k)];
            ql[j][h] = vl;
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
            for (int h = 0; h < H; ++h) cl[h] = ql[j][h];
            request(j, r + D);
            const long long base = (row0 + frame(r)) * Sm;
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
                    p = VIT ? fmax(prev[c], a1) : log_add64(prev[c], a1);
                    if ((c & 1) && ((skip >> c) & 1)) p = VIT ? fmax(p, a2) : log_add64(p, a2);
                }
                const double carry = p + (double)((c & 1) ? cl[c >> 1] : cb);
                if (dir == 0) alphas[base + m] = carry;
                else betas[base + (S - 1 - m)] = p;
                prev[c] = carry;
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
    if (lane == 0) ll[2 * b + dir] = S >= 2 ? (VIT ? fmax(v1, v2) : log_add64(v1, v2)) : v1;
}

// Back-trace of the Viterbi walk (ctc_alpha_beta<C, true>): one wave per utterance.  Lane 0 starts in the better of the
// last two states of frame T_b - 1 and walks down to frame 0: T_b - 1 dependent steps of up to three loads of
// v(t-1, .) (and the two labels the skip rule compares).  All three predecessors of (t,s) get the same lp(t,s) added, so
// the one the maximum came from is found by comparing v(t-1, .) directly - no back-pointers are stored and no sum is
// re-formed.  TIE RULE (the later emission wins, as rnnt_viterbi_backtrace waits): the walk starts in state S_b - 2
// when v(T_b-1,S_b-2) >= v(T_b-1,S_b-1), and among the predecessors whose v(t-1, .) equals the maximum it takes s - 2
// (where the skip is allowed), else s - 1, else s.  On a row with a path every cell of the walk has a finite v, so the
// maximum is finite and the walk ends in state 0 or 1 having passed every label.  frames[b][u] / ends[b][u] = the first
// / last frame the path spends in label u's state; the other lanes write the -1 padding behind U_b.  A row without a
// path (T_b = 0, or fewer frames than labels plus adjacent repeats: score -inf): -1 everywhere.
__global__ __launch_bounds__(64) void ctc_viterbi_backtrace(const double* __restrict__ v, const double* __restrict__ ll,
                                                            const int32_t* __restrict__ labels,
                                                            const int32_t* __restrict__ act_lens,
                                                            const int32_t* __restrict__ label_lens, int Tm, int U,
                                                            int32_t* __restrict__ frames, int32_t* __restrict__ ends,
                                                            float* __restrict__ scores) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int Tb = max(0, min(act_lens[b], Tm)), Ub = max(0, min(label_lens[b], U));   // as ctc_alpha_beta
    const double NEG = -(double)INFINITY;
    const double L = ll[2 * b];                      // -inf for an empty utterance
    const bool none = Tb == 0 || L == NEG;
    int32_t* fr = frames + (long long)b * U;
    int32_t* en = ends + (long long)b * U;
    for (int u = (none ? 0 : Ub) + lane; u < U; u += 64) {
        fr[u] = -1;
        en[u] = -1;
    }
    if (lane != 0) return;
    scores[b] = (float)L;
    if (none) return;
    const int S = 2 * Ub + 1, Sm = 2 * U + 1;
    const long long row0 = (long long)b * Tm;
    const int32_t* y = labels + (long long)b * U;
    int t = Tb - 1, s = S - 1;
    if (S >= 2) {
        const double* last = v + (row0 + t) * Sm;
        if (last[S - 2] >= last[S - 1]) s = S - 2;
    }
    if (s & 1) en[s >> 1] = t;
    for (; t > 0; --t) {
        const double* pr = v + (row0 + t - 1) * Sm;
        const double a0 = pr[s];
        const double a1 = s >= 1 ? pr[s - 1] : NEG;
        double a2 = NEG;
        bool skip = false;
        if ((s & 1) && s >= 3) {
            a2 = pr[s - 2];
            skip = y[s >> 1] != y[(s >> 1) - 1];
        }
        if (!skip) a2 = NEG;
        const double m = fmax(fmax(a0, a1), a2);
        // (the index tests keep a row of NaN logits, where m may be -inf, inside the plane)
        const int from = (skip && a2 == m) ? s - 2 : ((s >= 1 && a1 == m) ? s - 1 : s);
        if (from != s) {
            if (s & 1) fr[s >> 1] = t;
            if (from & 1) en[from >> 1] = t - 1;
            s = from;
        }
    }
    if (s & 1) fr[s >> 1] = 0;
}

// single block: costs[b] = -ll_alpha[b]; zero_infinity turns a non-finite cost into 0; dead[b] = 1 marks the
// utterances whose gradient is zeros (ll = -inf, or a cost zero_infinity replaced);
// optionally reduced[0] = reduce_scale * sum_b costs[b]
__global__ __launch_bounds__(256) void ctc_costs(const double* __restrict__ ll, float* __restrict__ costs, int B,
                                                 int zero_infinity, int32_t* __restrict__ dead,
                                                 float* __restrict__ reduced, float reduce_scale) {
    __shared__ float part[4];
    float acc = 0.f;
    for (int b = threadIdx.x; b < B; b += blockDim.x) {
        const double L = ll[2 * b];
        float c = (float)(-L);
        int d = L == -(double)INFINITY;
        if (zero_infinity && !isfinite(c)) { c = 0.f; d = 1; }
        costs[b] = c;
        dead[b] = d;
        acc += c;
    }
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0 && reduced) reduced[0] = reduce_scale * (part[0] + part[1] + part[2] + part[3]);
}

// ------------------------------------------------------------------ gradient
// grid (x, B), one wave per row of the [Tm, V] slab of utterance b.  Rows t >= T_b and dead utterances: zeros.
// A live row is written in two steps.  (1) every column gets scale * softmax - the logits read once, 16-byte accesses.
// (2) the few columns that carry a state of the lattice are written AGAIN as scale * (softmax - occupancy): the blank's
// U_b + 1 occupancies are summed lane-strided and reduced over the wave (a fixed butterfly), a label's by ONE lane that
// starts at the label's first position and follows ctc_label_chain's links - a fixed order, so the gradient is
// bit-identical from run to run (no atomics anywhere).  Between the steps the wave waits for its own stores
// (s_waitcnt vmcnt(0): on gfx9 a store leaves the counter when it has been written), so step 2 lands on top.
// Distinct labels are distinct columns; a label equal to the blank is not a transcript symbol and is left out.
template <typename T>
__global__ __launch_bounds__(256) void ctc_grad(const T* __restrict__ logits, T* __restrict__ grads,
                                                const int32_t* __restrict__ labels,
                                                const int32_t* __restrict__ act_lens,
                                                const int32_t* __restrict__ label_lens, int Tm, int U, int V, int blank,
                                                const float* __restrict__ lse, const double* __restrict__ alphas,
                                                const double* __restrict__ betas, const double* __restrict__ ll,
                                                const int32_t* __restrict__ dead, const int32_t* __restrict__ chain,
                                                float scale_host, const float* __restrict__ scale_dev,
                                                int scale_stride, int vec_ok) {
    constexpr int VEC = ElemIO<T>::VEC;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.y;
    const int Tb = max(0, min(act_lens[b], Tm)), Ub = max(0, min(label_lens[b], U));
    const int Sm = 2 * U + 1;
    const bool is_dead = dead[b] != 0;
    const double L = ll[2 * b];
    const float scale = scale_host * (scale_dev ? scale_dev[(long long)b * scale_stride] : 1.f);
    const int32_t* y = labels + (long long)b * U;
    const int32_t* nxt = chain + (long long)b * 2 * U;
    const int32_t* first = nxt + U;
    for (int t = blockIdx.x * 4 + wave; t < Tm; t += gridDim.x * 4) {
        const long long row = (long long)b * Tm + t;
        const T* z = logits + row * (long long)V;
        T* g = grads + row * (long long)V;
        const bool live = t < Tb && !is_dead;
        const float l = live ? lse[row] : 0.f;
        if (vec_ok) {
            for (int v = lane * VEC; v < V; v += 64 * VEC) {
                float o[VEC];
                if (live) {
                    float x[VEC];
                    ElemIO<T>::load_vec(z + v, x);
#pragma unroll
                    for (int i = 0; i < VEC; ++i) o[i] = scale * __expf(x[i] - l);
                } else {
#pragma unroll
                    for (int i = 0; i < VEC; ++i) o[i] = 0.f;
                }
                ElemIO<T>::store_vec(g + v, o);
            }
        } else {
            for (int v = lane; v < V; v += 64)
                ElemIO<T>::store(g + v, live ? scale * __expf(ElemIO<T>::load(z + v) - l) : 0.f);
        }
        if (!live) continue;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const double* a = alphas + row * Sm;
        const double* bt = betas + row * Sm;
        float acc = 0.f;
        for (int k = lane; k <= Ub; k += 64) acc += __expf((float)(a[2 * k] + bt[2 * k] - L));
        const float occ_blank = wave_sum(acc);
        if (lane == 0) ElemIO<T>::store(g + blank, scale * (__expf(ElemIO<T>::load(z + blank) - l) - occ_blank));
        for (int u = lane; u < Ub; u += 64) {
            if (!first[u]) continue;
            const int v = y[u];
            if (v < 0 || v >= V || v == blank) continue;
            float occ = 0.f;
            for (int k = u; k >= 0; k = nxt[k]) occ += __expf((float)(a[2 * k + 1] + bt[2 * k + 1] - L));
            ElemIO<T>::store(g + v, scale * (__expf(ElemIO<T>::load(z + v) - l) - occ));
        }
    }
}

// ------------------------------------------------------------------ greedy decoder
// row pass: k[b,t] = arg max_v z (lowest index on ties), lp[b,t] = z[k] - lse, for t < T_b
template <typename T>
__global__ __launch_bounds__(256) void ctc_argmax(const T* __restrict__ logits, const int32_t* __restrict__ act_lens,
                                                  int Tm, int V, int32_t* __restrict__ kbuf, float* __restrict__ lpbuf,
                                                  int vec_ok) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.y;
    const int Tb = max(0, min(act_lens[b], Tm));
    for (int t = blockIdx.x * 4 + wave; t < Tb; t += gridDim.x * 4) {
        const long long row = (long long)b * Tm + t;
        float bv;
        int bi;
        const float l = row_lse<T, true>(logits + row * (long long)V, V, vec_ok, lane, &bv, &bi);
        if (lane == 0) {
            kbuf[row] = bi;
            lpbuf[row] = bv - l;
        }
    }
}

// one wave per utterance: frame t is kept iff k_t != blank and (t == 0 or k_t != k_{t-1}); kept frames are compacted in
// order with a ballot and a prefix count, 64 frames per pass.  neglogp = -sum of lp over the kept frames (per-lane
// partial sums in frame order, one wave reduction at the end).  Behind the count tokens and frames are -1.
__global__ __launch_bounds__(64) void ctc_collapse(const int32_t* __restrict__ kbuf, const float* __restrict__ lpbuf,
                                                   const int32_t* __restrict__ act_lens, int Tm, int blank,
                                                   int32_t* __restrict__ tokens, int32_t* __restrict__ counts,
                                                   int32_t* __restrict__ frames, float* __restrict__ neglogp) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int Tb = max(0, min(act_lens[b], Tm));
    const long long row0 = (long long)b * Tm;
    int count = 0;
    float acc = 0.f;
    for (int t0 = 0; t0 < Tb; t0 += 64) {
        const int t = t0 + lane;
        int k = blank, kp = -1;
        if (t < Tb) {
            k = kbuf[row0 + t];
            if (t > 0) kp = kbuf[row0 + t - 1];
        }
        const bool keep = t < Tb && k != blank && (t == 0 || k != kp);
        const unsigned long long mask = __ballot(keep);
        if (keep) {
            const int at = count + __popcll(mask & ((1ull << lane) - 1ull));
            tokens[row0 + at] = k;
            frames[row0 + at] = t;
            acc += lpbuf[row0 + t];
        }
        count += __popcll(mask);
    }
    for (int t = count + lane; t < Tm; t += 64) {
        tokens[row0 + t] = -1;
        frames[row0 + t] = -1;
    }
    acc = wave_sum(acc);
    if (lane == 0) {
        counts[b] = count;
        neglogp[b] = -acc;
    }
}

inline int ctc_check(const char* who, int B, int T, int U, int V, int blank, int dtype) {
    ED_CHECK_ARG(B > 0 && T > 0 && U >= 0, "%s: B, T must be positive and U >= 0 (got %d, %d, %d)", who, B, T, U);
    ED_CHECK_ARG(U <= 1023, "%s: U = %d exceeds the supported maximum of 1023 labels per utterance", who, U);
    ED_CHECK_ARG(V >= 2, "%s: V = %d, need at least the blank and one symbol", who, V);
    ED_CHECK_ARG(blank >= 0 && blank < V, "%s: blank %d outside [0,%d)", who, blank, V);
    ED_CHECK_ARG(dtype == ED_F32 || dtype == ED_BF16, "%s: unsupported dtype code %d", who, dtype);
    return ED_OK;
}

// the first two stages of the loss and of the aligner: the row pass, then the lattice walk - one wave per
// (utterance, direction) (VIT: per utterance), C = max(2, ceil(S / 64)) states per lane (rounded up to a power of two)
inline void ctc_launch_rows(const void* logits, int dtype, const int32_t* labels, const int32_t* act_lens,
                            const int32_t* label_lens, int B, int T, int U, int V, int blank, float* lse, float* lpb,
                            float* lpl, hipStream_t stream) {
    const size_t esz = dtype == ED_F32 ? 4 : 2;
    const int vec_ok = ((V * esz) % 16 == 0) && (((uintptr_t)logits & 15) == 0);
    const dim3 grid1(ed_grid_for(T, 4, max(1, 256 * 16 / B)), B);
    if (dtype == ED_F32)
        hipLaunchKernelGGL(ctc_lse_gather<float>, grid1, dim3(256), 0, stream, (const float*)logits, labels, act_lens,
                           label_lens, T, U, V, blank, lse, lpb, lpl, vec_ok);
    else
        hipLaunchKernelGGL(ctc_lse_gather<bf16_t>, grid1, dim3(256), 0, stream, (const bf16_t*)logits, labels, act_lens,
                           label_lens, T, U, V, blank, lse, lpb, lpl, vec_ok);
}

template <bool VIT>
inline void ctc_launch_walk(const float* lpb, const float* lpl, const int32_t* labels, const int32_t* act_lens,
                            const int32_t* label_lens, int B, int T, int U, double* alphas, double* betas, double* ll,
                            hipStream_t stream) {
#define ED_CTC_AB(CC)                                                                                                 \
    hipLaunchKernelGGL((ctc_alpha_beta<CC, VIT>), dim3(VIT ? B : 2 * B), dim3(64), 0, stream, lpb, lpl, labels, act_lens, \
                       label_lens, T, U, alphas, betas, ll)
    const int per_lane = (2 * U + 1 + 63) / 64;
    if (per_lane <= 2) ED_CTC_AB(2);
    else if (per_lane <= 4) ED_CTC_AB(4);
    else if (per_lane <= 8) ED_CTC_AB(8);
    else if (per_lane <= 16) ED_CTC_AB(16);
    else ED_CTC_AB(32);
#undef ED_CTC_AB
}

}  // namespace

extern "C" size_t edgedict_ctc_workspace_bytes(int B, int T, int U) {
    if (B <= 0 || T <= 0 || U < 0) return 0;
    return ctc_ws(B, T, U).total;
}

extern "C" const void* edgedict_ctc_workspace_view(const void* workspace, int B, int T, int U, int which) {
    const CtcWs w = ctc_ws(B, T, U);
    const char* p = (const char*)workspace;
    switch (which) {
        case 0: return p + w.off_lse;
        case 1: return p + w.off_alpha;
        case 2: return p + w.off_beta;
        case 3: return p + w.off_ll;
        case 4: return p + w.off_lpb;
        case 5: return p + w.off_lpl;
        case 6: return p + w.off_flag;
        case 7: return p + w.off_chain;
    }
    return nullptr;
}

extern "C" int edgedict_ctc_loss_forward(const void* logits, int dtype, const int32_t* labels, const int32_t* act_lens,
                                         const int32_t* label_lens, int B, int T, int U, int V, int blank,
                                         int zero_infinity, float* costs, float* reduced, float reduce_scale,
                                         void* workspace, void* stream_) {
    if (int rc = ctc_check("ctc_loss_forward", B, T, U, V, blank, dtype)) return rc;
    ED_CHECK_ARG(logits && (labels || U == 0) && act_lens && label_lens && costs && workspace,
                 "ctc_loss_forward: null pointer argument");
    ED_CHECK_ARG(((uintptr_t)workspace & 15) == 0, "ctc_loss_forward: workspace must be 16-byte aligned");
    hipStream_t stream = (hipStream_t)stream_;
    const CtcWs w = ctc_ws(B, T, U);
    char* p = (char*)workspace;
    float* lse = (float*)(p + w.off_lse);
    float* lpb = (float*)(p + w.off_lpb);
    float* lpl = (float*)(p + w.off_lpl);
    double* alphas = (double*)(p + w.off_alpha);
    double* betas = (double*)(p + w.off_beta);
    double* ll = (double*)(p + w.off_ll);
    int32_t* dead = (int32_t*)(p + w.off_flag);
    int32_t* chain = (int32_t*)(p + w.off_chain);

    ctc_launch_rows(logits, dtype, labels, act_lens, label_lens, B, T, U, V, blank, lse, lpb, lpl, stream);
    ED_CHECK_LAUNCH("ctc_lse_gather");
    if (U > 0) {
        hipLaunchKernelGGL(ctc_label_chain, dim3(B), dim3(256), 0, stream, labels, label_lens, U, chain);
        ED_CHECK_LAUNCH("ctc_label_chain");
    }
    ctc_launch_walk<false>(lpb, lpl, labels, act_lens, label_lens, B, T, U, alphas, betas, ll, stream);
    ED_CHECK_LAUNCH("ctc_alpha_beta");
    hipLaunchKernelGGL(ctc_costs, dim3(1), dim3(256), 0, stream, ll, costs, B, zero_infinity ? 1 : 0, dead, reduced,
                       reduce_scale);
    ED_CHECK_LAUNCH("ctc_costs");
    return ED_OK;
}

// The forced aligner: the row pass of the loss, the Viterbi walk, its back-trace.  ctc_label_chain, the beta walk and
// ctc_costs are not launched; the workspace is the loss's (v where the alphas go).
extern "C" int edgedict_ctc_align(const void* logits, int dtype, const int32_t* labels, const int32_t* act_lens,
                                  const int32_t* label_lens, int B, int T, int U, int V, int blank, int32_t* frames,
                                  int32_t* ends, float* scores, void* workspace, void* stream_) {
    if (int rc = ctc_check("ctc_align", B, T, U, V, blank, dtype)) return rc;
    ED_CHECK_ARG(logits && (labels || U == 0) && act_lens && label_lens && (frames || U == 0) && (ends || U == 0) &&
                     scores && workspace,
                 "ctc_align: null pointer argument");
    ED_CHECK_ARG(((uintptr_t)workspace & 15) == 0, "ctc_align: workspace must be 16-byte aligned");
    hipStream_t stream = (hipStream_t)stream_;
    const CtcWs w = ctc_ws(B, T, U);
    char* p = (char*)workspace;
    float* lse = (float*)(p + w.off_lse);
    float* lpb = (float*)(p + w.off_lpb);
    float* lpl = (float*)(p + w.off_lpl);
    double* v = (double*)(p + w.off_alpha);
    double* ll = (double*)(p + w.off_ll);
    ctc_launch_rows(logits, dtype, labels, act_lens, label_lens, B, T, U, V, blank, lse, lpb, lpl, stream);
    ED_CHECK_LAUNCH("ctc_lse_gather");
    ctc_launch_walk<true>(lpb, lpl, labels, act_lens, label_lens, B, T, U, v, nullptr, ll, stream);
    ED_CHECK_LAUNCH("ctc_alpha_beta (viterbi)");
    hipLaunchKernelGGL(ctc_viterbi_backtrace, dim3(B), dim3(64), 0, stream, v, ll, labels, act_lens, label_lens, T, U,
                       frames, ends, scores);
    ED_CHECK_LAUNCH("ctc_viterbi_backtrace");
    return ED_OK;
}

extern "C" int edgedict_ctc_loss_backward(const void* logits, int dtype, void* grads, const int32_t* labels,
                                          const int32_t* act_lens, const int32_t* label_lens, int B, int T, int U, int V,
                                          int blank, const void* workspace, float grad_scale_host,
                                          const float* grad_scale_dev, int grad_scale_stride, void* stream_) {
    if (int rc = ctc_check("ctc_loss_backward", B, T, U, V, blank, dtype)) return rc;
    ED_CHECK_ARG(logits && grads && (labels || U == 0) && act_lens && label_lens && workspace,
                 "ctc_loss_backward: null pointer argument");
    hipStream_t stream = (hipStream_t)stream_;
    const CtcWs w = ctc_ws(B, T, U);
    const char* p = (const char*)workspace;
    const float* lse = (const float*)(p + w.off_lse);
    const double* alphas = (const double*)(p + w.off_alpha);
    const double* betas = (const double*)(p + w.off_beta);
    const double* ll = (const double*)(p + w.off_ll);
    const int32_t* dead = (const int32_t*)(p + w.off_flag);
    const int32_t* chain = (const int32_t*)(p + w.off_chain);
    const size_t esz = dtype == ED_F32 ? 4 : 2;
    const int vec_ok = ((V * esz) % 16 == 0) && (((uintptr_t)logits & 15) == 0) && (((uintptr_t)grads & 15) == 0);
    const dim3 grid(ed_grid_for(T, 4, max(1, 256 * 16 / B)), B);
    if (dtype == ED_F32)
        hipLaunchKernelGGL(ctc_grad<float>, grid, dim3(256), 0, stream, (const float*)logits, (float*)grads, labels,
                           act_lens, label_lens, T, U, V, blank, lse, alphas, betas, ll, dead, chain, grad_scale_host,
                           grad_scale_dev, grad_scale_stride, vec_ok);
    else
        hipLaunchKernelGGL(ctc_grad<bf16_t>, grid, dim3(256), 0, stream, (const bf16_t*)logits, (bf16_t*)grads, labels,
                           act_lens, label_lens, T, U, V, blank, lse, alphas, betas, ll, dead, chain, grad_scale_host,
                           grad_scale_dev, grad_scale_stride, vec_ok);
    ED_CHECK_LAUNCH("ctc_grad");
    return ED_OK;
}

extern "C" int edgedict_ctc_greedy(const void* logits, int dtype, const int32_t* act_lens, int B, int T, int V, int blank,
                                   int32_t* tokens, int32_t* counts, int32_t* frames, float* neglogp, void* scratch,
                                   void* stream_) {
    if (int rc = ctc_check("ctc_greedy", B, T, 0, V, blank, dtype)) return rc;
    ED_CHECK_ARG(logits && act_lens && tokens && counts && frames && neglogp && scratch,
                 "ctc_greedy: null pointer argument");
    hipStream_t stream = (hipStream_t)stream_;
    int32_t* kbuf = (int32_t*)scratch;
    float* lpbuf = (float*)scratch + (size_t)B * T;
    const size_t esz = dtype == ED_F32 ? 4 : 2;
    const int vec_ok = ((V * esz) % 16 == 0) && (((uintptr_t)logits & 15) == 0);
    const dim3 grid(ed_grid_for(T, 4, max(1, 256 * 16 / B)), B);
    if (dtype == ED_F32)
        hipLaunchKernelGGL(ctc_argmax<float>, grid, dim3(256), 0, stream, (const float*)logits, act_lens, T, V, kbuf,
                           lpbuf, vec_ok);
    else
        hipLaunchKernelGGL(ctc_argmax<bf16_t>, grid, dim3(256), 0, stream, (const bf16_t*)logits, act_lens, T, V, kbuf,
                           lpbuf, vec_ok);
    ED_CHECK_LAUNCH("ctc_argmax");
    hipLaunchKernelGGL(ctc_collapse, dim3(B), dim3(64), 0, stream, kbuf, lpbuf, act_lens, T, blank, tokens, counts,
                       frames, neglogp);
    ED_CHECK_LAUNCH("ctc_collapse");
    return ED_OK;
}
