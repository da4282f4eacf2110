// Batched greedy / streaming RNN-T search loop for gfx950.
//
// Replaces the per-frame Python loops of
//   Transducer.greedy_decode          rnnt/models.py:243-269  (log_softmax -> max, one symbol per
//                                     encoder frame, prediction net advanced for every row and the
//                                     new state kept only where the symbol is not blank)
//   PytorchStreamDecoder.decode       rnnt/stream.py:102-119  (argmax on raw logits, an arg-max
//                                     that is the <unk> id has its logit set to 0 and the arg-max
//                                     is retaken, prediction net advanced only on non-blank)
// The whole time loop runs inside ONE C call: per frame it enqueues the small dense products on
// the MFMA GEMM (gemm.hip), the LSTM cell (lstm.hip) and three tiny kernels from this file
// (broadcast-add+tanh on one frame, row-wise pick, masked state commit).  Nothing returns to the
// host between frames; token ids and scores stay on the device until the caller reads them.
#include "decode_net.hpp"
#include "bias_tables.hpp"

#include <algorithm>
#include <optional>
#include <vector>

namespace {

// hid[b, :] = tanh(E1[b*e_stride + :] + D1[b, :])
template <typename T>
__global__ void add_tanh_rows(const T* __restrict__ E1, long long e_stride,
                              const T* __restrict__ D1, T* __restrict__ hid, int B, int J) {
    const long long n = (long long)B * J;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (long long)gridDim.x * blockDim.x) {
        const int b = (int)(i / J), j = (int)(i % J);
        ElemIO<T>::store(hid + i, tanhf(ElemIO<T>::load(E1 + (long long)b * e_stride + j) +
                                        ElemIO<T>::load(D1 + i)));
    }
}

// One wave64 per row of fp32 logits [B, V]:
//   greedy mode (unk < 0): pred = argmax (first index on ties, as torch.max), score -= log p(pred)
//   stream mode (unk >= 0): pred = argmax of raw logits; if pred == unk the logit is treated as 0
//                           and the arg-max is retaken (rnnt/stream.py:105-108)
__global__ __launch_bounds__(256) void pick_kernel(const float* __restrict__ logits, int B, int V,
                                                   int unk, int32_t* __restrict__ pred,
                                                   int32_t* __restrict__ tokens, int tok_stride,
                                                   int t, float* __restrict__ score, int blank) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;
    const float* z = logits + (long long)b * V;
    float best = -INFINITY;
    int arg = 0x7fffffff;
    for (int v = lane; v < V; v += 64) {
        const float x = z[v];
        if (x > best) { best = x; arg = v; }   // strict >: keeps the first index within a lane
    }
    // wave arg-max with lowest-index tie break
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float ob = __shfl_xor(best, off, 64);
        const int oa = __shfl_xor(arg, off, 64);
        if (ob > best || (ob == best && oa < arg)) { best = ob; arg = oa; }
    }
    if (unk >= 0 && arg == unk) {
        best = -INFINITY;
        arg = 0x7fffffff;
        for (int v = lane; v < V; v += 64) {
            const float x = (v == unk) ? 0.f : z[v];
            if (x > best) { best = x; arg = v; }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float ob = __shfl_xor(best, off, 64);
            const int oa = __shfl_xor(arg, off, 64);
            if (ob > best || (ob == best && oa < arg)) { best = ob; arg = oa; }
        }
    }
    if (score) {
        float s = 0.f;
        for (int v = lane; v < V; v += 64) s += expf(z[v] - best);
        s = wave_sum(s);
        if (lane == 0) score[b] += logf(s);  // -(max log p) = log sum exp(z - max)
    }
    // a row without one comparable logit (all NaN / all -inf: `x > best` never held) leaves the sentinel: it emits blank,
    // as the fused frame does (decode_fused.hip dec_lstm_step) - the prediction network of that row does not advance and
    // no out-of-range id reaches `pred`, `tokens` or the embedding gather
    if ((unsigned)arg >= (unsigned)V) arg = min(max(blank, 0), V - 1);
    if (lane == 0) {
        pred[b] = arg;
        if (tokens) tokens[(long long)b * tok_stride + t] = arg;
    }
}

// where pred[b] != blank: dec_out[b] <- dec_new[b], h[l,b] <- h_new[l,b], c[l,b] <- c_new[l,b]
template <typename T>
__global__ void commit_kernel(const int32_t* __restrict__ pred, int blank, T* __restrict__ dec_out,
                              const T* __restrict__ dec_new, int P2, float* __restrict__ h,
                              const float* __restrict__ h_new, float* __restrict__ c,
                              const float* __restrict__ c_new, int L, int B, int H) {
    const long long n_dec = (long long)B * P2;
    const long long n_st = (long long)L * B * H;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n_dec + n_st;
         i += (long long)gridDim.x * blockDim.x) {
        if (i < n_dec) {
            const int b = (int)(i / P2);
            if (pred[b] != blank) dec_out[i] = dec_new[i];
        } else {
            const long long k = i - n_dec;
            const int b = (int)((k / H) % B);
            if (pred[b] != blank) {
                h[k] = h_new[k];
                c[k] = c_new[k];
            }
        }
    }
}

// One step of an LstmNet composed from the general kernels: the embedding of pred[b], per layer the input product and
// the LSTM cell from (h_state, c_state) [L, B, H] into u.h_new / u.c_new, then out [B, O] (out_dtype) = y_L Wo^T + bo
int composed_lstm_step(int dtype, int B, const LstmNet& n, const int32_t* pred, const float* h_state,
                       const float* c_state, const StepBufs& u, int out_dtype, void* out, hipStream_t s) {
    const int H = n.H;
    int rc;
    if ((rc = edgedict_embedding_fwd(dtype, n.emb_dtype, pred, 1, n.emb, u.x, B, 1, n.E, n.V, 0, 0, s))) return rc;
    const void* xin = u.x;
    int xin_dim = n.E;
    for (int k = 0; k < n.L; ++k) {
        if ((rc = edgedict_gemm(dtype, dtype, xin, xin_dim, 1, n.w_ih[k], xin_dim, 1, u.G, 4 * H, B, 4 * H, xin_dim,
                                n.b_ih[k], n.b_hh[k], 0, 1, s)))
            return rc;
        if ((rc = edgedict_lstm_forward(dtype, u.G, u.Hprev, u.Y[k & 1], u.Cst, n.w_hh[k], nullptr,
                                        h_state + (size_t)k * B * H, c_state + (size_t)k * B * H,
                                        u.h_new + (size_t)k * B * H, u.c_new + (size_t)k * B * H, B, 1, H, nullptr, s)))
            return rc;
        xin = u.Y[k & 1];
        xin_dim = H;
    }
    return edgedict_gemm(dtype, out_dtype, xin, H, 1, n.Wo, H, 1, out, n.O, B, n.O, H, n.bo, nullptr, 0, 1, s);
}

// The joint on the frame e1t composed from the general kernels, for the prediction-network output `dec` [B, P2]:
// D1 = dec W1d^T + b1;  hid = tanh(E1[:, t] + D1);  logits (fp32)
int composed_joint(const SearchNet& net, const char* e1t, const void* dec, const StepBufs& u, hipStream_t s) {
    const int dtype = net.dtype, B = net.B, J = net.J;
    int rc;
    if ((rc = edgedict_gemm(dtype, dtype, dec, net.P2, 1, net.W1d, net.ldw1, 1, u.D1, J, B, J, net.P2, net.b1, nullptr, 0,
                            1, s)))
        return rc;
    dispatch(dtype, [&](auto tag) {
        using T = decltype(tag);
        hipLaunchKernelGGL(add_tanh_rows<T>, dim3(ed_grid_for((long long)B * J, 256)), dim3(256), 0, s, (const T*)e1t,
                           net.e_row_stride, (const T*)u.D1, (T*)u.hid, B, J);
    });
    return edgedict_gemm(dtype, ED_F32, u.hid, J, 1, net.W2, J, 1, u.logits, net.V, B, net.V, J, net.b2, nullptr, 0, 1, s);
}

// the shapes alone, for the greedy search's size query
SearchNet net_dims(int dtype, int B, int J, int V, int E, int L, int H, int P2) {
    SearchNet n{};
    n.dtype = dtype; n.esz = dtype == ED_F32 ? 4 : 2;
    n.B = B; n.J = J; n.V = V; n.P2 = P2;
    n.pred.V = V; n.pred.E = E; n.pred.L = L; n.pred.H = H; n.pred.O = P2;
    return n;
}

}  // namespace

// The beam searches' step composed from the general kernels, in the form of ed_decode_fused_beam_step (decode_fused.hip):
// for the frame-synchronous search of decode_sync.hip, where ed_decode_fused_ok says no
int ed_decode_composed_beam_step(const SearchNet& net, const void* E1t, const float* h_state, const float* c_state,
                                 const StepBufs& u, hipStream_t s) {
    if (int rc = composed_lstm_step(net.dtype, net.B, net.pred, u.pred, h_state, c_state, u, net.dtype, u.dec_new, s))
        return rc;
    return composed_joint(net, (const char*)E1t, u.dec_new, u, s);
}

// The internal LM's logits composed from the general kernels: the joint on the all-zero encoder row `zero_row` [J] for
// every row, from D1 = dec W1d^T + b1 [B, J] as composed_joint left it (d1) - hid = tanh(0 + D1) into `hid`, then the
// logits product into `logits` (fp32 [B, V]).  Two launches.
static int composed_ilm_tail(const SearchNet& net, const void* zero_row, const void* d1, void* hid, float* logits,
                             hipStream_t s) {
    const int B = net.B, J = net.J;
    dispatch(net.dtype, [&](auto tag) {
        using T = decltype(tag);
        hipLaunchKernelGGL(add_tanh_rows<T>, dim3(ed_grid_for((long long)B * J, 256)), dim3(256), 0, s,
                           (const T*)zero_row, 0ll, (const T*)d1, (T*)hid, B, J);
    });
    return edgedict_gemm(net.dtype, ED_F32, hid, J, 1, net.W2, J, 1, logits, net.V, B, net.V, J, net.b2, nullptr, 0, 1, s);
}

// ed_decode_composed_beam_step, then the internal LM's logits of the same rows (ilm_logits, fp32 [B, V]; ilm_hid [B, J]
// scratch): two launches more
int ed_decode_composed_beam_step_ilm(const SearchNet& net, const void* E1t, const float* h_state, const float* c_state,
                                     const StepBufs& u, const void* zero_row, void* ilm_hid, float* ilm_logits,
                                     hipStream_t s) {
    if (int rc = ed_decode_composed_beam_step(net, E1t, h_state, c_state, u, s)) return rc;
    return composed_ilm_tail(net, zero_row, u.D1, ilm_hid, ilm_logits, s);
}

// the internal LM's logits alone for B rows of prediction-network output `dec` [B, P2]: three launches
int ed_decode_composed_ilm_logits(const SearchNet& net, const void* dec, const void* zero_row, void* d1, void* hid,
                                  float* logits, hipStream_t s) {
    if (int rc = edgedict_gemm(net.dtype, net.dtype, dec, net.P2, 1, net.W1d, net.ldw1, 1, d1, net.J, net.B, net.J, net.P2,
                               net.b1, nullptr, 0, 1, s))
        return rc;
    return composed_ilm_tail(net, zero_row, d1, hid, logits, s);
}

// One LM step for `rows` rows (decode_net.hpp): shared by the best-first searches here and the frame-synchronous one
int ed_decode_lm_step(int dtype, int rows, const LstmNet& lm, const float* h_state, const float* c_state,
                      const StepBufs& u, hipStream_t s) {
    if (ed_decode_fused_lm_ok(dtype, lm.emb_dtype, lm.V, lm.E, lm.H))
        return ed_decode_fused_lm_step(dtype, rows, lm, h_state, c_state, u, s);
    return composed_lstm_step(dtype, rows, lm, u.pred, h_state, c_state, u, ED_F32, u.logits, s);
}

extern "C" size_t edgedict_greedy_workspace_bytes(int dtype, int B, int J, int V, int E, int L,
                                                  int H, int P2) {
    if (B <= 0) return 0;
    return ws_layout(net_dims(dtype, B, J, V, E, L, H, P2)).total;
}

extern "C" int edgedict_greedy_decode(
    int dtype, const void* E1, long long e_row_stride, long long e_frame_stride, int B, int T,
    int J, const void* W1d, long long ldw1, const float* b1, int P2, const void* W2,
    const float* b2, int V, const void* emb, int emb_dtype, int E, int L,
    const void* const* w_ih, const void* const* w_hh, const float* const* b_ih,
    const float* const* b_hh, int H, const void* Wp, const float* bp, float* h_state,
    float* c_state, void* dec_out, int blank, int unk, int32_t* tokens_out, int tok_stride,
    float* score, void* workspace, void* stream_) {
    const SearchNet net{dtype, dtype == ED_F32 ? 4 : 2, E1, e_row_stride, e_frame_stride, B, J, W1d, ldw1, b1, P2, W2, b2, V,
                        {emb, emb_dtype, V, E, L, w_ih, w_hh, b_ih, b_hh, H, Wp, bp, P2}, blank, 0, 0, 0, 0};
    if (int rc = check_net(net, "greedy_decode", T >= 0, "", E1 && h_state && c_state && dec_out && workspace, false))
        return rc;
    hipStream_t s = (hipStream_t)stream_;
    const StepBufs u = bind((char*)workspace, ws_layout(net));

    // a frame is five fused launches (decode_fused.hip; the slice partials live in the logits buffer, which the fused
    // frame never fills); odd shapes: composed from the general kernels below
    const bool fused = ed_decode_fused_ok(dtype, emb_dtype, J, V, E, H, P2) &&
                       align256((size_t)B * V * 4) >= ed_decode_fused_ws_bytes(B, V);
    for (int t = 0; t < T; ++t) {
        int rc;
        const char* e1t = net.frame(t);
        if (fused) {
            if ((rc = ed_decode_fused_frame(net, e1t, h_state, c_state, dec_out, {unk, tokens_out, tok_stride, t, score}, u,
                                            s)))
                return rc;
            continue;
        }
        // joint on frame t, then the pick
        if ((rc = composed_joint(net, e1t, dec_out, u, s))) return rc;
        hipLaunchKernelGGL(pick_kernel, dim3((B + 3) / 4), dim3(256), 0, s, u.logits, B, V, unk, u.pred, tokens_out,
                           tok_stride, t, score, blank);
        // prediction network step on the picked symbols (for every row, committed where != blank)
        if ((rc = composed_lstm_step(dtype, B, net.pred, u.pred, h_state, c_state, u, dtype, u.dec_new, s))) return rc;
        const long long n = (long long)B * P2 + (long long)L * B * H;
        dispatch(dtype, [&](auto tag) {
            using ET = decltype(tag);
            hipLaunchKernelGGL(commit_kernel<ET>, dim3(ed_grid_for(n, 256)), dim3(256), 0, s, u.pred, blank, (ET*)dec_out,
                               (const ET*)u.dec_new, P2, h_state, u.h_new, c_state, u.c_new, L, B, H);
        });
    }
    ED_CHECK_LAUNCH("greedy_decode");
    return ED_OK;
}


// =====================================================================================
// Beam search (Graves 2012) as the reference's legacy Transducer.beam_search runs it
// (models.py:121-202, prefix=False), for a batch of utterances in lockstep.
//
// Per utterance and frame the reference keeps two Python lists: A (hypotheses still to expand) and
// B (hypotheses that emitted blank in this frame).  Here A is a score POOL in list order:
//   pool[0 .. W)                 the (at most W) survivors of the previous frame
//   pool[W + e*V + k]            child k of the e-th expansion of this frame (-inf for k == blank
//                                and for popped entries)
// so "max(A), first one on ties" is an arg-max with lowest-index tie break over the pool.  A child
// is materialised (token-tree node, state) only when it is popped.  Hypothesis = (node of the token
// tree, prediction-network state reference, last token, fp64 log-probability); the state a
// hypothesis carries is the one BEFORE its last token was consumed (models.py:170-171,185), the
// expansion recomputes the step on that last token.  B keeps its first W entries in insertion order
// (the reference's `sorted(...)` calls discard their result, models.py:141,195-196).
// One lockstep iteration = pop -> prediction-network step -> joint -> expand for every utterance
// whose loop is still open; the host reads the open flags once per iteration after the first W
// (an utterance needs at least W expansions per frame to fill B).
// =====================================================================================
namespace {

struct BeamPtrs {
    double* pool;        // [B][W + EM*V]
    double* bp_logp;     // [B][W]   survivors of the previous frame
    int32_t* bp_node;    // [B][W]
    int32_t* n_bp;       // [B]
    float* bp_h[2];      // [B][W][L][H] double-buffered per frame
    float* bp_c[2];
    double* bn_logp;     // [B][W]   B of the current frame (first W entries)
    int32_t* bn_node;
    int32_t* bn_ref;
    int32_t* n_b;        // [B]      len(B)
    double* max_b;       // [B]
    double* blk_max;     // [B][1 + EM]  max of pool segment 0 (the survivors) / 1 + e (children of expansion e) ...
    int32_t* blk_arg;    // [B][1 + EM]  ... and its first position in the pool (INT_MAX: nothing left)
    int32_t* exp_node;   // [B][EM]  node / state reference / score of the e-th popped hypothesis
    int32_t* exp_ref;
    double* exp_logp;
    int32_t* e_count;    // [B]
    float* f_h;          // [B][EM][L][H] states created in this frame
    float* f_c;
    int2* nodes;         // [B][NODES] (parent, token)
    int32_t* n_nodes;    // [B]
    int32_t* open;       // [B] the while-loop of this utterance is still running
    int32_t* lens;       // [B]
    int32_t* flags;      // [0] expansion cap hit, [1] node cap hit
    long long* total_exp;// [1]
    int32_t* root_tok;   // [B] last token of the tree root (node -1); null: BOS (the offline search)
    long long* stream_exp;// [B] expansions per utterance, or null
    // LM shallow fusion (all null / 0 without an LM): the LM's (h, c) ride along with the prediction network's, under the
    // same state references
    float* lm_bp_h[2];   // [B][W][lm_L][lm_H] double-buffered per frame
    float* lm_bp_c[2];
    float* lm_f_h;       // [B][EM][lm_L][lm_H] states created in this frame
    float* lm_f_c;
    int32_t* lm_pred;    // [B] the token the LM consumes in this iteration
    float* lm_h_state;   // [lm_L][B][lm_H] the popped hypothesis' LM state
    float* lm_c_state;
    const long long* n_committed;   // [B] committed tokens per stream, or null (offline: nothing committed)
    int lm_L, lm_H, lm_bos;
    // detail per token-tree node, beside `nodes` (both null: not kept - the plain searches): the encoder frame on which
    // the expansion that produced the node's token ran, and the token's score increment
    int32_t* nd_frame;   // [B][NODES]
    double* nd_logp;     // [B][NODES]
    const long long* frames_done;   // [B] frames of the stream since its reset, before this advance; null: 0 (offline)
    // contextual biasing (all null without a bias list): one phrase-automaton state per hypothesis, under the same state
    // references as (h, c) - the state BEFORE the hypothesis' last token - and the automaton's tables (edgedict_beam_bias_t)
    int32_t* bias_bp[2]; // [B][W] double-buffered per frame
    int32_t* bias_f;     // [B][EM] states made in this frame: goto(carried state, last token) of the e-th popped hypothesis
    const int32_t* bias_root_next;  // [V]
    const double* bias_held;        // [S]
    const double* bias_pend;        // [S]
    const int32_t* bias_row_ptr;    // [S + 1]
    const int32_t* bias_exc_tok;    // [n_exc] sorted inside a row
    const int32_t* bias_exc_next;   // [n_exc]
    int bias_S;                     // states of the automaton: every state read from a table or a pool is clamped to it
};

// bias_state(p, s) / bias_goto(p, s, k), the automaton's lookup on these tables: bias_tables.hpp

// (max, first position) of a workgroup's per-thread candidates: butterfly inside a wave, the four waves through LDS.
// Ties go to the lower position, -inf candidates carry INT_MAX.  Every thread gets the result.
__device__ __forceinline__ void block_argmax(double& v, int& a, double* s_v, int* s_a) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const double ov = __shfl_xor(v, off, 64);
        const int oa = __shfl_xor(a, off, 64);
        if (ov > v || (ov == v && oa < a)) { v = ov; a = oa; }
    }
    const int wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    __syncthreads();                       // (s_v / s_a may still be read from a previous use)
    if ((threadIdx.x & 63) == 0) { s_v[wave] = v; s_a[wave] = a; }
    __syncthreads();
    v = s_v[0]; a = s_a[0];
    for (int w = 1; w < nw; ++w)
        if (s_v[w] > v || (s_v[w] == v && s_a[w] < a)) { v = s_v[w]; a = s_a[w]; }
}
__device__ __forceinline__ float block_sum_max(float x, bool is_max, float* s_f) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const float o = __shfl_xor(x, off, 64);
        x = is_max ? fmaxf(x, o) : x + o;
    }
    const int wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s_f[wave] = x;
    __syncthreads();
    x = s_f[0];
    for (int w = 1; w < nw; ++w) x = is_max ? fmaxf(x, s_f[w]) : x + s_f[w];
    return x;
}

// A pool of W + expansions x V fp64 scores per utterance is searched twice per iteration (arg-max for the pop, max for
// the stop test): 20 k scores after ten expansions.  Each segment - the survivors, the V children of one expansion -
// therefore keeps its (max, first position); a pop or an expansion rescans ONE segment and then only the segment maxima.
__global__ __launch_bounds__(64) void beam_frame_begin(BeamPtrs p, int t, int W, int EM, int V) {
    const int b = blockIdx.x;
    const bool act = t < p.lens[b];
    if (threadIdx.x == 0) {
        p.open[b] = act ? 1 : 0;
        if (act) {
            p.e_count[b] = 0;
            p.n_b[b] = 0;
            p.max_b[b] = -INFINITY;
        }
    }
    if (!act) return;
    double best = -INFINITY;
    int arg = 0x7fffffff;
    const int nbp = p.n_bp[b];
    for (int i = threadIdx.x; i < W; i += 64) {
        const double v = i < nbp ? p.bp_logp[b * W + i] : -INFINITY;
        p.pool[(size_t)b * (W + (size_t)EM * V) + i] = v;
        if (v > best) { best = v; arg = i; }
    }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const double ov = __shfl_xor(best, off, 64);
        const int oa = __shfl_xor(arg, off, 64);
        if (ov > best || (ov == best && oa < arg)) { best = ov; arg = oa; }
    }
    if (threadIdx.x == 0) {
        p.blk_max[(size_t)b * (EM + 1)] = best;
        p.blk_arg[(size_t)b * (EM + 1)] = arg;
    }
}

// y* = max(A) (first on ties), removed from A; its last token -> pred, its state -> h/c_state
// DETAIL: a node created here also records its frame (t, counted from the stream's reset) and its token's increment
//   score(child in the pool) - score(popped parent) = pool[idx] - exp_logp[ep]      (fp64)
// which with an LM is the fused increment lp_rnnt + (lm_weight lp_lm + length_bonus), and with a bias list includes D.
// BIAS: y*'s automaton state s = goto(carried state, last token) goes under the expansion's slot (bias_f), where
// beam_expand reads it and a child's pop finds it as its carried state.
template <bool DETAIL, bool BIAS>
__device__ __forceinline__ void beam_pop_body(BeamPtrs& p, int cur, int W, int V, int EM, int L, int H, int B, int NODES,
                                              int bos, int32_t* __restrict__ pred, float* __restrict__ h_state,
                                              float* __restrict__ c_state, int t) {
    const int b = blockIdx.x, tid = threadIdx.x;
    if (!p.open[b]) return;
    double* pool = p.pool + (size_t)b * (W + (size_t)EM * V);
    const int e_n = p.e_count[b];
    double* bmax = p.blk_max + (size_t)b * (EM + 1);
    int32_t* barg = p.blk_arg + (size_t)b * (EM + 1);
    __shared__ double sb[4];
    __shared__ int sa[4];
    __shared__ int s_ref;
    // arg-max over the segment maxima (segments are in pool order, so the first position of the lowest segment wins ties)
    double best = -INFINITY;
    int arg = 0x7fffffff;
    for (int i = tid; i <= e_n; i += 256) {
        const double v = bmax[i];
        const int a = barg[i];
        if (v > best || (v == best && a < arg)) { best = v; arg = a; }
    }
    block_argmax(best, arg, sb, sa);
    const int idx = arg;
    const double popped = best;
    if (idx == 0x7fffffff) {                 // nothing left in A (cannot happen: a frame starts with >= 1 survivor)
        if (tid == 0) { p.flags[0] = 1; p.open[b] = 0; }
        return;
    }
    // the popped entry leaves A: rescan its segment
    {
        const int seg = idx < W ? 0 : 1 + (idx - W) / V;
        const int lo = seg == 0 ? 0 : W + (seg - 1) * V, n = seg == 0 ? W : V;
        double v2 = -INFINITY;
        int a2 = 0x7fffffff;
        for (int i = tid; i < n; i += 256) {
            const double v = (lo + i == idx) ? -INFINITY : pool[lo + i];
            if (v > v2) { v2 = v; a2 = lo + i; }
        }
        block_argmax(v2, a2, sb, sa);
        if (tid == 0) { bmax[seg] = v2; barg[seg] = v2 == -INFINITY ? 0x7fffffff : a2; }
    }
    if (tid == 0) {
        const int e = e_n;
        int node, ref, tok;
        if (idx < W) {
            node = p.bp_node[b * W + idx];
            ref = idx;
        } else {
            const int ep = (idx - W) / V, k = (idx - W) % V;
            int nn = p.n_nodes[b];
            if (nn >= NODES) { p.flags[1] = 1; nn = NODES - 1; }
            p.nodes[(size_t)b * NODES + nn] = make_int2(p.exp_node[b * EM + ep], k);
            if constexpr (DETAIL) {
                p.nd_frame[(size_t)b * NODES + nn] = (int32_t)((p.frames_done ? p.frames_done[b] : 0ll) + t);
                p.nd_logp[(size_t)b * NODES + nn] = __dsub_rn(popped, p.exp_logp[b * EM + ep]);
            }
            p.n_nodes[b] = nn + 1;
            node = nn;
            ref = W + ep;
        }
        tok = node < 0 ? (p.root_tok ? p.root_tok[b] : bos) : p.nodes[(size_t)b * NODES + node].y;
        pool[idx] = -INFINITY;
        p.exp_node[b * EM + e] = node;
        p.exp_ref[b * EM + e] = ref;
        p.exp_logp[b * EM + e] = popped;
        pred[b] = tok;
        // the LM's root token: lm_bos until the stream has committed a token, then the last committed one (root_tok)
        if (p.lm_pred)
            p.lm_pred[b] = node >= 0 ? tok : (p.n_committed && p.n_committed[b] > 0 ? p.root_tok[b] : p.lm_bos);
        if constexpr (BIAS) {
            const int s0 = ref < W ? p.bias_bp[cur][b * W + ref] : p.bias_f[b * EM + (ref - W)];
            p.bias_f[b * EM + e] = tok >= 0 && tok < V ? bias_goto(p, s0, tok) : 0;
        }
        s_ref = ref;
    }
    __syncthreads();
    const int ref = s_ref;
    const size_t LH = (size_t)L * H;
    const float* sh = ref < W ? p.bp_h[cur] + ((size_t)b * W + ref) * LH : p.f_h + ((size_t)b * EM + (ref - W)) * LH;
    const float* sc = ref < W ? p.bp_c[cur] + ((size_t)b * W + ref) * LH : p.f_c + ((size_t)b * EM + (ref - W)) * LH;
    for (int i = tid; i < (int)LH; i += 256) {
        const int l = i / H, j = i % H;
        h_state[((size_t)l * B + b) * H + j] = sh[i];
        c_state[((size_t)l * B + b) * H + j] = sc[i];
    }
    if (p.lm_pred) {
        const int LL = p.lm_L, HL = p.lm_H;
        const size_t LHl = (size_t)LL * HL;
        const float* lh = ref < W ? p.lm_bp_h[cur] + ((size_t)b * W + ref) * LHl : p.lm_f_h + ((size_t)b * EM + (ref - W)) * LHl;
        const float* lc = ref < W ? p.lm_bp_c[cur] + ((size_t)b * W + ref) * LHl : p.lm_f_c + ((size_t)b * EM + (ref - W)) * LHl;
        for (int i = tid; i < (int)LHl; i += 256) {
            const int l = i / HL, j = i % HL;
            p.lm_h_state[((size_t)l * B + b) * HL + j] = lh[i];
            p.lm_c_state[((size_t)l * B + b) * HL + j] = lc[i];
        }
    }
}

__global__ __launch_bounds__(256) void beam_pop(BeamPtrs p, int cur, int W, int V, int EM, int L,
                                                int H, int B, int NODES, int bos,
                                                int32_t* __restrict__ pred, float* __restrict__ h_state,
                                                float* __restrict__ c_state) {
    beam_pop_body<false, false>(p, cur, W, V, EM, L, H, B, NODES, bos, pred, h_state, c_state, 0);
}

// beam_pop that keeps the detail per node; t = the frame of this advance
__global__ __launch_bounds__(256) void beam_pop_detail(BeamPtrs p, int cur, int W, int V, int EM, int L, int H, int B,
                                                       int NODES, int bos, int32_t* __restrict__ pred,
                                                       float* __restrict__ h_state, float* __restrict__ c_state, int t) {
    beam_pop_body<true, false>(p, cur, W, V, EM, L, H, B, NODES, bos, pred, h_state, c_state, t);
}

// the two pops with a bias list
__global__ __launch_bounds__(256) void beam_pop_bias(BeamPtrs p, int cur, int W, int V, int EM, int L, int H, int B,
                                                     int NODES, int bos, int32_t* __restrict__ pred,
                                                     float* __restrict__ h_state, float* __restrict__ c_state) {
    beam_pop_body<false, true>(p, cur, W, V, EM, L, H, B, NODES, bos, pred, h_state, c_state, 0);
}

__global__ __launch_bounds__(256) void beam_pop_detail_bias(BeamPtrs p, int cur, int W, int V, int EM, int L, int H,
                                                            int B, int NODES, int bos, int32_t* __restrict__ pred,
                                                            float* __restrict__ h_state, float* __restrict__ c_state,
                                                            int t) {
    beam_pop_body<true, true>(p, cur, W, V, EM, L, H, B, NODES, bos, pred, h_state, c_state, t);
}

// log-softmax of the joint's logits; children into the pool, the blank child into B, the new
// prediction-network state into the frame's state pool; then the reference's stop test.
// LM: the LM's logits get the same log-softmax, and a non-blank child k scores
//   base + (double)lp_rnnt[k] + (lm_w * (double)lp_lm[k] + lm_b)      (fp64, this order, no contraction)
// the blank child keeps base + lp_rnnt[blank]; the LM's new state goes into its frame pool under the same slot.
// BIAS: with s = bias_f[slot] (written by the pop) a non-blank child k scores
//   (that score) + (held[goto(s, k)] - pend[s])                       (fp64, this order, no contraction)
// The segment is filled with the root's transition goto(0, k) for every k, then - after a barrier - the few tokens of
// s's exception row are rewritten with their own target, and only then is the segment's (max, first position) taken.
template <bool LM, bool BIAS>
__device__ __forceinline__ void beam_expand_body(BeamPtrs& p, const float* __restrict__ logits,
                                                 const float* __restrict__ h_new, const float* __restrict__ c_new,
                                                 const float* __restrict__ lm_logits,
                                                 const float* __restrict__ lm_h_new,
                                                 const float* __restrict__ lm_c_new, double lm_w, double lm_b,
                                                 int W, int V, int EM, int L, int H, int B, int blank) {
    const int b = blockIdx.x, tid = threadIdx.x;
    if (!p.open[b]) return;
    const float* z = logits + (size_t)b * V;
    __shared__ float sf[4];
    __shared__ double sd[4];
    __shared__ int si[4];
    float m = -INFINITY;
    for (int v = tid; v < V; v += 256) m = fmaxf(m, z[v]);
    m = block_sum_max(m, true, sf);
    float s = 0.f;
    for (int v = tid; v < V; v += 256) s += expf(z[v] - m);
    s = block_sum_max(s, false, sf);
    const float logs = logf(s);
    const float* zl = LM ? lm_logits + (size_t)b * V : nullptr;
    float ml = 0.f, logsl = 0.f;
    if constexpr (LM) {
        ml = -INFINITY;
        for (int v = tid; v < V; v += 256) ml = fmaxf(ml, zl[v]);
        ml = block_sum_max(ml, true, sf);
        float sl = 0.f;
        for (int v = tid; v < V; v += 256) sl += expf(zl[v] - ml);
        sl = block_sum_max(sl, false, sf);
        logsl = logf(sl);
    }
    const int e = p.e_count[b];
    const double base = p.exp_logp[b * EM + e];
    double* pool = p.pool + (size_t)b * (W + (size_t)EM * V);
    const int lo = W + e * V;
    double* seg = pool + lo;
    double best = -INFINITY;
    int arg = 0x7fffffff;
    // child v's score before the bias term
    auto child = [&](int v) -> double {
        if constexpr (LM)
            return base + (double)((z[v] - m) - logs) + __dadd_rn(__dmul_rn(lm_w, (double)((zl[v] - ml) - logsl)), lm_b);
        else
            return base + (double)((z[v] - m) - logs);
    };
    if constexpr (BIAS) {
        const int st = bias_state(p, p.bias_f[b * EM + e]);
        const double pend_s = p.bias_pend[st];
        for (int v = tid; v < V; v += 256)
            seg[v] = v == blank ? -INFINITY : __dadd_rn(child(v), __dsub_rn(p.bias_held[bias_state(p, p.bias_root_next[v])], pend_s));
        __syncthreads();
        const int r0 = p.bias_row_ptr[st], r1 = p.bias_row_ptr[st + 1];
        for (int i = r0 + tid; i < r1; i += 256) {
            const int v = p.bias_exc_tok[i];
            if (v != blank && v >= 0 && v < V)
                seg[v] = __dadd_rn(child(v), __dsub_rn(p.bias_held[bias_state(p, p.bias_exc_next[i])], pend_s));
        }
        __syncthreads();
        for (int v = tid; v < V; v += 256) {
            const double c = seg[v];
            if (c > best) { best = c; arg = lo + v; }
        }
    } else {
        for (int v = tid; v < V; v += 256) {
            const double c = v == blank ? -INFINITY : child(v);
            seg[v] = c;
            if (c > best) { best = c; arg = lo + v; }
        }
    }
    const size_t LH = (size_t)L * H;
    float* dh = p.f_h + ((size_t)b * EM + e) * LH;
    float* dc = p.f_c + ((size_t)b * EM + e) * LH;
    for (int i = tid; i < (int)LH; i += 256) {
        const int l = i / H, j = i % H;
        dh[i] = h_new[((size_t)l * B + b) * H + j];
        dc[i] = c_new[((size_t)l * B + b) * H + j];
    }
    if constexpr (LM) {
        const int HL = p.lm_H;
        const size_t LHl = (size_t)p.lm_L * HL;
        float* lh = p.lm_f_h + ((size_t)b * EM + e) * LHl;
        float* lc = p.lm_f_c + ((size_t)b * EM + e) * LHl;
        for (int i = tid; i < (int)LHl; i += 256) {
            const int l = i / HL, j = i % HL;
            lh[i] = lm_h_new[((size_t)l * B + b) * HL + j];
            lc[i] = lm_c_new[((size_t)l * B + b) * HL + j];
        }
    }
    // the new segment's (max, first position), then max(A) = max over the segment maxima
    block_argmax(best, arg, sd, si);
    double* bmax = p.blk_max + (size_t)b * (EM + 1);
    if (tid == 0) {
        bmax[e + 1] = best;
        p.blk_arg[(size_t)b * (EM + 1) + e + 1] = arg;
    }
    double amax = best;
    int dummy = 0;
    for (int i = tid; i <= e; i += 256) amax = fmax(amax, bmax[i]);       // (segments 0 .. e: written by earlier kernels)
    block_argmax(amax, dummy, sd, si);
    if (tid == 0) {
        const double lpb = base + (double)((z[blank] - m) - logs);
        const int j = p.n_b[b];
        if (j < W) {
            p.bn_logp[b * W + j] = lpb;
            p.bn_node[b * W + j] = p.exp_node[b * EM + e];
            p.bn_ref[b * W + j] = p.exp_ref[b * EM + e];
        }
        p.n_b[b] = j + 1;
        const double mb = fmax(p.max_b[b], lpb);
        p.max_b[b] = mb;
        p.e_count[b] = e + 1;
        atomicAdd((unsigned long long*)p.total_exp, 1ull);
        if (p.stream_exp) p.stream_exp[b] += 1;
        if (j + 1 >= W && mb >= amax) {
            p.open[b] = 0;
        } else if (e + 1 >= EM) {
            p.flags[0] = 1;
            p.open[b] = 0;
        }
    }
}

__global__ __launch_bounds__(256) void beam_expand(BeamPtrs p, const float* __restrict__ logits,
                                                   const float* __restrict__ h_new,
                                                   const float* __restrict__ c_new, int W, int V,
                                                   int EM, int L, int H, int B, int blank) {
    beam_expand_body<false, false>(p, logits, h_new, c_new, nullptr, nullptr, nullptr, 0.0, 0.0, W, V, EM, L, H, B,
                                   blank);
}

// beam_expand with LM shallow fusion (one workgroup per utterance; both rows are V <= a few thousand floats, so this is
// latency-bound: the two log-softmaxes are four block reductions over L2-resident rows)
__global__ __launch_bounds__(256) void beam_expand_lm(BeamPtrs p, const float* __restrict__ logits,
                                                      const float* __restrict__ h_new, const float* __restrict__ c_new,
                                                      const float* __restrict__ lm_logits,
                                                      const float* __restrict__ lm_h_new,
                                                      const float* __restrict__ lm_c_new, double lm_w, double lm_b,
                                                      int W, int V, int EM, int L, int H, int B, int blank) {
    beam_expand_body<true, false>(p, logits, h_new, c_new, lm_logits, lm_h_new, lm_c_new, lm_w, lm_b, W, V, EM, L, H, B,
                                  blank);
}

// the two expansions with a bias list
__global__ __launch_bounds__(256) void beam_expand_bias(BeamPtrs p, const float* __restrict__ logits,
                                                        const float* __restrict__ h_new,
                                                        const float* __restrict__ c_new, int W, int V, int EM, int L,
                                                        int H, int B, int blank) {
    beam_expand_body<false, true>(p, logits, h_new, c_new, nullptr, nullptr, nullptr, 0.0, 0.0, W, V, EM, L, H, B, blank);
}

__global__ __launch_bounds__(256) void beam_expand_lm_bias(BeamPtrs p, const float* __restrict__ logits,
                                                           const float* __restrict__ h_new,
                                                           const float* __restrict__ c_new,
                                                           const float* __restrict__ lm_logits,
                                                           const float* __restrict__ lm_h_new,
                                                           const float* __restrict__ lm_c_new, double lm_w, double lm_b,
                                                           int W, int V, int EM, int L, int H, int B, int blank) {
    beam_expand_body<true, true>(p, logits, h_new, c_new, lm_logits, lm_h_new, lm_c_new, lm_w, lm_b, W, V, EM, L, H, B,
                                 blank);
}

// B = B[:W] becomes the next frame's survivors (states gathered into the other buffer)
__global__ __launch_bounds__(256) void beam_frame_end(BeamPtrs p, int t, int cur, int W, int EM,
                                                      int L, int H) {
    const int b = blockIdx.x, tid = threadIdx.x;
    if (t >= p.lens[b]) return;
    const int n = min(p.n_b[b], W);
    const size_t LH = (size_t)L * H;
    for (int j = 0; j < n; ++j) {
        const int ref = p.bn_ref[b * W + j];
        const float* sh = ref < W ? p.bp_h[cur] + ((size_t)b * W + ref) * LH : p.f_h + ((size_t)b * EM + (ref - W)) * LH;
        const float* sc = ref < W ? p.bp_c[cur] + ((size_t)b * W + ref) * LH : p.f_c + ((size_t)b * EM + (ref - W)) * LH;
        float* dh = p.bp_h[cur ^ 1] + ((size_t)b * W + j) * LH;
        float* dc = p.bp_c[cur ^ 1] + ((size_t)b * W + j) * LH;
        for (int i = tid; i < (int)LH; i += 256) { dh[i] = sh[i]; dc[i] = sc[i]; }
        if (p.lm_pred) {
            const size_t LHl = (size_t)p.lm_L * p.lm_H;
            const float* lh = ref < W ? p.lm_bp_h[cur] + ((size_t)b * W + ref) * LHl
                                      : p.lm_f_h + ((size_t)b * EM + (ref - W)) * LHl;
            const float* lc = ref < W ? p.lm_bp_c[cur] + ((size_t)b * W + ref) * LHl
                                      : p.lm_f_c + ((size_t)b * EM + (ref - W)) * LHl;
            float* ldh = p.lm_bp_h[cur ^ 1] + ((size_t)b * W + j) * LHl;
            float* ldc = p.lm_bp_c[cur ^ 1] + ((size_t)b * W + j) * LHl;
            for (int i = tid; i < (int)LHl; i += 256) { ldh[i] = lh[i]; ldc[i] = lc[i]; }
        }
    }
    if (tid < n) {
        p.bp_logp[b * W + tid] = p.bn_logp[b * W + tid];
        p.bp_node[b * W + tid] = p.bn_node[b * W + tid];
    }
    if (p.bias_f)
        for (int j = tid; j < n; j += 256) {
            const int ref = p.bn_ref[b * W + j];
            p.bias_bp[cur ^ 1][b * W + j] = ref < W ? p.bias_bp[cur][b * W + ref] : p.bias_f[b * EM + (ref - W)];
        }
    if (tid == 0) p.n_bp[b] = n;
}

__global__ void beam_init(BeamPtrs p, int B, int W) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    p.n_bp[b] = 1;               // B = [empty hypothesis], models.py:148
    p.bp_logp[b * W] = 0.0;
    p.bp_node[b * W] = -1;
    p.n_nodes[b] = 0;
    p.open[b] = 0;
    if (p.bias_bp[0]) p.bias_bp[0][b * W] = 0;      // the empty hypothesis is at the automaton's root
    if (b == 0) { p.flags[0] = p.flags[1] = 0; *p.total_exp = 0; }
}

// ---- prefix=True (models.py:145-161): the prediction-network output of every expansion is kept per token-tree node
// (the reference's Sequence.g), and at the start of a frame the host - which owns the list logic of that branch -
// asks for log p(token | frame t, stored prediction) of a batch of (utterance, node, token) queries
template <typename T>
__global__ void beam_store_pred(BeamPtrs p, const T* __restrict__ dec_new, T* __restrict__ node_pred, int EM,
                                int NODES, int P2) {
    const int b = blockIdx.x;
    if (!p.open[b]) return;
    const int node = p.exp_node[b * EM + p.e_count[b]];        // -1 = the empty hypothesis: slot 0
    T* dst = node_pred + ((size_t)b * (NODES + 1) + (node + 1)) * P2;
    for (int i = threadIdx.x; i < P2; i += blockDim.x) dst[i] = dec_new[(size_t)b * P2 + i];
}
template <typename T>
__global__ void beam_query_gather(const T* __restrict__ node_pred, const int32_t* __restrict__ q_row,
                                  const int32_t* __restrict__ q_node, T* __restrict__ q_pred, int NODES, int P2) {
    const int q = blockIdx.x;
    const T* src = node_pred + ((size_t)q_row[q] * (NODES + 1) + (q_node[q] + 1)) * P2;
    for (int i = threadIdx.x; i < P2; i += blockDim.x) q_pred[(size_t)q * P2 + i] = src[i];
}
// hid[q, :] = tanh(E1[row(q), frame t, :] + D1[q, :])
template <typename T>
__global__ void beam_query_hidden(const T* __restrict__ E1t, long long e_stride, const int32_t* __restrict__ q_row,
                                  const T* __restrict__ D1, T* __restrict__ hid, int J) {
    const int q = blockIdx.x;
    const T* e = E1t + (long long)q_row[q] * e_stride;
    for (int j = threadIdx.x; j < J; j += blockDim.x)
        ElemIO<T>::store(hid + (size_t)q * J + j, tanhf(ElemIO<T>::load(e + j) + ElemIO<T>::load(D1 + (size_t)q * J + j)));
}
// out[q] = log_softmax(logits[q, :])[tok(q)], the arithmetic of beam_expand
__global__ __launch_bounds__(256) void beam_query_logp(const float* __restrict__ logits, const int32_t* __restrict__ q_tok,
                                                       float* __restrict__ out, int V) {
    const int q = blockIdx.x, tid = threadIdx.x;
    const float* z = logits + (size_t)q * V;
    __shared__ float sf[256];
    float m = -INFINITY;
    for (int v = tid; v < V; v += 256) m = fmaxf(m, z[v]);
    sf[tid] = m;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (tid < off) sf[tid] = fmaxf(sf[tid], sf[tid + off]);
        __syncthreads();
    }
    m = sf[0];
    __syncthreads();
    float sm = 0.f;
    for (int v = tid; v < V; v += 256) sm += expf(z[v] - m);
    sf[tid] = sm;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (tid < off) sf[tid] += sf[tid + off];
        __syncthreads();
    }
    if (tid == 0) out[q] = (z[q_tok[q]] - m) - logf(sf[0]);
}
constexpr int BEAM_QMAX = 1024;      // queries per batch of the prefix branch

template <typename T>
inline T* at(char* base, size_t off) { return (T*)(base + off); }

// The survivors of the previous frame (the list B) and the token tree: in the per-call workspace (offline search) or in
// the persistent state of the streams
struct SurvivorOffs {
    size_t bp_logp, bp_node, n_bp, bp_h0, bp_c0, nodes, n_nodes;
};

// per-call workspace of both beam searches
struct BeamWs {
    Ws step;   // the greedy loop's per-iteration buffers (prediction-network step + joint)
    size_t h_state, c_state;
    SurvivorOffs sv;                                                                   // offline only
    size_t pool, bp_h1, bp_c1, bn_logp, bn_node, bn_ref, n_b, max_b, blk_max, blk_arg, exp_node, exp_ref, exp_logp, e_count,
        f_h, f_c, open, lens, flags, total_exp;
    size_t c_old, c_mark, commit, n_commit;                                            // streaming only: compaction scratch
    size_t node_pred, q_row, q_node, q_tok, q_pred, q_D1, q_hid, q_logits, q_out;      // prefix = 1 only
    size_t total;
};
// nodes = token-tree capacity per utterance.  stream: the survivors and the tree live in the state
// (beam_stream_state_layout) and the compaction scratch is appended.  The order of the take() calls IS the layout callers
// have sized their buffers for (tests/golden/search_sizes.json): leave it alone.
inline BeamWs beam_layout(const SearchNet& n, size_t nodes, int prefix, bool stream) {
    BeamWs w{};
    w.step = ws_layout(n);
    size_t o = w.step.total;
    auto take = [&](size_t bytes) { size_t r = o; o += align256(bytes); return r; };
    auto own = [&](size_t bytes) { return stream ? (size_t)0 : take(bytes); };
    const size_t B = n.B, W = n.W, EM = n.EM, V = n.V, LH = (size_t)n.pred.L * n.pred.H;
    w.h_state = take(B * LH * 4);
    w.c_state = take(B * LH * 4);
    w.pool = take(B * (W + EM * V) * 8);
    w.sv.bp_logp = own(B * W * 8);
    w.sv.bp_node = own(B * W * 4);
    w.sv.n_bp = own(B * 4);
    w.sv.bp_h0 = own(B * W * LH * 4);
    w.bp_h1 = take(B * W * LH * 4);
    w.sv.bp_c0 = own(B * W * LH * 4);
    w.bp_c1 = take(B * W * LH * 4);
    w.bn_logp = take(B * W * 8);
    w.bn_node = take(B * W * 4);
    w.bn_ref = take(B * W * 4);
    w.n_b = take(B * 4);
    w.max_b = take(B * 8);
    w.blk_max = take(B * (EM + 1) * 8);
    w.blk_arg = take(B * (EM + 1) * 4);
    w.exp_node = take(B * EM * 4);
    w.exp_ref = take(B * EM * 4);
    w.exp_logp = take(B * EM * 8);
    w.e_count = take(B * 4);
    w.f_h = take(B * EM * LH * 4);
    w.f_c = take(B * EM * LH * 4);
    w.sv.nodes = own(B * nodes * 8);
    w.sv.n_nodes = own(B * 4);
    w.open = take(B * 4);
    w.lens = take(B * 4);
    w.flags = take(8);
    w.total_exp = take(8);
    if (stream) {
        w.c_old = take(B * nodes * 8);
        w.c_mark = take(B * nodes * 4);
        w.commit = take(B * nodes * 4);
        w.n_commit = take(B * 4);
    }
    if (prefix) {
        const size_t esz = n.esz, J = n.J, P2 = n.P2;
        w.node_pred = take(B * (nodes + 1) * P2 * esz);
        w.q_row = take((size_t)BEAM_QMAX * 4);
        w.q_node = take((size_t)BEAM_QMAX * 4);
        w.q_tok = take((size_t)BEAM_QMAX * 4);
        w.q_pred = take((size_t)BEAM_QMAX * P2 * esz);
        w.q_D1 = take((size_t)BEAM_QMAX * J * esz);
        w.q_hid = take((size_t)BEAM_QMAX * J * esz);
        w.q_logits = take((size_t)BEAM_QMAX * V * 4);
        w.q_out = take((size_t)BEAM_QMAX * 4);
    }
    w.total = o;
    return w;
}

// persistent state, per stream; with an LM the survivors' LM (h, c) [S][W][lm_L][lm_H] are appended behind the plain
// state (so that edgedict_beam_stream_read serves both forms), and with a bias list the survivors' automaton states
// [S][W] behind those
struct BeamStreamState {
    SurvivorOffs sv;
    size_t root_tok, n_committed, n_exp, lm_bp_h, lm_bp_c, bias_bp, total;
};
inline BeamStreamState beam_stream_state_layout(int S, int L, int H, int W, int NC, const edgedict_beam_lm_t* lm,
                                                const edgedict_beam_bias_t* bias = nullptr) {
    BeamStreamState w{};
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t r = o; o += align256(bytes); return r; };
    const size_t LH = (size_t)L * H;
    w.sv.bp_logp = take((size_t)S * W * 8);
    w.sv.bp_node = take((size_t)S * W * 4);
    w.sv.n_bp = take((size_t)S * 4);
    w.sv.bp_h0 = take((size_t)S * W * LH * 4);
    w.sv.bp_c0 = take((size_t)S * W * LH * 4);
    w.sv.nodes = take((size_t)S * NC * 8);
    w.sv.n_nodes = take((size_t)S * 4);
    w.root_tok = take((size_t)S * 4);
    w.n_committed = take((size_t)S * 8);
    w.n_exp = take((size_t)S * 8);
    if (lm) {
        w.lm_bp_h = take((size_t)S * W * lm->L * lm->H * 4);
        w.lm_bp_c = take((size_t)S * W * lm->L * lm->H * 4);
    }
    if (bias) w.bias_bp = take((size_t)S * W * 4);
    w.total = o;
    return w;
}

// LM shallow fusion: the LM step's buffers and the LM state pools, appended behind a search's workspace (offsets from
// `base`, a multiple of 256).  with_bp0: the survivors' buffer [0] lives here too (offline); the streaming search
// keeps it in its persistent state.
struct LmWs {
    size_t pred, h_state, c_state, h_new, c_new, x, G, Hprev, Y0, Y1, Cst, logits, bp_h0, bp_c0, bp_h1, bp_c1, f_h, f_c,
        total;
};
inline LmWs lm_ws_layout(size_t base, const SearchNet& n, const edgedict_beam_lm_t& lm, bool with_bp0) {
    LmWs w;
    size_t o = base;
    auto take = [&](size_t bytes) { size_t r = o; o += align256(bytes); return r; };
    const size_t B = n.B, W = n.W, EM = n.EM, esz = n.esz, H = lm.H, LH = (size_t)lm.L * lm.H;
    w.pred = take(B * 4);
    w.h_state = take(B * LH * 4);
    w.c_state = take(B * LH * 4);
    w.h_new = take(B * LH * 4);
    w.c_new = take(B * LH * 4);
    w.x = take(B * lm.E * esz);
    w.G = take(B * 4 * H * esz);
    w.Hprev = take(B * H * esz);
    w.Y0 = take(B * H * esz);
    w.Y1 = take(B * H * esz);
    w.Cst = take(B * H * 4);
    w.logits = take(B * n.V * 4);
    w.bp_h0 = w.bp_c0 = 0;
    if (with_bp0) {
        w.bp_h0 = take(B * W * LH * 4);
        w.bp_c0 = take(B * W * LH * 4);
    }
    w.bp_h1 = take(B * W * LH * 4);
    w.bp_c1 = take(B * W * LH * 4);
    w.f_h = take(B * EM * LH * 4);
    w.f_c = take(B * EM * LH * 4);
    w.total = o;
    return w;
}

// Contextual biasing: the automaton-state pools, appended behind a search's workspace and the LM's part of it (offsets
// from `base`, a multiple of 256).  with_bp0 as in lm_ws_layout.
struct BiasWs {
    size_t bp0, bp1, f, total;
};
inline BiasWs bias_ws_layout(size_t base, const SearchNet& n, bool with_bp0) {
    BiasWs w{};
    size_t o = base;
    auto take = [&](size_t bytes) { size_t r = o; o += align256(bytes); return r; };
    const size_t B = n.B, W = n.W, EM = n.EM;
    if (with_bp0) w.bp0 = take(B * W * 4);
    w.bp1 = take(B * W * 4);
    w.f = take(B * EM * 4);
    w.total = o;
    return w;
}
// workspace bytes behind the plain layout's `base`: the LM's part, then the bias list's
inline size_t ws_total(size_t base, const SearchNet& n, const edgedict_beam_lm_t* lm, const edgedict_beam_bias_t* bias,
                       bool with_bp0) {
    if (lm) base = lm_ws_layout(base, n, *lm, with_bp0).total;
    if (bias) base = bias_ws_layout(base, n, with_bp0).total;
    return base;
}

// Everything one beam-search call points at: the kernels' bundle, the host-side step buffers, and the LM's
struct BeamBufs {
    BeamPtrs q;
    StepBufs u;                      // prediction-network step + joint
    float *h_state, *c_state;        // [L][B][H] state of the popped hypotheses
    void* node_pred;                 // prefix = 1: the prediction stored per token-tree node (else null)
    const edgedict_beam_lm_t* lm;    // null: no LM
    bool bias;                       // a bias list: the *_bias kernels run
    LstmNet lm_net;
    StepBufs lmu;                    // the LM step's buffers (its symbol and state are q.lm_pred, q.lm_h/c_state)
};
// p / w: workspace and its layout (null: only the state is bound - reset);  st / a: the streams' persistent state (null:
// offline, the survivors live in the workspace);  lm / lw: the LM and its part of the workspace;  bias / bw: the bias
// list and its part
BeamBufs bind_beam_ptrs(char* p, const BeamWs* w, char* st, const BeamStreamState* a, const edgedict_beam_lm_t* lm,
                        const LmWs* lw, const edgedict_beam_bias_t* bias = nullptr, const BiasWs* bw = nullptr) {
    BeamBufs bb{};
    BeamPtrs& q = bb.q;
    bb.bias = bias != nullptr;
    if (bias) {
        q.bias_S = bias->S;
        q.bias_root_next = bias->root_next;
        q.bias_held = bias->held;
        q.bias_pend = bias->pend;
        q.bias_row_ptr = bias->row_ptr;
        q.bias_exc_tok = bias->exc_tok;
        q.bias_exc_next = bias->exc_next;
        q.bias_bp[0] = st ? at<int32_t>(st, a->bias_bp) : at<int32_t>(p, bw->bp0);
        if (p) {
            q.bias_bp[1] = at<int32_t>(p, bw->bp1);
            q.bias_f = at<int32_t>(p, bw->f);
        }
    }
    if (p) {
        bb.u = bind(p, w->step);
        bb.h_state = at<float>(p, w->h_state);
        bb.c_state = at<float>(p, w->c_state);
        if (w->node_pred) bb.node_pred = p + w->node_pred;
        q.pool = at<double>(p, w->pool);
        q.bp_h[1] = at<float>(p, w->bp_h1);
        q.bp_c[1] = at<float>(p, w->bp_c1);
        q.bn_logp = at<double>(p, w->bn_logp);
        q.bn_node = at<int32_t>(p, w->bn_node);
        q.bn_ref = at<int32_t>(p, w->bn_ref);
        q.n_b = at<int32_t>(p, w->n_b);
        q.max_b = at<double>(p, w->max_b);
        q.blk_max = at<double>(p, w->blk_max);
        q.blk_arg = at<int32_t>(p, w->blk_arg);
        q.exp_node = at<int32_t>(p, w->exp_node);
        q.exp_ref = at<int32_t>(p, w->exp_ref);
        q.exp_logp = at<double>(p, w->exp_logp);
        q.e_count = at<int32_t>(p, w->e_count);
        q.f_h = at<float>(p, w->f_h);
        q.f_c = at<float>(p, w->f_c);
        q.open = at<int32_t>(p, w->open);
        q.lens = at<int32_t>(p, w->lens);
        q.flags = at<int32_t>(p, w->flags);
        q.total_exp = at<long long>(p, w->total_exp);
    }
    char* home = st ? st : p;
    const SurvivorOffs& v = st ? a->sv : w->sv;
    q.bp_logp = at<double>(home, v.bp_logp);
    q.bp_node = at<int32_t>(home, v.bp_node);
    q.n_bp = at<int32_t>(home, v.n_bp);
    q.bp_h[0] = at<float>(home, v.bp_h0);
    q.bp_c[0] = at<float>(home, v.bp_c0);
    q.nodes = at<int2>(home, v.nodes);
    q.n_nodes = at<int32_t>(home, v.n_nodes);
    if (st) {       // (offline: the root's token is BOS, nothing is committed, expansions are counted per call only)
        q.root_tok = at<int32_t>(st, a->root_tok);
        q.stream_exp = at<long long>(st, a->n_exp);
        q.n_committed = at<long long>(st, a->n_committed);
    }
    bb.lm = lm;
    if (!lm) return bb;
    bb.lm_net = lm_net_of(*lm);
    q.lm_L = lm->L;
    q.lm_H = lm->H;
    q.lm_bos = lm->bos;
    q.lm_bp_h[0] = st ? at<float>(st, a->lm_bp_h) : at<float>(p, lw->bp_h0);
    q.lm_bp_c[0] = st ? at<float>(st, a->lm_bp_c) : at<float>(p, lw->bp_c0);
    if (!p) return bb;
    q.lm_bp_h[1] = at<float>(p, lw->bp_h1);
    q.lm_bp_c[1] = at<float>(p, lw->bp_c1);
    q.lm_f_h = at<float>(p, lw->f_h);
    q.lm_f_c = at<float>(p, lw->f_c);
    q.lm_pred = at<int32_t>(p, lw->pred);
    q.lm_h_state = at<float>(p, lw->h_state);
    q.lm_c_state = at<float>(p, lw->c_state);
    bb.lmu = StepBufs{nullptr, nullptr, at<float>(p, lw->logits), q.lm_pred, p + lw->x, p + lw->G, p + lw->Hprev,
                      {p + lw->Y0, p + lw->Y1}, at<float>(p, lw->Cst), at<float>(p, lw->h_new), at<float>(p, lw->c_new),
                      nullptr};
    return bb;
}

// an LM that the search can use: status code and message, or ED_OK
int lm_check(const edgedict_beam_lm_t* lm, int V, int prefix, const char* what) {
    if (!lm) return ED_OK;
    ED_CHECK_ARG(!prefix, "%s: prefix = 1 with an LM is not supported (it would need LM log-probs per token-tree node)",
                 what);
    ED_CHECK_ARG(lm->V == V, "%s: the LM's ntoken = %d differs from the transducer's vocabulary V = %d", what, lm->V, V);
    ED_CHECK_ARG(lm->L > 0 && lm->E > 0 && lm->H > 0, "%s: bad LM shape (L %d, E %d, H %d)", what, lm->L, lm->E, lm->H);
    ED_CHECK_ARG(lm->emb && lm->w_ih && lm->w_hh && lm->b_ih && lm->b_hh && lm->Wo && lm->bo, "%s: null LM pointer",
                 what);
    for (int k = 0; k < lm->L; ++k)
        ED_CHECK_ARG(lm->w_ih[k] && lm->w_hh[k] && lm->b_ih[k] && lm->b_hh[k], "%s: null LM layer %d pointer", what, k);
    ED_CHECK_ARG(lm->bos >= 0 && lm->bos < V, "%s: LM bos = %d outside the vocabulary", what, lm->bos);
    ED_CHECK_ARG(lm->emb_dtype == ED_F32 || lm->emb_dtype == ED_BF16, "%s: bad LM embedding dtype", what);
    ED_CHECK_ARG(isfinite(lm->weight) && isfinite(lm->length_bonus), "%s: LM weight / length bonus not finite", what);
    return ED_OK;
}

// a bias list that the search can use: status code and message, or ED_OK (the device tables themselves are trusted)
int bias_check(const edgedict_beam_bias_t* bias, int V, int prefix, const char* what) {
    if (!bias) return ED_OK;
    ED_CHECK_ARG(!prefix, "%s: prefix = 1 with a bias list is not supported (the prefix merge joins hypotheses in "
                          "different automaton states)", what);
    ED_CHECK_ARG(bias->V == V, "%s: the bias list's vocabulary = %d differs from the transducer's V = %d", what, bias->V,
                 V);
    ED_CHECK_ARG(bias->S > 0 && bias->n_exc >= 0, "%s: bad bias automaton (S %d, exceptions %d)", what, bias->S,
                 bias->n_exc);
    ED_CHECK_ARG(bias->root_next && bias->held && bias->pend && bias->row_ptr && bias->exc_tok && bias->exc_next,
                 "%s: null bias table pointer", what);
    return ED_OK;
}

// Sequence.g of the children (models.py:183): this expansion's prediction, kept per token-tree node
void store_pred(const SearchNet& net, const BeamBufs& bb, hipStream_t s) {
    dispatch(net.dtype, [&](auto tag) {
        using T = decltype(tag);
        hipLaunchKernelGGL(beam_store_pred<T>, dim3(net.B), dim3(64), 0, s, bb.q, (const T*)bb.u.dec_new,
                           (T*)bb.node_pred, net.EM, net.NODES, net.P2);
    });
}

// prefix = 1: the host list logic of models.py:145-161, run before every frame after the first.  Host mirrors of the
// survivors and of the token tree are members, so that their storage is reused from frame to frame.
struct PrefixMerge {
    const SearchNet& net;
    const BeamPtrs q;
    const int32_t* lens_host;
    hipStream_t s;
    const void* node_pred;
    int32_t *d_row, *d_node, *d_tok;            // one batch of (utterance, node, token) queries on the device ...
    void *d_pred, *d_D1, *d_hid;                // ... their stored predictions and joint buffers
    float *d_logits, *d_out;
    long long steps = 0;                        // prediction-network steps the reference spends in this branch
    std::vector<int32_t> nbp_h, node_h, nn_h, qrow, qnode, qtok;
    std::vector<double> logp_h;
    std::vector<float> qout;
    // the token tree is APPEND-ONLY (beam_expand writes node n_nodes[b]++ and nothing else): the host keeps a mirror and
    // fetches, per frame, only the node columns that are new since its last fetch - one strided copy of
    // [B] x [min_b mirrored[b], max_b n_nodes[b]) instead of the whole B x NODES tree (O(T^2 EM B) bytes per utterance
    // batch)
    std::vector<int2> nodes_h;
    std::vector<int32_t> mirrored;
    struct Pair { int b, j, i, q0, nq; };
    std::vector<Pair> pairs;
    std::vector<std::vector<int>> paths;        // per list entry: its nodes, last token first

    PrefixMerge(const SearchNet& net_, const BeamBufs& bb, char* p, const BeamWs& w, const int32_t* lens, hipStream_t s_)
        : net(net_), q(bb.q), lens_host(lens), s(s_), node_pred(bb.node_pred), d_row(at<int32_t>(p, w.q_row)),
          d_node(at<int32_t>(p, w.q_node)), d_tok(at<int32_t>(p, w.q_tok)), d_pred(p + w.q_pred), d_D1(p + w.q_D1),
          d_hid(p + w.q_hid), d_logits(at<float>(p, w.q_logits)), d_out(at<float>(p, w.q_out)),
          nodes_h((size_t)net_.B * net_.NODES), mirrored(net_.B, 0), paths(net_.W) {}

    int operator()(int t, const char* e1t) {
        const int B = net.B, W = net.W, NODES = net.NODES;
        nbp_h.resize(B); node_h.resize((size_t)B * W); logp_h.resize((size_t)B * W); nn_h.resize(B);
        ED_CHECK_HIP(hipMemcpyAsync(nbp_h.data(), q.n_bp, (size_t)B * 4, hipMemcpyDeviceToHost, s));
        ED_CHECK_HIP(hipMemcpyAsync(nn_h.data(), q.n_nodes, (size_t)B * 4, hipMemcpyDeviceToHost, s));
        ED_CHECK_HIP(hipStreamSynchronize(s));
        bool any = false;
        for (int b = 0; b < B; ++b) any = any || (t < lens_host[b] && nbp_h[b] > 1);
        if (!any) return ED_OK;
        int lo = NODES, hi = 0;
        for (int b = 0; b < B; ++b) {
            if (nn_h[b] > mirrored[b]) { lo = std::min(lo, mirrored[b]); hi = std::max(hi, nn_h[b]); }
        }
        ED_CHECK_HIP(hipMemcpyAsync(node_h.data(), q.bp_node, node_h.size() * 4, hipMemcpyDeviceToHost, s));
        ED_CHECK_HIP(hipMemcpyAsync(logp_h.data(), q.bp_logp, logp_h.size() * 8, hipMemcpyDeviceToHost, s));
        if (hi > lo)
            ED_CHECK_HIP(hipMemcpy2DAsync(nodes_h.data() + lo, (size_t)NODES * 8, q.nodes + lo, (size_t)NODES * 8,
                                          (size_t)(hi - lo) * 8, (size_t)B, hipMemcpyDeviceToHost, s));
        ED_CHECK_HIP(hipStreamSynchronize(s));
        for (int b = 0; b < B; ++b) mirrored[b] = std::max(mirrored[b], nn_h[b]);
        // every (j, i > j) with A[i] a proper prefix of A[j]: the tokens of A[j] behind A[i], each with the prediction
        // stored at the node before it on A[j]'s path (g; the first one is the prediction of A[i]'s sequence)
        pairs.clear();
        qrow.clear(); qnode.clear(); qtok.clear();
        for (int b = 0; b < B; ++b) {
            if (t >= lens_host[b]) continue;
            const int n = nbp_h[b];
            const int2* nd = nodes_h.data() + (size_t)b * NODES;
            for (int j = 0; j < n; ++j) {
                paths[j].clear();
                for (int x = node_h[(size_t)b * W + j]; x >= 0; x = nd[x].x) paths[j].push_back(x);
            }
            for (int j = 0; j + 1 < n; ++j) {
                const std::vector<int>& pj = paths[j];
                const int lj = (int)pj.size();
                for (int i = j + 1; i < n; ++i) {
                    // isprefix(A[i].k, A[j].k), by VALUE: the same token sequence can sit in the list twice, as two
                    // nodes (a hypothesis that survived as a blank child AND was re-created from its parent)
                    const std::vector<int>& pi = paths[i];
                    const int li = (int)pi.size();
                    if (li >= lj) continue;
                    bool pre = true;
                    for (int d = 0; d < li && pre; ++d) pre = nd[pi[li - 1 - d]].y == nd[pj[lj - 1 - d]].y;
                    if (!pre) continue;
                    Pair pr{b, j, i, (int)qrow.size(), lj - li};
                    for (int d = lj - li - 1; d >= 0; --d) {      // tokens of A[j] behind A[i], in order
                        qrow.push_back(b);
                        qnode.push_back(nd[pj[d]].x);             // g: the prediction stored at the node before it (-1: root)
                        qtok.push_back(nd[pj[d]].y);
                    }
                    pairs.push_back(pr);
                }
            }
        }
        if (pairs.empty()) return ED_OK;
        const int NQ = (int)qrow.size();
        qout.resize(NQ);
        for (int q0 = 0; q0 < NQ; q0 += BEAM_QMAX) {
            const int nq = std::min(BEAM_QMAX, NQ - q0);
            int rc;
            ED_CHECK_HIP(hipMemcpyAsync(d_row, qrow.data() + q0, (size_t)nq * 4, hipMemcpyHostToDevice, s));
            ED_CHECK_HIP(hipMemcpyAsync(d_node, qnode.data() + q0, (size_t)nq * 4, hipMemcpyHostToDevice, s));
            ED_CHECK_HIP(hipMemcpyAsync(d_tok, qtok.data() + q0, (size_t)nq * 4, hipMemcpyHostToDevice, s));
            dispatch(net.dtype, [&](auto tag) {
                using T = decltype(tag);
                hipLaunchKernelGGL(beam_query_gather<T>, dim3(nq), dim3(64), 0, s, (const T*)node_pred, d_row, d_node,
                                   (T*)d_pred, NODES, net.P2);
            });
            if ((rc = edgedict_gemm(net.dtype, net.dtype, d_pred, net.P2, 1, net.W1d, net.ldw1, 1, d_D1, net.J, nq, net.J,
                                    net.P2, net.b1, nullptr, 0, 1, s)))
                return rc;
            dispatch(net.dtype, [&](auto tag) {
                using T = decltype(tag);
                hipLaunchKernelGGL(beam_query_hidden<T>, dim3(nq), dim3(128), 0, s, (const T*)e1t, net.e_row_stride, d_row,
                                   (const T*)d_D1, (T*)d_hid, net.J);
            });
            if ((rc = edgedict_gemm(net.dtype, ED_F32, d_hid, net.J, 1, net.W2, net.J, 1, d_logits, net.V, nq, net.V, net.J,
                                    net.b2, nullptr, 0, 1, s)))
                return rc;
            hipLaunchKernelGGL(beam_query_logp, dim3(nq), dim3(256), 0, s, d_logits, d_tok, d_out, net.V);
            ED_CHECK_HIP(hipMemcpyAsync(qout.data() + q0, d_out, (size_t)nq * 4, hipMemcpyDeviceToHost, s));
            ED_CHECK_HIP(hipStreamSynchronize(s));
        }
        // A[j].logp = log_aplusb(A[j].logp, A[i].logp + sum): j ascending, i ascending; A[i] (i > j) still holds the
        // value it had when the frame began (its own turn as a "j" comes later)
        for (const Pair& pr : pairs) {
            double cur = logp_h[(size_t)pr.b * W + pr.i];
            for (int k = 0; k < pr.nq; ++k) cur += (double)qout[pr.q0 + k];
            double& a = logp_h[(size_t)pr.b * W + pr.j];
            const double hi = a > cur ? a : cur;
            a = hi + log1p(exp(-fabs(a - cur)));
            ++steps;
        }
        ED_CHECK_HIP(hipMemcpyAsync(q.bp_logp, logp_h.data(), logp_h.size() * 8, hipMemcpyHostToDevice, s));
        ED_CHECK_HIP(hipStreamSynchronize(s));       // (logp_h is reused by the next frame)
        return ED_OK;
    }
};

// one LM step for every row: token lm_pred[b] from (lm_h_state, lm_c_state) -> new state, fp32 logits [B, V]
int lm_step(int dtype, int B, const BeamBufs& bb, hipStream_t s) {
    return ed_decode_lm_step(dtype, B, bb.lm_net, bb.q.lm_h_state, bb.q.lm_c_state, bb.lmu, s);
}

// The frame loop shared by the offline search and the streaming one: frames [0, maxlen), utterance b taking part in
// frames t < lens[b]; per frame: frame begin -> lockstep pop / step / expand iterations -> frame end.  The survivors'
// states alternate between bp_h/bp_c[0] and [1], starting in [0]: after the loop utterance b's are in [lens[b] & 1].
// prefix_merge != null (prefix = 1): it runs the host list logic before every frame after the first, and every
// expansion's prediction is kept per node.
// bb.lm != null: every iteration also runs the LM step, and beam_expand_lm replaces beam_expand (no prefix_merge then).
// bb.q.nd_frame != null: beam_pop_detail replaces beam_pop.
// bb.bias: the *_bias instances of those four kernels run instead (no prefix_merge then).
int beam_frame_loop(const SearchNet& net, const BeamBufs& bb, int maxlen, PrefixMerge* prefix_merge, hipStream_t s) {
    const BeamPtrs& q = bb.q;
    const StepBufs& u = bb.u;
    const LstmNet& pn = net.pred;
    const int B = net.B, W = net.W;
    std::vector<int32_t> open_h(B);
    const bool fused_step = ed_decode_fused_ok(net.dtype, pn.emb_dtype, net.J, net.V, pn.E, pn.H, net.P2);
    int cur = 0;
    for (int t = 0; t < maxlen; ++t) {
        const char* e1t = net.frame(t);
        if (prefix_merge && t > 0) {
            const int rc = (*prefix_merge)(t, e1t);
            if (rc) return rc;
        }
        hipLaunchKernelGGL(beam_frame_begin, dim3(B), dim3(64), 0, s, q, t, W, net.EM, net.V);
        for (int it = 0;; ++it) {
            int rc;
            if (bb.bias && q.nd_frame)
                hipLaunchKernelGGL(beam_pop_detail_bias, dim3(B), dim3(256), 0, s, q, cur, W, net.V, net.EM, pn.L, pn.H, B,
                                   net.NODES, net.bos, u.pred, bb.h_state, bb.c_state, t);
            else if (bb.bias)
                hipLaunchKernelGGL(beam_pop_bias, dim3(B), dim3(256), 0, s, q, cur, W, net.V, net.EM, pn.L, pn.H, B,
                                   net.NODES, net.bos, u.pred, bb.h_state, bb.c_state);
            else if (q.nd_frame)
                hipLaunchKernelGGL(beam_pop_detail, dim3(B), dim3(256), 0, s, q, cur, W, net.V, net.EM, pn.L, pn.H, B,
                                   net.NODES, net.bos, u.pred, bb.h_state, bb.c_state, t);
            else
                hipLaunchKernelGGL(beam_pop, dim3(B), dim3(256), 0, s, q, cur, W, net.V, net.EM, pn.L, pn.H, B, net.NODES,
                                   net.bos, u.pred, bb.h_state, bb.c_state);
            // the LM's step on y*'s last token from y*'s LM state (its logits are only read by beam_expand_lm)
            if (bb.lm && (rc = lm_step(net.dtype, B, bb, s))) return rc;
            // prediction-network step on y*'s last token from y*'s state (models.py:164,126-132), then joint(x_t, pred)
            // (models.py:165): 3 + L fused launches (decode_fused.hip), or composed from the general kernels
            if (fused_step) rc = ed_decode_fused_beam_step(net, e1t, bb.h_state, bb.c_state, u, s);
            else rc = composed_lstm_step(net.dtype, B, pn, u.pred, bb.h_state, bb.c_state, u, net.dtype, u.dec_new, s);
            if (rc) return rc;
            if (prefix_merge) store_pred(net, bb, s);
            if (!fused_step && (rc = composed_joint(net, e1t, u.dec_new, u, s))) return rc;
            if (bb.bias && bb.lm)
                hipLaunchKernelGGL(beam_expand_lm_bias, dim3(B), dim3(256), 0, s, q, u.logits, u.h_new, u.c_new,
                                   bb.lmu.logits, bb.lmu.h_new, bb.lmu.c_new, bb.lm->weight, bb.lm->length_bonus, W, net.V,
                                   net.EM, pn.L, pn.H, B, net.blank);
            else if (bb.bias)
                hipLaunchKernelGGL(beam_expand_bias, dim3(B), dim3(256), 0, s, q, u.logits, u.h_new, u.c_new, W, net.V,
                                   net.EM, pn.L, pn.H, B, net.blank);
            else if (bb.lm)
                hipLaunchKernelGGL(beam_expand_lm, dim3(B), dim3(256), 0, s, q, u.logits, u.h_new, u.c_new, bb.lmu.logits,
                                   bb.lmu.h_new, bb.lmu.c_new, bb.lm->weight, bb.lm->length_bonus, W, net.V, net.EM, pn.L,
                                   pn.H, B, net.blank);
            else
                hipLaunchKernelGGL(beam_expand, dim3(B), dim3(256), 0, s, q, u.logits, u.h_new, u.c_new, W, net.V, net.EM,
                                   pn.L, pn.H, B, net.blank);
            if (it + 1 >= W) {   // B cannot hold W hypotheses before W expansions
                ED_CHECK_HIP(hipMemcpyAsync(open_h.data(), q.open, (size_t)B * 4, hipMemcpyDeviceToHost, s));
                ED_CHECK_HIP(hipStreamSynchronize(s));
                int any = 0;
                for (int b = 0; b < B; ++b) any |= open_h[b];
                if (!any) break;
            }
        }
        hipLaunchKernelGGL(beam_frame_end, dim3(B), dim3(256), 0, s, q, t, cur, W, net.EM, pn.L, pn.H);
        cur ^= 1;
    }
    return ED_OK;
}

// Per utterance the tokens of its first survivor (node[b * W], score -logp[b * W]): the token tree (row b of `nodes`,
// `stride` nodes apart) walked from that node to the root.  `what` opens the message of a path beyond max_tokens.
int read_best_path(int B, int W, const int32_t* node, const double* logp, const int2* nodes, size_t stride,
                   const char* what, int32_t* tokens_host, int max_tokens, int32_t* ntokens_host, double* score_host) {
    std::vector<int32_t> rev;
    for (int b = 0; b < B; ++b) {
        rev.clear();
        for (int n = node[(size_t)b * W]; n >= 0; n = nodes[(size_t)b * stride + n].x)
            rev.push_back(nodes[(size_t)b * stride + n].y);
        const int len = (int)rev.size();
        ntokens_host[b] = len;
        ED_CHECK_ARG(len <= max_tokens, "%s of %d tokens exceeds max_tokens = %d", what, len, max_tokens);
        for (int i = 0; i < len; ++i) tokens_host[(size_t)b * max_tokens + i] = rev[len - 1 - i];
        score_host[b] = -logp[(size_t)b * W];
    }
    return ED_OK;
}

// ---- N-best read-out with detail.  One thread per survivor path: depth first, then the tokens, frames and increments
// written root to leaf into the dense result rows [b][j][0, max_tokens).  A path deeper than max_tokens writes its
// length only (the host reports it); a walk never takes more than NODES steps.
struct NBestRes {
    size_t len, tok, frame, lp, total;
};
inline NBestRes nbest_result_layout(size_t B, size_t W, size_t MT) {
    NBestRes r{};
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t x = o; o += align256(bytes); return x; };
    r.len = take(B * W * 4);
    r.tok = take(B * W * MT * 4);
    r.frame = take(B * W * MT * 4);
    r.lp = take(B * W * MT * 8);
    r.total = o;
    return r;
}

__global__ __launch_bounds__(64) void beam_read_paths(BeamPtrs p, int W, int NODES, int MT, int32_t* __restrict__ r_len,
                                                      int32_t* __restrict__ r_tok, int32_t* __restrict__ r_frame,
                                                      double* __restrict__ r_lp) {
    const int b = blockIdx.x;
    const int nb = min(p.n_bp[b], W);
    const int2* tree = p.nodes + (size_t)b * NODES;
    const int32_t* fr = p.nd_frame + (size_t)b * NODES;
    const double* lp = p.nd_logp + (size_t)b * NODES;
    for (int j = threadIdx.x; j < W; j += 64) {
        const size_t row = (size_t)b * W + j;
        if (j >= nb) { r_len[row] = 0; continue; }
        const int leaf = p.bp_node[row];
        int d = 0;
        for (int n = leaf; n >= 0 && n < NODES && d <= NODES; n = tree[n].x) ++d;
        r_len[row] = d;
        if (d > MT) continue;
        int k = d;
        for (int n = leaf; n >= 0 && n < NODES && k > 0; n = tree[n].x) {
            --k;
            r_tok[row * MT + k] = tree[n].y;
            r_frame[row * MT + k] = fr[n];
            r_lp[row * MT + k] = lp[n];
        }
    }
}

// where an N-best read puts its results (all HOST)
struct NBestHost {
    int32_t *tokens, *frames;    // [B][W][max_tokens]
    double* token_logp;          // [B][W][max_tokens]
    int32_t* ntokens;            // [B][W]
    int32_t* nhyp;               // [B]
    double* logp;                // [B][W]
};

// The list B of every utterance from the device: the read-out kernel over the tree q points at, then only the lengths,
// the scores and the used columns of the result cross to the host.
int read_nbest(const BeamPtrs& q, int B, int W, int NODES, int max_tokens, void* result, const NBestHost& o,
               const char* what, hipStream_t s) {
    const NBestRes r = nbest_result_layout(B, W, max_tokens);
    char* rp = (char*)result;
    hipLaunchKernelGGL(beam_read_paths, dim3(B), dim3(64), 0, s, q, W, NODES, max_tokens, at<int32_t>(rp, r.len),
                       at<int32_t>(rp, r.tok), at<int32_t>(rp, r.frame), at<double>(rp, r.lp));
    ED_CHECK_LAUNCH(what);
    ED_CHECK_HIP(hipMemcpyAsync(o.nhyp, q.n_bp, (size_t)B * 4, hipMemcpyDeviceToHost, s));
    ED_CHECK_HIP(hipMemcpyAsync(o.logp, q.bp_logp, (size_t)B * W * 8, hipMemcpyDeviceToHost, s));
    ED_CHECK_HIP(hipMemcpyAsync(o.ntokens, rp + r.len, (size_t)B * W * 4, hipMemcpyDeviceToHost, s));
    ED_CHECK_HIP(hipStreamSynchronize(s));
    int maxlen = 0;
    for (int b = 0; b < B; ++b) {
        o.nhyp[b] = std::min(o.nhyp[b], W);
        for (int j = 0; j < o.nhyp[b]; ++j) {
            const int len = o.ntokens[(size_t)b * W + j];
            ED_CHECK_ARG(len <= max_tokens, "%s of %d tokens exceeds max_tokens = %d", what, len, max_tokens);
            maxlen = std::max(maxlen, len);
        }
    }
    if (maxlen > 0) {
        const size_t MT = (size_t)max_tokens, rows = (size_t)B * W;
        ED_CHECK_HIP(hipMemcpy2DAsync(o.tokens, MT * 4, rp + r.tok, MT * 4, (size_t)maxlen * 4, rows,
                                      hipMemcpyDeviceToHost, s));
        ED_CHECK_HIP(hipMemcpy2DAsync(o.frames, MT * 4, rp + r.frame, MT * 4, (size_t)maxlen * 4, rows,
                                      hipMemcpyDeviceToHost, s));
        ED_CHECK_HIP(hipMemcpy2DAsync(o.token_logp, MT * 8, rp + r.lp, MT * 8, (size_t)maxlen * 8, rows,
                                      hipMemcpyDeviceToHost, s));
        ED_CHECK_HIP(hipStreamSynchronize(s));
    }
    return ED_OK;
}

// the detail per node of the offline search's tree: its own buffer beside the workspace
struct DetailOffs {
    size_t nd_frame, nd_logp, total;
};
inline DetailOffs beam_detail_layout(size_t B, size_t nodes) {
    DetailOffs d{};
    d.nd_frame = 0;
    d.nd_logp = align256(B * nodes * 4);
    d.total = d.nd_logp + align256(B * nodes * 8);
    return d;
}

// what the detail-enabled offline search adds to the plain call
struct NBestOut {
    void* detail;        // device, edgedict_beam_detail_bytes
    void* result;        // device, edgedict_beam_nbest_result_bytes
    NBestHost host;
};
}  // namespace

int ed_decode_lm_check(const edgedict_beam_lm_t* lm, int V, int prefix, const char* what) {
    return lm_check(lm, V, prefix, what);
}
int ed_decode_bias_check(const edgedict_beam_bias_t* bias, int V, int prefix, const char* what) {
    return bias_check(bias, V, prefix, what);
}

extern "C" size_t edgedict_beam_lm_struct_bytes(void) { return sizeof(edgedict_beam_lm_t); }
extern "C" size_t edgedict_beam_bias_struct_bytes(void) { return sizeof(edgedict_beam_bias_t); }

extern "C" size_t edgedict_search_struct_bytes(int which) {
    return which == 0 ? sizeof(edgedict_search_net_t) : which == 1 ? sizeof(edgedict_search_opts_t) : 0;
}

namespace {
// internal-LM estimation and the n-gram LM are the frame-synchronous search's alone: the expansion searches refuse
// them, their size queries return 0
int no_sync_opts(const edgedict_search_opts_t& o, const char* what) {
    ED_CHECK_ARG(!o.ilm_weight, "%s: ilm_weight is not supported (internal-LM estimation is in sync_beam_search)", what);
    ED_CHECK_ARG(!o.ngram, "%s: ngram is not supported (the n-gram LM is fused into sync_beam_search)", what);
    return ED_OK;
}
}  // namespace

extern "C" size_t edgedict_beam_workspace_bytes(const edgedict_search_net_t* pn, int B, int T, int W, int max_expansions,
                                                int prefix, const edgedict_search_opts_t* opts) {
    if (!pn || !search_ptrs_ok(pn, opts)) return 0;
    const edgedict_search_opts_t o = search_opts_of(opts);
    if (o.ilm_weight || o.ngram || B <= 0 || W <= 0 || max_expansions <= 0) return 0;
    const SearchNet n = search_net_of(*pn, nullptr, 0, 0, B, W, max_expansions, 0);
    const size_t base = beam_layout(n, (size_t)(T < 0 ? 0 : T) * n.EM + 1, prefix, false).total;
    return ws_total(base, n, o.lm, o.bias, true);
}

namespace {
// Both offline searches.  nb == null: edgedict_beam_search, B[0] through tokens_host / ntokens_host / score_host;
// else edgedict_beam_search_nbest: the detail is kept per node and the whole list B is read through nb.
int beam_search_run(const edgedict_search_net_t* pn, const void* E1, long long e_row_stride, long long e_frame_stride,
                    int B, int T, const int32_t* lens_host, int W, int max_expansions, int prefix, int32_t* tokens_host,
                    int max_tokens, int32_t* ntokens_host, double* score_host, long long* expansions_host,
                    const edgedict_search_opts_t* opts, void* workspace, const NBestOut* nb, void* stream_) {
    const int EM = max_expansions;
    ED_CHECK_ARG(search_ptrs_ok(pn, opts), "%s: net / opts is not a pointer", nb ? "beam_search_nbest" : "beam_search");
    const edgedict_search_opts_t o = search_opts_of(opts);
    const edgedict_beam_lm_t* lm = o.lm;
    const edgedict_beam_bias_t* bias = o.bias;
    if (int rc = no_sync_opts(o, nb ? "beam_search_nbest" : "beam_search")) return rc;
    ED_CHECK_ARG(!nb || !prefix,
                 "beam_search_nbest: prefix = 1 is not supported (the prefix merge changes a hypothesis' score at frame "
                 "starts, so the per-token increments would no longer add up to it)");
    if (nb) {       // the plain call's outputs are not used: stand-ins for its null-pointer check
        const NBestHost& o = nb->host;
        ED_CHECK_ARG(nb->detail && nb->result && o.tokens && o.frames && o.token_logp && o.ntokens && o.nhyp && o.logp,
                     "beam_search_nbest: null pointer");
        tokens_host = o.tokens; ntokens_host = o.ntokens; score_host = o.logp;
    }
    ED_CHECK_ARG(pn, "beam_search: null pointer");
    const SearchNet net = search_net_of(*pn, E1, e_row_stride, e_frame_stride, B, W, EM, T * EM + 1);
    const int L = net.pred.L, H = net.pred.H, V = net.V;
    if (int rc = check_net(net, "beam_search", T >= 0 && W > 0 && EM >= W && max_tokens >= 0,
                           " (max_expansions must be >= W)",
                           (T == 0 || E1) && lens_host && tokens_host && ntokens_host && score_host && workspace, true))
        return rc;
    int maxlen = 0;
    if (int rc = check_lens(lens_host, B, T, "beam_search", &maxlen)) return rc;
    if (int rc = lm_check(lm, V, prefix, "beam_search")) return rc;
    if (int rc = bias_check(bias, V, prefix, "beam_search")) return rc;
    hipStream_t s = (hipStream_t)stream_;
    char* p = (char*)workspace;
    const BeamWs w = beam_layout(net, (size_t)T * EM + 1, prefix, false);
    LmWs lw{};
    if (lm) lw = lm_ws_layout(w.total, net, *lm, true);
    BiasWs bw{};
    if (bias) bw = bias_ws_layout(ws_total(w.total, net, lm, nullptr, true), net, true);
    BeamBufs bufs = bind_beam_ptrs(p, &w, nullptr, nullptr, lm, &lw, bias, &bw);
    if (nb) {
        const DetailOffs d = beam_detail_layout(B, (size_t)T * EM + 1);
        bufs.q.nd_frame = at<int32_t>((char*)nb->detail, d.nd_frame);
        bufs.q.nd_logp = at<double>((char*)nb->detail, d.nd_logp);
    }
    const BeamPtrs& q = bufs.q;

    const size_t LH = (size_t)L * H;
    ED_CHECK_HIP(hipMemcpyAsync(q.lens, lens_host, (size_t)B * 4, hipMemcpyHostToDevice, s));
    // the empty hypothesis' state is zero (Decoder.forward(empty, None), rnnt/models.py:150-153)
    ED_CHECK_HIP(hipMemsetAsync(q.bp_h[0], 0, (size_t)B * W * LH * 4, s));
    ED_CHECK_HIP(hipMemsetAsync(q.bp_c[0], 0, (size_t)B * W * LH * 4, s));
    // rows of finished / not yet popped utterances flow through the step kernels: keep them finite
    ED_CHECK_HIP(hipMemsetAsync(bufs.h_state, 0, (size_t)B * LH * 4, s));
    ED_CHECK_HIP(hipMemsetAsync(bufs.c_state, 0, (size_t)B * LH * 4, s));
    ED_CHECK_HIP(hipMemsetAsync(bufs.u.pred, 0, (size_t)B * 4, s));
    if (lm) {
        const size_t LHl = (size_t)lm->L * lm->H;
        // the LM's initial state is zero (LMModel.init_hidden, models.py:255-261); idle rows stay finite
        ED_CHECK_HIP(hipMemsetAsync(q.lm_bp_h[0], 0, (size_t)B * W * LHl * 4, s));
        ED_CHECK_HIP(hipMemsetAsync(q.lm_bp_c[0], 0, (size_t)B * W * LHl * 4, s));
        ED_CHECK_HIP(hipMemsetAsync(q.lm_h_state, 0, (size_t)B * LHl * 4, s));
        ED_CHECK_HIP(hipMemsetAsync(q.lm_c_state, 0, (size_t)B * LHl * 4, s));
        ED_CHECK_HIP(hipMemsetAsync(q.lm_pred, 0, (size_t)B * 4, s));
    }
    hipLaunchKernelGGL(beam_init, dim3((B + 63) / 64), dim3(64), 0, s, q, B, W);
    std::optional<PrefixMerge> merge;
    if (prefix) merge.emplace(net, bufs, p, w, lens_host, s);
    if (int rc = beam_frame_loop(net, bufs, maxlen, merge ? &*merge : nullptr, s)) return rc;
    ED_CHECK_LAUNCH("beam_search");
    const int NODES = net.NODES;
    if (nb) {       // results: the whole list B of the last frame, its paths walked on the device
        int32_t flags[2];
        long long total = 0;
        ED_CHECK_HIP(hipMemcpyAsync(flags, q.flags, 8, hipMemcpyDeviceToHost, s));
        ED_CHECK_HIP(hipMemcpyAsync(&total, q.total_exp, 8, hipMemcpyDeviceToHost, s));
        ED_CHECK_HIP(hipStreamSynchronize(s));
        ED_CHECK_ARG(!flags[0], "beam_search: an utterance needed more than max_expansions = %d expansions in one frame",
                     EM);
        ED_CHECK_ARG(!flags[1], "beam_search: token tree overflow");
        if (expansions_host) *expansions_host = total;
        return read_nbest(q, B, W, NODES, max_tokens, nb->result, nb->host, "beam_search: hypothesis", s);
    }
    // results: B[0] of the last frame (models.py:201-202), token tree walked on the host
    std::vector<double> logp((size_t)B * W);
    std::vector<int32_t> node((size_t)B * W), nn(B);
    std::vector<int2> nodes((size_t)B * NODES);
    int32_t flags[2];
    long long total = 0;
    ED_CHECK_HIP(hipMemcpyAsync(logp.data(), q.bp_logp, logp.size() * 8, hipMemcpyDeviceToHost, s));
    ED_CHECK_HIP(hipMemcpyAsync(node.data(), q.bp_node, node.size() * 4, hipMemcpyDeviceToHost, s));
    ED_CHECK_HIP(hipMemcpyAsync(nn.data(), q.n_nodes, nn.size() * 4, hipMemcpyDeviceToHost, s));
    ED_CHECK_HIP(hipMemcpyAsync(nodes.data(), q.nodes, nodes.size() * 8, hipMemcpyDeviceToHost, s));
    ED_CHECK_HIP(hipMemcpyAsync(flags, q.flags, 8, hipMemcpyDeviceToHost, s));
    ED_CHECK_HIP(hipMemcpyAsync(&total, q.total_exp, 8, hipMemcpyDeviceToHost, s));
    ED_CHECK_HIP(hipStreamSynchronize(s));
    ED_CHECK_ARG(!flags[0], "beam_search: an utterance needed more than max_expansions = %d expansions in one frame", EM);
    ED_CHECK_ARG(!flags[1], "beam_search: token tree overflow");
    if (expansions_host) *expansions_host = total + (merge ? merge->steps : 0);
    return read_best_path(B, W, node.data(), logp.data(), nodes.data(), (size_t)NODES, "beam_search: hypothesis",
                          tokens_host, max_tokens, ntokens_host, score_host);
}
}  // namespace

extern "C" size_t edgedict_beam_detail_bytes(int B, int T, int max_expansions) {
    if (B <= 0 || max_expansions <= 0) return 0;
    return beam_detail_layout(B, (size_t)(T < 0 ? 0 : T) * max_expansions + 1).total;
}

extern "C" size_t edgedict_beam_nbest_result_bytes(int B, int W, int max_tokens) {
    if (B <= 0 || W <= 0 || max_tokens < 0) return 0;
    return nbest_result_layout(B, W, max_tokens).total;
}

extern "C" int edgedict_beam_search_nbest(const edgedict_search_net_t* net, const void* E1, long long e_row_stride,
                                          long long e_frame_stride, int B, int T, const int32_t* lens_host, int W,
                                          int max_expansions, int prefix, int32_t* tokens_host, int32_t* frames_host,
                                          double* token_logp_host, int max_tokens, int32_t* ntokens_host,
                                          int32_t* nhyp_host, double* logp_host, long long* expansions_host,
                                          const edgedict_search_opts_t* opts, void* workspace, void* detail, void* result,
                                          void* stream_) {
    const NBestOut nb{detail, result, {tokens_host, frames_host, token_logp_host, ntokens_host, nhyp_host, logp_host}};
    return beam_search_run(net, E1, e_row_stride, e_frame_stride, B, T, lens_host, W, max_expansions, prefix, nullptr,
                           max_tokens, nullptr, nullptr, expansions_host, opts, workspace, &nb, stream_);
}

extern "C" int edgedict_beam_search(const edgedict_search_net_t* net, const void* E1, long long e_row_stride,
                                    long long e_frame_stride, int B, int T, const int32_t* lens_host, int W,
                                    int max_expansions, int prefix, int32_t* tokens_host, int max_tokens,
                                    int32_t* ntokens_host, double* score_host, long long* expansions_host,
                                    const edgedict_search_opts_t* opts, void* workspace, void* stream_) {
    return beam_search_run(net, E1, e_row_stride, e_frame_stride, B, T, lens_host, W, max_expansions, prefix, tokens_host,
                           max_tokens, ntokens_host, score_host, expansions_host, opts, workspace, nullptr, stream_);
}


// =====================================================================================
// Streaming beam search: the frame loop above over a persistent per-stream state, so that frames [0, t1) and then
// [t1, t2) give exactly what one offline call over [0, t2) gives (the reference's search is frame-synchronous and
// carries nothing from frame to frame but its list B).  After every advance each stream's token tree is compacted
// (beam_compact): nodes that are no ancestor of a survivor are dropped, the path from the root to the survivors' lowest
// common ancestor moves to the caller's committed log, and that ancestor becomes the new root (node -1, its token kept
// in root_tok).  The tree then holds only the part where the survivors still differ.
// =====================================================================================
namespace {
// streams [b0, b0 + n) with mask[b] != 0 (mask null: all) -> B = [empty hypothesis]: one survivor, logp 0, node -1
// with BOS as its last token, zero prediction-network state; empty tree and committed log
__global__ __launch_bounds__(256) void beam_stream_reset_kernel(BeamPtrs p, long long* n_committed,
                                                                const int32_t* __restrict__ mask, int b0, int W, int L,
                                                                int H, int bos) {
    const int b = b0 + blockIdx.x, tid = threadIdx.x;
    if (mask && !mask[b]) return;
    const size_t n = (size_t)W * L * H;
    float* h = p.bp_h[0] + (size_t)b * n;
    float* c = p.bp_c[0] + (size_t)b * n;
    for (size_t i = tid; i < n; i += 256) { h[i] = 0.f; c[i] = 0.f; }
    if (p.lm_bp_h[0]) {           // the LM's initial state is zero too (LMModel.init_hidden)
        const size_t nl = (size_t)W * p.lm_L * p.lm_H;
        float* lh = p.lm_bp_h[0] + (size_t)b * nl;
        float* lc = p.lm_bp_c[0] + (size_t)b * nl;
        for (size_t i = tid; i < nl; i += 256) { lh[i] = 0.f; lc[i] = 0.f; }
    }
    if (p.bias_bp[0])             // the automaton's root (state 0 of any bias list)
        for (int i = tid; i < W; i += 256) p.bias_bp[0][(size_t)b * W + i] = 0;
    if (tid == 0) {
        p.n_bp[b] = 1;
        p.bp_logp[(size_t)b * W] = 0.0;
        p.bp_node[(size_t)b * W] = -1;
        p.n_nodes[b] = 0;
        p.root_tok[b] = bos;
        n_committed[b] = 0;
        p.stream_exp[b] = 0;
    }
}

// the frame loop leaves the survivors' states of a stream that ran an odd number of frames in bp_h/bp_c[1] (workspace):
// move them home
__global__ __launch_bounds__(256) void beam_stream_settle(BeamPtrs p, int W, int L, int H) {
    const int b = blockIdx.x, tid = threadIdx.x;
    if (!(p.lens[b] & 1)) return;
    const size_t LH = (size_t)L * H, n = (size_t)p.n_bp[b] * LH, o = (size_t)b * W * LH;
    for (size_t i = tid; i < n; i += 256) {
        p.bp_h[0][o + i] = p.bp_h[1][o + i];
        p.bp_c[0][o + i] = p.bp_c[1][o + i];
    }
    if (p.lm_pred) {
        const size_t LHl = (size_t)p.lm_L * p.lm_H, nl = (size_t)p.n_bp[b] * LHl, ol = (size_t)b * W * LHl;
        for (size_t i = tid; i < nl; i += 256) {
            p.lm_bp_h[0][ol + i] = p.lm_bp_h[1][ol + i];
            p.lm_bp_c[0][ol + i] = p.lm_bp_c[1][ol + i];
        }
    }
    if (p.bias_f)
        for (int i = tid; i < p.n_bp[b]; i += 256) p.bias_bp[0][(size_t)b * W + i] = p.bias_bp[1][(size_t)b * W + i];
}

constexpr int BEAM_COMPACT_LDS_NODES = 4096;    // trees up to this capacity walk their parent links in LDS (32 KiB)

// One workgroup per stream that ran frames in this advance.
//  1. the old tree is copied aside (c_old) and the parent links staged in LDS when they fit;
//  2. one thread marks the ancestors of the survivors, survivor by survivor; a walk stops at the first node already
//     marked (or the root), so the whole pass touches every live node once.  Node ids grow from parent to child, and
//     the union of the walks so far is the chain root .. LCA plus branches below the LCA (ids > LCA), so a walk that
//     stops at a node with id <= the current LCA stopped ON the chain, at the new LCA: LCA = min(node of survivor 0,
//     stop node of every later walk), by node identity;
//  3. the path root .. LCA is appended to the committed log (commit[b][0, n_commit[b])) and the LCA becomes the root;
//  4. the nodes below the LCA that are marked are renumbered by an exclusive scan (order kept, so parents still precede
//     their children), written back with rewritten parent links, and the survivors' node ids remapped.
// DETAIL: the nodes' frames and increments (p.nd_frame / p.nd_logp) move with them - copied aside with the old tree,
// written back under the new ids, and those of the path root .. LCA written next to its tokens - and the stream's count
// of frames done grows by this advance's frames.
struct CompactDetail {
    int32_t* old_frame;      // [S][NC] scratch
    double* old_logp;
    int32_t* commit_frame;   // [S][NC] beside commit
    double* commit_logp;
    long long* frames_done;  // [S] (state)
};
template <bool DETAIL>
__device__ __forceinline__ void beam_compact_body(BeamPtrs& p, int W, int NC, int use_lds, int2* __restrict__ c_old,
                                                  int32_t* __restrict__ c_mark, int32_t* __restrict__ commit,
                                                  int32_t* __restrict__ n_commit, long long* __restrict__ n_committed,
                                                  const CompactDetail& cd) {
    const int b = blockIdx.x, tid = threadIdx.x;
    extern __shared__ int s_dyn[];
    __shared__ int s_scan[256];
    __shared__ int s_lca;
    if (p.lens[b] <= 0) {
        if (tid == 0) n_commit[b] = 0;
        return;
    }
    const int nn = p.n_nodes[b];
    int2* old = c_old + (size_t)b * NC;
    int2* tree = p.nodes + (size_t)b * NC;
    int* mark = use_lds ? s_dyn : c_mark + (size_t)b * NC;
    int* spar = use_lds ? s_dyn + NC : nullptr;
    for (int i = tid; i < nn; i += 256) {
        const int2 v = tree[i];
        old[i] = v;
        mark[i] = 0;
        if (use_lds) spar[i] = v.x;
        if constexpr (DETAIL) {
            cd.old_frame[(size_t)b * NC + i] = p.nd_frame[(size_t)b * NC + i];
            cd.old_logp[(size_t)b * NC + i] = p.nd_logp[(size_t)b * NC + i];
        }
    }
    __syncthreads();
    const int nb = p.n_bp[b];
    if (tid == 0) {
        int lca = p.bp_node[(size_t)b * W];
        for (int j = 0; j < nb; ++j) {
            int x = p.bp_node[(size_t)b * W + j];
            while (x >= 0 && !mark[x]) {
                mark[x] = 1;
                x = use_lds ? spar[x] : old[x].x;
            }
            if (j > 0) lca = min(lca, x);
        }
        // the committed tokens: root .. LCA, written last to first
        int d = 0;
        for (int x = lca; x >= 0; x = use_lds ? spar[x] : old[x].x) ++d;
        int k = d;
        for (int x = lca; x >= 0; x = use_lds ? spar[x] : old[x].x) {
            commit[(size_t)b * NC + --k] = old[x].y;
            if constexpr (DETAIL) {
                cd.commit_frame[(size_t)b * NC + k] = cd.old_frame[(size_t)b * NC + x];
                cd.commit_logp[(size_t)b * NC + k] = cd.old_logp[(size_t)b * NC + x];
            }
        }
        if constexpr (DETAIL) cd.frames_done[b] += p.lens[b];
        n_commit[b] = d;
        n_committed[b] += d;
        if (lca >= 0) p.root_tok[b] = old[lca].y;
        s_lca = lca;
    }
    __syncthreads();
    const int lca = s_lca;
    // exclusive scan of keep[i] = mark[i] && i > lca over contiguous per-thread ranges
    const int per = (nn + 255) / 256, lo = min(nn, tid * per), hi = min(nn, lo + per);
    int cnt = 0;
    for (int i = lo; i < hi; ++i) cnt += (mark[i] && i > lca) ? 1 : 0;
    s_scan[tid] = cnt;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        const int v = tid >= off ? s_scan[tid - off] : 0;
        __syncthreads();
        s_scan[tid] += v;
        __syncthreads();
    }
    int k = s_scan[tid] - cnt;
    const int kept = s_scan[255];
    for (int i = lo; i < hi; ++i) mark[i] = (mark[i] && i > lca) ? k++ : -1;     // mark -> new id (-1: dropped)
    __syncthreads();
    for (int i = tid; i < nn; i += 256) {
        const int ni = mark[i];
        if (ni < 0) continue;
        const int2 v = old[i];
        tree[ni] = make_int2(v.x == lca ? -1 : mark[v.x], v.y);
        if constexpr (DETAIL) {
            p.nd_frame[(size_t)b * NC + ni] = cd.old_frame[(size_t)b * NC + i];
            p.nd_logp[(size_t)b * NC + ni] = cd.old_logp[(size_t)b * NC + i];
        }
    }
    if (tid < nb) {
        const int x = p.bp_node[(size_t)b * W + tid];
        p.bp_node[(size_t)b * W + tid] = x == lca ? -1 : mark[x];
    }
    if (tid == 0) p.n_nodes[b] = kept;
}

__global__ __launch_bounds__(256) void beam_compact(BeamPtrs p, int W, int NC, int use_lds, int2* __restrict__ c_old,
                                                    int32_t* __restrict__ c_mark, int32_t* __restrict__ commit,
                                                    int32_t* __restrict__ n_commit, long long* __restrict__ n_committed) {
    beam_compact_body<false>(p, W, NC, use_lds, c_old, c_mark, commit, n_commit, n_committed, CompactDetail{});
}

__global__ __launch_bounds__(256) void beam_compact_detail(BeamPtrs p, int W, int NC, int use_lds,
                                                           int2* __restrict__ c_old, int32_t* __restrict__ c_mark,
                                                           int32_t* __restrict__ commit, int32_t* __restrict__ n_commit,
                                                           long long* __restrict__ n_committed, CompactDetail cd) {
    beam_compact_body<true>(p, W, NC, use_lds, c_old, c_mark, commit, n_commit, n_committed, cd);
}

// the detail-enabled streams' count of frames done -> 0, for streams [b0, b0 + n) with mask[b] != 0 (mask null: all)
__global__ void beam_detail_reset_kernel(long long* __restrict__ frames_done, const int32_t* __restrict__ mask, int b0,
                                         int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (mask && !mask[b0 + i]) return;
    frames_done[b0 + i] = 0;
}

// detail of the streams' trees: persistent (beside the state) and per call (beside the workspace)
struct StreamDetailState {
    size_t nd_frame, nd_logp, frames_done, total;
};
inline StreamDetailState stream_detail_state_layout(size_t S, size_t NC) {
    StreamDetailState d{};
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t r = o; o += align256(bytes); return r; };
    d.nd_frame = take(S * NC * 4);
    d.nd_logp = take(S * NC * 8);
    d.frames_done = take(S * 8);
    d.total = o;
    return d;
}
struct StreamDetailWs {
    size_t old_frame, old_logp, commit_frame, commit_logp, total;
};
inline StreamDetailWs stream_detail_ws_layout(size_t S, size_t NC) {
    StreamDetailWs d{};
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t r = o; o += align256(bytes); return r; };
    d.old_frame = take(S * NC * 4);
    d.old_logp = take(S * NC * 8);
    d.commit_frame = take(S * NC * 4);
    d.commit_logp = take(S * NC * 8);
    d.total = o;
    return d;
}
void bind_stream_detail(BeamPtrs& q, char* dstate, int S, int NC) {
    const StreamDetailState d = stream_detail_state_layout(S, NC);
    q.nd_frame = at<int32_t>(dstate, d.nd_frame);
    q.nd_logp = at<double>(dstate, d.nd_logp);
    q.frames_done = at<long long>(dstate, d.frames_done);
}

// what the detail-enabled advance adds to the plain call
struct StreamDetailArgs {
    void* dstate;                    // device, edgedict_beam_stream_detail_state_bytes
    void* dws;                       // device, edgedict_beam_stream_detail_workspace_bytes
    int32_t* commit_frame_host;      // HOST [S, node_capacity]
    double* commit_logp_host;        // HOST [S, node_capacity]
};

}  // namespace

extern "C" size_t edgedict_beam_stream_state_bytes(const edgedict_search_opts_t* opts, int S, int L, int H, int W,
                                                   int node_capacity) {
    if (!search_ptrs_ok(nullptr, opts)) return 0;
    const edgedict_search_opts_t o = search_opts_of(opts);
    if (o.ilm_weight || o.ngram || S <= 0 || W <= 0 || L <= 0 || H <= 0 || node_capacity <= 0) return 0;
    return beam_stream_state_layout(S, L, H, W, node_capacity, o.lm, o.bias).total;
}

extern "C" size_t edgedict_beam_stream_workspace_bytes(const edgedict_search_net_t* pn, int S, int W, int max_expansions,
                                                       int node_capacity, const edgedict_search_opts_t* opts) {
    if (!pn || !search_ptrs_ok(pn, opts)) return 0;
    const edgedict_search_opts_t o = search_opts_of(opts);
    if (o.ilm_weight || o.ngram || S <= 0 || W <= 0 || max_expansions <= 0 || node_capacity <= 0) return 0;
    const SearchNet n = search_net_of(*pn, nullptr, 0, 0, S, W, max_expansions, 0);
    const size_t base = beam_layout(n, (size_t)node_capacity, 0, true).total;
    return ws_total(base, n, o.lm, o.bias, false);
}

// opts->bias: only its presence matters here (the state then holds the survivors' automaton states; the root is state
// 0).  detail_state non-null: the selected streams' frame count -> 0 as well.
extern "C" int edgedict_beam_stream_reset(const edgedict_search_opts_t* opts, int S, int L, int H, int W,
                                          int node_capacity, int bos, const int32_t* mask, int mask_on_host, void* state,
                                          void* detail_state, void* stream_) {
    ED_CHECK_ARG(search_ptrs_ok(nullptr, opts), "beam_stream_reset: opts is not a pointer");
    const edgedict_search_opts_t o = search_opts_of(opts);
    const edgedict_beam_lm_t* lm = o.lm;
    const edgedict_beam_bias_t* bias = o.bias;
    if (int rc = no_sync_opts(o, "beam_stream_reset")) return rc;
    ED_CHECK_ARG(S > 0 && L > 0 && H > 0 && W > 0 && node_capacity > 0, "beam_stream_reset: bad shape");
    ED_CHECK_ARG(state, "beam_stream_reset: null state");
    ED_CHECK_ARG(!lm || (lm->L > 0 && lm->H > 0), "beam_stream_reset: bad LM shape");
    hipStream_t s = (hipStream_t)stream_;
    const BeamStreamState a = beam_stream_state_layout(S, L, H, W, node_capacity, lm, bias);
    char* st = (char*)state;
    const BeamPtrs q = bind_beam_ptrs(nullptr, nullptr, st, &a, lm, nullptr, bias, nullptr).q;
    long long* n_committed = at<long long>(st, a.n_committed);
    if (!mask || !mask_on_host) {
        hipLaunchKernelGGL(beam_stream_reset_kernel, dim3(S), dim3(256), 0, s, q, n_committed, mask, 0, W, L, H, bos);
    } else {            // host mask: one launch per run of selected streams
        for (int b = 0; b < S;) {
            if (!mask[b]) { ++b; continue; }
            int e = b;
            while (e < S && mask[e]) ++e;
            hipLaunchKernelGGL(beam_stream_reset_kernel, dim3(e - b), dim3(256), 0, s, q, n_committed,
                               (const int32_t*)nullptr, b, W, L, H, bos);
            b = e;
        }
    }
    ED_CHECK_LAUNCH("beam_stream_reset");
    if (!detail_state) return ED_OK;
    long long* fd = at<long long>((char*)detail_state, stream_detail_state_layout(S, node_capacity).frames_done);
    if (!mask || !mask_on_host) {
        hipLaunchKernelGGL(beam_detail_reset_kernel, dim3((S + 63) / 64), dim3(64), 0, s, fd, mask, 0, S);
    } else {
        for (int b = 0; b < S;) {
            if (!mask[b]) { ++b; continue; }
            int e = b;
            while (e < S && mask[e]) ++e;
            hipLaunchKernelGGL(beam_detail_reset_kernel, dim3((e - b + 63) / 64), dim3(64), 0, s, fd,
                               (const int32_t*)nullptr, b, e - b);
            b = e;
        }
    }
    ED_CHECK_LAUNCH("beam_stream_reset_detail");
    return ED_OK;
}

// The four detail arguments all null: the plain advance; all non-null: the detail is kept and committed too.
extern "C" int edgedict_beam_stream_advance(const edgedict_search_net_t* pn, const void* E1, long long e_row_stride,
                                            long long e_frame_stride, int S, const int32_t* n_frames_host, int W,
                                            int max_expansions, int node_capacity, int32_t* commit_host,
                                            int32_t* ncommit_host, long long* expansions_host,
                                            const edgedict_search_opts_t* opts, void* state, void* workspace,
                                            void* detail_state, void* detail_workspace, int32_t* commit_frame_host,
                                            double* commit_logp_host, void* stream_) {
    const int EM = max_expansions, NC = node_capacity;
    ED_CHECK_ARG(search_ptrs_ok(pn, opts), "beam_stream_advance: net / opts is not a pointer");
    const edgedict_search_opts_t o = search_opts_of(opts);
    const edgedict_beam_lm_t* lm = o.lm;
    const edgedict_beam_bias_t* bias = o.bias;
    if (int rc = no_sync_opts(o, "beam_stream_advance")) return rc;
    const StreamDetailArgs detail{detail_state, detail_workspace, commit_frame_host, commit_logp_host};
    const bool any_detail = detail_state || detail_workspace || commit_frame_host || commit_logp_host;
    const StreamDetailArgs* dt = any_detail ? &detail : nullptr;
    ED_CHECK_ARG(!dt || (dt->dstate && dt->dws && dt->commit_frame_host && dt->commit_logp_host),
                 "beam_stream_advance_detail: null pointer");
    ED_CHECK_ARG(pn, "beam_stream_advance: null pointer");
    const SearchNet net = search_net_of(*pn, E1, e_row_stride, e_frame_stride, S, W, EM, NC);
    const int L = net.pred.L, H = net.pred.H, V = net.V;
    if (int rc = check_net(net, "beam_stream_advance", W > 0 && EM >= W && NC > 0, " (max_expansions must be >= W)",
                           n_frames_host && commit_host && ncommit_host && state && workspace, true))
        return rc;
    if (int rc = lm_check(lm, V, 0, "beam_stream_advance")) return rc;
    if (int rc = bias_check(bias, V, 0, "beam_stream_advance")) return rc;
    int maxlen = 0;
    for (int b = 0; b < S; ++b) {
        ED_CHECK_ARG(n_frames_host[b] >= 0, "beam_stream_advance: n_frames[%d] = %d < 0", b, n_frames_host[b]);
        maxlen = std::max(maxlen, n_frames_host[b]);
    }
    ED_CHECK_ARG(maxlen == 0 || E1, "beam_stream_advance: null E1");
    hipStream_t s = (hipStream_t)stream_;
    const BeamStreamState a = beam_stream_state_layout(S, L, H, W, NC, lm, bias);
    const BeamWs w = beam_layout(net, (size_t)NC, 0, true);
    char* st = (char*)state;
    char* p = (char*)workspace;
    LmWs lw{};
    if (lm) lw = lm_ws_layout(w.total, net, *lm, false);
    BiasWs bw{};
    if (bias) bw = bias_ws_layout(ws_total(w.total, net, lm, nullptr, false), net, false);
    BeamBufs bufs = bind_beam_ptrs(p, &w, st, &a, lm, &lw, bias, &bw);
    if (dt) bind_stream_detail(bufs.q, (char*)dt->dstate, S, NC);
    const BeamPtrs& q = bufs.q;
    for (int b = 0; b < S; ++b) ncommit_host[b] = 0;
    if (expansions_host) *expansions_host = 0;
    if (maxlen == 0) return ED_OK;

    // every node a pop can create must fit: checked before anything runs, so an error leaves the state as it was
    std::vector<int32_t> nn(S);
    ED_CHECK_HIP(hipMemcpyAsync(nn.data(), q.n_nodes, (size_t)S * 4, hipMemcpyDeviceToHost, s));
    ED_CHECK_HIP(hipStreamSynchronize(s));
    for (int b = 0; b < S; ++b) {
        const long long need = (long long)nn[b] + (long long)n_frames_host[b] * EM;
        ED_CHECK_ARG(n_frames_host[b] == 0 || need <= NC,
                     "beam_stream_advance: stream %d may need %lld token-tree nodes (%d live + %d frames x "
                     "max_expansions %d) but node_capacity = %d",
                     b, need, nn[b], n_frames_host[b], EM, NC);
    }

    const size_t LH = (size_t)L * H;
    ED_CHECK_HIP(hipMemcpyAsync(q.lens, n_frames_host, (size_t)S * 4, hipMemcpyHostToDevice, s));
    // rows of finished / not yet popped streams flow through the step kernels: keep them finite
    ED_CHECK_HIP(hipMemsetAsync(bufs.h_state, 0, (size_t)S * LH * 4, s));
    ED_CHECK_HIP(hipMemsetAsync(bufs.c_state, 0, (size_t)S * LH * 4, s));
    ED_CHECK_HIP(hipMemsetAsync(bufs.u.pred, 0, (size_t)S * 4, s));
    if (lm) {
        const size_t LHl = (size_t)lm->L * lm->H;
        ED_CHECK_HIP(hipMemsetAsync(q.lm_h_state, 0, (size_t)S * LHl * 4, s));
        ED_CHECK_HIP(hipMemsetAsync(q.lm_c_state, 0, (size_t)S * LHl * 4, s));
        ED_CHECK_HIP(hipMemsetAsync(q.lm_pred, 0, (size_t)S * 4, s));
    }
    ED_CHECK_HIP(hipMemsetAsync(q.flags, 0, 8, s));
    ED_CHECK_HIP(hipMemsetAsync(q.total_exp, 0, 8, s));
    if (int rc = beam_frame_loop(net, bufs, maxlen, nullptr, s)) return rc;
    hipLaunchKernelGGL(beam_stream_settle, dim3(S), dim3(256), 0, s, q, W, L, H);
    const int use_lds = NC <= BEAM_COMPACT_LDS_NODES;
    int32_t* commit = at<int32_t>(p, w.commit);
    int32_t* n_commit = at<int32_t>(p, w.n_commit);
    CompactDetail cd{};
    if (dt) {
        const StreamDetailWs dw = stream_detail_ws_layout(S, NC);
        char* dp = (char*)dt->dws;
        cd = CompactDetail{at<int32_t>(dp, dw.old_frame), at<double>(dp, dw.old_logp), at<int32_t>(dp, dw.commit_frame),
                           at<double>(dp, dw.commit_logp),
                           at<long long>((char*)dt->dstate, stream_detail_state_layout(S, NC).frames_done)};
        hipLaunchKernelGGL(beam_compact_detail, dim3(S), dim3(256), use_lds ? (size_t)NC * 8 : 0, s, q, W, NC, use_lds,
                           at<int2>(p, w.c_old), at<int32_t>(p, w.c_mark), commit, n_commit,
                           at<long long>(st, a.n_committed), cd);
    } else {
        hipLaunchKernelGGL(beam_compact, dim3(S), dim3(256), use_lds ? (size_t)NC * 8 : 0, s, q, W, NC, use_lds,
                           at<int2>(p, w.c_old), at<int32_t>(p, w.c_mark), commit, n_commit,
                           at<long long>(st, a.n_committed));
    }
    ED_CHECK_LAUNCH("beam_stream_advance");
    int32_t flags[2];
    long long total = 0;
    ED_CHECK_HIP(hipMemcpyAsync(flags, q.flags, 8, hipMemcpyDeviceToHost, s));
    ED_CHECK_HIP(hipMemcpyAsync(&total, q.total_exp, 8, hipMemcpyDeviceToHost, s));
    ED_CHECK_HIP(hipMemcpyAsync(ncommit_host, n_commit, (size_t)S * 4, hipMemcpyDeviceToHost, s));
    ED_CHECK_HIP(hipStreamSynchronize(s));
    ED_CHECK_ARG(!flags[0], "beam_stream_advance: a stream needed more than max_expansions = %d expansions in one frame",
                 EM);
    ED_CHECK_ARG(!flags[1], "beam_stream_advance: token tree overflow (node_capacity = %d)", NC);
    if (expansions_host) *expansions_host = total;
    int maxc = 0;
    for (int b = 0; b < S; ++b) maxc = std::max(maxc, ncommit_host[b]);
    if (maxc > 0) {
        ED_CHECK_HIP(hipMemcpy2DAsync(commit_host, (size_t)NC * 4, commit, (size_t)NC * 4, (size_t)maxc * 4, (size_t)S,
                                      hipMemcpyDeviceToHost, s));
        if (dt) {
            ED_CHECK_HIP(hipMemcpy2DAsync(dt->commit_frame_host, (size_t)NC * 4, cd.commit_frame, (size_t)NC * 4,
                                          (size_t)maxc * 4, (size_t)S, hipMemcpyDeviceToHost, s));
            ED_CHECK_HIP(hipMemcpy2DAsync(dt->commit_logp_host, (size_t)NC * 8, cd.commit_logp, (size_t)NC * 8,
                                          (size_t)maxc * 8, (size_t)S, hipMemcpyDeviceToHost, s));
        }
        ED_CHECK_HIP(hipStreamSynchronize(s));
    }
    return ED_OK;
}

extern "C" size_t edgedict_beam_stream_detail_state_bytes(int S, int node_capacity) {
    if (S <= 0 || node_capacity <= 0) return 0;
    return stream_detail_state_layout(S, node_capacity).total;
}

extern "C" size_t edgedict_beam_stream_detail_workspace_bytes(int S, int node_capacity) {
    if (S <= 0 || node_capacity <= 0) return 0;
    return stream_detail_ws_layout(S, node_capacity).total;
}

extern "C" int edgedict_beam_stream_read(int S, int L, int H, int W, int node_capacity, const void* state,
                                         int32_t* tokens_host, int max_tokens, int32_t* ntokens_host,
                                         double* score_host, long long* ncommitted_host, long long* expansions_host,
                                         void* stream_) {
    ED_CHECK_ARG(S > 0 && L > 0 && H > 0 && W > 0 && node_capacity > 0 && max_tokens >= 0,
                 "beam_stream_read: bad shape");
    ED_CHECK_ARG(state && tokens_host && ntokens_host && score_host, "beam_stream_read: null pointer");
    hipStream_t s = (hipStream_t)stream_;
    const int NC = node_capacity;
    const BeamStreamState a = beam_stream_state_layout(S, L, H, W, NC, nullptr);
    const char* st = (const char*)state;
    std::vector<double> logp((size_t)S * W);
    std::vector<int32_t> node((size_t)S * W), nn(S);
    std::vector<long long> ncom(S), nexp(S);
    ED_CHECK_HIP(hipMemcpyAsync(logp.data(), st + a.sv.bp_logp, logp.size() * 8, hipMemcpyDeviceToHost, s));
    ED_CHECK_HIP(hipMemcpyAsync(node.data(), st + a.sv.bp_node, node.size() * 4, hipMemcpyDeviceToHost, s));
    ED_CHECK_HIP(hipMemcpyAsync(nn.data(), st + a.sv.n_nodes, nn.size() * 4, hipMemcpyDeviceToHost, s));
    ED_CHECK_HIP(hipMemcpyAsync(ncom.data(), st + a.n_committed, ncom.size() * 8, hipMemcpyDeviceToHost, s));
    ED_CHECK_HIP(hipMemcpyAsync(nexp.data(), st + a.n_exp, nexp.size() * 8, hipMemcpyDeviceToHost, s));
    ED_CHECK_HIP(hipStreamSynchronize(s));
    int maxnn = 0;
    for (int b = 0; b < S; ++b) maxnn = std::max(maxnn, nn[b]);
    std::vector<int2> nodes((size_t)S * std::max(maxnn, 1));
    if (maxnn > 0) {
        ED_CHECK_HIP(hipMemcpy2DAsync(nodes.data(), (size_t)maxnn * 8, st + a.sv.nodes, (size_t)NC * 8, (size_t)maxnn * 8,
                                      (size_t)S, hipMemcpyDeviceToHost, s));
        ED_CHECK_HIP(hipStreamSynchronize(s));
    }
    for (int b = 0; b < S; ++b) {
        if (ncommitted_host) ncommitted_host[b] = ncom[b];
        if (expansions_host) expansions_host[b] = nexp[b];
    }
    return read_best_path(S, W, node.data(), logp.data(), nodes.data(), (size_t)maxnn, "beam_stream_read: hypothesis tail",
                          tokens_host, max_tokens, ntokens_host, score_host);
}

extern "C" int edgedict_beam_stream_read_nbest(int S, int L, int H, int W, int node_capacity, const void* state,
                                               const void* detail_state, void* result, int32_t* tokens_host,
                                               int32_t* frames_host, double* token_logp_host, int max_tokens,
                                               int32_t* ntokens_host, int32_t* nhyp_host, double* logp_host,
                                               long long* ncommitted_host, long long* expansions_host,
                                               long long* frames_done_host, void* stream_) {
    ED_CHECK_ARG(S > 0 && L > 0 && H > 0 && W > 0 && node_capacity > 0 && max_tokens >= 0,
                 "beam_stream_read_nbest: bad shape");
    ED_CHECK_ARG(state && detail_state && result && tokens_host && frames_host && token_logp_host && ntokens_host &&
                     nhyp_host && logp_host,
                 "beam_stream_read_nbest: null pointer");
    hipStream_t s = (hipStream_t)stream_;
    const int NC = node_capacity;
    const BeamStreamState a = beam_stream_state_layout(S, L, H, W, NC, nullptr);
    BeamPtrs q = bind_beam_ptrs(nullptr, nullptr, (char*)state, &a, nullptr, nullptr).q;
    bind_stream_detail(q, (char*)detail_state, S, NC);
    if (ncommitted_host)
        ED_CHECK_HIP(hipMemcpyAsync(ncommitted_host, q.n_committed, (size_t)S * 8, hipMemcpyDeviceToHost, s));
    if (expansions_host)
        ED_CHECK_HIP(hipMemcpyAsync(expansions_host, q.stream_exp, (size_t)S * 8, hipMemcpyDeviceToHost, s));
    if (frames_done_host)
        ED_CHECK_HIP(hipMemcpyAsync(frames_done_host, q.frames_done, (size_t)S * 8, hipMemcpyDeviceToHost, s));
    const NBestHost o{tokens_host, frames_host, token_logp_host, ntokens_host, nhyp_host, logp_host};
    return read_nbest(q, S, W, NC, max_tokens, result, o, "beam_stream_read_nbest: hypothesis tail", s);
}
