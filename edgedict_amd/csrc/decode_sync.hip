// Frame-synchronous batched RNN-T beam search for gfx950 ("modified beam search": every hypothesis emits at most one
// symbol per frame, the rule of the greedy search), beside the best-first search of decode.hip.
//
// All B x W hypotheses of a batch are rows of ONE prediction-network step and ONE joint per frame: row b * W + i is
// hypothesis i of utterance b.  A row carries its last token and the prediction-network state from BEFORE that token was
// consumed, as the best-first search's hypotheses do, so a frame reuses that search's step (ed_decode_fused_beam_step,
// or the step composed from the general kernels) on B * W rows and gets fp32 logits [B * W, V] and the states after
// the token (h_new / c_new).  Per utterance and frame:
//   lp_i = log_softmax(logits_i) in fp32, (z - max) - log(sum exp(z - max));  candidate (i, k) scores
//   logp_i + (double) lp_i[k];  the W best of the n x V candidates are kept (score descending, then i, then k);
//   (i, blank) keeps i's sequence, token-tree node, token and state, (i, k) appends k: a new node with its frame and
//   lp_i[k], token k and the state after i's token;  two kept candidates with the same token sequence - always a
//   (j, blank) and an (i, k) - become one: logp = log(exp(a) + exp(b)) in fp64, the place of the better ranked one,
//   j's node, token and state.  After the last frame the beam is sorted by logp (ties keep beam order).
// Sequence identity is a 64-bit FNV-1a hash over the tokens plus the length, carried per hypothesis.
//
// A frame is a fixed list of launches whatever the beams hold - the gather of frame t's joint rows, the step, the
// per-row top-W (sync_row_topw: one workgroup per ROW), the per-utterance select / merge / state gather (sync_select:
// one workgroup per utterance, over the W x W row candidates) - and nothing in the loop waits for the host.  No
// atomics: results are bit-identical from run to run.  Rows without a hypothesis (early frames, after merges) carry
// logp = -inf, token BOS and a zero state; the rows of an utterance past its length keep its final beam and are left
// alone by both kernels.  Rows flow through the step kernels either way and are row-independent there.
//
// LM shallow fusion and a bias list (opts->lm / opts->bias, the *_fused kernels): a row also carries the LM state
// from before its last token and the phrase automaton's state after its sequence; a frame gains the LM step on all
// B * W rows (ed_decode_lm_step, behind the prediction-network step), and a non-blank candidate scores
//   ((logp_i + (double) lp_i[k]) + (lm_w * (double) lp_lm_i[k] + lm_b)) + (held[goto(s_i, k)] - pend[s_i])
// where a term is absent when its feature is.  Without either the plain kernels run, launch for launch.
//
// Internal-LM estimation (ILME; opts->ilm_weight, sync_row_topw_ilm): the prior the transducer learned from its
// training transcripts is subtracted while an external LM is added.  The internal LM's logits of a row are the step's
// joint on an all-zero encoder row, z_ilm = tanh(act(d W1d^T + b1)) W2^T + b2 for the row's prediction-network output d;
// lp_ilm is their fp32 log-softmax over the NON-BLANK symbols, and a non-blank candidate's score gains
// - ilm_w * (double) lp_ilm[k] behind the LM term and in front of the list's.  ILME carries no per-row state: the select
// kernels and the persistent state are untouched.  On the fused step the frame keeps its launch count (the joint-hidden
// kernel writes both hidden vectors from one product, the logits kernel runs on 2 B W rows); composed, two launches more.
//
// The back-off n-gram (opts->ngram, the third LM kind SB_LM_NGRAM; ngram_tables.hpp): a row carries ONE int32 state,
// the state AFTER its sequence (the automaton's convention, not the LSTM's), `start` for the empty one.  No step and no
// [B W, V] buffer: sync_row_topw_ngram's workgroup builds the row's image - step(s_i, .) in fp64 and next(s_i, .) - in
// dynamic LDS from the back-off chain of s_i, as ngram_rows of ngram.hip fills its HBM row, scores from it,
//   c = c + (weight * step(s_i, k) + bonus)        (ngram_term: product rounded, then the bonus; never through fp32),
// and writes a kept candidate's next state beside its score and token; the select kernel reads that field, so it walks
// no table.  A frame's launch list is the plain search's.  One LM at a time: opts->lm with opts->ngram is refused.
//
// Second half of the file: the streaming form (edgedict_sync_stream_*), the same frame loop on a persistent state.
#include "bias_tables.hpp"
#include "decode_net.hpp"
#include "ngram_tables.hpp"

#include <algorithm>
#include <cmath>
#include <type_traits>
#include <vector>

namespace {

constexpr int SB_MAXW = 32;
constexpr unsigned long long SB_HASH0 = 0xcbf29ce484222325ull, SB_PRIME = 0x100000001b3ull;

struct SyncPtrs {
    double* logp;               // [B*W]  -inf: the row holds no hypothesis
    int32_t* node;              // [B*W]  leaf in the token tree, -1: the root (empty sequence)
    unsigned long long* hash;   // [B*W]  FNV-1a over the tokens
    int32_t* len;               // [B*W]  tokens
    int32_t* pred;              // [B*W]  last token (the step's symbol, StepBufs::pred)
    float* hs[2];               // [L][B*W][H] state before the last token, double-buffered per frame
    float* cs[2];
    double* c_score;            // [B*W][W] a row's W best candidates, sorted (score descending, k ascending) ...
    int32_t* c_k;               // ... their tokens (INT_MAX: none) ...
    float* c_lp;                // ... and log-softmax values
    int2* nodes;                // [B][NODES] (parent, token)
    int32_t* nd_frame;          // [B][NODES] the frame a node was created on
    float* nd_lp;               // [B][NODES] its token's log-softmax value on that frame
    int32_t* n_nodes;           // [B]
    int32_t* lens;              // [B]
};

// What LM shallow fusion and a bias list add to the rows: the second argument block of the *_fused kernels (the plain
// kernels never see it).  Row r carries the LM state from BEFORE its last token, as it carries the prediction network's,
// the token the LM steps on (lm_bos for the empty sequence) and the phrase automaton's state after its sequence.
struct SyncFuse {
    float* lm_hs[2];            // [lm_L][B*W][lm_H], double-buffered per frame as hs / cs
    float* lm_cs[2];
    int32_t* lm_pred;           // [B*W]  len == 0 ? lm_bos : pred (the LM step's symbol)
    int lm_L, lm_H, lm_bos;
    double lm_w, lm_b;          // weight, length bonus
    int32_t* bias_st;           // [B*W]  0: the automaton's root
    const int32_t* bias_root_next;      // the tables of edgedict_beam_bias_t (bias_tables.hpp)
    const double* bias_held;
    const double* bias_pend;
    const int32_t* bias_row_ptr;
    const int32_t* bias_exc_tok;
    const int32_t* bias_exc_next;
    int bias_S, bias_V;
    int32_t* ng_st;             // [B*W]  the n-gram state AFTER the row's sequence (ng_start: the empty one)
    int32_t* ng_next;           // [B*W][W] beside c_k: the state after the candidate's token (per call: workspace)
    int ng_start;
};

// the LM kind of a kernel instantiation (false / true of the forms without an n-gram are the first two)
constexpr int SB_LM_NONE = 0, SB_LM_LSTM = 1, SB_LM_NGRAM = 2;
// The n-gram's image of a row in dynamic LDS: lp fp64 [V], next int32 [V], 12 bytes a symbol.  With the top-W kernel's
// static LDS (112 bytes) it has to fit the 64 KiB a launch gets without a function attribute; 1 KiB is left spare.
constexpr int SB_NGRAM_MAX_V = 5376;
constexpr int SB_NGRAM_MAX_ORDER = 6;
static_assert((size_t)SB_NGRAM_MAX_V * 12 + 1024 <= 65536, "the n-gram image must fit 64 KiB of LDS");

__device__ __forceinline__ float sb_block_sum_max(float x, bool is_max, float* s_f) {
    x = is_max ? wave_max(x) : wave_sum(x);
    const int wave = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s_f[wave] = x;
    __syncthreads();
    x = s_f[0];
    for (int w = 1; w < 4; ++w) x = is_max ? fmaxf(x, s_f[w]) : x + s_f[w];
    return x;
}

__global__ void sync_init(SyncPtrs p, int B, int W, int bos) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= B * W) return;
    p.logp[r] = r % W == 0 ? 0.0 : -(double)INFINITY;
    p.node[r] = -1;
    p.hash[r] = SB_HASH0;
    p.len[r] = 0;
    p.pred[r] = bos;
    if (r < B) p.n_nodes[r] = 0;
}

// out[b * W + i, :] = frame t of utterance b's joint rows
template <typename T>
__global__ void sync_gather(const T* __restrict__ E1, long long row_stride, long long frame_stride, int t,
                            T* __restrict__ out, int BW, int W, int J) {
    const long long n = (long long)BW * J;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int r = (int)(i / J), j = (int)(i % J);
        out[i] = E1[(long long)(r / W) * row_stride + (long long)t * frame_stride + j];
    }
}

// One workgroup per row: the row's log-softmax terms, then its W best candidates by W arg-max passes - pass j takes the
// best candidate that comes after pass j - 1's pick in the order (score descending, k ascending), so nothing is marked.
// The W best of an utterance's n x V candidates are among its rows' W best.
// CACHED (V <= 256 * SB_VPT): a thread keeps its SB_VPT scores in registers over the passes instead of reading the
// logits again; the arithmetic and the order are the same either way.
constexpr int SB_VPT = 8;
// LM / BIAS (sync_row_topw_fused): a non-blank candidate k scores
//   ((base + (double)lp[k]) + (lm_w * (double)lp_lm[k] + lm_b)) + (held[goto(s, k)] - pend[s])
// in fp64, in this order, without contraction (as beam_expand_body of decode.hip); lp_lm is the same fp32 log-softmax
// over the row's LM logits, s the row's automaton state.  A term is absent when its feature is; blank keeps
// base + lp[blank]; c_lp stays lp[k].  goto is bias_goto's binary search in s's (short) exception row, once per
// candidate in the CACHED form and once per candidate and pass in the other.
// ILM (sync_row_topw_ilm): a third max / sum pass over the row's internal-LM logits that skips `blank`, and behind the LM
// term  c = c - ilm_w * (double)lp_ilm[k]  (__dsub_rn / __dmul_rn: no contraction), so ilm_w = 0 leaves every bit.
// LM == SB_LM_NGRAM (sync_row_topw_ngram): before the scoring passes the workgroup builds the row's n-gram image in dynamic
// LDS, ng_lp[v] = step(s, v) in fp64 and ng_nx[v] = next(s, v), the way ngram_rows fills its HBM row: the back-off chain
// s_0 = s, s_1 = fail(s_0), ... of at most `order` states with its prefix sums acc_j, every column from the unigram level
// (acc_d + uni_lp), then level by level towards the longest context (acc_j + arc_lp over the columns of s_j's arcs), a
// barrier between levels, so that a column ends with the longest context that has it - step()'s answer, in step()'s order
// of additions.  lp and next of a column are written by the same thread in the same level.  Every clamp of
// ngram_tables.hpp is kept: whatever the tables hold, the fill reads inside them, writes inside [0, V) and ends.
// score(v) gains  c = c + ngram_term(weight, ng_lp[v], bonus)  for v != blank, and thread j writes pick j's next state.
template <bool CACHED, int LM, bool BIAS, bool ILM = false>
__device__ __forceinline__ void sync_row_topw_body(const SyncPtrs& p, const SyncFuse& f,
                                                   const float* __restrict__ logits,
                                                   const float* __restrict__ lm_logits, int t, int W, int V, int blank,
                                                   const float* __restrict__ ilm_logits = nullptr, double ilm_w = 0.0,
                                                   const NgramTables* lt = nullptr) {
    const int r = blockIdx.x, tid = threadIdx.x;
    if (t >= p.lens[r / W]) return;
    const double base = p.logp[r];
    if (base == -(double)INFINITY) return;      // (sync_select never reads the candidates of such a row)
    __shared__ float sf[4];
    __shared__ double sd[2][4];                 // by pass parity: one barrier per pass is enough
    __shared__ int si[2][4];
    const float* z = logits + (size_t)r * V;
    float m = -INFINITY;
    for (int v = tid; v < V; v += 256) m = fmaxf(m, z[v]);
    m = sb_block_sum_max(m, true, sf);
    float s = 0.f;
    for (int v = tid; v < V; v += 256) s += expf(z[v] - m);
    s = sb_block_sum_max(s, false, sf);
    const float logs = logf(s);
    const float* zl = nullptr;
    float ml = 0.f, logsl = 0.f;
    if constexpr (LM == SB_LM_LSTM) {
        zl = lm_logits + (size_t)r * V;
        ml = -INFINITY;
        for (int v = tid; v < V; v += 256) ml = fmaxf(ml, zl[v]);
        ml = sb_block_sum_max(ml, true, sf);
        float sl = 0.f;
        for (int v = tid; v < V; v += 256) sl += expf(zl[v] - ml);
        sl = sb_block_sum_max(sl, false, sf);
        logsl = logf(sl);
    }
    const float* zi = nullptr;
    float mi = 0.f, logsi = 0.f;
    if constexpr (ILM) {
        zi = ilm_logits + (size_t)r * V;
        mi = -INFINITY;
        for (int v = tid; v < V; v += 256)
            if (v != blank) mi = fmaxf(mi, zi[v]);
        mi = sb_block_sum_max(mi, true, sf);
        float si = 0.f;
        for (int v = tid; v < V; v += 256)
            if (v != blank) si += expf(zi[v] - mi);
        si = sb_block_sum_max(si, false, sf);
        logsi = logf(si);
    }
    int st = 0;
    double pend_s = 0.0;
    if constexpr (BIAS) {
        st = bias_state(f, f.bias_st[r]);
        pend_s = f.bias_pend[st];
    }
    extern __shared__ double ng_lds[];
    double* ng_lp = ng_lds;                     // [V]
    int* ng_nx = (int*)(ng_lds + V);            // [V]
    if constexpr (LM == SB_LM_NGRAM) {
        const NgramTables& g = *lt;
        const int s0 = ngram_state(g, f.ng_st[r]);
        int chain[SB_NGRAM_MAX_ORDER];
        double acc[SB_NGRAM_MAX_ORDER + 1];
        int d = 0, s = s0;
        acc[0] = 0.0;
#pragma unroll
        for (int it = 0; it < SB_NGRAM_MAX_ORDER; ++it) {
            if (it < g.lm_order && s != 0) {
                chain[it] = s;
                acc[it + 1] = acc[it] + g.lm_backoff[s];
                s = ngram_state(g, g.lm_fail[s]);
                d = it + 1;
            } else {
                chain[it] = 0;
                acc[it + 1] = acc[it];
            }
        }
        const double base_acc = acc[SB_NGRAM_MAX_ORDER];        // = acc[d]: the levels behind the chain add nothing
        for (int k = tid; k < V; k += 256) {
            const bool isb = k == blank;
            ng_lp[k] = isb ? 0.0 : base_acc + g.lm_uni_lp[k];
            ng_nx[k] = isb ? s0 : ngram_state(g, g.lm_uni_next[k]);
        }
#pragma unroll
        for (int j = SB_NGRAM_MAX_ORDER - 1; j >= 0; --j) {
            if (j >= d) continue;                               // (uniform in the workgroup)
            __syncthreads();
            int lo, hi;
            ngram_row(g, chain[j], lo, hi);
            const double a = acc[j];
            for (int i = lo + tid; i < hi; i += 256) {
                const int k = g.lm_arc_tok[i];
                if (k < 0 || k >= V || k == blank) continue;    // eos, or a corrupt entry
                ng_lp[k] = a + g.lm_arc_lp[i];
                ng_nx[k] = ngram_state(g, g.lm_arc_next[i]);
            }
        }
        __syncthreads();
    }
    auto score = [&](int v) -> double {
        double c = base + (double)((z[v] - m) - logs);
        if constexpr (LM == SB_LM_LSTM) {
            if (v != blank) c = c + __dadd_rn(__dmul_rn(f.lm_w, (double)((zl[v] - ml) - logsl)), f.lm_b);
        }
        if constexpr (LM == SB_LM_NGRAM) {
            if (v != blank) c = __dadd_rn(c, ngram_term(lt->lm_weight, ng_lp[v], lt->lm_bonus));
        }
        if constexpr (ILM) {
            if (v != blank) c = __dsub_rn(c, __dmul_rn(ilm_w, (double)((zi[v] - mi) - logsi)));
        }
        if constexpr (BIAS) {
            if (v != blank) c = __dadd_rn(c, __dsub_rn(f.bias_held[bias_goto(f, st, v)], pend_s));
        }
        return c;
    };
    double sc[SB_VPT];
    if constexpr (CACHED) {
#pragma unroll
        for (int i = 0; i < SB_VPT; ++i) {
            const int v = tid + 256 * i;
            sc[i] = v < V ? score(v) : -(double)INFINITY;
        }
    }
    double prev = (double)INFINITY, my_best = -(double)INFINITY;
    int prev_k = -1, my_arg = 0x7fffffff;
    for (int j = 0; j < W; ++j) {
        double best = -(double)INFINITY;
        int arg = 0x7fffffff;
        if constexpr (CACHED) {
#pragma unroll
            for (int i = 0; i < SB_VPT; ++i) {
                const int v = tid + 256 * i;
                const double c = sc[i];
                if ((c < prev || (c == prev && v > prev_k)) && c > best) { best = c; arg = v; }
            }
        } else {
            for (int v = tid; v < V; v += 256) {
                const double c = score(v);
                if ((c < prev || (c == prev && v > prev_k)) && c > best) { best = c; arg = v; }
            }
        }
        // (max, first position) of the workgroup: butterfly in the wave, the four waves through this pass' LDS slots
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const double ov = __shfl_xor(best, off, 64);
            const int oa = __shfl_xor(arg, off, 64);
            if (ov > best || (ov == best && oa < arg)) { best = ov; arg = oa; }
        }
        double* s_v = sd[j & 1];
        int* s_a = si[j & 1];
        if ((tid & 63) == 0) { s_v[tid >> 6] = best; s_a[tid >> 6] = arg; }
        __syncthreads();
        best = s_v[0]; arg = s_a[0];
#pragma unroll
        for (int w = 1; w < 4; ++w)
            if (s_v[w] > best || (s_v[w] == best && s_a[w] < arg)) { best = s_v[w]; arg = s_a[w]; }
        if (tid == j) { my_best = best; my_arg = arg; }
        prev = best;
        prev_k = arg;
    }
    // thread j writes pass j's pick after the loop: a load of z[arg] inside it would sit in front of every barrier
    if (tid < W) {
        p.c_score[(size_t)r * W + tid] = my_best;
        p.c_k[(size_t)r * W + tid] = my_arg;
        p.c_lp[(size_t)r * W + tid] = my_arg < V ? (z[my_arg] - m) - logs : 0.f;
        if constexpr (LM == SB_LM_NGRAM) f.ng_next[(size_t)r * W + tid] = my_arg < V ? ng_nx[my_arg] : f.ng_start;
    }
}

template <bool CACHED>
__global__ __launch_bounds__(256) void sync_row_topw(SyncPtrs p, const float* __restrict__ logits, int t, int W, int V) {
    sync_row_topw_body<CACHED, SB_LM_NONE, false>(p, SyncFuse{}, logits, nullptr, t, W, V, -1);
}

template <bool CACHED, bool LM, bool BIAS>
__global__ __launch_bounds__(256) void sync_row_topw_fused(SyncPtrs p, SyncFuse f, const float* __restrict__ logits,
                                                           const float* __restrict__ lm_logits, int t, int W, int V,
                                                           int blank) {
    sync_row_topw_body<CACHED, LM ? SB_LM_LSTM : SB_LM_NONE, BIAS>(p, f, logits, lm_logits, t, W, V, blank);
}

template <bool CACHED, bool LM, bool BIAS>
__global__ __launch_bounds__(256) void sync_row_topw_ilm(SyncPtrs p, SyncFuse f, const float* __restrict__ logits,
                                                         const float* __restrict__ lm_logits,
                                                         const float* __restrict__ ilm_logits, double ilm_w, int t, int W,
                                                         int V, int blank) {
    sync_row_topw_body<CACHED, LM ? SB_LM_LSTM : SB_LM_NONE, BIAS, true>(p, f, logits, lm_logits, t, W, V, blank, ilm_logits,
                                                                         ilm_w);
}

// the n-gram form, with or without ILME (ilm_logits null / ilm_w unread without); dynamic LDS: 12 V bytes
template <bool CACHED, bool BIAS, bool ILM>
__global__ __launch_bounds__(256) void sync_row_topw_ngram(SyncPtrs p, SyncFuse f, NgramTables lt,
                                                           const float* __restrict__ logits,
                                                           const float* __restrict__ ilm_logits, double ilm_w, int t, int W,
                                                           int V, int blank) {
    sync_row_topw_body<CACHED, SB_LM_NGRAM, BIAS, ILM>(p, f, logits, nullptr, t, W, V, blank, ilm_logits, ilm_w, &lt);
}

// One workgroup per utterance.  Wave 0, lane j = the j-th kept candidate: a W-way merge of the rows' sorted lists picks
// the W best in order (ties: the lower row, inside a row the list's order), equal sequences are paired and folded, the
// survivors close ranks, token children get their tree nodes, and the beam's small fields are rewritten in place (every
// read of them comes before the first write, all inside this wave).  Then the whole workgroup gathers the states into
// the other buffer: a blank child takes its parent's state before the token, a token child the state after it.
// STREAM (the streaming search below, whose states outlive the call): a node's frame counts from the stream's reset,
// frame0[b] + t, and an utterance past its length copies its rows' states through to the other buffer, so that every
// stream's states are in the buffer the next frame reads whatever its own frame count.
// LM / BIAS (the *_fused kernels): a token child also takes the LM state after its parent's token (lm_h_new / lm_c_new,
// the LM step's output) and the automaton state goto(s, k); a blank child or a folded pair keeps the parent's (the two
// partners hold the same sequence, so the same states); a row left without a hypothesis gets a zero LM state and the
// root.  The automaton state and the LM's next symbol are small fields of wave 0; the LM states are gathered by the
// whole workgroup through the same s_src table, and copied through where the prediction network's are.

// the rows [r0, r0 + W) of a [L][BW][H] state: src < 0 zero, src & 0x100 from the step's output, else from the old buffer
__device__ __forceinline__ void sb_gather_rows(const int* s_src, const float* __restrict__ old_h,
                                               const float* __restrict__ old_c, const float* __restrict__ new_h,
                                               const float* __restrict__ new_c, float* __restrict__ out_h,
                                               float* __restrict__ out_c, int r0, int W, size_t BW, int L, int H) {
    const int H4 = H / 4, LH4 = L * H4;
    for (int idx = threadIdx.x; idx < W * LH4; idx += 256) {
        const int pos = idx / LH4, rem = idx % LH4, l = rem / H4, j = rem % H4;
        const int src = s_src ? s_src[pos] : pos;
        const size_t dst = ((size_t)l * BW + r0 + pos) * H4 + j;
        float4 hv = make_float4(0.f, 0.f, 0.f, 0.f), cv = hv;
        if (src >= 0) {
            const size_t so = ((size_t)l * BW + r0 + (src & 0xff)) * H4 + j;
            hv = ((const float4*)((src & 0x100) ? new_h : old_h))[so];
            cv = ((const float4*)((src & 0x100) ? new_c : old_c))[so];
        }
        ((float4*)out_h)[dst] = hv;
        ((float4*)out_c)[dst] = cv;
    }
}

// LM == SB_LM_NGRAM: the row's n-gram state is a small field of wave 0 as the automaton's is - the kept candidate's next
// state comes from the top-W kernel's ng_next (no table is walked here), a blank child keeps its parent's, the fold
// carries it as it carries c_st / f_st, rows behind n_new get ng_start.  There are no LM state buffers to gather.
template <bool STREAM, int LM, bool BIAS>
__device__ __forceinline__ void sync_select_body(const SyncPtrs& p, const SyncFuse& f, const float* __restrict__ h_new,
                                                 const float* __restrict__ c_new, const float* __restrict__ lm_h_new,
                                                 const float* __restrict__ lm_c_new, int t, int cur, int W, int B, int L,
                                                 int H, int NODES, int blank, int bos,
                                                 const int32_t* __restrict__ frame0) {
    const int b = blockIdx.x, tid = threadIdx.x, r0 = b * W;
    if (t >= p.lens[b]) {
        if constexpr (STREAM) {
            const int H4 = H / 4, LH4 = L * H4;
            const size_t BW = (size_t)B * W;
            for (int idx = tid; idx < W * LH4; idx += 256) {
                const int pos = idx / LH4, rem = idx % LH4, l = rem / H4, j = rem % H4;
                const size_t at = ((size_t)l * BW + r0 + pos) * H4 + j;
                ((float4*)p.hs[cur ^ 1])[at] = ((const float4*)p.hs[cur])[at];
                ((float4*)p.cs[cur ^ 1])[at] = ((const float4*)p.cs[cur])[at];
            }
            if constexpr (LM == SB_LM_LSTM)
                sb_gather_rows(nullptr, f.lm_hs[cur], f.lm_cs[cur], nullptr, nullptr, f.lm_hs[cur ^ 1], f.lm_cs[cur ^ 1],
                               r0, W, (size_t)B * W, f.lm_L, f.lm_H);
        }
        return;
    }
    int frame = t;
    if constexpr (STREAM) frame += frame0[b];
    __shared__ int s_src[SB_MAXW];      // per new place: the parent's place, | 0x100 for a token child; -1: no hypothesis
    __shared__ double s_score[SB_MAXW * SB_MAXW];       // the rows' sorted lists: the merge's loads are a dependent chain
    for (int i = tid; i < W * W; i += 256) s_score[i] = p.c_score[(size_t)r0 * W + i];
    __syncthreads();
    if (tid < 64) {
        const int lane = tid;
        const bool row_ok = lane < W && p.logp[r0 + lane] != -(double)INFINITY;
        int head = 0;
        double hv = row_ok ? s_score[lane * W] : -(double)INFINITY;
        int sel_i = 0, sel_h = 0, n_kept = 0;
        double sel_v = -(double)INFINITY;
        for (int j = 0; j < W; ++j) {
            double v = hv;
            int a = hv == -(double)INFINITY ? 0x7fffffff : lane;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const double ov = __shfl_xor(v, off, 64);
                const int oa = __shfl_xor(a, off, 64);
                if (ov > v || (ov == v && oa < a)) { v = ov; a = oa; }
            }
            if (a == 0x7fffffff) break;         // fewer than W candidates: all are kept
            const int hd = __shfl(head, a, 64);
            if (lane == j) { sel_i = a; sel_h = hd; sel_v = v; }
            if (lane == a) {
                ++head;
                hv = head < W ? s_score[lane * W + head] : -(double)INFINITY;
            }
            ++n_kept;
        }
        const bool kept = lane < n_kept;
        // the candidate and its parent's fields
        const size_t ci = (size_t)(r0 + sel_i) * W + sel_h;
        const int k = kept ? p.c_k[ci] : blank;
        const float lp = kept ? p.c_lp[ci] : 0.f;
        const int par_node = p.node[r0 + sel_i], par_tok = p.pred[r0 + sel_i], par_len = p.len[r0 + sel_i];
        const unsigned long long par_hash = p.hash[r0 + sel_i];
        const int n_nodes0 = p.n_nodes[b];
        int par_st = 0;
        if constexpr (BIAS) par_st = f.bias_st[r0 + sel_i];
        const int is_blank = k == blank;
        int c_st = 0;
        if constexpr (BIAS) c_st = (is_blank || k < 0 || k >= f.bias_V) ? par_st : bias_goto(f, par_st, k);
        int c_ng = 0;
        if constexpr (LM == SB_LM_NGRAM) c_ng = !kept ? f.ng_start : is_blank ? f.ng_st[r0 + sel_i] : f.ng_next[ci];
        const unsigned long long c_hash = is_blank ? par_hash : (par_hash ^ (unsigned long long)(k + 1)) * SB_PRIME;
        const int c_len = is_blank ? par_len : par_len + 1;
        // the other kept candidate with the same sequence, if there is one
        int partner = -1;
        for (int jj = 0; jj < n_kept; ++jj) {
            const unsigned long long oh = __shfl(c_hash, jj, 64);
            const int ol = __shfl(c_len, jj, 64);
            if (kept && jj != lane && partner < 0 && oh == c_hash && ol == c_len) partner = jj;
        }
        const int pl = partner < 0 ? lane : partner;
        const double ov = __shfl(sel_v, pl, 64);
        const int o_blank = __shfl(is_blank, pl, 64);
        double v = sel_v;
        if (partner >= 0) {
            const double mx = fmax(sel_v, ov), mn = fmin(sel_v, ov);
            v = mx + log1p(exp(mn - mx));
        }
        const bool alive = kept && (partner < 0 || lane < partner);
        // a folded pair keeps the blank child's node, token and state: the older creation frame
        const int src = (partner >= 0 && !is_blank && o_blank) ? partner : lane;
        const int f_i = __shfl(sel_i, src, 64), f_k = __shfl(k, src, 64), f_blank = __shfl(is_blank, src, 64);
        const int f_node = __shfl(par_node, src, 64), f_tok = __shfl(par_tok, src, 64);
        const float f_lp = __shfl(lp, src, 64);
        int f_st = 0;
        if constexpr (BIAS) f_st = __shfl(c_st, src, 64);
        int f_ng = 0;
        if constexpr (LM == SB_LM_NGRAM) f_ng = __shfl(c_ng, src, 64);
        const unsigned long long below = (1ull << lane) - 1ull;
        const unsigned long long m_alive = __ballot(alive);
        const unsigned long long m_new = __ballot(alive && !f_blank);
        const int pos = __popcll(m_alive & below), n_new = __popcll(m_alive);
        const int nid = n_nodes0 + __popcll(m_new & below);
        if (alive) {
            const int row = r0 + pos;
            p.logp[row] = v;
            p.hash[row] = c_hash;
            p.len[row] = c_len;
            if (f_blank) {
                p.node[row] = f_node;
                p.pred[row] = f_tok;
                s_src[pos] = f_i;
            } else {
                if (nid < NODES) {
                    p.nodes[(size_t)b * NODES + nid] = make_int2(f_node, f_k);
                    p.nd_frame[(size_t)b * NODES + nid] = frame;
                    p.nd_lp[(size_t)b * NODES + nid] = f_lp;
                }
                p.node[row] = nid;
                p.pred[row] = f_k;
                s_src[pos] = f_i | 0x100;
            }
            if constexpr (LM == SB_LM_LSTM) f.lm_pred[row] = c_len == 0 ? f.lm_bos : (f_blank ? f_tok : f_k);
            if constexpr (LM == SB_LM_NGRAM) f.ng_st[row] = f_ng;
            if constexpr (BIAS) f.bias_st[row] = f_st;
        }
        if (lane >= n_new && lane < W) {
            const int row = r0 + lane;
            if constexpr (LM == SB_LM_LSTM) f.lm_pred[row] = f.lm_bos;
            if constexpr (LM == SB_LM_NGRAM) f.ng_st[row] = f.ng_start;
            if constexpr (BIAS) f.bias_st[row] = 0;
            p.logp[row] = -(double)INFINITY;
            p.hash[row] = SB_HASH0;
            p.len[row] = 0;
            p.node[row] = -1;
            p.pred[row] = bos;
            s_src[lane] = -1;
        }
        if (lane == 0) p.n_nodes[b] = n_nodes0 + __popcll(m_new);
    }
    __syncthreads();
    const float* hs_o = p.hs[cur];
    const float* cs_o = p.cs[cur];
    float* hs_n = p.hs[cur ^ 1];
    float* cs_n = p.cs[cur ^ 1];
    // 16 bytes per access: every buffer is 256-byte aligned and H a multiple of 4 (checked by the entry point; the LSTM
    // kernels of the step ask for a multiple of 8)
    const int H4 = H / 4, LH4 = L * H4;
    const size_t BW = (size_t)B * W;
    for (int idx = tid; idx < W * LH4; idx += 256) {
        const int pos = idx / LH4, rem = idx % LH4, l = rem / H4, j = rem % H4;
        const int src = s_src[pos];
        const size_t dst = ((size_t)l * BW + r0 + pos) * H4 + j;
        float4 hv = make_float4(0.f, 0.f, 0.f, 0.f), cv = hv;
        if (src >= 0) {
            const size_t so = ((size_t)l * BW + r0 + (src & 0xff)) * H4 + j;
            hv = ((const float4*)((src & 0x100) ? h_new : hs_o))[so];
            cv = ((const float4*)((src & 0x100) ? c_new : cs_o))[so];
        }
        ((float4*)hs_n)[dst] = hv;
        ((float4*)cs_n)[dst] = cv;
    }
    if constexpr (LM == SB_LM_LSTM)
        sb_gather_rows(s_src, f.lm_hs[cur], f.lm_cs[cur], lm_h_new, lm_c_new, f.lm_hs[cur ^ 1], f.lm_cs[cur ^ 1], r0, W,
                       BW, f.lm_L, f.lm_H);
}

__global__ __launch_bounds__(256) void sync_select(SyncPtrs p, const float* __restrict__ h_new,
                                                   const float* __restrict__ c_new, int t, int cur, int W, int B, int L,
                                                   int H, int NODES, int blank, int bos) {
    sync_select_body<false, SB_LM_NONE, false>(p, SyncFuse{}, h_new, c_new, nullptr, nullptr, t, cur, W, B, L, H, NODES, blank,
                                          bos, nullptr);
}

__global__ __launch_bounds__(256) void sync_stream_select(SyncPtrs p, const float* __restrict__ h_new,
                                                          const float* __restrict__ c_new, int t, int cur, int W, int B,
                                                          int L, int H, int NODES, int blank, int bos,
                                                          const int32_t* __restrict__ frame0) {
    sync_select_body<true, SB_LM_NONE, false>(p, SyncFuse{}, h_new, c_new, nullptr, nullptr, t, cur, W, B, L, H, NODES, blank,
                                         bos, frame0);
}

template <bool STREAM, int LM, bool BIAS>
__global__ __launch_bounds__(256) void sync_select_fused(SyncPtrs p, SyncFuse f, const float* __restrict__ h_new,
                                                         const float* __restrict__ c_new,
                                                         const float* __restrict__ lm_h_new,
                                                         const float* __restrict__ lm_c_new, int t, int cur, int W, int B,
                                                         int L, int H, int NODES, int blank, int bos,
                                                         const int32_t* __restrict__ frame0) {
    sync_select_body<STREAM, LM, BIAS>(p, f, h_new, c_new, lm_h_new, lm_c_new, t, cur, W, B, L, H, NODES, blank, bos, frame0);
}

// the fused forms' part of sync_init: the LM steps on lm_bos, the automaton stands on its root, the n-gram on `start`
__global__ void sync_init_fused(SyncFuse f, int BW) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= BW) return;
    if (f.lm_pred) f.lm_pred[r] = f.lm_bos;
    if (f.bias_st) f.bias_st[r] = 0;
    if (f.ng_st) f.ng_st[r] = f.ng_start;
}

// Read-out: an utterance's beam ranked by logp descending (ties keep beam order), every path walked root to leaf into
// the dense result rows [b][rank][0, MT).  A path longer than MT writes its length only.
__global__ __launch_bounds__(64) void sync_read(SyncPtrs p, int W, int NODES, int MT, int32_t* __restrict__ r_nhyp,
                                                int32_t* __restrict__ r_len, double* __restrict__ r_logp,
                                                int32_t* __restrict__ r_tok, int32_t* __restrict__ r_frame,
                                                double* __restrict__ r_lp) {
    const int b = blockIdx.x, j = threadIdx.x, r0 = b * W;
    if (j >= W) return;
    const double v = p.logp[r0 + j];
    const bool live = v != -(double)INFINITY;
    int rank = 0, n = 0;
    for (int jj = 0; jj < W; ++jj) {
        const double o = p.logp[r0 + jj];
        if (o != -(double)INFINITY) ++n;
        if (o > v || (o == v && jj < j)) ++rank;
    }
    if (j == 0) r_nhyp[b] = n;
    if (!live) return;          // (the slots behind n are not written)
    const size_t row = (size_t)r0 + rank;
    r_logp[row] = v;
    const int2* tree = p.nodes + (size_t)b * NODES;
    const int leaf = p.node[r0 + j];
    int d = 0;
    for (int nd = leaf; nd >= 0 && nd < NODES && d <= NODES; nd = tree[nd].x) ++d;
    r_len[row] = d;
    if (d > MT) return;
    int k = d;
    for (int nd = leaf; nd >= 0 && nd < NODES && k > 0; nd = tree[nd].x) {
        --k;
        r_tok[row * MT + k] = tree[nd].y;
        r_frame[row * MT + k] = p.nd_frame[(size_t)b * NODES + nd];
        r_lp[row * MT + k] = (double)p.nd_lp[(size_t)b * NODES + nd];
    }
}

struct SyncWs {
    Ws step;
    size_t step_at, e1g, hs0, hs1, cs0, cs1, logp, node, hash, len, c_score, c_k, c_lp, nodes, nd_frame, nd_lp, n_nodes,
        lens, total;
};
// `rows`: the step's layout for B * W rows
SyncWs sync_layout(const SearchNet& rows, size_t B, size_t W, size_t T) {
    SyncWs w{};
    const size_t BW = B * W, LH = (size_t)rows.pred.L * rows.pred.H, NODES = T * W;
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t r = o; o += align256(bytes); return r; };
    w.step = ws_layout(rows);
    w.step_at = take(w.step.total);
    w.e1g = take(BW * rows.J * rows.esz);
    w.hs0 = take(BW * LH * 4);
    w.hs1 = take(BW * LH * 4);
    w.cs0 = take(BW * LH * 4);
    w.cs1 = take(BW * LH * 4);
    w.logp = take(BW * 8);
    w.node = take(BW * 4);
    w.hash = take(BW * 8);
    w.len = take(BW * 4);
    w.c_score = take(BW * W * 8);
    w.c_k = take(BW * W * 4);
    w.c_lp = take(BW * W * 4);
    w.nodes = take(B * NODES * 8);
    w.nd_frame = take(B * NODES * 4);
    w.nd_lp = take(B * NODES * 4);
    w.n_nodes = take(B * 4);
    w.lens = take(B * 4);
    w.total = o;
    return w;
}

struct SyncRes {
    size_t nhyp, len, logp, tok, frame, lp, total;
};
SyncRes sync_result_layout(size_t B, size_t W, size_t MT) {
    SyncRes r{};
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t x = o; o += align256(bytes); return x; };
    r.nhyp = take(B * 4);
    r.len = take(B * W * 4);
    r.logp = take(B * W * 8);
    r.tok = take(B * W * MT * 4);
    r.frame = take(B * W * MT * 4);
    r.lp = take(B * W * MT * 8);
    r.total = o;
    return r;
}

template <typename T>
T* at(char* base, size_t off) { return (T*)(base + off); }

bool sync_dims_ok(const edgedict_search_net_t& n, int B, int T, int W) {
    return (n.dtype == ED_F32 || n.dtype == ED_BF16) && B > 0 && T > 0 && n.J > 0 && n.V > 0 && n.E > 0 && n.L > 0 &&
           n.H > 0 && n.H % 4 == 0 && n.P2 > 0 && W >= 1 && W <= SB_MAXW && (long long)B * W <= 0x7fffffff / 256;
}
// the step's network: B * W rows whose joint rows are gathered per frame, J apart (E1 is bound once the workspace is)
SearchNet sync_net_of(const edgedict_search_net_t& n, int rows, int W, int NODES) {
    return search_net_of(n, nullptr, (long long)n.J, 0, rows, W, 0, NODES);
}

// LM fusion / a bias list, host side.  Both parts are APPENDED behind a plain layout (offsets from `base`, a multiple of
// 256), so every plain offset holds in every form.  The rows' part - what SyncFuse points at - lives in the offline
// workspace or in the streams' persistent state; the LM step's buffers are always workspace.
struct SyncFuseRows {
    size_t lm_hs0, lm_hs1, lm_cs0, lm_cs1, lm_pred, bias_st, ng_st, total;
};
SyncFuseRows sync_fuse_rows_layout(size_t base, size_t rows, const edgedict_beam_lm_t* lm,
                                   const edgedict_beam_bias_t* bias, const edgedict_ngram_lm_t* ng) {
    SyncFuseRows a{};
    size_t o = base;
    auto take = [&](size_t bytes) { size_t r = o; o += align256(bytes); return r; };
    if (lm) {
        const size_t st = rows * (size_t)lm->L * lm->H * 4;
        a.lm_hs0 = take(st);
        a.lm_hs1 = take(st);
        a.lm_cs0 = take(st);
        a.lm_cs1 = take(st);
        a.lm_pred = take(rows * 4);
    }
    if (bias) a.bias_st = take(rows * 4);
    if (ng) a.ng_st = take(rows * 4);           // (last: every offset of the forms without an n-gram holds)
    a.total = o;
    return a;
}
// the n-gram's per-call scratch - the candidates' next states [rows][W] - behind every other part of a workspace
struct SyncNgramWs {
    size_t ng_next, total;
};
SyncNgramWs sync_ngram_ws_layout(size_t base, size_t rows, size_t W, const edgedict_ngram_lm_t* ng) {
    SyncNgramWs w{};
    w.total = base;
    if (ng) {
        w.ng_next = base;
        w.total = base + align256(rows * W * 4);
    }
    return w;
}
struct SyncFuseStep {
    size_t x, G, Hprev, Y0, Y1, Cst, h_new, c_new, logits, total;
};
SyncFuseStep sync_fuse_step_layout(size_t base, size_t rows, size_t esz, size_t V, const edgedict_beam_lm_t* lm) {
    SyncFuseStep w{};
    size_t o = base;
    auto take = [&](size_t bytes) { size_t r = o; o += align256(bytes); return r; };
    if (lm) {
        const size_t H = lm->H, LH = (size_t)lm->L * lm->H;
        w.x = take(rows * lm->E * esz);
        w.G = take(rows * 4 * H * esz);
        w.Hprev = take(rows * H * esz);
        w.Y0 = take(rows * H * esz);
        w.Y1 = take(rows * H * esz);
        w.Cst = take(rows * H * 4);
        w.h_new = take(rows * LH * 4);
        w.c_new = take(rows * LH * 4);
        w.logits = take(rows * V * 4);
    }
    w.total = o;
    return w;
}

// an LM / a bias list this search can use (checked before anything is launched)
int sync_fuse_check(const edgedict_beam_lm_t* lm, const edgedict_beam_bias_t* bias, int V, const char* what) {
    if (int rc = ed_decode_lm_check(lm, V, 0, what)) return rc;
    ED_CHECK_ARG(!lm || lm->H % 4 == 0, "%s: the LM's hidden width H = %d must be a multiple of 4", what, lm->H);
    return ed_decode_bias_check(bias, V, 0, what);
}
// what check_net leaves to this search: every layer's pointers and the embedding table's dtype
int sync_layers_check(const edgedict_search_net_t& n, const char* what) {
    for (int k = 0; k < n.L; ++k)
        ED_CHECK_ARG(n.w_ih[k] && n.w_hh[k] && n.b_ih[k] && n.b_hh[k], "%s: null pointer (layer %d)", what, k);
    ED_CHECK_ARG(n.emb_dtype == ED_F32 || n.emb_dtype == ED_BF16, "%s: bad embedding dtype", what);
    return ED_OK;
}
bool sync_fuse_dims_ok(const edgedict_beam_lm_t* lm, const edgedict_beam_bias_t* bias, int V) {
    return (!lm || (lm->V == V && lm->L > 0 && lm->E > 0 && lm->H > 0 && lm->H % 4 == 0)) && (!bias || bias->S > 0);
}
// An n-gram this search can use (null: none), checked before anything is launched; V / blank < 0: not known to the
// caller (the streaming reset and state query), the advance checks them.  The size queries call it too: they return 0
// where it fails, and the message says why.
int sync_ngram_check(const edgedict_ngram_lm_t* ng, const edgedict_beam_lm_t* lm, int V, int blank, const char* what) {
    if (!ng) return ED_OK;
    ED_CHECK_ARG(!lm, "%s: opts->lm and opts->ngram are both set (one LM at a time)", what);
    if (int rc = ed_ngram_check(ng, what)) return rc;
    ED_CHECK_ARG(V < 0 || ng->V == V, "%s: the n-gram's vocabulary (V = %d) differs from the transducer's (V = %d)", what,
                 ng->V, V);
    ED_CHECK_ARG(blank < 0 || ng->blank == blank, "%s: the n-gram's blank (%d) differs from the transducer's (%d)", what,
                 ng->blank, blank);
    ED_CHECK_ARG(std::isfinite(ng->weight) && ng->weight >= 0.0, "%s: the n-gram's weight = %g (must be finite and >= 0)",
                 what, ng->weight);
    ED_CHECK_ARG(std::isfinite(ng->length_bonus), "%s: the n-gram's length_bonus = %g is not finite", what,
                 ng->length_bonus);
    ED_CHECK_ARG(ng->V <= SB_NGRAM_MAX_V,
                 "%s: the n-gram's V = %d exceeds %d (the row's image, 12 bytes a symbol, has to fit 64 KiB of LDS)", what,
                 ng->V, SB_NGRAM_MAX_V);
    return ED_OK;
}

// One search call's fusion: the kernels' block, the LM as a network and its step's buffers
struct SyncFusion {
    bool lm, bias, ngram;       // lm: the LSTM
    NgramTables lt;
    SyncFuse f;
    LstmNet lm_net;
    StepBufs lmu;
};
// rows_base + ra: where the rows' part lives;  ws + wa: the LM step's buffers;  ws + na: the n-gram's scratch
SyncFusion sync_fuse_bind(char* rows_base, const SyncFuseRows& ra, char* ws, const SyncFuseStep* wa,
                          const edgedict_beam_lm_t* lm, const edgedict_beam_bias_t* bias,
                          const edgedict_ngram_lm_t* ng = nullptr, const SyncNgramWs* na = nullptr) {
    SyncFusion u{};
    u.lm = lm != nullptr;
    u.bias = bias != nullptr;
    u.ngram = ng != nullptr;
    SyncFuse& f = u.f;
    if (ng) {
        u.lt = ed_ngram_tables(ng);
        f.ng_st = at<int32_t>(rows_base, ra.ng_st);
        f.ng_next = na ? at<int32_t>(ws, na->ng_next) : nullptr;
        f.ng_start = ng->start;
    }
    if (lm) {
        f.lm_hs[0] = at<float>(rows_base, ra.lm_hs0); f.lm_hs[1] = at<float>(rows_base, ra.lm_hs1);
        f.lm_cs[0] = at<float>(rows_base, ra.lm_cs0); f.lm_cs[1] = at<float>(rows_base, ra.lm_cs1);
        f.lm_pred = at<int32_t>(rows_base, ra.lm_pred);
        f.lm_L = lm->L; f.lm_H = lm->H; f.lm_bos = lm->bos;
        f.lm_w = lm->weight; f.lm_b = lm->length_bonus;
        u.lm_net = lm_net_of(*lm);
        if (wa)
            u.lmu = StepBufs{nullptr, nullptr, at<float>(ws, wa->logits), f.lm_pred, ws + wa->x, ws + wa->G,
                             ws + wa->Hprev, {ws + wa->Y0, ws + wa->Y1}, at<float>(ws, wa->Cst), at<float>(ws, wa->h_new),
                             at<float>(ws, wa->c_new), nullptr};
    }
    if (bias) {
        f.bias_st = at<int32_t>(rows_base, ra.bias_st);
        f.bias_root_next = bias->root_next;
        f.bias_held = bias->held;
        f.bias_pend = bias->pend;
        f.bias_row_ptr = bias->row_ptr;
        f.bias_exc_tok = bias->exc_tok;
        f.bias_exc_next = bias->exc_next;
        f.bias_S = bias->S;
        f.bias_V = bias->V;
    }
    return u;
}

// ILME, host side: the buffers behind every other part of a workspace (offsets from `base`), sized for either step -
// fused: hid2 [2 rows, J] and logits2 fp32 [2 rows, V]; composed: their first halves and the zero encoder row.
struct SyncIlmWs {
    size_t hid2, logits2, zero_row, total;
};
SyncIlmWs sync_ilm_layout(size_t base, size_t rows, size_t esz, size_t J, size_t V, bool on) {
    SyncIlmWs w{};
    size_t o = base;
    auto take = [&](size_t bytes) { size_t r = o; o += align256(bytes); return r; };
    if (on) {
        w.hid2 = take(2 * rows * J * esz);
        w.logits2 = take(2 * rows * V * 4);
        w.zero_row = take(J * esz);
    }
    w.total = o;
    return w;
}
// a usable weight: finite and >= 0 (null: ILME is off)
bool sync_ilm_ok(const double* ilm_weight) { return !ilm_weight || (std::isfinite(*ilm_weight) && *ilm_weight >= 0.0); }
int sync_ilm_check(const double* ilm_weight, const char* what) {
    ED_CHECK_ARG(sync_ilm_ok(ilm_weight), "%s: ilm_weight = %g (must be finite and >= 0)", what, *ilm_weight);
    return ED_OK;
}
// One call's ILME: the weight, where the internal LM's logits of the rows are, the step's extra buffers
struct SyncIlm {
    double w;
    const float* logits;
    void* hid2;
    float* logits2;
    const void* zero_row;
};
// the step of one frame: u.logits holds the rows' RNN-T logits afterwards (with ILME on the fused step: u = ui, whose
// logits point into logits2)
int sync_step(bool fused, const SearchNet& net, const float* hs, const float* cs, const StepBufs& u, const SyncIlm* il,
              hipStream_t s) {
    if (!il) {
        if (fused) return ed_decode_fused_beam_step(net, net.E1, hs, cs, u, s);
        return ed_decode_composed_beam_step(net, net.E1, hs, cs, u, s);
    }
    if (fused) return ed_decode_fused_beam_step_ilm(net, net.E1, hs, cs, u, il->hid2, il->logits2, s);
    return ed_decode_composed_beam_step_ilm(net, net.E1, hs, cs, u, il->zero_row, il->hid2, il->logits2, s);
}
// binds ILME's buffers at p + a; `u` is the step's bundle, whose logits move into logits2 on the fused step
SyncIlm sync_ilm_bind(char* p, const SyncIlmWs& a, double w, bool fused, size_t rows, size_t V, StepBufs& u) {
    SyncIlm il{w, nullptr, p + a.hid2, at<float>(p, a.logits2), p + a.zero_row};
    if (fused) {
        u.logits = il.logits2;
        il.logits = il.logits2 + rows * V;
    } else {
        il.logits = il.logits2;
    }
    return il;
}

// The frame's last two launches: the per-row top-W and the select / merge / gather.  fu and il null: the plain kernels.
// ILME alone has no per-row state: its top-W kernel, then the plain select.  An n-gram (fu->ngram; never with fu->lm):
// sync_row_topw_ngram with 12 V bytes of dynamic LDS, then the select's SB_LM_NGRAM form.
template <bool STREAM>
void sync_launch_pick(const SyncPtrs& q, const SyncFusion* fu, const StepBufs& u, int t, int cur, int W, int B, int L,
                      int H, int NODES, int V, int blank, int bos, const int32_t* frame0, hipStream_t s,
                      const SyncIlm* il = nullptr) {
    const int BW = B * W;
    const bool cached = V <= 256 * SB_VPT;
    auto plain_select = [&] {
        if constexpr (STREAM)
            hipLaunchKernelGGL(sync_stream_select, dim3(B), dim3(256), 0, s, q, u.h_new, u.c_new, t, cur, W, B, L, H,
                               NODES, blank, bos, frame0);
        else
            hipLaunchKernelGGL(sync_select, dim3(B), dim3(256), 0, s, q, u.h_new, u.c_new, t, cur, W, B, L, H, NODES,
                               blank, bos);
    };
    if (fu && fu->ngram) {      // the n-gram forms: LM kind SB_LM_NGRAM x BIAS x ILM x CACHED, the image in dynamic LDS
        const size_t lds = (size_t)V * 12;
        auto go = [&](auto bias_tag, auto ilm_tag) {
            constexpr bool BIAS = decltype(bias_tag)::value, ILM = decltype(ilm_tag)::value;
            const float* iz = il ? il->logits : nullptr;
            const double iw = il ? il->w : 0.0;
            if (cached)
                hipLaunchKernelGGL((sync_row_topw_ngram<true, BIAS, ILM>), dim3(BW), dim3(256), lds, s, q, fu->f, fu->lt,
                                   u.logits, iz, iw, t, W, V, blank);
            else
                hipLaunchKernelGGL((sync_row_topw_ngram<false, BIAS, ILM>), dim3(BW), dim3(256), lds, s, q, fu->f, fu->lt,
                                   u.logits, iz, iw, t, W, V, blank);
            hipLaunchKernelGGL((sync_select_fused<STREAM, SB_LM_NGRAM, BIAS>), dim3(B), dim3(256), 0, s, q, fu->f, u.h_new,
                               u.c_new, (const float*)nullptr, (const float*)nullptr, t, cur, W, B, L, H, NODES, blank, bos,
                               frame0);
        };
        if (fu->bias && il) go(std::true_type{}, std::true_type{});
        else if (fu->bias) go(std::true_type{}, std::false_type{});
        else if (il) go(std::false_type{}, std::true_type{});
        else go(std::false_type{}, std::false_type{});
        return;
    }
    if (il) {
        const SyncFuse none{};
        const SyncFuse& f = fu ? fu->f : none;
        auto go = [&](auto lm_tag, auto bias_tag) {
            constexpr bool LM = decltype(lm_tag)::value, BIAS = decltype(bias_tag)::value;
            const float* lz = fu ? fu->lmu.logits : nullptr;
            if (cached)
                hipLaunchKernelGGL((sync_row_topw_ilm<true, LM, BIAS>), dim3(BW), dim3(256), 0, s, q, f, u.logits, lz,
                                   il->logits, il->w, t, W, V, blank);
            else
                hipLaunchKernelGGL((sync_row_topw_ilm<false, LM, BIAS>), dim3(BW), dim3(256), 0, s, q, f, u.logits, lz,
                                   il->logits, il->w, t, W, V, blank);
            if constexpr (LM || BIAS)
                hipLaunchKernelGGL((sync_select_fused<STREAM, LM, BIAS>), dim3(B), dim3(256), 0, s, q, f, u.h_new, u.c_new,
                                   (const float*)fu->lmu.h_new, (const float*)fu->lmu.c_new, t, cur, W, B, L, H, NODES,
                                   blank, bos, frame0);
            else
                plain_select();
        };
        const bool lm = fu && fu->lm, bias = fu && fu->bias;
        if (lm && bias) go(std::true_type{}, std::true_type{});
        else if (lm) go(std::true_type{}, std::false_type{});
        else if (bias) go(std::false_type{}, std::true_type{});
        else go(std::false_type{}, std::false_type{});
        return;
    }
    if (!fu) {
        if (cached) hipLaunchKernelGGL(sync_row_topw<true>, dim3(BW), dim3(256), 0, s, q, u.logits, t, W, V);
        else hipLaunchKernelGGL(sync_row_topw<false>, dim3(BW), dim3(256), 0, s, q, u.logits, t, W, V);
        plain_select();
        return;
    }
    auto go = [&](auto lm_tag, auto bias_tag) {
        constexpr bool LM = decltype(lm_tag)::value, BIAS = decltype(bias_tag)::value;
        const float* lz = fu->lmu.logits;
        if (cached)
            hipLaunchKernelGGL((sync_row_topw_fused<true, LM, BIAS>), dim3(BW), dim3(256), 0, s, q, fu->f, u.logits, lz, t,
                               W, V, blank);
        else
            hipLaunchKernelGGL((sync_row_topw_fused<false, LM, BIAS>), dim3(BW), dim3(256), 0, s, q, fu->f, u.logits, lz,
                               t, W, V, blank);
        hipLaunchKernelGGL((sync_select_fused<STREAM, LM, BIAS>), dim3(B), dim3(256), 0, s, q, fu->f, u.h_new, u.c_new,
                           (const float*)fu->lmu.h_new, (const float*)fu->lmu.c_new, t, cur, W, B, L, H, NODES, blank,
                           bos, frame0);
    };
    if (fu->lm && fu->bias) go(std::true_type{}, std::true_type{});
    else if (fu->lm) go(std::true_type{}, std::false_type{});
    else go(std::false_type{}, std::true_type{});
}

}  // namespace

// the plain size; an LM / a bias list / an n-gram append their parts behind it, ILME its buffers behind those, the
// n-gram's candidate field behind everything
extern "C" size_t edgedict_sync_beam_workspace_bytes(const edgedict_search_net_t* pn, int B, int T, int W,
                                                     const edgedict_search_opts_t* opts) {
    if (!pn || !search_ptrs_ok(pn, opts)) return 0;
    const edgedict_search_opts_t o = search_opts_of(opts);
    if (!sync_dims_ok(*pn, B, T, W) || !sync_fuse_dims_ok(o.lm, o.bias, pn->V) || !sync_ilm_ok(o.ilm_weight))
        return 0;
    if (sync_ngram_check(o.ngram, o.lm, pn->V, pn->blank, "sync_beam_workspace_bytes")) return 0;
    const SearchNet net = sync_net_of(*pn, B * W, W, T * W);
    const size_t BW = (size_t)B * W, esz = net.esz;
    const size_t plain = sync_layout(net, B, W, T).total;
    const size_t fuse =
        sync_fuse_rows_layout(sync_fuse_step_layout(plain, BW, esz, net.V, o.lm).total, BW, o.lm, o.bias, o.ngram).total;
    const size_t ilm = sync_ilm_layout(fuse, BW, esz, net.J, net.V, o.ilm_weight != nullptr).total;
    return sync_ngram_ws_layout(ilm, BW, W, o.ngram).total;
}

extern "C" size_t edgedict_sync_beam_result_bytes(int B, int W, int max_tokens) {
    if (B <= 0 || W <= 0 || max_tokens < 0) return 0;
    return sync_result_layout(B, W, max_tokens).total;
}

// opts null or all its members null: the plain search, launch for launch;  ilm_weight null: the search without ILME
extern "C" int edgedict_sync_beam_search(const edgedict_search_net_t* pn, const void* E1, long long e_row_stride,
                                         long long e_frame_stride, int B, int T, const int32_t* lens_host, int W,
                                         int32_t* tokens_host, int32_t* frames_host, double* token_logp_host,
                                         int max_tokens, int32_t* ntokens_host, int32_t* nhyp_host, double* logp_host,
                                         const edgedict_search_opts_t* opts, void* workspace, void* result,
                                         void* stream_) {
    ED_CHECK_ARG(search_ptrs_ok(pn, opts), "sync_beam_search: net / opts is not a pointer");
    const edgedict_search_opts_t o = search_opts_of(opts);
    const edgedict_beam_lm_t* lm = o.lm;
    const edgedict_beam_bias_t* bias = o.bias;
    const double* ilm_weight = o.ilm_weight;
    const edgedict_ngram_lm_t* ng = o.ngram;
    ED_CHECK_ARG(pn, "sync_beam_search: null pointer");
    const int BW = B * W, NODES = T * W;
    SearchNet net = sync_net_of(*pn, BW, W, NODES);
    const int dtype = net.dtype, J = net.J, V = net.V, L = net.pred.L, H = net.pred.H, blank = net.blank, bos = net.bos;
    ED_CHECK_ARG(W >= 1 && W <= SB_MAXW, "sync_beam_search: beam width W = %d outside [1, %d]", W, SB_MAXW);
    ED_CHECK_ARG(T > 0, "sync_beam_search: T = %d frames (must be > 0)", T);
    if (int rc = check_net(net, "sync_beam_search", sync_dims_ok(*pn, B, T, W) && max_tokens >= 0,
                           " (H must be a multiple of 4)",
                           E1 && lens_host && tokens_host && frames_host && token_logp_host && ntokens_host && nhyp_host &&
                               logp_host && workspace && result,
                           true))
        return rc;
    if (int rc = sync_layers_check(*pn, "sync_beam_search")) return rc;
    int maxlen = 0;
    if (int rc = check_lens(lens_host, B, T, "sync_beam_search", &maxlen)) return rc;
    if (int rc = sync_fuse_check(lm, bias, V, "sync_beam_search")) return rc;
    if (int rc = sync_ilm_check(ilm_weight, "sync_beam_search")) return rc;
    if (int rc = sync_ngram_check(ng, lm, V, blank, "sync_beam_search")) return rc;
    hipStream_t s = (hipStream_t)stream_;
    char* p = (char*)workspace;
    const SyncWs w = sync_layout(net, B, W, T);
    StepBufs u = bind(p + w.step_at, w.step);
    net.E1 = p + w.e1g;
    SyncPtrs q{};
    q.logp = at<double>(p, w.logp);
    q.node = at<int32_t>(p, w.node);
    q.hash = at<unsigned long long>(p, w.hash);
    q.len = at<int32_t>(p, w.len);
    q.pred = u.pred;
    q.hs[0] = at<float>(p, w.hs0); q.hs[1] = at<float>(p, w.hs1);
    q.cs[0] = at<float>(p, w.cs0); q.cs[1] = at<float>(p, w.cs1);
    q.c_score = at<double>(p, w.c_score);
    q.c_k = at<int32_t>(p, w.c_k);
    q.c_lp = at<float>(p, w.c_lp);
    q.nodes = at<int2>(p, w.nodes);
    q.nd_frame = at<int32_t>(p, w.nd_frame);
    q.nd_lp = at<float>(p, w.nd_lp);
    q.n_nodes = at<int32_t>(p, w.n_nodes);
    q.lens = at<int32_t>(p, w.lens);

    const size_t st = (size_t)BW * L * H * 4;
    ED_CHECK_HIP(hipMemcpyAsync(q.lens, lens_host, (size_t)B * 4, hipMemcpyHostToDevice, s));
    // the empty hypothesis' state is zero; both buffers, so that rows nothing writes stay finite in the step kernels
    ED_CHECK_HIP(hipMemsetAsync(q.hs[0], 0, st, s));
    ED_CHECK_HIP(hipMemsetAsync(q.hs[1], 0, st, s));
    ED_CHECK_HIP(hipMemsetAsync(q.cs[0], 0, st, s));
    ED_CHECK_HIP(hipMemsetAsync(q.cs[1], 0, st, s));
    hipLaunchKernelGGL(sync_init, dim3((BW + 255) / 256), dim3(256), 0, s, q, B, W, bos);
    SyncFusion fusion{};
    const SyncFusion* fu = nullptr;
    const size_t fuse_end =
        sync_fuse_rows_layout(sync_fuse_step_layout(w.total, BW, net.esz, V, lm).total, BW, lm, bias, ng).total;
    const size_t ilm_end = sync_ilm_layout(fuse_end, BW, net.esz, J, V, ilm_weight != nullptr).total;
    if (lm || bias || ng) {
        const SyncFuseStep wa = sync_fuse_step_layout(w.total, BW, net.esz, V, lm);
        const SyncFuseRows ra = sync_fuse_rows_layout(wa.total, BW, lm, bias, ng);
        const SyncNgramWs na = sync_ngram_ws_layout(ilm_end, BW, W, ng);
        fusion = sync_fuse_bind(p, ra, p, &wa, lm, bias, ng, &na);
        fu = &fusion;
        if (lm) {       // the empty sequence's LM state is zero, in both buffers as the prediction network's
            const size_t lst = (size_t)BW * lm->L * lm->H * 4;
            ED_CHECK_HIP(hipMemsetAsync(fusion.f.lm_hs[0], 0, lst, s));
            ED_CHECK_HIP(hipMemsetAsync(fusion.f.lm_hs[1], 0, lst, s));
            ED_CHECK_HIP(hipMemsetAsync(fusion.f.lm_cs[0], 0, lst, s));
            ED_CHECK_HIP(hipMemsetAsync(fusion.f.lm_cs[1], 0, lst, s));
        }
        hipLaunchKernelGGL(sync_init_fused, dim3((BW + 255) / 256), dim3(256), 0, s, fusion.f, BW);
    }
    const bool fused = ed_decode_fused_ok(dtype, net.pred.emb_dtype, J, V, net.pred.E, H, net.P2);
    SyncIlm ilm{};
    const SyncIlm* il = nullptr;
    if (ilm_weight) {
        const SyncIlmWs ia = sync_ilm_layout(fuse_end, BW, net.esz, J, V, true);
        ilm = sync_ilm_bind(p, ia, *ilm_weight, fused, BW, V, u);
        il = &ilm;
        ED_CHECK_HIP(hipMemsetAsync(p + ia.zero_row, 0, (size_t)J * net.esz, s));
    }
    int cur = 0;
    for (int t = 0; t < maxlen; ++t) {
        dispatch(dtype, [&](auto tag) {
            using ET = decltype(tag);
            hipLaunchKernelGGL(sync_gather<ET>, dim3(ed_grid_for((long long)BW * J, 256)), dim3(256), 0, s, (const ET*)E1,
                               e_row_stride, e_frame_stride, t, (ET*)(p + w.e1g), BW, W, J);
        });
        int rc = sync_step(fused, net, q.hs[cur], q.cs[cur], u, il, s);
        if (rc) return rc;
        if (fu && fu->lm &&
            (rc = ed_decode_lm_step(dtype, BW, fu->lm_net, fu->f.lm_hs[cur], fu->f.lm_cs[cur], fu->lmu, s)))
            return rc;
        sync_launch_pick<false>(q, fu, u, t, cur, W, B, L, H, NODES, V, blank, bos, nullptr, s, il);
        cur ^= 1;
    }
    // results: one read at the end - lengths and scores first, then only the used columns
    const SyncRes r = sync_result_layout(B, W, max_tokens);
    char* rp = (char*)result;
    hipLaunchKernelGGL(sync_read, dim3(B), dim3(64), 0, s, q, W, NODES, max_tokens, at<int32_t>(rp, r.nhyp),
                       at<int32_t>(rp, r.len), at<double>(rp, r.logp), at<int32_t>(rp, r.tok), at<int32_t>(rp, r.frame),
                       at<double>(rp, r.lp));
    ED_CHECK_LAUNCH("sync_beam_search");
    ED_CHECK_HIP(hipMemcpyAsync(nhyp_host, rp + r.nhyp, (size_t)B * 4, hipMemcpyDeviceToHost, s));
    ED_CHECK_HIP(hipMemcpyAsync(ntokens_host, rp + r.len, (size_t)BW * 4, hipMemcpyDeviceToHost, s));
    ED_CHECK_HIP(hipMemcpyAsync(logp_host, rp + r.logp, (size_t)BW * 8, hipMemcpyDeviceToHost, s));
    ED_CHECK_HIP(hipStreamSynchronize(s));
    int longest = 0;
    for (int b = 0; b < B; ++b)
        for (int j = 0; j < nhyp_host[b]; ++j) {
            const int len = ntokens_host[(size_t)b * W + j];
            ED_CHECK_ARG(len <= max_tokens, "sync_beam_search: hypothesis of %d tokens exceeds max_tokens = %d", len,
                         max_tokens);
            longest = std::max(longest, len);
        }
    if (longest > 0) {
        const size_t MT = (size_t)max_tokens;
        ED_CHECK_HIP(hipMemcpy2DAsync(tokens_host, MT * 4, rp + r.tok, MT * 4, (size_t)longest * 4, BW,
                                      hipMemcpyDeviceToHost, s));
        ED_CHECK_HIP(hipMemcpy2DAsync(frames_host, MT * 4, rp + r.frame, MT * 4, (size_t)longest * 4, BW,
                                      hipMemcpyDeviceToHost, s));
        ED_CHECK_HIP(hipMemcpy2DAsync(token_logp_host, MT * 8, rp + r.lp, MT * 8, (size_t)longest * 8, BW,
                                      hipMemcpyDeviceToHost, s));
        ED_CHECK_HIP(hipStreamSynchronize(s));
    }
    return ED_OK;
}

// ------------------------------------------------------------------------------------------------------------------
// Streaming form: the beams of S streams in a persistent STATE, advanced chunk by chunk (include/edgedict_hip.h states
// the contract).  The state is what SyncPtrs holds per utterance - the W rows' small fields, both state buffers, the
// token tree [S][NC] - plus per stream the frames since its reset and the tokens committed so far.  A frame is the
// offline loop's four launches (sync_stream_select = sync_select with the frame offset and the pass-through); after the
// last frame sync_stream_compact commits the path down to the live leaves' lowest common ancestor, re-roots the tree
// there and renumbers the nodes that a live leaf still reaches into [0, n_live).  hash / len / pred are over the whole
// sequence and stay as they are.  The beam stays in beam order; only the read-out (sync_read, unchanged) ranks it.
namespace {

struct SyncStreamState {
    size_t logp, node, hash, len, pred, hs0, hs1, cs0, cs1, nodes, nd_frame, nd_lp, n_nodes, frames_done, n_committed,
        total;
};
SyncStreamState sync_stream_state_layout(size_t S, size_t W, size_t L, size_t H, size_t NC) {
    SyncStreamState a{};
    const size_t SW = S * W;
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t r = o; o += align256(bytes); return r; };
    a.logp = take(SW * 8);
    a.node = take(SW * 4);
    a.hash = take(SW * 8);
    a.len = take(SW * 4);
    a.pred = take(SW * 4);
    a.hs0 = take(SW * L * H * 4);
    a.hs1 = take(SW * L * H * 4);
    a.cs0 = take(SW * L * H * 4);
    a.cs1 = take(SW * L * H * 4);
    a.nodes = take(S * NC * 8);
    a.nd_frame = take(S * NC * 4);
    a.nd_lp = take(S * NC * 4);
    a.n_nodes = take(S * 4);
    a.frames_done = take(S * 4);
    a.n_committed = take(S * 8);
    a.total = o;
    return a;
}

struct SyncStreamWs {
    Ws step;
    size_t step_at, e1g, c_score, c_k, c_lp, lens, remap, commit, total;
};
SyncStreamWs sync_stream_ws_layout(const SearchNet& rows, size_t S, size_t W, size_t NC) {
    SyncStreamWs w{};
    const size_t SW = S * W;
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t r = o; o += align256(bytes); return r; };
    w.step = ws_layout(rows);
    w.step_at = take(w.step.total);
    w.e1g = take(SW * rows.J * rows.esz);
    w.c_score = take(SW * W * 8);
    w.c_k = take(SW * W * 4);
    w.c_lp = take(SW * W * 4);
    w.lens = take(S * 4);
    w.remap = take(S * NC * 4);
    w.commit = take(S * (NC + 1) * 16);
    w.total = o;
    return w;
}

bool sync_stream_dims_ok(int S, int L, int H, int W, int NC) {
    return S > 0 && L > 0 && H > 0 && H % 4 == 0 && W >= 1 && W <= SB_MAXW && NC >= W &&
           (long long)S * W <= 0x7fffffff / 256 && (long long)S * ((long long)NC + 1) <= 0x7fffffff / 16;
}

// the state's part of SyncPtrs (the candidate lists and the lengths are per call: the workspace)
SyncPtrs sync_stream_bind(char* st, const SyncStreamState& a) {
    SyncPtrs q{};
    q.logp = at<double>(st, a.logp);
    q.node = at<int32_t>(st, a.node);
    q.hash = at<unsigned long long>(st, a.hash);
    q.len = at<int32_t>(st, a.len);
    q.pred = at<int32_t>(st, a.pred);
    q.hs[0] = at<float>(st, a.hs0); q.hs[1] = at<float>(st, a.hs1);
    q.cs[0] = at<float>(st, a.cs0); q.cs[1] = at<float>(st, a.cs1);
    q.nodes = at<int2>(st, a.nodes);
    q.nd_frame = at<int32_t>(st, a.nd_frame);
    q.nd_lp = at<float>(st, a.nd_lp);
    q.n_nodes = at<int32_t>(st, a.n_nodes);
    return q;
}

// One workgroup per stream s0 + blockIdx.x (mask: device int32 [S] or null): the empty hypothesis in row 0, zero states
// in BOTH buffers (whichever the next advance reads), an empty tree, no frames, nothing committed.
__global__ __launch_bounds__(256) void sync_stream_reset_kernel(SyncPtrs p, int32_t* __restrict__ frames_done,
                                                                long long* __restrict__ n_committed,
                                                                const int32_t* __restrict__ mask, int s0, int S, int W,
                                                                int L, int H, int bos) {
    const int b = s0 + blockIdx.x, tid = threadIdx.x, r0 = b * W;
    if (b >= S || (mask && !mask[b])) return;
    if (tid < W) {
        p.logp[r0 + tid] = tid == 0 ? 0.0 : -(double)INFINITY;
        p.node[r0 + tid] = -1;
        p.hash[r0 + tid] = SB_HASH0;
        p.len[r0 + tid] = 0;
        p.pred[r0 + tid] = bos;
    }
    if (tid == 0) {
        p.n_nodes[b] = 0;
        frames_done[b] = 0;
        n_committed[b] = 0;
    }
    const int H4 = H / 4, LH4 = L * H4;
    const size_t SW = (size_t)S * W;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int idx = tid; idx < W * LH4; idx += 256) {
        const int pos = idx / LH4, rem = idx % LH4, l = rem / H4, j = rem % H4;
        const size_t at = ((size_t)l * SW + r0 + pos) * H4 + j;
        ((float4*)p.hs[0])[at] = zero; ((float4*)p.hs[1])[at] = zero;
        ((float4*)p.cs[0])[at] = zero; ((float4*)p.cs[1])[at] = zero;
    }
}

// The fused forms' part of a reset, for the same streams: zero LM states in both buffers, the LM's next symbol lm_bos,
// the automaton's root.
__global__ __launch_bounds__(256) void sync_stream_reset_fused_kernel(SyncFuse f, const int32_t* __restrict__ mask,
                                                                      int s0, int S, int W) {
    const int b = s0 + blockIdx.x, tid = threadIdx.x, r0 = b * W;
    if (b >= S || (mask && !mask[b])) return;
    if (tid < W) {
        if (f.lm_pred) f.lm_pred[r0 + tid] = f.lm_bos;
        if (f.bias_st) f.bias_st[r0 + tid] = 0;
        if (f.ng_st) f.ng_st[r0 + tid] = f.ng_start;
    }
    if (!f.lm_pred) return;
    const int H4 = f.lm_H / 4, LH4 = f.lm_L * H4;
    const size_t SW = (size_t)S * W;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int idx = tid; idx < W * LH4; idx += 256) {
        const int pos = idx / LH4, rem = idx % LH4, l = rem / H4, j = rem % H4;
        const size_t at = ((size_t)l * SW + r0 + pos) * H4 + j;
        ((float4*)f.lm_hs[0])[at] = zero; ((float4*)f.lm_hs[1])[at] = zero;
        ((float4*)f.lm_cs[0])[at] = zero; ((float4*)f.lm_cs[1])[at] = zero;
    }
}

// One wave per stream, once per advance, after the last frame.  Node ids grow with creation and a parent is older than
// its child, which a dense renumbering in index order keeps: every walk towards the root strictly descends.
//   1. lane j = row j: the depth of its leaf; all live rows climb to the smallest depth, then together until they
//      stand on one node - the lowest common ancestor (the root, -1, as soon as one live row sits on it);
//   2. lane 0 writes the path root -> ancestor into the commit records (token, frame, lp), record 0 = the counts;
//   3. the nodes between a live leaf and the ancestor are marked, numbered by a running count over the marks, and moved
//      down to their numbers with their parents renamed (the ancestor's children get parent -1); a chunk of 64 nodes
//      is read whole before any of it is written, and a node never moves up, so nothing unread is overwritten;
//   4. the rows' leaves are renamed, the stream's counters advance.
// No atomics; the result depends on the tree alone.  `remap`: int32 [S][NC] scratch.
__global__ __launch_bounds__(64) void sync_stream_compact(SyncPtrs p, int32_t* __restrict__ frames_done,
                                                          long long* __restrict__ n_committed,
                                                          int32_t* __restrict__ remap, int4* __restrict__ commit, int W,
                                                          int NC) {
    const int b = blockIdx.x, lane = threadIdx.x, r0 = b * W;
    int2* tree = p.nodes + (size_t)b * NC;
    int32_t* nfr = p.nd_frame + (size_t)b * NC;
    float* nlp = p.nd_lp + (size_t)b * NC;
    int32_t* map = remap + (size_t)b * NC;
    int4* out = commit + (size_t)b * (NC + 1);
    const int n = min(max(p.n_nodes[b], 0), NC);
    const bool live = lane < W && p.logp[r0 + min(lane, W - 1)] != -(double)INFINITY;
    int leaf = live ? p.node[r0 + lane] : -1;
    if (leaf >= n) leaf = -1;               // (cannot happen on a state the advances wrote)
    // 1.
    int d = 0;
    for (int nd = leaf; nd >= 0 && d < n; nd = tree[nd].x) ++d;
    int dmin = live ? d : 0x7fffffff;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) dmin = min(dmin, __shfl_xor(dmin, off, 64));
    const unsigned long long m_live = __ballot(live);
    if (m_live == 0ull) dmin = 0;
    int a = leaf;
    for (int k = d; live && k > dmin && a >= 0; --k) a = tree[a].x;
    const int first = m_live ? __ffsll((unsigned long long)m_live) - 1 : 0;
    while (dmin > 0) {
        const int a0 = __shfl(a, first, 64);
        if (__ballot(live && a != a0) == 0ull) break;
        if (live && a >= 0) a = tree[a].x;
        --dmin;
    }
    const int lca = dmin > 0 ? __shfl(a, first, 64) : -1;
    // 2.
    if (lane == 0) {
        int k = dmin;
        for (int nd = lca; nd >= 0 && k > 0; nd = tree[nd].x) {
            --k;
            out[1 + k] = make_int4(tree[nd].y, nfr[nd], __float_as_int(nlp[nd]), 0);
        }
    }
    // 3.
    for (int i = lane; i < n; i += 64) map[i] = 0;
    __syncthreads();
    if (live) {
        int steps = 0;
        for (int nd = leaf; nd >= 0 && nd != lca && steps < n; nd = tree[nd].x, ++steps) map[nd] = 1;
    }
    __syncthreads();
    const unsigned long long below = (1ull << lane) - 1ull;
    int n_live = 0;
    for (int i0 = 0; i0 < n; i0 += 64) {
        const int i = i0 + lane;
        const bool m = i < n && map[i] != 0;
        const unsigned long long bal = __ballot(m);
        if (i < n) map[i] = m ? n_live + __popcll(bal & below) : -1;
        n_live += __popcll(bal);
    }
    __syncthreads();
    for (int i0 = 0; i0 < n; i0 += 64) {
        const int i = i0 + lane;
        const int id = i < n ? map[i] : -1;
        int2 nd = make_int2(-1, 0);
        int fr = 0;
        float lp = 0.f;
        if (id >= 0) {
            nd = tree[i];
            fr = nfr[i];
            lp = nlp[i];
            nd.x = (nd.x < 0 || nd.x == lca) ? -1 : map[nd.x];
        }
        __syncthreads();
        if (id >= 0) {
            tree[id] = nd;
            nfr[id] = fr;
            nlp[id] = lp;
        }
        __syncthreads();
    }
    // 4.
    if (live) p.node[r0 + lane] = (leaf < 0 || leaf == lca) ? -1 : map[leaf];
    if (lane == 0) {
        p.n_nodes[b] = n_live;
        frames_done[b] += p.lens[b];
        n_committed[b] += dmin;
        out[0] = make_int4(dmin, n_live, 0, 0);
    }
}

}  // namespace

// The fused forms append the rows' LM (h, c) in both buffers, the LM's next symbols and the automaton states behind the
// plain state, and the LM step's buffers behind the plain workspace: edgedict_sync_stream_read serves every form.
// (V is not known to the state query: the LM's own V sizes nothing there.)
extern "C" size_t edgedict_sync_stream_state_bytes(const edgedict_search_opts_t* opts, int S, int L, int H, int W,
                                                   int node_capacity) {
    if (!search_ptrs_ok(nullptr, opts)) return 0;
    const edgedict_search_opts_t o = search_opts_of(opts);
    if (!sync_stream_dims_ok(S, L, H, W, node_capacity) || !sync_fuse_dims_ok(o.lm, o.bias, o.lm ? o.lm->V : 0)) return 0;
    if (sync_ngram_check(o.ngram, o.lm, -1, -1, "sync_stream_state_bytes")) return 0;
    return sync_fuse_rows_layout(sync_stream_state_layout(S, W, L, H, node_capacity).total, (size_t)S * W, o.lm, o.bias,
                                 o.ngram)
        .total;
}

// the plain size; an LM appends its step's buffers, ILME its own behind them.  (The persistent state has no ILME part.)
extern "C" size_t edgedict_sync_stream_workspace_bytes(const edgedict_search_net_t* pn, int S, int W, int node_capacity,
                                                       const edgedict_search_opts_t* opts) {
    if (!pn || !search_ptrs_ok(pn, opts)) return 0;
    const edgedict_search_opts_t o = search_opts_of(opts);
    if (!sync_stream_dims_ok(S, pn->L, pn->H, W, node_capacity) || !sync_dims_ok(*pn, S, 1, W) ||
        !sync_fuse_dims_ok(o.lm, o.bias, pn->V) || !sync_ilm_ok(o.ilm_weight))
        return 0;
    if (sync_ngram_check(o.ngram, o.lm, pn->V, pn->blank, "sync_stream_workspace_bytes")) return 0;
    const SearchNet net = sync_net_of(*pn, S * W, W, node_capacity);
    const size_t SW = (size_t)S * W, esz = net.esz;
    const size_t plain = sync_stream_ws_layout(net, S, W, node_capacity).total;
    const size_t ilm = sync_ilm_layout(sync_fuse_step_layout(plain, SW, esz, net.V, o.lm).total, SW, esz, net.J, net.V,
                                       o.ilm_weight != nullptr)
                           .total;
    return sync_ngram_ws_layout(ilm, SW, W, o.ngram).total;
}

extern "C" size_t edgedict_sync_stream_result_bytes(int S, int W, int max_tokens) {
    if (S <= 0 || W < 1 || W > SB_MAXW || max_tokens < 0) return 0;
    return sync_result_layout(S, W, max_tokens).total;
}

#define SYNC_STREAM_CHECK_SHAPE(what, S, L, H, W, NC)                                                              \
    do {                                                                                                           \
        ED_CHECK_ARG(W >= 1 && W <= SB_MAXW, what ": beam width W = %d outside [1, %d]", W, SB_MAXW);              \
        ED_CHECK_ARG(S > 0, what ": S = %d streams (must be > 0)", S);                                             \
        ED_CHECK_ARG(NC >= W, what ": node_capacity = %d is too small (must be >= W = %d)", NC, W);                \
        ED_CHECK_ARG(L > 0 && H > 0 && H % 4 == 0, what ": bad shape (H = %d must be a positive multiple of 4)", H); \
        ED_CHECK_ARG(sync_stream_dims_ok(S, L, H, W, NC), what ": bad shape (too many rows or nodes)");            \
    } while (0)

// opts->lm / bias null: the plain reset.  (The LM's and the list's vocabulary are the advance's to check: V is not known
// here.  ILME carries no state: opts->ilm_weight is not read.)
extern "C" int edgedict_sync_stream_reset(const edgedict_search_opts_t* opts, int S, int L, int H, int W,
                                          int node_capacity, int bos, const int32_t* mask, int mask_on_host, void* state,
                                          void* stream_) {
    ED_CHECK_ARG(search_ptrs_ok(nullptr, opts), "sync_stream_reset: opts is not a pointer");
    const edgedict_search_opts_t o = search_opts_of(opts);
    const edgedict_beam_lm_t* lm = o.lm;
    const edgedict_beam_bias_t* bias = o.bias;
    const edgedict_ngram_lm_t* ng = o.ngram;
    SYNC_STREAM_CHECK_SHAPE("sync_stream_reset", S, L, H, W, node_capacity);
    ED_CHECK_ARG(bos >= 0, "sync_stream_reset: bos = %d outside the vocabulary", bos);
    ED_CHECK_ARG(state, "sync_stream_reset: null pointer (state)");
    if (int rc = sync_fuse_check(lm, bias, lm ? lm->V : (bias ? bias->V : 0), "sync_stream_reset")) return rc;
    if (int rc = sync_ngram_check(ng, lm, -1, -1, "sync_stream_reset")) return rc;
    hipStream_t s = (hipStream_t)stream_;
    char* st = (char*)state;
    const SyncStreamState a = sync_stream_state_layout(S, W, L, H, node_capacity);
    const SyncPtrs q = sync_stream_bind(st, a);
    int32_t* frames_done = at<int32_t>(st, a.frames_done);
    long long* n_committed = at<long long>(st, a.n_committed);
    SyncFusion fusion{};
    const bool any_fused = lm || bias || ng;
    if (any_fused)
        fusion = sync_fuse_bind(st, sync_fuse_rows_layout(a.total, (size_t)S * W, lm, bias, ng), nullptr, nullptr, lm, bias,
                                ng);
    if (!mask || !mask_on_host) {
        hipLaunchKernelGGL(sync_stream_reset_kernel, dim3(S), dim3(256), 0, s, q, frames_done, n_committed, mask, 0, S, W,
                           L, H, bos);
        if (any_fused)
            hipLaunchKernelGGL(sync_stream_reset_fused_kernel, dim3(S), dim3(256), 0, s, fusion.f, mask, 0, S, W);
    } else {            // host mask: one launch per run of selected streams
        for (int b = 0; b < S;) {
            if (!mask[b]) { ++b; continue; }
            int e = b;
            while (e < S && mask[e]) ++e;
            hipLaunchKernelGGL(sync_stream_reset_kernel, dim3(e - b), dim3(256), 0, s, q, frames_done, n_committed,
                               (const int32_t*)nullptr, b, S, W, L, H, bos);
            if (any_fused)
                hipLaunchKernelGGL(sync_stream_reset_fused_kernel, dim3(e - b), dim3(256), 0, s, fusion.f,
                                   (const int32_t*)nullptr, b, S, W);
            b = e;
        }
    }
    ED_CHECK_LAUNCH("sync_stream_reset");
    return ED_OK;
}

// opts null or all its members null: the plain advance, launch for launch;  ilm_weight null: the advance without ILME
extern "C" int edgedict_sync_stream_advance(const edgedict_search_net_t* pn, const void* E1, long long e_row_stride,
                                            long long e_frame_stride, int S, int T, const int32_t* n_frames_host, int W,
                                            int node_capacity, int32_t* live_host, int32_t* parity_host,
                                            void* commit_host, int max_commit, const edgedict_search_opts_t* opts,
                                            void* state, void* workspace, void* stream_) {
    const int NC = node_capacity;
    ED_CHECK_ARG(search_ptrs_ok(pn, opts), "sync_stream_advance: net / opts is not a pointer");
    const edgedict_search_opts_t o = search_opts_of(opts);
    const edgedict_beam_lm_t* lm = o.lm;
    const edgedict_beam_bias_t* bias = o.bias;
    const double* ilm_weight = o.ilm_weight;
    const edgedict_ngram_lm_t* ng = o.ngram;
    ED_CHECK_ARG(pn, "sync_stream_advance: null pointer");
    const int SW = S * W;
    SearchNet net = sync_net_of(*pn, SW, W, NC);
    const int dtype = net.dtype, J = net.J, V = net.V, L = net.pred.L, H = net.pred.H, blank = net.blank, bos = net.bos;
    SYNC_STREAM_CHECK_SHAPE("sync_stream_advance", S, L, H, W, NC);
    ED_CHECK_ARG(T >= 0, "sync_stream_advance: T = %d frames (must be >= 0)", T);
    if (int rc = check_net(net, "sync_stream_advance", sync_dims_ok(*pn, S, 1, W) && max_commit >= 0, "",
                           (E1 || T == 0) && n_frames_host && live_host && parity_host && commit_host && state && workspace,
                           true))
        return rc;
    if (int rc = sync_layers_check(*pn, "sync_stream_advance")) return rc;
    ED_CHECK_ARG(*parity_host == 0 || *parity_host == 1, "sync_stream_advance: parity = %d (0 or 1)", *parity_host);
    int maxlen = 0, cols = 0;
    for (int b = 0; b < S; ++b) {
        const int nf = n_frames_host[b];
        ED_CHECK_ARG(nf >= 0 && nf <= T, "sync_stream_advance: n_frames[%d] = %d outside [0, %d]", b, nf, T);
        ED_CHECK_ARG(live_host[b] >= 0 && live_host[b] <= NC, "sync_stream_advance: live[%d] = %d outside [0, %d]", b,
                     live_host[b], NC);
        ED_CHECK_ARG((long long)live_host[b] + (long long)nf * W <= NC,
                     "sync_stream_advance: stream %d may need %lld token-tree nodes (%d live + %d frames x W = %d), "
                     "node_capacity is %d",
                     b, (long long)live_host[b] + (long long)nf * W, live_host[b], nf, W, NC);
        maxlen = std::max(maxlen, nf);
        cols = std::max(cols, std::min(NC, live_host[b] + nf));
    }
    ED_CHECK_ARG(cols <= max_commit, "sync_stream_advance: max_commit = %d, this advance may commit %d tokens",
                 max_commit, cols);
    if (int rc = sync_fuse_check(lm, bias, V, "sync_stream_advance")) return rc;
    if (int rc = sync_ilm_check(ilm_weight, "sync_stream_advance")) return rc;
    if (int rc = sync_ngram_check(ng, lm, V, blank, "sync_stream_advance")) return rc;
    hipStream_t s = (hipStream_t)stream_;
    char* p = (char*)workspace;
    char* st = (char*)state;
    const SyncStreamWs w = sync_stream_ws_layout(net, S, W, NC);
    const SyncStreamState a = sync_stream_state_layout(S, W, L, H, NC);
    StepBufs u = bind(p + w.step_at, w.step);
    net.E1 = p + w.e1g;
    SyncPtrs q = sync_stream_bind(st, a);
    u.pred = q.pred;            // the step reads the rows' last tokens where the state keeps them
    q.c_score = at<double>(p, w.c_score);
    q.c_k = at<int32_t>(p, w.c_k);
    q.c_lp = at<float>(p, w.c_lp);
    q.lens = at<int32_t>(p, w.lens);
    int32_t* frames_done = at<int32_t>(st, a.frames_done);
    SyncFusion fusion{};
    const SyncFusion* fu = nullptr;
    if (lm || bias || ng) {
        const SyncFuseStep wa = sync_fuse_step_layout(w.total, SW, net.esz, V, lm);
        const SyncNgramWs na =
            sync_ngram_ws_layout(sync_ilm_layout(wa.total, SW, net.esz, J, V, ilm_weight != nullptr).total, SW, W, ng);
        fusion = sync_fuse_bind(st, sync_fuse_rows_layout(a.total, SW, lm, bias, ng), p, &wa, lm, bias, ng, &na);
        fu = &fusion;
    }

    ED_CHECK_HIP(hipMemcpyAsync(q.lens, n_frames_host, (size_t)S * 4, hipMemcpyHostToDevice, s));
    const bool fused = ed_decode_fused_ok(dtype, net.pred.emb_dtype, J, V, net.pred.E, H, net.P2);
    SyncIlm ilm{};
    const SyncIlm* il = nullptr;
    if (ilm_weight) {
        const SyncIlmWs ia =
            sync_ilm_layout(sync_fuse_step_layout(w.total, SW, net.esz, V, lm).total, SW, net.esz, J, V, true);
        ilm = sync_ilm_bind(p, ia, *ilm_weight, fused, SW, V, u);
        il = &ilm;
        if (maxlen > 0) ED_CHECK_HIP(hipMemsetAsync(p + ia.zero_row, 0, (size_t)J * net.esz, s));
    }
    int cur = *parity_host;
    for (int t = 0; t < maxlen; ++t) {
        dispatch(dtype, [&](auto tag) {
            using ET = decltype(tag);
            hipLaunchKernelGGL(sync_gather<ET>, dim3(ed_grid_for((long long)SW * J, 256)), dim3(256), 0, s, (const ET*)E1,
                               e_row_stride, e_frame_stride, t, (ET*)(p + w.e1g), SW, W, J);
        });
        int rc = sync_step(fused, net, q.hs[cur], q.cs[cur], u, il, s);
        if (rc) return rc;
        if (fu && fu->lm &&
            (rc = ed_decode_lm_step(dtype, SW, fu->lm_net, fu->f.lm_hs[cur], fu->f.lm_cs[cur], fu->lmu, s)))
            return rc;
        sync_launch_pick<true>(q, fu, u, t, cur, W, S, L, H, NC, V, blank, bos, (const int32_t*)frames_done, s, il);
        cur ^= 1;
    }
    hipLaunchKernelGGL(sync_stream_compact, dim3(S), dim3(64), 0, s, q, frames_done, at<long long>(st, a.n_committed),
                       at<int32_t>(p, w.remap), at<int4>(p, w.commit), W, NC);
    ED_CHECK_LAUNCH("sync_stream_advance");
    *parity_host = cur;
    // the one read of the advance: every stream's counts and the records this advance can have written
    ED_CHECK_HIP(hipMemcpy2DAsync(commit_host, ((size_t)max_commit + 1) * 16, p + w.commit, ((size_t)NC + 1) * 16,
                                  ((size_t)cols + 1) * 16, S, hipMemcpyDeviceToHost, s));
    ED_CHECK_HIP(hipStreamSynchronize(s));
    const int32_t* rec = (const int32_t*)commit_host;
    for (int b = 0; b < S; ++b) live_host[b] = rec[(size_t)b * ((size_t)max_commit + 1) * 4 + 1];
    return ED_OK;
}

extern "C" int edgedict_sync_stream_read(int S, int L, int H, int W, int node_capacity, const void* state, void* result,
                                         int32_t* tokens_host, int32_t* frames_host, double* token_logp_host,
                                         int max_tokens, int32_t* ntokens_host, int32_t* nhyp_host, double* logp_host,
                                         long long* ncommitted_host, long long* nframes_host, void* stream_) {
    const int NC = node_capacity;
    SYNC_STREAM_CHECK_SHAPE("sync_stream_read", S, L, H, W, NC);
    ED_CHECK_ARG(max_tokens >= 0, "sync_stream_read: max_tokens = %d (must be >= 0)", max_tokens);
    ED_CHECK_ARG(state && result && tokens_host && ntokens_host && nhyp_host && logp_host,
                 "sync_stream_read: null pointer");
    hipStream_t s = (hipStream_t)stream_;
    char* st = (char*)state;            // (read only: sync_read writes the result alone)
    const SyncStreamState a = sync_stream_state_layout(S, W, L, H, NC);
    const SyncPtrs q = sync_stream_bind(st, a);
    const SyncRes r = sync_result_layout(S, W, max_tokens);
    char* rp = (char*)result;
    const int SW = S * W;
    hipLaunchKernelGGL(sync_read, dim3(S), dim3(64), 0, s, q, W, NC, max_tokens, at<int32_t>(rp, r.nhyp),
                       at<int32_t>(rp, r.len), at<double>(rp, r.logp), at<int32_t>(rp, r.tok), at<int32_t>(rp, r.frame),
                       at<double>(rp, r.lp));
    ED_CHECK_LAUNCH("sync_stream_read");
    ED_CHECK_HIP(hipMemcpyAsync(nhyp_host, rp + r.nhyp, (size_t)S * 4, hipMemcpyDeviceToHost, s));
    ED_CHECK_HIP(hipMemcpyAsync(ntokens_host, rp + r.len, (size_t)SW * 4, hipMemcpyDeviceToHost, s));
    ED_CHECK_HIP(hipMemcpyAsync(logp_host, rp + r.logp, (size_t)SW * 8, hipMemcpyDeviceToHost, s));
    std::vector<int32_t> fd;
    if (nframes_host) {
        fd.resize(S);
        ED_CHECK_HIP(hipMemcpyAsync(fd.data(), st + a.frames_done, (size_t)S * 4, hipMemcpyDeviceToHost, s));
    }
    if (ncommitted_host)
        ED_CHECK_HIP(hipMemcpyAsync(ncommitted_host, st + a.n_committed, (size_t)S * 8, hipMemcpyDeviceToHost, s));
    ED_CHECK_HIP(hipStreamSynchronize(s));
    if (nframes_host)
        for (int b = 0; b < S; ++b) nframes_host[b] = fd[b];
    int longest = 0;
    for (int b = 0; b < S; ++b)
        for (int j = 0; j < nhyp_host[b]; ++j) {
            const int len = ntokens_host[(size_t)b * W + j];
            ED_CHECK_ARG(len <= max_tokens, "sync_stream_read: tail of %d tokens exceeds max_tokens = %d", len, max_tokens);
            longest = std::max(longest, len);
        }
    if (longest > 0) {
        // the used columns only - or, where the rows are short (the caller sizes max_tokens by the live trees), the
        // whole arrays in one piece each: a 2-D copy of S W short rows costs more than the bytes it saves
        const size_t MT = (size_t)max_tokens;
        const bool whole = (size_t)SW * MT * 8 <= ((size_t)1 << 20);
        auto fetch = [&](void* dst, const char* src, size_t esz) -> hipError_t {
            if (!dst) return hipSuccess;
            if (whole) return hipMemcpyAsync(dst, src, (size_t)SW * MT * esz, hipMemcpyDeviceToHost, s);
            return hipMemcpy2DAsync(dst, MT * esz, src, MT * esz, (size_t)longest * esz, SW, hipMemcpyDeviceToHost, s);
        };
        ED_CHECK_HIP(fetch(tokens_host, rp + r.tok, 4));
        ED_CHECK_HIP(fetch(frames_host, rp + r.frame, 4));
        ED_CHECK_HIP(fetch(token_logp_host, rp + r.lp, 8));
        ED_CHECK_HIP(hipStreamSynchronize(s));
    }
    return ED_OK;
}
