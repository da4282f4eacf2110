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
#include "decode_net.hpp"

#include <algorithm>

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
template <bool CACHED>
__global__ __launch_bounds__(256) void sync_row_topw(SyncPtrs p, const float* __restrict__ logits, int t, int W, int V) {
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
    double sc[SB_VPT];
    if constexpr (CACHED) {
#pragma unroll
        for (int i = 0; i < SB_VPT; ++i) {
            const int v = tid + 256 * i;
            sc[i] = v < V ? base + (double)((z[v] - m) - logs) : -(double)INFINITY;
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
                const double c = base + (double)((z[v] - m) - logs);
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
    }
}

// One workgroup per utterance.  Wave 0, lane j = the j-th kept candidate: a W-way merge of the rows' sorted lists picks
// the W best in order (ties: the lower row, inside a row the list's order), equal sequences are paired and folded, the
// survivors close ranks, token children get their tree nodes, and the beam's small fields are rewritten in place (every
// read of them comes before the first write, all inside this wave).  Then the whole workgroup gathers the states into
// the other buffer: a blank child takes its parent's state before the token, a token child the state after it.
__global__ __launch_bounds__(256) void sync_select(SyncPtrs p, const float* __restrict__ h_new,
                                                   const float* __restrict__ c_new, int t, int cur, int W, int B, int L,
                                                   int H, int NODES, int blank, int bos) {
    const int b = blockIdx.x, tid = threadIdx.x, r0 = b * W;
    if (t >= p.lens[b]) return;
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
        const int is_blank = k == blank;
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
                    p.nd_frame[(size_t)b * NODES + nid] = t;
                    p.nd_lp[(size_t)b * NODES + nid] = f_lp;
                }
                p.node[row] = nid;
                p.pred[row] = f_k;
                s_src[pos] = f_i | 0x100;
            }
        }
        if (lane >= n_new && lane < W) {
            const int row = r0 + lane;
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

SearchNet sync_dims(int dtype, int rows, int J, int V, int E, int L, int H, int P2) {
    SearchNet n{};
    n.dtype = dtype; n.esz = dtype == ED_F32 ? 4 : 2;
    n.B = rows; n.J = J; n.V = V; n.P2 = P2;
    n.pred.V = V; n.pred.E = E; n.pred.L = L; n.pred.H = H; n.pred.O = P2;
    return n;
}
bool sync_dims_ok(int dtype, int B, int T, int J, int V, int E, int L, int H, int P2, int W) {
    return (dtype == ED_F32 || dtype == ED_BF16) && B > 0 && T > 0 && J > 0 && V > 0 && E > 0 && L > 0 && H > 0 &&
           H % 4 == 0 && P2 > 0 && W >= 1 && W <= SB_MAXW && (long long)B * W <= 0x7fffffff / 256;
}

}  // namespace

extern "C" size_t edgedict_sync_beam_workspace_bytes(int dtype, int B, int T, int J, int V, int E, int L, int H, int P2,
                                                     int W) {
    if (!sync_dims_ok(dtype, B, T, J, V, E, L, H, P2, W)) return 0;
    return sync_layout(sync_dims(dtype, B * W, J, V, E, L, H, P2), B, W, T).total;
}

extern "C" size_t edgedict_sync_beam_result_bytes(int B, int W, int max_tokens) {
    if (B <= 0 || W <= 0 || max_tokens < 0) return 0;
    return sync_result_layout(B, W, max_tokens).total;
}

extern "C" int edgedict_sync_beam_search(
    int dtype, const void* E1, long long e_row_stride, long long e_frame_stride, int B, int T,
    const int32_t* lens_host, int J, const void* W1d, long long ldw1, const float* b1, int P2,
    const void* W2, const float* b2, int V, const void* emb, int emb_dtype, int E, int L,
    const void* const* w_ih, const void* const* w_hh, const float* const* b_ih,
    const float* const* b_hh, int H, const void* Wp, const float* bp, int blank, int bos, int W,
    int32_t* tokens_host, int32_t* frames_host, double* token_logp_host, int max_tokens, int32_t* ntokens_host,
    int32_t* nhyp_host, double* logp_host, void* workspace, void* result, void* stream_) {
    ED_CHECK_ARG(dtype == ED_F32 || dtype == ED_BF16, "sync_beam_search: bad dtype");
    ED_CHECK_ARG(W >= 1 && W <= SB_MAXW, "sync_beam_search: beam width W = %d outside [1, %d]", W, SB_MAXW);
    ED_CHECK_ARG(T > 0, "sync_beam_search: T = %d frames (must be > 0)", T);
    ED_CHECK_ARG(sync_dims_ok(dtype, B, T, J, V, E, L, H, P2, W) && max_tokens >= 0, "sync_beam_search: bad shape (H must be a multiple of 4)");
    ED_CHECK_ARG(E1 && lens_host && W1d && b1 && W2 && b2 && emb && w_ih && w_hh && b_ih && b_hh && Wp && bp &&
                     tokens_host && frames_host && token_logp_host && ntokens_host && nhyp_host && logp_host &&
                     workspace && result,
                 "sync_beam_search: null pointer");
    for (int k = 0; k < L; ++k)
        ED_CHECK_ARG(w_ih[k] && w_hh[k] && b_ih[k] && b_hh[k], "sync_beam_search: null pointer (layer %d)", k);
    ED_CHECK_ARG(emb_dtype == ED_F32 || emb_dtype == ED_BF16, "sync_beam_search: bad embedding dtype");
    ED_CHECK_ARG(blank >= 0 && blank < V && bos >= 0 && bos < V, "sync_beam_search: blank/bos outside the vocabulary");
    int maxlen = 0;
    for (int b = 0; b < B; ++b) {
        ED_CHECK_ARG(lens_host[b] >= 0 && lens_host[b] <= T, "sync_beam_search: lens[%d] = %d outside [0, %d]", b,
                     lens_host[b], T);
        maxlen = std::max(maxlen, lens_host[b]);
    }
    hipStream_t s = (hipStream_t)stream_;
    const int BW = B * W, NODES = T * W;
    // the step's network: B * W rows whose joint rows are gathered per frame, J apart
    char* p = (char*)workspace;
    SearchNet net{dtype, dtype == ED_F32 ? 4 : 2, nullptr, (long long)J, 0, BW, J, W1d, ldw1, b1, P2, W2, b2, V,
                  {emb, emb_dtype, V, E, L, w_ih, w_hh, b_ih, b_hh, H, Wp, bp, P2}, blank, bos, W, 0, NODES};
    const SyncWs w = sync_layout(net, B, W, T);
    const StepBufs u = bind(p + w.step_at, w.step);
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
    const bool fused = ed_decode_fused_ok(dtype, emb_dtype, J, V, E, H, P2);
    int cur = 0;
    for (int t = 0; t < maxlen; ++t) {
        dispatch(dtype, [&](auto tag) {
            using ET = decltype(tag);
            hipLaunchKernelGGL(sync_gather<ET>, dim3(ed_grid_for((long long)BW * J, 256)), dim3(256), 0, s, (const ET*)E1,
                               e_row_stride, e_frame_stride, t, (ET*)(p + w.e1g), BW, W, J);
        });
        int rc;
        if (fused) rc = ed_decode_fused_beam_step(net, net.E1, q.hs[cur], q.cs[cur], u, s);
        else rc = ed_decode_composed_beam_step(net, net.E1, q.hs[cur], q.cs[cur], u, s);
        if (rc) return rc;
        if (V <= 256 * SB_VPT) hipLaunchKernelGGL(sync_row_topw<true>, dim3(BW), dim3(256), 0, s, q, u.logits, t, W, V);
        else hipLaunchKernelGGL(sync_row_topw<false>, dim3(BW), dim3(256), 0, s, q, u.logits, t, W, V);
        hipLaunchKernelGGL(sync_select, dim3(B), dim3(256), 0, s, q, u.h_new, u.c_new, t, cur, W, B, L, H, NODES, blank,
                           bos);
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
