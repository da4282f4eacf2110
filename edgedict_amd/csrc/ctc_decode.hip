// CTC prefix beam search on the encoder's CTC head for gfx950, with N-best read-out and contextual biasing.
//
// THE SEARCH (per utterance, scores are fp64 log-probabilities, -inf is zero).  A hypothesis is a node of a token tree
// (parent, token, frame it was created on), node 0 the empty prefix.  It carries pb / pnb, the log-probability of its
// paths that end in blank / in its last token; tot = logadd(pb, pnb).  The beam starts as [root: pb 0, pnb -inf].
// For every frame t < T_b, with lp = log_softmax(z[b, t]):
//   1. candidates  C_t = the K = min(cand, V - 1) non-blank tokens of largest lp, in that order (ties: lower id)
//   2. stay        entry i (node n_i, last token e_i):  pb' = tot_i + lp[blank];  pnb' = pnb_i + lp[e_i] (not the root)
//   3. extend      entry i, candidate c:  p = (c == e_i ? pb_i : tot_i) + lp[c];  if the prefix (n_i, c) is beam entry j
//                  (node j has parent n_i and token c) then pnb'_j = logadd(pnb'_j, p), else it is a NEW candidate with
//                  pb = -inf, pnb = p.  Nothing else is credited to a new prefix (no resurrection term).  A candidate
//                  with p = -inf is no candidate.
//   4. select      the W best by logadd(pb', pnb') (+ the node's bias total Bn); ties go to the lower canonical index:
//                  the stays in beam order, then the new candidates in (i, c) order.  The new beam is in ranked order;
//                  only selected new candidates become nodes, so a tree has at most 1 + T_b W nodes.
// After the last frame the beam is the N-best list.  BIAS: a node carries the phrase automaton's state after its token,
// s = goto(s(parent), token), and Bn = Bn(parent) + D(s(parent), token), D(s, k) = held[goto(s, k)] - pend[s]; Bn enters
// the ranking and the reported logp only, pb / pnb stay pure CTC.  Pruning to C_t happens BEFORE the bias is seen.
// LM (a back-off n-gram, ngram_tables.hpp): a node carries the LM state after its token and the total
// Ln = Ln(parent) + (weight * step(s_lm(parent), token) + length_bonus); the root has the LM's start state and 0.  A new
// candidate ranks by (p + Bn) + Ln, a stay by (logadd(pb', pnb') + Bn) + Ln, the reported logp is (tot + Bn) + Ln; an
// extension that merges into an existing entry adds no LM term, and the candidate cut stays ahead of both terms.
//
// Kernels (no atomics, results bit-identical from run to run):
//   ctc_beam_rows    : one wave64 per row (b, t < T_b), as ctc_lse_gather: the row's log-sum-exp (16-byte loads when
//                      V * sizeof % 16 == 0), lp[blank], and the sorted top-K list (token, lp) by K passes of "the
//                      largest element after the previous winner" over the row, which the first pass left in the
//                      caches.  All O(V) work of the search is here, off the serial path.
//   ctc_beam_walk    : ONE WAVE per utterance, all T_b frames inside the launch.  The per-frame working set (<= W (K + 1)
//                      scores) and the double-buffered beam live in LDS; a one-wave workgroup's barrier orders its LDS
//                      traffic and costs nothing to wait on.  A frame's candidate list, lse and lp[blank] do not depend
//                      on the search and are requested D frames ahead; lp[e_i] of step 2 depends on the previous frame's
//                      selection: it is requested the moment that selection is made and first used after the next
//                      frame's extension step, so ONE dependent memory round trip per frame remains on the serial path,
//                      partly covered.
//   ctc_beam_readout : one wave per (utterance, hypothesis): walks the node to the root (its depth is known) and writes
//                      the dense result arrays; everything behind a count is -1 / 0.
// The streaming form (edgedict_ctc_stream_*, "the streaming form" below) carries the beam across chunks in a persistent
// state: ctc_beam_walk<.., STREAM = true>, whose STREAM = false arm is the offline walk untouched, plus
// ctc_stream_reset_kernel, ctc_stream_compact and ctc_stream_readout.
#include "bias_tables.hpp"
#include "common.hpp"
#include "ctc_rows.hpp"
#include "ngram_tables.hpp"

namespace {

constexpr int CB_MAXW = 32;    // beam width
constexpr int CB_MAXC = 64;    // candidates per frame: one per lane of the row pass and of the walk
constexpr int CB_NONE = 0x7fffffff;

struct CbWs {
    size_t off_lse, off_lpb, off_ctok, off_clp, off_nodes, off_fnode, off_fdepth, total;
};

inline size_t cb_up256(size_t n) { return ((n + 255) / 256) * 256; }

// tree nodes of an utterance: the root and at most W per frame
inline size_t cb_node_capacity(int T, int W) { return 1 + (size_t)T * W; }

inline CbWs cb_ws(int B, int T, int W, int cand) {
    CbWs w;
    const size_t rows = (size_t)B * T;
    size_t o = 0;
    w.off_lse = o;    o += cb_up256(rows * sizeof(float));
    w.off_lpb = o;    o += cb_up256(rows * sizeof(float));
    w.off_ctok = o;   o += cb_up256(rows * cand * sizeof(int32_t));
    w.off_clp = o;    o += cb_up256(rows * cand * sizeof(float));
    // a node is (parent, token, frame, lp bits)
    w.off_nodes = o;  o += cb_up256((size_t)B * cb_node_capacity(T, W) * sizeof(int4));
    w.off_fnode = o;  o += cb_up256((size_t)B * W * sizeof(int32_t));
    w.off_fdepth = o; o += cb_up256((size_t)B * W * sizeof(int32_t));
    w.total = o;
    return w;
}

// the automaton's tables under the names bias_tables.hpp reads them by
struct CbBias {
    const int32_t* bias_root_next;
    const double* bias_held;
    const double* bias_pend;
    const int32_t* bias_row_ptr;
    const int32_t* bias_exc_tok;
    const int32_t* bias_exc_next;
    int bias_S;
};

// The streaming form's persistent state (ctc_stream_* below): per stream the beam in ranked order - entry j's pb, pnb,
// bias total and LM total, its node, parent node, last token (-1: the empty prefix), tokens between the tree's root and
// it, automaton state and n-gram state -, the entry count, the tree's node count, the frames since the reset, and the
// token tree itself, NC nodes (parent, token, frame, lp bits) with the root in node 0.
struct CbStream {
    double *pb, *pnb, *bn, *ln;                     // [S][W]
    int32_t *node, *par, *tok, *dep, *st, *lm;      // [S][W]
    int32_t *count, *n_nodes, *frames;              // [S]
    int4* nodes;                                    // [S][NC]
};

struct CbStreamLayout {
    size_t pb, pnb, bn, ln, node, par, tok, dep, st, lm, count, n_nodes, frames, nodes, total;
};
inline CbStreamLayout cb_stream_layout(size_t S, size_t W, size_t NC) {
    CbStreamLayout a{};
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t r = o; o += cb_up256(bytes); return r; };
    a.pb = take(S * W * 8); a.pnb = take(S * W * 8); a.bn = take(S * W * 8); a.ln = take(S * W * 8);
    a.node = take(S * W * 4); a.par = take(S * W * 4); a.tok = take(S * W * 4); a.dep = take(S * W * 4);
    a.st = take(S * W * 4); a.lm = take(S * W * 4);
    a.count = take(S * 4); a.n_nodes = take(S * 4); a.frames = take(S * 4);
    a.nodes = take(S * NC * sizeof(int4));
    a.total = o;
    return a;
}
inline CbStream cb_stream_bind(char* st, const CbStreamLayout& a) {
    CbStream q;
    q.pb = (double*)(st + a.pb); q.pnb = (double*)(st + a.pnb); q.bn = (double*)(st + a.bn); q.ln = (double*)(st + a.ln);
    q.node = (int32_t*)(st + a.node); q.par = (int32_t*)(st + a.par); q.tok = (int32_t*)(st + a.tok);
    q.dep = (int32_t*)(st + a.dep); q.st = (int32_t*)(st + a.st); q.lm = (int32_t*)(st + a.lm);
    q.count = (int32_t*)(st + a.count); q.n_nodes = (int32_t*)(st + a.n_nodes); q.frames = (int32_t*)(st + a.frames);
    q.nodes = (int4*)(st + a.nodes);
    return q;
}

// the chunk workspace of an advance: the row pass's outputs for [S][Tc] rows, the streams' frame counts on the device,
// the compaction's renumbering scratch and its commit records (record 0 of a stream = its counts)
struct CbStreamWs {
    size_t off_lse, off_lpb, off_ctok, off_clp, off_nf, off_remap, off_commit, total;
};
inline CbStreamWs cb_stream_ws(size_t S, size_t Tc, size_t cand, size_t NC) {
    CbStreamWs w{};
    const size_t rows = S * Tc;
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t r = o; o += cb_up256(bytes); return r; };
    w.off_lse = take(rows * sizeof(float));
    w.off_lpb = take(rows * sizeof(float));
    w.off_ctok = take(rows * cand * sizeof(int32_t));
    w.off_clp = take(rows * cand * sizeof(float));
    w.off_nf = take(S * sizeof(int32_t));
    w.off_remap = take(S * NC * sizeof(int32_t));
    w.off_commit = take(S * (NC + 1) * sizeof(int4));
    w.total = o;
    return w;
}

inline bool cb_stream_dims_ok(int S, int W, int NC) {
    return S > 0 && W >= 1 && W <= CB_MAXW && NC >= W && (long long)S * W <= 0x7fffffffLL / 8 &&
           (long long)S * ((long long)NC + 1) <= 0x7fffffffLL / 16;
}

// max of a double over the wave, wave-uniform: the prefix-max inside each row of 16 lanes (row_shr:1, 2, 4, 8), then
// lane 15 of rows 0 / 2 into rows 1 / 3 (row_bcast:15) and lane 31 into rows 2, 3 (row_bcast:31) - lane 63 holds the
// maximum.  A lane without a source keeps its own value (`old` = the value, bound_ctrl off).  Six steps of two DPP moves
// and one v_max_f64, against six steps of two ds_bpermute round trips for a butterfly.
template <int CTRL, int ROWS>
__device__ __forceinline__ double dpp_max64(double v) {
    const int hi = __builtin_amdgcn_update_dpp(__double2hiint(v), __double2hiint(v), CTRL, ROWS, 0xf, false);
    const int lo = __builtin_amdgcn_update_dpp(__double2loint(v), __double2loint(v), CTRL, ROWS, 0xf, false);
    return fmax(v, __hiloint2double(hi, lo));
}
__device__ __forceinline__ double wave_max64(double v) {
    v = dpp_max64<0x111, 0xf>(v);
    v = dpp_max64<0x112, 0xf>(v);
    v = dpp_max64<0x114, 0xf>(v);
    v = dpp_max64<0x118, 0xf>(v);
    v = dpp_max64<0x142, 0xa>(v);
    v = dpp_max64<0x143, 0xc>(v);
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), 63),
                            __builtin_amdgcn_readlane(__double2loint(v), 63));
}

template <int CTRL, int ROWS>
__device__ __forceinline__ float dpp_max32(float v) {
    const int o = __builtin_amdgcn_update_dpp(__float_as_int(v), __float_as_int(v), CTRL, ROWS, 0xf, false);
    return fmaxf(v, __int_as_float(o));
}
__device__ __forceinline__ float wave_top(float v) {
    v = dpp_max32<0x111, 0xf>(v);
    v = dpp_max32<0x112, 0xf>(v);
    v = dpp_max32<0x114, 0xf>(v);
    v = dpp_max32<0x118, 0xf>(v);
    v = dpp_max32<0x142, 0xa>(v);
    v = dpp_max32<0x143, 0xc>(v);
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}
__device__ __forceinline__ double wave_top(double v) { return wave_max64(v); }

// The best (value, then lowest index) over the wave, wave-uniform: every lane brings its own best value bv and that
// value's index bm (CB_NONE: the lane has nothing, whatever bv holds).  The lanes that hold the wave's maximum are
// balloted and the lowest index among them is read out lane by lane - one lane unless values tie.  Returns the index
// (CB_NONE: no lane has anything) and leaves the maximum in wv.  bv must not be a NaN.
template <typename V>
__device__ __forceinline__ int wave_pick(V bv, int bm, V& wv) {
    wv = wave_top(bv);
    unsigned long long tied = __ballot(bm != CB_NONE && bv == wv);
    int wi = CB_NONE;
    while (tied) {
        const int l = __ffsll((long long)tied) - 1;
        tied &= tied - 1;
        wi = min(wi, __builtin_amdgcn_readlane(bm, l));
    }
    return wi;
}

// ------------------------------------------------------------------ the row pass
// grid (x, B) as ctc_lse_gather: 4 waves per block, one row per wave per iteration, rows t >= T_b are never read.
// Pass k of the top-K list finds the largest non-blank element AFTER the previous winner (pv, pi) in the order "value
// descending, index ascending": x < pv, or x == pv with a higher index.  A lane sees its columns in ascending order and
// replaces its best on a strictly larger value only; wave_pick prefers the value, then the lower index.  A NaN
// compares false everywhere and is never a candidate; a list that runs out of elements is closed with token -1 / -inf.
// Candidate k is kept by lane k, the list is written with one store per lane: ctok / clp [rows][cand], K used.
template <typename T>
__global__ __launch_bounds__(256) void ctc_beam_rows(const T* __restrict__ logits, const int32_t* __restrict__ act_lens,
                                                     int Tm, int V, int blank, int K, int cand,
                                                     float* __restrict__ lse, float* __restrict__ lpb,
                                                     int32_t* __restrict__ ctok, float* __restrict__ clp, int vec_ok) {
    constexpr int VEC = ElemIO<T>::VEC;
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
        float pv = INFINITY;
        int pi = -1;
        int my_tok = -1;
        float my_lp = -INFINITY;
        for (int k = 0; k < K; ++k) {
            float bv = -INFINITY;
            int bi = CB_NONE;
            auto see = [&](float x, int idx) {
                const bool after = idx != blank && (x < pv || (x == pv && idx > pi));
                if (after && (x > bv || bi == CB_NONE)) { bv = x; bi = idx; }
            };
            if (vec_ok) {
                for (int v = lane * VEC; v < V; v += 64 * VEC) {
                    float x[VEC];
                    ElemIO<T>::load_vec(z + v, x);
#pragma unroll
                    for (int i = 0; i < VEC; ++i) see(x[i], v + i);
                }
            } else {
                for (int v = lane; v < V; v += 64) see(ElemIO<T>::load(z + v), v);
            }
            float wv;
            const int wi = wave_pick(bv, bi, wv);
            if (lane == k) {
                my_tok = wi == CB_NONE ? -1 : wi;
                my_lp = wi == CB_NONE ? -INFINITY : wv - l;
            }
            pv = wi == CB_NONE ? -INFINITY : wv;      // (nothing found: after -inf / CB_NONE nothing is "after")
            pi = wi;
        }
        if (lane < K) {
            ctok[row * cand + lane] = my_tok;
            clp[row * cand + lane] = my_lp;
        }
    }
}

// ------------------------------------------------------------------ the search
// blockIdx.x = utterance, 64 threads.  LDS: the scores of the frame's items (stays 0 .. nb - 1 in beam order, then the
// new candidates nb + i K + c: the canonical index of the tie rule), the beam twice (read `cur`, build `cur ^ 1`), the
// stays' new pb / pnb, the frame's candidate list.  Per frame:
//   C  every item (i, c): p and its ranking score into s_sc; lane (g, c) takes candidate c of the entries g, g + G, ...
//      (K rounded up to a power of two Kp, G = 64 / Kp groups: no division per item)
//   B  lane j < nb, stay j: pb', pnb' with lp[e_j] (the gather requested at the end of the previous frame, the same fp32
//      expression z - lse the row pass formed, so a token of the list has the same bits either way and is taken from the
//      list).  Where e_j stands in the candidate list: one ballot per entry, lane c holding candidate c; where j's
//      parent stands in the beam: the entries' nodes read out of lane registers.  Entry j's parent can be in the beam
//      once at most, so pnb'_j receives at most ONE extension - no order to fix - and that extension's item is struck
//      from s_sc
//   D  up to W rounds of (best, lowest index) over the wave (wave_pick).  Lane l owns the items l, l + 64, ...: up to
//      R = 8 of them in registers, struck there when they win; a frame with more than 64 R items leaves them in LDS, a
//      lane keeps the best of its own and only the round's winner looks at its items again
//   E  lane r builds entry r of the new beam; new nodes take consecutive ids in ranked order (ballot + prefix count) and
//      are written with one 16-byte store; the gather for the next frame is requested.
// The ring q* holds lse, lp[blank] and lane l's candidate l of the D frames ahead (static slots, as ctc_alpha_beta).
// LM: step C makes one n-gram lookup per live item (a binary search per back-off level: dependent reads of tables that
// stay in the caches), step E one more per selected new node to keep its state; the LM = false instantiations are the
// kernels without any of it.
template <typename T, bool BIAS, bool LM, bool STREAM = false>
__global__ __launch_bounds__(64) void ctc_beam_walk(const T* __restrict__ logits, const int32_t* __restrict__ act_lens,
                                                    int Tm, int V, int W, int K, int cand,
                                                    const float* __restrict__ lse, const float* __restrict__ lpb,
                                                    const int32_t* __restrict__ ctok, const float* __restrict__ clp,
                                                    int4* __restrict__ nodes, int NC, int32_t* __restrict__ fnode,
                                                    int32_t* __restrict__ fdepth, int32_t* __restrict__ n_hyp,
                                                    double* __restrict__ logp, CbBias bt, NgramTables lt,
                                                    CbStream ss) {
    constexpr int D = 4, R = 8;
    __shared__ double s_sc[CB_MAXW * (CB_MAXC + 1)];
    __shared__ double s_pb[2][CB_MAXW], s_pnb[2][CB_MAXW], s_tot[2][CB_MAXW], s_bn[2][CB_MAXW];
    __shared__ double s_pbn[CB_MAXW], s_pnbn[CB_MAXW];
    __shared__ int s_node[2][CB_MAXW], s_tok[2][CB_MAXW], s_par[2][CB_MAXW], s_dep[2][CB_MAXW], s_st[2][CB_MAXW];
    __shared__ int s_ctok[CB_MAXC];
    __shared__ float s_clp[CB_MAXC];
    __shared__ double s_ln[2][LM ? CB_MAXW : 1];
    __shared__ int s_lm[2][LM ? CB_MAXW : 1];

    const int b = blockIdx.x, lane = threadIdx.x;
    const int Tb = max(0, min(act_lens[b], Tm));
    const double NEG = -(double)INFINITY;
    const long long row0 = (long long)b * Tm;
    int4* nd = nodes + (long long)b * NC;

    // the extension step's lane -> (entry group, candidate) map: Kp = K rounded up to a power of two, G = 64 / Kp groups
    const int sh = 32 - __clz(K - 1), Kp = 1 << sh, G = 64 >> sh;
    int cur = 0, nb = 1, nnodes = 1, f0 = 0;
    float ge = 0.f;                                   // lp[e_lane] of the coming frame
    if (STREAM) {
        // the beam as the previous advance (or the reset) left it; ge, which the offline walk requests at the end of the
        // previous frame, comes from this chunk's first row by the same fp32 expression
        nb = min(max(ss.count[b], 1), W);
        nnodes = min(max(ss.n_nodes[b], 1), NC);
        f0 = ss.frames[b];
        if (lane < nb) {
            const int e = b * W + lane;
            const double pb = ss.pb[e], pnb = ss.pnb[e];
            const int tok = ss.tok[e];
            s_pb[0][lane] = pb; s_pnb[0][lane] = pnb; s_tot[0][lane] = log_add64(pb, pnb); s_bn[0][lane] = ss.bn[e];
            s_node[0][lane] = ss.node[e]; s_tok[0][lane] = tok; s_par[0][lane] = ss.par[e]; s_dep[0][lane] = ss.dep[e];
            s_st[0][lane] = ss.st[e];
            if (LM) { s_ln[0][lane] = ss.ln[e]; s_lm[0][lane] = ss.lm[e]; }
            if (Tb > 0 && tok >= 0 && tok < V) ge = ElemIO<T>::load(logits + row0 * (long long)V + tok) - lse[row0];
        }
    } else if (lane == 0) {
        s_pb[0][0] = 0.0; s_pnb[0][0] = NEG; s_tot[0][0] = 0.0; s_bn[0][0] = 0.0;
        s_node[0][0] = 0; s_tok[0][0] = -1; s_par[0][0] = -1; s_dep[0][0] = 0; s_st[0][0] = 0;
        nd[0] = make_int4(-1, -1, -1, 0);
        if (LM) { s_ln[0][0] = 0.0; s_lm[0][0] = lt.lm_start; }
    }
    float qlse[D], qlpb[D], qlp[D];
    int qtok[D];
    auto request = [&](int j, int r) {                // (static j)
        float a = 0.f, c = 0.f, p = -INFINITY;
        int k = -1;
        if (r < Tb) {
            a = lse[row0 + r];
            c = lpb[row0 + r];
            if (lane < K) {
                k = ctok[(row0 + r) * cand + lane];
                p = clp[(row0 + r) * cand + lane];
            }
        }
        qlse[j] = a; qlpb[j] = c; qtok[j] = k; qlp[j] = p;
    };
#pragma unroll
    for (int j = 0; j < D; ++j) request(j, j);
    __syncthreads();

    for (int r0 = 0; r0 < Tb; r0 += D) {
#pragma unroll
        for (int j = 0; j < D; ++j) {
            const int r = r0 + j;
            if (r >= Tb) break;
            const float cb = qlpb[j], lse_next = qlse[(j + 1) % D];
            const int ctk = qtok[j];                  // candidate `lane` of this frame (-1: none)
            if (lane < K) {
                s_ctok[lane] = ctk;
                s_clp[lane] = qlp[j];
            }
            request(j, r + D);
            __syncthreads();
            // ---- C: the extension items; lane (g, c) takes candidate c of the entries g, g + G, ...
            const int N = nb * K;
            {
                const int c = lane & (Kp - 1);
                const int tk = c < K ? s_ctok[c] : -1;
                const double lpc = c < K ? (double)s_clp[c] : NEG;
                for (int i = lane >> sh; i < nb; i += G) {
                    if (c >= K) continue;
                    double p = (tk == s_tok[cur][i] ? s_pb[cur][i] : s_tot[cur][i]) + lpc;
                    if (tk < 0) p = NEG;
                    const bool real = p > NEG;
                    if (BIAS && real) {
                        const int s = bias_state(bt, s_st[cur][i]);
                        const int n = bias_goto(bt, s, tk);
                        p += s_bn[cur][i] + (bt.bias_held[n] - bt.bias_pend[s]);
                    }
                    if (LM && real) {
                        int nx;
                        const double l = ngram_step(lt, s_lm[cur][i], tk, &nx);
                        p += s_ln[cur][i] + ngram_term(lt.lm_weight, l, lt.lm_bonus);
                    }
                    s_sc[nb + i * K + c] = p;
                }
            }
            // ---- B: the stays.  ci: where entry `lane`'s token stands in the candidate list (lane c holds candidate c:
            // a ballot per entry), pi: where its parent stands in the beam; -1: not there
            const bool stay = lane < nb;
            const int tokj = stay ? s_tok[cur][lane] : -1, parj = stay ? s_par[cur][lane] : -2;
            const int nodej = stay ? s_node[cur][lane] : -3;
            int ci = -1, pi = -1;
            for (int k = 0; k < nb; ++k) {          // (entry k's token and node out of lane k's registers)
                const int tkk = __builtin_amdgcn_readlane(tokj, k), nk = __builtin_amdgcn_readlane(nodej, k);
                const unsigned long long at = __ballot(ctk >= 0 && ctk == tkk);
                if (lane == k && at) ci = __ffsll((long long)at) - 1;
                if (parj == nk) pi = k;
            }
            __syncthreads();
            if (stay) {
                const double pbn = s_tot[cur][lane] + (double)cb;
                double pnbn = NEG;
                if (STREAM ? tokj >= 0 : nodej != 0) {     // (a re-rooted tree's node 0 is a prefix with a token)
                    pnbn = s_pnb[cur][lane] + (double)(ci >= 0 ? s_clp[ci] : ge);
                    if (ci >= 0 && pi >= 0) {
                        const double pe = (tokj == s_tok[cur][pi] ? s_pb[cur][pi] : s_tot[cur][pi]) + (double)s_clp[ci];
                        pnbn = log_add64(pnbn, pe);
                        s_sc[nb + pi * K + ci] = NEG;
                    }
                }
                s_pbn[lane] = pbn;
                s_pnbn[lane] = pnbn;
                double rk = log_add64(pbn, pnbn);
                if (BIAS) rk += s_bn[cur][lane];
                if (LM) rk += s_ln[cur][lane];
                s_sc[lane] = rk;
            }
            __syncthreads();
            // ---- D: select.  Lane l owns the items l, l + 64, ...: up to R of them in registers (W = 10 with 32
            // candidates: 6), beyond that in LDS
            const int NT = nb + N;
            int nsel = 0, mysel = 0;
            if (NT <= 64 * R) {
                double loc[R];
#pragma unroll
                for (int k = 0; k < R; ++k) loc[k] = lane + 64 * k < NT ? s_sc[lane + 64 * k] : NEG;
                for (int q = 0; q < W; ++q) {
                    double bv = NEG;
                    int bk = 0;
#pragma unroll
                    for (int k = 0; k < R; ++k)
                        if (loc[k] > bv) { bv = loc[k]; bk = k; }
                    double wv;
                    const int wi = wave_pick(bv, bv > NEG ? lane + 64 * bk : CB_NONE, wv);
                    if (wi == CB_NONE) break;         // (wave-uniform)
                    if (lane == q) mysel = wi;
#pragma unroll
                    for (int k = 0; k < R; ++k)
                        if (wi == lane + 64 * k) loc[k] = NEG;
                    ++nsel;
                }
            } else {
                double bv;
                int bi;
                auto rescan = [&]() {
                    bv = NEG;
                    bi = CB_NONE;
                    for (int m = lane; m < NT; m += 64) {
                        const double v = s_sc[m];
                        if (v > bv) { bv = v; bi = m; }
                    }
                };
                rescan();
                for (int q = 0; q < W; ++q) {
                    double wv;
                    const int wi = wave_pick(bv, bi, wv);
                    if (wi == CB_NONE) break;         // (wave-uniform)
                    if (lane == q) mysel = wi;
                    if ((wi & 63) == lane) {
                        s_sc[wi] = NEG;
                        rescan();
                    }
                    ++nsel;
                }
            }
            // ---- E: the new beam
            const int nxt = cur ^ 1;
            const bool have = lane < nsel, fresh = have && mysel >= nb;
            const unsigned long long mask = __ballot(fresh);
            if (have) {
                int node, tok, par, dep, st = 0, slm = 0;
                double pb, pnb, bn = 0.0, ln = 0.0;
                if (!fresh) {
                    if (LM) { slm = s_lm[cur][mysel]; ln = s_ln[cur][mysel]; }
                    node = s_node[cur][mysel]; tok = s_tok[cur][mysel]; par = s_par[cur][mysel];
                    dep = s_dep[cur][mysel]; st = s_st[cur][mysel]; bn = s_bn[cur][mysel];
                    pb = s_pbn[mysel]; pnb = s_pnbn[mysel];
                } else {
                    const int m = mysel - nb, i = m / K, c = m - i * K;
                    tok = s_ctok[c];
                    node = nnodes + __popcll(mask & ((1ull << lane) - 1ull));
                    par = s_node[cur][i];
                    dep = s_dep[cur][i] + 1;
                    pb = NEG;
                    pnb = (tok == s_tok[cur][i] ? s_pb[cur][i] : s_tot[cur][i]) + (double)s_clp[c];
                    if (BIAS) {
                        const int s = bias_state(bt, s_st[cur][i]);
                        st = bias_goto(bt, s, tok);
                        bn = s_bn[cur][i] + (bt.bias_held[st] - bt.bias_pend[s]);
                    }
                    if (LM) {
                        const double l = ngram_step(lt, s_lm[cur][i], tok, &slm);
                        ln = s_ln[cur][i] + ngram_term(lt.lm_weight, l, lt.lm_bonus);
                    }
                    if (node < NC) nd[node] = make_int4(par, tok, f0 + r, __float_as_int(s_clp[c]));
                }
                s_node[nxt][lane] = node; s_tok[nxt][lane] = tok; s_par[nxt][lane] = par; s_dep[nxt][lane] = dep;
                s_st[nxt][lane] = st; s_bn[nxt][lane] = bn;
                if (LM) { s_lm[nxt][lane] = slm; s_ln[nxt][lane] = ln; }
                s_pb[nxt][lane] = pb; s_pnb[nxt][lane] = pnb; s_tot[nxt][lane] = log_add64(pb, pnb);
                if (r + 1 < Tb && tok >= 0 && tok < V)
                    ge = ElemIO<T>::load(logits + (row0 + r + 1) * (long long)V + tok) - lse_next;
            }
            nnodes += __popcll(mask);
            nb = nsel;
            cur = nxt;
            __syncthreads();
        }
    }
    if (STREAM) {
        if (lane < nb) {
            const int e = b * W + lane;
            ss.pb[e] = s_pb[cur][lane]; ss.pnb[e] = s_pnb[cur][lane]; ss.bn[e] = s_bn[cur][lane];
            ss.node[e] = s_node[cur][lane]; ss.par[e] = s_par[cur][lane]; ss.tok[e] = s_tok[cur][lane];
            ss.dep[e] = s_dep[cur][lane]; ss.st[e] = s_st[cur][lane];
            if (LM) { ss.ln[e] = s_ln[cur][lane]; ss.lm[e] = s_lm[cur][lane]; }
        }
        if (lane == 0) {
            ss.count[b] = nb;
            ss.n_nodes[b] = min(nnodes, NC);
            ss.frames[b] = f0 + Tb;
        }
        return;
    }
    if (lane < W) {
        const bool live = lane < nb;
        fnode[b * W + lane] = live ? s_node[cur][lane] : -1;
        fdepth[b * W + lane] = live ? s_dep[cur][lane] : 0;
        double lp = live ? s_tot[cur][lane] + (BIAS ? s_bn[cur][lane] : 0.0) : NEG;
        if (LM && live) lp += s_ln[cur][lane];
        logp[b * W + lane] = lp;
    }
    if (lane == 0) n_hyp[b] = nb;
}

// ------------------------------------------------------------------ the read-out
// blockIdx.x = b W + h.  tokens / frames / token_lp [B][W][Tm]: hypothesis h's tokens, their creation frames and their
// log-softmax values on those frames, root to leaf; -1 / -1 / 0 behind ntok[b][h] (a hypothesis has at most T_b <= Tm
// tokens: a node made on frame t is at depth <= t + 1).  The walk is a chain of dependent 16-byte loads, one lane's.
__global__ __launch_bounds__(64) void ctc_beam_readout(const int4* __restrict__ nodes, int NC,
                                                       const int32_t* __restrict__ fnode,
                                                       const int32_t* __restrict__ fdepth, int Tm,
                                                       int32_t* __restrict__ tokens, int32_t* __restrict__ frames,
                                                       float* __restrict__ token_lp, int32_t* __restrict__ ntok, int W) {
    const int bh = blockIdx.x, b = bh / W, lane = threadIdx.x;
    const int dep = max(0, min(fdepth[bh], Tm));
    const long long o = (long long)bh * Tm;
    for (int pos = dep + lane; pos < Tm; pos += 64) {
        tokens[o + pos] = -1;
        frames[o + pos] = -1;
        token_lp[o + pos] = 0.f;
    }
    if (lane != 0) return;
    ntok[bh] = dep;
    const int4* nd = nodes + (long long)b * NC;
    int node = fnode[bh];
    for (int pos = dep - 1; pos >= 0; --pos) {
        int4 rec = make_int4(-1, -1, -1, 0);
        if (node > 0 && node < NC) rec = nd[node];
        tokens[o + pos] = rec.y;
        frames[o + pos] = rec.z;
        token_lp[o + pos] = __int_as_float(rec.w);
        node = rec.x;
    }
}

// ------------------------------------------------------------------ the streaming form
// S streams whose logits arrive chunk by chunk; after any number of chunks a stream's state holds exactly the beam the
// offline walk has after the same frames.  An advance is ctc_beam_rows on the chunk's [S, Tc, V] logits (the streams'
// frame counts n_frames[s] in 0 .. Tc as its lengths), ctc_beam_walk<.., STREAM = true> - the same wave per stream, all
// of the chunk's frames inside the launch, the beam loaded from the state at entry and stored at exit, absolute frame
// numbers in new nodes - and ctc_stream_compact.  Where a carried beam differs from a beam inside the offline loop:
//   - lp[e_lane] of the chunk's first frame (`ge`) cannot have been requested at the end of the previous frame, whose
//     next row is in this chunk: the walk forms it for every loaded entry from the chunk's first row, load(z) - lse in
//     fp32 as the offline request does;
//   - the request ring starts and drains on n_frames[s] as it does on T_b offline: every request and every frame is
//     guarded by r < T_b, so 0, 1 and counts that are no multiple of D need nothing of their own;
//   - after a compaction node 0 is a prefix with a token and a pnb: "the empty prefix" is tok < 0, not node == 0.  Node
//     ids enter no ranking (ties go by canonical index), so renumbering changes no result.
//
// ctc_stream_reset_kernel: one thread per selected stream (mask: device int32 [S] or null): entry 0 = the empty prefix
// (pb 0, pnb -inf, totals 0, automaton state 0, the LM's start state) on a tree of the root alone.
__global__ __launch_bounds__(64) void ctc_stream_reset_kernel(CbStream ss, const int32_t* __restrict__ mask, int S,
                                                              int W, int NC, int lm_start) {
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= S || (mask && !mask[s])) return;
    const double NEG = -(double)INFINITY;
    for (int j = 0; j < W; ++j) {
        const int e = s * W + j;
        ss.pb[e] = j == 0 ? 0.0 : NEG; ss.pnb[e] = NEG; ss.bn[e] = 0.0; ss.ln[e] = 0.0;
        ss.node[e] = j == 0 ? 0 : -1; ss.par[e] = -1; ss.tok[e] = -1; ss.dep[e] = 0; ss.st[e] = 0; ss.lm[e] = lm_start;
    }
    ss.count[s] = 1;
    ss.n_nodes[s] = 1;
    ss.frames[s] = 0;
    ss.nodes[(long long)s * NC] = make_int4(-1, -1, -1, 0);
}

// One wave per stream, once per advance, after the walk.  Node ids grow with creation and a parent is older than its
// child, which a dense renumbering in index order keeps; entry j's `dep` is the number of tokens between the root and
// its node.
//   1. lane j = entry j: all entries climb to the smallest depth, then together until they stand on one node - the
//      lowest common ancestor of the live entries' nodes (the root at the latest);
//   2. lane 0 writes the tokens below the old root down to the ancestor into the commit records (token, frame, lp
//      bits): every live hypothesis and every later one starts with them, so no later frame can change them.  Record 0
//      = (tokens committed, nodes kept, tokens of the longest uncommitted tail);
//   3. the nodes from a live entry's node up to the ancestor are marked, numbered by a running count over the marks (the
//      ancestor, the oldest of them, becomes node 0 with parent -1) and moved down to their numbers with their parents
//      renamed; a chunk of 64 nodes is read whole before any of it is written and a node never moves up, so nothing
//      unread is overwritten;
//   4. the entries' node and par are renamed (an entry on the ancestor has par -1), dep loses the committed tokens.
// The ancestor of a set that contains both a prefix and its parent is the parent or above it, so a parent that is in
// the beam is never cut away: the walk's "is j's parent in the beam" test sees after the compaction what it saw before.
// No atomics; the result depends on the state alone.  `remap`: int32 [S][NC] scratch.
__global__ __launch_bounds__(64) void ctc_stream_compact(CbStream ss, int W, int NC, int32_t* __restrict__ remap,
                                                         int4* __restrict__ commit) {
    const int s = blockIdx.x, lane = threadIdx.x;
    int4* tree = ss.nodes + (long long)s * NC;
    int32_t* map = remap + (long long)s * NC;
    int4* out = commit + (long long)s * (NC + 1);
    const int n = min(max(ss.n_nodes[s], 1), NC);
    const int nb = min(max(ss.count[s], 1), W);
    const bool live = lane < nb;
    const int e = s * W + min(lane, W - 1);
    int leaf = live ? ss.node[e] : 0;
    int d = live ? ss.dep[e] : 0;
    if (leaf < 0 || leaf >= n || d < 0 || d >= n) { leaf = 0; d = 0; }      // (not on a state the advances wrote)
    auto up = [&](int a) { return a > 0 && a < n ? max(tree[a].x, 0) : 0; };
    // 1.
    int depth = live ? d : 0x7fffffff;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) depth = min(depth, __shfl_xor(depth, off, 64));
    int a = leaf;
    for (int k = d; live && k > depth; --k) a = up(a);
    while (depth > 0) {
        const int a0 = __shfl(a, 0, 64);
        if (__ballot(live && a != a0) == 0ull) break;
        if (live) a = up(a);
        --depth;
    }
    const int lca = depth > 0 ? __shfl(a, 0, 64) : 0;
    // 2.
    if (lane == 0) {
        int k = depth;
        for (int nd = lca; k > 0; nd = up(nd)) {
            --k;
            const int4 rec = tree[nd];
            out[1 + k] = make_int4(rec.y, rec.z, rec.w, 0);
        }
    }
    // 3.
    for (int i = lane; i < n; i += 64) map[i] = 0;
    __syncthreads();
    if (live) {
        int nd = leaf;
        for (int k = d; k > depth; --k) {
            map[nd] = 1;
            nd = up(nd);
        }
    }
    if (lane == 0) map[lca] = 1;
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
        int4 rec = make_int4(-1, -1, -1, 0);
        if (id >= 0) {
            rec = tree[i];
            rec.x = (i == lca || rec.x < 0 || rec.x >= n) ? -1 : map[rec.x];
        }
        __syncthreads();
        if (id >= 0) tree[id] = rec;
        __syncthreads();
    }
    // 4.
    if (live) {
        const int par = ss.par[e];
        ss.node[e] = max(map[leaf], 0);
        ss.par[e] = (leaf == lca || par < 0 || par >= n) ? -1 : map[par];
        ss.dep[e] = d - depth;
    }
    int tail = live ? d - depth : 0;                // the longest uncommitted tail: what a read-out has to hold
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) tail = max(tail, __shfl_xor(tail, off, 64));
    if (lane == 0) {
        ss.n_nodes[s] = n_live;
        out[0] = make_int4(depth, n_live, tail, 0);
    }
}

// The uncommitted part: blockIdx.x = s W + h, ctc_beam_readout on the state.  tokens / frames / token_lp [S][W][MT]: the
// tokens between the root and entry h's node (dep of them: the root's own token is committed), -1 / -1 / 0 behind;
// logp = (logadd(pb, pnb) + Bn) + Ln in the offline walk's association order (a total that is not carried is +0.0,
// which changes no bit of a sum that is not -0.0, and tot + 0.0 never is), -inf behind n_hyp[s].
__global__ __launch_bounds__(64) void ctc_stream_readout(CbStream ss, int W, int NC, int MT,
                                                         int32_t* __restrict__ tokens, int32_t* __restrict__ frames,
                                                         float* __restrict__ token_lp, int32_t* __restrict__ ntok,
                                                         int32_t* __restrict__ n_hyp, double* __restrict__ logp) {
    const int sh = blockIdx.x, s = sh / W, h = sh - s * W, lane = threadIdx.x;
    const int nb = min(max(ss.count[s], 1), W);
    const bool live = h < nb;
    const int dep = live ? max(0, min(ss.dep[sh], MT)) : 0;
    const long long o = (long long)sh * MT;
    for (int pos = dep + lane; pos < MT; pos += 64) {
        tokens[o + pos] = -1;
        frames[o + pos] = -1;
        token_lp[o + pos] = 0.f;
    }
    if (lane != 0) return;
    ntok[sh] = dep;
    double lp = -(double)INFINITY;
    if (live) {
        lp = log_add64(ss.pb[sh], ss.pnb[sh]) + ss.bn[sh];
        lp += ss.ln[sh];
    }
    logp[sh] = lp;
    if (h == 0) n_hyp[s] = nb;
    const int4* nd = ss.nodes + (long long)s * NC;
    int node = live ? ss.node[sh] : -1;
    for (int pos = dep - 1; pos >= 0; --pos) {
        int4 rec = make_int4(-1, -1, -1, 0);
        if (node >= 0 && node < NC) rec = nd[node];
        tokens[o + pos] = rec.y;
        frames[o + pos] = rec.z;
        token_lp[o + pos] = __int_as_float(rec.w);
        node = rec.x;
    }
}

}  // namespace

extern "C" size_t edgedict_ctc_beam_workspace_bytes(int B, int T, int W, int cand) {
    if (B <= 0 || T <= 0 || W < 1 || W > CB_MAXW || cand < 1 || cand > CB_MAXC) return 0;
    return cb_ws(B, T, W, cand).total;
}

extern "C" int edgedict_ctc_beam_search_fused(const void* logits, int dtype, const int32_t* act_lens, int B, int T, int V,
                                              int blank, int W, int cand, const edgedict_ctc_beam_opts_t* opts,
                                              int32_t* tokens, int32_t* frames, float* token_lp, int32_t* ntok,
                                              int32_t* n_hyp, double* logp, void* workspace, void* stream_) {
    ED_CHECK_ARG(!opts || (uintptr_t)opts >= 4096, "ctc_beam_search: opts is not a pointer");
    const edgedict_beam_bias_t* bias = opts ? opts->bias : nullptr;
    const edgedict_ngram_lm_t* lm = opts ? opts->ngram : nullptr;
    ED_CHECK_ARG(B > 0 && T > 0, "ctc_beam_search: B, T must be positive (got %d, %d)", B, T);
    ED_CHECK_ARG(V >= 2, "ctc_beam_search: V = %d, need at least the blank and one symbol", V);
    ED_CHECK_ARG(blank >= 0 && blank < V, "ctc_beam_search: blank %d outside [0,%d)", blank, V);
    ED_CHECK_ARG(dtype == ED_F32 || dtype == ED_BF16, "ctc_beam_search: unsupported dtype code %d", dtype);
    ED_CHECK_ARG(W >= 1 && W <= CB_MAXW, "ctc_beam_search: W = %d outside [1,%d]", W, CB_MAXW);
    ED_CHECK_ARG(cand >= 1 && cand <= CB_MAXC, "ctc_beam_search: cand = %d outside [1,%d]", cand, CB_MAXC);
    ED_CHECK_ARG(logits && act_lens && tokens && frames && token_lp && ntok && n_hyp && logp && workspace,
                 "ctc_beam_search: null pointer argument");
    ED_CHECK_ARG(((uintptr_t)workspace & 15) == 0, "ctc_beam_search: workspace must be 16-byte aligned");
    ED_CHECK_ARG((long long)B * W * T <= 0x7fffffffLL && (long long)B * T * cand <= 0x7fffffffLL,
                 "ctc_beam_search: B x T x max(W, cand) = %d x %d x %d exceeds 2^31 - 1", B, T, max(W, cand));
    CbBias bt{};
    if (bias) {
        ED_CHECK_ARG(bias->V == V, "ctc_beam_search: the bias list's vocabulary = %d differs from the head's V = %d",
                     bias->V, V);
        ED_CHECK_ARG(bias->S > 0 && bias->n_exc >= 0, "ctc_beam_search: bad bias automaton (S %d, exceptions %d)",
                     bias->S, bias->n_exc);
        ED_CHECK_ARG(bias->root_next && bias->held && bias->pend && bias->row_ptr && bias->exc_tok && bias->exc_next,
                     "ctc_beam_search: null bias table pointer");
        bt = CbBias{bias->root_next, bias->held, bias->pend, bias->row_ptr, bias->exc_tok, bias->exc_next, bias->S};
    }
    NgramTables lt{};
    if (lm) {
        if (int rc = ed_ngram_check(lm, "ctc_beam_search")) return rc;
        ED_CHECK_ARG(lm->V == V, "ctc_beam_search: the n-gram's vocabulary = %d differs from the head's V = %d", lm->V, V);
        ED_CHECK_ARG(lm->blank == blank, "ctc_beam_search: the n-gram's blank = %d differs from the search's %d",
                     lm->blank, blank);
        ED_CHECK_ARG(isfinite(lm->weight) && lm->weight >= 0.0 && isfinite(lm->length_bonus),
                     "ctc_beam_search: lm weight %g must be finite and >= 0, length_bonus %g finite", lm->weight,
                     lm->length_bonus);
        lt = ed_ngram_tables(lm);
    }
    hipStream_t stream = (hipStream_t)stream_;
    const CbWs w = cb_ws(B, T, W, cand);
    char* p = (char*)workspace;
    float* lse = (float*)(p + w.off_lse);
    float* lpb = (float*)(p + w.off_lpb);
    int32_t* ctok = (int32_t*)(p + w.off_ctok);
    float* clp = (float*)(p + w.off_clp);
    int4* nodes = (int4*)(p + w.off_nodes);
    int32_t* fnode = (int32_t*)(p + w.off_fnode);
    int32_t* fdepth = (int32_t*)(p + w.off_fdepth);
    const int K = min(cand, V - 1);
    const int NC = (int)cb_node_capacity(T, W);

    const size_t esz = dtype == ED_F32 ? 4 : 2;
    const int vec_ok = ((V * esz) % 16 == 0) && (((uintptr_t)logits & 15) == 0);
    const dim3 grid1(ed_grid_for(T, 4, max(1, 256 * 16 / B)), B);
    if (dtype == ED_F32)
        hipLaunchKernelGGL(ctc_beam_rows<float>, grid1, dim3(256), 0, stream, (const float*)logits, act_lens, T, V, blank,
                           K, cand, lse, lpb, ctok, clp, vec_ok);
    else
        hipLaunchKernelGGL(ctc_beam_rows<bf16_t>, grid1, dim3(256), 0, stream, (const bf16_t*)logits, act_lens, T, V,
                           blank, K, cand, lse, lpb, ctok, clp, vec_ok);
    ED_CHECK_LAUNCH("ctc_beam_rows");
#define ED_CB_WALK(TT, BB, LL)                                                                                  \
    hipLaunchKernelGGL((ctc_beam_walk<TT, BB, LL>), dim3(B), dim3(64), 0, stream, (const TT*)logits, act_lens, T, V, \
                       W, K, cand, lse, lpb, ctok, clp, nodes, NC, fnode, fdepth, n_hyp, logp, bt, lt, CbStream{})
#define ED_CB_WALK_T(TT)                                                                  \
    do {                                                                                  \
        if (lm) { if (bias) ED_CB_WALK(TT, true, true); else ED_CB_WALK(TT, false, true); } \
        else { if (bias) ED_CB_WALK(TT, true, false); else ED_CB_WALK(TT, false, false); }  \
    } while (0)
    if (dtype == ED_F32) ED_CB_WALK_T(float); else ED_CB_WALK_T(bf16_t);
#undef ED_CB_WALK_T
#undef ED_CB_WALK
    ED_CHECK_LAUNCH("ctc_beam_walk");
    hipLaunchKernelGGL(ctc_beam_readout, dim3(B * W), dim3(64), 0, stream, (const int4*)nodes, NC, fnode, fdepth, T,
                       tokens, frames, token_lp, ntok, W);
    ED_CHECK_LAUNCH("ctc_beam_readout");
    return ED_OK;
}

extern "C" int edgedict_ctc_beam_search(const void* logits, int dtype, const int32_t* act_lens, int B, int T, int V,
                                        int blank, int W, int cand, const edgedict_beam_bias_t* bias, int32_t* tokens,
                                        int32_t* frames, float* token_lp, int32_t* ntok, int32_t* n_hyp, double* logp,
                                        void* workspace, void* stream) {
    const edgedict_ctc_beam_opts_t opts{bias, nullptr};
    return edgedict_ctc_beam_search_fused(logits, dtype, act_lens, B, T, V, blank, W, cand, &opts, tokens, frames,
                                          token_lp, ntok, n_hyp, logp, workspace, stream);
}

// ------------------------------------------------------------------ the streaming form's entry points
namespace {

// the checks of edgedict_ctc_beam_search_fused on opts; V < 0: the call does not know the vocabulary (the reset)
int cb_stream_opts(const char* what, const edgedict_ctc_beam_opts_t* opts, int V, int blank, CbBias* bt,
                   NgramTables* lt, bool* has_bias, bool* has_lm) {
    ED_CHECK_ARG(!opts || (uintptr_t)opts >= 4096, "%s: opts is not a pointer", what);
    const edgedict_beam_bias_t* bias = opts ? opts->bias : nullptr;
    const edgedict_ngram_lm_t* lm = opts ? opts->ngram : nullptr;
    ED_CHECK_ARG((!bias || (uintptr_t)bias >= 4096) && (!lm || (uintptr_t)lm >= 4096),
                 "%s: opts->bias / opts->ngram is not a pointer", what);
    *bt = CbBias{};
    *lt = NgramTables{};
    if (bias) {
        ED_CHECK_ARG(V < 0 || bias->V == V, "%s: the bias list's vocabulary = %d differs from the head's V = %d", what,
                     bias->V, V);
        ED_CHECK_ARG(bias->S > 0 && bias->n_exc >= 0, "%s: bad bias automaton (S %d, exceptions %d)", what, bias->S,
                     bias->n_exc);
        ED_CHECK_ARG(bias->root_next && bias->held && bias->pend && bias->row_ptr && bias->exc_tok && bias->exc_next,
                     "%s: null bias table pointer", what);
        *bt = CbBias{bias->root_next, bias->held, bias->pend, bias->row_ptr, bias->exc_tok, bias->exc_next, bias->S};
    }
    if (lm) {
        if (int rc = ed_ngram_check(lm, what)) return rc;
        ED_CHECK_ARG(V < 0 || lm->V == V, "%s: the n-gram's vocabulary = %d differs from the head's V = %d", what, lm->V,
                     V);
        ED_CHECK_ARG(V < 0 || lm->blank == blank, "%s: the n-gram's blank = %d differs from the search's %d", what,
                     lm->blank, blank);
        ED_CHECK_ARG(isfinite(lm->weight) && lm->weight >= 0.0 && isfinite(lm->length_bonus),
                     "%s: lm weight %g must be finite and >= 0, length_bonus %g finite", what, lm->weight,
                     lm->length_bonus);
        *lt = ed_ngram_tables(lm);
    }
    *has_bias = bias != nullptr;
    *has_lm = lm != nullptr;
    return ED_OK;
}

#define CB_STREAM_CHECK_SHAPE(what, S, W, NC)                                                                     \
    do {                                                                                                          \
        ED_CHECK_ARG(S > 0, what ": S = %d streams (must be > 0)", S);                                            \
        ED_CHECK_ARG(W >= 1 && W <= CB_MAXW, what ": W = %d outside [1,%d]", W, CB_MAXW);                         \
        ED_CHECK_ARG(NC >= W, what ": node_capacity = %d is too small (must be >= W = %d)", NC, W);               \
        ED_CHECK_ARG(cb_stream_dims_ok(S, W, NC), what ": S x W or S x node_capacity exceeds the index range");   \
    } while (0)

}  // namespace

extern "C" size_t edgedict_ctc_stream_state_bytes(int S, int W, int node_capacity) {
    if (!cb_stream_dims_ok(S, W, node_capacity)) return 0;
    return cb_stream_layout(S, W, node_capacity).total;
}

extern "C" size_t edgedict_ctc_stream_workspace_bytes(int S, int Tc, int W, int cand, int node_capacity) {
    if (!cb_stream_dims_ok(S, W, node_capacity) || Tc <= 0 || cand < 1 || cand > CB_MAXC ||
        (long long)S * Tc * cand > 0x7fffffffLL)
        return 0;
    return cb_stream_ws(S, Tc, cand, node_capacity).total;
}

extern "C" int edgedict_ctc_stream_reset(int S, int W, int node_capacity, const edgedict_ctc_beam_opts_t* opts,
                                         const int32_t* mask, void* state, void* stream_) {
    const int NC = node_capacity;
    CB_STREAM_CHECK_SHAPE("ctc_stream_reset", S, W, NC);
    ED_CHECK_ARG(state, "ctc_stream_reset: null pointer argument (state)");
    ED_CHECK_ARG(((uintptr_t)state & 15) == 0, "ctc_stream_reset: state must be 16-byte aligned");
    ED_CHECK_ARG(!mask || (uintptr_t)mask >= 4096, "ctc_stream_reset: mask is not a pointer");
    CbBias bt;
    NgramTables lt;
    bool has_bias, has_lm;
    if (int rc = cb_stream_opts("ctc_stream_reset", opts, -1, -1, &bt, &lt, &has_bias, &has_lm)) return rc;
    const CbStream ss = cb_stream_bind((char*)state, cb_stream_layout(S, W, NC));
    hipLaunchKernelGGL(ctc_stream_reset_kernel, dim3((S + 63) / 64), dim3(64), 0, (hipStream_t)stream_, ss, mask, S, W,
                       NC, has_lm ? lt.lm_start : 0);
    ED_CHECK_LAUNCH("ctc_stream_reset");
    return ED_OK;
}

extern "C" int edgedict_ctc_stream_advance(const void* logits, int dtype, const int32_t* n_frames_host, int S, int Tc,
                                           int V, int blank, int W, int cand, int node_capacity,
                                           const edgedict_ctc_beam_opts_t* opts, int32_t* live_host, void* commit_host,
                                           int max_commit, void* state, void* workspace, void* stream_) {
    const int NC = node_capacity;
    CB_STREAM_CHECK_SHAPE("ctc_stream_advance", S, W, NC);
    ED_CHECK_ARG(Tc > 0, "ctc_stream_advance: Tc = %d frames in the chunk (must be > 0)", Tc);
    ED_CHECK_ARG(V >= 2, "ctc_stream_advance: V = %d, need at least the blank and one symbol", V);
    ED_CHECK_ARG(blank >= 0 && blank < V, "ctc_stream_advance: blank %d outside [0,%d)", blank, V);
    ED_CHECK_ARG(dtype == ED_F32 || dtype == ED_BF16, "ctc_stream_advance: unsupported dtype code %d", dtype);
    ED_CHECK_ARG(cand >= 1 && cand <= CB_MAXC, "ctc_stream_advance: cand = %d outside [1,%d]", cand, CB_MAXC);
    ED_CHECK_ARG(logits && n_frames_host && live_host && commit_host && state && workspace,
                 "ctc_stream_advance: null pointer argument");
    ED_CHECK_ARG((uintptr_t)logits >= 4096 && (uintptr_t)state >= 4096 && (uintptr_t)workspace >= 4096,
                 "ctc_stream_advance: logits / state / workspace is not a pointer");
    ED_CHECK_ARG(((uintptr_t)workspace & 15) == 0 && ((uintptr_t)state & 15) == 0,
                 "ctc_stream_advance: state and workspace must be 16-byte aligned");
    ED_CHECK_ARG((long long)S * Tc * cand <= 0x7fffffffLL, "ctc_stream_advance: S x Tc x cand = %d x %d x %d exceeds 2^31 - 1",
                 S, Tc, cand);
    ED_CHECK_ARG(max_commit >= 0, "ctc_stream_advance: max_commit = %d (must be >= 0)", max_commit);
    CbBias bt;
    NgramTables lt;
    bool has_bias, has_lm;
    if (int rc = cb_stream_opts("ctc_stream_advance", opts, V, blank, &bt, &lt, &has_bias, &has_lm)) return rc;
    int cols = 0;
    for (int s = 0; s < S; ++s) {
        const int nf = n_frames_host[s], lv = live_host[s];
        ED_CHECK_ARG(nf >= 0 && nf <= Tc, "ctc_stream_advance: n_frames[%d] = %d outside [0, %d]", s, nf, Tc);
        ED_CHECK_ARG(lv >= 1 && lv <= NC, "ctc_stream_advance: live[%d] = %d outside [1, %d]", s, lv, NC);
        ED_CHECK_ARG((long long)lv + (long long)nf * W <= NC,
                     "ctc_stream_advance: stream %d may need %lld token-tree nodes (%d live + %d frames x W = %d), "
                     "node_capacity is %d",
                     s, (long long)lv + (long long)nf * W, lv, nf, W, NC);
        cols = std::max(cols, std::min(NC, lv - 1 + nf));      // a hypothesis has at most that many uncommitted tokens
    }
    ED_CHECK_ARG(cols <= max_commit, "ctc_stream_advance: max_commit = %d, this advance may commit %d tokens", max_commit,
                 cols);
    hipStream_t stream = (hipStream_t)stream_;
    char* p = (char*)workspace;
    const CbStreamWs w = cb_stream_ws(S, Tc, cand, NC);
    const CbStream ss = cb_stream_bind((char*)state, cb_stream_layout(S, W, NC));
    float* lse = (float*)(p + w.off_lse);
    float* lpb = (float*)(p + w.off_lpb);
    int32_t* ctok = (int32_t*)(p + w.off_ctok);
    float* clp = (float*)(p + w.off_clp);
    int32_t* nf_dev = (int32_t*)(p + w.off_nf);
    const int K = min(cand, V - 1);

    ED_CHECK_HIP(hipMemcpyAsync(nf_dev, n_frames_host, (size_t)S * 4, hipMemcpyHostToDevice, stream));
    const size_t esz = dtype == ED_F32 ? 4 : 2;
    const int vec_ok = ((V * esz) % 16 == 0) && (((uintptr_t)logits & 15) == 0);
    const dim3 grid1(ed_grid_for(Tc, 4, max(1, 256 * 16 / S)), S);
    if (dtype == ED_F32)
        hipLaunchKernelGGL(ctc_beam_rows<float>, grid1, dim3(256), 0, stream, (const float*)logits,
                           (const int32_t*)nf_dev, Tc, V, blank, K, cand, lse, lpb, ctok, clp, vec_ok);
    else
        hipLaunchKernelGGL(ctc_beam_rows<bf16_t>, grid1, dim3(256), 0, stream, (const bf16_t*)logits,
                           (const int32_t*)nf_dev, Tc, V, blank, K, cand, lse, lpb, ctok, clp, vec_ok);
    ED_CHECK_LAUNCH("ctc_stream_advance (rows)");
#define ED_CB_WALK(TT, BB, LL)                                                                                       \
    hipLaunchKernelGGL((ctc_beam_walk<TT, BB, LL, true>), dim3(S), dim3(64), 0, stream, (const TT*)logits,           \
                       (const int32_t*)nf_dev, Tc, V, W, K, cand, lse, lpb, ctok, clp, ss.nodes, NC, (int32_t*)nullptr, \
                       (int32_t*)nullptr, (int32_t*)nullptr, (double*)nullptr, bt, lt, ss)
#define ED_CB_WALK_T(TT)                                                                          \
    do {                                                                                          \
        if (has_lm) { if (has_bias) ED_CB_WALK(TT, true, true); else ED_CB_WALK(TT, false, true); } \
        else { if (has_bias) ED_CB_WALK(TT, true, false); else ED_CB_WALK(TT, false, false); }      \
    } while (0)
    if (dtype == ED_F32) ED_CB_WALK_T(float); else ED_CB_WALK_T(bf16_t);
#undef ED_CB_WALK_T
#undef ED_CB_WALK
    ED_CHECK_LAUNCH("ctc_stream_advance (walk)");
    hipLaunchKernelGGL(ctc_stream_compact, dim3(S), dim3(64), 0, stream, ss, W, NC, (int32_t*)(p + w.off_remap),
                       (int4*)(p + w.off_commit));
    ED_CHECK_LAUNCH("ctc_stream_advance (compact)");
    // the one read of the advance: every stream's counts and the records this advance can have written
    ED_CHECK_HIP(hipMemcpy2DAsync(commit_host, ((size_t)max_commit + 1) * 16, p + w.off_commit, ((size_t)NC + 1) * 16,
                                  ((size_t)cols + 1) * 16, S, hipMemcpyDeviceToHost, stream));
    ED_CHECK_HIP(hipStreamSynchronize(stream));
    const int32_t* rec = (const int32_t*)commit_host;
    for (int s = 0; s < S; ++s) live_host[s] = rec[(size_t)s * ((size_t)max_commit + 1) * 4 + 1];
    return ED_OK;
}

extern "C" int edgedict_ctc_stream_nbest(int S, int W, int node_capacity, const void* state, int max_tokens,
                                         int32_t* tokens, int32_t* frames, float* token_lp, int32_t* ntok,
                                         int32_t* n_hyp, double* logp, void* stream_) {
    const int NC = node_capacity;
    CB_STREAM_CHECK_SHAPE("ctc_stream_nbest", S, W, NC);
    ED_CHECK_ARG(max_tokens >= 1 && (long long)S * W * max_tokens <= 0x7fffffffLL,
                 "ctc_stream_nbest: max_tokens = %d (must be >= 1, S x W x max_tokens < 2^31)", max_tokens);
    ED_CHECK_ARG(state && tokens && frames && token_lp && ntok && n_hyp && logp,
                 "ctc_stream_nbest: null pointer argument");
    ED_CHECK_ARG(((uintptr_t)state & 15) == 0, "ctc_stream_nbest: state must be 16-byte aligned");
    const CbStream ss = cb_stream_bind((char*)state, cb_stream_layout(S, W, NC));
    hipLaunchKernelGGL(ctc_stream_readout, dim3(S * W), dim3(64), 0, (hipStream_t)stream_, ss, W, NC, max_tokens, tokens,
                       frames, token_lp, ntok, n_hyp, logp);
    ED_CHECK_LAUNCH("ctc_stream_nbest");
    return ED_OK;
}
