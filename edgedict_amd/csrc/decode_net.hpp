// The search network and the buffers of one search step, stated once for decode.hip (the search loops, a step composed
// from the general kernels) and decode_fused.hip (the same step as fused launches).  Host-side only.
#pragma once
#include "common.hpp"

static inline size_t align256(size_t x) { return (x + 255) / 256 * 256; }

// f(ET{}) with ET = the element type of `dtype`: the one place a kernel template is picked from a dtype code
template <typename F>
static inline void dispatch(int dtype, F&& f) {
    if (dtype == ED_F32) f(float{});
    else f(bf16_t{});
}

// Embedding -> L LSTM layers -> Linear.  The transducer's prediction network (Wo = its projection, O = P2) and the
// fusion LM (edgedict_beam_lm_t: Wo = its decoder, O = V) are both one.
struct LstmNet {
    const void* emb;                 // [V, E] in emb_dtype
    int emb_dtype, V, E, L;
    const void* const* w_ih;         // HOST arrays [L] of DEVICE pointers: [4H, E or H], [4H, H] in the search's dtype,
    const void* const* w_hh;         // fp32 [4H]
    const float* const* b_ih;
    const float* const* b_hh;
    int H;
    const void* Wo;                  // [O, H] in the search's dtype
    const float* bo;                 // fp32 [O]
    int O;
};

// the fusion LM as an LstmNet (its decoder is the output layer, O = V)
static inline LstmNet lm_net_of(const edgedict_beam_lm_t& lm) {
    return LstmNet{lm.emb, lm.emb_dtype, lm.V, lm.E, lm.L, lm.w_ih, lm.w_hh, lm.b_ih, lm.b_hh, lm.H, lm.Wo, lm.bo, lm.V};
}

// Weights and shapes of one search call, as the extern "C" searches take them (include/edgedict_hip.h)
struct SearchNet {
    int dtype, esz;
    const void* E1;                  // the joint's encoder rows; row b of frame t at (b * e_row_stride + t * e_frame_stride)
    long long e_row_stride, e_frame_stride;
    int B, J;
    const void* W1d;                 // joint: hid = tanh(E1 + pred W1d^T + b1), logits = hid W2^T + b2
    long long ldw1;
    const float* b1;
    int P2;
    const void* W2;
    const float* b2;
    int V;
    LstmNet pred;                    // the prediction network
    int blank;
    int bos, W, EM, NODES;           // beam searches only: width, expansions per frame, token-tree capacity per utterance
    const char* frame(int t) const { return (const char*)E1 + (size_t)t * e_frame_stride * esz; }
};

// The public network (edgedict_search_net_t, non-null) as the SearchNet of a call over `rows` rows; a size query passes
// no E1 and reads the shapes alone
static inline SearchNet search_net_of(const edgedict_search_net_t& n, const void* E1, long long e_row_stride,
                                      long long e_frame_stride, int rows, int W, int EM, int NODES) {
    return SearchNet{n.dtype, n.dtype == ED_F32 ? 4 : 2, E1, e_row_stride, e_frame_stride, rows, n.J, n.W1d, n.ldw1, n.b1,
                     n.P2, n.W2, n.b2, n.V,
                     {n.emb, n.emb_dtype, n.V, n.E, n.L, n.w_ih, n.w_hh, n.b_ih, n.b_hh, n.H, n.Wp, n.bp, n.P2},
                     n.blank, n.bos, W, EM, NODES};
}
// An address in the first page is no object: it is an integer that a caller written for ABI version 1 (positional
// network arguments) left where `net` or `opts` now stand.  Such a call is refused, never dereferenced.
static inline bool not_a_pointer(const void* p) { return p && (uintptr_t)p < 4096; }
static inline bool search_ptrs_ok(const edgedict_search_net_t* n, const edgedict_search_opts_t* o) {
    return !not_a_pointer(n) && !not_a_pointer(o);
}
// the optional features of a call: a null pointer is all members null
static inline edgedict_search_opts_t search_opts_of(const edgedict_search_opts_t* o) {
    return o ? *o : edgedict_search_opts_t{};
}

// The argument checks the searches share, in the order they have always run: dtype, shape, null pointers, and for the
// beam searches blank / bos.  shape_ok / ptrs_ok carry the caller's own conditions, shape_note the tail of its message.
static inline int check_net(const SearchNet& n, const char* what, bool shape_ok, const char* shape_note, bool ptrs_ok,
                            bool beam) {
    const LstmNet& p = n.pred;
    ED_CHECK_ARG(n.dtype == ED_F32 || n.dtype == ED_BF16, "%s: bad dtype", what);
    ED_CHECK_ARG(shape_ok && n.B > 0 && n.J > 0 && n.V > 0 && p.L > 0 && p.H > 0 && n.P2 > 0 && p.E > 0, "%s: bad shape%s",
                 what, shape_note);
    ED_CHECK_ARG(ptrs_ok && n.W1d && n.b1 && n.W2 && n.b2 && p.emb && p.w_ih && p.w_hh && p.b_ih && p.b_hh && p.Wo && p.bo,
                 "%s: null pointer", what);
    ED_CHECK_ARG(!beam || (n.blank >= 0 && n.blank < n.V && n.bos >= 0 && n.bos < n.V),
                 "%s: blank/bos outside the vocabulary", what);
    return ED_OK;
}
// every utterance's frame count inside [0, T]; *maxlen = the largest
static inline int check_lens(const int32_t* lens_host, int B, int T, const char* what, int* maxlen) {
    *maxlen = 0;
    for (int b = 0; b < B; ++b) {
        ED_CHECK_ARG(lens_host[b] >= 0 && lens_host[b] <= T, "%s: lens[%d] = %d outside [0, %d]", what, b, lens_host[b], T);
        *maxlen = lens_host[b] > *maxlen ? lens_host[b] : *maxlen;
    }
    return ED_OK;
}

// Per-iteration buffers of the prediction-network step and the joint: offsets into a workspace ...
struct Ws {
    size_t D1, hid, logits, pred, x, G, Hprev, Y0, Y1, Cst, h_new, c_new, dec_new, total;
};
static inline Ws ws_layout(const SearchNet& n) {
    const int esz = n.esz, B = n.B, J = n.J, V = n.V, E = n.pred.E, L = n.pred.L, H = n.pred.H, P2 = n.P2;
    Ws w;
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t r = o; o += align256(bytes); return r; };
    w.D1 = take((size_t)B * J * esz);
    w.hid = take((size_t)B * J * esz);
    w.logits = take((size_t)B * V * 4);
    w.pred = take((size_t)B * 4);
    w.x = take((size_t)B * E * esz);
    w.G = take((size_t)B * 4 * H * esz);
    w.Hprev = take((size_t)B * H * esz);
    w.Y0 = take((size_t)B * H * esz);
    w.Y1 = take((size_t)B * H * esz);
    w.Cst = take((size_t)B * H * 4);
    w.h_new = take((size_t)L * B * H * 4);
    w.c_new = take((size_t)L * B * H * 4);
    w.dec_new = take((size_t)B * P2 * esz);
    w.total = o;
    return w;
}
// ... and the pointers.  An LM's step uses the same bundle (no D1 / hid / dec_new; logits = its output).
struct StepBufs {
    void *D1, *hid;                  // [B, J]
    float* logits;                   // fp32 [B, V]; the fused greedy frame keeps its slice partials here instead
    int32_t* pred;                   // [B] the symbol the network consumes
    void *x, *G, *Hprev, *Y[2];      // embedding rows, gate pre-activations, LSTM scratch, layer outputs (ping-pong)
    float *Cst, *h_new, *c_new;      // h_new / c_new: [L, B, H] candidates
    void* dec_new;                   // [B, P2]
};
static inline StepBufs bind(char* p, const Ws& w) {
    return {p + w.D1, p + w.hid, (float*)(p + w.logits), (int32_t*)(p + w.pred), p + w.x, p + w.G, p + w.Hprev,
            {p + w.Y0, p + w.Y1}, (float*)(p + w.Cst), (float*)(p + w.h_new), (float*)(p + w.c_new), p + w.dec_new};
}

// decode_fused.hip: a step as fused launches, for the shapes *_ok accepts (otherwise decode.hip composes it)
bool ed_decode_fused_ok(int dtype, int emb_dtype, int J, int V, int E, int H, int P2);
bool ed_decode_fused_lm_ok(int dtype, int emb_dtype, int V, int E, int H);
size_t ed_decode_fused_ws_bytes(int B, int V);
// what the greedy frame does with its pick (the beam search's steps take their symbol from u.pred instead)
struct GreedyOut {
    int unk;
    int32_t* tokens;
    long long tok_stride;
    int t;
    float* score;
};
int ed_decode_fused_frame(const SearchNet& net, const void* E1t, float* h_state, float* c_state, void* dec_out,
                          const GreedyOut& out, const StepBufs& u, hipStream_t s);
int ed_decode_fused_beam_step(const SearchNet& net, const void* E1t, const float* h_state, const float* c_state,
                              const StepBufs& u, hipStream_t s);
// decode.hip: the same step composed from the general kernels, for any shape
int ed_decode_composed_beam_step(const SearchNet& net, const void* E1t, const float* h_state, const float* c_state,
                                 const StepBufs& u, hipStream_t s);
// Internal-LM estimation (decode_sync.hip, ilm_score.hip).  The internal LM's logits of a row are the joint on an
// all-zero encoder row.  The *_step_ilm forms are the beam step plus those logits for the same rows: fused, hid2 [2 B, J]
// and logits2 fp32 [2 B, V] hold the step's rows and then the internal LM's (u.hid / u.logits are not written); composed,
// u.logits as ever and ilm_logits fp32 [B, V] (zero_row: J zero elements, ilm_hid [B, J] scratch).  The *_ilm_logits
// forms are the internal LM's logits alone for net.B rows of prediction-network output `dec` [B, P2].
int ed_decode_fused_beam_step_ilm(const SearchNet& net, const void* E1t, const float* h_state, const float* c_state,
                                  const StepBufs& u, void* hid2, float* logits2, hipStream_t s);
int ed_decode_composed_beam_step_ilm(const SearchNet& net, const void* E1t, const float* h_state, const float* c_state,
                                     const StepBufs& u, const void* zero_row, void* ilm_hid, float* ilm_logits,
                                     hipStream_t s);
int ed_decode_fused_ilm_logits(const SearchNet& net, const void* dec, void* hid, float* logits, hipStream_t s);
int ed_decode_composed_ilm_logits(const SearchNet& net, const void* dec, const void* zero_row, void* d1, void* hid,
                                  float* logits, hipStream_t s);
int ed_decode_fused_lm_step(int dtype, int B, const LstmNet& lm, const float* h_state, const float* c_state,
                            const StepBufs& u, hipStream_t s);
// decode.hip: one LM step for `rows` rows, token u.pred[r] from (h_state, c_state) [L, rows, H] -> u.h_new / u.c_new and
// fp32 logits u.logits [rows, V]: the fused step where ed_decode_fused_lm_ok holds, the composed one otherwise
int ed_decode_lm_step(int dtype, int rows, const LstmNet& lm, const float* h_state, const float* c_state,
                      const StepBufs& u, hipStream_t s);
// decode.hip: an LM / a bias list that a search over the vocabulary V can use: ED_OK, or a status with a message
int ed_decode_lm_check(const edgedict_beam_lm_t* lm, int V, int prefix, const char* what);
int ed_decode_bias_check(const edgedict_beam_bias_t* bias, int V, int prefix, const char* what);
