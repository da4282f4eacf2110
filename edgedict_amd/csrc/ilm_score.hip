// The transducer's internal LM as a scorer (gfx950): per-token log P_ILM(y_u | y_<u) of teacher-forced label sequences,
// the number one looks at (as a perplexity) to choose the ilm_weight of the frame-synchronous search (decode_sync.hip).
//
// The internal LM's logits of a row of prediction-network output d [P2] are the joint on an all-zero encoder row,
//   z_ilm = tanh(act(d W1d^T + b1)) W2^T + b2,
// bit for bit what the search's step computes for the same row: the fused step's kernels (dec_joint_hidden_ilm in its
// single-epilogue form, dec_logits_pick) where ed_decode_fused_ok holds, the general kernels on a zero row otherwise.
// ilm_logprob_rows then reads a row's logits with one wave: the log-sum-exp over the NON-BLANK symbols in fp32, in the
// row kernel's form (z - max) - log(sum exp(z - max)), and the target's value.  No atomics: the same bits every run.
#include "decode_net.hpp"

namespace {

// out[b, u] = lp_ilm[b, u][targets[b, u]] for u < ylen[b], else 0.  A blank target has probability 0 under the internal
// LM (-inf); a target outside the vocabulary gives NaN.  4 waves per workgroup, one row each.
__global__ __launch_bounds__(256) void ilm_logprob_rows(const float* __restrict__ logits, const int32_t* __restrict__ targets,
                                                        const int32_t* __restrict__ ylen, float* __restrict__ out, int B,
                                                        int U, int V, int blank) {
    const int lane = threadIdx.x & 63;
    const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= (long long)B * U) return;
    const int b = (int)(r / U), u = (int)(r % U);
    if (u >= ylen[b]) {
        if (lane == 0) out[r] = 0.f;
        return;
    }
    const float* z = logits + r * V;
    float m = -INFINITY;
    for (int v = lane; v < V; v += 64)
        if (v != blank) m = fmaxf(m, z[v]);
    m = wave_max(m);
    float s = 0.f;
    for (int v = lane; v < V; v += 64)
        if (v != blank) s += expf(z[v] - m);
    s = wave_sum(s);
    if (lane != 0) return;
    const int k = targets[r];
    float lp;
    if (k < 0 || k >= V) lp = NAN;
    else if (k == blank) lp = -INFINITY;
    else lp = (z[k] - m) - logf(s);
    out[r] = lp;
}

struct IlmWs {
    size_t d1, hid, zero_row, total;
};
IlmWs ilm_layout(size_t R, size_t J, size_t esz) {
    IlmWs w{};
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t r = o; o += align256(bytes); return r; };
    w.d1 = take(R * J * esz);
    w.hid = take(R * J * esz);
    w.zero_row = take(J * esz);
    w.total = o;
    return w;
}

}  // namespace

extern "C" size_t edgedict_ilm_workspace_bytes(int dtype, int R, int J) {
    if ((dtype != ED_F32 && dtype != ED_BF16) || R <= 0 || J <= 0) return 0;
    return ilm_layout(R, J, dtype == ED_F32 ? 4 : 2).total;
}

extern "C" int edgedict_ilm_logits(int dtype, const void* dec, int R, int P2, int J, const void* W1d, long long ldw1,
                                   const float* b1, const void* W2, const float* b2, int V, int emb_dtype, int E, int H,
                                   float* logits, void* workspace, void* stream_) {
    ED_CHECK_ARG(dtype == ED_F32 || dtype == ED_BF16, "ilm_logits: bad dtype");
    ED_CHECK_ARG(R > 0 && P2 > 0 && J > 0 && V > 0 && E > 0 && H > 0 && ldw1 >= P2,
                 "ilm_logits: bad shape (R=%d P2=%d J=%d V=%d)", R, P2, J, V);
    ED_CHECK_ARG(emb_dtype == ED_F32 || emb_dtype == ED_BF16, "ilm_logits: bad embedding dtype");
    ED_CHECK_ARG(dec && W1d && b1 && W2 && b2 && logits && workspace, "ilm_logits: null pointer");
    hipStream_t s = (hipStream_t)stream_;
    SearchNet net{};
    net.dtype = dtype; net.esz = dtype == ED_F32 ? 4 : 2;
    net.B = R; net.J = J; net.W1d = W1d; net.ldw1 = ldw1; net.b1 = b1; net.P2 = P2; net.W2 = W2; net.b2 = b2; net.V = V;
    const IlmWs w = ilm_layout(R, J, net.esz);
    char* p = (char*)workspace;
    if (ed_decode_fused_ok(dtype, emb_dtype, J, V, E, H, P2)) return ed_decode_fused_ilm_logits(net, dec, p + w.hid, logits, s);
    ED_CHECK_HIP(hipMemsetAsync(p + w.zero_row, 0, (size_t)J * net.esz, s));
    return ed_decode_composed_ilm_logits(net, dec, p + w.zero_row, p + w.d1, p + w.hid, logits, s);
}

extern "C" int edgedict_ilm_logprobs(const float* logits, const int32_t* targets, const int32_t* ylen, int B, int U, int V,
                                     int blank, float* out, void* stream_) {
    ED_CHECK_ARG(B > 0 && U > 0 && (long long)B * U <= 0x7fffffffLL, "ilm_logprobs: bad shape (B=%d U=%d)", B, U);
    ED_CHECK_ARG(V >= 2, "ilm_logprobs: V = %d, need at least the blank and one symbol", V);
    ED_CHECK_ARG(blank >= 0 && blank < V, "ilm_logprobs: blank %d outside [0,%d)", blank, V);
    ED_CHECK_ARG(logits && targets && ylen && out, "ilm_logprobs: null pointer");
    const long long rows = (long long)B * U;
    hipLaunchKernelGGL(ilm_logprob_rows, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream_, logits,
                       targets, ylen, out, B, U, V, blank);
    ED_CHECK_LAUNCH("ilm_logprobs");
    return ED_OK;
}
