// Blank-frame skipping ahead of the RNN-T beam searches for gfx950: the CTC head's blank posterior decides which
// encoder frames a search sees at all.
//
// With z = the head's raw logits [B, T, V] and lp_blank(b, t) = z[blank] - lse(z) (<= 0), frame t < T_b is KEPT iff
// lp_blank(b, t) <= log_thr, log_thr = (float)log(threshold) formed once on the host: a frame on which CTC gives the
// blank more than `threshold` of the mass is dropped.  threshold = 1 keeps every frame (lp_blank is clamped to <= 0).
// The searches then run on the kept frames alone, compacted to the front of a shorter [B, Tc, P] encoder output, and
// frame_map turns a frame number of the short sequence back into the original one.
//
// Kernels (no atomics, results bit-identical from run to run):
//   frame_skip_rows   : one wave64 per row (b, t), the grid of ctc_argmax: row_lse of ctc_rows.hpp, then
//                       lp_blank = min(z[blank] - lse, 0).  Rows t >= T_b are never read; their lp_blank is 0.
//   frame_skip_scan   : ONE WAVE per utterance, 64 frames per pass, ballot + prefix pop-count as ctc_collapse:
//                       frame_map[b, j] = the original index of the j-th kept frame (stable), -1 behind kept[b].
//   frame_skip_gather : out[b, j, :] = enc_out[b, frame_map[b, j], :] for j < kept[b], zeros for kept[b] <= j < Tc (the
//                       padded rows go through the joint's row product and must be defined).  One wave per row, 16-byte
//                       copies when P * esize % 16 == 0 and both pointers are aligned, element copies otherwise.
// A NaN in a row makes its lp_blank NaN, which the clamp turns into 0: such a frame is kept only at threshold 1.
#include "common.hpp"
#include "ctc_rows.hpp"

namespace {

// grid (x, B): 4 waves per block, one row per wave per iteration
template <typename T>
__global__ __launch_bounds__(256) void frame_skip_rows(const T* __restrict__ logits, const int32_t* __restrict__ act_lens,
                                                       int Tm, int V, int blank, float* __restrict__ lp_blank,
                                                       int vec_ok) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.y;
    const int Tb = max(0, min(act_lens[b], Tm));
    for (int t = blockIdx.x * 4 + wave; t < Tm; t += gridDim.x * 4) {
        const long long row = (long long)b * Tm + t;
        float lp = 0.f;
        if (t < Tb) {                                 // (wave-uniform)
            const T* z = logits + row * (long long)V;
            const float l = row_lse<T, false>(z, V, vec_ok, lane, nullptr, nullptr);
            lp = fminf(ElemIO<T>::load(z + blank) - l, 0.f);
        }
        if (lane == 0) lp_blank[row] = lp;
    }
}

// blockIdx.x = utterance, 64 threads
__global__ __launch_bounds__(64) void frame_skip_scan(const float* __restrict__ lp_blank,
                                                      const int32_t* __restrict__ act_lens, int Tm, float log_thr,
                                                      int32_t* __restrict__ frame_map, int32_t* __restrict__ kept) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int Tb = max(0, min(act_lens[b], Tm));
    const long long row0 = (long long)b * Tm;
    int count = 0;
    for (int t0 = 0; t0 < Tb; t0 += 64) {
        const int t = t0 + lane;
        const bool keep = t < Tb && lp_blank[row0 + t] <= log_thr;
        const unsigned long long mask = __ballot(keep);
        if (keep) frame_map[row0 + count + __popcll(mask & ((1ull << lane) - 1ull))] = t;
        count += __popcll(mask);
    }
    for (int t = count + lane; t < Tm; t += 64) frame_map[row0 + t] = -1;
    if (lane == 0) kept[b] = count;
}

// grid (x, B): 4 waves per block, one output row per wave per iteration.  E is an unsigned integer of the element's
// size: the copy never interprets the bits.  A map entry outside [0, Tm) (a raw C-ABI caller may pass one) reads
// nothing and gives a row of zeros.
template <typename E>
__global__ __launch_bounds__(256) void frame_skip_gather(const E* __restrict__ enc, const int32_t* __restrict__ frame_map,
                                                         const int32_t* __restrict__ kept, int Tm, int P, int Tc,
                                                         E* __restrict__ out, int vec_ok) {
    constexpr int VEC = 16 / (int)sizeof(E);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.y;
    const int n = max(0, min(kept[b], Tc));
    for (int j = blockIdx.x * 4 + wave; j < Tc; j += gridDim.x * 4) {
        int src = j < n ? frame_map[(long long)b * Tm + j] : -1;
        if (src >= Tm) src = -1;
        const E* x = enc + ((long long)b * Tm + max(src, 0)) * (long long)P;
        E* y = out + ((long long)b * Tc + j) * (long long)P;
        if (vec_ok) {
            for (int p = lane * VEC; p < P; p += 64 * VEC) {
                uint4 v = make_uint4(0u, 0u, 0u, 0u);
                if (src >= 0) v = *reinterpret_cast<const uint4*>(x + p);
                *reinterpret_cast<uint4*>(y + p) = v;
            }
        } else {
            for (int p = lane; p < P; p += 64) y[p] = src >= 0 ? x[p] : (E)0;
        }
    }
}

inline int frame_skip_check(const char* who, int B, int T, int dtype) {
    ED_CHECK_ARG(B > 0 && T > 0, "%s: B, T must be positive (got %d, %d)", who, B, T);
    ED_CHECK_ARG(B <= 65535, "%s: B = %d exceeds the grid's 65535 utterances per launch", who, B);
    ED_CHECK_ARG((long long)B * T <= 0x7fffffffLL, "%s: B x T = %d x %d exceeds 2^31 - 1", who, B, T);
    ED_CHECK_ARG(dtype == ED_F32 || dtype == ED_BF16, "%s: unsupported dtype code %d", who, dtype);
    return ED_OK;
}

}  // namespace

extern "C" int edgedict_frame_skip_scan(const void* logits, int dtype, const int32_t* act_lens, int B, int T, int V,
                                        int blank, float log_thr, float* lp_blank, int32_t* frame_map, int32_t* kept,
                                        void* stream_) {
    if (int rc = frame_skip_check("frame_skip_scan", B, T, dtype)) return rc;
    ED_CHECK_ARG(V >= 2, "frame_skip_scan: V = %d, need at least the blank and one symbol", V);
    ED_CHECK_ARG(blank >= 0 && blank < V, "frame_skip_scan: blank %d outside [0,%d)", blank, V);
    // log(threshold) of a threshold in (0, 1]: finite and <= 0 (this also refuses a NaN)
    ED_CHECK_ARG(log_thr <= 0.f && log_thr >= -3.0e38f, "frame_skip_scan: log_thr = %g is not the log of a threshold in (0, 1]",
                 (double)log_thr);
    ED_CHECK_ARG(logits && act_lens && lp_blank && frame_map && kept, "frame_skip_scan: null pointer argument");
    hipStream_t stream = (hipStream_t)stream_;
    const size_t esz = dtype == ED_F32 ? 4 : 2;
    const int vec_ok = (((size_t)V * esz) % 16 == 0) && (((uintptr_t)logits & 15) == 0);
    const dim3 grid(ed_grid_for(T, 4, max(1, 256 * 16 / B)), B);
    if (dtype == ED_F32)
        hipLaunchKernelGGL(frame_skip_rows<float>, grid, dim3(256), 0, stream, (const float*)logits, act_lens, T, V,
                           blank, lp_blank, vec_ok);
    else
        hipLaunchKernelGGL(frame_skip_rows<bf16_t>, grid, dim3(256), 0, stream, (const bf16_t*)logits, act_lens, T, V,
                           blank, lp_blank, vec_ok);
    ED_CHECK_LAUNCH("frame_skip_rows");
    hipLaunchKernelGGL(frame_skip_scan, dim3(B), dim3(64), 0, stream, (const float*)lp_blank, act_lens, T, log_thr,
                       frame_map, kept);
    ED_CHECK_LAUNCH("frame_skip_scan");
    return ED_OK;
}

extern "C" int edgedict_frame_skip_gather(const void* enc_out, int dtype, const int32_t* frame_map, const int32_t* kept,
                                          int B, int T, int P, int Tc, void* out, void* stream_) {
    if (int rc = frame_skip_check("frame_skip_gather", B, T, dtype)) return rc;
    ED_CHECK_ARG(P > 0, "frame_skip_gather: P must be positive (got %d)", P);
    ED_CHECK_ARG(Tc >= 1 && Tc <= T, "frame_skip_gather: Tc = %d outside [1, T = %d]", Tc, T);
    ED_CHECK_ARG(enc_out && frame_map && kept && out, "frame_skip_gather: null pointer argument");
    hipStream_t stream = (hipStream_t)stream_;
    const size_t esz = dtype == ED_F32 ? 4 : 2;
    ED_CHECK_ARG(((uintptr_t)enc_out & (esz - 1)) == 0 && ((uintptr_t)out & (esz - 1)) == 0,
                 "frame_skip_gather: enc_out and out must be aligned to their element size");
    const int vec_ok = (((size_t)P * esz) % 16 == 0) && (((uintptr_t)enc_out & 15) == 0) && (((uintptr_t)out & 15) == 0);
    const dim3 grid(ed_grid_for(Tc, 4, max(1, 256 * 16 / B)), B);
    if (dtype == ED_F32)
        hipLaunchKernelGGL(frame_skip_gather<uint32_t>, grid, dim3(256), 0, stream, (const uint32_t*)enc_out, frame_map,
                           kept, T, P, Tc, (uint32_t*)out, vec_ok);
    else
        hipLaunchKernelGGL(frame_skip_gather<uint16_t>, grid, dim3(256), 0, stream, (const uint16_t*)enc_out, frame_map,
                           kept, T, P, Tc, (uint16_t*)out, vec_ok);
    ED_CHECK_LAUNCH("frame_skip_gather");
    return ED_OK;
}
