// Batched edit distance for gfx950: the error counts (distance, substitutions, deletions, insertions) of up to 32
// hypotheses per utterance against the utterance's reference - what an error rate (metrics.py: token / word error rate,
// the oracle rate of an N-best list, the expected number of errors) is made of.
//
// Hypotheses hyps [B, N, Uh] int32 with hyp_lens [B, N] and n_hyp [B] live slots (the layout of ctc_score.hip, so
// N-best lists go in as they already travel), references refs [B, Ur] int32 with ref_lens [B]; symbols are compared with
// == only, every int32 value is a symbol.  With h = hyps[b, n, :H] and r = refs[b, :R], d(i, j) is the cheapest way to
// turn r[:j] into h[:i] with the integer edge costs
//     hit            h[i-1] == r[j-1]                                   0
//     substitution   otherwise                                          K
//     deletion       a reference element without a hypothesis element   K        (j-1 -> j)
//     insertion      a hypothesis element without a reference element   K + 1    (i-1 -> i)
// K = 4096, d(0, j) = j K, d(i, 0) = i (K + 1).  For H, R <= 1023 the value v = d(H, R) decomposes exactly:
// dist = v / K is the Levenshtein distance and ins = v % K (<= 1023 < K) the number of insertions of the
// minimum-distance alignment with the FEWEST insertions; ins - del = H - R is fixed, so that alignment also has the fewest
// deletions and the most substitutions: del = ins - (H - R), sub = dist - ins - del.  out[b, n] = (dist, sub, del, ins);
// -1 in all four for the slots n >= n_hyp[b].  The largest value formed is 1023 * 4097: int32 throughout.
//
//   edit_distance_walk<C> : ONE WAVE per (b, n), blockIdx.x = b N + n, so an utterance's hypotheses - which share the
//                    reference - sit in adjacent workgroups.  Lane l owns the C consecutive reference columns
//                    j in (C l, C l + C]; the lane's C reference symbols stay in registers for the whole walk.  The
//                    wave walks the hypothesis row by row on e(i, j) = d(i, j) - j K, in which a deletion costs
//                    nothing: e(i, j) = min(e(i-1, j) + K + 1, e(i-1, j-1) - (hit ? K : 0), e(i, j-1)), e(i, 0) =
//                    i (K + 1), e(0, j) = 0.  Per row a lane makes one serial pass over its C columns (the up and the
//                    diagonal term, a running minimum), the deletion chain across lanes is an inclusive min-scan of the
//                    lanes' minima (row_shr:1/2/4/8, row_bcast:15, row_bcast:31 DPP moves), and ONE wave_shr:1 move
//                    hands lane l the scan of lane l - 1 - which is at once the value entering its columns from the
//                    left and the diagonal term of its first column in the next row.  Hypothesis tokens are read 64
//                    at a time, one per lane, one block ahead of the rows that use them, and handed out by readlane.
//                    Columns behind R compute values nobody uses: data only moves towards higher columns.
//                                                                                                   latency-bound.
// Tokens behind hyp_lens / ref_lens and the slots behind n_hyp are never read.  No LDS, no atomics, no MFMA, no
// workspace; one launch, bit-identical from run to run.
#include "common.hpp"

#include <limits.h>

namespace {

constexpr int EDIT_MAX_N = 32;
constexpr int EDIT_MAX_U = 1023;
constexpr int EDIT_K = 4096;

// min(v, v of the lane the DPP pattern `CTRL` names); a lane without a source, or in a row outside `ROWS`, keeps v
template <int CTRL, int ROWS>
__device__ __forceinline__ int edit_dpp_min(int v) {
    return min(v, __builtin_amdgcn_update_dpp(INT_MAX, v, CTRL, ROWS, 0xf, false));
}

// inclusive min-scan over the 64 lanes
__device__ __forceinline__ int edit_wave_scan_min(int v) {
    v = edit_dpp_min<0x111, 0xf>(v);                 // row_shr:1
    v = edit_dpp_min<0x112, 0xf>(v);                 // row_shr:2
    v = edit_dpp_min<0x114, 0xf>(v);                 // row_shr:4
    v = edit_dpp_min<0x118, 0xf>(v);                 // row_shr:8: every row of 16 lanes is scanned
    v = edit_dpp_min<0x142, 0xa>(v);                 // row_bcast:15 into rows 1 and 3
    v = edit_dpp_min<0x143, 0xc>(v);                 // row_bcast:31 into rows 2 and 3
    return v;
}

// blockIdx.x = b N + n, 64 threads, all of them active in every DPP move.
template <int C>
__global__ __launch_bounds__(64) void edit_distance_walk(const int32_t* __restrict__ hyps,
                                                         const int32_t* __restrict__ hyp_lens,
                                                         const int32_t* __restrict__ n_hyp,
                                                         const int32_t* __restrict__ refs,
                                                         const int32_t* __restrict__ ref_lens, int N, int Uh, int Ur,
                                                         int32_t* __restrict__ out) {
    const int b = blockIdx.x / N, n = blockIdx.x - b * N;
    const int lane = threadIdx.x;
    int32_t* o = out + (long long)blockIdx.x * 4;
    const int live = n_hyp ? max(0, min(n_hyp[b], N)) : N;
    if (n >= live) {
        if (lane < 4) o[lane] = -1;
        return;
    }
    const int H = max(0, min(hyp_lens[blockIdx.x], Uh));
    const int R = max(0, min(ref_lens[b], Ur));
    const int32_t* y = hyps + (long long)blockIdx.x * Uh;
    const int32_t* r = refs + (long long)b * Ur;
    int rk[C];                                       // the lane's reference symbols (columns behind R: unused)
    int prev[C];                                     // e(i - 1, .) of the lane's columns
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const int k = C * lane + c;                  // column j = k + 1
        rk[c] = k < R ? r[k] : 0;
        prev[c] = 0;
    }
    int left = 0;                                    // e(i - 1, C lane): lane 0's is the boundary (i - 1)(K + 1)
    int tok = lane < H ? y[lane] : 0;                // rows i0 + 1 .. i0 + 64, one per lane
    for (int i0 = 0; i0 < H; i0 += 64) {
        const int cur = tok;
        tok = i0 + 64 + lane < H ? y[i0 + 64 + lane] : 0;
        const int rows = min(64, H - i0);
        for (int ii = 0; ii < rows; ++ii) {
            const int h = __builtin_amdgcn_readlane(cur, ii);
            const int edge = (i0 + ii + 1) * (EDIT_K + 1);                  // e(i, 0)
            int diag = left, run = INT_MAX;
            int loc[C];
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const int u = min(prev[c] + (EDIT_K + 1), diag - (rk[c] == h ? EDIT_K : 0));
                diag = prev[c];
                run = min(run, u);
                loc[c] = run;
            }
            if (lane == 0) run = min(run, edge);
            const int scan = edit_wave_scan_min(run);
            left = __builtin_amdgcn_update_dpp(0, scan, 0x138, 0xf, 0xf, false);   // wave_shr:1
            if (lane == 0) left = edge;
#pragma unroll
            for (int c = 0; c < C; ++c) prev[c] = min(left, loc[c]);
        }
    }
    // d(H, R) = e(H, R) + R K; column R is slot (R - 1) % C of lane (R - 1) / C.  R = 0: the boundary H (K + 1)
    int v = 0;
#pragma unroll
    for (int c = 0; c < C; ++c)
        if (C * lane + c == R - 1) v = prev[c];
    v = __shfl(v, R >= 1 ? (R - 1) / C : 0, 64) + R * EDIT_K;
    if (R == 0) v = H * (EDIT_K + 1);
    const int dist = v / EDIT_K, ins = v % EDIT_K;
    const int del = ins - (H - R), sub = dist - ins - del;
    if (lane < 4) o[lane] = lane == 0 ? dist : (lane == 1 ? sub : (lane == 2 ? del : ins));
}

}  // namespace

extern "C" int edgedict_edit_distance(const int32_t* hyps, const int32_t* hyp_lens, const int32_t* n_hyp,
                                      const int32_t* refs, const int32_t* ref_lens, int B, int N, int Uh, int Ur,
                                      int32_t* out, void* stream_) {
    ED_CHECK_ARG(B >= 1, "edit_distance: B must be positive (got %d)", B);
    ED_CHECK_ARG(N >= 1 && N <= EDIT_MAX_N, "edit_distance: N = %d outside [1, %d] hypotheses per utterance", N,
                 EDIT_MAX_N);
    ED_CHECK_ARG(Uh >= 0 && Uh <= EDIT_MAX_U, "edit_distance: Uh = %d outside [0, %d] tokens per hypothesis", Uh,
                 EDIT_MAX_U);
    ED_CHECK_ARG(Ur >= 0 && Ur <= EDIT_MAX_U, "edit_distance: Ur = %d outside [0, %d] tokens per reference", Ur,
                 EDIT_MAX_U);
    ED_CHECK_ARG((long long)B * N <= 0x7fffffffLL, "edit_distance: B * N = %lld exceeds the grid", (long long)B * N);
    ED_CHECK_ARG((hyps || Uh == 0) && hyp_lens && (refs || Ur == 0) && ref_lens && out,
                 "edit_distance: null pointer argument");
    hipStream_t stream = (hipStream_t)stream_;
#define ED_EDIT(CC)                                                                                                   \
    hipLaunchKernelGGL((edit_distance_walk<CC>), dim3(B * N), dim3(64), 0, stream, hyps, hyp_lens, n_hyp, refs,       \
                       ref_lens, N, Uh, Ur, out)
    // C = ceil(Ur / 64) reference columns per lane, rounded up to a power of two, from the call's Ur
    const int per_lane = (Ur + 63) / 64;
    if (per_lane <= 1) ED_EDIT(1);
    else if (per_lane <= 2) ED_EDIT(2);
    else if (per_lane <= 4) ED_EDIT(4);
    else if (per_lane <= 8) ED_EDIT(8);
    else ED_EDIT(16);
#undef ED_EDIT
    ED_CHECK_LAUNCH("edit_distance_walk");
    return ED_OK;
}
