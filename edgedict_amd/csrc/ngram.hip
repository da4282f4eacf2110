// The back-off n-gram outside a search (gfx950): dense per-state rows and the sentence scorer.  The lookup itself,
// and what it guarantees on corrupt tables, is ngram_tables.hpp's.  No atomics, no host sync, no LDS; results are
// bit-identical from run to run, and - every score being a chain of fp64 additions in the order NGramLM.step states -
// bit-identical to the host's.
//
//   ngram_rows   : ONE WAVE per row r (blockIdx.x, 64 threads).  The back-off chain s_0 = states[r], s_1 = fail(s_0), ...
//                  is at most `order` states long; its prefix sums acc_j = ((0 + backoff[s_0]) + ...) + backoff[s_{j-1}]
//                  are the same additions step() makes on the way down.  The row is then filled from the unigram level
//                  (acc_d + uni_lp[k] for every k, coalesced) UP to the longest context, level j overwriting the
//                  columns of its own arcs with acc_j + arc_lp: a token's final value comes from the longest context
//                  that has it, which is step()'s answer.  Two levels can write the same column from different lanes,
//                  so the levels' stores are ordered (a fence and the one-wave workgroup's barrier between levels).
//   ngram_score  : ONE WAVE per hypothesis.  The tokens are walked in order, wave-uniformly; a row is searched
//                  co-operatively, 64 arcs per load and one ballot (rows are sorted, a round whose first arc is already
//                  beyond the token ends the search), rows longer than 64 arcs take several rounds.  Lane 0 writes.
#include "common.hpp"
#include "ngram_tables.hpp"

namespace {

constexpr int NG_MAX_ORDER = 6;

__global__ __launch_bounds__(64) void ngram_rows(NgramTables lt, const int32_t* __restrict__ states, float* lp,
                                                 int32_t* next) {
    const int r = blockIdx.x, lane = threadIdx.x;
    const int V = lt.lm_V, blank = lt.lm_blank;
    const int s0 = ngram_state(lt, states[r]);
    int chain[NG_MAX_ORDER];
    double acc[NG_MAX_ORDER + 1];
    int d = 0, s = s0;
    acc[0] = 0.0;
#pragma unroll
    for (int it = 0; it < NG_MAX_ORDER; ++it) {
        if (it < lt.lm_order && s != 0) {
            chain[it] = s;
            acc[it + 1] = acc[it] + lt.lm_backoff[s];
            s = ngram_state(lt, lt.lm_fail[s]);
            d = it + 1;
        } else {
            chain[it] = 0;
            acc[it + 1] = acc[it];
        }
    }
    float* row = lp + (long long)r * V;
    int32_t* nrow = next ? next + (long long)r * V : nullptr;
    const double base = acc[NG_MAX_ORDER];          // = acc[d]: the levels behind the chain add nothing
    for (int k = lane; k < V; k += 64) {
        const bool isb = k == blank;
        row[k] = isb ? 0.f : (float)(base + lt.lm_uni_lp[k]);
        if (nrow) nrow[k] = isb ? s0 : ngram_state(lt, lt.lm_uni_next[k]);
    }
#pragma unroll
    for (int j = NG_MAX_ORDER - 1; j >= 0; --j) {
        if (j >= d) continue;                       // (wave-uniform)
        __threadfence_block();
        __syncthreads();
        int lo, hi;
        ngram_row(lt, chain[j], lo, hi);
        const double a = acc[j];
        for (int i = lo + lane; i < hi; i += 64) {
            const int k = lt.lm_arc_tok[i];
            if (k < 0 || k >= V || k == blank) continue;          // eos, or a corrupt entry
            row[k] = (float)(a + lt.lm_arc_lp[i]);
            if (nrow) nrow[k] = ngram_state(lt, lt.lm_arc_next[i]);
        }
    }
}

// step(s, k) by the whole wave: wave-uniform arguments and results
__device__ __forceinline__ double ngram_step_wave(const NgramTables& lt, int s, int k, int lane, int* next) {
    s = ngram_state(lt, s);
    k = min(max(k, 0), lt.lm_V);
    double acc = 0.0;
    for (int it = 0; it < lt.lm_order && s != 0; ++it) {
        int lo, hi;
        ngram_row(lt, s, lo, hi);
        for (int base = lo; base < hi; base += 64) {
            const int i = base + lane;
            const int t = i < hi ? lt.lm_arc_tok[i] : 0x7fffffff;
            const unsigned long long hit = __ballot(t == k);
            if (hit) {
                const int at = base + (__ffsll((long long)hit) - 1);
                *next = ngram_state(lt, lt.lm_arc_next[at]);
                return acc + lt.lm_arc_lp[at];
            }
            if (__builtin_amdgcn_readfirstlane(t) > k) break;     // sorted: the token is not in this row
        }
        acc = acc + lt.lm_backoff[s];
        s = ngram_state(lt, lt.lm_fail[s]);
    }
    *next = ngram_state(lt, lt.lm_uni_next[k]);
    return acc + lt.lm_uni_lp[k];
}

__global__ __launch_bounds__(64) void ngram_score(NgramTables lt, const int32_t* __restrict__ hyps,
                                                  const int32_t* __restrict__ hyp_lens,
                                                  const int32_t* __restrict__ n_hyp, int N, int U, int bos, int eos,
                                                  double* __restrict__ total, float* __restrict__ token_lp) {
    const int bn = blockIdx.x, b = bn / N, n = bn - b * N, lane = threadIdx.x;
    const long long o = (long long)bn * U;
    const bool live = !n_hyp || n < n_hyp[b];
    const int len = live ? max(0, min(hyp_lens[bn], U)) : 0;
    if (token_lp)
        for (int u = len + lane; u < U; u += 64) token_lp[o + u] = 0.f;
    const double NEG = -(double)INFINITY;
    double sum = live ? 0.0 : NEG;
    int s = bos ? lt.lm_start : 0;
    bool ok = live;
    for (int u = 0; u < len; ++u) {
        const int k = hyps[o + u];
        double l = 0.0;
        if (ok) {
            if (k < 0 || k >= lt.lm_V || k == lt.lm_blank) {
                ok = false;
                sum = NEG;
                l = NEG;
            } else {
                int nx;
                l = ngram_step_wave(lt, s, k, lane, &nx);
                s = nx;
                sum = sum + l;
            }
        }
        if (token_lp && lane == 0) token_lp[o + u] = (float)l;
    }
    if (ok && eos) {
        int nx;
        sum = sum + ngram_step_wave(lt, s, lt.lm_V, lane, &nx);
    }
    if (lane == 0) total[bn] = sum;
}

}  // namespace

// the checks every entry point that takes an n-gram makes, before any launch; `what` names the entry point
int ed_ngram_check(const edgedict_ngram_lm_t* lm, const char* what) {
    ED_CHECK_ARG((uintptr_t)lm >= 4096, "%s: the n-gram is not a pointer", what);
    ED_CHECK_ARG(lm->V >= 2, "%s: the n-gram's V = %d, need at least the blank and one symbol", what, lm->V);
    ED_CHECK_ARG(lm->order >= 1 && lm->order <= NG_MAX_ORDER, "%s: the n-gram's order = %d outside [1, %d]", what,
                 lm->order, NG_MAX_ORDER);
    ED_CHECK_ARG(lm->S > 0 && lm->n_arcs >= 0, "%s: bad n-gram tables (S %d, arcs %d)", what, lm->S, lm->n_arcs);
    ED_CHECK_ARG(lm->start >= 0 && lm->start < lm->S, "%s: the n-gram's start state %d outside [0, %d)", what, lm->start,
                 lm->S);
    ED_CHECK_ARG(lm->blank >= 0 && lm->blank < lm->V, "%s: the n-gram's blank %d outside [0, %d)", what, lm->blank,
                 lm->V);
    ED_CHECK_ARG(lm->uni_lp && lm->uni_next && lm->row_ptr && lm->fail && lm->backoff && lm->arc_tok && lm->arc_lp &&
                     lm->arc_next,
                 "%s: null n-gram table pointer", what);
    return ED_OK;
}

NgramTables ed_ngram_tables(const edgedict_ngram_lm_t* lm) {
    return NgramTables{lm->uni_lp, lm->uni_next, lm->row_ptr, lm->fail,  lm->backoff, lm->arc_tok, lm->arc_lp,
                       lm->arc_next, lm->V,      lm->order,  lm->S,      lm->n_arcs,  lm->start,   lm->blank,
                       lm->weight,   lm->length_bonus};
}

extern "C" size_t edgedict_ngram_lm_struct_bytes(void) { return sizeof(edgedict_ngram_lm_t); }

extern "C" int edgedict_ngram_logprobs(const edgedict_ngram_lm_t* lm, const int32_t* states, int R, float* lp,
                                       int32_t* next, void* stream_) {
    if (int rc = ed_ngram_check(lm, "ngram_logprobs")) return rc;
    ED_CHECK_ARG(R > 0, "ngram_logprobs: R = %d must be positive", R);
    ED_CHECK_ARG(states && lp, "ngram_logprobs: null pointer argument");
    ED_CHECK_ARG((long long)R * lm->V <= 0x7fffffffLL, "ngram_logprobs: R x V = %d x %d exceeds 2^31 - 1", R, lm->V);
    hipLaunchKernelGGL(ngram_rows, dim3(R), dim3(64), 0, (hipStream_t)stream_, ed_ngram_tables(lm), states, lp, next);
    ED_CHECK_LAUNCH("ngram_rows");
    return ED_OK;
}

extern "C" int edgedict_ngram_score(const edgedict_ngram_lm_t* lm, const int32_t* hyps, const int32_t* hyp_lens,
                                    const int32_t* n_hyp, int B, int N, int U, int bos, int eos, double* total,
                                    float* token_lp, void* stream_) {
    if (int rc = ed_ngram_check(lm, "ngram_score")) return rc;
    ED_CHECK_ARG(B > 0 && N > 0, "ngram_score: B, N must be positive (got %d, %d)", B, N);
    ED_CHECK_ARG(U >= 0, "ngram_score: U = %d must not be negative", U);
    ED_CHECK_ARG(hyp_lens && total && (hyps || U == 0), "ngram_score: null pointer argument");
    ED_CHECK_ARG((long long)B * N * max(U, 1) <= 0x7fffffffLL, "ngram_score: B x N x U = %d x %d x %d exceeds 2^31 - 1", B,
                 N, U);
    hipLaunchKernelGGL(ngram_score, dim3(B * N), dim3(64), 0, (hipStream_t)stream_, ed_ngram_tables(lm), hyps, hyp_lens,
                       n_hyp, N, U, bos, eos, total, U ? token_lp : nullptr);
    ED_CHECK_LAUNCH("ngram_score");
    return ED_OK;
}
