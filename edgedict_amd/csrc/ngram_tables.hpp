// The back-off n-gram's device lookup (edgedict_ngram_lm_t, include/edgedict_hip.h), shared by csrc/ngram.hip (dense
// rows, sentence scorer) and ctc_decode.hip's CTC prefix search.  P is the kernel's argument block; it names the tables
// lm_uni_lp / lm_uni_next [V + 1], lm_row_ptr [S + 1], lm_fail / lm_backoff [S], lm_arc_tok / lm_arc_lp / lm_arc_next
// [n_arcs] (sorted inside a row) and the counts lm_V, lm_order, lm_S, lm_n_arcs.
//
// Whatever the tables hold, a lookup reads inside them and ends: the state is clamped into [0, S) on entry and after
// every fail / next read, row bounds into [0, n_arcs], and the back-off loop runs at most lm_order times.  A corrupt
// table gives a wrong score, never a hang or an out-of-range read.
#pragma once

#include "common.hpp"

// the tables as every kernel carries them
struct NgramTables {
    const double* lm_uni_lp;
    const int32_t* lm_uni_next;
    const int32_t* lm_row_ptr;
    const int32_t* lm_fail;
    const double* lm_backoff;
    const int32_t* lm_arc_tok;
    const double* lm_arc_lp;
    const int32_t* lm_arc_next;
    int lm_V, lm_order, lm_S, lm_n_arcs, lm_start, lm_blank;
    double lm_weight, lm_bonus;
};

// host side (ngram.hip): the argument checks of every entry point that takes an n-gram (ED_OK, or ED_ERR_INVALID with
// the message set; `what` names the entry point), and the kernels' argument block of a checked struct
int ed_ngram_check(const edgedict_ngram_lm_t* lm, const char* what);
NgramTables ed_ngram_tables(const edgedict_ngram_lm_t* lm);

template <typename P>
__device__ __forceinline__ int ngram_state(const P& p, int s) { return min(max(s, 0), p.lm_S - 1); }

// the row of state s, clamped
template <typename P>
__device__ __forceinline__ void ngram_row(const P& p, int s, int& lo, int& hi) {
    lo = min(max(p.lm_row_ptr[s], 0), p.lm_n_arcs);
    hi = min(max(p.lm_row_ptr[s + 1], 0), p.lm_n_arcs);
}

// A token's fused LM term weight * l + bonus as the host forms it: the product is rounded, then the bonus is added.
// Without the pragma the compiler contracts the two into one fused multiply-add, which rounds once.
__device__ __forceinline__ double ngram_term(double weight, double l, double bonus) {
#pragma clang fp contract(off)
    const double prod = weight * l;
    return prod + bonus;
}

// step(s, k): log p(k | s) in the order of additions NGramLM.step states, the state after k into *next.  k = V is eos.
template <typename P>
__device__ __forceinline__ double ngram_step(const P& p, int s, int k, int* next) {
    s = ngram_state(p, s);
    k = min(max(k, 0), p.lm_V);
    double acc = 0.0;
    for (int it = 0; it < p.lm_order && s != 0; ++it) {
        int lo, hi;
        ngram_row(p, s, lo, hi);
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            const int t = p.lm_arc_tok[mid];
            if (t == k) {
                *next = ngram_state(p, p.lm_arc_next[mid]);
                return acc + p.lm_arc_lp[mid];
            }
            if (t < k) lo = mid + 1; else hi = mid;
        }
        acc = acc + p.lm_backoff[s];
        s = ngram_state(p, p.lm_fail[s]);
    }
    *next = ngram_state(p, p.lm_uni_next[k]);
    return acc + p.lm_uni_lp[k];
}
