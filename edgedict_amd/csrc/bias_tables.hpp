// The phrase automaton's device lookup (edgedict_beam_bias_t, include/edgedict_hip.h), shared by every search that
// carries a bias list: decode.hip's RNN-T beam searches and ctc_decode.hip's CTC prefix search.  P is the kernel's
// argument block; it names the tables bias_root_next [V], bias_row_ptr [S + 1], bias_exc_tok / bias_exc_next [n_exc]
// (sorted inside a row) and the state count bias_S.
#pragma once

#include "common.hpp"

// a state as the tables may be indexed with it (a stale or foreign state must not read out of range)
template <typename P>
__device__ __forceinline__ int bias_state(const P& p, int s) { return min(max(s, 0), p.bias_S - 1); }

// goto(s, k) of the phrase automaton: the exception row of s (binary search), else the root's transition
template <typename P>
__device__ __forceinline__ int bias_goto(const P& p, int s, int k) {
    s = bias_state(p, s);
    int lo = p.bias_row_ptr[s], hi = p.bias_row_ptr[s + 1];
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const int t = p.bias_exc_tok[mid];
        if (t == k) return bias_state(p, p.bias_exc_next[mid]);
        if (t < k) lo = mid + 1; else hi = mid;
    }
    return bias_state(p, p.bias_root_next[k]);
}
