// Confidence of N-best hypotheses (gfx950): the two kernels of the post-pass decode.hypothesis_confidence /
// decode.ctc_hypothesis_confidence.  The pass re-evaluates the joint at each token's (frame, prefix) - or reads the CTC
// head's logits on the token's frame - and reduces every row of logits to five statistics of the acoustic model's
// output distribution; the measures (normalised Shannon entropy, Tsallis entropy, ...) are formed from them on the host.
//
//   conf_hidden_rows   hid[r, :] = tanh(E1[enc_row[r], :] + D1[dec_row[r], :] (+ b1)), stored in the compute dtype: the
//                      composed search step's add_tanh_rows (decode.hip) with both operands gathered.  The rounding
//                      points are that kernel's: the operands as they are stored, one rounding of hid.
//   conf_row_stats     one wave per row of logits z [V] (fp32 or bf16), 4 waves per workgroup:
//                        m = max z;  s = sum e^(z - m);  a = sum e^(z - m) (z - m);  q = sum e^(alpha (z - m))
//                      stats[r] = { (z[k] - m) - log s,  -log s,  (z[blank] - m) - log s,  log s - a / s,
//                                   log q - alpha log s };  top[r] = arg max z (lowest index on ties).
// The dense products between them go through edgedict_gemm.  No atomics: the same bits on every run.
#include "decode_net.hpp"

namespace {

// One thread per access of N elements (VEC: 16 bytes; else one element).  A row whose enc_row / dec_row lies outside
// [0, n_enc_rows) / [0, n_dec_rows) is written as NaN and nothing is read for it.
template <typename ET, bool VEC>
__global__ __launch_bounds__(256) void conf_hidden_rows(const ET* __restrict__ E1, int n_enc_rows,
                                                        const ET* __restrict__ D1, int n_dec_rows,
                                                        const float* __restrict__ b1, const int32_t* __restrict__ enc_row,
                                                        const int32_t* __restrict__ dec_row, ET* __restrict__ hid, int R,
                                                        int J) {
    constexpr int N = VEC ? ElemIO<ET>::VEC : 1;
    const int per_row = J / N;                                      // VEC: J % N == 0 (the host checked)
    const long long n = (long long)R * per_row;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int r = (int)(i / per_row), j = (int)(i % per_row) * N;
        const int er = enc_row[r], dr = dec_row[r];
        const bool ok = er >= 0 && er < n_enc_rows && dr >= 0 && dr < n_dec_rows;
        ET* out = hid + (long long)r * J + j;
        float h[N];
        if (ok) {
            float e[N], d[N];
            if constexpr (VEC) {
                ElemIO<ET>::load_vec(E1 + (long long)er * J + j, e);
                ElemIO<ET>::load_vec(D1 + (long long)dr * J + j, d);
            } else {
                e[0] = ElemIO<ET>::load(E1 + (long long)er * J + j);
                d[0] = ElemIO<ET>::load(D1 + (long long)dr * J + j);
            }
#pragma unroll
            for (int k = 0; k < N; ++k) {
                float x = e[k] + d[k];
                if (b1) x += b1[j + k];
                h[k] = tanhf(x);
            }
        } else {
#pragma unroll
            for (int k = 0; k < N; ++k) h[k] = NAN;
        }
        if constexpr (VEC) ElemIO<ET>::store_vec(out, h);
        else ElemIO<ET>::store(out, h[0]);                          // (the conversion keeps a NaN a NaN)
    }
}

// A lane keeps up to CONF_REGS logits of its row: rows of V <= 64 * CONF_REGS are read once, longer ones once per pass.
constexpr int CONF_REGS = 32;
constexpr int CONF_REG_V = 64 * CONF_REGS;

// VEC: 16-byte loads (the row's base and pitch are 16-byte aligned); the access that straddles V reads its live elements
// one by one, so nothing behind V is ever read.  REG: V <= CONF_REG_V, the row in registers.
template <typename LT, bool VEC, bool REG>
__global__ __launch_bounds__(256) void conf_row_stats(const LT* __restrict__ logits, long long ld, int n_logit_rows,
                                                      const int32_t* __restrict__ rows,
                                                      const int32_t* __restrict__ tokens, int R, int V, int blank,
                                                      float alpha, float* __restrict__ stats, int32_t* __restrict__ top) {
    constexpr int N = VEC ? ElemIO<LT>::VEC : 1;
    constexpr int CH = CONF_REGS / N;                               // accesses a lane holds in REG form
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= R) return;
    float* out = stats + (long long)r * 5;
    const long long row = rows ? (long long)rows[r] : (long long)r;
    if (row < 0 || row >= n_logit_rows) {                           // nothing is read for such a row
        if (lane < 5) out[lane] = NAN;
        if (lane == 0) top[r] = -1;
        return;
    }
    const LT* z = logits + row * ld;
    const int nacc = (V + N - 1) / N;

    auto fetch = [&](int c, float (&o)[N]) {                        // c < nacc; elements behind V come as -inf
        if constexpr (VEC) {
            if (c * N + N <= V) {
                ElemIO<LT>::load_vec(z + (long long)c * N, o);
                return;
            }
        }
#pragma unroll
        for (int k = 0; k < N; ++k) o[k] = c * N + k < V ? ElemIO<LT>::load(z + c * N + k) : -INFINITY;
    };
    float reg[REG ? CONF_REGS : 1];
    if constexpr (REG) {
#pragma unroll
        for (int i = 0; i < CH; ++i) {
            const int c = lane + 64 * i;
            float o[N];
#pragma unroll
            for (int k = 0; k < N; ++k) o[k] = -INFINITY;
            if (c < nacc) fetch(c, o);
#pragma unroll
            for (int k = 0; k < N; ++k) reg[i * N + k] = o[k];
        }
    }
    // f(v, x) for every element this lane owns, v ascending; elements behind V come as -inf
    auto pass = [&](auto&& f) {
        if constexpr (REG) {
#pragma unroll
            for (int i = 0; i < CH; ++i) {
                const int c = lane + 64 * i;
#pragma unroll
                for (int k = 0; k < N; ++k) f(c * N + k, reg[i * N + k]);
            }
        } else {
            for (int c = lane; c < nacc; c += 64) {
                float o[N];
                fetch(c, o);
#pragma unroll
                for (int k = 0; k < N; ++k) f(c * N + k, o[k]);
            }
        }
    };

    float best = -INFINITY;
    int arg = 0x7fffffff;
    bool bad = false;
    pass([&](int v, float x) {
        bad |= x != x;
        if (x > best) { best = x; arg = v; }                        // strict >: the first index within a lane
    });
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float ob = __shfl_xor(best, off, 64);
        const int oa = __shfl_xor(arg, off, 64);
        if (ob > best || (ob == best && oa < arg)) { best = ob; arg = oa; }
    }
    // a NaN anywhere in the row, or no finite-or-+inf logit at all: NaN statistics, no arg max
    if (__any(bad) || best == -INFINITY) {
        if (lane < 5) out[lane] = NAN;
        if (lane == 0) top[r] = -1;
        return;
    }
    const float m = best;
    float s = 0.f, a = 0.f, q = 0.f;
    pass([&](int v, float x) {
        if (x > -INFINITY) {                                        // a -inf logit adds exactly 0: no 0 * inf is formed
            const float t = x - m;
            const float e = expf(t);
            s += e;
            a += e * t;
            q += expf(alpha * t);
        }
    });
    s = wave_sum(s);
    a = wave_sum(a);
    q = wave_sum(q);
    if (lane != 0) return;
    const float ls = logf(s);
    const int k = tokens[r];
    out[0] = (k < 0 || k >= V) ? NAN : (ElemIO<LT>::load(z + k) - m) - ls;
    out[1] = -ls;
    out[2] = (ElemIO<LT>::load(z + blank) - m) - ls;
    out[3] = ls - a / s;
    out[4] = logf(q) - alpha * ls;
    top[r] = arg;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int edgedict_conf_hidden_rows(int dtype, const void* E1, int n_enc_rows, const void* D1, int n_dec_rows,
                                         const float* b1, const int32_t* enc_row, const int32_t* dec_row, int R, int J,
                                         void* hid, void* stream_) {
    ED_CHECK_ARG(dtype == ED_F32 || dtype == ED_BF16, "conf_hidden_rows: bad dtype");
    ED_CHECK_ARG(R > 0 && J > 0 && n_enc_rows >= 0 && n_dec_rows >= 0, "conf_hidden_rows: bad shape (R=%d J=%d)", R, J);
    ED_CHECK_ARG(enc_row && dec_row && hid && (E1 || n_enc_rows == 0) && (D1 || n_dec_rows == 0),
                 "conf_hidden_rows: null pointer");
    hipStream_t s = (hipStream_t)stream_;
    dispatch(dtype, [&](auto tag) {
        using T = decltype(tag);
        constexpr int N = ElemIO<T>::VEC;
        const bool vec = J % N == 0 && aligned16(E1) && aligned16(D1) && aligned16(hid);
        const long long work = (long long)R * (vec ? J / N : J);
        const dim3 grid(ed_grid_for(work, 256));
        if (vec)
            hipLaunchKernelGGL((conf_hidden_rows<T, true>), grid, dim3(256), 0, s, (const T*)E1, n_enc_rows, (const T*)D1,
                               n_dec_rows, b1, enc_row, dec_row, (T*)hid, R, J);
        else
            hipLaunchKernelGGL((conf_hidden_rows<T, false>), grid, dim3(256), 0, s, (const T*)E1, n_enc_rows,
                               (const T*)D1, n_dec_rows, b1, enc_row, dec_row, (T*)hid, R, J);
    });
    ED_CHECK_LAUNCH("conf_hidden_rows");
    return ED_OK;
}

extern "C" int edgedict_conf_row_stats(const void* logits, int dtype, long long ld, int n_logit_rows, const int32_t* rows,
                                       const int32_t* tokens, int R, int V, int blank, float alpha, float* stats,
                                       int32_t* top, void* stream_) {
    ED_CHECK_ARG(dtype == ED_F32 || dtype == ED_BF16, "conf_row_stats: bad dtype");
    ED_CHECK_ARG(V >= 2, "conf_row_stats: V = %d, need at least two symbols", V);
    ED_CHECK_ARG(R > 0 && R <= 0x7fffffff - 3 && ld >= V && n_logit_rows >= 0 && (rows || R <= n_logit_rows),
                 "conf_row_stats: bad shape (R=%d V=%d ld=%lld rows of logits=%d)", R, V, ld, n_logit_rows);
    ED_CHECK_ARG(blank >= 0 && blank < V, "conf_row_stats: blank %d outside [0,%d)", blank, V);
    ED_CHECK_ARG(alpha > 0.f && alpha < 1.f, "conf_row_stats: alpha must lie inside (0, 1)");
    ED_CHECK_ARG(tokens && stats && top && (logits || n_logit_rows == 0), "conf_row_stats: null pointer");
    hipStream_t s = (hipStream_t)stream_;
    const dim3 grid((unsigned)((R + 3) / 4));
    dispatch(dtype, [&](auto tag) {
        using T = decltype(tag);
        const bool vec = aligned16(logits) && (ld * (long long)sizeof(T)) % 16 == 0;
        const bool reg = V <= CONF_REG_V;
        auto launch = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, grid, dim3(256), 0, s, (const T*)logits, ld, n_logit_rows, rows, tokens, R, V,
                               blank, alpha, stats, top);
        };
        if (vec && reg) launch(conf_row_stats<T, true, true>);
        else if (vec) launch(conf_row_stats<T, true, false>);
        else if (reg) launch(conf_row_stats<T, false, true>);
        else launch(conf_row_stats<T, false, false>);
    });
    ED_CHECK_LAUNCH("conf_row_stats");
    return ED_OK;
}
