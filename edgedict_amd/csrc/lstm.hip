// LSTM time recurrence (forward and BPTT) for gfx950.
//
// Replaces the cuDNN/MIOpen RNN behind nn.LSTM as the reference uses it:
//   encoder  rnnt/models.py:45-46,65   six 1-layer batch_first LSTMs, state (hs[i], cs[i])
//   decoder  rnnt/models.py:145-147,155 one multi-layer LSTM
// PyTorch cell semantics: gate order i,f,g,o in the 4H rows of weight_ih / weight_hh,
//   i,f,o = sigmoid, g = tanh,  c' = f*c + i*g,  h' = o*tanh(c').
//
// Division of labour: the input product X*W_ih^T + b_ih + b_hh for ALL timesteps
// is one big MFMA GEMM (gemm.hip) that leaves pre-activations in G[B,T,4H].  What remains is the
// strictly serial part, h_{t-1}*W_hh^T, handled here as ONE SMALL KERNEL PER TIMESTEP:
// a dependent kernel boundary costs ~1.5 us on MI355X, less than any software grid barrier
// (MI355X_MICROARCH.md price list: boundary 1.45 us vs barrier-xcd 4-5 us), and needs no
// co-residency assumptions.
//
// Forward step t, workgroup (unit block j0..j0+3, batch block of 64 rows), 4 waves:
//   each wave owns a quarter of K = H and multiplies Hprev[:, t, kslice] (64 x K/4) by the
//   16 W_hh rows {gate*H + j0 + u} with v_mfma 16x16 tiles, operands loaded straight from
//   L2 into VGPRs (no LDS staging: nothing is reused inside the workgroup);
//   the four partial 64x16 tiles are reduced through LDS, then one thread per (row, unit)
//   applies the cell update and writes, in place, the post-activation gates over G[:, t],
//   c_t, h_t -> Y[:, t] and h_t -> Hprev[:, t+1].
// Backward step t, workgroup (16 units, 16 batch rows): dh = dY[:, t] + dG[:, t+1] * W_hh
//   (K = 4H, one gate per wave, operand W_hh^T), then the cell backward, writing the
//   pre-activation gradients in place over G[:, t] and carrying dc in a [B,H] fp32 buffer.
// After the sweep G holds dG for every t, and dX / dW_ih / dW_hh / db are plain GEMMs / column sums.
#include <stdlib.h>

#include <mutex>

#include "common.hpp"
#include "lstm_fast.hpp"

namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_t;
typedef __attribute__((ext_vector_type(4))) float f32x4_t;

__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + expf(-x)); }

// ---- fragment loads straight from global memory (row-major, K contiguous) -------------
// bf16: lane holds 8 consecutive k (16 B) of row (lane & 15), k offset (lane >> 4) * 8
__device__ __forceinline__ bf16x8_t load_frag(const bf16_t* row_ptr, int k, int kmax, bool row_ok) {
    uint4 v = make_uint4(0, 0, 0, 0);
    if (row_ok && k + 8 <= kmax) v = *reinterpret_cast<const uint4*>(row_ptr + k);
    return *reinterpret_cast<bf16x8_t*>(&v);
}
__device__ __forceinline__ float load_frag(const float* row_ptr, int k, int kmax, bool row_ok) {
    return (row_ok && k < kmax) ? row_ptr[k] : 0.f;
}
__device__ __forceinline__ f32x4_t mma(bf16x8_t a, bf16x8_t b, f32x4_t c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ f32x4_t mma(float a, float b, f32x4_t c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}
template <typename T> struct MK;
template <> struct MK<bf16_t> { static constexpr int K = 32, LANE_K = 8; };
template <> struct MK<float> { static constexpr int K = 4, LANE_K = 1; };

constexpr int UNITS = 4;  // hidden units per forward workgroup (x 4 gates = one 16-wide N tile)

// fp32 operands, K slice [kbeg, kend) a multiple of 16 long, rows 16-byte aligned: ONE 16-byte load per lane and operand
// feeds FOUR 16x16x4 MFMA steps - lane (r, kq) holds k = 16 c + 4 kq + j (j = 0..3) of chunk c, and MFMA j of the chunk
// takes element j of every lane: the same permutation of k on both operands, i.e. the same dot product summed in
// another order.  CHK chunks of both operands are requested together.  (The scalar form below issues one dependent L2
// round trip per MFMA step: 64 per wave at H = 1024 - the fp32 step took 46 us, 3 us of them arithmetic; this is what
// made the exact mode's encoder 7 x slower than it has to be.)
template <int M>
__device__ __forceinline__ void f32_product16(f32x4_t (&acc)[M], const float* const (&ap)[M], const float* wp,
                                              int kbeg, int kend, int lane) {
    constexpr int CHK = M >= 4 ? 8 : 16;
    const int ko = (lane >> 4) * 4;
    for (int k = kbeg; k < kend; k += 16 * CHK) {
        float4 bq[CHK], aq[CHK][M];
#pragma unroll
        for (int c = 0; c < CHK; ++c) {
            const int kk = min(k + 16 * c, kend - 16) + ko;          // (clamped: a repeated chunk is skipped below)
            bq[c] = *reinterpret_cast<const float4*>(wp + kk);
#pragma unroll
            for (int m = 0; m < M; ++m) aq[c][m] = *reinterpret_cast<const float4*>(ap[m] + kk);
        }
#pragma unroll
        for (int c = 0; c < CHK; ++c) {
            if (k + 16 * c < kend) {
                const float bv[4] = {bq[c].x, bq[c].y, bq[c].z, bq[c].w};
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int m = 0; m < M; ++m) {
                        const float av[4] = {aq[c][m].x, aq[c][m].y, aq[c][m].z, aq[c][m].w};
                        acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j], bv[j], acc[m], 0, 0, 0);
                    }
            }
        }
    }
}

template <typename T>
__global__ __launch_bounds__(256) void lstm_step_fwd(
    T* __restrict__ G, T* __restrict__ Hprev, T* __restrict__ Y, float* __restrict__ Cst,
    const T* __restrict__ Whh, const float* __restrict__ c0, float* __restrict__ hN,
    float* __restrict__ cN, int B, int Tn, int H, int t) {
    __shared__ float red[4][64][17];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j0 = blockIdx.x * UNITS;
    const int b0 = blockIdx.y * 64;
    constexpr int MKK = MK<T>::K, LK = MK<T>::LANE_K;

    // K slice of this wave, rounded to whole MFMA steps
    const int steps_total = (H + MKK - 1) / MKK;
    const int steps_per_wave = (steps_total + 3) / 4;
    const int kbeg = wave * steps_per_wave * MKK;
    const int kend = min(H, kbeg + steps_per_wave * MKK);

    // B operand rows: n = gate*UNITS + unit  ->  W_hh row gate*H + j0 + unit
    const int n = lane & 15;
    const int wrow = (n / UNITS) * H + j0 + (n % UNITS);
    const bool w_ok = (j0 + (n % UNITS)) < H;
    const T* wptr = Whh + (long long)wrow * H;
    const int koff = (lane >> 4) * LK;

    f32x4_t acc[4];
    const T* aptr[4];
    bool a_ok[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        acc[m] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
        const int b = b0 + m * 16 + (lane & 15);
        a_ok[m] = b < B;
        aptr[m] = Hprev + ((long long)min(b, B - 1) * Tn + t) * H;
    }
    if constexpr (sizeof(T) == 4) {
        if ((H & 63) == 0) {       // wave slices of H / 4, a multiple of 16 (rows past B: clamped, never stored)
            const float* ap[4] = {(const float*)aptr[0], (const float*)aptr[1], (const float*)aptr[2], (const float*)aptr[3]};
            f32_product16<4>(acc, ap, (const float*)wptr, kbeg, kend, lane);
        } else {
            for (int k = kbeg; k < kend; k += MKK) {
                const auto bf = load_frag(wptr, k + koff, H, w_ok);
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    const auto af = load_frag(aptr[m], k + koff, H, a_ok[m]);
                    acc[m] = mma(af, bf, acc[m]);
                }
            }
        }
    } else
    for (int k = kbeg; k < kend; k += MKK) {
        const auto bf = load_frag(wptr, k + koff, H, w_ok);
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const auto af = load_frag(aptr[m], k + koff, H, a_ok[m]);
            acc[m] = mma(af, bf, acc[m]);
        }
    }
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r)
            red[wave][m * 16 + (lane >> 4) * 4 + r][lane & 15] = acc[m][r];
    __syncthreads();

    const int bl = threadIdx.x / UNITS, u = threadIdx.x % UNITS;
    const int b = b0 + bl, j = j0 + u;
    if (b >= B || j >= H) return;
    float pre[4];
    T* grow = G + ((long long)b * Tn + t) * 4 * H;
#pragma unroll
    for (int gate = 0; gate < 4; ++gate) {
        const int col = gate * UNITS + u;
        pre[gate] = red[0][bl][col] + red[1][bl][col] + red[2][bl][col] + red[3][bl][col] +
                    ElemIO<T>::load(grow + gate * H + j);
    }
    const float ig = sigmoidf_(pre[0]), fg = sigmoidf_(pre[1]), gg = tanhf(pre[2]),
                og = sigmoidf_(pre[3]);
    const float cprev = (t > 0) ? Cst[((long long)b * Tn + t - 1) * H + j] : (c0 ? c0[(long long)b * H + j] : 0.f);
    const float c = fg * cprev + ig * gg;
    const float h = og * tanhf(c);
    ElemIO<T>::store(grow + 0 * H + j, ig);
    ElemIO<T>::store(grow + 1 * H + j, fg);
    ElemIO<T>::store(grow + 2 * H + j, gg);
    ElemIO<T>::store(grow + 3 * H + j, og);
    Cst[((long long)b * Tn + t) * H + j] = c;
    ElemIO<T>::store(Y + ((long long)b * Tn + t) * H + j, h);
    if (t + 1 < Tn) {
        ElemIO<T>::store(Hprev + ((long long)b * Tn + t + 1) * H + j, h);
    } else {
        if (hN) hN[(long long)b * H + j] = h;
        if (cN) cN[(long long)b * H + j] = c;
    }
}

// =====================================================================================
// fp32, launch-persistent (round 6): ALL T steps of one layer in ONE launch.
//
// The exact-f32 mode is the token-exact mode (greedy / stream / beam tokens equal to the reference's), and its encoder
// is a chain of T launches of lstm_step_fwd<float> per layer: 20.6 us per layer-step at E6D2, of which ~3 us are the
// dependent launch boundary and ~6 us the re-fetch of the workgroup's 64 KB W_hh slice, in front of a gather of the
// 256 KB of fp32 h_{t-1} that every workgroup needs anyway.  Here a workgroup owns its (4 units x 4 gates, 64 rows)
// for the whole sequence - the structure of the bf16 stack's stack_fwd_lpw_kernel without the wavefront around it:
//   * its W_hh slice (16 rows x H fp32) stays in NCH float4 registers per lane (wave w: k quarter w);
//   * c_t of a thread's (row, unit) stays in a register;
//   * h_t goes to Hprev[:, t + 1] with write-through 4-byte stores; readers gather Hprev[:, t] with L2-coherent loads
//     and recognise what is not written yet by the fill pattern (all ones: a NaN no h = o * tanh(c) can be) - the
//     host fills Hprev before the launch; every dword is checked (the four units of a row's 16 bytes come from four
//     threads), a wave that came too early sleeps and gathers again (bounded: give-up word of the encoder stack);
//   * the arithmetic is lstm_step_fwd<float>'s, instruction for instruction: the same K quarters per wave, the same
//     chunk order inside f32_product16, the same order of the four partial sums, the same cell math - outputs, saved
//     gates and states are BIT-IDENTICAL to the per-step kernels (tests/test_lstm_gpu.py), so the token-exactness
//     pinned on the reference's goldens carries over.
// Needs every workgroup resident at once ((H / 4) x ceil(B / 64) <= CUs) and H in {256, 512, 1024}; else the per-step
// kernels run.  EDGEDICT_LSTM_F32_LPW=0 switches it off.
// =====================================================================================
typedef __attribute__((ext_vector_type(4))) unsigned u32x4_lstm_t;

// Tiling: a workgroup owns 16 ROWS x 16 UNITS (x 4 gates), not the step kernel's 64 rows x 4 units: what a workgroup must
// gather per step is the h of ITS rows - 16 x H fp32 = 64 KB instead of 256 KB, and the per-CU fetch rate is what bounds a
// step (first version, 64 x 4: 13 us per layer-step; this one: see DESIGN 4.33) - while its W_hh slice grows to 64 rows x H =
// 256 KB, i.e. 4 x NCH float4 registers per lane, which one wave per SIMD has (512).  Per output element nothing changes:
// the same K quarter per wave, the same chunk order, one v_mfma_f32_16x16x4_f32 chain per (row, gate column).
template <int NCH>        // 16-k chunks per wave quarter: H = 64 NCH
__global__ __launch_bounds__(256, 1) void lstm_fwd_lpw_f32(
    float* __restrict__ G, float* __restrict__ Hprev, float* __restrict__ Y, float* __restrict__ Cst,
    const float* __restrict__ Whh, const float* __restrict__ c0, float* __restrict__ hN, float* __restrict__ cN,
    int B, int Tn, unsigned* err) {
    constexpr int H = 64 * NCH;
    constexpr int CHK = NCH < 8 ? NCH : 8;          // chunks requested together (f32_product16: 8)
    constexpr int WU = 16;                          // units per workgroup
    __shared__ float red[4][16][4 * WU + 1];
    __shared__ unsigned bail_s;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j0 = blockIdx.x * WU;
    const int b0 = blockIdx.y * 16;
    const int kbeg = wave * (H / 4);
    const int n = lane & 15, ko = (lane >> 4) * 4;
    if (tid == 0) bail_s = 0u;

    // ---- stationary weights: gate g's row g*H + j0 + n, this wave's K quarter
    float4 wq[4][NCH];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const float* wptr = Whh + (long long)(g * H + j0 + n) * H + kbeg + ko;
#pragma unroll
        for (int c = 0; c < NCH; ++c) wq[g][c] = *reinterpret_cast<const float4*>(wptr + 16 * c);
    }
    // ---- this lane's row of h (fragment row n), as a byte offset into Hprev at frame 0
    // (readfirstlane returns a SIGNED int: through unsigned temporaries, or a low word with bit 31 set sign-extends
    // into the high word of the base)
    const unsigned long long hp = (unsigned long long)Hprev;
    const unsigned hp_lo = (unsigned)__builtin_amdgcn_readfirstlane((unsigned)hp);
    const unsigned hp_hi = (unsigned)__builtin_amdgcn_readfirstlane((unsigned)(hp >> 32));
    const __amdgpu_buffer_rsrc_t rh = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(((unsigned long long)hp_hi << 32) | (unsigned long long)hp_lo), 0,
        (int)((unsigned)B * (unsigned)Tn * (unsigned)H * 4u), 0x00020000);
    const unsigned aoff = (unsigned)(((long long)min(b0 + n, B - 1) * Tn * H + kbeg + ko) * 4);

    // ---- this thread's cell: row bl, unit u
    const int bl = tid / WU, u = tid % WU;
    const bool live = b0 + bl < B;
    // (rows past the batch compute on a clamped row and store nothing: every address a load could be speculated to
    // stays inside the tensors)
    const int b = min(b0 + bl, B - 1), j = j0 + u;
    float cprev = c0 ? c0[(long long)b * H + j] : 0.f;
    float pre_g[4];
    {
        const float* grow = G + ((long long)b * Tn) * 4 * H;
#pragma unroll
        for (int gate = 0; gate < 4; ++gate) pre_g[gate] = grow[gate * H + j];
    }
    __syncthreads();

    for (int t = 0; t < Tn; ++t) {
        f32x4_t acc[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) acc[g] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
        const unsigned toff = (unsigned)t * (unsigned)(H * 4);
        // CHK chunks are requested together, looked at (all ones = a peer has not written it yet: sleep, request again),
        // then multiplied - f32_product16's batches and chunk order
#pragma unroll
        for (int c0i = 0; c0i < NCH; c0i += CHK) {
            float4 aq[CHK];
            unsigned tries = 0;
            for (;;) {
                unsigned worst = 0u;
#pragma unroll
                for (int c = 0; c < CHK; ++c) {
                    const u32x4_lstm_t v = __builtin_amdgcn_raw_buffer_load_b128(rh, aoff + (unsigned)((c0i + c) * 64), toff, 16);
                    aq[c] = *reinterpret_cast<const float4*>(&v);
                    worst = max(worst, max(max(v[0], v[1]), max(v[2], v[3])));
                }
                if (t == 0 || !__any(worst == 0xffffffffu)) break;     // (frame 0 was written before the launch)
                __builtin_amdgcn_s_sleep(2);
                if (++tries > (1u << 20)) {                            // a peer never became resident
                    if (err) atomicCAS(err, 0u, 710u);
                    bail_s = 1u;
                    break;
                }
            }
#pragma unroll
            for (int c = 0; c < CHK; ++c) {
                const float av[4] = {aq[c].x, aq[c].y, aq[c].z, aq[c].w};
#pragma unroll
                for (int jj = 0; jj < 4; ++jj)
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const float4 wv = wq[g][c0i + c];
                        const float bv[4] = {wv.x, wv.y, wv.z, wv.w};
                        acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[jj], bv[jj], acc[g], 0, 0, 0);
                    }
            }
        }
        // partial tile of this wave: rows (lane >> 4) * 4 + r, gate g's column n
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
            for (int r = 0; r < 4; ++r) red[wave][(lane >> 4) * 4 + r][g * WU + n] = acc[g][r];
        __syncthreads();
        if (bail_s) break;
        {
            float pre[4];
#pragma unroll
            for (int gate = 0; gate < 4; ++gate) {
                const int col = gate * WU + u;
                pre[gate] = red[0][bl][col] + red[1][bl][col] + red[2][bl][col] + red[3][bl][col] + pre_g[gate];
            }
            const float ig = sigmoidf_(pre[0]), fg = sigmoidf_(pre[1]), gg = tanhf(pre[2]), og = sigmoidf_(pre[3]);
            // (the contraction lstm_step_fwd<float> compiles `fg * cprev + ig * gg` to - fg * cprev rounded, then one
            // fma - spelled out: left to the compiler this kernel got the other pairing, one ulp apart)
            const float fc = fg * cprev;
            const float c = __builtin_fmaf(ig, gg, fc);
            const float h = og * tanhf(c);
            cprev = c;
            const long long row = (long long)b * Tn + t;
            // publish first: h_t is what the peers wait for (16 consecutive units of a row: 64 bytes per row)
            if (live && t + 1 < Tn)
                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(h), rh, (unsigned)(((row + 1) * H + j) * 4), 0, 16);
            float* grow = G + row * 4 * H;
            if (live) {
                grow[0 * H + j] = ig;
                grow[1 * H + j] = fg;
                grow[2 * H + j] = gg;
                grow[3 * H + j] = og;
                Cst[row * H + j] = c;
                Y[row * H + j] = h;
            }
            if (t + 1 < Tn) {
#pragma unroll
                for (int gate = 0; gate < 4; ++gate) pre_g[gate] = grow[4 * H + gate * H + j];      // next frame's pre-activations
            } else if (live) {
                if (hN) hN[(long long)b * H + j] = h;
                if (cN) cN[(long long)b * H + j] = c;
            }
        }
        __syncthreads();          // red is rewritten by the next step
    }
}

// Hprev[:, 0, :] <- h0 (or zeros)
template <typename T>
__global__ void lstm_init_hprev(T* __restrict__ Hprev, const float* __restrict__ h0, int B, int Tn,
                                int H) {
    const long long n = (long long)B * H;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (long long)gridDim.x * blockDim.x) {
        const long long b = i / H, j = i % H;
        ElemIO<T>::store(Hprev + (b * Tn) * H + j, h0 ? h0[i] : 0.f);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void lstm_step_bwd(
    T* __restrict__ G, const T* __restrict__ dY, const float* __restrict__ Cst,
    const float* __restrict__ c0, const T* __restrict__ WhhT, float* __restrict__ dC, int B,
    int Tn, int H, int t) {
    __shared__ float red[4][16][17];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j0 = blockIdx.x * 16;
    const int b0 = blockIdx.y * 16;
    constexpr int MKK = MK<T>::K, LK = MK<T>::LANE_K;
    const int K = 4 * H;

    f32x4_t acc = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    if (t + 1 < Tn) {
        const int steps_total = (K + MKK - 1) / MKK;
        const int steps_per_wave = (steps_total + 3) / 4;
        const int kbeg = wave * steps_per_wave * MKK;
        const int kend = min(K, kbeg + steps_per_wave * MKK);
        const int rb = b0 + (lane & 15);
        const bool a_ok = rb < B;
        const T* aptr = G + ((long long)min(rb, B - 1) * Tn + t + 1) * K;
        const int jn = j0 + (lane & 15);
        const bool w_ok = jn < H;
        const T* wptr = WhhT + (long long)min(jn, H - 1) * K;
        const int koff = (lane >> 4) * LK;
        f32x4_t acc2 = (f32x4_t){0.f, 0.f, 0.f, 0.f};
        int k = kbeg;
        if constexpr (sizeof(T) == 4) {
            if ((H & 15) == 0) {   // wave slices of H
                f32x4_t a1[1] = {acc};
                const float* ap[1] = {(const float*)aptr};
                f32_product16<1>(a1, ap, (const float*)wptr, kbeg, kend, lane);
                acc = a1[0];
                k = kend;
            }
        }
        for (; k + MKK < kend; k += 2 * MKK) {  // two independent accumulation chains
            const auto a0 = load_frag(aptr, k + koff, K, a_ok);
            const auto w0 = load_frag(wptr, k + koff, K, w_ok);
            const auto a1 = load_frag(aptr, k + MKK + koff, K, a_ok);
            const auto w1 = load_frag(wptr, k + MKK + koff, K, w_ok);
            acc = mma(a0, w0, acc);
            acc2 = mma(a1, w1, acc2);
        }
        for (; k < kend; k += MKK) {
            const auto a0 = load_frag(aptr, k + koff, K, a_ok);
            const auto w0 = load_frag(wptr, k + koff, K, w_ok);
            acc = mma(a0, w0, acc);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[r] += acc2[r];
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) red[wave][(lane >> 4) * 4 + r][lane & 15] = acc[r];
    __syncthreads();

    const int bl = threadIdx.x >> 4, nl = threadIdx.x & 15;
    const int b = b0 + bl, j = j0 + nl;
    if (b >= B || j >= H) return;
    const long long row = (long long)b * Tn + t;
    float dh = red[0][bl][nl] + red[1][bl][nl] + red[2][bl][nl] + red[3][bl][nl];
    if (dY) dh += ElemIO<T>::load(dY + row * H + j);
    T* grow = G + row * 4 * H;
    const float ig = ElemIO<T>::load(grow + j), fg = ElemIO<T>::load(grow + H + j),
                gg = ElemIO<T>::load(grow + 2 * H + j), og = ElemIO<T>::load(grow + 3 * H + j);
    const float c = Cst[row * H + j];
    const float cprev = (t > 0) ? Cst[(row - 1) * H + j] : (c0 ? c0[(long long)b * H + j] : 0.f);
    const float tc = tanhf(c);
    const float dct = dC[(long long)b * H + j] + dh * og * (1.f - tc * tc);
    ElemIO<T>::store(grow + j, dct * gg * ig * (1.f - ig));
    ElemIO<T>::store(grow + H + j, dct * cprev * fg * (1.f - fg));
    ElemIO<T>::store(grow + 2 * H + j, dct * ig * (1.f - gg * gg));
    ElemIO<T>::store(grow + 3 * H + j, dh * tc * og * (1.f - og));
    dC[(long long)b * H + j] = dct * fg;
}

__global__ void fill_f32(float* p, long long n, float v) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (long long)gridDim.x * blockDim.x)
        p[i] = v;
}

// the launch-persistent fp32 forward covers this geometry (see lstm_fwd_lpw_f32)
bool f32_lpw_ok(int B, int Tn, int H) {
    const char* e = getenv("EDGEDICT_LSTM_F32_LPW");        // read per call: tests compare both paths in one process
    if (e && atoi(e) == 0) return false;
    if (!(H == 256 || H == 512 || H == 1024) || Tn < 2) return false;
    if ((unsigned long long)B * Tn * H * 4ull >= (1ull << 32)) return false;      // one 32-bit buffer descriptor
    const int n_cu = ed_device_cus();
    return (long long)(H / 16) * ((B + 15) / 16) <= n_cu;      // every workgroup (16 rows x 16 units) resident at once
}

extern "C" void* edgedict_stack_error_words(int host);      // encoder_stack.hip: the give-up words of the bounded waits

// Two launch-persistent kernels must never share the chip: each spins until ALL of its workgroups are resident, and two
// half-resident ones (the encoder's on the caller's stream, the prediction network's on the auxiliary stream: fp32 mode
// runs both through here) would wait for each other's CUs until the bounded spins give up.  Launches of this kernel on
// one device are therefore chained: a launch on another stream than the last one waits for that one's event.
struct LpwChain {
    std::mutex mu;
    hipEvent_t ev[16] = {};
    hipStream_t last[16] = {};
    bool valid[16] = {};
};
LpwChain g_lpw_chain;

int lpw_chain_before(hipStream_t s, int* dev_out) {
    int dev = 0;
    ED_CHECK_HIP(hipGetDevice(&dev));
    ED_CHECK_ARG(dev >= 0 && dev < 16, "lstm: device ordinal %d out of range", dev);
    *dev_out = dev;
    std::lock_guard<std::mutex> lock(g_lpw_chain.mu);
    if (!g_lpw_chain.ev[dev]) ED_CHECK_HIP(hipEventCreateWithFlags(&g_lpw_chain.ev[dev], hipEventDisableTiming));
    // (EDGEDICT_LSTM_LPW_NOCHAIN=1: test aid - tests/test_lstm_gpu.py shows the hazard is real)
    const char* e_nc = getenv("EDGEDICT_LSTM_LPW_NOCHAIN");
    if (g_lpw_chain.valid[dev] && g_lpw_chain.last[dev] != s && !(e_nc && atoi(e_nc)))
        ED_CHECK_HIP(hipStreamWaitEvent(s, g_lpw_chain.ev[dev], 0));
    return ED_OK;
}

int lpw_chain_after(hipStream_t s, int dev) {
    std::lock_guard<std::mutex> lock(g_lpw_chain.mu);
    ED_CHECK_HIP(hipEventRecord(g_lpw_chain.ev[dev], s));
    g_lpw_chain.last[dev] = s;
    g_lpw_chain.valid[dev] = true;
    return ED_OK;
}

template <typename T>
int run_fwd(void* G, void* Hprev, void* Y, float* Cst, const void* Whh, const float* h0,
            const float* c0, float* hN, float* cN, int B, int Tn, int H, hipStream_t s) {
    if constexpr (sizeof(T) == 4) {
        if (f32_lpw_ok(B, Tn, H)) {
            // frames 1 .. T-1 of Hprev: "not written yet" (all ones); frame 0: h0
            ED_CHECK_HIP(hipMemsetAsync(Hprev, 0xff, (size_t)B * Tn * H * sizeof(float), s));
            hipLaunchKernelGGL(lstm_init_hprev<float>, dim3(ed_grid_for((long long)B * H, 256)), dim3(256), 0, s,
                               (float*)Hprev, h0, B, Tn, H);
            ED_CHECK_LAUNCH("lstm_init_hprev");
            unsigned* err = reinterpret_cast<unsigned*>(edgedict_stack_error_words(0));
            if (err) err += 2;                 // the step kernels' word (encoder_stack.py reports code 7xx as a forward wait)
            int dev = 0;
            {
                const int rc = lpw_chain_before(s, &dev);
                if (rc != ED_OK) return rc;
            }
            const dim3 grid(H / 16, (B + 15) / 16);
            if (H == 1024)
                hipLaunchKernelGGL(lstm_fwd_lpw_f32<16>, grid, dim3(256), 0, s, (float*)G, (float*)Hprev, (float*)Y, Cst,
                                   (const float*)Whh, c0, hN, cN, B, Tn, err);
            else if (H == 512)
                hipLaunchKernelGGL(lstm_fwd_lpw_f32<8>, grid, dim3(256), 0, s, (float*)G, (float*)Hprev, (float*)Y, Cst,
                                   (const float*)Whh, c0, hN, cN, B, Tn, err);
            else
                hipLaunchKernelGGL(lstm_fwd_lpw_f32<4>, grid, dim3(256), 0, s, (float*)G, (float*)Hprev, (float*)Y, Cst,
                                   (const float*)Whh, c0, hN, cN, B, Tn, err);
            ED_CHECK_LAUNCH("lstm_fwd_lpw_f32");
            return lpw_chain_after(s, dev);
        }
    }
    hipLaunchKernelGGL(lstm_init_hprev<T>, dim3(ed_grid_for((long long)B * H, 256)), dim3(256), 0,
                       s, (T*)Hprev, h0, B, Tn, H);
    ED_CHECK_LAUNCH("lstm_init_hprev");
    dim3 grid((H + UNITS - 1) / UNITS, (B + 63) / 64);
    for (int t = 0; t < Tn; ++t) {
        hipLaunchKernelGGL(lstm_step_fwd<T>, grid, dim3(256), 0, s, (T*)G, (T*)Hprev, (T*)Y, Cst,
                           (const T*)Whh, c0, hN, cN, B, Tn, H, t);
    }
    ED_CHECK_LAUNCH("lstm_step_fwd");
    return ED_OK;
}

template <typename T>
int run_bwd(void* G, const void* dY, const float* Cst, const float* c0, const void* WhhT,
            float* dC, int B, int Tn, int H, hipStream_t s) {
    hipLaunchKernelGGL(fill_f32, dim3(ed_grid_for((long long)B * H, 256)), dim3(256), 0, s, dC,
                       (long long)B * H, 0.f);
    ED_CHECK_LAUNCH("lstm dC init");
    dim3 grid((H + 15) / 16, (B + 15) / 16);
    for (int t = Tn - 1; t >= 0; --t) {
        hipLaunchKernelGGL(lstm_step_bwd<T>, grid, dim3(256), 0, s, (T*)G, (const T*)dY, Cst, c0,
                           (const T*)WhhT, dC, B, Tn, H, t);
    }
    ED_CHECK_LAUNCH("lstm_step_bwd");
    return ED_OK;
}

}  // namespace

extern "C" size_t edgedict_lstm_workspace_bytes(int dtype, int B, int H) {
    if (B <= 0 || H <= 0 || !ed_lstm_fast_ok(dtype, H)) return 0;
    return ed_lstm_fast_ws_bytes(B, H);
}

extern "C" int edgedict_lstm_pack_weights(int src_dtype, const void* Whh, void* packed_fwd,
                                          void* packed_bwd, int H, void* stream) {
    ED_CHECK_ARG(src_dtype == ED_F32 || src_dtype == ED_BF16, "lstm_pack_weights: bad dtype");
    ED_CHECK_ARG(H > 0 && H % 32 == 0, "lstm_pack_weights: hidden size %d must be a multiple of 32", H);
    ED_CHECK_ARG(Whh && (packed_fwd || packed_bwd), "lstm_pack_weights: null pointer");
    return ed_lstm_pack(src_dtype, Whh, packed_fwd, packed_bwd, H, (hipStream_t)stream);
}

extern "C" int edgedict_lstm_forward(int dtype, void* G, void* Hprev, void* Y, float* Cst,
                                     const void* Whh, const void* Whh_packed, const float* h0,
                                     const float* c0, float* hN, float* cN, int B, int T, int H,
                                     void* ws, void* stream) {
    ED_CHECK_ARG(dtype == ED_F32 || dtype == ED_BF16, "lstm_forward: bad dtype %d", dtype);
    ED_CHECK_ARG(B > 0 && T > 0 && H > 0, "lstm_forward: B,T,H must be positive (got %d,%d,%d)", B, T, H);
    ED_CHECK_ARG(H % 8 == 0, "lstm_forward: hidden size %d must be a multiple of 8", H);
    ED_CHECK_ARG(G && Hprev && Y && Cst && (Whh || Whh_packed), "lstm_forward: null pointer");
    if (Whh_packed && ws && ed_lstm_fast_ok(dtype, H))
        return ed_lstm_fwd_fast(G, Hprev, Y, Cst, Whh_packed, h0, c0, hN, cN, B, T, H, ws,
                                (hipStream_t)stream);
    ED_CHECK_ARG(Whh, "lstm_forward: the generic path needs the plain W_hh");
    if (dtype == ED_F32)
        return run_fwd<float>(G, Hprev, Y, Cst, Whh, h0, c0, hN, cN, B, T, H, (hipStream_t)stream);
    return run_fwd<bf16_t>(G, Hprev, Y, Cst, Whh, h0, c0, hN, cN, B, T, H, (hipStream_t)stream);
}

extern "C" int edgedict_lstm_backward(int dtype, void* G, const void* dY, const float* Cst,
                                      const float* c0, const void* WhhT, const void* WhhT_packed,
                                      float* dC_ws, int B, int T, int H, void* ws, void* stream) {
    ED_CHECK_ARG(dtype == ED_F32 || dtype == ED_BF16, "lstm_backward: bad dtype %d", dtype);
    ED_CHECK_ARG(B > 0 && T > 0 && H > 0, "lstm_backward: B,T,H must be positive");
    ED_CHECK_ARG(H % 8 == 0, "lstm_backward: hidden size %d must be a multiple of 8", H);
    ED_CHECK_ARG(G && Cst && (WhhT || WhhT_packed) && dC_ws, "lstm_backward: null pointer");
    if (WhhT_packed && ws && ed_lstm_fast_ok(dtype, H))
        return ed_lstm_bwd_fast(G, dY, Cst, c0, WhhT_packed, dC_ws, B, T, H, ws,
                                (hipStream_t)stream);
    ED_CHECK_ARG(WhhT, "lstm_backward: the generic path needs the plain W_hh^T");
    if (dtype == ED_F32)
        return run_bwd<float>(G, dY, Cst, c0, WhhT, dC_ws, B, T, H, (hipStream_t)stream);
    return run_bwd<bf16_t>(G, dY, Cst, c0, WhhT, dC_ws, B, T, H, (hipStream_t)stream);
}
