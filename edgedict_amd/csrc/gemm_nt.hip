// bf16 "NT" GEMM fast path:  C[M,N] (+)= A[M,K] * B[N,K]^T + bias1[N] + bias2[N]
// (both operands K-contiguous, bf16 output).  Serves the large forward products of the path --
// joint logits hid x W2^T (rnnt/models.py:165-167,177), the encoder input products X x W_ih^T
// (rnnt/models.py:45-46,65) -- and, with a pre-transposed weight copy, their dX products.
//
// Differences from the general kernel in gemm.hip (register staging, two barriers per K step):
//   * operand tiles go HBM -> LDS directly (global_load_lds_dwordx4, 1 KiB per wave instruction),
//     double-buffered: the DMA of K-tile t+1 is in flight under the MFMAs of tile t; ONE barrier
//     per K step; no staging registers, no ds_write pass;
//   * the LDS image is lane-linear (a DMA cannot scatter), so the bank swizzle is applied on the
//     SOURCE side: lane l of an 8-row x 128-byte piece fetches 16-byte chunk (l%8) ^ (l/8) of its
//     row, which leaves every row a full 128-byte line in HBM and makes the ds_read_b128 fragment
//     reads (16 rows x one chunk) conflict-free.
// Tile 128x128x64, 4 waves (2x2), wave tile 64x64 = 4x4 MFMA 16x16x32 tiles, 64 KB LDS
// (2 workgroups per CU: one's epilogue stores overlap the other's main loop).
// Requirements (else gemm.hip's kernel runs): K % 64 == 0, lda/ldb % 8 == 0, 16-byte aligned
// operands, bf16 output with ldc % 8 == 0 and N % 8 == 0, split_k == 1.
#include "common.hpp"
#include "gemm_plan.hpp"

namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_t;
typedef __attribute__((ext_vector_type(4))) float f32x4_t;

constexpr int BK = 64;

struct NtArgs {
    const bf16_t* A;
    const bf16_t* B;
    bf16_t* C;
    const float* bias1;
    const float* bias2;
    long long lda, ldb, ldc;
    int M, N, K;
    int accumulate;
    int n_tiles, tiles;
    int debug;   // probe only: 1 = skip the C stores, 2 = skip the K loop
};

__device__ __forceinline__ void glds16(const bf16_t* src, unsigned char* lds_wave_base) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                     (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 0);
}

// (A 3-buffer variant with counted `s_waitcnt vmcnt(8)` + raw s_barrier, 96 KB LDS and ONE workgroup
// per CU was measured and is slower on every shape of this path: joint logits 4.6 vs 3.6 ms,
// 4096^3 657 vs 901 TF/s.  Two co-resident workgroups hide latency better than a deeper pipeline.)
// Instantiations <TM, TN, WT> (output tile TM x TN, wave tile WT x WT, (TM/WT) x (TN/WT) waves):
//   <128,128,64>  4 waves, 64 KB LDS, 2 workgroups per CU: the default for grids that fill the chip.
//   (<256,128,64>, 8 waves, 96 KB LDS, ONE workgroup per CU, was measured: 25 % fewer operand bytes
//    per flop and half the per-tile overheads do not make up for the lost second workgroup -
//    joint logits 4.19 vs 3.54 ms, dhid 2.63 vs 2.35 ms.  Instantiate it with
//    EDGEDICT_GEMM_NT_TILE=256 to re-measure.)
//   <64,64,32>    4 waves, 32 KB: SMALL problems (the encoder's chunked dX products,
//                 1024x1024x4096: 64 big tiles would use a quarter of the chip's fetch bandwidth;
//                 4x the workgroups fetch 2x the bytes at 4x the rate).
template <int TM, int TN, int WT>
__global__ __launch_bounds__((TM / WT) * (TN / WT) * 64, (TM / WT) * (TN / WT) == 4 ? 2 : 1)
void gemm_nt_kernel(NtArgs g) {
    constexpr int WAVES_N = TN / WT;
    constexpr int WAVES = (TM / WT) * WAVES_N, THREADS = WAVES * 64;
    constexpr int BM = TM, BN = TN;
    constexpr int MI = WT / 16, NJ = WT / 16;       // 16x16 MFMA tiles per wave along M / N
    constexpr int PIECES_A = TM / 8 / WAVES;        // 1 KiB DMA pieces per wave and K tile
    constexpr int PIECES_B = TN / 8 / WAVES;
    constexpr int A_BYTES = TM * BK * 2, B_BYTES = TN * BK * 2;
    constexpr int BUF_BYTES = A_BYTES + B_BYTES;
    constexpr int CCH = TN / 8;                     // 16-byte chunks per staged C row
    static_assert(TM * TN * 2 <= 2 * BUF_BYTES, "C staging must fit in the operand buffers");
    __shared__ __attribute__((aligned(1024))) unsigned char smem[2 * BUF_BYTES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = wave / WAVES_N, wn = wave % WAVES_N;   // wave rows wm * WT, wave cols wn * WT
    const int r16 = lane & 15, kq = lane >> 4;
    const int KT = g.K / BK;

    // XCD-aware tile order: consecutive workgroups of ONE XCD (blockIdx % 8) walk adjacent tiles,
    // so the A row panel they share stays in that XCD's L2.  One tile per workgroup: a persistent
    // variant (512 workgroups walking contiguous tile ranges, DMA pipeline kept full across tiles)
    // was measured SLOWER (joint dhid 3.25 vs 2.45 ms): co-resident persistent workgroups run in
    // phase, so their epilogues coincide instead of hiding under each other's main loops.
    int tile = blockIdx.x;
    {
        const int nx = 8, q = g.tiles / nx, r = g.tiles % nx, x = tile % nx, i = tile / nx;
        tile = (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + i;
    }
    const int m0 = (tile / g.n_tiles) * BM, n0 = (tile % g.n_tiles) * BN;

    // this lane's DMA sources: piece p = i*4 + wave covers tile rows p*8 .. p*8+7; lane l fetches
    // 16-byte chunk (l%8) ^ (l/8) of its row (source-side swizzle, LDS image stays lane-linear)
    const int prow = lane >> 3;
    const int chunk = (lane & 7) ^ prow;
    const bf16_t* asrc[PIECES_A];
    const bf16_t* bsrc[PIECES_B];
#pragma unroll
    for (int i = 0; i < PIECES_A; ++i)
        asrc[i] = g.A + (long long)min(m0 + (i * WAVES + wave) * 8 + prow, g.M - 1) * g.lda + chunk * 8;
#pragma unroll
    for (int i = 0; i < PIECES_B; ++i)
        bsrc[i] = g.B + (long long)min(n0 + (i * WAVES + wave) * 8 + prow, g.N - 1) * g.ldb + chunk * 8;
    auto issue = [&](int buf, int k0) {
        unsigned char* base = smem + buf * BUF_BYTES;
#pragma unroll
        for (int i = 0; i < PIECES_A; ++i) glds16(asrc[i] + k0, base + (i * WAVES + wave) * 1024);
#pragma unroll
        for (int i = 0; i < PIECES_B; ++i) glds16(bsrc[i] + k0, base + A_BYTES + (i * WAVES + wave) * 1024);
    };

    f32x4_t acc[MI][NJ];
    // operands swapped (B fragment first): lane holds D[n = (lane>>4)*4 + q][m = lane & 15], i.e.
    // FOUR CONSECUTIVE COLUMNS of one C row -> 8-byte packed stores in the epilogue
    auto compute = [&](int buf) {
        const unsigned char* sA = smem + buf * BUF_BYTES;
        const unsigned char* sB = sA + A_BYTES;
#pragma unroll
        for (int ks = 0; ks < BK / 32; ++ks) {
            bf16x8_t a[MI], b[NJ];
#pragma unroll
            for (int i = 0; i < MI; ++i) {
                const int ra = wm * WT + i * 16 + r16;
                a[i] = *reinterpret_cast<const bf16x8_t*>(sA + ra * 128 + (((ks * 4 + kq) ^ (ra & 7)) << 4));
            }
#pragma unroll
            for (int i = 0; i < NJ; ++i) {
                const int rb = wn * WT + i * 16 + r16;
                b[i] = *reinterpret_cast<const bf16x8_t*>(sB + rb * 128 + (((ks * 4 + kq) ^ (rb & 7)) << 4));
            }
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int j = 0; j < NJ; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b[j], a[i], acc[i][j], 0, 0, 0);
        }
    };

    issue(0, 0);
    {
        // biases enter through the accumulators.  They are ordinary loads, and hipcc waits vmcnt(0)
        // at the first use of an ordinary load while a DMA is in flight: issue them here and use
        // them right after the first __syncthreads() of the K loop, which waits vmcnt(0) anyway.
        float4 bv[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int nc = n0 + wn * WT + j * 16 + kq * 4;   // 4 consecutive columns of this lane
            bv[j] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (nc < g.N) {   // N % 8 == 0: the 4 columns are all inside or all outside
                if (g.bias1) bv[j] = *reinterpret_cast<const float4*>(g.bias1 + nc);
                if (g.bias2) {
                    const float4 v = *reinterpret_cast<const float4*>(g.bias2 + nc);
                    bv[j].x += v.x; bv[j].y += v.y; bv[j].z += v.z; bv[j].w += v.w;
                }
            }
        }
        for (int kt = 0; kt < ((g.debug & 2) ? 1 : KT); ++kt) {
            __syncthreads();   // vmcnt(0) + barrier: this K tile landed everywhere, the other buffer is free
            if (kt == 0) {
#pragma unroll
                for (int i = 0; i < MI; ++i)
#pragma unroll
                    for (int j = 0; j < NJ; ++j) acc[i][j] = (f32x4_t){bv[j].x, bv[j].y, bv[j].z, bv[j].w};
            }
            if (kt + 1 < KT) issue((kt + 1) & 1, (kt + 1) * BK);
            compute(kt & 1);
        }
        // ---- epilogue: the operand tiles are dead after this barrier; C is staged in LDS
        __syncthreads();
        unsigned char* sC = smem;   // [TM rows][CCH chunks of 16 B], chunk ^= row & (CCH - 1)
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int nl = wn * WT + j * 16 + kq * 4;        // 4 consecutive columns nl .. nl+3
#pragma unroll
            for (int i = 0; i < MI; ++i) {
                const int ml = wm * WT + i * 16 + r16;
                uint2 pk;
                pk.x = f32x2_to_bf16x2(acc[i][j][0], acc[i][j][1]);
                pk.y = f32x2_to_bf16x2(acc[i][j][2], acc[i][j][3]);
                *reinterpret_cast<uint2*>(sC + ml * (TN * 2) + ((((nl >> 3) ^ (ml & (CCH - 1))) << 4) | ((nl & 4) << 1))) = pk;
            }
        }
        __syncthreads();
#pragma unroll
        for (int it = 0; it < BM * BN / 8 / THREADS; ++it) {
            const int c = threadIdx.x + it * THREADS;
            const int rl = c / CCH, ch = c % CCH;
            const int row = m0 + rl, col = n0 + ch * 8;
            if (row >= g.M || col >= g.N || ((g.debug & 1) && row > 0)) continue;
            uint4 v = *reinterpret_cast<const uint4*>(sC + rl * (TN * 2) + ((ch ^ (rl & (CCH - 1))) << 4));
            bf16_t* dst = g.C + (long long)row * g.ldc + col;
            if (g.accumulate) {
                float x[8], y[8];
                ElemIO<bf16_t>::load_vec(dst, x);
                ElemIO<bf16_t>::load_vec(reinterpret_cast<const bf16_t*>(&v), y);
#pragma unroll
                for (int e = 0; e < 8; ++e) x[e] += y[e];
                ElemIO<bf16_t>::store_vec(dst, x);
            } else {
                *reinterpret_cast<uint4*>(dst) = v;
            }
        }
    }
}

// Small-M, long-K products - the encoder stack's per-chunk dX = dG x W_ih ([768..1536 x 1024 x 4096],
// accumulated in place on the side stream under the BPTT): 64 x 64 tiles so that every CU has one, and then
// the whole product is 64 K steps of 16 KB per workgroup - a latency chain.  The double-buffered kernel above
// drains its DMA queue at every step (0.5 us per step, 32 us per product); this one keeps a ring of three
// K stages with COUNTED waits (one stage always in flight across the barrier).  Three, not four: with four
// (64 KB) two of these workgroups fill a CU's LDS and the BPTT's own workgroups (37 KB) queue behind them -
// 23.7 us per product alone, but the training step got 0.8 ms SLOWER than with the drained kernel.
__global__ __launch_bounds__(256, 2) void gemm_nt_ring64_kernel(NtArgs g) {
    constexpr int TM = 64, TN = 64, WT = 32, WAVES = 4, THREADS = 256, NS = 3;   // 48 KB: see below
    constexpr int MI = 2, NJ = 2, PIECES = 2;
    constexpr int A_BYTES = TM * BK * 2, BUF_BYTES = 2 * A_BYTES;      // 16 KB per stage
    constexpr int CCH = TN / 8;
    __shared__ __attribute__((aligned(1024))) unsigned char smem[NS * BUF_BYTES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int r16 = lane & 15, kq = lane >> 4;
    const int KT = g.K / BK;
    int tile = blockIdx.x;
    {
        const int nx = 8, q = g.tiles / nx, r = g.tiles % nx, x = tile % nx, i = tile / nx;
        tile = (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + i;
    }
    const int m0 = (tile / g.n_tiles) * TM, n0 = (tile % g.n_tiles) * TN;
    const int prow = lane >> 3;
    const int chunk = (lane & 7) ^ prow;
    const bf16_t* asrc[PIECES];
    const bf16_t* bsrc[PIECES];
#pragma unroll
    for (int i = 0; i < PIECES; ++i) {
        asrc[i] = g.A + (long long)min(m0 + (i * WAVES + wave) * 8 + prow, g.M - 1) * g.lda + chunk * 8;
        bsrc[i] = g.B + (long long)min(n0 + (i * WAVES + wave) * 8 + prow, g.N - 1) * g.ldb + chunk * 8;
    }
    auto issue = [&](int q) {
        unsigned char* base = smem + (q % NS) * BUF_BYTES;
#pragma unroll
        for (int i = 0; i < PIECES; ++i) glds16(asrc[i] + q * BK, base + (i * WAVES + wave) * 1024);
#pragma unroll
        for (int i = 0; i < PIECES; ++i) glds16(bsrc[i] + q * BK, base + A_BYTES + (i * WAVES + wave) * 1024);
    };
    f32x4_t acc[MI][NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int nc = n0 + wn * WT + j * 16 + kq * 4;
        float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
        if (nc < g.N) {
            if (g.bias1) bv = *reinterpret_cast<const float4*>(g.bias1 + nc);
            if (g.bias2) {
                const float4 v = *reinterpret_cast<const float4*>(g.bias2 + nc);
                bv.x += v.x; bv.y += v.y; bv.z += v.z; bv.w += v.w;
            }
        }
#pragma unroll
        for (int i = 0; i < MI; ++i) acc[i][j] = (f32x4_t){bv.x, bv.y, bv.z, bv.w};
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // ordinary loads done before the DMA counting starts
    issue(0);
    issue(1);
    for (int q = 0; q < KT; ++q) {
        if (q + 1 < KT) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        asm volatile("s_barrier" ::: "memory");          // stage q landed everywhere; stage q - 1 is read out
        if (q + 2 < KT) issue(q + 2);
        const unsigned char* sA = smem + (q % NS) * BUF_BYTES;
        const unsigned char* sB = sA + A_BYTES;
#pragma unroll
        for (int ks = 0; ks < BK / 32; ++ks) {
            bf16x8_t a[MI], b[NJ];
#pragma unroll
            for (int i = 0; i < MI; ++i) {
                const int ra = wm * WT + i * 16 + r16;
                a[i] = *reinterpret_cast<const bf16x8_t*>(sA + ra * 128 + (((ks * 4 + kq) ^ (ra & 7)) << 4));
            }
#pragma unroll
            for (int i = 0; i < NJ; ++i) {
                const int rb = wn * WT + i * 16 + r16;
                b[i] = *reinterpret_cast<const bf16x8_t*>(sB + rb * 128 + (((ks * 4 + kq) ^ (rb & 7)) << 4));
            }
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int j = 0; j < NJ; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b[j], a[i], acc[i][j], 0, 0, 0);
        }
    }
    __syncthreads();
    unsigned char* sC = smem;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int nl = wn * WT + j * 16 + kq * 4;
#pragma unroll
        for (int i = 0; i < MI; ++i) {
            const int ml = wm * WT + i * 16 + r16;
            uint2 pk;
            pk.x = f32x2_to_bf16x2(acc[i][j][0], acc[i][j][1]);
            pk.y = f32x2_to_bf16x2(acc[i][j][2], acc[i][j][3]);
            *reinterpret_cast<uint2*>(sC + ml * (TN * 2) + ((((nl >> 3) ^ (ml & (CCH - 1))) << 4) | ((nl & 4) << 1))) = pk;
        }
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < TM * TN / 8 / THREADS; ++it) {
        const int c = threadIdx.x + it * THREADS;
        const int rl = c / CCH, ch = c % CCH;
        const int row = m0 + rl, col = n0 + ch * 8;
        if (row >= g.M || col >= g.N) continue;
        uint4 v = *reinterpret_cast<const uint4*>(sC + rl * (TN * 2) + ((ch ^ (rl & (CCH - 1))) << 4));
        bf16_t* dst = g.C + (long long)row * g.ldc + col;
        if (g.accumulate) {
            float x[8], y[8];
            ElemIO<bf16_t>::load_vec(dst, x);
            ElemIO<bf16_t>::load_vec(reinterpret_cast<const bf16_t*>(&v), y);
#pragma unroll
            for (int e = 0; e < 8; ++e) x[e] += y[e];
            ElemIO<bf16_t>::store_vec(dst, x);
        } else {
            *reinterpret_cast<uint4*>(dst) = v;
        }
    }
}

}  // namespace

int ed_gemm_nt_launch(const GemmCall& c, const GemmPlan& p, hipStream_t s) {
    const int tn = (p.kernel == ED_K_NT_64 || p.kernel == ED_K_NT_RING64) ? 64 : 128;
    NtArgs g;
    g.A = (const bf16_t*)c.A; g.B = (const bf16_t*)c.B; g.C = (bf16_t*)c.C;
    g.bias1 = c.bias1; g.bias2 = c.bias2;
    g.lda = c.lda; g.ldb = c.ldb; g.ldc = c.ldc;
    g.M = c.M; g.N = c.N; g.K = c.K;
    g.accumulate = c.accumulate;
    g.debug = ed_env_once("EDGEDICT_GEMM_NT_DEBUG", 0);
    g.n_tiles = (c.N + tn - 1) / tn;
    g.tiles = (int)p.grid;
    const dim3 grid(p.grid), block(p.block);
    if (p.kernel == ED_K_NT_RING64) hipLaunchKernelGGL(gemm_nt_ring64_kernel, grid, block, 0, s, g);
    else if (p.kernel == ED_K_NT_64) hipLaunchKernelGGL((gemm_nt_kernel<64, 64, 32>), grid, block, 0, s, g);
    else if (p.kernel == ED_K_NT_256X128) hipLaunchKernelGGL((gemm_nt_kernel<256, 128, 64>), grid, block, 0, s, g);
    else hipLaunchKernelGGL((gemm_nt_kernel<128, 128, 64>), grid, block, 0, s, g);
    ED_CHECK_LAUNCH("gemm_nt");
    return ED_OK;
}
