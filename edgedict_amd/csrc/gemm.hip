// MFMA GEMM for gfx950:  C[M,N] (+)= A[M,K] * B[N,K]^T + bias1[N] + bias2[N]
//
// One kernel template serves every dense product on the RNN-T path (reference call sites:
// nn.LSTM input products rnnt/models.py:45-46,65; nn.Linear at rnnt/models.py:129,135,148,156,
// 165-167 and their autograd transposes).  Both operands are described by (pointer, leading
// dimension, k_major flag):
//     k_major = 1 : element (row, k) at  p[row*ld + k]   (K contiguous: x @ W^T forward form)
//     k_major = 0 : element (row, k) at  p[k*ld + row]   (row contiguous: the transposed
//                   operand of dX = dY*W and dW = dY^T*X; transposed on the way into LDS)
// so NT / NN / TN / TT products need no materialised transposes.
//
// Tiling (wave64, 256 threads = 2x2 waves): block tile 128x128, wave tile 64x64 = 4x4 MFMA tiles
// of 16x16.  bf16 inputs use v_mfma_f32_16x16x32_bf16 (BK = 64), fp32 inputs use the exact
// v_mfma_f32_16x16x4_f32 (BK = 16).  Accumulation is always fp32.  Operand tiles are staged
// global -> registers -> LDS (rows padded by 16 B against ds_read bank conflicts) with the next
// tile's global loads issued before the current tile's MFMAs.
// split_k > 1 partitions K over workgroups (XCD-aware: one K slice per XCD) and combines with fp32
// atomics (gradient "+=").
#include "common.hpp"
#include "gemm_plan.hpp"
#include "blaslt.hpp"

namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_t;
typedef __attribute__((ext_vector_type(4))) float f32x4_t;

constexpr int BM = 128, BN = 128;
constexpr int THREADS = 256;

template <typename TI> struct Cfg;
template <> struct Cfg<bf16_t> {
    static constexpr int BK = 64;      // elements of K per LDS tile
    static constexpr int ROW = BK + 8; // padded LDS row (elements): 144 B
    static constexpr int VEC = 8;      // elements per 16-byte chunk
};
template <> struct Cfg<float> {
    static constexpr int BK = 16;
    static constexpr int ROW = BK + 4;  // 80 B
    static constexpr int VEC = 4;
};

struct GemmArgs {
    const void* A;
    const void* B;
    void* C;
    const float* bias1;
    const float* bias2;
    long long lda, ldb, ldc;
    int M, N, K;
    int a_vec, b_vec;  // 16-byte vector path usable for the operand
    int c_vec;         // bf16 output rows are 16-byte addressable (ldc % 8 == 0, N % 8 == 0)
    int accumulate;
    int split_k;
    int k_per_split;  // multiple of BK
    int items;        // tiles * split_k
    float* partials;  // non-null: slice s stores its tiles to partials + s*partial_stride ([M][N] dense,
    long long partial_stride;   // plain stores, no atomics); the caller sums the slices
};

// ---- staging registers: the 16-byte chunks one thread moves per operand tile
template <typename TI> struct Stage { uint4 v[Cfg<TI>::BK * BM / Cfg<TI>::VEC / THREADS]; };

template <typename TI, bool FAST>
__device__ __forceinline__ uint4 load_chunk_guarded(const TI* p, long long ld, int vec_ok,
                                                    int r0, int rmax, int c0, int cmax,
                                                    bool along_row) {
    // Loads VEC elements starting at logical (r0, c0) walking along the contiguous dimension.
    // along_row: contiguous index is c (k_major: r = row, c = k); else contiguous index is r.
    constexpr int VEC = Cfg<TI>::VEC;
    if constexpr (FAST) {
        // host guarantees 16-byte alignment and that the contiguous extent is a multiple of VEC,
        // so a chunk is either wholly inside or wholly outside: one unconditional load from a
        // clamped address + select.  No branches, no waits: every load of a tile is in flight
        // together.
        const bool ok = (r0 < rmax) && (c0 < cmax);
        const long long off = along_row ? (long long)r0 * ld + c0 : (long long)c0 * ld + r0;
        uint4 v = *reinterpret_cast<const uint4*>(p + (ok ? off : 0));
        if (!ok) v = make_uint4(0, 0, 0, 0);
        return v;
    }
    uint4 out = make_uint4(0, 0, 0, 0);
    TI* o = reinterpret_cast<TI*>(&out);
    if (along_row) {
        if (r0 >= rmax) return out;
        const TI* src = p + (long long)r0 * ld + c0;
        if (vec_ok && c0 + VEC <= cmax) return *reinterpret_cast<const uint4*>(src);
#pragma unroll
        for (int i = 0; i < VEC; ++i)
            if (c0 + i < cmax) o[i] = src[i];
    } else {
        if (c0 >= cmax) return out;
        const TI* src = p + (long long)c0 * ld + r0;
        if (vec_ok && r0 + VEC <= rmax) return *reinterpret_cast<const uint4*>(src);
#pragma unroll
        for (int i = 0; i < VEC; ++i)
            if (r0 + i < rmax) o[i] = src[i];
    }
    return out;
}

// K-major operand: chunk c -> (row = c / (BK/VEC), kc = c % (BK/VEC))
template <typename TI, bool FAST>
__device__ __forceinline__ void gload_kmajor(Stage<TI>& st, const TI* p, long long ld, int vec_ok,
                                             int row0, int rows, int k0, int kend) {
    constexpr int CPR = Cfg<TI>::BK / Cfg<TI>::VEC;
    constexpr int N = Cfg<TI>::BK * BM / Cfg<TI>::VEC / THREADS;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const int c = threadIdx.x + i * THREADS;
        const int r = c / CPR, kc = c % CPR;
        st.v[i] = load_chunk_guarded<TI, FAST>(p, ld, vec_ok, row0 + r, rows,
                                               k0 + kc * Cfg<TI>::VEC, kend, true);
    }
}
// bf16 tiles: the 16-byte chunk kc of row r lives at chunk position kc ^ ((r >> 3) & 7).  Rows that
// are 8 apart start on the same LDS bank (8 * 144 B = 9 * 128 B), which is exactly the stride of
// the transposing store below; the XOR spreads them over the 8 chunk positions.
template <typename TI> __device__ __forceinline__ int swz(int r, int kc) { return kc; }
template <> __device__ __forceinline__ int swz<bf16_t>(int r, int kc) { return kc ^ ((r >> 3) & 7); }

template <typename TI>
__device__ __forceinline__ void sstore_kmajor(const Stage<TI>& st, TI* lds) {
    constexpr int CPR = Cfg<TI>::BK / Cfg<TI>::VEC;
    constexpr int N = Cfg<TI>::BK * BM / Cfg<TI>::VEC / THREADS;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const int c = threadIdx.x + i * THREADS;
        const int r = c / CPR, kc = c % CPR;
        *reinterpret_cast<uint4*>(lds + r * Cfg<TI>::ROW + swz<TI>(r, kc) * Cfg<TI>::VEC) = st.v[i];
    }
}

// Row-major-in-k ("transposed") operand.  fp32: item = (k, 4 rows); bf16: item = (k pair, 8 rows)
template <bool FAST>
__device__ __forceinline__ void gload_tr(Stage<float>& st, const float* p, long long ld,
                                         int vec_ok, int row0, int rows, int k0, int kend) {
    constexpr int CPK = BM / 4;  // chunks per k line
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int c = threadIdx.x + i * THREADS;
        const int k = c / CPK, rc = c % CPK;
        st.v[i] = load_chunk_guarded<float, FAST>(p, ld, vec_ok, row0 + rc * 4, rows, k0 + k, kend,
                                                  false);
    }
}
__device__ __forceinline__ void sstore_tr(const Stage<float>& st, float* lds) {
    constexpr int CPK = BM / 4;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int c = threadIdx.x + i * THREADS;
        const int k = c / CPK, rc = c % CPK;
        const float* f = reinterpret_cast<const float*>(&st.v[i]);
#pragma unroll
        for (int j = 0; j < 4; ++j) lds[(rc * 4 + j) * Cfg<float>::ROW + k] = f[j];
    }
}
template <bool FAST>
__device__ __forceinline__ void gload_tr(Stage<bf16_t>& st, const bf16_t* p, long long ld,
                                         int vec_ok, int row0, int rows, int k0, int kend) {
    constexpr int CPK = BM / 8;  // 16 chunks per k line
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int item = threadIdx.x + i * THREADS;  // 512 items = 32 k-pairs x 16 chunks
        const int kp = item / CPK, rc = item % CPK;
        st.v[2 * i] = load_chunk_guarded<bf16_t, FAST>(p, ld, vec_ok, row0 + rc * 8, rows,
                                                       k0 + 2 * kp, kend, false);
        st.v[2 * i + 1] = load_chunk_guarded<bf16_t, FAST>(p, ld, vec_ok, row0 + rc * 8, rows,
                                                           k0 + 2 * kp + 1, kend, false);
    }
}
__device__ __forceinline__ void sstore_tr(const Stage<bf16_t>& st, bf16_t* lds) {
    constexpr int CPK = BM / 8;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int item = threadIdx.x + i * THREADS;
        const int kp = item / CPK, rc = item % CPK;
        const unsigned* a = reinterpret_cast<const unsigned*>(&st.v[2 * i]);      // k even
        const unsigned* b = reinterpret_cast<const unsigned*>(&st.v[2 * i + 1]);  // k odd
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            // rows 2j, 2j+1 of this chunk; pack (k, k+1) for each row into one dword
            const unsigned lo = (a[j] & 0xffffu) | (b[j] << 16);
            const unsigned hi = (a[j] >> 16) | (b[j] & 0xffff0000u);
            // all 8 rows of this chunk share (row >> 3) = rc, hence one swizzled chunk position
            const int pos = (((kp >> 2) ^ (rc & 7)) << 3) + ((2 * kp) & 7);
            unsigned* d0 = reinterpret_cast<unsigned*>(lds + (rc * 8 + 2 * j) * Cfg<bf16_t>::ROW + pos);
            unsigned* d1 = reinterpret_cast<unsigned*>(lds + (rc * 8 + 2 * j + 1) * Cfg<bf16_t>::ROW + pos);
            *d0 = lo;
            *d1 = hi;
        }
    }
}

template <typename TI, bool KMAJOR, bool FAST>
__device__ __forceinline__ void gload(Stage<TI>& st, const TI* p, long long ld, int vec_ok,
                                      int row0, int rows, int k0, int kend) {
    if constexpr (KMAJOR) gload_kmajor<TI, FAST>(st, p, ld, vec_ok, row0, rows, k0, kend);
    else gload_tr<FAST>(st, p, ld, vec_ok, row0, rows, k0, kend);
}
template <typename TI, bool KMAJOR>
__device__ __forceinline__ void sstore(const Stage<TI>& st, TI* lds) {
    if constexpr (KMAJOR) sstore_kmajor<TI>(st, lds);
    else sstore_tr(st, lds);
}

// ---- MFMA over one LDS tile pair
__device__ __forceinline__ void mma_tile(const bf16_t* sA, const bf16_t* sB, f32x4_t (&acc)[4][4],
                                         int wm, int wn, int lane) {
    constexpr int ROW = Cfg<bf16_t>::ROW;
    const int r = lane & 15, kq = lane >> 4;
#pragma unroll
    for (int ks = 0; ks < Cfg<bf16_t>::BK / 32; ++ks) {
        bf16x8_t a[4], b[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int ra = wm * 64 + i * 16 + r, rb = wn * 64 + i * 16 + r;
            a[i] = *reinterpret_cast<const bf16x8_t*>(sA + ra * ROW + swz<bf16_t>(ra, ks * 4 + kq) * 8);
            b[i] = *reinterpret_cast<const bf16x8_t*>(sB + rb * ROW + swz<bf16_t>(rb, ks * 4 + kq) * 8);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
    }
}
__device__ __forceinline__ void mma_tile(const float* sA, const float* sB, f32x4_t (&acc)[4][4],
                                         int wm, int wn, int lane) {
    constexpr int ROW = Cfg<float>::ROW;
    const int r = lane & 15, kq = lane >> 4;
#pragma unroll
    for (int ks = 0; ks < Cfg<float>::BK / 4; ++ks) {
        float a[4], b[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            a[i] = sA[(wm * 64 + i * 16 + r) * ROW + ks * 4 + kq];
            b[i] = sB[(wn * 64 + i * 16 + r) * ROW + ks * 4 + kq];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[j], acc[i][j], 0, 0, 0);
    }
}

template <typename TI, typename TO, bool A_KM, bool B_KM, bool FAST>
__global__ __launch_bounds__(THREADS) void gemm_kernel(GemmArgs g) {
    using C_ = Cfg<TI>;
    __shared__ __attribute__((aligned(16))) TI smem[(BM + BN) * C_::ROW];
    TI* sA = smem;
    TI* sB = smem + BM * C_::ROW;

    // N index fastest: consecutive blocks share the same A row panel (L2 reuse)
    const int n_tiles = (g.N + BN - 1) / BN;
    // split-K launches are 1-D with the K slice FASTEST (slice = id % split_k, split_k % 8 == 0):
    // workgroup id % 8 is the XCD, so every tile of one K slice runs on the SAME XCD and the slice's
    // operand rows are fetched from HBM once into that XCD's L2 instead of once per XCD
    // (measured on the joint dW2 product: 26.5 GB of HBM reads for 4.5 GB of operands before).
    // Work items = tiles x K slices.  A normal launch has one workgroup per item; a BACKGROUND launch
    // (edgedict_gemm_bg) has only as many workgroups as are resident at once and each walks its
    // items (stride gridDim.x, a multiple of split_k: the slice, hence the XCD, stays fixed).  A
    // grid with more workgroups than fit parks its tail in the dispatcher, and on this chip that
    // blocks the dispatch of OTHER queues' kernels (measured: 60 us per tiny kernel on the main
    // stream while a 1280-workgroup dW GEMM ran on the auxiliary stream).
    const TI* A = reinterpret_cast<const TI*>(g.A);
    const TI* B = reinterpret_cast<const TI*>(g.B);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = wave >> 1, wn = wave & 1;
  for (int item = blockIdx.x; item < g.items; item += gridDim.x) {
    const int tile = g.split_k > 1 ? item / g.split_k : item;
    const int slice = g.split_k > 1 ? item % g.split_k : 0;
    const int m0 = (tile / n_tiles) * BM;
    const int n0 = (tile % n_tiles) * BN;
    const int kbeg = slice * g.k_per_split;
    const int kend = min(g.K, kbeg + g.k_per_split);

    f32x4_t acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

    Stage<TI> ra, rb;
    if (kbeg < kend) {
        gload<TI, A_KM, FAST>(ra, A, g.lda, g.a_vec, m0, g.M, kbeg, kend);
        gload<TI, B_KM, FAST>(rb, B, g.ldb, g.b_vec, n0, g.N, kbeg, kend);
        sstore<TI, A_KM>(ra, sA);
        sstore<TI, B_KM>(rb, sB);
    }
    __syncthreads();
    for (int k0 = kbeg; k0 < kend; k0 += C_::BK) {
        const bool more = (k0 + C_::BK) < kend;
        if (more) {
            gload<TI, A_KM, FAST>(ra, A, g.lda, g.a_vec, m0, g.M, k0 + C_::BK, kend);
            gload<TI, B_KM, FAST>(rb, B, g.ldb, g.b_vec, n0, g.N, k0 + C_::BK, kend);
        }
        mma_tile(sA, sB, acc, wm, wn, lane);
        __syncthreads();
        if (more) {
            sstore<TI, A_KM>(ra, sA);
            sstore<TI, B_KM>(rb, sB);
        }
        __syncthreads();
    }

    // epilogue: lane holds D[row = (lane>>4)*4 + r][col = lane&15] of each 16x16 tile
    TO* C = reinterpret_cast<TO*>(g.C);
    const bool first_split = (slice == 0);
    if constexpr (sizeof(TO) == 2 && sizeof(TI) == 2) {
        if (g.c_vec) {
            // bf16 output: round in registers, stage the 128x128 tile in LDS (the operand tiles
            // are dead after the last barrier) and leave the CU as full 16-byte row segments
            constexpr int CROW = BN + 8;
            bf16_t* sC = reinterpret_cast<bf16_t*>(smem);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int cl = wn * 64 + j * 16 + (lane & 15);
                const int col = n0 + cl;
                float bias = 0.f;
                if (col < g.N) {
                    if (g.bias1) bias += g.bias1[col];
                    if (g.bias2) bias += g.bias2[col];
                }
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        sC[(wm * 64 + i * 16 + (lane >> 4) * 4 + r) * CROW + cl] =
                            f32_to_bf16(acc[i][j][r] + bias);
            }
            __syncthreads();
#pragma unroll
            for (int it = 0; it < BM * BN / 8 / THREADS; ++it) {
                const int c = threadIdx.x + it * THREADS;
                const int rl = c / (BN / 8), ch = c % (BN / 8);
                const int row = m0 + rl, col = n0 + ch * 8;
                if (row >= g.M || col >= g.N) continue;
                uint4 v = *reinterpret_cast<const uint4*>(sC + rl * CROW + ch * 8);
                bf16_t* dst = reinterpret_cast<bf16_t*>(C) + (long long)row * g.ldc + col;
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
            __syncthreads();   // staging tile consumed before the next item's operand tiles land
            continue;
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int col = n0 + wn * 64 + j * 16 + (lane & 15);
        if (col >= g.N) continue;
        float bias = 0.f;
        if (first_split) {
            if (g.bias1) bias += g.bias1[col];
            if (g.bias2) bias += g.bias2[col];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = m0 + wm * 64 + i * 16 + (lane >> 4) * 4 + r;
                if (row >= g.M) continue;
                const float v = acc[i][j][r] + bias;
                TO* dst = C + (long long)row * g.ldc + col;
                if constexpr (sizeof(TO) == 4) {
                    if (g.partials) g.partials[slice * g.partial_stride + (long long)row * g.N + col] = v;
                    else if (g.split_k > 1) atomicAdd(reinterpret_cast<float*>(dst), v);
                    else if (g.accumulate) *dst = *dst + v;
                    else *dst = v;
                } else {
                    if (g.accumulate) ElemIO<TO>::store(dst, ElemIO<TO>::load(dst) + v);
                    else ElemIO<TO>::store(dst, v);
                }
            }
        }
    }
  }   // items
}

template <typename TI, typename TO, bool FAST>
int launch2(const GemmArgs& g, int a_km, int b_km, dim3 grid, hipStream_t s, int pad) {
    // pad = extra dynamic LDS claimed per workgroup (occupancy cap of background GEMMs)
    if (a_km && b_km) hipLaunchKernelGGL((gemm_kernel<TI, TO, true, true, FAST>), grid, dim3(THREADS), pad, s, g);
    else if (a_km && !b_km) hipLaunchKernelGGL((gemm_kernel<TI, TO, true, false, FAST>), grid, dim3(THREADS), pad, s, g);
    else if (!a_km && b_km) hipLaunchKernelGGL((gemm_kernel<TI, TO, false, true, FAST>), grid, dim3(THREADS), pad, s, g);
    else hipLaunchKernelGGL((gemm_kernel<TI, TO, false, false, FAST>), grid, dim3(THREADS), pad, s, g);
    ED_CHECK_LAUNCH("gemm");
    return ED_OK;
}
// C[m][n] (+)= sum_s part[s][m][n]
__global__ void reduce_partials_kernel(const float* __restrict__ part, long long stride, int S,
                                       float* __restrict__ C, long long ldc, long long M, int N,
                                       int accumulate) {
    const long long n = M * N;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (long long)gridDim.x * blockDim.x) {
        float a = 0.f;
        for (int s = 0; s < S; ++s) a += part[s * stride + i];
        float* dst = C + (i / N) * ldc + (i % N);
        *dst = accumulate ? *dst + a : a;
    }
}

__global__ void zero_f32(float* p, long long rows, long long cols, long long ld) {
    const long long n = rows * cols;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (long long)gridDim.x * blockDim.x)
        p[(i / cols) * ld + (i % cols)] = 0.f;
}

}  // namespace

// ---------------------------------------------------------------- the plan: which kernel, which grid, how many slices
static int pow2_slices(int split_k) {   // quiet slices: the next power of two >= split_k, at most 8
    int p2 = 1;
    while (p2 < split_k && p2 < 8) p2 *= 2;
    return p2;
}
static bool vec16(const void* p, long long ld, int vec) { return (uintptr_t)p % 16 == 0 && ld % vec == 0; }
// what the direct-to-LDS bf16 NT kernels (gemm_nt.hip, gemm_nt256.hip, gemm_nt256r.hip) take
static bool nt_ok(const GemmCall& c) {
    if ((uintptr_t)c.bias1 % 16 != 0 || (uintptr_t)c.bias2 % 16 != 0) return false;   // float4 bias loads
    return c.dtype_in == ED_BF16 && c.dtype_out == ED_BF16 && c.a_kmajor && c.b_kmajor && c.split_k == 1 && c.M > 0 &&
           c.N > 0 && c.K >= 64 && c.K % 64 == 0 && c.lda % 8 == 0 && c.ldb % 8 == 0 && c.ldc % 8 == 0 && c.N % 8 == 0 &&
           (uintptr_t)c.A % 16 == 0 && (uintptr_t)c.B % 16 == 0 && (uintptr_t)c.C % 16 == 0;
}
static bool nt256_shape_ok(int M, int N, int K) { return M > 0 && N > 0 && K >= 128 && K % 64 == 0; }
static bool tn256_ok(const GemmCall& c) {
    return ed_env_once("EDGEDICT_GEMM_TN256", 1) && c.M >= 8 && c.N >= 8 && c.K >= 1 && c.M % 8 == 0 && c.N % 8 == 0 &&
           c.lda % 8 == 0 && c.ldb % 8 == 0 && (uintptr_t)c.A % 16 == 0 && (uintptr_t)c.B % 16 == 0;
}

int ed_gemm_plan(const GemmCall& c, GemmPlan& p) {
    p = GemmPlan{};
    const int M = c.M, N = c.N, K = c.K, n_cu = ed_device_cus();
    if (M == 0 || N == 0) return ED_OK;
    p.split = 1;
    const bool has_bias = c.bias1 || c.bias2;
    // bf16 NT products with K % 64 == 0 take the direct-to-LDS kernels
    const bool nt = ed_env_once("EDGEDICT_GEMM_NT", 1) && c.max_wg_per_cu == 0 && nt_ok(c);
    // large ones (worth it from ~2 tiles per CU on; the 128 x 128 kernel keeps the small and the accumulating products)
    // and the log-sum-exp entry: 256 x 256 tiles, ahead of the vendor route
    const long long tiles256 = (long long)((M + 255) / 256) * ((N + 255) / 256);
    if (c.lse_part || (nt && ed_env_once("EDGEDICT_GEMM_NT256", 1) && !c.accumulate && nt256_shape_ok(M, N, K) &&
                       tiles256 >= 512)) {
        ED_CHECK_ARG(tiles256 < (1ll << 31), "gemm: too many tiles");
        // the persistent ring kernel: one workgroup per CU walks the tiles.  A workgroup keeps ONE bias fragment, so with
        // a bias all of its tiles must lie in the same column tile; else one tile per workgroup (gemm_nt256.hip).
        // (EDGEDICT_GEMM_NT256R is read at every call: tests/test_gemm_gpu.py compares both kernels in one process)
        const int n_tiles = (N + 255) / 256, cus = n_cu - n_cu % 8;
        const int grid = (int)(tiles256 < cus ? tiles256 : cus);
        const bool ring = ed_env_now("EDGEDICT_GEMM_NT256R", 1) &&
                          !(has_bias && tiles256 > grid && ((grid / 8) % n_tiles != 0 || grid % 8 != 0));
        p.kernel = !ring ? ED_K_NT256 : c.lse_part ? ED_K_NT256R_LSE : ED_K_NT256R;
        p.grid = ring ? grid : (unsigned)tiles256;
        p.block = 512;
        p.lds = ring ? ED_NT256R_LDS_BYTES : ED_NT256_LDS_BYTES;
        return ED_OK;
    }
    // the one plain product that is large AND output-heavy (short K: the joint's logits) goes to the vendor library
    // when it is there (blaslt.cpp says why), and so do the long-K, few-tiles products of the encoder stack's backward
    // chain (dX of a chunk: [768..1536 x 1024 x 4096], 19-23 us there vs 32 us here, tools/blas_probe2.py;
    // EDGEDICT_BLASLT_SMALL measured: step 27.17 -> 27.01 ms); everything else runs here
    const bool plain_nt = c.dtype_in == ED_BF16 && c.dtype_out == ED_BF16 && c.a_kmajor && c.b_kmajor && c.split_k == 1 &&
                          c.max_wg_per_cu == 0 && c.lda % 8 == 0 && c.ldb % 8 == 0 && c.ldc % 8 == 0;
    if (plain_nt && !c.accumulate && !c.bias2 && K >= 1 && K <= 1024 && N >= 1024 && (long long)M * N >= (1ll << 28))
        p.vendor = ED_VENDOR_NT_LOGITS;
    else if (plain_nt && !has_bias && K >= 2048 && M <= 4096 && N <= 2048 && M >= 256 &&
             ed_env_once("EDGEDICT_BLASLT_SMALL", 1))
        p.vendor = ED_VENDOR_NT_SMALL;
    if (nt) {
        // small problem: spread it out over 64 x 64 tiles (<256,128,64> measured slower everywhere; kept for
        // re-measurement), and those with a long K onto the ring kernel
        const int force = ed_env_once("EDGEDICT_GEMM_NT_TILE", 0);
        int tm = 128, tn = 128;
        if (force == 64 || (!force && (long long)((M + 127) / 128) * ((N + 127) / 128) <= 128)) tm = tn = 64;
        else if (force == 256) tm = 256;
        const long long tiles = (long long)((M + tm - 1) / tm) * ((N + tn - 1) / tn);
        ED_CHECK_ARG(tiles < (1ll << 31), "gemm: too many tiles");
        p.kernel = tm == 256 ? ED_K_NT_256X128 : tm == 128 ? ED_K_NT_128 :
                   ed_env_once("EDGEDICT_GEMM_NT_RING", 1) && K >= 1024 && !ed_env_once("EDGEDICT_GEMM_NT_DEBUG", 0)
                       ? ED_K_NT_RING64 : ED_K_NT_64;   // (the probe bits exist in gemm_nt_kernel only)
        p.grid = (unsigned)tiles;
        p.block = tm == 256 ? 512 : 256;
        return ED_OK;
    }
    // large bf16 weight gradients (both operands row-major over the reduction) from the background entries: 256-row tiles
    // pull fewer bytes per flop through the CU fetch path that the recurrence beside them is bound by - with a partials
    // buffer the own quiet kernel (gemm_tn256.hip) + the reduce pass, else the vendor's
    const bool dw = c.dtype_in == ED_BF16 && c.dtype_out == ED_F32 && !c.a_kmajor && !c.b_kmajor &&
                    (long long)M * N >= (1ll << 18);
    if (dw && c.partials && K >= 1024 && tn256_ok(c)) {
        // K slices that fill the chip with one workgroup per CU (96 KB LDS), at most slice_cap, at least 8 K stages each
        const long long tiles = (long long)((M + 255) / 256) * ((N + 127) / 128);
        long long s = n_cu / tiles < c.slice_cap ? n_cu / tiles : c.slice_cap;
        while (s > 1 && s * 8 > (K + 31) / 32) --s;
        if (s < 1) s = 1;
        ED_CHECK_ARG(tiles * s < (1ll << 30), "gemm_tn256: too many tiles");
        const int items = (int)(tiles * s);
        int grid = n_cu < items ? n_cu : items;
        if (grid > 8) grid = grid / 8 * 8;
        const int per = (items + grid - 1) / grid;    // items a workgroup walks
        p.kernel = ED_K_TN256;
        p.grid = (items + per - 1) / per;
        p.block = 512;
        p.lds = ED_TN256_LDS_BYTES;
        p.split = (int)s;
        p.k_per_split = (int)(((K + s - 1) / s + 63) / 64 * 64);
        p.reduce_after = !c.unreduced;
        return ED_OK;
    }
    if (dw && (c.max_wg_per_cu > 0 || c.partials) && !has_bias && K >= 4096 && c.lda % 8 == 0 && c.ldb % 8 == 0 &&
        c.ldc % 4 == 0)
        p.vendor = ED_VENDOR_TN_F32;
    // ---- the generic kernel
    const bool f32 = c.dtype_in == ED_F32;
    const int bk = f32 ? 16 : 64, vec = f32 ? 4 : 8, ktiles = (K + bk - 1) / bk;
    int split = c.split_k;
    if (c.partials) split = pow2_slices(split);   // quiet: few long-lived slices (power of two keeps slice <-> XCD set fixed)
    else if (split > 1) split = (split + 7) / 8 * 8;   // whole K slices per XCD (see the kernel)
    if (split > ktiles) split = ktiles > 0 ? ktiles : 1;
    p.split = split;
    p.k_per_split = ktiles > 0 ? ((ktiles + split - 1) / split) * bk : bk;
    p.zero_first = split > 1 && !c.accumulate && !c.partials;
    p.reduce_after = c.partials && !c.unreduced;
    const long long tiles = (long long)((M + BM - 1) / BM) * ((N + BN - 1) / BN);
    ED_CHECK_ARG(tiles < (1ll << 31), "gemm: too many tiles");
    ED_CHECK_ARG(tiles * split < (1ll << 31), "gemm: too many workgroups");
    long long nwg = tiles * split;
    if (c.max_wg_per_cu > 0) {
        // background: only as many workgroups as are resident at once (see the kernel) ...
        long long cap = (long long)c.max_wg_per_cu * n_cu;
        if (split > 1) cap = cap / split * split;   // keep item % split_k fixed per workgroup
        if (cap >= split && nwg > cap) nwg = cap;
        // ... and each claims enough extra LDS that only max_wg_per_cu workgroups fit on a CU
        const int stat = (BM + BN) * (f32 ? Cfg<float>::ROW * 4 : Cfg<bf16_t>::ROW * 2);
        const int want = (160 * 1024) / (c.max_wg_per_cu + 1) + 1024;   // one more would not fit
        if (want > stat) p.lds = (want - stat + 255) / 256 * 256;
    }
    p.grid = (unsigned)nwg;
    p.block = THREADS;
    // FAST: both operands 16-byte aligned with a leading dimension that is a multiple of the vector width, and the
    // contiguous extent of each operand a multiple of it as well
    const bool fast = vec16(c.A, c.lda, vec) && vec16(c.B, c.ldb, vec) && (c.a_kmajor ? K : M) % vec == 0 &&
                      (c.b_kmajor ? K : N) % vec == 0;
    p.kernel = (f32 ? ED_K_GENERIC_F32_F32 : c.dtype_out == ED_F32 ? ED_K_GENERIC_BF16_F32 : ED_K_GENERIC_BF16_BF16) + fast;
    return ED_OK;
}

static int generic_launch(const GemmCall& c, const GemmPlan& p, hipStream_t s) {
    const int vec = c.dtype_in == ED_F32 ? 4 : 8;
    GemmArgs g;
    g.A = c.A; g.B = c.B; g.C = c.C; g.bias1 = c.bias1; g.bias2 = c.bias2;
    g.lda = c.lda; g.ldb = c.ldb; g.ldc = c.ldc; g.M = c.M; g.N = c.N; g.K = c.K;
    g.a_vec = vec16(c.A, c.lda, vec);
    g.b_vec = vec16(c.B, c.ldb, vec);
    g.c_vec = c.dtype_out == ED_BF16 && vec16(c.C, c.ldc, 8) && c.N % 8 == 0;
    g.accumulate = c.accumulate;
    g.split_k = p.split;
    g.k_per_split = p.k_per_split;
    g.items = (int)((long long)((c.M + BM - 1) / BM) * ((c.N + BN - 1) / BN) * p.split);
    g.partials = c.partials;
    g.partial_stride = (long long)c.M * c.N;
    const dim3 grid(p.grid, 1, 1);
    switch (p.kernel) {
    case ED_K_GENERIC_BF16_BF16_FAST: return launch2<bf16_t, bf16_t, true>(g, c.a_kmajor, c.b_kmajor, grid, s, p.lds);
    case ED_K_GENERIC_BF16_BF16: return launch2<bf16_t, bf16_t, false>(g, c.a_kmajor, c.b_kmajor, grid, s, p.lds);
    case ED_K_GENERIC_BF16_F32_FAST: return launch2<bf16_t, float, true>(g, c.a_kmajor, c.b_kmajor, grid, s, p.lds);
    case ED_K_GENERIC_BF16_F32: return launch2<bf16_t, float, false>(g, c.a_kmajor, c.b_kmajor, grid, s, p.lds);
    case ED_K_GENERIC_F32_F32_FAST: return launch2<float, float, true>(g, c.a_kmajor, c.b_kmajor, grid, s, p.lds);
    default: return launch2<float, float, false>(g, c.a_kmajor, c.b_kmajor, grid, s, p.lds);
    }
}

int ed_gemm_run(const GemmCall& c, const GemmPlan& p, hipStream_t s, int* slices) {
    if (slices) *slices = p.split;
    if (p.kernel == ED_K_NONE) return ED_OK;
    if (p.vendor == ED_VENDOR_TN_F32
            ? ed_blaslt_tn_f32(c.A, c.lda, c.B, c.ldb, (float*)c.C, c.ldc, c.M, c.N, c.K, c.accumulate, s)
            : p.vendor && ed_blaslt_nt_bf16(c.A, c.lda, c.B, c.ldb, c.C, c.ldc, c.M, c.N, c.K, c.bias1, c.accumulate, s)) {
        if (slices) *slices = 1;
        return ED_OK;
    }
    if (p.zero_first) {
        hipLaunchKernelGGL(zero_f32, dim3(ed_grid_for((long long)c.M * c.N, 256)), dim3(256), 0, s, (float*)c.C,
                           (long long)c.M, (long long)c.N, c.ldc);
        ED_CHECK_LAUNCH("gemm zero");
    }
    const int rc = p.kernel == ED_K_TN256 ? ed_gemm_tn256_launch(c, p, s)
                 : p.kernel >= ED_K_NT256R ? ed_gemm_nt256r_launch(c, p, s)
                 : p.kernel == ED_K_NT256 ? ed_gemm_nt256_launch(c, p, s)
                 : p.kernel >= ED_K_NT_64 ? ed_gemm_nt_launch(c, p, s) : generic_launch(c, p, s);
    if (rc != ED_OK || !p.reduce_after) return rc;
    hipLaunchKernelGGL(reduce_partials_kernel, dim3(ed_grid_for((long long)c.M * c.N, 256, 2048)), dim3(256), 0, s,
                       c.partials, (long long)c.M * c.N, p.split, (float*)c.C, c.ldc, (long long)c.M, c.N, c.accumulate);
    ED_CHECK_LAUNCH("gemm reduce_partials");
    return ED_OK;
}

// ---------------------------------------------------------------- entry points: validate, describe, plan, run
static int gemm_validate(const GemmCall& c, bool bg) {
    if (c.lse_part) {
        ED_CHECK_ARG(nt256_shape_ok(c.M, c.N, c.K) && nt_ok(c),
                     "gemm_nt_lse: needs bf16 K-contiguous operands, K %% 64 == 0, K >= 128, N %% 8 == 0, "
                     "16-byte aligned pointers and leading dimensions (M=%d N=%d K=%d)", c.M, c.N, c.K);
        return ED_OK;
    }
    ED_CHECK_ARG(!bg || (c.max_wg_per_cu >= 1 && c.max_wg_per_cu <= 8), "gemm_bg: max_wg_per_cu must be 1..8");
    ED_CHECK_ARG(!c.partials || c.dtype_out == ED_F32, "gemm_bg: the quiet (partials) form needs an fp32 output");
    ED_CHECK_ARG(!c.partials || (!c.bias1 && !c.bias2), "gemm_bg: the quiet (partials) form takes no bias");
    ED_CHECK_ARG(c.dtype_in == ED_F32 || c.dtype_in == ED_BF16, "gemm: bad input dtype %d", c.dtype_in);
    ED_CHECK_ARG(c.dtype_out == ED_F32 || c.dtype_out == ED_BF16, "gemm: bad output dtype %d", c.dtype_out);
    ED_CHECK_ARG(!(c.dtype_in == ED_F32 && c.dtype_out == ED_BF16), "gemm: fp32 inputs with bf16 output is not supported");
    ED_CHECK_ARG(c.M >= 0 && c.N >= 0 && c.K >= 0, "gemm: negative dimension");
    ED_CHECK_ARG(c.split_k >= 1, "gemm: split_k must be >= 1");
    ED_CHECK_ARG(c.split_k == 1 || c.dtype_out == ED_F32, "gemm: split_k > 1 needs an fp32 output (atomic +=)");
    // (K == 0: the operands are empty and never read - an empty tensor has no address -, C still gets the bias)
    ED_CHECK_ARG(c.M == 0 || c.N == 0 || (c.C && (c.K == 0 || (c.A && c.B))), "gemm: null operand");
    return ED_OK;
}
static int gemm_go(const GemmCall& c, bool bg, void* stream, int* slices = nullptr) {
    GemmPlan p;
    int rc = gemm_validate(c, bg);
    if (rc == ED_OK) rc = ed_gemm_plan(c, p);
    return rc == ED_OK ? ed_gemm_run(c, p, (hipStream_t)stream, slices) : rc;
}

// internal (encoder_stack.hip): quiet background product that leaves the slices UNREDUCED in `partials`; returns the
// number of slices written through *slices (every caller's partials buffer holds 8 slices: encoder_stack.hip tmpW)
int ed_gemm_quiet_partials(int dtype_in, const void* A, long long lda, int a_kmajor, const void* B,
                           long long ldb, int b_kmajor, int M, int N, int K, int split_k,
                           int max_wg_per_cu, float* partials, int* slices, hipStream_t stream) {
    ED_CHECK_ARG(partials, "gemm: quiet product without a partials buffer");
    return gemm_go({dtype_in, ED_F32, A, lda, a_kmajor, B, ldb, b_kmajor, partials, N, M, N, K, nullptr, nullptr, 0, split_k,
                    max_wg_per_cu, partials, 8, true, nullptr}, false, stream, slices);
}

extern "C" int edgedict_gemm(int dtype_in, int dtype_out, const void* A, long long lda, int a_kmajor,
                             const void* B, long long ldb, int b_kmajor, void* C, long long ldc,
                             int M, int N, int K, const float* bias1, const float* bias2,
                             int accumulate, int split_k, void* stream) {
    return gemm_go({dtype_in, dtype_out, A, lda, a_kmajor, B, ldb, b_kmajor, C, ldc, M, N, K, bias1, bias2, accumulate,
                    split_k, 0, nullptr, 0, false, nullptr}, false, stream);
}

extern "C" int edgedict_gemm_nt_lse(const void* A, long long lda, const void* B, long long ldb, void* C,
                                    long long ldc, int M, int N, int K, const float* bias,
                                    float* lse_part, void* stream) {
    ED_CHECK_ARG(A && B && C && lse_part, "gemm_nt_lse: null pointer");
    return gemm_go({ED_BF16, ED_BF16, A, lda, 1, B, ldb, 1, C, ldc, M, N, K, bias, nullptr, 0, 1, 0, nullptr, 0, false,
                    lse_part}, false, stream);
}

// (the caller's partials buffer holds the next power of two >= split_k, at most 8, slices)
extern "C" int edgedict_gemm_bg(int dtype_in, int dtype_out, const void* A, long long lda,
                                int a_kmajor, const void* B, long long ldb, int b_kmajor, void* C,
                                long long ldc, int M, int N, int K, const float* bias1,
                                const float* bias2, int accumulate, int split_k,
                                int max_wg_per_cu, float* partials, void* stream) {
    return gemm_go({dtype_in, dtype_out, A, lda, a_kmajor, B, ldb, b_kmajor, C, ldc, M, N, K, bias1, bias2, accumulate,
                    split_k, max_wg_per_cu, partials, pow2_slices(split_k), false, nullptr}, true, stream);
}

extern "C" int edgedict_gemm_plan(int dtype_in, int dtype_out, const void* A, long long lda, int a_kmajor,
                                  const void* B, long long ldb, int b_kmajor, void* C, long long ldc, int M,
                                  int N, int K, const float* bias1, const float* bias2, int accumulate,
                                  int split_k, int max_wg_per_cu, float* partials, int lse, int unreduced,
                                  int32_t* record) {
    static float lse_dummy[2];
    ED_CHECK_ARG(record, "gemm_plan: null record");
    const GemmCall c = {dtype_in, dtype_out, A, lda, a_kmajor, B, ldb, b_kmajor, C, ldc, M, N, K, bias1, bias2, accumulate,
                        split_k, max_wg_per_cu, partials, unreduced ? 8 : pow2_slices(split_k), unreduced != 0,
                        lse ? lse_dummy : nullptr};
    GemmPlan p;
    int rc = gemm_validate(c, max_wg_per_cu != 0 && !unreduced);
    if (rc == ED_OK) rc = ed_gemm_plan(c, p);
    if (rc != ED_OK) return rc;
    const int32_t r[ED_GEMM_PLAN_WORDS] = {p.kernel, (int32_t)p.grid, p.block, p.lds, p.split, p.k_per_split,
                                           p.zero_first, p.reduce_after, p.vendor};
    for (int i = 0; i < ED_GEMM_PLAN_WORDS; ++i) record[i] = r[i];
    return ED_OK;
}
