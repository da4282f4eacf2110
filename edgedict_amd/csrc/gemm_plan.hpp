// The GEMM family's internal interface: one description of a product (GemmCall), one plan of how it runs (GemmPlan).
// gemm.hip decides (ed_gemm_plan) and dispatches (ed_gemm_run); gemm_nt.hip, gemm_nt256.hip, gemm_nt256r.hip and
// gemm_tn256.hip each hold their kernels and ONE launcher that fills the argument block and launches what the plan says.
#pragma once
#include <hip/hip_runtime.h>

struct GemmCall {
    int dtype_in, dtype_out;
    const void* A; long long lda; int a_kmajor;
    const void* B; long long ldb; int b_kmajor;
    void* C; long long ldc;
    int M, N, K;
    const float* bias1; const float* bias2;
    int accumulate, split_k;
    int max_wg_per_cu;   // > 0: background form (edgedict_gemm_bg)
    float* partials;     // non-null: quiet form, the K slices are written once and summed by a reduce pass
    int slice_cap;       // the most slices `partials` holds for the tn256 kernel (the generic kernel rounds split_k itself)
    bool unreduced;      // leave the slices in `partials`, C == partials (ed_gemm_quiet_partials)
    float* lse_part;     // non-null: edgedict_gemm_nt_lse ([M][ceil(N/64)][2] fp32 log-sum-exp partials)
};

// One value per __global__ entry (the generic kernel's four layout pairs share a value: the layout is in the call).
// The numbers are part of edgedict_gemm_plan's record (include/edgedict_hip.h).
enum GemmKernel {
    ED_K_NONE = 0,                                        // empty product: nothing runs
    ED_K_GENERIC_BF16_BF16 = 1, ED_K_GENERIC_BF16_BF16_FAST = 2,   // gemm.hip gemm_kernel<TI, TO, ., ., FAST>
    ED_K_GENERIC_BF16_F32 = 3, ED_K_GENERIC_BF16_F32_FAST = 4,
    ED_K_GENERIC_F32_F32 = 5, ED_K_GENERIC_F32_F32_FAST = 6,
    ED_K_NT_64 = 7, ED_K_NT_128 = 8, ED_K_NT_256X128 = 9,   // gemm_nt.hip gemm_nt_kernel<64,64,32> <128,128,64> <256,128,64>
    ED_K_NT_RING64 = 10,                                  // gemm_nt.hip gemm_nt_ring64_kernel
    ED_K_NT256 = 11,                                      // gemm_nt256.hip
    ED_K_NT256R = 12, ED_K_NT256R_LSE = 13,               // gemm_nt256r.hip gemm_nt256r_kernel<LSE>
    ED_K_TN256 = 14,                                      // gemm_tn256.hip
};
// vendor routes (blaslt.hpp) that are tried first; the plan's kernel runs when the bridge declines
enum GemmVendor { ED_VENDOR_NONE = 0, ED_VENDOR_NT_LOGITS = 1, ED_VENDOR_NT_SMALL = 2, ED_VENDOR_TN_F32 = 3 };

struct GemmPlan {
    int kernel;              // GemmKernel
    unsigned grid;
    int block, lds;          // threads per workgroup, dynamic LDS bytes
    int split, k_per_split;  // K slices that run (1 and 0 for the kernels that do not split K)
    bool zero_first;         // atomics need a defined starting value: zero_f32 precedes
    bool reduce_after;       // reduce_partials_kernel sums the slices into C
    int vendor;              // GemmVendor
};

constexpr int ED_NT256_LDS_BYTES = 128 * 1024, ED_NT256R_LDS_BYTES = 129 * 1024, ED_TN256_LDS_BYTES = 96 * 1024;

// Pure: no launch, no HIP call but ed_device_cus(), writes nothing but `p` (and the error text when it fails).
int ed_gemm_plan(const GemmCall& c, GemmPlan& p);
// *slices (nullable): the number of K slices written (1 when a vendor route took the product)
int ed_gemm_run(const GemmCall& c, const GemmPlan& p, hipStream_t s, int* slices = nullptr);

int ed_gemm_nt_launch(const GemmCall& c, const GemmPlan& p, hipStream_t s);
int ed_gemm_nt256_launch(const GemmCall& c, const GemmPlan& p, hipStream_t s);
int ed_gemm_nt256r_launch(const GemmCall& c, const GemmPlan& p, hipStream_t s);
int ed_gemm_tn256_launch(const GemmCall& c, const GemmPlan& p, hipStream_t s);
