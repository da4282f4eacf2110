/*
 * edgedict_hip.h — C ABI of libedgedict_hip.so, the MI355X (gfx950) RNN-Transducer engine.
 *
 * This is the drop-in boundary one level below the Python class surface
 * (rnnt.models.Transducer / rnnt.stream.PytorchStreamDecoder).  Every entry point
 *   - takes raw DEVICE pointers, sizes and a hipStream_t (passed as void*),
 *   - allocates no caller-visible buffer: the caller (the PyTorch caching allocator in our host
 *     code) owns every tensor and workspace it passes in,
 *   - keeps exactly this per-DEVICE state, created lazily under a mutex and never exposed: three
 *     internal HIP streams + an event pool for the encoder-stack scheduler (edgedict_aux_stream,
 *     edgedict_stack_*), a pinned host word for the give-up codes of bounded in-kernel waits
 *     (edgedict_stack_wsr_error), the timing record read by edgedict_stack_last_timing /
 *     edgedict_stack_launch_times (two 64 KB device buffers, allocated only once
 *     edgedict_stack_time_launches(1) was called), and - only with EDGEDICT_BLASLT=1 in the
 *     environment, when a product is routed to the vendor library - one hipBLASLt handle per device
 *     with a 64 MiB workspace per (device, stream).  Entry points are re-entrant per device; calls that touch
 *     the same device from several host threads must be serialised by the caller
 *     (nn.DataParallel's one-thread-per-GPU pattern is fine: different devices),
 *   - never aborts: it returns ED_OK or a negative status and leaves a message in
 *     edgedict_last_error() (thread-local) which the binding raises as RuntimeError.
 *
 * dtype codes: activations/weights are either fp32 (parity mode) or bf16 (throughput mode);
 * reductions, LSTM cell state, softmax denominators, alpha/beta and costs are always fp32.
 *
 * Each block below cites the reference interface (file:line under the upstream repo)
 * whose arithmetic it replaces.
 */
#ifndef EDGEDICT_HIP_H
#define EDGEDICT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EDGEDICT_ABI_VERSION 2

#define ED_OK 0
#define ED_ERR_INVALID (-1) /* bad argument (shape / dtype / alignment) */
#define ED_ERR_LAUNCH (-2)  /* HIP runtime reported an error */

#define ED_F32 0
#define ED_BF16 1

const char* edgedict_last_error(void);
int edgedict_abi_version(void);

/* ------------------------------------------------------------------------------------
 * RNN-T loss.  Replaces warprnnt_pytorch.RNNTLoss(blank) as called at
 * rnnt/models.py:221,238 and cli/lightning.py:40,91 (third-party, un-vendored; its public
 * C entry points are compute_rnnt_loss / get_workspace_size, which this pair mirrors).
 *
 *   acts        [B, T, U1, V]  raw joint logits (NOT log-softmaxed), contiguous, acts_dtype
 *   labels      [B, U1-1]      int32, padded arbitrarily beyond label_lens[b]
 *   act_lens    [B] int32      valid frames per utterance   (1 <= act_lens[b] <= T)
 *   label_lens  [B] int32      valid labels per utterance   (0 <= label_lens[b] <= U1-1)
 *   costs       [B] fp32       out: -log P(y|x) per utterance
 *   reduced     [1] fp32       out (nullable): reduce_scale * sum_b costs[b]  ('mean' => 1/B)
 *   workspace   edgedict_rnnt_workspace_bytes(B,T,U1) bytes, 16-byte aligned; forward fills
 *               it (log-softmax denominators, alpha, beta, log-likelihoods) and backward
 *               reads it, so it must be kept alive between the two calls.
 *
 * backward writes d(sum_b scale*cost_b)/d(acts) into grads (same shape/dtype as acts):
 *   scale_b = grad_scale_host * (grad_scale_dev ? grad_scale_dev[b*grad_scale_stride] : 1)
 * (stride 0 = one scalar for the batch, stride 1 = per-utterance, reduction 'none') so that the 'mean' reduction's 1/B and autograd's incoming grad_output need no host sync.
 * Cells outside an utterance's (act_lens, label_lens+1) box get exact zeros.
 * Limits: U1 <= 1024, for every edgedict_rnnt_loss_* entry point and for the aligner's (edgedict_rnnt_align*) alike: a
 * larger U1 is ED_ERR_INVALID before anything is launched, and no output is written (edgedict_rnnt_workspace_bytes
 * itself has no limit).  V*sizeof(dtype) must be a multiple of 16 for the vector path (other V take a scalar path).
 */
size_t edgedict_rnnt_workspace_bytes(int B, int T, int U1);
int edgedict_rnnt_loss_forward(const void* acts, int acts_dtype, const int32_t* labels,
                               const int32_t* act_lens, const int32_t* label_lens, int B, int T,
                               int U1, int V, int blank, float* costs, float* reduced,
                               float reduce_scale, void* workspace, void* stream);
/* packed-lattice forward (bf16 logits) with the per-row log-sum-exp partials produced by
 * edgedict_gemm_nt_lse: lse_parts [M_valid][lse_slots][2], lse_slots = ceil(V/64).  Same results as
 * edgedict_rnnt_loss_forward_packed up to the summation order of the denominators. */
int edgedict_rnnt_loss_forward_packed_parts(const void* acts, const int32_t* labels,
                                            const int32_t* act_lens, const int32_t* label_lens,
                                            const long long* row_offsets, int B, int T, int U1,
                                            int V, int blank, float* costs, float* reduced,
                                            float reduce_scale, void* workspace,
                                            const float* lse_parts, int lse_slots, void* stream);
int edgedict_rnnt_loss_backward(const void* acts, int acts_dtype, void* grads,
                                const int32_t* labels, const int32_t* act_lens,
                                const int32_t* label_lens, int B, int T, int U1, int V, int blank,
                                const void* workspace, float grad_scale_host,
                                const float* grad_scale_dev, int grad_scale_stride, void* stream);
/* PACKED lattice variants: `acts` / `grads` hold ONLY the cells inside each utterance's box, row of
 * cell (b,t,u) = row_offsets[b] + t*(label_lens[b]+1) + u (int64 device array [B], exclusive prefix
 * sums of act_lens[b]*(label_lens[b]+1)); T, U1 still bound the (dense, small) lattice workspace.
 * The joint network then only multiplies valid rows: on the E6D2 bench batch 65 % of the dense
 * B*T*U1 rows.  Arithmetic per cell is identical to the dense entry points. */
int edgedict_rnnt_loss_forward_packed(const void* acts, int acts_dtype, const int32_t* labels,
                                      const int32_t* act_lens, const int32_t* label_lens,
                                      const long long* row_offsets, int B, int T, int U1, int V,
                                      int blank, float* costs, float* reduced, float reduce_scale,
                                      void* workspace, void* stream);
int edgedict_rnnt_loss_backward_packed(const void* acts, int acts_dtype, void* grads,
                                       const int32_t* labels, const int32_t* act_lens,
                                       const int32_t* label_lens, const long long* row_offsets,
                                       int B, int T, int U1, int V, int blank, const void* workspace,
                                       float grad_scale_host, const float* grad_scale_dev,
                                       int grad_scale_stride, void* stream);
/* edgedict_rnnt_loss_backward_packed that also leaves the COLUMN SUMS of the gradient matrix it writes (of the fp32 values
 * before they are rounded to the gradient's dtype) as `edgedict_rnnt_grad_colsum_rows(...)` partial rows of V floats in
 * colsum_parts: their sum over rows is the joint's output-bias gradient (rnnt/models.py:165-167 through autograd), which
 * otherwise takes a second pass over the matrix (2.2 GB at the E6D2 bench batch).  _rows returns 0 when the fused form
 * is not available (V * sizeof(element) not a multiple of 16, or V > 2048 for bf16 / 1024 for f32). */
int edgedict_rnnt_grad_colsum_rows(int acts_dtype, int B, int T, int U1, int V);
int edgedict_rnnt_loss_backward_packed_colsum(const void* acts, int acts_dtype, void* grads,
                                              const int32_t* labels, const int32_t* act_lens,
                                              const int32_t* label_lens, const long long* row_offsets,
                                              int B, int T, int U1, int V, int blank, const void* workspace,
                                              float grad_scale_host, const float* grad_scale_dev,
                                              int grad_scale_stride, float* colsum_parts, void* stream);
/* the same for utterances [b0, b0 + nb) of the batch only (all array arguments are still the whole batch's):
 * lets the host pipeline the gradient of one group of utterances (HBM-bound) against the joint's dhid product
 * of the previous group (matrix-pipe-bound) on a second stream. */
int edgedict_rnnt_loss_backward_packed_range(const void* acts, int acts_dtype, void* grads,
                                             const int32_t* labels, const int32_t* act_lens,
                                             const int32_t* label_lens, const long long* row_offsets,
                                             int B, int T, int U1, int V, int blank, const void* workspace,
                                             float grad_scale_host, const float* grad_scale_dev,
                                             int grad_scale_stride, int b0, int nb, void* stream);
/* FastEmit (Yu et al. 2021): the four backward entry points above with `fastemit_lambda` behind their own arguments.
 * The gradient that flows through the label emissions is scaled by 1 + lambda:
 *   wb = exp(alpha + lp_blank + beta(t+1,u) - L),  wl = exp(alpha + lp_label + beta(t,u+1) - L)
 *   grad(t,u,k) = softmax_k (wb + (1 + lambda) wl) - [k == blank] wb - [k == labels[u]] (1 + lambda) wl
 * The COSTS of the forward call stay the plain negative log-likelihood (validation losses stay comparable across
 * lambdas); the workspace is the one any forward entry point filled.  lambda == 0 launches the kernels of the plain
 * entry points (bit-identical gradients and column sums); lambda < 0, NaN or infinite is ED_ERR_INVALID, reported
 * before anything is launched. */
int edgedict_rnnt_loss_backward_fe(const void* acts, int acts_dtype, void* grads, const int32_t* labels,
                                   const int32_t* act_lens, const int32_t* label_lens, int B, int T, int U1, int V,
                                   int blank, const void* workspace, float grad_scale_host,
                                   const float* grad_scale_dev, int grad_scale_stride, float fastemit_lambda,
                                   void* stream);
int edgedict_rnnt_loss_backward_packed_fe(const void* acts, int acts_dtype, void* grads, const int32_t* labels,
                                          const int32_t* act_lens, const int32_t* label_lens,
                                          const long long* row_offsets, int B, int T, int U1, int V, int blank,
                                          const void* workspace, float grad_scale_host, const float* grad_scale_dev,
                                          int grad_scale_stride, float fastemit_lambda, void* stream);
int edgedict_rnnt_loss_backward_packed_colsum_fe(const void* acts, int acts_dtype, void* grads, const int32_t* labels,
                                                 const int32_t* act_lens, const int32_t* label_lens,
                                                 const long long* row_offsets, int B, int T, int U1, int V, int blank,
                                                 const void* workspace, float grad_scale_host,
                                                 const float* grad_scale_dev, int grad_scale_stride,
                                                 float* colsum_parts, float fastemit_lambda, void* stream);
int edgedict_rnnt_loss_backward_packed_range_fe(const void* acts, int acts_dtype, void* grads, const int32_t* labels,
                                                const int32_t* act_lens, const int32_t* label_lens,
                                                const long long* row_offsets, int B, int T, int U1, int V, int blank,
                                                const void* workspace, float grad_scale_host,
                                                const float* grad_scale_dev, int grad_scale_stride, int b0, int nb,
                                                float fastemit_lambda, void* stream);
/* Forced alignment: the single best alignment of a KNOWN transcript (Viterbi over the lattice of the loss),
 *   v(t,u) = max(v(t-1,u) + lp_blank(t-1,u), v(t,u-1) + lp_label(t,u-1)),  score = v(T_b-1,U_b) + lp_blank(T_b-1,U_b).
 * Arguments as the forward entry points' (dense; packed; packed bf16 with the log-sum-exp partials), with
 *   frames  [B, U1-1] int32  out: frames[b][u] = frame on which label u of utterance b is emitted, -1 for u >= label_lens[b]
 *   scores  [B] fp32         out: log-probability of that alignment (<= -cost); -inf for an empty utterance (T_b <= 0,
 *                            whose frames are all -1)
 * in place of costs / reduced.  Lengths are clamped as the loss clamps them.  TIE RULE: where both predecessors of a
 * cell score equal, the path comes from the blank one (t - 1).  The workspace (same size and layout as the loss's) is
 * scratch: v lies where the alphas go, the beta plane is not written. */
int edgedict_rnnt_align(const void* acts, int acts_dtype, const int32_t* labels, const int32_t* act_lens,
                        const int32_t* label_lens, int B, int T, int U1, int V, int blank, int32_t* frames,
                        float* scores, void* workspace, void* stream);
int edgedict_rnnt_align_packed(const void* acts, int acts_dtype, const int32_t* labels, const int32_t* act_lens,
                               const int32_t* label_lens, const long long* row_offsets, int B, int T, int U1, int V,
                               int blank, int32_t* frames, float* scores, void* workspace, void* stream);
int edgedict_rnnt_align_packed_parts(const void* acts, const int32_t* labels, const int32_t* act_lens,
                                     const int32_t* label_lens, const long long* row_offsets, int B, int T, int U1,
                                     int V, int blank, int32_t* frames, float* scores, void* workspace,
                                     const float* lse_parts, int lse_slots, void* stream);
/* Alignment-restricted RNN-T loss (Ar-RNN-T, Mahadeokar et al. 2021): per-label emission windows.
 *   win_lo, win_hi  [B, U1-1] int32 (device): label u of utterance b may be emitted - the lattice step (t,u) -> (t,u+1) -
 *                   on the frames win_lo[b][u] <= t <= win_hi[b][u] only.  Entries with u >= label_lens[b] are ignored,
 *                   blank transitions are never restricted, values outside [0, T_b) match no frame.
 * cost_b = -log of the probability summed over the alignments that respect every window (windows that cover every frame:
 * the plain loss, bit for bit).  The *_ar forward entry points are the plain ones with the windows behind label_lens:
 * the first stage writes lp_label = -inf for the masked cells into the workspace, which is all the later stages see of
 * the windows.  With elo_u = max(lo_0..lo_u) and ehi_u = min(hi_u..hi_{U_b-1}, T_b-1), no alignment exists iff
 * elo_u > ehi_u for some u: then cost_b = +inf (and `reduced` = +inf), the gradient of utterance b is zero, nothing is
 * NaN and the other utterances are unaffected - decided on the device.  Null windows are ED_ERR_INVALID before anything
 * is launched (U1 == 1, no labels, excepted). */
int edgedict_rnnt_loss_forward_ar(const void* acts, int acts_dtype, const int32_t* labels, const int32_t* act_lens,
                                  const int32_t* label_lens, const int32_t* win_lo, const int32_t* win_hi, int B, int T,
                                  int U1, int V, int blank, float* costs, float* reduced, float reduce_scale,
                                  void* workspace, void* stream);
int edgedict_rnnt_loss_forward_packed_ar(const void* acts, int acts_dtype, const int32_t* labels,
                                         const int32_t* act_lens, const int32_t* label_lens, const int32_t* win_lo,
                                         const int32_t* win_hi, const long long* row_offsets, int B, int T, int U1, int V,
                                         int blank, float* costs, float* reduced, float reduce_scale, void* workspace,
                                         void* stream);
int edgedict_rnnt_loss_forward_packed_parts_ar(const void* acts, const int32_t* labels, const int32_t* act_lens,
                                               const int32_t* label_lens, const int32_t* win_lo, const int32_t* win_hi,
                                               const long long* row_offsets, int B, int T, int U1, int V, int blank,
                                               float* costs, float* reduced, float reduce_scale, void* workspace,
                                               const float* lse_parts, int lse_slots, void* stream);
/* Backward of a workspace an *_ar forward call filled; arguments as the *_fe entry points' (fastemit_lambda >= 0, 0 for
 * none).  With the restricted alpha, beta and L:
 *   grad(t,u,k) = softmax_k (wb + (1 + lambda) wl) - [k == blank] wb - [k == labels[u]] (1 + lambda) wl,
 * wl = 0 where the label is masked; a cell with alpha = -inf or beta = -inf (no window-respecting alignment passes
 * through it) gets an all-zero row and its logits are not read.  Takes no windows: they are in the workspace. */
int edgedict_rnnt_loss_backward_ar(const void* acts, int acts_dtype, void* grads, const int32_t* labels,
                                   const int32_t* act_lens, const int32_t* label_lens, int B, int T, int U1, int V,
                                   int blank, const void* workspace, float grad_scale_host,
                                   const float* grad_scale_dev, int grad_scale_stride, float fastemit_lambda,
                                   void* stream);
int edgedict_rnnt_loss_backward_packed_ar(const void* acts, int acts_dtype, void* grads, const int32_t* labels,
                                          const int32_t* act_lens, const int32_t* label_lens,
                                          const long long* row_offsets, int B, int T, int U1, int V, int blank,
                                          const void* workspace, float grad_scale_host, const float* grad_scale_dev,
                                          int grad_scale_stride, float fastemit_lambda, void* stream);
int edgedict_rnnt_loss_backward_packed_colsum_ar(const void* acts, int acts_dtype, void* grads, const int32_t* labels,
                                                 const int32_t* act_lens, const int32_t* label_lens,
                                                 const long long* row_offsets, int B, int T, int U1, int V, int blank,
                                                 const void* workspace, float grad_scale_host,
                                                 const float* grad_scale_dev, int grad_scale_stride,
                                                 float* colsum_parts, float fastemit_lambda, void* stream);
int edgedict_rnnt_loss_backward_packed_range_ar(const void* acts, int acts_dtype, void* grads, const int32_t* labels,
                                                const int32_t* act_lens, const int32_t* label_lens,
                                                const long long* row_offsets, int B, int T, int U1, int V, int blank,
                                                const void* workspace, float grad_scale_host,
                                                const float* grad_scale_dev, int grad_scale_stride, int b0, int nb,
                                                float fastemit_lambda, void* stream);
/* The forced aligner under windows: the best alignment among those that respect them.  Windows that admit none give
 * score -inf and a frames row of all -1. */
int edgedict_rnnt_align_ar(const void* acts, int acts_dtype, const int32_t* labels, const int32_t* act_lens,
                           const int32_t* label_lens, const int32_t* win_lo, const int32_t* win_hi, int B, int T, int U1,
                           int V, int blank, int32_t* frames, float* scores, void* workspace, void* stream);
int edgedict_rnnt_align_packed_ar(const void* acts, int acts_dtype, const int32_t* labels, const int32_t* act_lens,
                                  const int32_t* label_lens, const int32_t* win_lo, const int32_t* win_hi,
                                  const long long* row_offsets, int B, int T, int U1, int V, int blank, int32_t* frames,
                                  float* scores, void* workspace, void* stream);
int edgedict_rnnt_align_packed_parts_ar(const void* acts, const int32_t* labels, const int32_t* act_lens,
                                        const int32_t* label_lens, const int32_t* win_lo, const int32_t* win_hi,
                                        const long long* row_offsets, int B, int T, int U1, int V, int blank,
                                        int32_t* frames, float* scores, void* workspace, const float* lse_parts,
                                        int lse_slots, void* stream);
/* Windows around the frames of an alignment (frames [B, U] int32 as the aligner writes them), left, right >= 0:
 * win_lo = max(0, f - left), win_hi = min(T_b - 1, f + right); for u >= label_lens[b]: win_lo = 0, win_hi = T - 1.
 * T = 0 stands for the largest act_lens of the batch (found on the device). */
int edgedict_rnnt_alignment_windows(const int32_t* frames, const int32_t* act_lens, const int32_t* label_lens, int B,
                                    int T, int U, int left, int right, int32_t* win_lo, int32_t* win_hi, void* stream);
/* The live cells of the restricted lattice (finite alpha and finite beta) from the windows alone: column u is alive on
 * the frames [elo_{u-1}, ehi_u] (column 0 from frame 0, column U_b up to frame T_b - 1).
 *   band   [B, T, 2] int32  out: (first, last) live label column of each frame; (0, -1) where the frame has none
 *   cells  [B] int64        out: live cells of the utterance (0 where the windows admit no alignment)
 * U1 <= 2048. */
int edgedict_rnnt_band(const int32_t* win_lo, const int32_t* win_hi, const int32_t* act_lens, const int32_t* label_lens,
                       int B, int T, int U1, int32_t* band, long long* cells, void* stream);
/* ---- band-packed lattice: joint + loss on the live cells of the band table only (edgedict_rnnt_band).
 * Band row of a live cell: row(b,t,u) = row_off[b][t] + (u - ulo[b][t]), ulo <= u <= uhi; rows of a frame, frames of an
 * utterance and utterances follow each other; an utterance without an alignment owns no rows.
 *   edgedict_rnnt_band_offsets: row_off [B, T] int64 out = exclusive prefix sum of the widths max(0, uhi - ulo + 1) in
 *                               (b, t) order; total [1] int64 out = M_band (= sum of cells)
 *   edgedict_rnnt_band_rows:    row_tu [rows] int32 out = t << 16 | u of every band row (T, U1 < 65536) */
int edgedict_rnnt_band_offsets(const int32_t* band, const long long* cells, int B, int T, long long* row_off,
                               long long* total, void* stream);
int edgedict_rnnt_band_rows(const int32_t* band, const long long* row_off, int B, int T, int U1, long long rows,
                            int32_t* row_tu, void* stream);
/* The *_packed_ar forward entry points with acts (and lse_parts) on band rows [M_band, .].  Every cell of the boxes
 * gets its workspace planes: a live cell exactly as the *_ar kernels form them, a dead cell lp_blank = lp_label = -inf
 * and denominator 0; alpha and beta on live cells, the likelihoods and the costs are the *_packed_ar path's. */
int edgedict_rnnt_loss_forward_band(const void* acts, int acts_dtype, const int32_t* labels, const int32_t* act_lens,
                                    const int32_t* label_lens, const int32_t* win_lo, const int32_t* win_hi,
                                    const int32_t* band, const long long* row_off, const int32_t* row_tu,
                                    const long long* cells, int B, int T, int U1, int V, int blank, float* costs,
                                    float* reduced, float reduce_scale, void* workspace, void* stream);
int edgedict_rnnt_loss_forward_band_parts(const void* acts, const int32_t* labels, const int32_t* act_lens,
                                          const int32_t* label_lens, const int32_t* win_lo, const int32_t* win_hi,
                                          const int32_t* band, const long long* row_off, const int32_t* row_tu,
                                          const long long* cells, int B, int T, int U1, int V, int blank, float* costs,
                                          float* reduced, float reduce_scale, void* workspace, const float* lse_parts,
                                          int lse_slots, void* stream);
/* Backward of a workspace a *_band forward call filled: acts and grads on band rows, every row a live cell (the live-cell
 * arithmetic of the *_ar kernels; no zero rows exist).  The colsum form writes all
 * edgedict_rnnt_grad_colsum_rows(...) partial rows, zeros where a workgroup had no rows. */
int edgedict_rnnt_loss_backward_band(const void* acts, int acts_dtype, void* grads, const int32_t* labels,
                                     const int32_t* act_lens, const int32_t* label_lens, const long long* row_off,
                                     const int32_t* row_tu, const long long* cells, int B, int T, int U1, int V, int blank,
                                     const void* workspace, float grad_scale_host, const float* grad_scale_dev,
                                     int grad_scale_stride, float fastemit_lambda, void* stream);
int edgedict_rnnt_loss_backward_band_colsum(const void* acts, int acts_dtype, void* grads, const int32_t* labels,
                                            const int32_t* act_lens, const int32_t* label_lens, const long long* row_off,
                                            const int32_t* row_tu, const long long* cells, int B, int T, int U1, int V,
                                            int blank, const void* workspace, float grad_scale_host,
                                            const float* grad_scale_dev, int grad_scale_stride, float* colsum_parts,
                                            float fastemit_lambda, void* stream);
/* debug / test accessors into a filled workspace (device pointers):
 * which: 0 = log-softmax denominators f32[B,T,U1], 1 = alphas f64[B,T,U1], 2 = betas f64,
 * 3 = log-likelihoods f64[B,2] (alpha-side, beta-side), 4 = lp_blank f32[B,T,U1], 5 = lp_label */
const void* edgedict_rnnt_workspace_view(const void* workspace, int B, int T, int U1, int which);

/* ------------------------------------------------------------------------------------
 * Dense product on the matrix cores:  C[M,N] (+)= A[M,K] * B[N,K]^T + bias1[N] + bias2[N].
 * Replaces the cuBLAS/cuDNN GEMMs behind nn.Linear / nn.LSTM input products
 * (rnnt/models.py:45-46,65,129,135,148,156,165-167) and their autograd transposes.
 *   x_kmajor = 1: element (row,k) at p[row*ld + k];  x_kmajor = 0: at p[k*ld + row]
 *   dtype_in : ED_BF16 (v_mfma_f32_16x16x32_bf16) or ED_F32 (exact v_mfma_f32_16x16x4_f32)
 *   dtype_out: ED_F32 or (bf16 inputs only) ED_BF16; accumulation is always fp32
 *   bias1/bias2: nullable fp32 [N];  accumulate != 0: C += ...;
 *   split_k > 1: K is partitioned over workgroups and combined with fp32 atomics
 *                (fp32 output only; used for weight gradients whose M*N is small and K huge)
 */
int edgedict_gemm(int dtype_in, int dtype_out, const void* A, long long lda, int a_kmajor,
                  const void* B, long long ldb, int b_kmajor, void* C, long long ldc, int M, int N,
                  int K, const float* bias1, const float* bias2, int accumulate, int split_k,
                  void* stream);

/* Background variant for products that are OFF the critical path (weight gradients) and run on a
 * side stream next to latency-bound kernels.  Identical arithmetic, three scheduling differences:
 *   - every workgroup claims enough extra LDS that at most max_wg_per_cu are resident per CU, and
 *     only as many workgroups are launched as are resident at once (each walks its work items): a
 *     long-lived GEMM can neither fill a CU nor park a tail of workgroups in the dispatcher;
 *   - with `partials` (fp32 [P][M][N], P = smallest power of two >= split_k, at most 8) the K
 *     slices are written ONCE, at the end of each workgroup, with plain stores and summed by a
 *     small reduce kernel - no atomics, no dirty lines while the main loop runs.  Measured on
 *     MI355X (tools/boundary_probe.hip): a concurrent kernel that streams writes / fp32 atomics
 *     raises every dependent kernel boundary on the other streams from 2.4 us to 10 / 8-32 us
 *     (the end-of-kernel L2 write-back has to flush everybody's dirty lines); reads cost nothing. */
int edgedict_gemm_bg(int dtype_in, int dtype_out, const void* A, long long lda, int a_kmajor,
                     const void* B, long long ldb, int b_kmajor, void* C, long long ldc, int M,
                     int N, int K, const float* bias1, const float* bias2, int accumulate,
                     int split_k, int max_wg_per_cu, float* partials, void* stream);

/* C[M,N] = A[M,K] B[N,K]^T + bias (bf16, both operands K-contiguous: the joint's logits product,
 * rnnt/models.py:177) with the log-softmax partials of every row fused into the epilogue:
 * lse_part [M][ceil(N/64)][2] fp32 = (max, sum exp(x - max)) of the bf16-rounded outputs over 64-column
 * slots - edgedict_rnnt_loss_forward_packed_parts finishes the denominators from them instead of
 * re-reading the M x N logits.  K %% 64 == 0, K >= 128, N %% 8 == 0. */
int edgedict_gemm_nt_lse(const void* A, long long lda, const void* B, long long ldb, void* C,
                         long long ldc, int M, int N, int K, const float* bias, float* lse_part,
                         void* stream);

/* DRY RUN of the three entry points above (and of the encoder stack's internal quiet products): which kernel a product
 * would run, with which launch - nothing is launched, no pointer is dereferenced (only alignment and nullness count) and
 * no device is needed (without one the plan assumes 256 compute units).  Arguments as edgedict_gemm_bg, with
 *   max_wg_per_cu = 0 : the plan of edgedict_gemm
 *   lse != 0          : the plan of edgedict_gemm_nt_lse (bf16 K-contiguous operands, bias1 = its bias)
 *   unreduced != 0    : the internal quiet form that leaves its K slices in `partials` (C = partials, ldc = N)
 * record [ED_GEMM_PLAN_WORDS] int32 out:
 *   [0] kernel id   0 none (empty product)
 *                   1 / 2 gemm_kernel<bf16, bf16> plain / FAST (vector loads without guards), 3 / 4 <bf16, f32>,
 *                   5 / 6 <f32, f32> (gemm.hip; the layout pair of the call picks one of four instantiations)
 *                   7 gemm_nt_kernel<64,64,32>, 8 <128,128,64>, 9 <256,128,64>, 10 gemm_nt_ring64_kernel (gemm_nt.hip)
 *                   11 gemm_nt256_kernel, 12 gemm_nt256r_kernel<false>, 13 gemm_nt256r_kernel<true> (log-sum-exp)
 *                   14 gemm_tn256_kernel
 *   [1] grid (workgroups)   [2] block (threads)   [3] dynamic LDS bytes
 *   [4] K slices that run (1: K is not split)      [5] K per slice (0 for the kernels that never split K)
 *   [6] 1: a zero pass precedes (atomic split-K into a fresh C)   [7] 1: the reduce pass over `partials` follows
 *   [8] vendor route tried first where the library has the bridge (the kernel above runs when it declines):
 *       0 none, 1 large short-K bf16 NT (the joint's logits), 2 small long-K bf16 NT, 3 bf16 TN with fp32 output
 * Returns what the entry point would return for arguments it rejects. */
#define ED_GEMM_PLAN_WORDS 9
int edgedict_gemm_plan(int dtype_in, int dtype_out, const void* A, long long lda, int a_kmajor,
                       const void* B, long long ldb, int b_kmajor, void* C, long long ldc, int M, int N,
                       int K, const float* bias1, const float* bias2, int accumulate, int split_k,
                       int max_wg_per_cu, float* partials, int lse, int unreduced, int32_t* record);


/* ------------------------------------------------------------------------------------
 * LayerNorm fused with the residual add and the encoder's TimeReduction.
 * Replaces nn.LayerNorm at rnnt/models.py:124,132 and the per-layer
 * `xs = xs + lstm(xs); xs = Sequential(LayerNorm[, TimeReduction])(xs)` at rnnt/models.py:47-53,
 * 66-70 with TimeReduction.forward rnnt/models.py:21-29 (zero-pad AFTER the norm, pair mean).
 *   x, res (nullable)  [B,T,D] dtype;  s = x + res is what gets normalised
 *   y                  [B, ceil(T/reduce), D] dtype;  reduce in {1,2}
 *   mean, rstd         fp32 [B*T] saved for backward
 * backward: ds [B,T,D] dtype (gradient wrt x AND wrt res), dgamma/dbeta fp32 [D] are ACCUMULATED
 * (atomic +=), pass NULL to skip.
 */
int edgedict_layernorm_fwd(int dtype, const void* x, const void* res, const float* gamma,
                           const float* beta, void* y, float* mean, float* rstd, int B, int T,
                           int D, int reduce, float eps, void* stream);
int edgedict_layernorm_bwd(int dtype, const void* dout, const void* x, const void* res,
                           const float* gamma, const float* mean, const float* rstd, void* ds,
                           float* dgamma, float* dbeta, int B, int T, int D, int reduce,
                           void* stream);

/* ------------------------------------------------------------------------------------
 * LSTM time recurrence.  Replaces the cuDNN RNN behind nn.LSTM (rnnt/models.py:45-46,65 encoder
 * layers; rnnt/models.py:145-147,155 prediction network).  PyTorch gate order i,f,g,o.
 * forward:
 *   G      [B,T,4H] dtype  in : X*W_ih^T + b_ih + b_hh (from edgedict_gemm)
 *                          out: post-activation gates i,f,g,o (saved for backward, in place)
 *   Hprev  [B,T,H]  dtype  out: h_{t-1} per step (row t=0 <- h0); operand of dW_hh later
 *   Y      [B,T,H]  dtype  out: h_t
 *   Cst    [B,T,H]  fp32   out: c_t
 *   Whh    [4H,H]   dtype;  h0,c0 fp32 [B,H] nullable (= zeros);  hN,cN fp32 [B,H] nullable
 * backward (after forward, same buffers):
 *   dY     [B,T,H]  dtype  gradient wrt h_t (nullable = zeros)
 *   G                     in : saved gates;  out: dL/d(pre-activations) for every t (in place)
 *   WhhT   [H,4H]   dtype  (edgedict_transpose of Whh);  dC_ws fp32 [B,H] scratch
 * One kernel launch per timestep (kernel boundary ~1.5us < any grid barrier on MI355X).
 * Limits: H % 8 == 0.  Gradients wrt (h0,c0) are not produced.
 *
 * bf16 fast path (H % 32 == 0): pass the fragment-order weight image built by
 * edgedict_lstm_pack_weights (packed_fwd for forward, packed_bwd for backward; each 4H*H bf16,
 * rebuilt whenever W_hh changes) and a workspace of edgedict_lstm_workspace_bytes(dtype,B,H)
 * bytes (ping-pong fragment images of h_t / dG_t); the plain Whh / WhhT may then be NULL.
 * With NULL packed weights or workspace the generic path runs (any dtype).
 */
size_t edgedict_lstm_workspace_bytes(int dtype, int B, int H);
int edgedict_lstm_pack_weights(int src_dtype, const void* Whh, void* packed_fwd, void* packed_bwd,
                               int H, void* stream);
int edgedict_lstm_forward(int dtype, void* G, void* Hprev, void* Y, float* Cst, const void* Whh,
                          const void* Whh_packed, const float* h0, const float* c0, float* hN,
                          float* cN, int B, int T, int H, void* ws, void* stream);
int edgedict_lstm_backward(int dtype, void* G, const void* dY, const float* Cst, const float* c0,
                           const void* WhhT, const void* WhhT_packed, float* dC_ws, int B, int T,
                           int H, void* ws, void* stream);

/* ------------------------------------------------------------------------------------
 * Layer-pipelined LSTM encoder stack (bf16).  One call per direction replaces the whole of
 * Encoder.forward's LayerNorm + ResLayerNormLSTM.forward (rnnt/models.py:55-75,124,131-134:
 * per layer nn.LSTM, residual add for layers > 0, LayerNorm, optional TimeReduction
 * rnnt/models.py:21-29) and its autograd.  The layers run as a skewed wavefront: one launch
 * carries a time step of every runnable layer, the input products are chunked GEMMs on an
 * internal side stream, weight gradients overlap the BPTT of the layers below
 * (csrc/encoder_stack.hip).  The caller's stream is forked at entry and joined at exit.
 *
 * Layouts (all device memory, owned by the caller, kept from forward to backward):
 *   activations are TIME-MAJOR;  gate columns of G are interleaved: column of (gate g, unit j)
 *   = (j/16)*64 + g*16 + j%16  (gate order i,f,g,o);  weight images come from
 *   edgedict_stack_pack_weights (rebuilt whenever the fp32 master weights change).
 * Limits: H % 32 == 0, H <= 2048, L <= 8, reduce in {1,2}, residual layers need I == H.
 * The library keeps its internal streams (recurrence, chunk GEMMs, weight gradients)
 * and an event pool per device (created on first use).
 */
typedef struct edgedict_stack_layer {
    int T;                 /* time steps of this layer */
    int I;                 /* input width */
    int reduce;            /* time reduction after this layer's LayerNorm: 1 or 2 */
    int residual;          /* LayerNorm(y + x) instead of LayerNorm(y) */
    const void* wih_p;     /* bf16 [4H, I]  rows in interleaved gate order */
    const void* wih_t;     /* bf16 [I, 4H]  its transpose (K-contiguous operand of the dX product); backward only */
    const float* bias_p;   /* f32  [4H]     b_ih + b_hh, interleaved */
    const void* whh_f;     /* bf16 forward fragment image of W_hh (4H*H) */
    const void* whh_b;     /* bf16 backward fragment image of W_hh (4H*H); backward only */
    const float* ln_gamma; /* f32 [H] */
    const float* ln_beta;  /* f32 [H] */
    void* X;               /* bf16 [T, B, I]    layer input (layer 0: written by the input LayerNorm) */
    void* G;               /* bf16 [T, B, 4H]   gates after forward, dL/d(pre-activation) after backward */
    void* Yx;              /* bf16 [T+1, B, H]  row 0 = h0, row t+1 = h_t */
    float* Cx;             /* f32  [T+1, B, H]  row 0 = c0, row t+1 = c_t */
    float* mean;           /* f32  [T, B] LayerNorm statistics */
    float* rstd;
    /* backward only */
    void* dZ;              /* bf16 [T, B, H] dL/d(LayerNorm input) = dL/dh_t from above */
    void* dX;              /* bf16 [T, B, I] dL/d(layer input); pass dZ itself for residual layers
                              (the product is accumulated in place); unused for layer 0 */
    float* dW_ih;          /* f32 [4H, I] out, natural gate order */
    float* dW_hh;          /* f32 [4H, H] out */
    float* db;             /* f32 [4H] out (gradient of b_ih and of b_hh) */
    float* db_hh;          /* nullable second destination of the same values (b_hh.grad when accumulating) */
    float* dgamma;         /* f32 [H] ACCUMULATED (+=): zero before the call */
    float* dbeta;
    const void* whh_s;     /* bf16 split-K fragment image of W_hh (edgedict_stack_pack_sk), nullable: with it (and B <= 64,
                              H % 64 == 0, H <= 1024, EDGEDICT_STACK_BWD_SK != 0) the BPTT runs on the split-K
                              weights-stationary kernel, several steps per launch; without it one launch per step */
    /* nn.Dropout behind this layer's LayerNorm (+ TimeReduction), rnnt/models.py:47-53,70 - training mode only, the
       caller passes 0 in eval mode: element (b, tau, j) of the layer's [B, ceil(T / reduce), H] output is zeroed with
       probability drop_p and scaled by 1 / (1 - drop_p) otherwise; the mask is the counter-based one of
       edgedict_dropout (same hash, same batch-first element index, drop_seed), regenerated in the backward pass */
    float drop_p;
    unsigned drop_seed;
} edgedict_stack_layer_t;

#define EDGEDICT_STACK_SERIAL 1     /* run everything on the caller's stream (debug / bit-exact check) */
#define EDGEDICT_STACK_DW_AT_END 2  /* weight gradients after the BPTT instead of under it */
#define EDGEDICT_STACK_ACCUM_GRADS 8 /* dW_ih / dW_hh / db / db_hh are existing gradient buffers: += instead of = */
#define EDGEDICT_STACK_INFERENCE 64 /* no backward pass will follow this forward: the workspace carries no dG images /
   split-K partials (edgedict_stack_workspace_bytes is smaller), edgedict_stack_backward refuses the descriptor */
#define EDGEDICT_STACK_SIDE_STREAM_PER_LAYER 4 /* experiment: chunk GEMMs on one side stream PER LAYER.
   Measured 2x SLOWER end to end: more streams than hardware queues serialises everything. */

typedef struct edgedict_stack_desc {
    int B, H, L;
    int chunk;             /* frames (at the stack's output rate) per input-product chunk */
    int lag;               /* launches between consecutive layers; 0 = chunk*f0 + 5 */
    int split_k;           /* K slices of the (quiet) weight-gradient products: 1, 2, 4 or 8; 0 = 2 */
    int flags;
    float eps;
    const edgedict_stack_layer_t* layers;   /* HOST array [L] */
    const void* x;         /* [B, T0, I0] batch-first encoder input, x_dtype (ED_F32 / ED_BF16) */
    int x_dtype, T0, I0;
    const float* in_gamma; /* f32 [I0] input LayerNorm */
    const float* in_beta;
    float* in_mean;        /* f32 [B*T0] */
    float* in_rstd;
    const float* h0;       /* f32 [L, B, H] nullable (= zeros) */
    const float* c0;
    void* out;             /* bf16 [B, T_out, H] batch-first stack output */
    const void* dout;      /* backward: bf16 [B, T_out, H] */
    float* d_in_gamma;     /* backward: f32 [I0] ACCUMULATED */
    float* d_in_beta;
    void* ws;              /* edgedict_stack_workspace_bytes(desc) bytes, 256-byte aligned */
    size_t ws_bytes;
    /* backward, optional: called on the HOST, synchronously from edgedict_stack_backward, as soon as the
       LAST kernel that accumulates dW_ih / dW_hh / db of `layer` has been enqueued on the auxiliary
       stream (edgedict_aux_stream(2)) - the layers finish top-down, layer L-1 roughly L-1 chunks of
       launches before layer 0.  A data-parallel host orders that layer's gradient all-reduce behind
       the auxiliary stream's position at that moment, so the exchange of layers L-1 .. 1 runs under
       the BPTT of the layers below (reference: DDP's bucketed all-reduce, cli/lightning.py:325-331).
       The callback must not call back into this library. */
    void (*grads_final)(int layer, void* user);
    void* grads_final_user;
} edgedict_stack_desc_t;

/* sizeof(edgedict_stack_layer_t) (which = 0) / sizeof(edgedict_stack_desc_t) (which = 1): lets a
 * foreign-language binding verify its struct mirror */
size_t edgedict_stack_struct_bytes(int which);
/* The library's internal streams of the current device (0 = recurrence, 1 = chunk GEMMs, 2 = the
 * low-priority weight-gradient stream), created on first use.  Host code that wants to run its
 * own off-critical-path work (e.g. the joint network's weight gradients) concurrently should
 * borrow stream 2 instead of creating more streams: beyond the 4 hardware queues HIP multiplexes
 * streams and every cross-stream dependency gets slower. */
void* edgedict_aux_stream(int which);
/* Debug / test aid: which internal streams of the current device still have work enqueued (hipStreamQuery; bit 0
 * recurrence, bit 1 chunk GEMMs, bit 2 auxiliary, bits 3.. lazily created per-layer side streams).  Every entry
 * point joins the streams it used into the caller's stream before it returns, so with the CALLER's stream idle a
 * set bit is work nothing is ordered behind (tests/conftest.py asserts mask == 0 after every GPU test).  Creates
 * nothing. */
int edgedict_streams_busy(unsigned* mask);
size_t edgedict_stack_workspace_bytes(const edgedict_stack_desc_t* desc);
/* fp32 master weights of one layer (nn.LSTM's weight_ih_l0 [4H, I], weight_hh_l0 [4H, H], biases [4H]) -> the bf16
 * images edgedict_stack_layer_t points at.  Every output is optional (null = skip): wih_p (+ bias_p, needs b_ih / b_hh)
 * and whh_f are what the forward pass reads; wih_t, whh_b (and edgedict_stack_pack_sk's image) only the backward pass -
 * a trainer rebuilds the first group in front of the next forward pass and the second behind it. */
int edgedict_stack_pack_weights(const float* w_ih, const float* w_hh, const float* b_ih,
                                const float* b_hh, int H, int I, void* wih_p, void* wih_t,
                                float* bias_p, void* whh_f, void* whh_b, void* stream);
/* W_hh [4H, H] f32 (H % 64 == 0, H <= 1024) -> bf16 split-K image for the weights-stationary BPTT kernel
 * (edgedict_stack_layer_t.whh_s, 4H*H elements): workgroup (unit block of 64, quarter of the 4H interleaved gate
 * columns) keeps its 128 KB in registers for a whole launch */
int edgedict_stack_pack_sk(const float* w_hh, int H, void* whh_s, void* stream);
/* give-up code of the last encoder-stack launch on the current device that ran into one of its bounded
 * in-kernel waits (0 = none since the last call of this function; reading clears it): 5xx / 6xx a chunk flag of
 * the forward / backward pass, 7xx a peer of the launch-persistent forward, 8xx a side stream's counter wait,
 * 9xx a peer of the split-K BPTT (csrc/stack_kernels.hip) */
int edgedict_stack_wsr_error(void);
/* the 3 give-up words behind edgedict_stack_wsr_error of the current device (pinned, mapped host memory):
 * host = 0 -> the DEVICE-visible address (what edgedict_adam_step_guarded takes as skip_words, n_skip = 3),
 * host = 1 -> the host address of the same words (tests poke it).  NULL on failure. */
void* edgedict_stack_error_words(int host);
/* debug: a zeroed device buffer of >= 8 x 8 int64 in which the first workgroup of every layer of the
 * launch-persistent forward / split-K BPTT launches accumulates the 100 MHz ticks it spent per phase
 * (tools/lpw_trace.py, tools/sk_trace.py); NULL switches it off.  Not part of the hot path. */
int edgedict_stack_wsr_set_trace(void* device_buffer);
int edgedict_stack_forward(const edgedict_stack_desc_t* desc, void* stream);
/* measurement aid: HIP-event time (on the recurrence stream) from the first to the last wavefront
 * launch of the most recent forward (backward = 0) or backward (1) call on this device, and the
 * number of launches in it; blocks until that call's launches have executed. */
int edgedict_stack_last_timing(int backward, float* ms, int* launches);
/* which recurrence kernel the most recent forward (backward = 0) / backward (1) call on this device ran:
 * kind 0 = one launch per time step (stack_fwd_kernel / stack_bwd_kernel), 1 = launch-persistent forward
 * (stack_fwd_lpw_kernel), 2 = split-K weights-stationary BPTT (stack_bwd_sk_kernel); steps_per_launch =
 * consecutive time steps of a layer one launch carries (0 for kind 0). */
int edgedict_stack_last_mode(int backward, int* kind, int* steps_per_launch);
/* measurement aid, opt-in: with on != 0 every wavefront launch of the following forward / backward calls on
 * this device stamps its first workgroup's start and its last workgroup's end (constant 100 MHz clock) into
 * an internal device buffer (64 KB per direction, allocated on first use).  edgedict_stack_launch_times then
 * returns the SUM of the launches' own durations of the most recent call and their number: the kernels'
 * average duration as a profiler's begin/end timestamps see it, without the gaps between dependent launches
 * that edgedict_stack_last_timing's span includes.  The two atomics per workgroup cost time: switch it off
 * for timed runs. */
int edgedict_stack_time_launches(int on);
int edgedict_stack_launch_times(int backward, float* sum_ms, int* launches);
/* debug / profiling: the raw stamps behind edgedict_stack_launch_times - out[2 k] = first workgroup's start,
 * out[2 k + 1] = last workgroup's end of wavefront launch k of the last call (100 MHz ticks), in issue order;
 * synchronises the device.  tools/lpw_timeline.py */
int edgedict_stack_launch_stamps(int backward, unsigned long long* out, int max_launches, int* launches);
/* Dry run of the scheduler (no device needed, nothing is launched; buffer pointers in the descriptor
 * only have to be non-NULL): the launch index that carries every layer-step and the number of
 * launches issued when each chunk's side-stream product was enqueued.
 *   step_launch     HOST int32 [sum_l T_l], layer-major, frame t of layer l at offset(l) + t
 *   chunk_enqueued  HOST int32 [sum_l nchunks_l], nchunks_l = ceil(T_l / (chunk * f_l)); -1 = from the start
 *   n_launches, max_slots  HOST int32: launches of the step kernel, most layer-steps in one launch */
int edgedict_stack_schedule(const edgedict_stack_desc_t* d, int backward, int32_t* step_launch,
                            int32_t* chunk_enqueued, int32_t* n_launches, int32_t* max_slots);
/* dry run of the backward pass that reports WHAT is enqueued, in enqueue order: quadruples (kind, layer, arg, stream) of
 * HOST int32, the first `capacity` of them written to `events`, their number to *n_events.  kind: 1 a BPTT launch (arg =
 * its index), 2 a LayerNorm-backward chunk that writes layer `layer`'s partial rows (arg = chunk), 3 layer's LayerNorm
 * parameter sum, 4 a weight-gradient product with its un-permute (arg 0 = dW_ih, 1 = dW_hh), 5 layer's bias gradient
 * (column sum + un-permute), 6 the grads_final callback of the layer, 7 the layer-0 dX product, 8 the input norm's
 * parameter gradient, 9 the end of the pass.  stream: 0 recurrence, 1 side, 2 weight-gradient stream.  layer = -1 where
 * none applies.  d->grads_final is called as in edgedict_stack_schedule. */
int edgedict_stack_schedule_events(const edgedict_stack_desc_t* d, int32_t* events, int capacity, int32_t* n_events);
/* EDGEDICT_STACK_TAIL (read once from the environment; on unless it is 0): on, the bias column sums of layers 1 and 0 run
 * on the side stream beside those layers' weight-gradient products, not behind them in the serial chain the caller waits
 * for after the last BPTT launch (the weight-gradient stream joins them before grads_final fires) - for a layer whose
 * weight gradients are issued in one call; a layer issued in segments keeps its bias updates in order on the
 * weight-gradient stream.  0 enqueues everything where it was before.  No kernel, no input and the order of no gradient's
 * updates changes.
 * edgedict_stack_tail_mode(on >= 0) overrides the environment for the process (0 off, else on: tests and tools compare
 * both settings in one process), (-1) drops the override, any other value only queries; returns 1 or 0, the setting in
 * effect.  A backward call reads the setting once, when it starts. */
int edgedict_stack_tail_mode(int bits);
int edgedict_stack_backward(const edgedict_stack_desc_t* desc, void* stream);

/* ------------------------------------------------------------------------------------
 * Streaming helpers.
 * cast / transpose: weight copies in the compute dtype (fp32 master -> bf16), dst[c][r]=src[r][c].
 * colsum: out[n] += sum_m x[m*ld+n]  (bias gradients; ATOMIC accumulate into fp32 out).
 * embedding: nn.Embedding(V,E,padding_idx=PAD) lookup with the BOS left-pad of
 *            Decoder.forward (rnnt/models.py:150-153) folded in; backward scatters with atomics
 *            and skips the padding row.
 * joint_hidden: hid[b,t,u,:] = tanh(E1[b,t,:] + D1[b,u,:])  (Joint.forward rnnt/models.py:169-179
 *            with the first Linear split over [enc;dec]); backward returns fp32
 *            dE1[B,T,J] = sum_u dpre, dD1[B,U1,J] = sum_t dpre with dpre = dhid*(1-hid^2).
 */
int edgedict_cast(int src_dtype, const void* src, int dst_dtype, void* dst, long long n,
                  void* stream);
int edgedict_transpose(int src_dtype, const void* src, int dst_dtype, void* dst, int R, int C,
                       void* stream);
int edgedict_colsum(int dtype, const void* x, long long ld, float* out, long long M, int N,
                    void* stream);
int edgedict_embedding_fwd(int out_dtype, int emb_dtype, const int32_t* tokens, int tok_stride,
                           const void* emb, void* out, int B, int Uout, int E, int V,
                           int prepend_bos, int bos, void* stream);
int edgedict_embedding_bwd(int dtype, const int32_t* tokens, int tok_stride, const void* dout,
                           float* demb, int B, int Uout, int E, int V, int prepend_bos, int bos,
                           int pad, void* stream);
/* dropout: y[i] = x[i] * keep(seed, i) / (1-p) with a counter-based mask (nn.Dropout /
 *          nn.LSTM(dropout=p) in training mode, rnnt/models.py:47-53,145-147); the backward pass is
 *          the same call on the incoming gradient with the same seed.  x == y is allowed.
 * spec_mask: zero-fill the SpecAugment time / frequency intervals (TimeMasking / FrequencyMasking,
 *          rnnt/transforms.py:54-146, applied after frame stacking) of a resident feature batch
 *          x fp32 [B,T,F]; t_iv int32 [B][n_t][2], f_iv int32 [B][n_f][2] = half-open [start,end)
 *          intervals over the frame index / the stacked feature index. */
int edgedict_dropout(int dtype, const void* x, void* y, long long n, float p, unsigned seed,
                     void* stream);
int edgedict_spec_mask(float* x, int B, int T, int F, const int32_t* t_iv, int n_t,
                       const int32_t* f_iv, int n_f, void* stream);
int edgedict_joint_hidden_fwd(int dtype, const void* E1, const void* D1, void* hid, int B, int T,
                              int U1, int J, void* stream);
int edgedict_joint_hidden_bwd(int dtype, const void* dhid, const void* hid, float* dE1,
                              float* dD1, int B, int T, int U1, int J, void* stream);
/* packed-lattice forms (see edgedict_rnnt_loss_forward_packed): hid / dhid hold only valid cells;
 * dE1 rows t >= act_lens[b] and dD1 rows u > label_lens[b] come out as zeros. */
int edgedict_joint_hidden_fwd_packed(int dtype, const void* E1, const void* D1, void* hid,
                                     const int32_t* act_lens, const int32_t* label_lens,
                                     const long long* row_offsets, int B, int T, int U1, int J,
                                     void* stream);
int edgedict_joint_hidden_bwd_packed(int dtype, const void* dhid, const void* hid, float* dE1,
                                     float* dD1, const int32_t* act_lens, const int32_t* label_lens,
                                     const long long* row_offsets, int B, int T, int U1, int J,
                                     void* stream);
/* band-packed forms (see edgedict_rnnt_band_offsets): hid / dhid hold the `rows` live cells only; dE1 rows of frames
 * without a live cell and dD1 rows of columns that are never alive come out as zeros. */
int edgedict_joint_hidden_fwd_band(int dtype, const void* E1, const void* D1, void* hid, const int32_t* band,
                                   const long long* row_off, long long rows, int B, int T, int U1, int J, void* stream);
int edgedict_joint_hidden_bwd_band(int dtype, const void* dhid, const void* hid, float* dE1, float* dD1,
                                   const int32_t* band, const long long* row_off, long long rows, int B, int T, int U1,
                                   int J, void* stream);

/* ------------------------------------------------------------------------------------
 * Optimiser step on flat fp32 buffers (torch.optim.Adam semantics, cli/train.py:135-146,268)
 * and the global-norm clip coefficient of clip_grad_norm_ (cli/train.py:262-267).
 *   effective gradient = g * grad_scale_host * (grad_scale ? *grad_scale : 1): the host factor
 *               carries 1/world_size of the data-parallel mean, the nullable device scalar the
 *               clip coefficient (no host sync);  p_bf16: nullable bf16 copy of the new params
 *   grad_clip_coef: coef = min(1, max_norm / (pre_scale*||g||_2 + 1e-6)), norm_out nullable
 */
int edgedict_adam_step(float* p, const float* g, float* m, float* v, long long n, float lr,
                       float beta1, float beta2, float eps, int step, float weight_decay,
                       float grad_scale_host, const float* grad_scale, void* p_bf16, void* stream);
/* The same step, skipped entirely (p, m, v untouched) when any of the n_skip (<= 16) device-visible words
 * at skip_words is non-zero: the trainer passes edgedict_stack_error_words(0), so the gradients of a step
 * whose encoder stack gave up a bounded in-kernel wait are never applied - without a host synchronisation;
 * the host raises at its next edgedict_stack_wsr_error().  The words live in pinned host memory: a one-lane
 * kernel ORs them into guard_scratch[0] (caller-owned DEVICE word) right before the update, which reads
 * only that word (reading the host words from every workgroup cost 0.3-1 ms per step). */
int edgedict_adam_step_guarded(float* p, const float* g, float* m, float* v, long long n, float lr,
                               float beta1, float beta2, float eps, int step, float weight_decay,
                               float grad_scale_host, const float* grad_scale, void* p_bf16,
                               const unsigned* skip_words, int n_skip, unsigned* guard_scratch,
                               void* stream);
int edgedict_grad_clip_coef(const float* g, long long n, float max_norm, float pre_scale,
                            float* sumsq_ws, float* coef, float* norm_out, void* stream);
/* measurement aid, not on the hot path: a stand-in for a collective library's resident kernels - `workgroups`
 * workgroups of 512 threads with >= 128 live registers per lane that read-modify-write buf[0, n_floats) `passes`
 * times (values unchanged).  tools/rccl_footprint.py runs it on the auxiliary stream at every grads_final point of
 * the backward pass (where cli/lightning.py:325-331's bucketed all-reduce would run) to see what the recurrence
 * launches lose to it and that no bounded in-kernel wait gives up. */
int edgedict_debug_footprint(float* buf, long long n_floats, int workgroups, int passes, void* stream);

/* ------------------------------------------------------------------------------------
 * Log-mel filterbank front-end.  Replaces FilterbankFeatures.forward (rnnt/features.py:106-152,
 * twin parts/features.py:298-347) + Downsample.forward (rnnt/transforms.py:38-51) in one kernel;
 * the STFT spectrum never reaches HBM.
 *   wave      fp32 [B, N] (row stride wave_stride); lengths nullable int32 [B] valid samples
 *   window    fp32 [n_fft]  hann(win_length, periodic=False) centred in n_fft, zeros outside
 *             [win_lo, win_hi);  twiddle fp32 [n_fft/2][2] = cos,sin(2*pi*k/n_fft)
 *   fb        fp32 [n_mels, n_fft/2+1] mel weights; fb_range int32 [n_mels][2] non-zero support
 *   out[b*o_b + (f/stack)*o_group + (f%stack)*o_k + m*o_m], f < frames_out (multiple of stack):
 *             frames f >= 1+N_b/hop (no such STFT frame) and f >= ceil(N_b/hop) (the reference's
 *             seq_len mask) are written as zeros.
 * dither: wave[b,n] += amplitude * N(0,1) in place (rnnt/features.py:111-112), counter-based RNG.
 */
int edgedict_dither(float* wave, long long wave_stride, int B, int N, const int32_t* lengths,
                    float amplitude, unsigned seed, void* stream);
int edgedict_fbank_forward(const float* wave, long long wave_stride, int B, int N,
                           const int32_t* lengths, const float* window, const float* twiddle,
                           const float* fb, const int32_t* fb_range, int n_fft, int win_lo,
                           int win_hi, int hop, int n_mels, float preemph, int do_log, void* out,
                           int out_dtype, long long o_b, long long o_group, long long o_k,
                           long long o_m, int stack, int frames_out, void* stream);
/* The Jasper-derived twin, FilterbankFeatures.forward(x, seq_len) of parts/features.py:298-347:
 * the STFT runs over the whole padded row (reflect padding at N, not at the utterance end),
 * seq_len (samples, int32 [B], nullable) only MASKS frames f >= ceil(seq_len/hop) to zero;
 *   out fp32 [b*o_b + (c*n_mels + m)*o_m + f], c < copies ("frame splicing" as the reference writes
 *   it, :111-123, stacks `copies` identical blocks along the feature axis; o_copy = n_mels*o_m),
 *   frames_out <= o_m (a larger o_m leaves the caller's pad_to padding untouched: pre-zeroed);
 *   normalize 0 none / 1 per_feature / 2 all_features = normalize_batch (:80-109): mean and
 *   unbiased std over the first ceil(seq_len/hop) frames, std + 1e-5;
 *   n_signal (0 or N: none): samples [n_signal, N) are zeros appended AFTER the pre-emphasis - the
 *   reference zero-pads the already pre-emphasised short input to win_length (:289-294). */
int edgedict_fbank_forward_masked(const float* wave, long long wave_stride, int B, int N,
                                  const int32_t* seq_len, const float* window,
                                  const float* twiddle, const float* fb, const int32_t* fb_range,
                                  int n_fft, int win_lo, int win_hi, int hop, int n_mels,
                                  float preemph, int do_log, float* out, long long o_b,
                                  long long o_m, int frames_out, int copies, long long o_copy,
                                  int normalize, int n_signal, void* stream);

/* ------------------------------------------------------------------------------------
 * Batched greedy / streaming search: the whole per-frame loop of Transducer.greedy_decode
 * (rnnt/models.py:243-269) or PytorchStreamDecoder.decode (rnnt/stream.py:102-119) in one call.
 *   E1        dtype, frame t of row b at E1[b*e_row_stride + t*e_frame_stride + j]: the encoder
 *             half of the joint's first Linear, enc_out * W1[:, :P_enc]^T, for all T frames
 *   W1d       dtype [J, P2] view (leading dimension ldw1) = W1[:, P_enc:];  b1 fp32 [J]
 *   W2        dtype [V, J]; b2 fp32 [V];  emb [V, E] (emb_dtype);  Wp dtype [P2, H]; bp fp32 [P2]
 *   w_ih/w_hh/b_ih/b_hh  HOST arrays of L device pointers (prediction-network LSTM layers)
 *   h_state, c_state fp32 [L,B,H] and dec_out dtype [B,P2]: prediction-network state, in/out
 *   unk < 0 : greedy mode  (log-softmax max; score[b] += -max log p; nullable score)
 *   unk >= 0: stream mode  (raw-logit arg-max with the reference's <unk> rule)
 *   tokens_out int32, token of row b at frame t stored at tokens_out[b*tok_stride + t] (nullable)
 *   workspace: edgedict_greedy_workspace_bytes(...) bytes, 256-byte aligned
 */
size_t edgedict_greedy_workspace_bytes(int dtype, int B, int J, int V, int E, int L, int H, int P2);
int edgedict_greedy_decode(int dtype, const void* E1, long long e_row_stride,
                           long long e_frame_stride, int B, int T, int J, const void* W1d,
                           long long ldw1, const float* b1, int P2, const void* W2,
                           const float* b2, int V, const void* emb, int emb_dtype, int E, int L,
                           const void* const* w_ih, const void* const* w_hh,
                           const float* const* b_ih, const float* const* b_hh, int H,
                           const void* Wp, const float* bp, float* h_state, float* c_state,
                           void* dec_out, int blank, int unk, int32_t* tokens_out, int tok_stride,
                           float* score, void* workspace, void* stream);
/* Route query: 1 where the searches run a frame / an expansion of these dimensions as the fused launches of
 * csrc/decode_fused.hip, 0 where they compose it from the general kernels (csrc/decode.hip).  dtype = the search's
 * compute dtype, emb_dtype = the embedding table's (ED_F32 / ED_BF16).  Touches no device. */
int edgedict_decode_fused_ok(int dtype, int emb_dtype, int J, int V, int E, int H, int P2);

/* ------------------------------------------------------------------------------------
 * GRU time recurrence (the module_type='GRU' encoder variant, ResLayerNormGRU rnnt/models.py:77-116;
 * PyTorch nn.GRU semantics, gate order r,z,n).  Batch-first buffers, one kernel per time step:
 *   G      [B,T,3H] dtype  in : x W_ih^T + b_ih for every t;  out: r, z, n (post-activation)
 *   Hprev  [B,T,H]  dtype  out: h_{t-1} per step (row t=0 <- h0 or zeros)
 *   Y      [B,T,H]  dtype  out: h_t;   HN [B,T,H] dtype out: W_hn h_{t-1} + b_hn (saved for BPTT)
 *   Whh    [3H,H]   dtype; b_hh fp32 [3H]; h0 fp32 [B,H] nullable; hN fp32 [B,H] nullable
 * backward (after forward, same buffers):
 *   G      in: r,z,n;  out: dL/d(input-side pre-activations)    -> dX, dW_ih, db_ih
 *   DH     [B,T,3H] dtype out: dL/d(hidden-side pre-activations) -> dW_hh (with Hprev), db_hh
 *   dY     [B,T,H] dtype nullable;  WhhT [H,3H] dtype;  dh_ws fp32 [B,H] scratch
 * Limits: H % 8 == 0.  The gradient wrt h0 is not produced.
 */
int edgedict_gru_forward(int dtype, void* G, void* Hprev, void* Y, void* HN, const void* Whh,
                         const float* b_hh, const float* h0, float* hN, int B, int T, int H,
                         void* stream);
int edgedict_gru_backward(int dtype, void* G, void* DH, const void* dY, const void* Hprev,
                          const void* HN, const void* WhhT, float* dh_ws, int B, int T, int H,
                          void* stream);

/* ------------------------------------------------------------------------------------
 * Convolutional waveform front-end (FrontEnd, rnnt/models.py:313-365; DilatedConvBlock :323-339;
 * CausalConv1d :314-318), channels-last activations [B, T, C].  A convolution = im2col gather +
 * edgedict_gemm against the weight viewed as [C_out, C_in*k] (column c*k + j); its backward =
 * two GEMMs + the col2im gather.
 *   conv_out_frames(Tin, k, s)   frames after Conv1d(padding k-1, stride s) minus the k-1 dropped ones
 *   conv_im2col   x [B,Tin,C] (in_dtype) -> cols [B,Tout,C*k] (out_dtype); f32->f32, f32->bf16, bf16->bf16
 *   conv_col2im   dcols [B,Tout,C*k] -> dx [B,Tin,C] (same dtype), gather form (no atomics)
 *   gelu_groupnorm_fwd  out = GroupNorm_1group(GELU(y)) with per-channel gamma/beta; y,out [B,T,C];
 *                       mean, rstd fp32 [B] (saved for backward); exact-erf GELU, eps as nn.GroupNorm
 *   gelu_groupnorm_bwd  dy wrt y, dgamma/dbeta fp32 [C] (written, not accumulated); C <= 256;
 *                       workspace of gelu_groupnorm_bwd_workspace_bytes(B,T,C) bytes
 */
int edgedict_conv_out_frames(int Tin, int k, int s);
int edgedict_conv_im2col(int in_dtype, int out_dtype, const void* x, void* cols, int B, int Tin, int C,
                         int k, int s, void* stream);
int edgedict_conv_col2im(int dtype, const void* dcols, void* dx, int B, int Tin, int C, int k, int s,
                         void* stream);
int edgedict_gelu_groupnorm_fwd(int dtype, const void* y, const float* gamma, const float* beta,
                                void* out, float* mean, float* rstd, int B, int T, int C, float eps,
                                void* stream);
size_t edgedict_gelu_groupnorm_bwd_workspace_bytes(int B, int T, int C);
int edgedict_gelu_groupnorm_bwd(int dtype, const void* y, const void* dout, const float* gamma,
                                const float* mean, const float* rstd, void* dy, float* dgamma,
                                float* dbeta, void* workspace, int B, int T, int C, void* stream);

/* Number of products edgedict_gemm has handed to hipBLASLt in this process (only the large,
 * short-K bf16 NT product of the joint's logits qualifies; csrc/blaslt.cpp).  0 when the vendor
 * library is absent or EDGEDICT_BLASLT=0: every product then runs on this library's kernels. */
long long edgedict_blaslt_calls(void);

/* ------------------------------------------------------------------------------------
 * Streaming encoder step (bf16): PytorchStreamDecoder.decode's `self.encoder(xs, (enc_h, enc_c))`
 * (rnnt/stream.py:93-100) on a chunk of a few frames for B concurrent streams - Encoder.forward
 * rnnt/models.py:131-136 without its output projection: input LayerNorm, then per layer T fused LSTM steps
 * (input product + recurrent product + cell in one launch per frame) and the residual / LayerNorm / TimeReduction
 * of ResLayerNormLSTM.forward :55-75.  One native call instead of ~4 launches per layer-frame plus host glue.
 *   xs            [B, T, I0] x_dtype (ED_F32 or ED_BF16), I0 % 8 == 0;  H % 32 == 0
 *   w_ih / w_hh   HOST arrays [L] of bf16 DEVICE matrices [4H, K_l] / [4H, H] (PyTorch gate order i,f,g,o)
 *   b_ih / b_hh / ln_gamma / ln_beta  HOST arrays [L] of fp32 DEVICE vectors;  reduce HOST int [L] in {1, 2}
 *   h_state / c_state  fp32 [L, B, H], updated in place;  out bf16 [B, T_out, H], T_out returned through *T_out
 */
size_t edgedict_stream_encoder_workspace_bytes(int B, int T, int I0, int H, int L);
int edgedict_stream_encoder_step(const void* xs, int x_dtype, int B, int T, int I0, int H, int L,
                                 const float* in_gamma, const float* in_beta, const void* const* w_ih,
                                 const void* const* w_hh, const float* const* b_ih, const float* const* b_hh,
                                 const float* const* ln_gamma, const float* const* ln_beta, const int* reduce,
                                 float* h_state, float* c_state, void* out, int* T_out, void* workspace,
                                 void* stream);

/* ------------------------------------------------------------------------------------
 * What every search below takes: the transducer's search network, described once, and the optional features.
 *   edgedict_search_net_t   the joint and the prediction network, operands as edgedict_greedy_decode's (w_ih / w_hh /
 *                           b_ih / b_hh: HOST arrays [L] of DEVICE pointers), the compute dtype, blank, and bos = the token
 *                           the empty hypothesis feeds first (BOS = 2, zero state).  The size queries read only the shape
 *                           fields (dtype, J, P2, V, E, L, H) and return 0 for a null network
 *   edgedict_search_opts_t  lm: LM shallow fusion, bias: contextual biasing, ilm_weight (a HOST double): internal-LM
 *                           estimation - each specified in its own block below.  A null member switches its feature off,
 *                           a null opts pointer is all members null: the plain search, launch for launch and bit for bit.
 *                           ngram: a back-off n-gram LM (edgedict_ngram_lm_t below) fused into the frame-synchronous
 *                           search, specified in that search's block; lm and ngram both non-null is an argument error
 *                           (one LM at a time).  The expansion searches (edgedict_beam_*) refuse ilm_weight and ngram
 *                           before they touch the device.  The struct GREW AT ITS END (ngram, 24 -> 32 bytes) without a
 *                           new ABI version: every member is read, so a caller must pass the struct of this header -
 *                           a binding checks edgedict_search_struct_bytes(1) == 32
 * A descriptor leads every argument list: net where the function needs the network (opts then stands in front of the
 * trailing buffers), opts where it does not.  A non-null net / opts below address 4096 - the integer a caller written
 * for ABI version 1 passes in that place - is an argument error (size queries: 0), never dereferenced.
 * search_struct_bytes: sizeof(edgedict_search_net_t) (which = 0) / sizeof(edgedict_search_opts_t) (which = 1), for
 * bindings that mirror them.
 */
struct edgedict_beam_lm_t;
struct edgedict_beam_bias_t;
struct edgedict_ngram_lm_t;
typedef struct edgedict_search_net_t {
    int dtype;
    int J;
    const void* W1d;
    long long ldw1;
    const float* b1;
    int P2;
    const void* W2;
    const float* b2;
    int V;
    const void* emb;
    int emb_dtype, E, L;
    const void* const* w_ih;
    const void* const* w_hh;
    const float* const* b_ih;
    const float* const* b_hh;
    int H;
    const void* Wp;
    const float* bp;
    int blank, bos;
} edgedict_search_net_t;
typedef struct edgedict_search_opts_t {
    const struct edgedict_beam_lm_t* lm;
    const struct edgedict_beam_bias_t* bias;
    const double* ilm_weight;
    const struct edgedict_ngram_lm_t* ngram;
} edgedict_search_opts_t;
size_t edgedict_search_struct_bytes(int which);

/* ------------------------------------------------------------------------------------
 * Batched beam search: the reference's legacy Transducer.beam_search (models.py:121-202; Sequence
 * models.py:212-224) for B utterances in lockstep, over the maintained model's prediction network and
 * joint.  net / opts as above, E1 and its strides as edgedict_greedy_decode's, plus
 *   lens_host        HOST int32 [B]: encoder frames of each utterance (<= T)
 *   W                beam width;  max_expansions >= W: cap on pops per utterance and frame
 *                    (exceeding it is an error, never a silent truncation)
 *   tokens_host      HOST int32 [B, max_tokens]: tokens of B[0] (no blanks, no BOS)
 *   ntokens_host     HOST int32 [B];  score_host HOST fp64 [B] = -log p of that hypothesis
 *   prefix           0 / 1: the `prefix` argument of the reference method.  1 = models.py:145-161: at the start of every
 *                    frame the probability of reaching a hypothesis A[j] through a later list entry A[i] that is a
 *                    proper prefix of it (the missing tokens emitted on this frame, each from the prediction-network
 *                    output stored when that position was expanded - Sequence.g) is folded into logp(A[j]) with
 *                    log_aplusb, pairs in the reference's order.  The list logic runs on the host (the call already
 *                    synchronises every lockstep iteration), the joint evaluations as one batched device pass per frame
 *   expansions_host  HOST, nullable: total number of prediction-network steps (pops; with prefix = 1 also one per
 *                    merged pair, as the reference spends them)
 * Scores are accumulated in fp64 from fp32 log-softmax values, as the reference's Python floats
 * are.  The call synchronises the stream (the loop's stop test is data dependent).
 */
size_t edgedict_beam_workspace_bytes(const edgedict_search_net_t* net, int B, int T, int W, int max_expansions,
                                     int prefix, const edgedict_search_opts_t* opts);
int edgedict_beam_search(const edgedict_search_net_t* net, const void* E1, long long e_row_stride,
                         long long e_frame_stride, int B, int T, const int32_t* lens_host, int W, int max_expansions,
                         int prefix, int32_t* tokens_host, int max_tokens, int32_t* ntokens_host, double* score_host,
                         long long* expansions_host, const edgedict_search_opts_t* opts, void* workspace, void* stream);

/* ------------------------------------------------------------------------------------
 * Streaming beam search: edgedict_beam_search (prefix = 0) with its frame-to-frame list B kept in a
 * persistent STATE for S streams, so that advancing over frames [0, t1) and then [t1, t2) gives
 * exactly what one offline call over [0, t2) gives.  Per stream the state holds the survivors (fp64
 * logp, token-tree node, prediction-network (h, c) [W][L][H], their count), the token tree
 * (parent, token) with its node count and the last token of its root, and the count of committed
 * tokens.  After every advance each stream's tree is compacted: nodes that are no ancestor of a
 * survivor are dropped, the tokens from the root down to the survivors' lowest common ancestor are
 * COMMITTED (they can no longer change) and returned to the caller, who keeps the log, and that
 * ancestor becomes the new root.  The tree's size then does not depend on how long a stream has run.
 *   node_capacity   token-tree nodes per stream; an advance whose streams may need more (live nodes +
 *                   frames x max_expansions) fails before it runs, naming node_capacity
 * beam_stream_state_bytes     device bytes of the state (contents undefined until a reset of all streams)
 * beam_stream_workspace_bytes device bytes of the per-call workspace of beam_stream_advance
 * beam_stream_reset           streams with mask[b] != 0 (mask null: all; mask_on_host: HOST int32 [S], else
 *                             device) -> the empty hypothesis: one survivor, logp 0, `bos` fed first, zero
 *                             state, empty tree and committed log
 * beam_stream_advance         operands as edgedict_beam_search; E1 holds the encoder half of the joint's first
 *                             Linear of this chunk's frames.  n_frames_host HOST int32 [S]: frames of each
 *                             stream in this chunk (0: the stream sits the chunk out, its state unchanged).
 *                             commit_host HOST int32 [S, node_capacity] / ncommit_host HOST int32 [S]: the
 *                             tokens committed by this advance; expansions_host HOST, nullable: pops of
 *                             this call.  Synchronises the stream.  After an error other than the capacity
 *                             check the advanced streams' state is undefined (reset them).
 * beam_stream_read            per stream: the uncommitted tail of B[0] (the tokens from the root to its node,
 *                             no blanks, no BOS; the full hypothesis is the committed log followed by it),
 *                             its score -logp (fp64), the number of committed tokens before the tail
 *                             (ncommitted_host, nullable) and the expansions since the stream's reset
 *                             (expansions_host, nullable).  Synchronises the stream.
 * The state's and the workspace's layout depend on opts (an LM and a bias list append their parts): size, reset and
 * advance a state with the same features.  detail_state of reset and detail_state / detail_workspace /
 * commit_frame_host / commit_logp_host of advance are the N-best detail (below): all null for none, partly null is an
 * argument error.
 */
size_t edgedict_beam_stream_state_bytes(const edgedict_search_opts_t* opts, int S, int L, int H, int W,
                                        int node_capacity);
size_t edgedict_beam_stream_workspace_bytes(const edgedict_search_net_t* net, int S, int W, int max_expansions,
                                            int node_capacity, const edgedict_search_opts_t* opts);
int edgedict_beam_stream_reset(const edgedict_search_opts_t* opts, int S, int L, int H, int W, int node_capacity,
                               int bos, const int32_t* mask, int mask_on_host, void* state, void* detail_state,
                               void* stream);
int edgedict_beam_stream_advance(const edgedict_search_net_t* net, const void* E1, long long e_row_stride,
                                 long long e_frame_stride, int S, const int32_t* n_frames_host, int W,
                                 int max_expansions, int node_capacity, int32_t* commit_host, int32_t* ncommit_host,
                                 long long* expansions_host, const edgedict_search_opts_t* opts, void* state,
                                 void* workspace, void* detail_state, void* detail_workspace,
                                 int32_t* commit_frame_host, double* commit_logp_host, void* stream);
int edgedict_beam_stream_read(int S, int L, int H, int W, int node_capacity, const void* state,
                              int32_t* tokens_host, int max_tokens, int32_t* ntokens_host,
                              double* score_host, long long* ncommitted_host,
                              long long* expansions_host, void* stream);

/* ------------------------------------------------------------------------------------
 * LM shallow fusion for both beam searches: an external LSTM language model (the reference's LMModel,
 * models.py:224-261: Embedding -> nn.LSTM stack -> Linear -> log_softmax, trained by cli/train_lm.py on
 * the transducer's vocabulary) runs one step per expansion beside the prediction network.  A popped
 * hypothesis y* (fp64 score `base`) feeds its last token to the LM from y*'s stored LM state; with
 * lp_lm = log_softmax(LM logits) (fp32, all ntoken entries) the children are scored, in fp64 and in
 * exactly this order,
 *   non-blank child k:  base + (double)lp_rnnt[k] + (weight * (double)lp_lm[k] + length_bonus)
 *   blank child:        base + (double)lp_rnnt[blank]                       (the LM sees no blank)
 * No end-of-sentence term (the LM has no EOS token).  The stop test, B[:W] and B[0] are the plain
 * search's, applied to the fused scores; the returned score is -(fused logp).  The root of a tree the
 * LM has never seen feeds `bos` (cli/train_lm.py:42 prepends 1) from a zero state (init_hidden); a
 * stream that has committed tokens feeds its last committed token, as the prediction network does.
 * weight = length_bonus = 0 gives tokens, scores and expansion counts bit-equal to the plain search.
 * A positive length_bonus can raise the pops per frame: hitting max_expansions stays an error.
 *   L, E, H, V   layers, embedding width, hidden width, ntoken (must equal the transducer's V)
 *   emb          [V, E] in emb_dtype;  w_ih / w_hh / b_ih / b_hh: HOST arrays [L] of DEVICE pointers
 *                ([4H, E or H], [4H, H] in the search's dtype; fp32 [4H]);  Wo [V, H] dtype, bo fp32 [V]
 * The searches take the LM as opts->lm (null: exactly the plain call).
 * prefix = 1 with an LM is refused (it would need LM log-probs stored per token-tree node).  The
 * streaming state with an LM appends the survivors' LM (h, c) behind the plain layout, so
 * edgedict_beam_stream_read serves both; reset and advance of such a state must be given the LM too.
 * beam_lm_struct_bytes: sizeof(edgedict_beam_lm_t), for bindings that mirror it.
 */
typedef struct edgedict_beam_lm_t {
    int L, E, H, V;
    const void* emb;
    int emb_dtype;
    const void* const* w_ih;
    const void* const* w_hh;
    const float* const* b_ih;
    const float* const* b_hh;
    const void* Wo;
    const float* bo;
    int bos;
    double weight;
    double length_bonus;
} edgedict_beam_lm_t;

size_t edgedict_beam_lm_struct_bytes(void);

/* ------------------------------------------------------------------------------------
 * N-best lists with token frames and log-probs from both beam searches.  edgedict_beam_search_nbest and
 * the streaming calls with their detail pointers run the searches above (same frame loop, same pops, same scores) and keep, beside every
 * token-tree node, a DETAIL:
 *   frame   the encoder frame on which the expansion that produced the node's token ran (offline: the
 *           index into the utterance; streaming: counted since the stream's last reset)
 *   logp    the token's score increment, score(child in the pool) - score(popped parent), an fp64
 *           difference; with an LM the fused increment lp_rnnt + (weight * lp_lm + length_bonus)
 * and return the WHOLE list B of the last frame (n <= W hypotheses, in B's insertion order; entry 0 is
 * what the plain calls return, logp[.][0] = -score bit for bit), each hypothesis root to leaf with its
 * tokens, frames and increments.  The paths are walked by a kernel into a dense device result
 * [B][W][max_tokens]; only the lengths, the scores and the used columns of it are copied to the host.
 * The plain entry points are unchanged and run the kernels they ran before; the detail lives in
 * buffers of its own with their own size queries:
 *   beam_detail_bytes(B, T, max_expansions)            device bytes of the offline search's detail
 *   beam_nbest_result_bytes(B, W, max_tokens)          device bytes of the read-out's result
 *   beam_stream_detail_state_bytes(S, node_capacity)   persistent, beside the streams' state: the
 *                                                      nodes' detail and the frames done per stream
 *   beam_stream_detail_workspace_bytes(S, node_capacity) per call, beside beam_stream_advance's
 *                                                      workspace (compaction moves the detail too)
 * beam_search_nbest            operands as edgedict_beam_search (workspace sized by
 *                              edgedict_beam_workspace_bytes with prefix = 0), with the outputs
 *                                tokens_host / frames_host  HOST int32 [B, W, max_tokens]
 *                                token_logp_host            HOST fp64  [B, W, max_tokens]
 *                                ntokens_host HOST int32 [B, W];  nhyp_host HOST int32 [B] (= n)
 *                                logp_host    HOST fp64  [B, W] = log p (fused with an LM)
 *                              Entries behind n / behind a hypothesis' length are not written.  An
 *                              utterance of 0 frames has one empty hypothesis with logp 0.  prefix = 1
 *                              is refused (-1) before anything runs: the prefix merge changes a score
 *                              at frame starts, so the increments would no longer add up to it.  A
 *                              hypothesis longer than max_tokens is an error, never a truncation.
 * beam_stream_reset, detail    the reset, and the selected streams' frame count -> 0
 * beam_stream_advance, detail  the advance; additionally commit_frame_host HOST int32
 *                              / commit_logp_host HOST fp64 [S, node_capacity]: frames and increments of
 *                              the tokens committed by this advance, next to commit_host
 * beam_stream_read_nbest       per stream the uncommitted tails of every entry of B as above (the full
 *                              hypothesis is the committed log followed by the tail); ncommitted_host,
 *                              expansions_host as edgedict_beam_stream_read; frames_done_host HOST int64
 *                              [S], nullable: frames since the stream's reset.  Synchronises the stream.
 * A state advanced with the detail must always be reset, advanced and read with it.
 */
size_t edgedict_beam_detail_bytes(int B, int T, int max_expansions);
size_t edgedict_beam_nbest_result_bytes(int B, int W, int max_tokens);
int edgedict_beam_search_nbest(const edgedict_search_net_t* net, const void* E1, long long e_row_stride,
                               long long e_frame_stride, int B, int T, const int32_t* lens_host, int W,
                               int max_expansions, int prefix, int32_t* tokens_host, int32_t* frames_host,
                               double* token_logp_host, int max_tokens, int32_t* ntokens_host, int32_t* nhyp_host,
                               double* logp_host, long long* expansions_host, const edgedict_search_opts_t* opts,
                               void* workspace, void* detail, void* result, void* stream);
size_t edgedict_beam_stream_detail_state_bytes(int S, int node_capacity);
size_t edgedict_beam_stream_detail_workspace_bytes(int S, int node_capacity);
int edgedict_beam_stream_read_nbest(int S, int L, int H, int W, int node_capacity, const void* state,
                                    const void* detail_state, void* result, int32_t* tokens_host,
                                    int32_t* frames_host, double* token_logp_host, int max_tokens,
                                    int32_t* ntokens_host, int32_t* nhyp_host, double* logp_host,
                                    long long* ncommitted_host, long long* expansions_host,
                                    long long* frames_done_host, void* stream);

/* ------------------------------------------------------------------------------------
 * Contextual biasing (phrase boosting) for both beam searches: a phrase automaton (the phrases' trie with
 * Aho-Corasick failure links, built on the host: edgedict_amd/bias.py) whose state every hypothesis
 * carries under the same state reference as the prediction network's (h, c) - the state BEFORE the
 * hypothesis' last token.  Popping y* with last token tok from carried state s0 gives s = goto(s0, tok),
 * kept under the expansion's slot; the children are scored, in fp64 and in exactly this order,
 *   non-blank child k:  (base + (double)lp_rnnt[k]) + D(s, k)              D(s, k) = held[goto(s, k)] - pend[s]
 *   with an LM:         ((base + (double)lp_rnnt[k]) + (weight * (double)lp_lm[k] + length_bonus)) + D(s, k)
 *   blank child:        base + (double)lp_rnnt[blank]
 * The kernels read only these DEVICE tables:
 *   root_next [V] int32   goto(0, k)
 *   held, pend [S] fp64   bonus held on entering a state / still pending in it (0 once a phrase ended)
 *   row_ptr [S + 1] int32, exc_tok / exc_next [n_exc] int32: per state the EXCEPTIONS, the tokens (sorted)
 *                         where goto(s, k) != goto(0, k), and their targets; every other token takes root_next
 * All targets must lie in [0, S) and exc_tok in [0, V): the tables are trusted (ContextGraph writes them).
 * The searches take the list as opts->bias, with or without opts->lm: bias = null is exactly the call
 * without it (same kernels, same layouts).  With a bias list the searches run the separately
 * compiled beam_pop[_detail]_bias / beam_expand[_lm]_bias kernels; prefix = 1 is refused.  The offline
 * workspace and the streams' state / workspace append the bias state arrays behind the LM's part, so
 * edgedict_beam_stream_read[_nbest] serve every form; a state sized with a bias list must be reset and
 * advanced with one (the list may change at a reset: the root state is 0 in every automaton).
 * beam_bias_struct_bytes: sizeof(edgedict_beam_bias_t), for bindings that mirror it.
 */
typedef struct edgedict_beam_bias_t {
    int S, V, n_exc;
    const int32_t* root_next;
    const double* held;
    const double* pend;
    const int32_t* row_ptr;
    const int32_t* exc_tok;
    const int32_t* exc_next;
} edgedict_beam_bias_t;

size_t edgedict_beam_bias_struct_bytes(void);

/* ------------------------------------------------------------------------------------
 * Row log-softmax (LMModel.forward's F.log_softmax(decoded, dim=-1), models.py:251):
 *   x fp32 or bf16 (x_dtype) [M, N] rows of leading dimension ldx;  y fp32 [M, N] contiguous.
 *   y = (x - max) - log(sum exp(x - max)) per row, fp32 arithmetic.
 */
int edgedict_log_softmax_rows(int x_dtype, const void* x, long long ldx, float* y, int M, int N,
                              void* stream);
/* Its backward:  dx = dy - exp(y) * rowsum(dy).  y fp32 [M, N] contiguous (the forward's output), dy fp32 rows of
 * leading dimension lddy, dx [M, N] contiguous in dx_dtype (the dtype the logits had). */
int edgedict_log_softmax_rows_bwd(const float* y, const float* dy, long long lddy, int dx_dtype, void* dx, int M,
                                  int N, void* stream);

/* ------------------------------------------------------------------------------------
 * Softmax negative log-likelihood on raw logits (the LM's training loss and sentence scorer: log_softmax followed by
 * NLLLoss(ignore_index) of cli/train_lm.py, csrc/lm_loss.hip).
 *
 *   logits   [M, V]  fp32 or bf16 (dtype code), rows of leading dimension ldx >= V.  16-byte accesses when the base
 *                    pointer is 16-byte aligned and V and ldx are multiples of 16 / sizeof(dtype); otherwise a scalar
 *                    path.
 *   targets  [M]     int32.  Row m is IGNORED when targets[m] == ignore_index or lies outside [0, V).
 *   lse      [M]     fp32 out (nullable): max + log(sum exp(z - max)), fp32 arithmetic
 *   nll      [M]     fp32 out: lse - z[m, targets[m]], exactly 0 for an ignored row
 *   stats    [2]     fp64 out (nullable): {sum of nll over the valid rows, number of valid rows}, added in a fixed
 *                    order by one workgroup (no atomics).  NULL = forward-only scoring: nll (and lse) only.
 *   reduced  [1]     fp32 out (nullable, needs stats): mean ? sum / count : sum; 'mean' over zero valid rows is 0.
 *
 * backward overwrites the logits IN PLACE, in their dtype, with d(loss)/d(logits): a valid row gets
 * g_m * (exp(z - lse[m]) - onehot(targets[m])), an ignored row exact zeros (it is not read).  g_m = grad[m *
 * grad_stride] (grad_stride 1: a gradient per row, reduction 'none'; 0: one device scalar), divided by stats[1] when
 * mean != 0 (zero when no row is valid).  Everything is read on the device; neither call synchronises.
 * Forward plus backward read the logits twice and write them once; loss, nll, lse and the gradient are bit-identical
 * from run to run.
 */
int edgedict_softmax_nll_forward(int dtype, const void* logits, long long ldx, const int32_t* targets, int M, int V,
                                 int ignore_index, float* lse, float* nll, double* stats, float* reduced, int mean,
                                 void* stream);
int edgedict_softmax_nll_backward(int dtype, void* logits, long long ldx, const int32_t* targets, int M, int V,
                                  int ignore_index, const float* lse, const float* grad, int grad_stride,
                                  const double* stats, int mean, void* stream);

/* ------------------------------------------------------------------------------------
 * CTC loss (Graves et al. 2006) on the encoder's auxiliary head, and the CTC greedy decoder.  Not in the
 * reference: the auxiliary term of  loss = rnnt + ctc_weight * ctc  (Transducer(ctc_weight=...)).
 *
 *   logits      [B, T, V]   raw head logits (NOT log-softmaxed), contiguous, dtype code
 *   labels      [B, U]      int32, values in [0, V) other than blank, padded arbitrarily beyond label_lens[b]
 *                           (nullable when U == 0)
 *   act_lens    [B] int32   valid frames per utterance; rows t >= act_lens[b] are never read
 *   label_lens  [B] int32   valid labels per utterance (0 <= label_lens[b] <= U); both are clamped to [0, T] / [0, U]
 *   costs       [B] fp32    out: -log P(y|x) per utterance; +inf where no path exists (act_lens[b] <= 0, or fewer
 *                           frames than labels + adjacent repeats) - with zero_infinity != 0 such a cost is 0
 *   reduced     [1] fp32    out (nullable): reduce_scale * sum_b costs[b]  ('mean' => 1/B)
 *   workspace   edgedict_ctc_workspace_bytes(B,T,U) bytes, 16-byte aligned; forward fills it (log-sum-exps, the
 *               blank's and the labels' log-probabilities, fp64 alpha / beta over the 2U+1 states, log-likelihoods,
 *               dead-utterance flags, same-label links) and backward reads it: keep it alive between the two.
 *               beta(t,s) does NOT contain frame t's own log-probability: occupancy = exp(alpha + beta - ll).
 *
 * backward writes d(sum_b scale_b * cost_b)/d(logits) into grads (same shape / dtype as logits), scale_b as
 * edgedict_rnnt_loss_backward defines it.  Rows t >= act_lens[b] and utterances without a path (or whose cost
 * zero_infinity replaced) get exact zeros.  The gradient is bit-identical from run to run.
 * Limits: U <= 1023, V >= 2; V*sizeof(dtype) a multiple of 16 for the vector path (other V take a scalar path).
 * edgedict_ctc_workspace_view (debug reader): which = 0 log-sum-exp [B,T] f32, 1 alpha / 2 beta [B,T,2U+1] f64,
 * 3 log-likelihoods [B,2] f64 (alpha side, beta side), 4 lp_blank [B,T] f32, 5 lp_label [B,T,U] f32,
 * 6 dead flags [B] int32, 7 same-label links [B,2,U] int32.
 *
 * edgedict_ctc_greedy: k_t = arg max_v logits[b,t,:] (lowest index on ties) for t < act_lens[b]; frame t is kept iff
 * k_t != blank and (t == 0 or k_t != k_{t-1}).  tokens / frames [B, T] int32: the kept symbols and their frame
 * indices, -1 behind counts[b]; neglogp [B] fp32 = -sum over kept frames of log_softmax(logits[b,t])[k_t];
 * scratch: 8 * B * T bytes.
 *
 * edgedict_ctc_align: the forced aligner of the head - Viterbi over the loss's lattice, fp64 carry,
 *   v(t,s) = max(v(t-1,s), v(t-1,s-1), [skip(s)] v(t-1,s-2)) + (double)lp(t,s),  lp the loss's fp32 log-probabilities.
 *   frames, ends [B, U] int32  out: the first / last frame the best path spends in label u's state; strictly
 *                              increasing in u, ends[u] < frames[u+1], at most act_lens[b] - 1; -1 behind label_lens[b]
 *                              (both nullable when U == 0)
 *   scores       [B] fp32      out: the best path's log-probability (<= -cost)
 *   A row without a path (act_lens[b] <= 0, or fewer frames than labels + adjacent repeats): score -inf, frames and
 *   ends all -1; the other rows are unaffected.  TIE RULE: the later emission wins - the path ends in the last label's
 *   state when that scores >= the final blank, and among the equal best predecessors of a state it comes from s - 2
 *   (where the skip is allowed), else s - 1, else s.  Three launches (the loss's row pass, the walk, the back-trace),
 *   no host sync, no atomics, bit-identical from run to run.  The workspace (size and layout of the loss's, 16-byte
 *   aligned) is scratch: v lies where the alphas go (view 1), the beta plane is not written.
 */
size_t edgedict_ctc_workspace_bytes(int B, int T, int U);
const void* edgedict_ctc_workspace_view(const void* workspace, int B, int T, int U, int which);
int edgedict_ctc_loss_forward(const void* logits, int dtype, const int32_t* labels, const int32_t* act_lens,
                              const int32_t* label_lens, int B, int T, int U, int V, int blank, int zero_infinity,
                              float* costs, float* reduced, float reduce_scale, void* workspace, void* stream);
int edgedict_ctc_loss_backward(const void* logits, int dtype, void* grads, const int32_t* labels,
                               const int32_t* act_lens, const int32_t* label_lens, int B, int T, int U, int V,
                               int blank, const void* workspace, float grad_scale_host, const float* grad_scale_dev,
                               int grad_scale_stride, void* stream);
int edgedict_ctc_greedy(const void* logits, int dtype, const int32_t* act_lens, int B, int T, int V, int blank,
                        int32_t* tokens, int32_t* counts, int32_t* frames, float* neglogp, void* scratch,
                        void* stream);
int edgedict_ctc_align(const void* logits, int dtype, const int32_t* labels, const int32_t* act_lens,
                       const int32_t* label_lens, int B, int T, int U, int V, int blank, int32_t* frames,
                       int32_t* ends, float* scores, void* workspace, void* stream);

/* ------------------------------------------------------------------------------------
 * CTC scores of N-best lists (csrc/ctc_score.hip): the CTC log-likelihood of up to 32 hypotheses per utterance on the
 * head's logits - what rescoring the transducer's N-best lists with the head needs, without the loss's planes.
 *   logits   [B, T, V]  dtype     raw head logits, contiguous
 *   act_lens [B]        int32     frames per utterance (clamped to [0, T])
 *   hyps     [B, N, U]  int32     token sequences without blanks (nullable when U == 0); entries behind hyp_lens[b, n]
 *                                 and the slots n >= n_hyp[b] are never read
 *   hyp_lens [B, N]     int32     tokens per hypothesis (clamped to [0, U])
 *   n_hyp    [B]        int32     live slots per utterance (clamped to [0, N]); null: all N are live
 *   scores   [B, N]     fp64 out  ll of hyps[b, n, :hyp_lens[b, n]] over the frames t < act_lens[b], as the loss defines
 *                                 it (-cost); -inf for a hypothesis without a path (act_lens[b] <= 0, fewer frames than
 *                                 tokens + adjacent repeats, a token outside [0, V)) and for the slots n >= n_hyp[b]
 * Two launches: a row pass (log-sum-exp and lp[blank] per frame, once per utterance) and ONE wave per (b, n) that walks
 * the alpha recursion with the loss's arithmetic (fp64 carry) reading the labels' logits directly; nothing is stored
 * per lattice state.  No host sync, no atomics, bit-identical from run to run.  1 <= N <= 32, U <= 1023 (U == 0: every
 * hypothesis is empty and scores the sum of lp[blank]), V >= 2.  The workspace (16-byte aligned, scratch) holds two
 * [B, T] fp32 arrays: edgedict_ctc_score_workspace_bytes depends on B and T only (0 for arguments out of range).
 */
size_t edgedict_ctc_score_workspace_bytes(int B, int T, int N, int U);
int edgedict_ctc_score_nbest(const void* logits, int dtype, const int32_t* act_lens, const int32_t* hyps,
                             const int32_t* hyp_lens, const int32_t* n_hyp, int B, int T, int N, int U, int V,
                             int blank, double* scores, void* workspace, void* stream);

/* ------------------------------------------------------------------------------------
 * Batched edit distance (csrc/edit_distance.hip): the error counts of up to 32 hypotheses per utterance against the
 * utterance's reference - the integers every error rate is made of (the reference's validation loop, cli/train.py:
 * 273-319, takes its WER from a third-party package; edgedict_amd/metrics.py builds the rates on this).
 *   hyps     [B, N, Uh] int32     hypothesis tokens (nullable when Uh == 0); entries behind hyp_lens[b, n] and the slots
 *                                 n >= n_hyp[b] are never read.  Plain pairs: N = 1
 *   hyp_lens [B, N]     int32     tokens per hypothesis (clamped to [0, Uh])
 *   n_hyp    [B]        int32     live slots per utterance (clamped to [0, N]); null: all N are live
 *   refs     [B, Ur]    int32     reference tokens (nullable when Ur == 0); entries behind ref_lens[b] are never read
 *   ref_lens [B]        int32     tokens per reference (clamped to [0, Ur])
 *   out      [B, N, 4]  int32 out (dist, sub, del, ins); -1 in all four for the slots n >= n_hyp[b]
 * Symbols are compared with == only: every int32 value is a symbol.  d(i, j), the cheapest way to turn ref[:j] into
 * hyp[:i], has the integer edge costs hit 0, substitution K, deletion (a reference element without a hypothesis
 * element) K, insertion (a hypothesis element without a reference element) K + 1, K = 4096, d(0, j) = j K, d(i, 0) =
 * i (K + 1).  v = d(H, R): dist = v / K is the Levenshtein distance, ins = v % K the insertions of the minimum-distance
 * alignment with the FEWEST insertions (hence the fewest deletions and the most substitutions), del = ins - (H - R),
 * sub = dist - ins - del; hits = R - sub - del.
 * One launch, one wave64 per (b, n); no workspace, no host sync, no atomics, bit-identical from run to run.
 * B >= 1, 1 <= N <= 32, 0 <= Uh, Ur <= 1023; arguments are validated before anything is launched.
 */
int edgedict_edit_distance(const int32_t* hyps, const int32_t* hyp_lens, const int32_t* n_hyp, const int32_t* refs,
                           const int32_t* ref_lens, int B, int N, int Uh, int Ur, int32_t* out, void* stream);

/* ------------------------------------------------------------------------------------
 * The risk layer of MWER training (csrc/mwer.hip): the expected number of errors of an N-best list under its own
 * renormalised posterior, and its derivative with respect to every hypothesis' cost.
 *   costs      [B, N]  fp32      negative log-likelihood of every hypothesis, finite or +inf
 *   errs               int32     errors of every hypothesis, element (b N + n) * err_stride: err_stride 1 reads a
 *                                [B, N] array, 4 reads `dist` out of edgedict_edit_distance's [B, N, 4]
 *   n_hyp      [B]     int32     live slots per utterance (clamped to [0, N]); null: all N
 *   ref_costs  [B]     fp32      nullable: negative log-likelihood of the reference, for the nll_weight term of `reduced`
 *   risk       [B]     fp32 out  e_min + sum_n p_n d_n
 *   post       [B, N]  fp32 out  p
 *   coef       [B, N]  fp32 out  scale p_n (dbar - d_n) = d(scale risk[b]) / d costs[b, n]
 *   reduced    [1]     fp32 out  nullable: scale * sum_b (risk[b] + nll_weight * ref_costs[b]), the stored risk values
 *                                added in a fixed order in fp64; without ref_costs the second term is absent
 * Slot n is live iff n < n_hyp[b] and costs[b, n] < +inf.  Over the live slots, in fp64: m = min c, w = exp(-(c - m)),
 * p = w / sum w, e_min = min errs, d = errs - e_min (an integer difference), dbar = sum p d.  Dead slots have post =
 * coef = 0, an utterance without a live slot has risk 0; live hypotheses that all have the same error count give
 * coefficients of exactly 0.  One wave64 per utterance plus one wave for `reduced`; no workspace, no host sync, no
 * atomics, bit-identical from run to run.  B >= 1, 1 <= N <= 32, err_stride 1 or 4, B * N < 2^31; arguments are
 * validated before anything is launched (-1 with a message; needs no device).
 */
int edgedict_mwer_risk(const float* costs, const int32_t* errs, int err_stride, const int32_t* n_hyp,
                       const float* ref_costs, int B, int N, double nll_weight, double scale, float* risk, float* post,
                       float* coef, float* reduced, void* stream);

/* ------------------------------------------------------------------------------------
 * CTC prefix beam search on the head's logits (csrc/ctc_decode.hip states the search): per utterance the W best
 * prefixes after the last frame, ranked, with the frame each token's node was created on.  No prediction network and
 * no joint: a row pass over [B, T, V] (log-sum-exp, lp[blank], the sorted top-cand list per frame), one launch that
 * walks all frames of every utterance, one read-out launch.  No host sync; results bit-identical from run to run.
 *
 *   logits, dtype, act_lens, B, T, V, blank   as edgedict_ctc_greedy (rows t >= act_lens[b] are never read)
 *   W          beam width, 1 .. 32
 *   cand       candidates per frame, 1 .. 64: the min(cand, V - 1) most probable non-blank tokens of a frame are the
 *              only ones a prefix is extended with (ties: the lower token id)
 *   bias       nullable: a phrase automaton (edgedict_beam_bias_t above, bias->V == V).  A node carries the state after
 *              its token and the total Bn = sum of D(s, k) from the root; Bn enters the ranking and logp only.  The
 *              candidate list is cut BEFORE the bias is seen: a boosted token outside the top `cand` is not rescued.
 *   tokens, frames [B, W, T] int32, token_lp [B, W, T] fp32: hypothesis h's tokens root to leaf, the frame each was
 *              created on, log_softmax(logits[b, frame])[token]; -1 / -1 / 0 behind ntok[b, h]
 *   ntok [B, W] int32, n_hyp [B] int32 (hypotheses h >= n_hyp[b]: ntok 0, logp -inf)
 *   logp [B, W] fp64  logadd(pb, pnb) (+ Bn with a bias list), descending in h; act_lens[b] <= 0: the empty prefix, 0
 *   workspace  edgedict_ctc_beam_workspace_bytes(B, T, W, cand) bytes, 16-byte aligned (0 for arguments out of range)
 */
size_t edgedict_ctc_beam_workspace_bytes(int B, int T, int W, int cand);
int edgedict_ctc_beam_search(const void* logits, int dtype, const int32_t* act_lens, int B, int T, int V, int blank,
                             int W, int cand, const edgedict_beam_bias_t* bias, int32_t* tokens, int32_t* frames,
                             float* token_lp, int32_t* ntok, int32_t* n_hyp, double* logp, void* workspace,
                             void* stream);

/* ------------------------------------------------------------------------------------
 * Back-off n-gram language model in device tables (csrc/ngram_tables.hpp, csrc/ngram.hip; edgedict_amd/ngram.py
 * writes the tables).  Symbols are the ids 0 .. V-1 plus eos = V (tables only); <s> is the BOS id inside contexts; the
 * blank is no symbol.  A state is a context of 0 .. order-1 tokens, state 0 the empty one, `start` the state of (BOS).
 *   uni_lp, uni_next  [V + 1]  fp64 natural-log unigrams (blank: 0, never read) and the state after them
 *   row_ptr           [S + 1]  per state a row of arcs sorted by token; state 0's row is empty
 *   fail, backoff     [S]      the state of the context without its oldest token; the back-off weight (fp64)
 *   arc_tok, arc_lp, arc_next [n_arcs]
 * step(s, k), in exactly this order of fp64 additions:
 *   acc = 0;  repeat: s == 0: return acc + uni_lp[k], uni_next[k];  k in row(s): return acc + arc_lp, arc_next;
 *                     acc = acc + backoff[s]; s = fail[s]
 * The kernels clamp every state into [0, S), every row bound into [0, n_arcs], and leave the back-off loop after
 * `order` rounds: a corrupt table gives a wrong score, never a hang or an out-of-range read.  The pointers must not be
 * null (an empty table is a pointer to one element).  weight / length_bonus are read by the fused search only.
 * ngram_lm_struct_bytes: sizeof(edgedict_ngram_lm_t), for bindings that mirror it.
 */
typedef struct edgedict_ngram_lm_t {
    int V, order, S, n_arcs, start, blank;
    const double* uni_lp;
    const int32_t* uni_next;
    const int32_t* row_ptr;
    const int32_t* fail;
    const double* backoff;
    const int32_t* arc_tok;
    const double* arc_lp;
    const int32_t* arc_next;
    double weight, length_bonus;
} edgedict_ngram_lm_t;

size_t edgedict_ngram_lm_struct_bytes(void);
/* Dense rows: lp [R, V] fp32, lp[r][k] = (float)step(states[r], k), 0 in the blank column - the lp_lm row format of the
 * RNN-T searches; next [R, V] int32 (nullable): the state after k (blank column: the clamped state itself).
 * states [R] int32.  One wave per row; no atomics, results bit-identical from run to run. */
int edgedict_ngram_logprobs(const edgedict_ngram_lm_t* lm, const int32_t* states, int R, float* lp, int32_t* next,
                            void* stream);
/* Sentence scores in the N-best layout of edgedict_ctc_score_nbest: hyps [B, N, U] int32 (nullable when U == 0),
 * hyp_lens [B, N], n_hyp [B] (nullable: all N slots live).  total [B, N] fp64 = the sum of the steps in token order from
 * `start` (bos != 0) or state 0, then the eos step (eos != 0); -inf for a token outside [0, V) or the blank, and for the
 * slots behind n_hyp[b].  token_lp [B, N, U] fp32 (nullable): every step's value, 0 behind the hypothesis.  One wave per
 * hypothesis; a row is searched 64 arcs per load. */
int edgedict_ngram_score(const edgedict_ngram_lm_t* lm, const int32_t* hyps, const int32_t* hyp_lens,
                         const int32_t* n_hyp, int B, int N, int U, int bos, int eos, double* total, float* token_lp,
                         void* stream);

/* edgedict_ctc_beam_search with its options as a struct: the phrase automaton and / or an n-gram LM (both nullable, and
 * opts itself: null is {null, null}).  With an n-gram a prefix carries one LM state and the total
 * Ln = sum (weight * step + length_bonus) over its tokens; a new candidate ranks by (p + Bn) + Ln, a stay by
 * (logadd(pb, pnb) + Bn) + Ln, and logp is (tot + Bn) + Ln; pb / pnb stay pure CTC, the candidate cut stays ahead of
 * both terms, an extension that merges into an existing entry adds nothing.  ngram->V == V, ngram->blank == blank,
 * 1 <= order <= 6, S > 0, non-null tables, finite weight >= 0 and finite bonus, else ED_ERR_INVALID before any launch.
 * ngram = null launches the kernels of edgedict_ctc_beam_search; the workspace is the same. */
typedef struct edgedict_ctc_beam_opts_t {
    const edgedict_beam_bias_t* bias;
    const edgedict_ngram_lm_t* ngram;
} edgedict_ctc_beam_opts_t;
int edgedict_ctc_beam_search_fused(const void* logits, int dtype, const int32_t* act_lens, int B, int T, int V,
                                   int blank, int W, int cand, const edgedict_ctc_beam_opts_t* opts, int32_t* tokens,
                                   int32_t* frames, float* token_lp, int32_t* ntok, int32_t* n_hyp, double* logp,
                                   void* workspace, void* stream);

/* ------------------------------------------------------------------------------------
 * Streaming CTC prefix beam search: the search above for S streams whose head logits arrive chunk by chunk.  The beams
 * live in a persistent device STATE; after any number of advances a stream's state holds exactly the beam that
 * edgedict_ctc_beam_search_fused has after the same frames (same opts), bit for bit, and ctc_stream_nbest returns it.
 *
 * State per stream: the beam in ranked order (up to W entries of pb, pnb, bias total, LM total in fp64, and per entry
 * node, parent, last token, depth below the tree's root, automaton state, n-gram state), the entry count, the node count,
 * the frames since the reset, and the token tree: node_capacity (NC) nodes of int4 (parent, token, frame, lp bits), the
 * root in node 0.  The layout does not depend on opts.
 *
 *   ctc_stream_state_bytes(S, W, NC)                 device bytes of the state (contents undefined until a reset of
 *                                                    all streams); 0 for S <= 0, W outside 1 .. 32, NC < W
 *   ctc_stream_workspace_bytes(S, Tc, W, cand, NC)   device bytes of an advance over chunks of up to Tc frames; 0 for
 *                                                    bad shapes (also Tc <= 0, cand outside 1 .. 64)
 *   ctc_stream_reset    streams with mask[s] != 0 (mask: DEVICE int32 [S], null: all) -> the empty prefix alone: pb 0,
 *                       pnb -inf, totals 0, automaton state 0, opts->ngram's start state (0 without one), a tree of the
 *                       root, no frames.  One launch, no sync.
 *   ctc_stream_advance  stream s takes the first n_frames_host[s] (HOST int32 [S], 0 .. Tc) frames of logits [S, Tc, V]
 *                       (dtype code; rows behind are never read).  Three launches - the row pass of the offline search
 *                       on the chunk, the walk (one wave per stream, all frames inside the launch, the beam loaded
 *                       from and stored to the state, absolute frame numbers in new nodes), the compaction - then ONE
 *                       device-to-host read and one stream synchronisation.  The compaction (one wave per stream, no
 *                       atomics) finds the lowest common ancestor of the live entries' nodes, writes the tokens below
 *                       the old root down to it as commit records, makes it the root (node 0) and renumbers the nodes
 *                       a live entry still reaches densely, entries' node / parent renamed.
 *                         live_host   HOST int32 [S], in and out: the stream's tree nodes (1 after a reset, else what
 *                                     the previous advance wrote).  live[s] + n_frames[s] * W > NC is refused before
 *                                     anything is launched: nothing is ever truncated.
 *                         commit_host HOST [S][max_commit + 1] records of 16 bytes {int32, int32, float bits, 0}:
 *                                     record 0 = (tokens committed by this advance, live nodes, tokens of the stream's
 *                                     longest uncommitted hypothesis tail), records 1 .. = (token, frame since the
 *                                     reset, lp) root-side first.  max_commit >= max over s of
 *                                     min(NC, live[s] - 1 + n_frames[s]); NC always suffices.
 *   ctc_stream_nbest    the uncommitted part, as edgedict_ctc_beam_search's outputs on DEVICE arrays: tokens / frames
 *                       [S, W, max_tokens] int32 and token_lp fp32 (-1 / -1 / 0 behind ntok), ntok [S, W], n_hyp [S],
 *                       logp [S, W] fp64 = (logadd(pb, pnb) + Bn) + Ln, -inf behind n_hyp.  max_tokens >= 1 and
 *                       at least the longest tail the advances reported (a longer tail is cut to max_tokens).  One launch, no sync; the state is not
 *                       modified.  A whole hypothesis is the stream's commit records so far followed by this part.
 *
 * W, cand, dtype, V, blank, opts (bias list, n-gram: vocabulary and blank, tables, weight) are checked as by
 * edgedict_ctc_beam_search_fused, null and non-pointer arguments and NC < W too: ED_ERR_INVALID with a message naming
 * ctc_stream_*, before anything is launched.  state and workspace 16-byte aligned.  Results are bit-identical from run
 * to run.  The same opts must be given to the reset and to every advance of an utterance. */
size_t edgedict_ctc_stream_state_bytes(int S, int W, int node_capacity);
size_t edgedict_ctc_stream_workspace_bytes(int S, int Tc, int W, int cand, int node_capacity);
int edgedict_ctc_stream_reset(int S, int W, int node_capacity, const edgedict_ctc_beam_opts_t* opts, const int32_t* mask,
                              void* state, void* stream);
int edgedict_ctc_stream_advance(const void* logits, int dtype, const int32_t* n_frames_host, int S, int Tc, int V,
                                int blank, int W, int cand, int node_capacity, const edgedict_ctc_beam_opts_t* opts,
                                int32_t* live_host, void* commit_host, int max_commit, void* state, void* workspace,
                                void* stream);
int edgedict_ctc_stream_nbest(int S, int W, int node_capacity, const void* state, int max_tokens, int32_t* tokens,
                              int32_t* frames, float* token_lp, int32_t* ntok, int32_t* n_hyp, double* logp,
                              void* stream);

/* ------------------------------------------------------------------------------------
 * Blank-frame skipping ahead of the RNN-T beam searches (csrc/frame_skip.hip): the CTC head's blank posterior decides
 * which encoder frames a search sees.  No host sync inside either call, no atomics; results bit-identical from run to
 * run.
 *
 * edgedict_frame_skip_scan (two launches: a row pass, one wave per utterance for the compaction):
 *   logits, dtype, act_lens, B, T, V, blank   as edgedict_ctc_greedy (rows t >= act_lens[b] are never read)
 *   log_thr    (float)log(threshold) of a threshold in (0, 1], formed once on the host: finite, <= 0
 *   lp_blank   [B, T] fp32 out: min(logits[b,t,blank] - lse(logits[b,t,:]), 0) for t < act_lens[b], 0 behind
 *   frame_map  [B, T] int32 out: the original index of the j-th kept frame in ascending order, -1 behind kept[b];
 *              frame t < act_lens[b] is kept iff lp_blank[b,t] <= log_thr (log_thr = 0 keeps every frame)
 *   kept       [B] int32 out
 *
 * edgedict_frame_skip_gather (one launch):
 *   enc_out    [B, T, P] contiguous, dtype code; out [B, Tc, P] of the same dtype, 1 <= Tc <= T
 *   out[b,j,:] = enc_out[b, frame_map[b,j], :] for j < min(kept[b], Tc), zeros for the other rows (and for a map entry
 *   outside [0, T)).  16-byte copies when P * sizeof(dtype) is a multiple of 16 and both pointers are 16-byte aligned,
 *   element copies otherwise.
 * Limits: B <= 65535, B x T <= 2^31 - 1, V >= 2.
 */
int edgedict_frame_skip_scan(const void* logits, int dtype, const int32_t* act_lens, int B, int T, int V, int blank,
                             float log_thr, float* lp_blank, int32_t* frame_map, int32_t* kept, void* stream);
int edgedict_frame_skip_gather(const void* enc_out, int dtype, const int32_t* frame_map, const int32_t* kept, int B,
                               int T, int P, int Tc, void* out, void* stream);

/* ------------------------------------------------------------------------------------
 * Frame-synchronous batched RNN-T beam search (csrc/decode_sync.hip states the search): every hypothesis emits at most
 * one symbol per frame, all B x W hypotheses advance through one prediction-network step and one joint per frame, equal
 * token sequences are merged by log-add.  A second search beside edgedict_beam_search*, NOT the same algorithm: the two
 * do not return the same hypotheses.  A fixed list of launches per frame, no host synchronisation inside the frame
 * loop, no atomics; results are bit-identical from run to run.
 *
 *   operands   as edgedict_beam_search_nbest without max_expansions, prefix, expansions_host and detail
 *   W          beam width, 1 .. 32;  T > 0;  lens_host[b] in [0, T];  H a multiple of 4 (the LSTM kernels ask for 8)
 *   tokens_host / frames_host  HOST int32 [B, W, max_tokens]: hypothesis h's tokens root to leaf and the frame each
 *              token's node was created on;  token_logp_host HOST fp64 [B, W, max_tokens]: the token's log-softmax
 *              value on that frame (NOT an increment of logp: logp sums over alignments)
 *   ntokens_host HOST int32 [B, W];  nhyp_host HOST int32 [B] (= n <= W);  logp_host HOST fp64 [B, W], descending in h
 *              Entries behind n / behind a hypothesis' length are not written.  An utterance of 0 frames has one empty
 *              hypothesis with logp 0.  A hypothesis holds at most lens[b] tokens; one longer than max_tokens is an
 *              error, never a truncation.
 *   workspace  edgedict_sync_beam_workspace_bytes(...) bytes (0 for arguments out of range), 256-byte aligned
 *   result     edgedict_sync_beam_result_bytes(B, W, max_tokens) bytes on the device
 * Arguments are checked before anything is launched: a bad W, T <= 0, a null pointer give -1 and a message.
 * Synchronises the stream once, at the end.
 */
size_t edgedict_sync_beam_workspace_bytes(const edgedict_search_net_t* net, int B, int T, int W,
                                          const edgedict_search_opts_t* opts);
size_t edgedict_sync_beam_result_bytes(int B, int W, int max_tokens);
int edgedict_sync_beam_search(const edgedict_search_net_t* net, const void* E1, long long e_row_stride,
                              long long e_frame_stride, int B, int T, const int32_t* lens_host, int W,
                              int32_t* tokens_host, int32_t* frames_host, double* token_logp_host, int max_tokens,
                              int32_t* ntokens_host, int32_t* nhyp_host, double* logp_host,
                              const edgedict_search_opts_t* opts, void* workspace, void* result, void* stream);

/* ------------------------------------------------------------------------------------
 * Streaming form of the frame-synchronous search: the beams of S streams live in a persistent device STATE, so that
 * advancing over frames [0, t1) and then [t1, t2) leaves exactly the beam edgedict_sync_beam_search has after t2 frames,
 * and sync_stream_read after any advance returns what that search returns over the frames since the stream's reset.
 * Per stream the state holds the W rows (fp64 logp, token-tree node, sequence hash and length, last token), the rows'
 * prediction-network (h, c) [L][S*W][H] in two buffers (read / written alternately per frame), the token tree
 * (parent, token, frame, lp) [node_capacity] with its node count, the frames since the reset and the committed tokens.
 * A frame is the offline search's launches; a stream that is past its n_frames copies its rows' states through to the
 * other buffer, so every stream finds its states where the next frame reads.  After the last frame ONE launch per
 * advance compacts every stream's tree: the path from the root to the lowest common ancestor of the live rows' leaves
 * is COMMITTED (no later frame can change it) and returned, that ancestor becomes the root, the nodes still reachable
 * from a live leaf are renumbered densely.  The committed path is the TREE's common ancestor: a sequence that was
 * pruned and created again has a second node chain, so it can be shorter than the beam's common token prefix.
 *
 *   node_capacity  token-tree nodes per stream, >= W.  An advance adds at most n_frames[s] * W nodes to stream s:
 *                  one with live[s] + n_frames[s] * W > node_capacity fails before anything is launched
 *   sync_stream_state_bytes      device bytes of the state (contents undefined until a reset of all streams)
 *   sync_stream_workspace_bytes  device bytes of the per-call workspace of sync_stream_advance
 *   sync_stream_result_bytes     device bytes of sync_stream_read's result buffer
 *                  (all three: 0 for arguments out of range; buffers 256-byte aligned)
 *   sync_stream_reset    streams with mask[s] != 0 (mask null: all; mask_on_host: HOST int32 [S], else device) -> the
 *                  empty hypothesis, zero states, an empty tree, no frames, nothing committed
 *   sync_stream_advance  operands as edgedict_sync_beam_search; E1 holds this chunk's T frames per stream.
 *                  n_frames_host HOST int32 [S] in [0, T] (0: the stream sits the chunk out, its beam unchanged)
 *                  live_host   HOST int32 [S], in and out: every stream's live tree nodes - 0 after its reset, else
 *                              what the previous advance wrote
 *                  parity_host HOST int32, in and out: which state buffer holds the states; 0 before the first
 *                              advance on a state, then what the previous advance wrote (resets leave it alone)
 *                  commit_host HOST [S][1 + max_commit] records of 16 bytes {int32, int32, float, int32}: record 0 =
 *                              {tokens committed by this advance, live nodes, -, -}, record 1 + k = {token, frame
 *                              (counted from the stream's reset), the token's log-softmax value on that frame, -}.
 *                              max_commit >= min(node_capacity, max over s of live[s] + n_frames[s])
 *                  One device-to-host copy and one stream synchronisation, after the compaction; nothing inside the
 *                  frame loop waits for the host.  After an error other than an argument or capacity error the
 *                  advanced streams' state is undefined (reset them).
 *   sync_stream_read     as edgedict_sync_beam_search's outputs, for the UNCOMMITTED tails: ranked by logp descending
 *                  (ties keep beam order); a full hypothesis is the stream's committed log followed by its tail.
 *                  frames_host / token_logp_host are nullable (tokens only); entries behind a tail's length are
 *                  undefined.  ncommitted_host / nframes_host HOST int64 [S], nullable: committed tokens and frames
 *                  since the reset.  Does not modify the state.  A tail longer than max_tokens is an error (a tail holds at
 *                  most live[s] tokens).  Synchronises the stream.
 * Every entry point checks its arguments before any launch (W outside [1, 32], S <= 0, node_capacity < W, null
 * pointers, dtypes, blank / bos, n_frames, H % 4) and returns -1 with a message.
 */
size_t edgedict_sync_stream_state_bytes(const edgedict_search_opts_t* opts, int S, int L, int H, int W,
                                        int node_capacity);
size_t edgedict_sync_stream_workspace_bytes(const edgedict_search_net_t* net, int S, int W, int node_capacity,
                                            const edgedict_search_opts_t* opts);
size_t edgedict_sync_stream_result_bytes(int S, int W, int max_tokens);
int edgedict_sync_stream_reset(const edgedict_search_opts_t* opts, int S, int L, int H, int W, int node_capacity,
                               int bos, const int32_t* mask, int mask_on_host, void* state, void* stream);
int edgedict_sync_stream_advance(const edgedict_search_net_t* net, const void* E1, long long e_row_stride,
                                 long long e_frame_stride, int S, int T, const int32_t* n_frames_host, int W,
                                 int node_capacity, int32_t* live_host, int32_t* parity_host, void* commit_host,
                                 int max_commit, const edgedict_search_opts_t* opts, void* state, void* workspace,
                                 void* stream);
int edgedict_sync_stream_read(int S, int L, int H, int W, int node_capacity, const void* state, void* result,
                              int32_t* tokens_host, int32_t* frames_host, double* token_logp_host, int max_tokens,
                              int32_t* ntokens_host, int32_t* nhyp_host, double* logp_host,
                              long long* ncommitted_host, long long* nframes_host, void* stream);

/* ------------------------------------------------------------------------------------
 * LM shallow fusion and contextual biasing in the frame-synchronous search, offline and streaming: opts->lm and
 * opts->bias of the edgedict_sync_* entry points.  Either may be null, and with both null the calls ARE the plain ones
 * (same kernels, same layouts, same bits).
 *
 * Every row carries, beside its prediction-network state, the LM state from BEFORE its last token and the phrase
 * automaton's state s after its sequence (root: 0).  Per frame every row steps the LM on its last token - a row with
 * the empty sequence on lm->bos from a zero state - which gives fp32 LM logits; lp_lm is their log-softmax in the
 * formula of the RNN-T row.  Candidate (i, k) scores
 *   blank:      logp_i + (double)lp_i[blank]
 *   non-blank:  ((logp_i + (double)lp_i[k]) + (weight * (double)lp_lm_i[k] + length_bonus)) + (held[goto(s_i, k)] - pend[s_i])
 * in fp64, in this order, without contraction; a term is absent when its feature is.  Selection, merging and the final
 * ranking are the plain search's on these scores: a token child takes the LM state after its parent's token and the
 * state goto(s_i, k), a blank child or a folded pair keeps the parent's, a row left empty gets zeros and the root.
 * logp is the fused score; token_logp and frames are what the plain search returns (the RNN-T log-softmax value on the
 * node's creation frame).  No pending bonus is settled at the end of an utterance.  weight = length_bonus = 0 is
 * bit-equal to the plain search.  A frame is the plain search's launches plus the LM step on all B * W rows
 * (lm->L + 1 launches on the fused step); a bias list adds none.
 *
 *   sync_beam_workspace_bytes            the plain workspace + the LM step's buffers + the rows' LM (h, c) [lm->L][B*W][lm->H]
 *                                        in two buffers, the LM's next symbols and the automaton states
 *   sync_stream_state_bytes              the plain state with the rows' LM (h, c) in both buffers, the LM's next symbols
 *                                        and the automaton states APPENDED: edgedict_sync_stream_read serves every form.
 *                                        A state sized with an LM / a list must be reset and advanced with one
 *   sync_stream_workspace_bytes          the plain workspace + the LM step's buffers
 *   sync_stream_reset                    the plain reset; the selected streams' LM states are zeroed, their automaton
 *                                        states set to the root (the list may change at a reset)
 *   sync_stream_advance                  the plain advance on the fused scores; compaction is unchanged
 * Checked before anything is launched (-1 and a message): the LM's ntoken and the list's vocabulary equal V, lm->H a
 * multiple of 4, lm->bos inside the vocabulary, finite weight / length_bonus, non-null weights and tables, bias->S > 0.
 * The size queries return 0 for arguments out of range.
 */

/* ------------------------------------------------------------------------------------
 * Internal-LM estimation (ILME) in the frame-synchronous search, offline and streaming, and the internal LM as a scorer.
 * opts->ilm_weight (a HOST double, or null) of the edgedict_sync_* entry points switches it on; with ilm_weight null the
 * calls ARE the ones without it (same kernels, same layouts, same bits), and lm / bias may be null as there.
 *
 * For a row whose prediction-network output after its last token is d [P2], the internal LM's logits are the step's
 * joint on an all-zero encoder row, z_ilm = tanh(act(d W1d^T + b1)) W2^T + b2 (act: the rounding to the compute dtype),
 * and lp_ilm[k] = (z_ilm[k] - m) - log(sum_{v != blank} exp(z_ilm[v] - m)), m = max_{v != blank} z_ilm[v], in fp32.
 * A non-blank candidate's score is, in fp64 without contraction and in this order,
 *   c = logp_i + (double)lp_i[k];  c = c + (weight * (double)lp_lm_i[k] + length_bonus);
 *   c = c - ilm_weight * (double)lp_ilm_i[k];  c = c + (held[goto(s_i, k)] - pend[s_i])
 * (a term is absent when its feature is); blank keeps logp_i + lp_i[blank]; token_logp stays lp_i[k].  ilm_weight = 0
 * runs the ILME kernels and is bit-equal to the call without it.  ILME carries no per-row state: the persistent state
 * of a stream, its reset and its read take no part in it.  Launches per frame: on the fused step none more (one
 * joint-hidden kernel writes both hidden vectors, the logits kernel runs on 2 B W rows); on the composed step two more.
 *
 *   sync_beam_workspace_bytes / sync_stream_workspace_bytes   the size without it + ILME's buffers (hidden vectors
 *                                        [2 rows, J], fp32 logits [2 rows, V], a zero encoder row)
 * Checked before anything is launched (-1 and a message): ilm_weight finite and >= 0.  The size queries return 0 then.
 *
 *   ilm_workspace_bytes(dtype, R, J)     scratch of ilm_logits for R rows (0 for arguments out of range)
 *   ilm_logits      logits fp32 [R, V] = z_ilm of R rows `dec` [R, P2] (compute dtype), by the kernels the search's step
 *                   uses for a network of these widths (emb_dtype, E, H pick the route as they do there)
 *   ilm_logprobs    out fp32 [B, U]: lp_ilm[b, u][targets[b, u]] from logits [B * U, V] for u < ylen[b], exactly 0
 *                   behind it (targets int32 [B, U], ylen int32 [B], both on the device).  A blank target gives -inf, one
 *                   outside the vocabulary NaN.  One wave per row, no atomics: the same bits every run.
 */
size_t edgedict_ilm_workspace_bytes(int dtype, int R, int J);
int edgedict_ilm_logits(int dtype, const void* dec, int R, int P2, int J, const void* W1d, long long ldw1,
                        const float* b1, const void* W2, const float* b2, int V, int emb_dtype, int E, int H,
                        float* logits, void* workspace, void* stream);
int edgedict_ilm_logprobs(const float* logits, const int32_t* targets, const int32_t* ylen, int B, int U, int V,
                          int blank, float* out, void* stream);

/* ------------------------------------------------------------------------------------
 * The back-off n-gram LM in the frame-synchronous search, offline and streaming: opts->ngram (an edgedict_ngram_lm_t,
 * above; null: the calls without it, same kernels, same layouts, same bits) of the edgedict_sync_* entry points.
 * opts->lm and opts->ngram both non-null is an argument error: one LM at a time.  bias and ilm_weight combine with it.
 *
 * A row carries ONE int32 n-gram state s: the state AFTER its token sequence (the phrase automaton's convention, not
 * the LSTM's); the empty sequence stands on ngram->start, the context (BOS).  A non-blank candidate scores, in fp64
 * without contraction and in this order,
 *   c = logp_i + (double)lp_i[k];  c = c + (weight * step(s_i, k) + length_bonus);
 *   c = c - ilm_weight * (double)lp_ilm_i[k];  c = c + (held[goto(a_i, k)] - pend[a_i])
 * (a term is absent when its feature is), step(s, k) the fp64 value of the chain of additions stated with
 * edgedict_ngram_lm_t - never rounded through fp32, so the n-gram term is the host's bit for bit.  Blank keeps
 * logp_i + lp_i[blank]; token_logp stays lp_i[k].  A token child takes next(s_i, k), a blank child or a folded pair the
 * parent's state, a row left without a hypothesis `start`.  weight = length_bonus = 0 is bit-equal to the plain search
 * (every table value finite).
 *
 * No launch and no [B W, V] buffer more per frame: the per-row top-W kernel builds the row's image (step(s_i, .) fp64 [V]
 * and next(s_i, .) int32 [V], 12 bytes a symbol) in dynamic LDS from the back-off chain of s_i - the unigram level first,
 * then every longer context's arcs over it, a barrier between levels - and writes, beside a kept candidate's score and
 * token, its next state (int32 [B W][W], workspace); the select kernel reads that and keeps a per-row ng_st [B W].
 * V <= 5376: the image and the kernel's static LDS fit the 64 KiB a launch gets.
 *
 *   sync_beam_workspace_bytes            the size without it + ng_st [B W] behind the fused rows' part + the candidates'
 *                                        next states [B W][W] behind everything else
 *   sync_stream_state_bytes              ng_st [S W] APPENDED behind the fused rows' part: every other offset holds
 *   sync_stream_workspace_bytes          the size without it + the candidates' next states
 *   sync_stream_reset                    the selected streams' rows back on `start`
 * Checked before anything is launched (-1 and a message that the entry point's name leads; size queries: 0, and the
 * reason is left in edgedict_last_error): the rules of edgedict_ngram_logprobs for the struct, ngram->V == V and
 * ngram->blank == blank (the reset and the state query know neither: the advance checks), weight finite and >= 0,
 * length_bonus finite, V <= 5376, lm and ngram not both set.  lm->bos has no counterpart: nothing but `start` is read.
 */

/* ------------------------------------------------------------------------------------
 * Confidence of N-best hypotheses (csrc/confidence.hip): the two kernels of a post-pass over the lists any search
 * returned.  The caller re-evaluates the joint at every token's (encoder frame, prefix) - conf_hidden_rows between two
 * edgedict_gemm calls - or takes the CTC head's logits, and conf_row_stats reduces each row of logits to five
 * statistics of the acoustic model's output distribution over all V symbols, the blank included.  LM and bias terms
 * take no part.  Nothing is allocated, nothing synchronises, no atomics: the same bits on every run.
 *
 *   conf_hidden_rows  hid [R, J] (dtype) = tanh(E1[enc_row[r], :] + D1[dec_row[r], :] + b1): E1 [n_enc_rows, J] and
 *                     D1 [n_dec_rows, J] contiguous in dtype, b1 fp32 [J] or null (nothing is added: D1 then already
 *                     holds the bias, as the search step's first product does), enc_row / dec_row int32 [R] on the
 *                     device.  The sum is formed in fp32 from the stored operands and hid is rounded once: the rounding
 *                     points of the search's composed step.  16-byte loads and stores when J is a multiple of the 16-byte
 *                     width and the three pointers are 16-byte aligned, element by element otherwise.  A row whose
 *                     index lies outside [0, n_enc_rows) / [0, n_dec_rows) is written as NaN and nothing is read for it.
 *   conf_row_stats    logits [n_logit_rows, ld] in dtype (fp32 or bf16; ld >= V elements between rows; what lies behind
 *                     column V is never read), rows int32 [R] or null (row r reads logits row rows[r]; null: row r, and
 *                     R <= n_logit_rows), tokens int32 [R], 0 < alpha < 1.  One wave per row, 4 per workgroup; a row of
 *                     V <= 2048 is read once into registers, a longer one once per pass.  In fp32, with m = max z,
 *                     s = sum e^(z - m), a = sum e^(z - m) (z - m), q = sum e^(alpha (z - m)) (a -inf logit adds exactly
 *                     0 to all three), stats fp32 [R, 5] =
 *                       { logp = (z[tokens[r]] - m) - log s,  logp_max = -log s,  logp_blank = (z[blank] - m) - log s,
 *                         H = log s - a / s  (Shannon entropy, nats),  log sum_v p_v^alpha = log q - alpha log s }
 *                     and top int32 [R] = arg max z, the lowest index on ties.  A token outside [0, V) gives NaN in logp
 *                     only.  A row that holds a NaN or nothing above -inf, and a rows[r] outside [0, n_logit_rows) (for
 *                     which nothing is read), give five NaN and top = -1; other rows are not affected.
 * Checked before the launch (-1 and a message): dtype, R > 0, J > 0, V >= 2, ld >= V, blank inside [0, V), alpha inside
 * (0, 1), null pointers.
 */
int edgedict_conf_hidden_rows(int dtype, const void* E1, int n_enc_rows, const void* D1, int n_dec_rows, const float* b1,
                              const int32_t* enc_row, const int32_t* dec_row, int R, int J, void* hid, void* stream);
int edgedict_conf_row_stats(const void* logits, int dtype, long long ld, int n_logit_rows, const int32_t* rows,
                            const int32_t* tokens, int R, int V, int blank, float alpha, float* stats, int32_t* top,
                            void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EDGEDICT_HIP_H */
