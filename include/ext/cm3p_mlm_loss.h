/*
 * cm3p_mlm_loss.h - the masked-LM loss without the logits tensor: an extension ABI of libcm3p_hip.so next to cm3p_hip.h.
 *
 * What these entry points replace is the training path of cm3p_hip.h's masked-LM head: the decoder GEMM that writes fp32 logits
 * [T, Vp] (cm3p_gemm_bf16 with CM3P_EPI_F32 / CM3P_EPI_F32_BIAS), cm3p_ce_masked_stats and cm3p_ce_masked_dlogits_bf16 that read them
 * (CM3PPredictionHead's decoder + ForMaskedLMLoss; ref:cm3p/modeling_cm3p.py:987-996,1229-1238, TF:loss/loss_utils.py:32-46,74-91).
 * Here the decoder's logit tiles
 *     x[r, c] = sum_k y[r, k] * W[c, k] (+ bias[c])       bf16 MFMA, fp32 accumulation, the bias added in fp32 afterwards
 * are consumed where they are computed, once for the row statistics and once more for the gradient; no logit is stored.
 * Python binding: cm3p_amd/_lib.py MLM_LOSS_SIGNATURES; see INTEGRATION.md.
 *
 * Conventions: those of cm3p_hip.h (plain C types, device pointers 16-byte aligned, CM3P_OK or a negative CM3P_ERR_* code, nothing
 * allocates or synchronises, "bf16" buffers are raw uint16 bit patterns).  Shared arguments:
 *   y [T, H] bf16 (the head's LayerNorm output), W [Vp, H] bf16 (the decoder weight, rows [V, Vp) padding), bias [Vp] fp32 or NULL,
 *   target [T] int64, T >= 0 (0 launches nothing), H a multiple of 8, Vp a multiple of 64, 1 <= V <= Vp.
 *   A row is live when its label differs from ignore_index and lies in [0, V) - the rule of cm3p_ce_masked_stats; every other label is
 *   compared, never used as an index.  Columns [V, Vp) take no part, whatever W and bias hold there.
 * NULL pointers (bias excepted), V > Vp, a shape outside the above, a misaligned buffer and an undersized workspace answer
 * CM3P_ERR_INVALID before any HIP call.  Equal inputs give equal bits (fixed reduction orders, no atomics).  A 128-row tile without
 * a live row runs no matrix product.
 */
#ifndef CM3P_MLM_LOSS_H
#define CM3P_MLM_LOSS_H

#include <stdint.h>

#include "../cm3p_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Version of this header; cm3p_mlm_loss_abi_version() must return it.  (cm3p_hip.h's own version does not move with this file.) */
#define CM3P_MLM_LOSS_ABI_VERSION 1
int cm3p_mlm_loss_abi_version(void);

/* ---------------------------------------------------------------------------------------------------------------
 * Replaces the decoder GEMM + cm3p_ce_masked_stats: lse_rows[r] = log sum_{c < V} exp(x[r, c]), loss_rows[r] = lse_r - x[r, target_r]
 * for live rows, both exact 0 for the others.  Per (128-column vocabulary tile, row) one pair (M, S) = (max x, sum exp(x - M)) over the
 * tile's columns below V goes to the workspace; a second kernel folds the pairs in ascending tile order,
 * lse = M + log(sum_t S_t exp(M_t - M)), M = max_t M_t.
 * ws: at least cm3p_mlm_lse_workspace_bytes(T, Vp) bytes (ws_bytes: what the caller passes; checked).
 */
int cm3p_mlm_lse(const void* y, const void* W, const float* bias, const int64_t* target, int64_t ignore_index, int64_t T, int64_t H,
                 int64_t V, int64_t Vp, float* loss_rows, float* lse_rows, void* ws, int64_t ws_bytes, void* stream);

/* Host-only: T * ceil(Vp / 128) * 8 bytes (at most T * Vp / 8); a negative CM3P_ERR_* code for T < 0 or a Vp that is no positive
 * multiple of 64. */
int64_t cm3p_mlm_lse_workspace_bytes(int64_t T, int64_t Vp);

/* ---------------------------------------------------------------------------------------------------------------
 * Replaces cm3p_ce_masked_dlogits_bf16 (same output contract) without its logits argument: recomputes each tile and writes
 *     dlogits_bf16[r, c] = bf16(s * (exp(x[r, c] - lse_rows[r]) - [c == target_r])),   s = scale_a[0] * scale_b[0] (device scalars)
 * for live rows and c < V, exact zeros for every other row and for the pad columns: all of [T, Vp] (row pitch Vp, 64-bit offsets) is
 * written.  colsum[c] (fp32 [Vp]) = sum_r of the unrounded values in a fixed order - inside a 128-row tile the lane's 4 rows, 16
 * lanes, two waves; then the row tiles ascending; accumulate != 0 adds that sum to what colsum holds (row chunks of one batch),
 * accumulate == 0 overwrites.  lse_rows: what cm3p_mlm_lse wrote for these rows.
 * ws: at least cm3p_mlm_dlogits_workspace_bytes(T, Vp) bytes (the per-row-tile column sums; checked against ws_bytes).
 */
int cm3p_mlm_dlogits(const void* y, const void* W, const float* bias, const int64_t* target, int64_t ignore_index, const float* lse_rows,
                     const float* scale_a, const float* scale_b, int64_t T, int64_t H, int64_t V, int64_t Vp, void* dlogits_bf16, float* colsum,
                     int accumulate, void* ws, int64_t ws_bytes, void* stream);

/* Host-only: ceil(T / 128) * Vp * 4 bytes; a negative CM3P_ERR_* code as above. */
int64_t cm3p_mlm_dlogits_workspace_bytes(int64_t T, int64_t Vp);

#ifdef __cplusplus
}
#endif
#endif /* CM3P_MLM_LOSS_H */
