/*
 * cm3p_mlm_topk.h - masked-LM top-k predictions without the logits tensor: an extension ABI of libcm3p_hip.so next to cm3p_hip.h and
 * ext/cm3p_mlm_loss.h.
 *
 * What this entry point replaces is the prediction / evaluation path of the masked-LM head: the decoder GEMM that writes fp32 logits
 * [T, Vp] (cm3p_gemm_bf16 with CM3P_EPI_F32 / CM3P_EPI_F32_BIAS) followed by argmax / top-k over them (masked-token prediction,
 * fill-mask, the masked-LM accuracy and top-5 accuracy of an evaluation loop).  Here the decoder's logit tiles
 *     x[r, c] = sum_k y[r, k] * W[c, k] (+ bias[c])       bf16 MFMA, fp32 accumulation, the bias added in fp32 afterwards
 * are consumed where they are computed: each 128-column tile leaves its k best columns and its (max, sum exp) pair per row, and a
 * second kernel merges the tiles.  No logit is stored.
 * Python binding: cm3p_amd/_lib.py MLM_TOPK_SIGNATURES; see INTEGRATION.md.
 *
 * Conventions: those of ext/cm3p_mlm_loss.h (plain C types, device pointers 16-byte aligned, CM3P_OK or a negative CM3P_ERR_* code,
 * nothing allocates or synchronises, "bf16" buffers are raw uint16 bit patterns):
 *   y [T, H] bf16 (the head's LayerNorm output), W [Vp, H] bf16 (the decoder weight, rows [V, Vp) padding), bias [Vp] fp32 or NULL,
 *   T >= 0 (0 launches nothing), H a multiple of 8, Vp a multiple of 64, 1 <= V <= Vp, 1 <= k <= 8.
 *   Every row is live: the caller selects the rows it wants predictions for, there is no label argument.
 *   Columns [V, Vp) take no part, whatever W and bias hold there.
 * NULL pointers (bias excepted), k outside 1..8, V > Vp, a shape outside the above, a misaligned buffer and an undersized workspace
 * answer CM3P_ERR_INVALID before any HIP call.  Equal inputs give equal bits (fixed orders, no atomics); row offsets are 64-bit.
 * Finite logits are assumed: the rank of a NaN logit is unspecified (it is never used as an index, and nothing outside the buffers
 * is read or written because of it).
 */
#ifndef CM3P_MLM_TOPK_H
#define CM3P_MLM_TOPK_H

#include <stdint.h>

#include "../../cm3p_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Version of this header; cm3p_mlm_topk_abi_version() must return it.  (cm3p_hip.h's own version does not move with this file.) */
#define CM3P_MLM_TOPK_ABI_VERSION 1
int cm3p_mlm_topk_abi_version(void);

/* ---------------------------------------------------------------------------------------------------------------
 * top_idx [T, k] int32 / top_val [T, k] fp32: the k columns c < V with the largest x[r, c], ordered by (value descending, column
 * ascending), and their fp32 logits.  Equal values - +0.0 and -0.0 are equal - rank the lower column first: argmax's first-maximum
 * rule extended to k.  When V < k, slots V .. k - 1 hold index -1 and value -inf.
 * lse_rows [T] fp32 = log sum_{c < V} exp(x[r, c]) by the fold of cm3p_mlm_lse: per 128-column tile (M, S) = (max x, sum exp(x - M)),
 * then lse = M + log(sum_t S_t exp(M_t - M)), M = max_t M_t, the tiles in ascending order.
 * Per (128-column tile, row) the tile's k candidates (value, column), found in k rounds of "largest remaining element, lowest column on
 * a tie", and the (M, S) pair go to the workspace; the second kernel merges the tiles in ascending order under the same ordering rule.
 * ws: at least cm3p_mlm_topk_workspace_bytes(T, Vp, k) bytes (ws_bytes: what the caller passes; checked).
 */
int cm3p_mlm_topk(const void* y, const void* W, const float* bias, int64_t T, int64_t H, int64_t V, int64_t Vp, int k,
                  int32_t* top_idx, float* top_val, float* lse_rows, void* ws, int64_t ws_bytes, void* stream);

/* Host-only: T * ceil(Vp / 128) * (k + 1) * 8 bytes - k (value, column) pairs and one (M, S) pair per (tile, row); with Vp a
 * multiple of 128 and k = 8 that is T * Vp * 9 / 16 bytes, 14 % of the fp32 logits.  A negative CM3P_ERR_* code for T < 0, a Vp that is no positive
 * multiple of 64 or k outside 1..8. */
int64_t cm3p_mlm_topk_workspace_bytes(int64_t T, int64_t Vp, int k);

#ifdef __cplusplus
}
#endif
#endif /* CM3P_MLM_TOPK_H */
