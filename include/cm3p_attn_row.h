/*
 * cm3p_attn_row.h - single-query attention for the pooled CLS row: an extension ABI of libcm3p_hip.so next to cm3p_hip.h.
 *
 * Where the pooled output h[:, 0] is the only consumer of an encoder's last layer, that layer needs attention for ONE query per
 * sequence - position 0 - against every key.  These entry points are that attention, forward and backward, under the contract
 * cm3p_hip.h states for cm3p_attn_fwd / cm3p_attn_bwd (and their _varlen forms): the same function of the same qkv buffer,
 * restricted to query row 0.  Kernels: csrc/attention_row.hip.  Python binding: cm3p_amd/_lib.py ROW_SIGNATURES; see INTEGRATION.md.
 *
 * Conventions: those of cm3p_hip.h (plain C types, CM3P_OK or a negative CM3P_ERR_* code, nothing allocates or synchronises, "bf16"
 * buffers are raw uint16 bit patterns).  qkv, out, dout, dqkv, lse and the rotary tables must be 16-byte aligned; cu_seqlens 4-byte.
 *
 *   qkv: [B, S, 3, nh, 64] bf16, q and k already rotated.  Packed form (cu_seqlens != NULL): [total, 3, nh, 64]; sequence b owns rows
 *        cu_seqlens[b] .. cu_seqlens[b + 1] - 1 (int32, B + 1 entries on the device), S is max_seqlen, and there is no key mask.  The
 *        query of sequence b is its first row; a sequence of length 0 has none (forward: zeros and lse = +inf; backward: nothing to write).
 *   key kv is visible iff  key_mask[b, kv] != 0 (key_mask [B, S] bytes, or NULL)  AND  (window < 0  OR  kv <= window).
 *        The query at position 0 is computed like any other query, also where key_mask[b, 0] == 0.
 *   q_prescaled != 0: the q third holds q * scale * log2(e) (cm3p_qkv_gemm_rope with that q_scale) and the kernels skip the scaling;
 *        q_prescaled == 0: plain q, scale * log2(e) is applied in fp32 to the score.  `scale` is always the softmax scale.
 *
 * Every refusal answers CM3P_ERR_INVALID before any HIP call: a NULL or misaligned pointer; B, S or nh <= 0; scale not above 0; a key
 * mask together with cu_seqlens; cu_seqlens with total <= 0; one rotary table without the other; pos_batch_stride other than 0 or S.
 */
#ifndef CM3P_ATTN_ROW_H
#define CM3P_ATTN_ROW_H

#include <stdint.h>

#include "cm3p_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Version of this header; cm3p_attn_row_abi_version() must return it.  (cm3p_hip.h's own version does not move with this file.) */
#define CM3P_ATTN_ROW_ABI_VERSION 1
int cm3p_attn_row_abi_version(void);

/* Forward.  out: [B, nh, 64] bf16; lse: [B, nh] fp32, the natural-log sum-exp of the scaled scores of the visible keys.  A query
 * with no visible key gives exact zeros and lse = +inf.  Scores, their maximum, the sum of exponentials and the sum of p * v are
 * fp32; p is NOT rounded to bf16 before it multiplies v.  The reduction order is fixed: equal inputs give equal bits. */
int cm3p_attn_row_fwd(const void* qkv, void* out, float* lse, const uint8_t* key_mask, const int* cu_seqlens, int B, int S,
                      int64_t total, int nh, int window, float scale, int q_prescaled, void* stream);

/* Backward.  out / lse: what the forward stored; dout: [B, nh, 64] bf16.  dqkv: the FULL layout of qkv, [B, S, 3, nh, 64] (or
 * [total, 3, nh, 64]) bf16, every element overwritten:
 *   q third: exact zeros except on the query rows, which hold dq = scale * sum_kv dS[kv] k[kv] - the gradient w.r.t. the UN-scaled
 *            rotated q in both q_prescaled modes, as cm3p_attn_bwd stores it;
 *   k third: dk[kv] = scale * dS[kv] * q;      v third: dv[kv] = p[kv] * dO;      invisible and padded keys: exact zeros,
 * with p[kv] = exp(score[kv] - lse), dS[kv] = p[kv] * (dO . v[kv] - delta) and delta = sum_d dO[d] * out[d] taken from the stored
 * bf16 `out`.  If cos_tab / sin_tab ([n_pos, 32] fp32) are not NULL the inverse rotary rotation is applied to dq and dk before the
 * store; the table row of key kv of sequence b is b * pos_batch_stride + kv (pos_batch_stride 0 or S), in the packed form the
 * token's own row (per-token tables; pos_batch_stride is ignored).  Fixed reduction order, no atomics. */
int cm3p_attn_row_bwd(const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv, const uint8_t* key_mask,
                      const int* cu_seqlens, int B, int S, int64_t total, int nh, int window, float scale, const float* cos_tab,
                      const float* sin_tab, int64_t pos_batch_stride, int q_prescaled, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CM3P_ATTN_ROW_H */
