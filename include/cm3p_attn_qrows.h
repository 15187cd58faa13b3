/*
 * cm3p_attn_qrows.h - attention for a LIST of query rows against all keys: an extension ABI of libcm3p_hip.so next to cm3p_hip.h.
 *
 * Where only some rows of an encoder's last layer are consumed - the pooled CLS row of each sequence and the rows that carry a
 * masked-LM label - that layer needs attention for those queries only, against every key.  These entry points are that attention,
 * forward and backward, on the matrix cores (v_mfma_f32_32x32x16_bf16), under the contract cm3p_hip.h states for cm3p_attn_fwd /
 * cm3p_attn_bwd (and their _varlen forms): the same function of the same qkv buffer, restricted to the listed queries ("same" is the
 * same function, not the same bits).  head_dim 64 only.  Kernels: csrc/attention_qrows.hip.  Python binding: cm3p_amd/_lib.py
 * QROWS_SIGNATURES; see INTEGRATION.md.
 *
 * Conventions: those of cm3p_hip.h (plain C types, CM3P_OK or a negative CM3P_ERR_* code, nothing allocates or synchronises, "bf16"
 * buffers are raw uint16 bit patterns).  qkv, out, dout, dqkv, lse and the rotary tables must be 16-byte aligned; cu_seqlens, qrows
 * and qcu 4-byte.
 *
 *   qkv:   [B, S, 3, nh, 64] bf16, q and k already rotated, `total` = B * S rows.  Packed form (cu_seqlens != NULL):
 *          [total, 3, nh, 64]; sequence b owns rows cu_seqlens[b] .. cu_seqlens[b + 1] - 1 (int32, B + 1 entries on the device,
 *          cu_seqlens[0] = 0 and cu_seqlens[B] = total: the sequences cover every row), S is max_seqlen, and there is no key mask.
 *   qrows: int32 [n], GLOBAL row numbers into the row axis of qkv (b * S + pos, or the packed row), strictly ascending.
 *   qcu:   int32 [B + 1]: sequence b owns qrows[qcu[b] .. qcu[b + 1] - 1] - possibly none -, every one of them a row of sequence b.
 *   qmax:  the largest per-sequence count (it sizes the grid; a sequence's queries beyond qmax would not be computed).
 *   key kv is visible to the query at position pos_q of its sequence iff
 *          key_mask[b, kv] != 0 (key_mask [B, S] bytes, or NULL)  AND  (window < 0  OR  |pos_q - kv| <= window).
 *          pos_q is the query's POSITION (qrows[i] minus the sequence's first row), not its index in the list.  A query whose own
 *          key_mask byte is 0 is computed like any other.  A query with no visible key gives exact zeros and lse = +inf.
 *   q_prescaled != 0: the q third holds q * scale * log2(e) (cm3p_qkv_gemm_rope with that q_scale) and the kernels skip the scaling;
 *          q_prescaled == 0: plain q, scale * log2(e) is applied in fp32 to the score.  `scale` is always the softmax scale.
 *
 * The kernels TRUST qrows and qcu (the caller validates them: cm3p_amd.encoder does it with the one host read that gives n and qmax);
 * what they read from them is clamped into the sequence before an address is formed, so a wrong list gives wrong numbers, not a
 * read or write outside the buffers.  Every row offset is a 64-bit product.
 *
 * Every refusal answers CM3P_ERR_INVALID before any HIP call: a NULL or misaligned pointer (out, lse, dout and qrows may be NULL
 * when n == 0: they are not read); B, S or nh <= 0; n < 0; qmax <= 0 with n > 0; total <= 0; a key mask together with cu_seqlens;
 * one rotary table without the other; pos_batch_stride other than 0 or S; scale not above 0.
 * n == 0 is valid: the forward launches nothing, the backward writes an all-zero dqkv.
 */
#ifndef CM3P_ATTN_QROWS_H
#define CM3P_ATTN_QROWS_H

#include <stdint.h>

#include "cm3p_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Version of this header; cm3p_attn_qrows_abi_version() must return it.  (cm3p_hip.h's own version does not move with this file.) */
#define CM3P_ATTN_QROWS_ABI_VERSION 1
int cm3p_attn_qrows_abi_version(void);

/* Forward.  out: [n, nh, 64] bf16 and lse: [nh, n] fp32 (the natural-log sum-exp of the scaled scores of the visible keys), compact,
 * in qrows order.  Scores, their running maximum and the sum of exponentials are fp32; p is rounded to bf16 as the MFMA operand of
 * the p v product, as in cm3p_attn_fwd.  The reduction order is fixed: equal inputs give equal bits. */
int cm3p_attn_qrows_fwd(const void* qkv, void* out, float* lse, const uint8_t* key_mask, const int* cu_seqlens, const int* qrows,
                        const int* qcu, int n, int qmax, int B, int S, int64_t total, int nh, int window, float scale, int q_prescaled,
                        void* stream);

/* Backward.  out / lse: what the forward stored; dout: [n, nh, 64] bf16.  dqkv: the FULL layout of qkv, [B, S, 3, nh, 64] (or
 * [total, 3, nh, 64]) bf16, every element overwritten:
 *   q third: exact zeros except on the listed rows, which hold dq = scale * sum_kv dS[q, kv] k[kv] - the gradient w.r.t. the
 *            UN-scaled rotated q in both q_prescaled modes, as cm3p_attn_bwd stores it;
 *   k third: dk[kv] = scale * sum_q dS[q, kv] q;    v third: dv[kv] = sum_q p[q, kv] dO[q] - sums over the LISTED queries only;
 *            invisible and padded keys: exact zeros,
 * with p = exp(score - lse), dS = p * (dO . v[kv] - delta) and delta = sum_d dO[d] * out[d] taken from the stored bf16 `out` (both
 * kernels of the backward form it with the same instructions: one delta, equal bits).  p and dS are rounded to bf16 as MFMA operands,
 * as in cm3p_attn_bwd.  If cos_tab / sin_tab ([n_pos, 32] fp32) are not NULL the inverse rotary rotation is applied to dq and dk
 * before the store; the table row of position pos of sequence b is b * pos_batch_stride + pos (pos_batch_stride 0 or S), in the
 * packed form the token's own row (per-token tables; pos_batch_stride is ignored).  Fixed reduction order, no atomics, no workspace. */
int cm3p_attn_qrows_bwd(const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv, const uint8_t* key_mask,
                        const int* cu_seqlens, const int* qrows, const int* qcu, int n, int qmax, int B, int S, int64_t total, int nh,
                        int window, float scale, const float* cos_tab, const float* sin_tab, int64_t pos_batch_stride, int q_prescaled,
                        void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CM3P_ATTN_QROWS_H */
