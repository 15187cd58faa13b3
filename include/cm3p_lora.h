/*
 * cm3p_lora.h - low-rank adapters (LoRA) on the fused encoder stack: the extension ABI of libcm3p_hip.so next to cm3p_hip.h.
 *
 * The reference has no adapters; what these entry points restate is the usual definition W_eff = W + s B A (s = alpha / r) of a
 * low-rank update of an nn.Linear weight W [N, K] with A [r, K] and B [N, r], specialised to this stack: the adapter is folded
 * into the bf16 copy every training step makes of W anyway (cm3p_cast_f32_bf16_t_multi), so every GEMM runs unchanged, and only
 * the adapter gradients are new work (cm3p_lora_grad).  Python binding: cm3p_amd/_lib.py EXT_SIGNATURES; see INTEGRATION.md.
 *
 * Conventions: those of cm3p_hip.h (plain C types, device pointers 16-byte aligned, CM3P_OK or a negative CM3P_ERR_* code, nothing
 * allocates or synchronises, "bf16" buffers are raw uint16 bit patterns).  r is one of 8, 16, 32, 64.  Null pointers and an
 * unsupported r answer CM3P_ERR_INVALID before any HIP call.
 */
#ifndef CM3P_LORA_H
#define CM3P_LORA_H

#include <stdint.h>

#include "cm3p_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Version of this header; cm3p_lora_abi_version() must return it.  (cm3p_hip.h's own version does not move with this file.) */
#define CM3P_LORA_ABI_VERSION 1
int cm3p_lora_abi_version(void);

/* ---------------------------------------------------------------------------------------------------------------
 * Merged cast: the adapted form of cm3p_cast_f32_bf16_t_multi.  For n matrices in ONE launch
 *     out[nrow, k] = bf16_rne(W[nrow, k] + s * sum_{j < r} B[nrow, j] * A[j, k])      out_t = the same values transposed [cols, rows]
 * The sum over j is formed in fp32 (fused multiply-adds, j ascending), scaled by s, added to W in fp32 and rounded ONCE.  Where
 * s * sum is zero the element is bf16_rne(W) in bits (B = 0: the output of cm3p_cast_f32_bf16_t_multi).
 * Table: n rows of CM3P_LORA_CAST_FIELDS int64 - W (fp32 [rows, cols]), A (fp32 [r, cols]), B (fp32 [rows, r]), s (the float's bit
 * pattern in the low 32 bits), rows, cols (multiples of 8, below 2^24), r, out (bf16 [rows, cols]), out_t (bf16 [cols, rows]), index
 * of the matrix's first 64 x 64 block - with first-block indices ascending from 0 by ceil(rows / 64) * ceil(cols / 64) each.
 * A NEGATIVE rows entry -2 I marks a Wi weight [2 I, cols], I % 32 == 0: `out` gets the interleaved row order of cm3p_gemm_geglu
 * (row 64 q + t <- row 32 q + t for t < 32, row I + 32 q + t - 32 otherwise); out_t stays the canonical transpose.
 * host_table: the table in host memory - every field is validated there before the launch; dev_table: the same int64s on the
 * device (the caller's copy; it must outlive the launch).
 */
#define CM3P_LORA_CAST_FIELDS 10
int cm3p_lora_merge_cast_multi(const int64_t* host_table, const int64_t* dev_table, int n, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Adapter gradients of one adapted weight, the chain rule through W + s B A with the bf16 rounding taken as the identity:
 *     u = bf16(X a^T) [T, r]      v = bf16(DY b) [T, r]      dB = s * DY^T u [N, r]      dA = s * v^T X [r, K]
 * X [T, K] (row pitch ldx elements) and DY [T, N] (row pitch ldy) are the bf16 operands of the projection's weight-gradient GEMM;
 * a = bf16_rne(A), b = bf16_rne(B) (A fp32 [r, K], B fp32 [N, r], each rounded once); all products run on bf16 MFMA with fp32
 * accumulation.  The sum over tokens has a fixed order - inside a row block of cm3p_lora_grad_row_block(T) tokens in steps of 32
 * ascending, then over the row blocks ascending - so equal inputs give equal bits; there are no atomics.  s == 0 writes exact zeros.
 * dA, dB: fp32, contiguous, overwritten.  T >= 1; K, N multiples of 8 (below 2^24); ldx >= K, ldy >= N, multiples of 8.
 * ws: workspace of at least cm3p_lora_grad_workspace_bytes(T, K, N, r) bytes (ws_bytes: what the caller passes; checked).
 * Launches: operand preparation, the two "down" products, the two token-reduction "up" products, the ordered combine.
 */
int cm3p_lora_grad(const void* X, int64_t ldx, const void* DY, int64_t ldy, const float* A, const float* B, float s, float* dA,
                   float* dB, int64_t T, int64_t K, int64_t N, int r, void* ws, int64_t ws_bytes, void* stream);

/* Host-only: bytes of cm3p_lora_grad's workspace (bf16 copies of A and B^T, u^T and v^T, the per-row-block fp32 partial sums);
 * a negative CM3P_ERR_* code for arguments cm3p_lora_grad refuses. */
int64_t cm3p_lora_grad_workspace_bytes(int64_t T, int64_t K, int64_t N, int r);

/* Host-only: the tokens per row block of cm3p_lora_grad's token reduction at this T (a multiple of 256; ceil(T / it) partial sums
 * are combined).  CM3P_ERR_INVALID for T < 1. */
int cm3p_lora_grad_row_block(int64_t T);

#ifdef __cplusplus
}
#endif
#endif /* CM3P_LORA_H */
