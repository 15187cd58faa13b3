// Launchers of the matrix-core attention kernels for head sizes 96 and 128 (attention_hd.hip).  Plain C++: the C ABI reaches them
// through cm3p_attn_fwd_generic / cm3p_attn_bwd_generic (attention_generic.hip), which have validated every argument.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

bool cm3p_attn_hd_supported(int head_dim);  // 96 or 128
int cm3p_attn_hd_fwd(const uint16_t* qkv, uint16_t* out, float* lse, const uint8_t* key_mask, int B, int S, int nh, int head_dim, int window,
                     float scale, hipStream_t stream);
int cm3p_attn_hd_bwd(const uint16_t* qkv, const uint16_t* out, const uint16_t* dout, const float* lse, float* delta, uint16_t* dqkv,
                     const uint8_t* key_mask, int B, int S, int nh, int head_dim, int window, float scale, hipStream_t stream);
