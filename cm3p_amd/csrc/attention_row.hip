// Single-query attention for the pooled CLS row (include/cm3p_attn_row.h): query position 0 of every sequence against all of its
// keys, forward and backward, head_dim 64, gfx950.
//
// Where h[:, 0] is the only consumer of an encoder's last layer, the S x S attention of that layer shrinks to one row per
// (sequence, head).  There is no matrix to feed to the matrix cores - the work is S dot products of 64 and one weighted sum of S
// rows - so these are plain fp32 VALU kernels: ordinary 16-byte vector loads and stores, no LDS-DMA, no inline assembly.
//
// Thread mapping (both kernels): one workgroup per (sequence, head); EIGHT lanes share a key, lane j of the group owning head dims
// 8 j .. 8 j + 7 (one 16-byte load of the 128-byte k or v row: a group reads whole rows, a wave eight rows per instruction).  A dot
// product of 64 is eight fused multiply-adds per lane (dims ascending) and a three-step butterfly over the group (an IEEE add is
// commutative, so all eight lanes hold the same bits).  A workgroup of G groups takes keys g, g + G, g + 2 G, ... in group g.
//
// Rounding path (tests/attn_row_refs.py derives its bounds from exactly this):
//   forward   s = fp32 dot, times scale * log2(e) in fp32 unless q is pre-scaled; pass 1 takes the exact maximum m over the visible
//             keys; pass 2 recomputes s (same instructions, same bits), p = exp2(s - m) in fp32, l = sum p and acc[d] = sum p * v[d] in
//             fp32.  p is NOT rounded to bf16 before it multiplies v (there is no MFMA operand to feed).  out = bf16(acc / l),
//             lse = (m + log2 l) * ln 2.
//   backward  delta = fp32 sum_d dO[d] * out[d] from the stored bf16 out; p = exp2(s - lse * log2 e); dS = p * (dO . v - delta);
//             dv = bf16(p * dO); dk = bf16(rot(dS * kmul * q)) with kmul = scale (plain q) or ln 2 (pre-scaled q, which already
//             carries scale * log2 e); dq = bf16(rot(scale * sum_kv dS k)) - all fp32 up to the one bf16 rounding of the store.
//   Reduction order (fixed; no atomics, equal inputs give equal bits): per group over its keys ascending, then a butterfly over the
//   eight groups of a wave, then over the waves ascending through LDS.
// LDS: a [waves][64 + 1] fp32 exchange buffer written once per kernel by lanes 0 .. 7 of each wave (consecutive floats: no bank
// conflict worth a swizzle); occupancy is bounded by the workgroup size, not by registers (< 64 VGPRs) or LDS (< 3 KiB).
// Bounds: a sequence's row range is clamped to [0, total] (packed) before any address is formed; row indices are clamped to the
// sequence for loads and stores are predicated on them; every row offset is a 64-bit product.
#include "common.h"

#include "../../include/cm3p_attn_row.h"

#pragma clang fp contract(off)  // every fused multiply-add below is written out: pass 1 and pass 2 of the forward must agree in bits

namespace {

constexpr float kRowLog2e = 1.4426950408889634f;
constexpr float kRowLn2 = 0.69314718055994531f;
constexpr int kFwdThreads = 512, kFwdWaves = kFwdThreads / 64, kFwdGroups = kFwdThreads / 8;
constexpr int kBwdThreads = 256, kBwdWaves = kBwdThreads / 64, kBwdGroups = kBwdThreads / 8;

struct RowSeq {
    int64_t row0;  // first row of the sequence in the token-major tensors
    int len;       // its rows
};
__device__ __forceinline__ RowSeq row_seq(const int* __restrict__ cu, int64_t total, int b, int S) {
    if (!cu) return RowSeq{(int64_t)b * S, S};
    int64_t r0 = cu[b], r1 = cu[b + 1];
    r0 = r0 < 0 ? 0 : (r0 > total ? total : r0);
    r1 = r1 < r0 ? r0 : (r1 > total ? total : r1);
    return RowSeq{r0, (int)(r1 - r0)};
}
// keys 0 .. key_limit - 1 pass the window rule for query 0 (the mask rule is per key)
__device__ __forceinline__ int key_limit(int len, int window) { return (window < 0 || window >= len) ? len : window + 1; }

__device__ __forceinline__ float dot8(const float (&a)[8], const float (&b)[8]) {
    float s = a[0] * b[0];
#pragma unroll
    for (int i = 1; i < 8; ++i) s = __builtin_fmaf(a[i], b[i], s);
    return s;
}
__device__ __forceinline__ float group_sum8(float v) {  // over the eight lanes that share a key
    v += __shfl_xor(v, 1, 64);
    v += __shfl_xor(v, 2, 64);
    v += __shfl_xor(v, 4, 64);
    return v;
}
__device__ __forceinline__ float groups_sum(float v) {  // over the eight groups of a wave (lanes with equal lane & 7)
    v += __shfl_xor(v, 8, 64);
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    return v;
}
__device__ __forceinline__ void load8(const uint16_t* p, float (&f)[8]) { unpack8(*reinterpret_cast<const uint4*>(p), f); }

template <bool PRE>
__global__ __launch_bounds__(kFwdThreads) void attn_row_fwd_kernel(const uint16_t* __restrict__ qkv, uint16_t* __restrict__ out, float* __restrict__ lse,
                                                                    const uint8_t* __restrict__ kmask, const int* __restrict__ cu, int64_t total, int S,
                                                                    int nh, int window, float c) {
    __shared__ float red[kFwdWaves][65];
    const int bh = blockIdx.x, b = bh / nh, head = bh % nh;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, grp = tid >> 3, j = tid & 7;
    const RowSeq sq = row_seq(cu, total, b, S);
    uint16_t* o = out + (int64_t)bh * 64;
    if (sq.len <= 0) {  // (packed form only: a sequence without rows has no query)
        if (tid < 64) o[tid] = 0;
        if (tid == 0) lse[bh] = __builtin_huge_valf();
        return;
    }
    const int64_t ld = (int64_t)3 * nh * 64;
    const uint16_t* qrow = qkv + sq.row0 * ld + head * 64 + 8 * j;
    const uint16_t* kbase = qrow + nh * 64;
    const uint16_t* vbase = kbase + nh * 64;
    const uint8_t* mrow = kmask ? kmask + (int64_t)b * S : nullptr;
    const int klim = key_limit(sq.len, window);
    float q[8];
    load8(qrow, q);

    // pass 1: the exact maximum of the visible scores (log2 units)
    float m = -__builtin_huge_valf();
    for (int kv0 = 0; kv0 < klim; kv0 += kFwdGroups) {
        const int kv = kv0 + grp, kvc = kv < klim ? kv : klim - 1;
        const bool ok = kv < klim && (mrow ? mrow[kvc] != 0 : true);
        float k[8];
        load8(kbase + kvc * ld, k);
        float s = group_sum8(dot8(q, k));
        if constexpr (!PRE) s = s * c;
        m = fmaxf(m, ok ? s : -__builtin_huge_valf());
    }
    m = wave_max(m);
    if (lane == 0) red[wid][0] = m;
    __syncthreads();
    m = red[0][0];
#pragma unroll
    for (int w = 1; w < kFwdWaves; ++w) m = fmaxf(m, red[w][0]);
    __syncthreads();

    // pass 2: p = exp2(s - m), l = sum p, acc = sum p v
    float l = 0.f, acc[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = 0.f;
    for (int kv0 = 0; kv0 < klim; kv0 += kFwdGroups) {
        const int kv = kv0 + grp, kvc = kv < klim ? kv : klim - 1;
        const bool ok = kv < klim && (mrow ? mrow[kvc] != 0 : true);
        float k[8], v[8];
        load8(kbase + kvc * ld, k);
        load8(vbase + kvc * ld, v);
        float s = group_sum8(dot8(q, k));
        if constexpr (!PRE) s = s * c;
        const float p = ok ? __builtin_amdgcn_exp2f(s - m) : 0.f;
        l += p;
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] = __builtin_fmaf(p, v[i], acc[i]);
    }
    l = groups_sum(l);
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = groups_sum(acc[i]);
    if (lane < 8) {
#pragma unroll
        for (int i = 0; i < 8; ++i) red[wid][8 * j + i] = acc[i];
        if (lane == 0) red[wid][64] = l;
    }
    __syncthreads();
    if (tid < 64) {
        float a = red[0][tid], lt = red[0][64];
#pragma unroll
        for (int w = 1; w < kFwdWaves; ++w) {
            a += red[w][tid];
            lt += red[w][64];
        }
        o[tid] = lt > 0.f ? f32_to_bf16_bits(a / lt) : (uint16_t)0;
        if (tid == 0) lse[bh] = lt > 0.f ? (m + __log2f(lt)) * kRowLn2 : __builtin_huge_valf();
    }
}

// the inverse rotary rotation of the lane's eight values: lanes j < 4 hold head dims d = 8 j + i (the "a" half), lanes j >= 4 hold
// d + 32 (the "b" half) of the same table columns; a' = a cos + b sin, b' = b cos - a sin
__device__ __forceinline__ void unrotate8(float (&x)[8], const float (&other)[8], const float* __restrict__ cos_row, const float* __restrict__ sin_row,
                                          int j) {
    const f32x4 c0 = *reinterpret_cast<const f32x4*>(cos_row + 8 * (j & 3)), c1 = *reinterpret_cast<const f32x4*>(cos_row + 8 * (j & 3) + 4);
    const f32x4 s0 = *reinterpret_cast<const f32x4*>(sin_row + 8 * (j & 3)), s1 = *reinterpret_cast<const f32x4*>(sin_row + 8 * (j & 3) + 4);
    const float sign = j < 4 ? 1.f : -1.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const float cs = i < 4 ? c0[i & 3] : c1[i & 3], sn = i < 4 ? s0[i & 3] : s1[i & 3];
        x[i] = __builtin_fmaf(x[i], cs, sign * (other[i] * sn));
    }
}

template <bool PRE, bool ROPE>
__global__ __launch_bounds__(kBwdThreads) void attn_row_bwd_kernel(const uint16_t* __restrict__ qkv, const uint16_t* __restrict__ o_rows,
                                                                    const uint16_t* __restrict__ d_o, const float* __restrict__ lse,
                                                                    uint16_t* __restrict__ dqkv, const uint8_t* __restrict__ kmask,
                                                                    const int* __restrict__ cu, int64_t total, int S, int nh, int window, float scale,
                                                                    const float* __restrict__ rope_cos, const float* __restrict__ rope_sin,
                                                                    int64_t pos_batch_stride) {
    __shared__ float red[kBwdWaves][64];
    const int bh = blockIdx.x, b = bh / nh, head = bh % nh;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, grp = tid >> 3, j = tid & 7;
    const RowSeq sq = row_seq(cu, total, b, S);
    if (sq.len <= 0) return;
    const int64_t ld = (int64_t)3 * nh * 64;
    const int64_t col = head * 64 + 8 * j;
    const uint16_t* qrow = qkv + sq.row0 * ld + col;
    const uint16_t* kbase = qrow + nh * 64;
    const uint16_t* vbase = kbase + nh * 64;
    uint16_t* dq_base = dqkv + sq.row0 * ld + col;
    const uint8_t* mrow = kmask ? kmask + (int64_t)b * S : nullptr;
    const int klim = key_limit(sq.len, window);
    const int64_t pos0 = cu ? sq.row0 : (int64_t)b * pos_batch_stride;
    float q[8], go[8], ov[8];
    load8(qrow, q);
    load8(d_o + (int64_t)bh * 64 + 8 * j, go);
    load8(o_rows + (int64_t)bh * 64 + 8 * j, ov);
    const float delta = group_sum8(dot8(go, ov));
    const float lse2 = lse[bh] * kRowLog2e;  // +inf for a query without a visible key: p = 0 everywhere
    const float c = scale * kRowLog2e, kmul = PRE ? kRowLn2 : scale;
    const uint4 zero4 = uint4{0u, 0u, 0u, 0u};

    float dq[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) dq[i] = 0.f;
    for (int kv0 = 0; kv0 < sq.len; kv0 += kBwdGroups) {
        const int kv = kv0 + grp, kvc = kv < sq.len ? kv : sq.len - 1;
        const bool in = kv < sq.len;
        const bool ok = kv < klim && (mrow ? mrow[kvc] != 0 : true);
        float k[8], v[8];
        load8(kbase + kvc * ld, k);
        load8(vbase + kvc * ld, v);
        float s = group_sum8(dot8(q, k));
        if constexpr (!PRE) s = s * c;
        const float dp = group_sum8(dot8(go, v));
        const float p = ok ? __builtin_amdgcn_exp2f(s - lse2) : 0.f;
        const float ds = ok ? p * (dp - delta) : 0.f;
        const float dsk = ds * kmul;
        float dk[8], dv[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            dk[i] = dsk * q[i];
            dv[i] = p * go[i];
            dq[i] = __builtin_fmaf(ds, k[i], dq[i]);
        }
        if constexpr (ROPE) {
            float other[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) other[i] = __shfl_xor(dk[i], 4, 64);
            unrotate8(dk, other, rope_cos + (pos0 + kvc) * 32, rope_sin + (pos0 + kvc) * 32, j);
        }
        if (in) {
            uint16_t* drow = dq_base + kv * ld;
            if (kv != 0) *reinterpret_cast<uint4*>(drow) = zero4;  // (the query row's q third is stored below)
            *reinterpret_cast<uint4*>(drow + nh * 64) = ok ? pack8(dk) : zero4;
            *reinterpret_cast<uint4*>(drow + 2 * nh * 64) = ok ? pack8(dv) : zero4;
        }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) dq[i] = groups_sum(dq[i]);
    if (lane < 8) {
#pragma unroll
        for (int i = 0; i < 8; ++i) red[wid][8 * j + i] = dq[i];
    }
    __syncthreads();
    if (tid < 8) {
        float own[8], other[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            float a = red[0][8 * j + i], t = red[0][8 * (j ^ 4) + i];
#pragma unroll
            for (int w = 1; w < kBwdWaves; ++w) {
                a += red[w][8 * j + i];
                t += red[w][8 * (j ^ 4) + i];
            }
            own[i] = a * scale;
            other[i] = t * scale;
        }
        if constexpr (ROPE) unrotate8(own, other, rope_cos + pos0 * 32, rope_sin + pos0 * 32, j);
        *reinterpret_cast<uint4*>(dq_base) = pack8(own);
    }
}

bool row_args_ok(const void* qkv, const void* out, const float* lse, const uint8_t* key_mask, const int* cu, int B, int S, int64_t total, int nh,
                 float scale) {
    return qkv && out && lse && cm3p_aligned16(qkv) && cm3p_aligned16(out) && cm3p_aligned16(lse) && B > 0 && S > 0 && nh > 0 && scale > 0.f &&
           !(key_mask && cu) && (!cu || (total > 0 && (reinterpret_cast<uintptr_t>(cu) & 3u) == 0)) && (int64_t)B * nh < (int64_t(1) << 31) &&
           (int64_t)nh * 192 < (int64_t(1) << 31);
}

}  // namespace

extern "C" {

int cm3p_attn_row_abi_version(void) { return CM3P_ATTN_ROW_ABI_VERSION; }

int cm3p_attn_row_fwd(const void* qkv, void* out, float* lse, const uint8_t* key_mask, const int* cu_seqlens, int B, int S, int64_t total, int nh,
                      int window, float scale, int q_prescaled, void* stream) {
    CM3P_REQUIRE(row_args_ok(qkv, out, lse, key_mask, cu_seqlens, B, S, total, nh, scale));
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const uint16_t* x = static_cast<const uint16_t*>(qkv);
    uint16_t* o = static_cast<uint16_t*>(out);
    const float c = scale * kRowLog2e;
    if (q_prescaled) attn_row_fwd_kernel<true><<<dim3(B * nh), dim3(kFwdThreads), 0, st>>>(x, o, lse, key_mask, cu_seqlens, total, S, nh, window, c);
    else attn_row_fwd_kernel<false><<<dim3(B * nh), dim3(kFwdThreads), 0, st>>>(x, o, lse, key_mask, cu_seqlens, total, S, nh, window, c);
    CM3P_LAUNCH_CHECK();
    return CM3P_OK;
}

int cm3p_attn_row_bwd(const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv, const uint8_t* key_mask, const int* cu_seqlens,
                      int B, int S, int64_t total, int nh, int window, float scale, const float* cos_tab, const float* sin_tab,
                      int64_t pos_batch_stride, int q_prescaled, void* stream) {
    CM3P_REQUIRE(row_args_ok(qkv, out, lse, key_mask, cu_seqlens, B, S, total, nh, scale));
    CM3P_REQUIRE(dout && dqkv && cm3p_aligned16(dout) && cm3p_aligned16(dqkv));
    CM3P_REQUIRE((cos_tab == nullptr) == (sin_tab == nullptr) && cm3p_aligned16(cos_tab) && cm3p_aligned16(sin_tab));
    CM3P_REQUIRE(pos_batch_stride == 0 || pos_batch_stride == S);
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid(B * nh), block(kBwdThreads);
    auto go = [&](auto pre, auto rope) {
        attn_row_bwd_kernel<decltype(pre)::value, decltype(rope)::value><<<grid, block, 0, st>>>(
            static_cast<const uint16_t*>(qkv), static_cast<const uint16_t*>(out), static_cast<const uint16_t*>(dout), lse, static_cast<uint16_t*>(dqkv),
            key_mask, cu_seqlens, total, S, nh, window, scale, cos_tab, sin_tab, pos_batch_stride);
        return CM3P_OK;
    };
    const int rc = cm3p_with_layout(q_prescaled != 0, cos_tab != nullptr, go);
    if (rc != CM3P_OK) return rc;
    CM3P_LAUNCH_CHECK();
    return CM3P_OK;
}

}  // extern "C"
