// The 128 x 128 logit tile of the masked-LM head (gfx950), shared by csrc/mlm_loss.hip and csrc/mlm_topk.hip:
//     x[r, c] = sum_k y[r, k] * W[c, k],   fp32 accumulation in v_mfma_f32_16x16x32_bf16
// with the main loop of csrc/gemm.hip's gemm_bf16_kernel (both operands k-contiguous: 128 x 128 x 64 per 256-thread workgroup, two LDS
// stages, register staging, one barrier per k-step).  The tile stays in registers; what a kernel does with it is its own epilogue.
// An accumulator lane holds 4 consecutive columns of one row (gemm.hip's epilogue comment): acc[i][j][e] of wave (wm, wn) is
//     row    wm * 64 + i * 16 + (lane & 15)
//     column wn * 64 + j * 16 + 4 * (lane >> 4) + e
// of the tile, so a row reduction runs over the 4 j tiles in the lane, over lanes l, l + 16, l + 32, l + 48, then over the two wn waves.
#pragma once

#include "common.h"

namespace {

constexpr int BM = 128, BN = 128, BK = 64;
constexpr int kStageBytes = BM * BK * 2;  // 16 KiB per operand per stage

// byte offset of 16-byte chunk c (8 k-values) of row r in a k-contiguous tile image: ds_read_b128 fragments are bank-conflict free
__device__ __forceinline__ int kc_off(int r, int c) { return r * 128 + ((c ^ (r & 7)) << 4); }

// a thread's 4 chunks of a [128 rows][64 k] operand tile; rows at or past `extent` and k at or past K read as zero
struct TileLoader {
    const uint16_t* ptr[4];
    bool row_ok[4];
    int koff[4];
    int lds[4];

    __device__ __forceinline__ void init(const uint16_t* base, int64_t ld, int64_t idx0, int64_t extent, int tid) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int q = tid + 256 * i, r = q >> 3, c = q & 7;
            row_ok[i] = idx0 + r < extent;
            koff[i] = c * 8;
            ptr[i] = base + (idx0 + r) * ld + c * 8;
            lds[i] = kc_off(r, c);
        }
    }
    __device__ __forceinline__ void load(uint4 (&r)[4], int64_t k0, int64_t kend) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const bool ok = row_ok[i] && (k0 + koff[i] < kend);
            r[i] = ok ? *reinterpret_cast<const uint4*>(ptr[i]) : uint4{0u, 0u, 0u, 0u};
            ptr[i] += BK;
        }
    }
    __device__ __forceinline__ void store(char* stage, const uint4 (&r)[4]) const {
#pragma unroll
        for (int i = 0; i < 4; ++i) *reinterpret_cast<uint4*>(stage + lds[i]) = r[i];
    }
};

// fragment of 16 rows x 32 k: lane l holds element (idx0 + (l & 15), kk * 32 + 8 * (l >> 4) + j), j = 0..7
__device__ __forceinline__ bf16x8 load_frag(const char* stage, int idx0, int kk, int lane) {
    return *reinterpret_cast<const bf16x8*>(stage + kc_off(idx0 + (lane & 15), kk * 4 + (lane >> 4)));
}

// acc[i][j] = the wave's 64 x 64 quarter of the tile; ends on a barrier, after which no wave reads the stages again
__device__ __forceinline__ void tile_logits(f32x4 (&acc)[4][4], char* smem, const uint16_t* y, const uint16_t* W, int64_t T, int64_t Vp,
                                            int64_t H, int64_t m0, int64_t n0, int tid) {
    const int lane = tid & 63, wid = tid >> 6, wm = wid >> 1, wn = wid & 1;
    TileLoader la, lb;
    la.init(y, H, m0, T, tid);
    lb.init(W, H, n0, Vp, tid);
    const int nk = (int)((H + BK - 1) / BK);
    uint4 ra[4], rb[4];
    la.load(ra, 0, H);
    lb.load(rb, 0, H);
    la.store(smem, ra);
    lb.store(smem + kStageBytes, rb);
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
        const char* sa = smem + (kt & 1) * 2 * kStageBytes;
        const char* sb = sa + kStageBytes;
        const bool more = kt + 1 < nk;
        if (more) {
            la.load(ra, (int64_t)(kt + 1) * BK, H);
            lb.load(rb, (int64_t)(kt + 1) * BK, H);
        }
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            bf16x8 fa[4], fb[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) fa[i] = load_frag(sa, wm * 64 + i * 16, kk, lane);
#pragma unroll
            for (int j = 0; j < 4; ++j) fb[j] = load_frag(sb, wn * 64 + j * 16, kk, lane);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb[j], fa[i], acc[i][j], 0, 0, 0);
        }
        if (more) {
            char* na = smem + ((kt + 1) & 1) * 2 * kStageBytes;
            la.store(na, ra);
            lb.store(na + kStageBytes, rb);
        }
        __syncthreads();
    }
}

inline int64_t tiles_of(int64_t n) { return (n + 127) / 128; }

inline bool shapes_ok(int64_t T, int64_t H, int64_t V, int64_t Vp) {
    // (tile counts are ints and one grid dimension: 2^31 - 1 workgroups)
    return T >= 0 && H >= 8 && H % 8 == 0 && Vp >= 64 && Vp % 64 == 0 && V >= 1 && V <= Vp && T < (int64_t(1) << 40) && Vp < (int64_t(1) << 31) &&
           tiles_of(T) * tiles_of(Vp) < (int64_t(1) << 31);
}

}  // namespace
