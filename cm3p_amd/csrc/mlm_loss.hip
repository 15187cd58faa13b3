// Masked-LM loss without the logits tensor (gfx950): include/ext/cm3p_mlm_loss.h.
//
// Both main kernels compute 128 x 128 tiles of the decoder logits
//     x[r, c] = sum_k y[r, k] * W[c, k] (+ bias[c]),   fp32 accumulation in v_mfma_f32_16x16x32_bf16, the bias added in fp32 afterwards
// (csrc/mlm_tile.h's tile_logits, shared with csrc/mlm_topk.hip) with the main loop of csrc/gemm.hip's gemm_bf16_kernel (both operands k-contiguous: 128 x 128 x 64 per 256-thread workgroup, two LDS
// stages, register staging, one barrier per k-step) and consume the tile in registers.  No logit reaches HBM.
//   mlm_tile_kernel<false> ("lse"):     per row of the tile the maximum M and sum exp(x - M) over the tile's columns below V, written as one
//       (M, S) pair per (vocabulary tile, row); the lane that holds the row's target column writes that logit to loss_rows[r].
//       mlm_lse_combine_kernel folds the pairs over the vocabulary tiles in ascending order: lse = M + log(sum_t S_t exp(M_t - M)),
//       loss = lse - x[target].
//   mlm_tile_kernel<true> ("dlogits"):  recomputes the tile and stores bf16(s * (exp(x - lse_r) - [c == target_r])); the tile's column sums
//       of the unrounded values go to partial[row tile][c], which mlm_colsum_combine_kernel adds over the row tiles in ascending order.
// An accumulator lane holds 4 consecutive columns of one row (gemm.hip's epilogue comment), so a row reduction runs over the 4 j tiles
// in the lane, over lanes l, l + 16, l + 32, l + 48, then over the two wn waves through LDS; a column reduction over the 4 i tiles, the 16
// lanes of a group, then the two wm waves.  Every order is fixed: equal inputs give equal bits, there are no atomics.
// A row tile without a live row (label == ignore_index or outside [0, V)) and a column tile at or past V issue no MFMA: the lse kernel
// returns, the dlogits kernel writes its zeros.  Labels are compared, never used as an index, before they are known to lie in [0, V).
// The reductions reuse the operand stages' LDS after the main loop's last barrier, so the kernels stay at gemm_bf16_kernel's 64 KiB.
#include "common.h"
#include "mlm_tile.h"

#include "../../include/ext/cm3p_mlm_loss.h"

namespace {

struct MlmArgs {
    const uint16_t* y;      // [T, H] bf16
    const uint16_t* W;      // [Vp, H] bf16
    const float* bias;      // [Vp] or NULL
    const int64_t* target;  // [T]
    int64_t ignore_index, T, H, V, Vp;
    int tiles_n;
    // lse
    float* loss_rows;  // [T]: the target's logit here, the loss after the combine
    float2* part;      // [tiles_n][T] (M, S)
    // dlogits
    const float* lse_rows;
    const float* scale_a;
    const float* scale_b;
    uint16_t* dl;     // [T, Vp] bf16
    float* colpart;   // [tiles_m][Vp]
};

template <bool DL>
__global__ __launch_bounds__(256, 2) void mlm_tile_kernel(const MlmArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wm = wid >> 1, wn = wid & 1;
    // XCD-aware tile order as in gemm_bf16_kernel (speed only): consecutive tiles of an XCD share the y row panel
    const int nwg = gridDim.x, bid = blockIdx.x;
    const int q8 = nwg / 8, r8 = nwg % 8, xcd = bid % 8;
    const int swz = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + bid / 8;
    const int tm = swz / a.tiles_n, tn = swz % a.tiles_n;
    const int64_t m0 = (int64_t)tm * BM, n0 = (int64_t)tn * BN;

    // the tile's labels: -1 for every row that takes no part (past T, ignored, outside the vocabulary)
    int64_t my_t = -1;
    if (tid < BM && m0 + tid < a.T) {
        const int64_t t = a.target[m0 + tid];
        if (t != a.ignore_index && (uint64_t)t < (uint64_t)a.V) my_t = t;
    }
    const bool any_live = __syncthreads_or(my_t >= 0) != 0;
    if (!any_live || n0 >= a.V) {
        if constexpr (DL) {  // the tile's zeros: 16 chunks of 8 bf16 per row (Vp is a multiple of 64), and the tile's column sums
#pragma unroll
            for (int it = 0; it < 8; ++it) {
                const int q = tid + 256 * it, r = q >> 4, c = q & 15;
                if (m0 + r < a.T && n0 + c * 8 < a.Vp) *reinterpret_cast<uint4*>(a.dl + (m0 + r) * a.Vp + n0 + c * 8) = uint4{0u, 0u, 0u, 0u};
            }
            if (tid < BN && n0 + tid < a.Vp) a.colpart[(int64_t)tm * a.Vp + n0 + tid] = 0.f;
        }
        return;  // (lse: the combine never reads the pairs of a row that is not live, and every tile at or past V is outside its loop)
    }

    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    tile_logits(acc, smem, a.y, a.W, a.T, a.Vp, a.H, m0, n0, tid);

    // the stages are free: labels, per-row lse and the reduction scratch live there from here on
    int64_t* tg = reinterpret_cast<int64_t*>(smem);          // [128]
    float* ls = reinterpret_cast<float*>(smem + 1024);       // [128]
    float* red = reinterpret_cast<float*>(smem + 2048);      // [2][128]
    float* redm = reinterpret_cast<float*>(smem + 3072);     // [128]
    if (tid < BM) {
        tg[tid] = my_t;
        if constexpr (DL) ls[tid] = my_t >= 0 ? a.lse_rows[m0 + tid] : 0.f;
    }
    // x = acc + bias; lane's columns n .. n + 3 of tile j, n = n0 + wn * 64 + j * 16 + 4 * (lane >> 4)
    const int64_t nb = n0 + wn * 64 + 4 * (lane >> 4);
    if (a.bias) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t n = nb + j * 16;
            if (n < a.Vp) {
                const f32x4 b = *reinterpret_cast<const f32x4*>(a.bias + n);
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[i][j] += b;
            }
        }
    }
    __syncthreads();

    if constexpr (!DL) {
        // row maximum over the tile's columns below V (a pad column is never a logit, whatever W and bias hold there)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float mx = -__builtin_huge_valf();
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (nb + j * 16 + e < a.V) mx = fmaxf(mx, acc[i][j][e]);
            mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
            mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
            if (lane < 16) red[wn * BM + wm * 64 + i * 16 + lane] = mx;
        }
        __syncthreads();
        float M[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = wm * 64 + i * 16 + (lane & 15);
            M[i] = fmaxf(red[row], red[BM + row]);  // (column n0 is below V, so wave wn = 0 holds at least one logit)
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = wm * 64 + i * 16 + (lane & 15);
            const int64_t t = tg[row];
            float s = 0.f;
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int64_t c = nb + j * 16 + e;
                    if (c < a.V) {
                        s += expf(acc[i][j][e] - M[i]);
                        if (c == t) a.loss_rows[m0 + row] = acc[i][j][e];  // one lane of the whole grid per live row
                    }
                }
            s += __shfl_xor(s, 16, 64);
            s += __shfl_xor(s, 32, 64);
            if (lane < 16) {
                red[wn * BM + row] = s;
                if (wn == 0) redm[row] = M[i];
            }
        }
        __syncthreads();
        if (tid < BM && m0 + tid < a.T) a.part[(int64_t)tn * a.T + m0 + tid] = float2{redm[tid], red[tid] + red[BM + tid]};
    } else {
        const float s = a.scale_a[0] * a.scale_b[0];
        f32x4 cs[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) cs[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = wm * 64 + i * 16 + (lane & 15);
            const int64_t m = m0 + row;
            const int64_t t = tg[row];
            const float lse = ls[row];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int64_t n = nb + j * 16;
                if (n >= a.Vp) continue;
                f32x4 g;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int64_t c = n + e;
                    g[e] = (t >= 0 && c < a.V) ? s * (expf(acc[i][j][e] - lse) - (c == t ? 1.0f : 0.0f)) : 0.f;
                }
                cs[j] += g;
                if (m < a.T) *reinterpret_cast<uint2*>(a.dl + m * a.Vp + n) = uint2{pack_bf16x2(g[0], g[1]), pack_bf16x2(g[2], g[3])};
            }
        }
        // column sums of the unrounded values: the lane's 4 rows above, then the 16 lanes of the group, then the two wm waves
#pragma unroll
        for (int j = 0; j < 4; ++j) {
#pragma unroll
            for (int o = 1; o < 16; o <<= 1)
#pragma unroll
                for (int e = 0; e < 4; ++e) cs[j][e] += __shfl_xor(cs[j][e], o, 64);
            if ((lane & 15) == 0) *reinterpret_cast<f32x4*>(red + wm * BN + wn * 64 + j * 16 + 4 * (lane >> 4)) = cs[j];
        }
        __syncthreads();
        if (tid < BN && n0 + tid < a.Vp) a.colpart[(int64_t)tm * a.Vp + n0 + tid] = red[tid] + red[BN + tid];
    }
}

// one thread per row: the (M, S) pairs of the vocabulary tiles in ascending order
__global__ __launch_bounds__(256) void mlm_lse_combine_kernel(const float2* __restrict__ part, const int64_t* __restrict__ target,
                                                              int64_t ignore_index, int64_t T, int64_t V, int tiles,
                                                              float* __restrict__ loss_rows, float* __restrict__ lse_rows) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= T) return;
    const int64_t t = target[r];
    if (t == ignore_index || (uint64_t)t >= (uint64_t)V) {
        loss_rows[r] = 0.f;
        lse_rows[r] = 0.f;
        return;
    }
    float M = -__builtin_huge_valf();
    for (int k = 0; k < tiles; ++k) M = fmaxf(M, part[(int64_t)k * T + r].x);
    float S = 0.f;
    for (int k = 0; k < tiles; ++k) {
        const float2 p = part[(int64_t)k * T + r];
        S += p.y * expf(p.x - M);
    }
    const float lse = M + logf(S);
    lse_rows[r] = lse;
    loss_rows[r] = lse - loss_rows[r];
}

// one thread per column: the row tiles' sums in ascending order, then the value colsum held when `accumulate`
__global__ __launch_bounds__(256) void mlm_colsum_combine_kernel(const float* __restrict__ colpart, int tiles_m, int64_t Vp, int accumulate,
                                                                 float* __restrict__ colsum) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= Vp) return;
    float s = 0.f;
    for (int k = 0; k < tiles_m; ++k) s += colpart[(int64_t)k * Vp + c];
    colsum[c] = accumulate ? colsum[c] + s : s;
}

}  // namespace

extern "C" {

int cm3p_mlm_loss_abi_version(void) { return CM3P_MLM_LOSS_ABI_VERSION; }

int64_t cm3p_mlm_lse_workspace_bytes(int64_t T, int64_t Vp) {
    if (T < 0 || Vp < 64 || Vp % 64 != 0) return CM3P_ERR_INVALID;
    return T * tiles_of(Vp) * 8;
}

int64_t cm3p_mlm_dlogits_workspace_bytes(int64_t T, int64_t Vp) {
    if (T < 0 || Vp < 64 || Vp % 64 != 0) return CM3P_ERR_INVALID;
    return tiles_of(T) * Vp * 4;
}

int cm3p_mlm_lse(const void* y, const void* W, const float* bias, const int64_t* target, int64_t ignore_index, int64_t T, int64_t H,
                 int64_t V, int64_t Vp, float* loss_rows, float* lse_rows, void* ws, int64_t ws_bytes, void* stream) {
    CM3P_REQUIRE(y && W && target && loss_rows && lse_rows && ws);
    CM3P_REQUIRE(shapes_ok(T, H, V, Vp));
    CM3P_REQUIRE(cm3p_aligned16(y) && cm3p_aligned16(W) && (!bias || cm3p_aligned16(bias)) && cm3p_aligned16(target) && cm3p_aligned16(loss_rows) &&
                 cm3p_aligned16(lse_rows) && cm3p_aligned16(ws));
    CM3P_REQUIRE(ws_bytes >= cm3p_mlm_lse_workspace_bytes(T, Vp));
    if (T == 0) return CM3P_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    MlmArgs a{};
    a.y = static_cast<const uint16_t*>(y);
    a.W = static_cast<const uint16_t*>(W);
    a.bias = bias;
    a.target = target;
    a.ignore_index = ignore_index;
    a.T = T, a.H = H, a.V = V, a.Vp = Vp;
    a.tiles_n = (int)tiles_of(V);  // (tiles at or past V hold no logit)
    a.loss_rows = loss_rows;
    a.part = static_cast<float2*>(ws);
    mlm_tile_kernel<false><<<(unsigned)(tiles_of(T) * a.tiles_n), 256, 4 * kStageBytes, s>>>(a);
    CM3P_LAUNCH_CHECK();
    mlm_lse_combine_kernel<<<(unsigned)((T + 255) / 256), 256, 0, s>>>(a.part, target, ignore_index, T, V, a.tiles_n, loss_rows, lse_rows);
    CM3P_LAUNCH_CHECK();
    return CM3P_OK;
}

int cm3p_mlm_dlogits(const void* y, const void* W, const float* bias, const int64_t* target, int64_t ignore_index, const float* lse_rows,
                     const float* scale_a, const float* scale_b, int64_t T, int64_t H, int64_t V, int64_t Vp, void* dlogits_bf16, float* colsum,
                     int accumulate, void* ws, int64_t ws_bytes, void* stream) {
    CM3P_REQUIRE(y && W && target && lse_rows && scale_a && scale_b && dlogits_bf16 && colsum && ws);
    CM3P_REQUIRE(shapes_ok(T, H, V, Vp));
    CM3P_REQUIRE(cm3p_aligned16(y) && cm3p_aligned16(W) && (!bias || cm3p_aligned16(bias)) && cm3p_aligned16(target) && cm3p_aligned16(lse_rows) &&
                 cm3p_aligned16(dlogits_bf16) && cm3p_aligned16(colsum) && cm3p_aligned16(ws));
    CM3P_REQUIRE(ws_bytes >= cm3p_mlm_dlogits_workspace_bytes(T, Vp));
    if (T == 0) return CM3P_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    MlmArgs a{};
    a.y = static_cast<const uint16_t*>(y);
    a.W = static_cast<const uint16_t*>(W);
    a.bias = bias;
    a.target = target;
    a.ignore_index = ignore_index;
    a.T = T, a.H = H, a.V = V, a.Vp = Vp;
    a.tiles_n = (int)tiles_of(Vp);  // (every column of [T, Vp] is written)
    a.lse_rows = lse_rows;
    a.scale_a = scale_a;
    a.scale_b = scale_b;
    a.dl = static_cast<uint16_t*>(dlogits_bf16);
    a.colpart = static_cast<float*>(ws);
    const int tiles_m = (int)tiles_of(T);
    mlm_tile_kernel<true><<<(unsigned)((int64_t)tiles_m * a.tiles_n), 256, 4 * kStageBytes, s>>>(a);
    CM3P_LAUNCH_CHECK();
    mlm_colsum_combine_kernel<<<(unsigned)((Vp + 255) / 256), 256, 0, s>>>(a.colpart, tiles_m, Vp, accumulate, colsum);
    CM3P_LAUNCH_CHECK();
    return CM3P_OK;
}

}  // extern "C"
