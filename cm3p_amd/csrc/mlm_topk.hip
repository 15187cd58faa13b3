// Masked-LM top-k predictions without the logits tensor (gfx950): include/ext/predict/cm3p_mlm_topk.h.
//
// mlm_topk_tile_kernel computes one 128 x 128 tile of the decoder logits x = y W^T (+ bias) per workgroup (csrc/mlm_tile.h's tile_logits,
// the grid and tile order of csrc/mlm_loss.hip's mlm_tile_kernel) and consumes it in registers.  Per row of the tile it leaves in the
// workspace
//   - the (M, S) = (max x, sum exp(x - M)) pair over the tile's columns below V, computed as mlm_tile_kernel<false> computes it, and
//   - the tile's k best columns as (value, column), ordered by (value descending, column ascending).
// The k candidates come from k rounds of "largest remaining element, lowest column on a tie"; after a round the winner's element is set
// to -inf in the registers that hold the tile, as the pad columns [V, Vp) are from the start, and an element that is -inf is never chosen:
// a round that finds nothing leaves (-inf, -1).  A round reduces over the lane's 16 values of the row in ascending column order (a later
// element wins only when it is strictly larger), over the 4 lanes of the row by butterfly (larger value, then lower column), and over the
// two column waves through LDS (wave 0 holds the lower columns and wins a tie).  No sorting network, no runtime-indexed register.
// mlm_topk_combine_kernel, one thread per row, merges the tiles in ascending order into 8 fully unrolled register slots: a candidate goes
// before the first slot whose value is strictly smaller (every column seen before is lower, so an equal value stays in front), and the
// rest of a tile is skipped once one of its candidates finds no slot.  lse folds as mlm_lse_combine_kernel folds it.
// Every order is fixed: equal inputs give equal bits, there are no atomics.  A NaN compares false everywhere: it is never chosen and
// never an index.
#include "common.h"
#include "mlm_tile.h"

#include "../../include/ext/predict/cm3p_mlm_topk.h"

namespace {

constexpr int kMaxK = 8;

struct TopkArgs {
    const uint16_t* y;  // [T, H] bf16
    const uint16_t* W;  // [Vp, H] bf16
    const float* bias;  // [Vp] or NULL
    int64_t T, H, V, Vp;
    int tiles_n, k;
    float2* part;  // [tiles_n][k + 1][T]: slots 0 .. k - 1 (value, column as int bits), slot k (M, S)
};

__global__ __launch_bounds__(256, 2) void mlm_topk_tile_kernel(const TopkArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wm = wid >> 1, wn = wid & 1;
    // XCD-aware tile order as in gemm_bf16_kernel (speed only): consecutive tiles of an XCD share the y row panel
    const int nwg = gridDim.x, bid = blockIdx.x;
    const int q8 = nwg / 8, r8 = nwg % 8, xcd = bid % 8;
    const int swz = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + bid / 8;
    const int tm = swz / a.tiles_n, tn = swz % a.tiles_n;
    const int64_t m0 = (int64_t)tm * BM, n0 = (int64_t)tn * BN;  // (n0 < V: the grid has ceil(V / 128) column tiles)

    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    tile_logits(acc, smem, a.y, a.W, a.T, a.Vp, a.H, m0, n0, tid);

    // the stages are free: the reduction scratch lives there from here on
    float* red = reinterpret_cast<float*>(smem);          // [2][128] row maxima of the two column waves
    float* reds = reinterpret_cast<float*>(smem + 1024);  // [2][128] row sums
    float* cv = reinterpret_cast<float*>(smem + 2048);    // [2 round parities][2][128] a wave's best value of the round
    int* cc = reinterpret_cast<int*>(smem + 4096);        // [2][2][128] and its column
    const float ninf = -__builtin_huge_valf();
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
    // a pad column is never a logit, whatever W and bias hold there: -inf takes no part in a maximum, adds exp(-inf) = +0 to a sum and is
    // never a round's winner
    const int cb = (int)nb;                                                        // (Vp < 2^31)
    const int lim = (int)(a.V - nb < 64 ? (a.V - nb > 0 ? a.V - nb : 0) : 64);     // the lane's columns nb + c, c < lim, are below V
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (j * 16 + e >= lim) acc[i][j][e] = ninf;

    // ---- (M, S) of the tile, as mlm_tile_kernel<false>: 15 maxima / adds in the lane, 2 over the lanes, 1 over the two waves
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        float mx = ninf;
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) mx = fmaxf(mx, acc[i][j][e]);
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        if (lane < 16) red[wn * BM + wm * 64 + i * 16 + lane] = mx;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = wm * 64 + i * 16 + (lane & 15);
        const float M = fmaxf(red[row], red[BM + row]);  // (column n0 is below V, so wave wn = 0 holds at least one logit)
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (j * 16 + e < lim) s += expf(acc[i][j][e] - M);
        s += __shfl_xor(s, 16, 64);
        s += __shfl_xor(s, 32, 64);
        if (lane < 16) reds[wn * BM + row] = s;
    }
    __syncthreads();
    const int64_t slot0 = (int64_t)tn * (a.k + 1);
    if (tid < BM && m0 + tid < a.T) a.part[(slot0 + a.k) * a.T + m0 + tid] = float2{fmaxf(red[tid], red[BM + tid]), reds[tid] + reds[BM + tid]};

    // ---- k rounds; round r writes parity r & 1 of cv / cc, whose readers of round r - 2 are behind round r - 1's barrier
    for (int r = 0; r < a.k; ++r) {
        float* rv = cv + (r & 1) * 2 * BM;
        int* rc = cc + (r & 1) * 2 * BM;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float bv = ninf;
            int bc = -1;
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float v = acc[i][j][e];
                    if (v > bv) {  // ascending columns: an equal value later on does not replace the earlier one
                        bv = v;
                        bc = cb + j * 16 + e;
                    }
                }
#pragma unroll
            for (int o = 16; o <= 32; o <<= 1) {
                const float ov = __shfl_xor(bv, o, 64);
                const int oc = __shfl_xor(bc, o, 64);
                if (ov > bv || (ov == bv && oc < bc)) {  // (two lanes without a candidate hold the same (-inf, -1))
                    bv = ov;
                    bc = oc;
                }
            }
            if (lane < 16) {
                rv[wn * BM + wm * 64 + i * 16 + lane] = bv;
                rc[wn * BM + wm * 64 + i * 16 + lane] = bc;
            }
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = wm * 64 + i * 16 + (lane & 15);
            const float v0 = rv[row], v1 = rv[BM + row];
            const bool hi = v1 > v0;  // wave 0 holds the lower columns: it keeps a tie
            const float wv = hi ? v1 : v0;
            const int wc = hi ? rc[BM + row] : rc[row];
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (cb + j * 16 + e == wc) acc[i][j][e] = ninf;  // (wc = -1: no column)
            if (wn == 0 && lane < 16 && m0 + row < a.T) a.part[(slot0 + r) * a.T + m0 + row] = float2{wv, __int_as_float(wc)};
        }
    }
}

// one thread per row: the tiles in ascending order
__global__ __launch_bounds__(256) void mlm_topk_combine_kernel(const float2* __restrict__ part, int64_t T, int tiles, int k,
                                                               int32_t* __restrict__ top_idx, float* __restrict__ top_val,
                                                               float* __restrict__ lse_rows) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= T) return;
    const float ninf = -__builtin_huge_valf();
    float tv[kMaxK];
    int tc[kMaxK];
#pragma unroll
    for (int s = 0; s < kMaxK; ++s) {
        tv[s] = ninf;
        tc[s] = -1;
    }
    float M = ninf;
    for (int t = 0; t < tiles; ++t) {
        const float2* p = part + (int64_t)t * (k + 1) * T + r;
        M = fmaxf(M, p[(int64_t)k * T].x);
        for (int c = 0; c < k; ++c) {
            const float2 q = p[(int64_t)c * T];
            float v = q.x;
            int col = __float_as_int(q.y);
            bool moved = false;  // once the candidate has taken a slot, what it displaced moves one slot down
            bool among_k = false;
#pragma unroll
            for (int s = 0; s < kMaxK; ++s) {
                const bool sw = moved || v > tv[s];
                const float v2 = tv[s];
                const int c2 = tc[s];
                tv[s] = sw ? v : v2;
                tc[s] = sw ? col : c2;
                v = sw ? v2 : v;
                col = sw ? c2 : col;
                moved = sw;
                if (s == k - 1) among_k = sw;
            }
            // not among the best k: the tile's remaining candidates sort after this one.  (Slots only move down, so what the slots past
            // k - 1 hold never reaches an output.)
            if (!among_k) break;
        }
    }
    float S = 0.f;
    for (int t = 0; t < tiles; ++t) {
        const float2 p = part[((int64_t)t * (k + 1) + k) * T + r];
        S += p.y * expf(p.x - M);
    }
    lse_rows[r] = M + logf(S);
#pragma unroll
    for (int s = 0; s < kMaxK; ++s)
        if (s < k) {
            top_idx[r * k + s] = tc[s];
            top_val[r * k + s] = tv[s];
        }
}

}  // namespace

extern "C" {

int cm3p_mlm_topk_abi_version(void) { return CM3P_MLM_TOPK_ABI_VERSION; }

int64_t cm3p_mlm_topk_workspace_bytes(int64_t T, int64_t Vp, int k) {
    if (T < 0 || Vp < 64 || Vp % 64 != 0 || k < 1 || k > kMaxK) return CM3P_ERR_INVALID;
    return T * tiles_of(Vp) * (k + 1) * 8;
}

int cm3p_mlm_topk(const void* y, const void* W, const float* bias, int64_t T, int64_t H, int64_t V, int64_t Vp, int k, int32_t* top_idx,
                  float* top_val, float* lse_rows, void* ws, int64_t ws_bytes, void* stream) {
    CM3P_REQUIRE(y && W && top_idx && top_val && lse_rows && ws);
    CM3P_REQUIRE(k >= 1 && k <= kMaxK);
    CM3P_REQUIRE(shapes_ok(T, H, V, Vp));
    CM3P_REQUIRE(cm3p_aligned16(y) && cm3p_aligned16(W) && (!bias || cm3p_aligned16(bias)) && cm3p_aligned16(top_idx) && cm3p_aligned16(top_val) &&
                 cm3p_aligned16(lse_rows) && cm3p_aligned16(ws));
    CM3P_REQUIRE(ws_bytes >= cm3p_mlm_topk_workspace_bytes(T, Vp, k));
    if (T == 0) return CM3P_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    TopkArgs a{};
    a.y = static_cast<const uint16_t*>(y);
    a.W = static_cast<const uint16_t*>(W);
    a.bias = bias;
    a.T = T, a.H = H, a.V = V, a.Vp = Vp;
    a.tiles_n = (int)tiles_of(V);  // (tiles at or past V hold no logit)
    a.k = k;
    a.part = static_cast<float2*>(ws);
    mlm_topk_tile_kernel<<<(unsigned)(tiles_of(T) * a.tiles_n), 256, 4 * kStageBytes, s>>>(a);
    CM3P_LAUNCH_CHECK();
    mlm_topk_combine_kernel<<<(unsigned)((T + 255) / 256), 256, 0, s>>>(a.part, T, a.tiles_n, k, top_idx, top_val, lse_rows);
    CM3P_LAUNCH_CHECK();
    return CM3P_OK;
}

}  // extern "C"
