// Low-rank adapters (LoRA) on the encoder's projection weights: include/cm3p_lora.h.
//
//   merged cast      W_eff = bf16(W + s B A) and its transpose for many matrices in one launch: cast_f32_bf16_t_multi_kernel
//                    (elementwise.hip) with the r-term fp32 sum added before the one rounding.  The GEMMs never see the adapter.
//   adapter grads    u = bf16(X a^T), v = bf16(DY b) ("down": skinny products, [T, r] out), then dB = s DY^T u and dA = s v^T X ("up":
//                    reductions over the T tokens).  HBM-bound: X and DY are read once by each stage; u and v are T r bf16 each and
//                    are kept TRANSPOSED ([r, Tp]) so that the up stage reads 8 consecutive tokens of one adapter column with one
//                    16-byte load.  The token sum is ordered: 32 tokens per MFMA step ascending inside a row block, one fp32 partial
//                    per row block, combined ascending by lora_reduce_kernel.  No atomics.
//
// MFMA: v_mfma_f32_16x16x32_bf16.  Lane (i = lane % 16, g = lane / 16) supplies row i of the first operand and column i of the second at
// the contraction indices 8 g .. 8 g + 7, and receives D[4 g + e][i], e < 4.  Both operands are filled with the SAME rule, so only the
// pairing of the contraction index matters, not which eight the hardware calls 8 g .. 8 g + 7.
#include "common.h"

#include "../../include/cm3p_lora.h"

namespace {

constexpr bool lora_rank_ok(int r) { return r == 8 || r == 16 || r == 32 || r == 64; }
constexpr int kF = CM3P_LORA_CAST_FIELDS;

__device__ __forceinline__ f32x4 mfma16(uint4 a, uint4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// One 64 x 64 tile of one matrix per block, as cast_f32_bf16_t_multi_kernel; A's 64 columns and B's 64 rows of the tile wait in LDS as
// fp32.  Thread (row, 4 columns): four fma chains over j ascending.
__global__ __launch_bounds__(256) void lora_merge_cast_multi_kernel(const int64_t* __restrict__ table, int n) {
    __shared__ float As[64][64];
    __shared__ float Bs[64][65];  // 65: the four rows a wave reads at one j sit in four banks
    __shared__ uint16_t tile[64][66];
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (table[kF * mid + 9] <= (int64_t)blockIdx.x) lo = mid;
        else hi = mid - 1;
    }
    const int64_t* e = table + kF * lo;
    const float* x = reinterpret_cast<const float*>(e[0]);
    const float* A = reinterpret_cast<const float*>(e[1]);
    const float* B = reinterpret_cast<const float*>(e[2]);
    const float s = __builtin_bit_cast(float, (uint32_t)e[3]);
    const int rows_arg = (int)e[4], cols = (int)e[5], r = (int)e[6];
    uint16_t* y = reinterpret_cast<uint16_t*>(e[7]);
    uint16_t* yt = reinterpret_cast<uint16_t*>(e[8]);
    const bool interleave = rows_arg < 0;
    const int rows = interleave ? -rows_arg : rows_arg, half = rows >> 1;
    const int blk = (int)((int64_t)blockIdx.x - e[9]);
    const int tiles_c = (cols + 63) / 64;
    const int r0 = (blk / tiles_c) * 64, c0 = (blk % tiles_c) * 64;
    const int tid = threadIdx.x;
    for (int idx = tid; idx < r * 64; idx += 256) {
        const int j = idx >> 6, c = idx & 63;
        As[j][c] = c0 + c < cols ? A[(int64_t)j * cols + c0 + c] : 0.f;
    }
    for (int idx = tid; idx < 64 * r; idx += 256) {
        const int row = idx / r, j = idx - row * r;
        Bs[row][j] = r0 + row < rows ? B[(int64_t)(r0 + row) * r + j] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int rr = it * 16 + (tid >> 4), c = (tid & 15) * 4;
        if (r0 + rr < rows && c0 + c < cols) {
            const f32x4 w = *reinterpret_cast<const f32x4*>(x + (int64_t)(r0 + rr) * cols + c0 + c);
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            for (int j = 0; j < r; ++j) {
                const float b = Bs[rr][j];
                const f32x4 a = *reinterpret_cast<const f32x4*>(&As[j][c]);
                acc.x = __builtin_fmaf(b, a.x, acc.x);
                acc.y = __builtin_fmaf(b, a.y, acc.y);
                acc.z = __builtin_fmaf(b, a.z, acc.z);
                acc.w = __builtin_fmaf(b, a.w, acc.w);
            }
            const f32x4 d = acc * s;
            // (a zero update leaves W's own bits, sign of zero included: B = 0 is cm3p_cast_f32_bf16_t_multi)
            const f32x4 v = {d.x == 0.f ? w.x : w.x + d.x, d.y == 0.f ? w.y : w.y + d.y, d.z == 0.f ? w.z : w.z + d.z, d.w == 0.f ? w.w : w.w + d.w};
            const uint32_t lo2 = pack_bf16x2(v.x, v.y), hi2 = pack_bf16x2(v.z, v.w);
            int yr = r0 + rr;
            if (interleave) yr = yr < half ? (yr >> 5) * 64 + (yr & 31) : ((yr - half) >> 5) * 64 + 32 + ((yr - half) & 31);
            *reinterpret_cast<uint2*>(y + (int64_t)yr * cols + c0 + c) = uint2{lo2, hi2};
            tile[rr][c] = (uint16_t)lo2;
            tile[rr][c + 1] = (uint16_t)(lo2 >> 16);
            tile[rr][c + 2] = (uint16_t)hi2;
            tile[rr][c + 3] = (uint16_t)(hi2 >> 16);
        }
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const int c = it * 32 + (tid >> 3), rr = (tid & 7) * 8;
        if (c0 + c < cols && r0 + rr < rows) {
            uint32_t w[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) w[k] = (uint32_t)tile[rr + 2 * k][c] | ((uint32_t)tile[rr + 2 * k + 1][c] << 16);
            *reinterpret_cast<uint4*>(yt + (int64_t)(c0 + c) * rows + r0 + rr) = uint4{w[0], w[1], w[2], w[3]};
        }
    }
}

// a = bf16(A) [r, K] and bt = bf16(B)^T [r, N]: the operands of the down stage, each value rounded once
__global__ __launch_bounds__(256) void lora_prep_kernel(const float* __restrict__ A, const float* __restrict__ B, uint16_t* __restrict__ a16,
                                                        uint16_t* __restrict__ bt16, int64_t K, int64_t N, int r) {
    const int64_t nA = (int64_t)r * K, nB = (int64_t)r * N;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nA + nB; i += (int64_t)gridDim.x * 256) {
        if (i < nA) {
            a16[i] = f32_to_bf16_bits(A[i]);
        } else {
            const int64_t q = i - nA, j = q / N, nn = q - j * N;
            bt16[q] = f32_to_bf16_bits(B[nn * r + j]);
        }
    }
}

struct LoraDownProb {
    const uint16_t* M;  // [T, C] bf16, row pitch ldm
    int64_t ldm;
    const uint16_t* P;  // [r, C] bf16
    int C;
    uint16_t* outT;  // [r, Tp] bf16: outT[j][t] = bf16(sum_c M[t, c] P[j, c]); columns T .. Tp - 1 are written as zeros
};
struct LoraDownArgs {
    LoraDownProb p[2];
    int64_t T, Tp;
    int r;
};

// 64 tokens per block, 16 per wave; blockIdx.y picks the product (u or v).  RT = ceil(r / 16) accumulator tiles per wave.
template <int RT>
__global__ __launch_bounds__(256) void lora_down_kernel(const LoraDownArgs a) {
    const LoraDownProb p = a.p[blockIdx.y];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 15, g = lane >> 4;
    const int64_t t0 = (int64_t)blockIdx.x * 64 + wave * 16, t = t0 + i;
    const bool row_ok = t < a.T;
    f32x4 acc[RT];
#pragma unroll
    for (int jt = 0; jt < RT; ++jt) acc[jt] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < p.C; k0 += 32) {
        const int kk = k0 + g * 8;  // (C % 8 == 0: a group of eight is inside or outside as a whole)
        const bool k_ok = kk < p.C;
        uint4 xa = {0u, 0u, 0u, 0u};
        if (row_ok && k_ok) xa = *reinterpret_cast<const uint4*>(p.M + t * p.ldm + kk);
#pragma unroll
        for (int jt = 0; jt < RT; ++jt) {
            const int j = jt * 16 + i;
            uint4 pb = {0u, 0u, 0u, 0u};
            if (k_ok && j < a.r) pb = *reinterpret_cast<const uint4*>(p.P + (int64_t)j * p.C + kk);
            acc[jt] = mfma16(xa, pb, acc[jt]);  // D[token 4 g + e][j = i]
        }
    }
#pragma unroll
    for (int jt = 0; jt < RT; ++jt) {
        const int j = jt * 16 + i;
        if (j < a.r)
            *reinterpret_cast<uint2*>(p.outT + (int64_t)j * a.Tp + t0 + g * 4) = uint2{pack_bf16x2(acc[jt][0], acc[jt][1]), pack_bf16x2(acc[jt][2], acc[jt][3])};
    }
}

struct LoraUpProb {
    const uint16_t* M;  // [T, C] bf16, row pitch ldm
    int64_t ldm;
    int C;
    const uint16_t* wT;  // [r, Tp] bf16
    float* part;         // [row blocks][C r] fp32 partial sums in the layout of the result
};
struct LoraUpArgs {
    LoraUpProb p[2];  // 0: dB [N, r] = DY^T u    1: dA [r, K] = v^T X
    int64_t T, Tp;
    int r, tb;
};

// One block: 64 columns of M x one row block of tokens.  Per step 32 tokens x 64 columns of M go through LDS (coalesced 16-byte loads in,
// column walks out: the MFMA wants 8 consecutive tokens of one column per lane), wave w takes columns 16 w .. 16 w + 15.
// ROWS_ARE_J: the result's rows are adapter columns (dA [r, C]); otherwise they are M's columns (dB [C, r]).  Either way a lane ends with
// four consecutive fp32 of one result row.
template <int RT, bool ROWS_ARE_J>
__device__ __forceinline__ void lora_up_body(const LoraUpProb& p, const LoraUpArgs& a, uint32_t (*tile)[33]) {
    const int c0 = blockIdx.x * 64;
    if (c0 >= p.C) return;  // (block-uniform: the two products share one grid)
    const int tid = threadIdx.x, lane = tid & 63, cw = (tid >> 6) * 16, i = lane & 15, g = lane >> 4;
    const int64_t tb0 = (int64_t)blockIdx.y * a.tb;
    const int64_t tend = tb0 + a.tb < a.T ? tb0 + a.tb : a.T;
    const int lrow = tid >> 3, lc = (tid & 7) * 8;
    const bool col_ok = c0 + lc < p.C;
    auto gload = [&](int64_t t0) {
        uint4 w = {0u, 0u, 0u, 0u};
        if (t0 + lrow < a.T && col_ok) w = *reinterpret_cast<const uint4*>(p.M + (t0 + lrow) * p.ldm + c0 + lc);
        return w;
    };
    uint4 cur = gload(tb0);
    f32x4 acc[RT];
#pragma unroll
    for (int jt = 0; jt < RT; ++jt) acc[jt] = f32x4{0.f, 0.f, 0.f, 0.f};
    const uint16_t* t16 = reinterpret_cast<const uint16_t*>(&tile[0][0]);  // row pitch 66 halves
    for (int64_t t0 = tb0; t0 < tend; t0 += 32) {
        uint32_t* dst = &tile[lrow][lc >> 1];
        dst[0] = cur.x;
        dst[1] = cur.y;
        dst[2] = cur.z;
        dst[3] = cur.w;
        __syncthreads();
        if (t0 + 32 < tend) cur = gload(t0 + 32);
        uint32_t mw[4];
#pragma unroll
        for (int q = 0; q < 4; ++q)
            mw[q] = (uint32_t)t16[(8 * g + 2 * q) * 66 + cw + i] | ((uint32_t)t16[(8 * g + 2 * q + 1) * 66 + cw + i] << 16);
        const uint4 mf = {mw[0], mw[1], mw[2], mw[3]};
#pragma unroll
        for (int jt = 0; jt < RT; ++jt) {
            const int j = jt * 16 + i;
            uint4 wf = {0u, 0u, 0u, 0u};
            if (j < a.r) wf = *reinterpret_cast<const uint4*>(p.wT + (int64_t)j * a.Tp + t0 + 8 * g);  // (t0 + 32 <= Tp)
            acc[jt] = ROWS_ARE_J ? mfma16(wf, mf, acc[jt]) : mfma16(mf, wf, acc[jt]);
        }
        __syncthreads();
    }
    float* out = p.part + (int64_t)blockIdx.y * p.C * a.r;
#pragma unroll
    for (int jt = 0; jt < RT; ++jt) {
        if constexpr (ROWS_ARE_J) {  // D[j = 16 jt + 4 g + e][column c0 + cw + i]: four j of one column... stored per j row
            const int c = c0 + cw + i;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int j = jt * 16 + 4 * g + e;
                if (j < a.r && c < p.C) out[(int64_t)j * p.C + c] = acc[jt][e];
            }
        } else {  // D[column c0 + cw + 4 g + e][j = 16 jt + i]
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int c = c0 + cw + 4 * g + e, j = jt * 16 + i;
                if (j < a.r && c < p.C) out[(int64_t)c * a.r + j] = acc[jt][e];
            }
        }
    }
}

template <int RT>
__global__ __launch_bounds__(256) void lora_up_kernel(const LoraUpArgs a) {
    __shared__ uint32_t tile[32][33];
    if (blockIdx.z == 0) lora_up_body<RT, false>(a.p[0], a, tile);
    else lora_up_body<RT, true>(a.p[1], a, tile);
}

// result = s * (partial 0 + partial 1 + ...), ascending; both results in one launch
__global__ __launch_bounds__(256) void lora_reduce_kernel(const float* __restrict__ partB, float* __restrict__ dB, int64_t nB4,
                                                          const float* __restrict__ partA, float* __restrict__ dA, int64_t nA4, int nrb, float s) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nB4 + nA4; i += (int64_t)gridDim.x * 256) {
        const bool isB = i < nB4;
        const int64_t q = isB ? i : i - nB4, n4 = isB ? nB4 : nA4;
        const f32x4* src = reinterpret_cast<const f32x4*>(isB ? partB : partA) + q;
        f32x4 v = src[0];
        for (int b = 1; b < nrb; ++b) v += src[(int64_t)b * n4];
        v = s == 0.f ? f32x4{0.f, 0.f, 0.f, 0.f} : v * s;
        reinterpret_cast<f32x4*>(isB ? dB : dA)[q] = v;
    }
}

inline int lora_row_block(int64_t T) {
    int64_t tb = 256;
    while ((T + tb - 1) / tb > 64) tb *= 2;
    return (int)tb;
}

struct LoraWs {
    int64_t a16, bt16, uT, vT, partA, partB, total, Tp;
    int tb, nrb;
};
inline bool lora_grad_shape_ok(int64_t T, int64_t K, int64_t N, int r) {
    return lora_rank_ok(r) && T >= 1 && T < (int64_t(1) << 31) - 64 && K > 0 && N > 0 && K % 8 == 0 && N % 8 == 0 && K < (1 << 24) && N < (1 << 24);
}
inline LoraWs lora_ws(int64_t T, int64_t K, int64_t N, int r) {
    LoraWs w;
    w.Tp = (T + 63) / 64 * 64;
    w.tb = lora_row_block(T);
    w.nrb = (int)((T + w.tb - 1) / w.tb);
    int64_t off = 0;  // (every piece is a multiple of 16 bytes: r >= 8, K, N, Tp multiples of 8)
    w.a16 = off, off += r * K * 2;
    w.bt16 = off, off += r * N * 2;
    w.uT = off, off += r * w.Tp * 2;
    w.vT = off, off += r * w.Tp * 2;
    w.partA = off, off += (int64_t)w.nrb * r * K * 4;
    w.partB = off, off += (int64_t)w.nrb * r * N * 4;
    w.total = off;
    return w;
}

inline int lora_grid(int64_t items) {
    int64_t b = (items + 255) / 256;
    return (int)(b > 2048 ? 2048 : (b < 1 ? 1 : b));
}

}  // namespace

extern "C" {

int cm3p_lora_abi_version(void) { return CM3P_LORA_ABI_VERSION; }

int cm3p_lora_merge_cast_multi(const int64_t* host_table, const int64_t* dev_table, int n, void* stream) {
    CM3P_REQUIRE(host_table && dev_table && n > 0);
    int64_t blocks = 0;
    for (int i = 0; i < n; ++i) {
        const int64_t* e = host_table + (int64_t)kF * i;
        const bool il = e[4] < 0;
        const int64_t rows = il ? -e[4] : e[4], cols = e[5];
        CM3P_REQUIRE(e[0] && e[1] && e[2] && e[7] && e[8]);
        CM3P_REQUIRE(e[6] >= 0 && e[6] <= 64 && lora_rank_ok((int)e[6]));
        CM3P_REQUIRE(rows > 0 && cols > 0 && rows % 8 == 0 && cols % 8 == 0 && rows < (1 << 24) && cols < (1 << 24));
        CM3P_REQUIRE(!il || rows % 64 == 0);
        for (int f : {0, 1, 2, 7, 8}) CM3P_REQUIRE((e[f] & 15) == 0);
        CM3P_REQUIRE(e[9] == blocks);
        blocks += ((rows + 63) / 64) * ((cols + 63) / 64);
        CM3P_REQUIRE(blocks < (int64_t(1) << 31));
    }
    lora_merge_cast_multi_kernel<<<(int)blocks, 256, 0, static_cast<hipStream_t>(stream)>>>(dev_table, n);
    CM3P_LAUNCH_CHECK();
    return CM3P_OK;
}

int64_t cm3p_lora_grad_workspace_bytes(int64_t T, int64_t K, int64_t N, int r) {
    if (!lora_grad_shape_ok(T, K, N, r)) return CM3P_ERR_INVALID;
    return lora_ws(T, K, N, r).total;
}

int cm3p_lora_grad_row_block(int64_t T) {
    CM3P_REQUIRE(T >= 1);
    return lora_row_block(T);
}

int cm3p_lora_grad(const void* X, int64_t ldx, const void* DY, int64_t ldy, const float* A, const float* B, float s, float* dA,
                   float* dB, int64_t T, int64_t K, int64_t N, int r, void* ws, int64_t ws_bytes, void* stream) {
    CM3P_REQUIRE(X && DY && A && B && dA && dB && ws);
    CM3P_REQUIRE(lora_grad_shape_ok(T, K, N, r));
    CM3P_REQUIRE(ldx >= K && ldy >= N && ldx % 8 == 0 && ldy % 8 == 0);
    for (const void* q : {X, DY, (const void*)A, (const void*)B, (const void*)dA, (const void*)dB, (const void*)ws}) CM3P_REQUIRE(cm3p_aligned16(q));
    const LoraWs w = lora_ws(T, K, N, r);
    CM3P_REQUIRE(ws_bytes >= w.total);
    hipStream_t st = static_cast<hipStream_t>(stream);
    char* base = static_cast<char*>(ws);
    uint16_t* a16 = reinterpret_cast<uint16_t*>(base + w.a16);
    uint16_t* bt16 = reinterpret_cast<uint16_t*>(base + w.bt16);
    uint16_t* uT = reinterpret_cast<uint16_t*>(base + w.uT);
    uint16_t* vT = reinterpret_cast<uint16_t*>(base + w.vT);
    float* partA = reinterpret_cast<float*>(base + w.partA);
    float* partB = reinterpret_cast<float*>(base + w.partB);
    const uint16_t* Xb = static_cast<const uint16_t*>(X);
    const uint16_t* DYb = static_cast<const uint16_t*>(DY);

    lora_prep_kernel<<<lora_grid((int64_t)r * (K + N)), 256, 0, st>>>(A, B, a16, bt16, K, N, r);
    CM3P_LAUNCH_CHECK();

    LoraDownArgs d;
    d.p[0] = LoraDownProb{Xb, ldx, a16, (int)K, uT};
    d.p[1] = LoraDownProb{DYb, ldy, bt16, (int)N, vT};
    d.T = T, d.Tp = w.Tp, d.r = r;
    const dim3 dgrid((unsigned)(w.Tp / 64), 2, 1);
    if (r <= 16) lora_down_kernel<1><<<dgrid, 256, 0, st>>>(d);
    else if (r == 32) lora_down_kernel<2><<<dgrid, 256, 0, st>>>(d);
    else lora_down_kernel<4><<<dgrid, 256, 0, st>>>(d);
    CM3P_LAUNCH_CHECK();

    LoraUpArgs u;
    u.p[0] = LoraUpProb{DYb, ldy, (int)N, uT, partB};
    u.p[1] = LoraUpProb{Xb, ldx, (int)K, vT, partA};
    u.T = T, u.Tp = w.Tp, u.r = r, u.tb = w.tb;
    const int64_t cmax = K > N ? K : N;
    const dim3 ugrid((unsigned)((cmax + 63) / 64), (unsigned)w.nrb, 2);
    if (r <= 16) lora_up_kernel<1><<<ugrid, 256, 0, st>>>(u);
    else if (r == 32) lora_up_kernel<2><<<ugrid, 256, 0, st>>>(u);
    else lora_up_kernel<4><<<ugrid, 256, 0, st>>>(u);
    CM3P_LAUNCH_CHECK();

    const int64_t nB4 = N * r / 4, nA4 = (int64_t)r * K / 4;
    lora_reduce_kernel<<<lora_grid(nB4 + nA4), 256, 0, st>>>(partB, dB, nB4, partA, dA, nA4, w.nrb, s);
    CM3P_LAUNCH_CHECK();
    return CM3P_OK;
}

}  // extern "C"
