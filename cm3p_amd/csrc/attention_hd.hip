// Attention for head sizes 96 and 128 on the matrix cores (v_mfma_f32_32x32x16_bf16), gfx950.
//
// A 768-wide tower with 8 heads has head_dim 96, a 1024-wide one 128: the sizes people choose when they widen a tower.  The contract is
// attention_generic.hip's, and these kernels sit behind its entry points (cm3p_attn_fwd_generic / cm3p_attn_bwd_generic):
//     visible(b, q, kv) = key_mask[b, kv] AND (window < 0 OR |q - kv| <= window);  rows with no visible key: exact zeros, lse = +inf;
//     padded queries are computed like any other query; padded keys receive exactly zero dK and dV.
// Layout: qkv [B, S, 3, nh, D] bf16 (q, k already rotated: cm3p_rope_apply_generic), out [B, S, nh, D] bf16, lse / delta [B, nh, S] fp32.
//
// Formulation (attention.hip's, with the head dimension as a template parameter): one workgroup = 4 waves = 128 queries (dK/dV: keys) of
// one (batch, head), 32 per wave; the other side arrives in tiles of 32 rows, staged in LDS as bf16 by ordinary vector loads and
// ds_write, double buffered (the next tile's global loads are issued before the products of this one, one barrier per tile).
//   forward  S^T = K Q^T, D / 16 MFMAs: the query sits on the lane, so the row maximum and sum are in-lane plus one exchange between the
//            lane halves; P is rounded to bf16 in the accumulator registers and is the B operand of O^T += V^T P^T (V^T by
//            ds_read_b64_tr_b16) without crossing LDS.  O^T is D / 32 accumulator blocks (64 registers at D = 128), Q^T D / 16 fragments (32).
//   dQ       recomputes S^T, dP^T = V dO^T, dS^T = P^T o (dP^T - delta), dQ^T += K^T dS^T; delta = sum_d dO O from the stored bf16 out.
//   dK, dV   key on the lane: S = Q K^T, dP = dO V^T (K, V fragments in registers; Q, dO tiles in LDS, read as rows and transposed);
//            dV^T += dO^T P and dK^T += Q^T dS take the accumulators as B operands.  Two O^T-sized accumulators.
// Sliding-window layers visit only the tiles the band can touch (O(S window)); a wave skips the tiles outside its own 32 rows' band.
// Every sum has a fixed order: no atomics, no workspace, the same bits on every call.  LDS rows are 2 D + 16 bytes apart: the 16-byte
// row fragments of 16 consecutive rows and the 4-row blocks of a transposed read each fall into different banks.
// No LDS-DMA here, hence no bounds-audit hooks (build.AUDIT_SOURCES); every global read clamps or guards its row.
#include "attention_hd.h"

#include "attn_common.h"

namespace {

constexpr int kHdTile = 32;    // rows of a staged tile
constexpr int kHdBlock = 128;  // rows of a workgroup (4 waves x 32)

template <int D>
struct Hd {
    static_assert(D % 32 == 0, "whole 32-column accumulator blocks");
    static constexpr int NS = D / 16;   // k-steps of a product over the head dimension
    static constexpr int NB = D / 32;   // accumulator blocks of a [D x 32] result
    static constexpr int CPR = D / 8;   // 16-byte chunks per row
    static constexpr int PITCH = 2 * D + 16;
    static constexpr int TILE = kHdTile * PITCH;
    static constexpr int CHUNKS = kHdTile * CPR;
    static constexpr int NCH = (CHUNKS + 255) / 256;  // chunks per thread
};

// rows r0 .. r0 + 31 of a [*, D] bf16 matrix with row stride `ld` elements -> registers; rows >= limit read as zero
template <int D>
__device__ __forceinline__ void hd_gload(uint4 (&v)[Hd<D>::NCH], const uint16_t* base, int64_t ld, int r0, int limit, int tid) {
#pragma unroll
    for (int i = 0; i < Hd<D>::NCH; ++i) {
        const int q = tid + 256 * i, row = q / Hd<D>::CPR, c = q % Hd<D>::CPR;
        const int r = r0 + row;
        v[i] = (q < Hd<D>::CHUNKS && r < limit) ? *reinterpret_cast<const uint4*>(base + (int64_t)r * ld + c * 8) : uint4{0u, 0u, 0u, 0u};
    }
}
template <int D>
__device__ __forceinline__ void hd_lstore(char* tile, const uint4 (&v)[Hd<D>::NCH], int tid) {
#pragma unroll
    for (int i = 0; i < Hd<D>::NCH; ++i) {
        const int q = tid + 256 * i, row = q / Hd<D>::CPR, c = q % Hd<D>::CPR;
        if (q < Hd<D>::CHUNKS) *reinterpret_cast<uint4*>(tile + row * Hd<D>::PITCH + c * 16) = v[i];
    }
}

// row fragment (A operand) of a staged tile: lane holds X[lane & 31][16 s + 8 (lane >> 5) + j]
template <int D>
__device__ __forceinline__ bf16x8 hd_frag_R(const char* tile, int s, int lane) {
    return *reinterpret_cast<const bf16x8*>(tile + (lane & 31) * Hd<D>::PITCH + (2 * s + (lane >> 5)) * 16);
}
// A-operand fragment of X^T (rows = columns 32 cblk .. 32 cblk + 31 of the tile, k = its 16 rows from krow0) for X^T * Y with Y
// from accumulators: element j of lane half hh is row krow0 + 8 (j >> 2) + 4 hh + (j & 3) - the order acc_to_frag delivers.
template <int D>
__device__ __forceinline__ bf16x8 hd_frag_T(const char* tile, int krow0, int cblk, int lane) {
    const int g = lane >> 4, hh = g >> 1, i = lane & 15;
    const int row = krow0 + 4 * hh + (i >> 2);
    const int col = 32 * cblk + 16 * (g & 1) + 4 * (i & 3);
    const bf16x4 lo = lds_read_tr16(tile + row * Hd<D>::PITCH + col * 2);
    const bf16x4 hi = lds_read_tr16(tile + (row + 8) * Hd<D>::PITCH + col * 2);
    return cat_bf16x4(lo, hi);
}
// the lane's half of one row as MFMA B-operand fragments: element j of fragment s is column 16 s + 8 hh + j
template <int D>
__device__ __forceinline__ void hd_row_frags(bf16x8 (&f)[Hd<D>::NS], const uint16_t* row, int hh) {
#pragma unroll
    for (int s = 0; s < Hd<D>::NS; ++s) f[s] = *reinterpret_cast<const bf16x8*>(row + 16 * s + 8 * hh);
}
// accumulator blocks (lane = row, register i of block cb = column 32 cb + 8 (i >> 2) + 4 hh + (i & 3)) -> one bf16 row
template <int D>
__device__ __forceinline__ void hd_store_row(uint16_t* dst, const f32x16 (&a)[Hd<D>::NB], float mul, int hh) {
#pragma unroll
    for (int cb = 0; cb < Hd<D>::NB; ++cb)
#pragma unroll
        for (int g = 0; g < 4; ++g)
            *reinterpret_cast<uint2*>(dst + 32 * cb + 8 * g + 4 * hh) =
                uint2{pack_bf16x2(a[cb][4 * g] * mul, a[cb][4 * g + 1] * mul), pack_bf16x2(a[cb][4 * g + 2] * mul, a[cb][4 * g + 3] * mul)};
}

__device__ __forceinline__ float hd_max16(const f32x16& a) {
    const float m0 = max3(a[0], a[1], a[2]), m1 = max3(a[3], a[4], a[5]), m2 = max3(a[6], a[7], a[8]);
    const float m3 = max3(a[9], a[10], a[11]), m4 = max3(a[12], a[13], a[14]);
    return max3(max3(m0, m1, m2), max3(m3, m4, a[15]), m0);
}

// the tiles [first, last] of 32 rows that the band of rows [R0, R0 + n - 1] can touch (the whole axis for a global layer)
struct HdRange {
    int lo, hi;  // rows
    __device__ __forceinline__ HdRange(int R0, int n, int window, int S) {
        lo = window < 0 ? 0 : max(0, R0 - window);
        hi = window < 0 ? S - 1 : min(S - 1, R0 + n - 1 + window);
    }
};

// ---------------------------------------------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(256) void attn_hd_fwd_kernel(const uint16_t* __restrict__ qkv, uint16_t* __restrict__ out, float* __restrict__ lse,
                                                          const uint8_t* __restrict__ kmask, int S, int nh, int window_arg, float scale) {
    using H = Hd<D>;
    __shared__ __attribute__((aligned(16))) char Ts[2][2][H::TILE];  // [stage][K, V]
    __shared__ __attribute__((aligned(16))) uint8_t Ms[2][kHdTile];   // key validity
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, hh = lane >> 5, l31 = lane & 31;
    const int head = blockIdx.y, b = blockIdx.z;
    const int window = window_arg < 0 ? -1 : min(window_arg, S);  // (a wider band is the whole axis; keeps row + window inside int)
    const int Q0 = blockIdx.x * kHdBlock, q0 = Q0 + 32 * wid, qrow = q0 + l31;
    const int64_t ld = (int64_t)3 * nh * D;
    const uint16_t* qbase = qkv + (int64_t)b * S * ld + head * D;
    const uint16_t* kbase = qbase + nh * D;
    const uint16_t* vbase = qbase + 2 * nh * D;
    const float c = scale * kLog2e;

    bf16x8 qf[H::NS];
    hd_row_frags<D>(qf, qbase + (int64_t)min(qrow, S - 1) * ld, hh);
    f32x16 oacc[H::NB];
#pragma unroll
    for (int cb = 0; cb < H::NB; ++cb)
#pragma unroll
        for (int i = 0; i < 16; ++i) oacc[cb][i] = 0.f;
    float m_run = kNegInf, l_run = 0.f;  // log2 units; l_run: this lane half's keys

    const int lo = window < 0 ? INT_MIN : qrow - window, hi = window < 0 ? INT_MAX : qrow + window;
    const HdRange blk(Q0, kHdBlock, window, S), wav(q0, 32, window, S);
    const bool wave_live = q0 < S;
    const int t_lo = blk.lo / kHdTile, t_hi = blk.hi / kHdTile;

    uint4 kr[H::NCH], vr[H::NCH];
    uint8_t mreg = 0;
    auto gload = [&](int t) {
        hd_gload<D>(kr, kbase, ld, t * kHdTile, S, tid);
        hd_gload<D>(vr, vbase, ld, t * kHdTile, S, tid);
        if (tid < kHdTile) {
            const int key = t * kHdTile + tid;
            mreg = key < S ? (kmask ? (uint8_t)(kmask[(int64_t)b * S + key] != 0) : (uint8_t)1) : (uint8_t)0;
        }
    };
    auto lstore = [&](int stage) {
        hd_lstore<D>(Ts[stage][0], kr, tid);
        hd_lstore<D>(Ts[stage][1], vr, tid);
        if (tid < kHdTile) Ms[stage][tid] = mreg;
    };

    gload(t_lo);
    lstore(0);
    __syncthreads();

    for (int t = t_lo; t <= t_hi; ++t) {
        const int stage = (t - t_lo) & 1;
        const bool more = t < t_hi;
        if (more) gload(t + 1);
        const int key0 = t * kHdTile;
        if (wave_live && key0 <= wav.hi && key0 + kHdTile - 1 >= wav.lo) {
            const char* Kt = Ts[stage][0];
            const char* Vt = Ts[stage][1];
            f32x16 sacc;
#pragma unroll
            for (int i = 0; i < 16; ++i) sacc[i] = 0.f;
#pragma unroll
            for (int s = 0; s < H::NS; ++s) sacc = mfma32(hd_frag_R<D>(Kt, s, lane), qf[s], sacc);
            // accumulator register 4 g + r is key key0 + 8 g + 4 hh + r of this lane's query
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const uint32_t mb = *reinterpret_cast<const uint32_t*>(&Ms[stage][8 * g + 4 * hh]);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int key = key0 + 8 * g + 4 * hh + r;
                    const bool ok = (((mb >> (8 * r)) & 0xffu) != 0u) & (key >= lo) & (key <= hi);
                    sacc[4 * g + r] = ok ? sacc[4 * g + r] * c : kNegInf;
                }
            }
            float mt = hd_max16(sacc);
            mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
            const float m_new = fmaxf(m_run, mt);
            const float m_use = m_new > kNegInf ? m_new : 0.f;      // (no visible key so far: every p below is exp2(-inf) = 0)
            const float alpha = __builtin_amdgcn_exp2f(m_run - m_use);  // (m_run = -inf: 0, and O = l = 0)
            float psum = 0.f;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const float p = __builtin_amdgcn_exp2f(sacc[i] - m_use);
                sacc[i] = p;
                psum += p;
            }
            l_run = __builtin_fmaf(l_run, alpha, psum);
            m_run = m_new;
            if (!__all(alpha == 1.0f)) {
#pragma unroll
                for (int cb = 0; cb < H::NB; ++cb)
#pragma unroll
                    for (int i = 0; i < 16; ++i) oacc[cb][i] *= alpha;
            }
            // O^T += V^T P^T: P goes from the accumulators to the B operand, rounded to bf16
#pragma unroll
            for (int sp = 0; sp < 2; ++sp) {
                const bf16x8 pf = acc_to_frag(sacc, sp);
#pragma unroll
                for (int cb = 0; cb < H::NB; ++cb) oacc[cb] = mfma32(hd_frag_T<D>(Vt, 16 * sp, cb, lane), pf, oacc[cb]);
            }
        }
        if (more) lstore(stage ^ 1);
        __syncthreads();
    }

    const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
    const float inv = l_tot > 0.f ? 1.0f / l_tot : 0.f;
    if (qrow < S) {
        hd_store_row<D>(out + ((int64_t)b * S + qrow) * nh * D + head * D, oacc, inv, hh);
        if (hh == 0) lse[((int64_t)b * nh + head) * S + qrow] = l_tot > 0.f ? (m_run + __log2f(l_tot)) * 0.69314718055994531f : __builtin_huge_valf();
    }
}

// ---------------------------------------------------------------------------------------------------------------
// dQ (gradient w.r.t. the rotated q, times scale) and delta[b, h, q] = sum_d dO[q, d] O[q, d]: the forward's geometry
// ---------------------------------------------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(256) void attn_hd_dq_kernel(const uint16_t* __restrict__ qkv, const uint16_t* __restrict__ o_rows,
                                                         const uint16_t* __restrict__ d_o, const float* __restrict__ lse, float* __restrict__ delta,
                                                         uint16_t* __restrict__ dqkv, const uint8_t* __restrict__ kmask, int S, int nh, int window_arg,
                                                         float scale) {
    using H = Hd<D>;
    __shared__ __attribute__((aligned(16))) char Ts[2][2][H::TILE];  // [stage][K, V]
    __shared__ __attribute__((aligned(16))) uint8_t Ms[2][kHdTile];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, hh = lane >> 5, l31 = lane & 31;
    const int head = blockIdx.y, b = blockIdx.z;
    const int window = window_arg < 0 ? -1 : min(window_arg, S);
    const int Q0 = blockIdx.x * kHdBlock, q0 = Q0 + 32 * wid, qrow = q0 + l31, qc = min(qrow, S - 1);
    const int64_t ld = (int64_t)3 * nh * D, ldo = (int64_t)nh * D;
    const uint16_t* qbase = qkv + (int64_t)b * S * ld + head * D;
    const uint16_t* kbase = qbase + nh * D;
    const uint16_t* vbase = qbase + 2 * nh * D;
    const float c = scale * kLog2e;

    bf16x8 qf[H::NS], gf[H::NS];
    hd_row_frags<D>(qf, qbase + (int64_t)qc * ld, hh);
    hd_row_frags<D>(gf, d_o + ((int64_t)b * S + qc) * ldo + head * D, hh);
    float dlt = 0.f;
    {
        bf16x8 of[H::NS];
        hd_row_frags<D>(of, o_rows + ((int64_t)b * S + qc) * ldo + head * D, hh);
#pragma unroll
        for (int s = 0; s < H::NS; ++s)
#pragma unroll
            for (int j = 0; j < 8; ++j) dlt = __builtin_fmaf((float)of[s][j], (float)gf[s][j], dlt);
        dlt += __shfl_xor(dlt, 32, 64);  // (both halves add the same two numbers)
    }
    const int64_t stat = ((int64_t)b * nh + head) * S + qc;
    const float lse2 = lse[stat] * kLog2e;  // +inf (no visible key): p = 0 everywhere
    if (qrow < S && hh == 0) delta[stat] = dlt;

    f32x16 dqacc[H::NB];
#pragma unroll
    for (int cb = 0; cb < H::NB; ++cb)
#pragma unroll
        for (int i = 0; i < 16; ++i) dqacc[cb][i] = 0.f;

    const int lo = window < 0 ? INT_MIN : qrow - window, hi = window < 0 ? INT_MAX : qrow + window;
    const HdRange blk(Q0, kHdBlock, window, S), wav(q0, 32, window, S);
    const bool wave_live = q0 < S;
    const int t_lo = blk.lo / kHdTile, t_hi = blk.hi / kHdTile;

    uint4 kr[H::NCH], vr[H::NCH];
    uint8_t mreg = 0;
    auto gload = [&](int t) {
        hd_gload<D>(kr, kbase, ld, t * kHdTile, S, tid);
        hd_gload<D>(vr, vbase, ld, t * kHdTile, S, tid);
        if (tid < kHdTile) {
            const int key = t * kHdTile + tid;
            mreg = key < S ? (kmask ? (uint8_t)(kmask[(int64_t)b * S + key] != 0) : (uint8_t)1) : (uint8_t)0;
        }
    };
    auto lstore = [&](int stage) {
        hd_lstore<D>(Ts[stage][0], kr, tid);
        hd_lstore<D>(Ts[stage][1], vr, tid);
        if (tid < kHdTile) Ms[stage][tid] = mreg;
    };

    gload(t_lo);
    lstore(0);
    __syncthreads();

    for (int t = t_lo; t <= t_hi; ++t) {
        const int stage = (t - t_lo) & 1;
        const bool more = t < t_hi;
        if (more) gload(t + 1);
        const int key0 = t * kHdTile;
        if (wave_live && key0 <= wav.hi && key0 + kHdTile - 1 >= wav.lo) {
            const char* Kt = Ts[stage][0];
            const char* Vt = Ts[stage][1];
            f32x16 sacc, dpacc;
#pragma unroll
            for (int i = 0; i < 16; ++i) sacc[i] = dpacc[i] = 0.f;
#pragma unroll
            for (int s = 0; s < H::NS; ++s) {
                sacc = mfma32(hd_frag_R<D>(Kt, s, lane), qf[s], sacc);    // S^T = K Q^T
                dpacc = mfma32(hd_frag_R<D>(Vt, s, lane), gf[s], dpacc);  // dP^T = V dO^T
            }
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const uint32_t mb = *reinterpret_cast<const uint32_t*>(&Ms[stage][8 * g + 4 * hh]);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int key = key0 + 8 * g + 4 * hh + r;
                    const bool ok = (((mb >> (8 * r)) & 0xffu) != 0u) & (key >= lo) & (key <= hi);
                    const float p = ok ? __builtin_amdgcn_exp2f(__builtin_fmaf(sacc[4 * g + r], c, -lse2)) : 0.f;
                    sacc[4 * g + r] = p * (dpacc[4 * g + r] - dlt);  // dS^T
                }
            }
            // dQ^T += K^T dS^T
#pragma unroll
            for (int sp = 0; sp < 2; ++sp) {
                const bf16x8 df = acc_to_frag(sacc, sp);
#pragma unroll
                for (int cb = 0; cb < H::NB; ++cb) dqacc[cb] = mfma32(hd_frag_T<D>(Kt, 16 * sp, cb, lane), df, dqacc[cb]);
            }
        }
        if (more) lstore(stage ^ 1);
        __syncthreads();
    }
    if (qrow < S) hd_store_row<D>(dqkv + ((int64_t)b * S + qrow) * ld + head * D, dqacc, scale, hh);
}

// ---------------------------------------------------------------------------------------------------------------
// dK (times scale), dV: one workgroup = 128 keys, 32 per wave, key on the lane; query tiles (q, dO, lse, delta) staged in LDS
// ---------------------------------------------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(256) void attn_hd_dkv_kernel(const uint16_t* __restrict__ qkv, const uint16_t* __restrict__ d_o,
                                                          const float* __restrict__ lse, const float* __restrict__ delta,
                                                          uint16_t* __restrict__ dqkv, const uint8_t* __restrict__ kmask, int S, int nh, int window_arg,
                                                          float scale) {
    using H = Hd<D>;
    __shared__ __attribute__((aligned(16))) char Ts[2][2][H::TILE];  // [stage][Q, dO]
    __shared__ __attribute__((aligned(16))) float Ls[2][kHdTile], Ds[2][kHdTile];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, hh = lane >> 5, l31 = lane & 31;
    const int head = blockIdx.y, b = blockIdx.z;
    const int window = window_arg < 0 ? -1 : min(window_arg, S);
    const int K0 = blockIdx.x * kHdBlock, k0 = K0 + 32 * wid, key = k0 + l31, kc = min(key, S - 1);
    const int64_t ld = (int64_t)3 * nh * D, ldo = (int64_t)nh * D;
    const uint16_t* qbase = qkv + (int64_t)b * S * ld + head * D;
    const uint16_t* gbase = d_o + (int64_t)b * S * ldo + head * D;
    const int64_t stat0 = ((int64_t)b * nh + head) * S;
    const float c = scale * kLog2e;

    bf16x8 kf[H::NS], vf[H::NS];
    hd_row_frags<D>(kf, qbase + (int64_t)kc * ld + nh * D, hh);
    hd_row_frags<D>(vf, qbase + (int64_t)kc * ld + 2 * nh * D, hh);
    const bool key_ok = key < S && (kmask ? kmask[(int64_t)b * S + kc] != 0 : true);
    f32x16 dkacc[H::NB], dvacc[H::NB];
#pragma unroll
    for (int cb = 0; cb < H::NB; ++cb)
#pragma unroll
        for (int i = 0; i < 16; ++i) dkacc[cb][i] = dvacc[cb][i] = 0.f;

    const int lo = window < 0 ? INT_MIN : key - window, hi = window < 0 ? INT_MAX : key + window;
    const HdRange blk(K0, kHdBlock, window, S), wav(k0, 32, window, S);
    const bool wave_live = k0 < S;
    const int t_lo = blk.lo / kHdTile, t_hi = blk.hi / kHdTile;

    uint4 qr[H::NCH], gr[H::NCH];
    float lreg = 0.f, dreg = 0.f;
    auto gload = [&](int t) {
        hd_gload<D>(qr, qbase, ld, t * kHdTile, S, tid);
        hd_gload<D>(gr, gbase, ldo, t * kHdTile, S, tid);
        if (tid < kHdTile) {
            const int q = t * kHdTile + tid;
            lreg = q < S ? lse[stat0 + q] * kLog2e : __builtin_huge_valf();  // rows past the sequence: p = 0
            dreg = q < S ? delta[stat0 + q] : 0.f;
        }
    };
    auto lstore = [&](int stage) {
        hd_lstore<D>(Ts[stage][0], qr, tid);
        hd_lstore<D>(Ts[stage][1], gr, tid);
        if (tid < kHdTile) {
            Ls[stage][tid] = lreg;
            Ds[stage][tid] = dreg;
        }
    };

    gload(t_lo);
    lstore(0);
    __syncthreads();

    for (int t = t_lo; t <= t_hi; ++t) {
        const int stage = (t - t_lo) & 1;
        const bool more = t < t_hi;
        if (more) gload(t + 1);
        const int qt0 = t * kHdTile;
        if (wave_live && qt0 <= wav.hi && qt0 + kHdTile - 1 >= wav.lo) {
            const char* Qt = Ts[stage][0];
            const char* Gt = Ts[stage][1];
            f32x16 sacc, dpacc;
#pragma unroll
            for (int i = 0; i < 16; ++i) sacc[i] = dpacc[i] = 0.f;
#pragma unroll
            for (int s = 0; s < H::NS; ++s) {
                sacc = mfma32(hd_frag_R<D>(Qt, s, lane), kf[s], sacc);    // S = Q K^T
                dpacc = mfma32(hd_frag_R<D>(Gt, s, lane), vf[s], dpacc);  // dP = dO V^T
            }
            // accumulator register 4 g + r is query qt0 + 8 g + 4 hh + r against this lane's key
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 l4 = *reinterpret_cast<const f32x4*>(&Ls[stage][8 * g + 4 * hh]);
                const f32x4 d4 = *reinterpret_cast<const f32x4*>(&Ds[stage][8 * g + 4 * hh]);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int q = qt0 + 8 * g + 4 * hh + r;
                    const bool ok = key_ok & (q < S) & (q >= lo) & (q <= hi);
                    const float p = ok ? __builtin_amdgcn_exp2f(__builtin_fmaf(sacc[4 * g + r], c, -l4[r])) : 0.f;
                    sacc[4 * g + r] = p;
                    dpacc[4 * g + r] = p * (dpacc[4 * g + r] - d4[r]);  // dS
                }
            }
            // dV^T += dO^T P, dK^T += Q^T dS
#pragma unroll
            for (int sp = 0; sp < 2; ++sp) {
                const bf16x8 pf = acc_to_frag(sacc, sp), df = acc_to_frag(dpacc, sp);
#pragma unroll
                for (int cb = 0; cb < H::NB; ++cb) {
                    dvacc[cb] = mfma32(hd_frag_T<D>(Gt, 16 * sp, cb, lane), pf, dvacc[cb]);
                    dkacc[cb] = mfma32(hd_frag_T<D>(Qt, 16 * sp, cb, lane), df, dkacc[cb]);
                }
            }
        }
        if (more) lstore(stage ^ 1);
        __syncthreads();
    }
    if (key < S) {
        uint16_t* dst = dqkv + ((int64_t)b * S + key) * ld + nh * D + head * D;
        hd_store_row<D>(dst, dkacc, key_ok ? scale : 0.f, hh);  // (a padded key's accumulators are zero: p = 0 throughout)
        hd_store_row<D>(dst + nh * D, dvacc, key_ok ? 1.0f : 0.f, hh);
    }
}

}  // namespace

bool cm3p_attn_hd_supported(int head_dim) { return head_dim == 96 || head_dim == 128; }

int cm3p_attn_hd_fwd(const uint16_t* qkv, uint16_t* out, float* lse, const uint8_t* key_mask, int B, int S, int nh, int head_dim, int window,
                     float scale, hipStream_t stream) {
    CM3P_REQUIRE(cm3p_attn_hd_supported(head_dim) && B <= 65535 && nh <= 65535);
    const dim3 grid((S + kHdBlock - 1) / kHdBlock, nh, B);
    if (head_dim == 96) attn_hd_fwd_kernel<96><<<grid, 256, 0, stream>>>(qkv, out, lse, key_mask, S, nh, window, scale);
    else attn_hd_fwd_kernel<128><<<grid, 256, 0, stream>>>(qkv, out, lse, key_mask, S, nh, window, scale);
    CM3P_LAUNCH_CHECK();
    return CM3P_OK;
}

int cm3p_attn_hd_bwd(const uint16_t* qkv, const uint16_t* out, const uint16_t* dout, const float* lse, float* delta, uint16_t* dqkv,
                     const uint8_t* key_mask, int B, int S, int nh, int head_dim, int window, float scale, hipStream_t stream) {
    CM3P_REQUIRE(cm3p_attn_hd_supported(head_dim) && B <= 65535 && nh <= 65535);
    const dim3 grid((S + kHdBlock - 1) / kHdBlock, nh, B);
    if (head_dim == 96) {
        attn_hd_dq_kernel<96><<<grid, 256, 0, stream>>>(qkv, out, dout, lse, delta, dqkv, key_mask, S, nh, window, scale);
        attn_hd_dkv_kernel<96><<<grid, 256, 0, stream>>>(qkv, dout, lse, delta, dqkv, key_mask, S, nh, window, scale);
    } else {
        attn_hd_dq_kernel<128><<<grid, 256, 0, stream>>>(qkv, out, dout, lse, delta, dqkv, key_mask, S, nh, window, scale);
        attn_hd_dkv_kernel<128><<<grid, 256, 0, stream>>>(qkv, dout, lse, delta, dqkv, key_mask, S, nh, window, scale);
    }
    CM3P_LAUNCH_CHECK();
    return CM3P_OK;
}
