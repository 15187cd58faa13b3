// Attention for a list of query rows against all keys (include/cm3p_attn_qrows.h): forward and backward on the matrix cores
// (v_mfma_f32_32x32x16_bf16), head_dim 64, gfx950.
//
// Where the consumers of an encoder's last layer are the CLS row of each sequence and the rows that carry a masked-LM label - about
// 15 % of the rows - that layer needs attention for those queries only.  The contract is cm3p_attn_fwd / cm3p_attn_bwd's, restricted
// to the listed queries:
//     visible(b, q, kv) = key_mask[b, kv] AND (window < 0 OR |pos_q - kv| <= window), pos_q the query's position in its sequence;
//     queries with no visible key: exact zeros, lse = +inf; padded queries are computed like any other query;
//     dk / dv sum over the listed queries; invisible and padded keys receive exactly zero dK and dV; the q third of dqkv is zero off the list.
// Layout: qkv [rows, 3, nh, 64] bf16 (q, k already rotated), qrows int32 [n] global rows (ascending), qcu int32 [B + 1] the list's
// split by sequence; out / dout [n, nh, 64] bf16 and lse [nh, n] fp32 are compact in list order; dqkv has qkv's layout.
//
// Formulation: attention_hd.hip's at D = 64 (compiler-scheduled, double-buffered, fixed order), with the query side read through
// the list.  One workgroup = 4 waves; the other side arrives in tiles of 32 rows, staged in LDS as bf16 by ordinary vector loads
// and ds_write, double buffered (the next tile's global loads are issued before the products of this one, one barrier per tile).
//   forward  a workgroup takes 128 consecutive list entries ("slots") of one (sequence, head), 32 per wave, the query on the lane:
//            ONE indirection per lane.  S^T = K Q^T, P rounded to bf16 in the accumulator registers as the B operand of
//            O^T += V^T P^T.  Key tiles 0 .. len / 32 (sliding layers: the tiles the band of the workgroup's first and last
//            position can touch; a wave skips the tiles outside the band of ITS first and last position - the list is ascending, so
//            these two bound every position between them; every product that is computed is masked per element).
//   dQ       the forward's geometry: recomputes S^T, dP^T = V dO^T, dS^T = P^T o (dP^T - delta), dQ^T += K^T dS^T; the row is stored
//            at the query's own row of dqkv's q third.
//   dK, dV   a workgroup takes 128 keys of one (sequence, head), key on the lane; the sequence's list entries arrive in tiles of 32
//            slots (q through the list, dO / out / lse compact) with their positions; a slot past the list reads as zeros with
//            lse = +inf (p = 0).  Sliding layers: the slot range whose positions the key block's band can touch comes from two
//            binary searches in the (ascending) list.  This kernel also writes the zeros of the q third for its 128 rows; it runs
//            FIRST, the dQ kernel then overwrites the listed rows (same stream: ordered).
//   delta    = sum_d dO[d] out[d] from the stored bf16 out, per 16-byte chunk a chain of fused multiply-adds (dims ascending), the
//            eight chunk sums added as ((c0 + c1) + (c2 + c3)) + ((c4 + c5) + (c6 + c7)) - in BOTH backward kernels, so that they use
//            one delta in bits without a workspace between them.
// Rounding path: attention_hd.hip's (tests/attention_refs.py counts it: p and dS rounded to bf16 as MFMA operands, one bf16 store);
// the inverse rotary rotation of dq / dk, when tables are given, is applied in fp32 to the scaled accumulators before that store.
// Every sum has a fixed order: no atomics, no workspace, the same bits on every call.  LDS rows are 144 bytes apart (attention_hd.hip).
// No LDS-DMA here, hence no bounds-audit hooks (build.AUDIT_SOURCES).  Bounds: the kernels trust the list, but a sequence's row
// range is clamped to [0, total], its share of the list to [0, n] and every listed row into its sequence before an address is
// formed; loads past a tile's valid rows are predicated; every row offset is a 64-bit product.
#include "attn_common.h"

#include "../../include/cm3p_attn_qrows.h"

namespace {

constexpr int kTile = 32;     // rows of a staged tile
constexpr int kBlock = 128;   // rows (list slots or keys) of a workgroup (4 waves x 32)
constexpr int kPitch = 144;   // bytes between the LDS rows of a tile (128 + 16)
constexpr int kTileBytes = kTile * kPitch;
constexpr float kLn2 = 0.69314718055994531f;

struct QSeq {
    int64_t row0;  // first row of the sequence in the token-major tensors
    int len;       // its rows
    int q_lo, nq;  // its share of the list: slots q_lo .. q_lo + nq - 1
};
__device__ __forceinline__ QSeq q_seq(const int* __restrict__ cu, int64_t total, const int* __restrict__ qcu, int n, int b, int S) {
    QSeq s;
    if (!cu) {
        s.row0 = (int64_t)b * S;
        s.len = S;
    } else {
        int64_t r0 = cu[b], r1 = cu[b + 1];
        r0 = r0 < 0 ? 0 : (r0 > total ? total : r0);
        r1 = r1 < r0 ? r0 : (r1 > total ? total : r1);
        s.row0 = r0;
        s.len = (int)min(r1 - r0, (int64_t)S);
    }
    const int a = min(max(qcu[b], 0), n), e = min(max(qcu[b + 1], a), n);
    s.q_lo = a;
    s.nq = e - a;
    return s;
}
// position inside the sequence of list slot `slot` (0 <= slot < nq, len > 0), clamped into the sequence
__device__ __forceinline__ int slot_pos(const int* __restrict__ qrows, const QSeq& sq, int slot) {
    const int64_t p = (int64_t)qrows[sq.q_lo + slot] - sq.row0;
    return (int)(p < 0 ? 0 : (p > sq.len - 1 ? sq.len - 1 : p));
}
// first slot of the sequence whose global row is >= target (nq if none): the list is ascending
__device__ __forceinline__ int lower_slot(const int* __restrict__ qrows, const QSeq& sq, int64_t target) {
    int lo = 0, hi = sq.nq;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((int64_t)qrows[sq.q_lo + mid] < target) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// row fragment (A operand) of a staged tile: lane holds X[lane & 31][16 s + 8 (lane >> 5) + j]
__device__ __forceinline__ bf16x8 qr_frag_R(const char* tile, int s, int lane) {
    return *reinterpret_cast<const bf16x8*>(tile + (lane & 31) * kPitch + (2 * s + (lane >> 5)) * 16);
}
// A-operand fragment of X^T (rows = columns 32 cblk .. 32 cblk + 31 of the tile, k = its 16 rows from krow0) for X^T * Y with Y
// from accumulators: element j of lane half hh is row krow0 + 8 (j >> 2) + 4 hh + (j & 3) - the order acc_to_frag delivers.
__device__ __forceinline__ bf16x8 qr_frag_T(const char* tile, int krow0, int cblk, int lane) {
    const int g = lane >> 4, hh = g >> 1, i = lane & 15;
    const int row = krow0 + 4 * hh + (i >> 2);
    const int col = 32 * cblk + 16 * (g & 1) + 4 * (i & 3);
    const bf16x4 lo = lds_read_tr16(tile + row * kPitch + col * 2);
    const bf16x4 hi = lds_read_tr16(tile + (row + 8) * kPitch + col * 2);
    return cat_bf16x4(lo, hi);
}
// the lane's half of one row as MFMA B-operand fragments: element j of fragment s is column 16 s + 8 hh + j
__device__ __forceinline__ void qr_row_frags(bf16x8 (&f)[4], const uint16_t* row, int hh) {
#pragma unroll
    for (int s = 0; s < 4; ++s) f[s] = *reinterpret_cast<const bf16x8*>(row + 16 * s + 8 * hh);
}
// the thread's 16-byte chunk (tid & 7) of tile row tid >> 3 -> LDS
__device__ __forceinline__ void qr_lstore(char* tile, const uint4& v, int tid) { *reinterpret_cast<uint4*>(tile + (tid >> 3) * kPitch + (tid & 7) * 16) = v; }

// sum over one 16-byte chunk of dO o out: a product and seven fused multiply-adds, dims ascending
__device__ __forceinline__ float chunk_dot(const bf16x8& a, const bf16x8& b) {
    float s = (float)a[0] * (float)b[0];
#pragma unroll
    for (int j = 1; j < 8; ++j) s = __builtin_fmaf((float)a[j], (float)b[j], s);
    return s;
}

// accumulator blocks (lane = row, register i of block cb = column 32 cb + 8 (i >> 2) + 4 hh + (i & 3)) times mul -> one bf16 row;
// ROPE: the inverse rotary rotation a' = a cos + b sin, b' = b cos - a sin first (a = columns 0 .. 31, b = a's column + 32: both on this lane)
template <bool ROPE>
__device__ __forceinline__ void qr_store_row(uint16_t* dst, const f32x16 (&acc)[2], float mul, int hh, const float* __restrict__ cos_row,
                                             const float* __restrict__ sin_row) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        float a[4], b[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            a[r] = acc[0][4 * g + r] * mul;
            b[r] = acc[1][4 * g + r] * mul;
        }
        if constexpr (ROPE) {
            const f32x4 c4 = *reinterpret_cast<const f32x4*>(cos_row + 8 * g + 4 * hh), s4 = *reinterpret_cast<const f32x4*>(sin_row + 8 * g + 4 * hh);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float ar = __builtin_fmaf(a[r], c4[r], b[r] * s4[r]), br = __builtin_fmaf(b[r], c4[r], -(a[r] * s4[r]));
                a[r] = ar;
                b[r] = br;
            }
        }
        *reinterpret_cast<uint2*>(dst + 8 * g + 4 * hh) = uint2{pack_bf16x2(a[0], a[1]), pack_bf16x2(a[2], a[3])};
        *reinterpret_cast<uint2*>(dst + 32 + 8 * g + 4 * hh) = uint2{pack_bf16x2(b[0], b[1]), pack_bf16x2(b[2], b[3])};
    }
}
__device__ __forceinline__ void qr_zero_row(uint16_t* dst, int hh) {
#pragma unroll
    for (int g = 0; g < 8; ++g) *reinterpret_cast<uint2*>(dst + 8 * g + 4 * hh) = uint2{0u, 0u};
}

__device__ __forceinline__ float qr_max16(const f32x16& a) {
    const float m0 = max3(a[0], a[1], a[2]), m1 = max3(a[3], a[4], a[5]), m2 = max3(a[6], a[7], a[8]);
    const float m3 = max3(a[9], a[10], a[11]), m4 = max3(a[12], a[13], a[14]);
    return max3(max3(m0, m1, m2), max3(m3, m4, a[15]), m0);
}

// the geometry the forward and the dQ kernel share: the workgroup's and the wave's slots, positions and key tiles
struct QGeo {
    int slot, pos;       // the lane's list slot (may be >= nq: then `pos` is the last slot's) and position
    bool live, wave_live;
    int lo, hi;          // the lane's visible key range by the window rule
    int w_lo, w_hi;      // the keys the wave's band can touch
    int t_lo, t_hi;      // the key tiles the workgroup visits
    __device__ __forceinline__ QGeo(const int* __restrict__ qrows, const QSeq& sq, int J0, int wid, int l31, int window) {
        const int j0 = J0 + 32 * wid, last = sq.nq - 1;
        slot = j0 + l31;
        live = slot <= last;
        wave_live = j0 <= last;
        pos = slot_pos(qrows, sq, min(slot, last));
        const int b_first = slot_pos(qrows, sq, J0), b_last = slot_pos(qrows, sq, min(J0 + kBlock - 1, last));
        const int w_first = slot_pos(qrows, sq, min(j0, last)), w_last = slot_pos(qrows, sq, min(j0 + 31, last));
        lo = window < 0 ? INT_MIN : pos - window;
        hi = window < 0 ? INT_MAX : pos + window;
        w_lo = window < 0 ? 0 : max(0, w_first - window);
        w_hi = window < 0 ? sq.len - 1 : min(sq.len - 1, w_last + window);
        t_lo = (window < 0 ? 0 : max(0, b_first - window)) / kTile;
        t_hi = (window < 0 ? sq.len - 1 : min(sq.len - 1, b_last + window)) / kTile;
    }
};

// rows r0 .. r0 + 31 of the sequence's k (or v) -> the thread's chunk; rows >= len read as zero
__device__ __forceinline__ uint4 key_chunk(const uint16_t* base, int64_t ld, int r0, int len, int tid) {
    const int r = r0 + (tid >> 3);
    return r < len ? *reinterpret_cast<const uint4*>(base + (int64_t)r * ld + (tid & 7) * 8) : uint4{0u, 0u, 0u, 0u};
}

// ---------------------------------------------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------------------------------------------
template <bool PRE>
__global__ __launch_bounds__(256) void attn_qrows_fwd_kernel(const uint16_t* __restrict__ qkv, uint16_t* __restrict__ out, float* __restrict__ lse,
                                                             const uint8_t* __restrict__ kmask, const int* __restrict__ cu, int64_t total,
                                                             const int* __restrict__ qrows, const int* __restrict__ qcu, int n, int S, int nh,
                                                             int window_arg, float scale) {
    __shared__ __attribute__((aligned(16))) char Ts[2][2][kTileBytes];  // [stage][K, V]
    __shared__ __attribute__((aligned(16))) uint8_t Ms[2][kTile];        // key validity
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, hh = lane >> 5, l31 = lane & 31;
    const int head = blockIdx.y, b = blockIdx.z;
    const QSeq sq = q_seq(cu, total, qcu, n, b, S);
    const int J0 = blockIdx.x * kBlock;
    if (J0 >= sq.nq || sq.len <= 0) return;  // (the whole workgroup: no barrier has been reached)
    const int window = window_arg < 0 ? -1 : min(window_arg, S);  // (a wider band is the whole axis; keeps pos + window inside int)
    const QGeo g(qrows, sq, J0, wid, l31, window);
    const int64_t ld = (int64_t)3 * nh * 64;
    const uint16_t* qbase = qkv + sq.row0 * ld + head * 64;
    const uint16_t* kbase = qbase + nh * 64;
    const uint16_t* vbase = qbase + 2 * nh * 64;
    const float c = scale * kLog2e;

    bf16x8 qf[4];
    qr_row_frags(qf, qbase + (int64_t)g.pos * ld, hh);
    f32x16 oacc[2];
#pragma unroll
    for (int cb = 0; cb < 2; ++cb)
#pragma unroll
        for (int i = 0; i < 16; ++i) oacc[cb][i] = 0.f;
    float m_run = kNegInf, l_run = 0.f;  // log2 units; l_run: this lane half's keys

    uint4 kr, vr;
    uint8_t mreg = 0;
    auto gload = [&](int t) {
        kr = key_chunk(kbase, ld, t * kTile, sq.len, tid);
        vr = key_chunk(vbase, ld, t * kTile, sq.len, tid);
        if (tid < kTile) {
            const int key = t * kTile + tid;
            mreg = key < sq.len ? (kmask ? (uint8_t)(kmask[(int64_t)b * S + key] != 0) : (uint8_t)1) : (uint8_t)0;
        }
    };
    auto lstore = [&](int stage) {
        qr_lstore(Ts[stage][0], kr, tid);
        qr_lstore(Ts[stage][1], vr, tid);
        if (tid < kTile) Ms[stage][tid] = mreg;
    };

    gload(g.t_lo);
    lstore(0);
    __syncthreads();

    for (int t = g.t_lo; t <= g.t_hi; ++t) {
        const int stage = (t - g.t_lo) & 1;
        const bool more = t < g.t_hi;
        if (more) gload(t + 1);
        const int key0 = t * kTile;
        if (g.wave_live && key0 <= g.w_hi && key0 + kTile - 1 >= g.w_lo) {
            const char* Kt = Ts[stage][0];
            const char* Vt = Ts[stage][1];
            f32x16 sacc;
#pragma unroll
            for (int i = 0; i < 16; ++i) sacc[i] = 0.f;
#pragma unroll
            for (int s = 0; s < 4; ++s) sacc = mfma32(qr_frag_R(Kt, s, lane), qf[s], sacc);
            // accumulator register 4 gg + r is key key0 + 8 gg + 4 hh + r of this lane's query
#pragma unroll
            for (int gg = 0; gg < 4; ++gg) {
                const uint32_t mb = *reinterpret_cast<const uint32_t*>(&Ms[stage][8 * gg + 4 * hh]);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int key = key0 + 8 * gg + 4 * hh + r;
                    const bool ok = (((mb >> (8 * r)) & 0xffu) != 0u) & (key >= g.lo) & (key <= g.hi);
                    sacc[4 * gg + r] = ok ? (PRE ? sacc[4 * gg + r] : sacc[4 * gg + r] * c) : kNegInf;
                }
            }
            float mt = qr_max16(sacc);
            mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
            const float m_new = fmaxf(m_run, mt);
            const float m_use = m_new > kNegInf ? m_new : 0.f;          // (no visible key so far: every p below is exp2(-inf) = 0)
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
                for (int cb = 0; cb < 2; ++cb)
#pragma unroll
                    for (int i = 0; i < 16; ++i) oacc[cb][i] *= alpha;
            }
            // O^T += V^T P^T: P goes from the accumulators to the B operand, rounded to bf16
#pragma unroll
            for (int sp = 0; sp < 2; ++sp) {
                const bf16x8 pf = acc_to_frag(sacc, sp);
#pragma unroll
                for (int cb = 0; cb < 2; ++cb) oacc[cb] = mfma32(qr_frag_T(Vt, 16 * sp, cb, lane), pf, oacc[cb]);
            }
        }
        if (more) lstore(stage ^ 1);
        __syncthreads();
    }

    const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
    const float inv = l_tot > 0.f ? 1.0f / l_tot : 0.f;
    if (g.live) {
        const int64_t gi = (int64_t)sq.q_lo + g.slot;
        qr_store_row<false>(out + gi * nh * 64 + head * 64, oacc, inv, hh, nullptr, nullptr);
        if (hh == 0) lse[(int64_t)head * n + gi] = l_tot > 0.f ? (m_run + __log2f(l_tot)) * kLn2 : __builtin_huge_valf();
    }
}

// ---------------------------------------------------------------------------------------------------------------
// dQ (gradient w.r.t. the un-scaled rotated q): the forward's geometry; runs AFTER the dK / dV kernel (which zeroes the q third)
// ---------------------------------------------------------------------------------------------------------------
template <bool PRE, bool ROPE>
__global__ __launch_bounds__(256) void attn_qrows_dq_kernel(const uint16_t* __restrict__ qkv, const uint16_t* __restrict__ o_rows,
                                                            const uint16_t* __restrict__ d_o, const float* __restrict__ lse, uint16_t* __restrict__ dqkv,
                                                            const uint8_t* __restrict__ kmask, const int* __restrict__ cu, int64_t total,
                                                            const int* __restrict__ qrows, const int* __restrict__ qcu, int n, int S, int nh,
                                                            int window_arg, float scale, const float* __restrict__ rope_cos,
                                                            const float* __restrict__ rope_sin, int64_t pos_batch_stride) {
    __shared__ __attribute__((aligned(16))) char Ts[2][2][kTileBytes];  // [stage][K, V]
    __shared__ __attribute__((aligned(16))) uint8_t Ms[2][kTile];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, hh = lane >> 5, l31 = lane & 31;
    const int head = blockIdx.y, b = blockIdx.z;
    const QSeq sq = q_seq(cu, total, qcu, n, b, S);
    const int J0 = blockIdx.x * kBlock;
    if (J0 >= sq.nq || sq.len <= 0) return;
    const int window = window_arg < 0 ? -1 : min(window_arg, S);
    const QGeo g(qrows, sq, J0, wid, l31, window);
    const int64_t ld = (int64_t)3 * nh * 64, ldo = (int64_t)nh * 64;
    const uint16_t* qbase = qkv + sq.row0 * ld + head * 64;
    const uint16_t* kbase = qbase + nh * 64;
    const uint16_t* vbase = qbase + 2 * nh * 64;
    const float c = scale * kLog2e;
    const int64_t gi = (int64_t)sq.q_lo + min(g.slot, sq.nq - 1);

    bf16x8 qf[4], gf[4];
    qr_row_frags(qf, qbase + (int64_t)g.pos * ld, hh);
    qr_row_frags(gf, d_o + gi * ldo + head * 64, hh);
    float dlt;
    {
        // the lane half holds chunks hh, 2 + hh, 4 + hh, 6 + hh of the row; the dK / dV kernel adds the same eight chunk sums in the same tree
        bf16x8 of[4];
        qr_row_frags(of, o_rows + gi * ldo + head * 64, hh);
        float pr[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const float cs = chunk_dot(gf[s], of[s]);
            pr[s] = cs + __shfl_xor(cs, 32, 64);  // c(2 s) + c(2 s + 1)
        }
        dlt = (pr[0] + pr[1]) + (pr[2] + pr[3]);
    }
    const float lse2 = lse[(int64_t)head * n + gi] * kLog2e;  // +inf (no visible key): p = 0 everywhere

    f32x16 dqacc[2];
#pragma unroll
    for (int cb = 0; cb < 2; ++cb)
#pragma unroll
        for (int i = 0; i < 16; ++i) dqacc[cb][i] = 0.f;

    uint4 kr, vr;
    uint8_t mreg = 0;
    auto gload = [&](int t) {
        kr = key_chunk(kbase, ld, t * kTile, sq.len, tid);
        vr = key_chunk(vbase, ld, t * kTile, sq.len, tid);
        if (tid < kTile) {
            const int key = t * kTile + tid;
            mreg = key < sq.len ? (kmask ? (uint8_t)(kmask[(int64_t)b * S + key] != 0) : (uint8_t)1) : (uint8_t)0;
        }
    };
    auto lstore = [&](int stage) {
        qr_lstore(Ts[stage][0], kr, tid);
        qr_lstore(Ts[stage][1], vr, tid);
        if (tid < kTile) Ms[stage][tid] = mreg;
    };

    gload(g.t_lo);
    lstore(0);
    __syncthreads();

    for (int t = g.t_lo; t <= g.t_hi; ++t) {
        const int stage = (t - g.t_lo) & 1;
        const bool more = t < g.t_hi;
        if (more) gload(t + 1);
        const int key0 = t * kTile;
        if (g.wave_live && key0 <= g.w_hi && key0 + kTile - 1 >= g.w_lo) {
            const char* Kt = Ts[stage][0];
            const char* Vt = Ts[stage][1];
            f32x16 sacc, dpacc;
#pragma unroll
            for (int i = 0; i < 16; ++i) sacc[i] = dpacc[i] = 0.f;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                sacc = mfma32(qr_frag_R(Kt, s, lane), qf[s], sacc);    // S^T = K Q^T
                dpacc = mfma32(qr_frag_R(Vt, s, lane), gf[s], dpacc);  // dP^T = V dO^T
            }
#pragma unroll
            for (int gg = 0; gg < 4; ++gg) {
                const uint32_t mb = *reinterpret_cast<const uint32_t*>(&Ms[stage][8 * gg + 4 * hh]);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int key = key0 + 8 * gg + 4 * hh + r;
                    const bool ok = (((mb >> (8 * r)) & 0xffu) != 0u) & (key >= g.lo) & (key <= g.hi);
                    const float e = PRE ? sacc[4 * gg + r] - lse2 : __builtin_fmaf(sacc[4 * gg + r], c, -lse2);
                    const float p = ok ? __builtin_amdgcn_exp2f(e) : 0.f;
                    sacc[4 * gg + r] = p * (dpacc[4 * gg + r] - dlt);  // dS^T
                }
            }
            // dQ^T += K^T dS^T
#pragma unroll
            for (int sp = 0; sp < 2; ++sp) {
                const bf16x8 df = acc_to_frag(sacc, sp);
#pragma unroll
                for (int cb = 0; cb < 2; ++cb) dqacc[cb] = mfma32(qr_frag_T(Kt, 16 * sp, cb, lane), df, dqacc[cb]);
            }
        }
        if (more) lstore(stage ^ 1);
        __syncthreads();
    }
    if (g.live) {
        const int64_t tr = (cu ? sq.row0 : (int64_t)b * pos_batch_stride) + g.pos;
        qr_store_row<ROPE>(dqkv + (sq.row0 + g.pos) * ld + head * 64, dqacc, scale, hh, ROPE ? rope_cos + tr * 32 : nullptr,
                           ROPE ? rope_sin + tr * 32 : nullptr);
    }
}

// ---------------------------------------------------------------------------------------------------------------
// dK, dV and the zeros of the q third: one workgroup = 128 keys, 32 per wave, key on the lane; tiles of 32 list slots (q, dO, lse,
// delta, position) staged in LDS
// ---------------------------------------------------------------------------------------------------------------
template <bool PRE, bool ROPE>
__global__ __launch_bounds__(256) void attn_qrows_dkv_kernel(const uint16_t* __restrict__ qkv, const uint16_t* __restrict__ o_rows,
                                                             const uint16_t* __restrict__ d_o, const float* __restrict__ lse, uint16_t* __restrict__ dqkv,
                                                             const uint8_t* __restrict__ kmask, const int* __restrict__ cu, int64_t total,
                                                             const int* __restrict__ qrows, const int* __restrict__ qcu, int n, int S, int nh,
                                                             int window_arg, float scale, const float* __restrict__ rope_cos,
                                                             const float* __restrict__ rope_sin, int64_t pos_batch_stride) {
    __shared__ __attribute__((aligned(16))) char Ts[2][2][kTileBytes];  // [stage][Q, dO]
    __shared__ __attribute__((aligned(16))) float Ls[2][kTile], Ds[2][kTile];
    __shared__ __attribute__((aligned(16))) int Ps[2][kTile];           // the slots' positions
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, hh = lane >> 5, l31 = lane & 31;
    const int head = blockIdx.y, b = blockIdx.z;
    const QSeq sq = q_seq(cu, total, qcu, n, b, S);
    const int K0 = blockIdx.x * kBlock;
    if (K0 >= sq.len) return;  // (also a sequence without rows)
    const int window = window_arg < 0 ? -1 : min(window_arg, S);
    const int k0 = K0 + 32 * wid, key = k0 + l31, kc = min(key, sq.len - 1);
    const int64_t ld = (int64_t)3 * nh * 64, ldo = (int64_t)nh * 64;
    const uint16_t* qbase = qkv + sq.row0 * ld + head * 64;
    const float c = scale * kLog2e;

    bf16x8 kf[4], vf[4];
    qr_row_frags(kf, qbase + (int64_t)kc * ld + nh * 64, hh);
    qr_row_frags(vf, qbase + (int64_t)kc * ld + 2 * nh * 64, hh);
    const bool key_ok = key < sq.len && (kmask ? kmask[(int64_t)b * S + kc] != 0 : true);
    f32x16 dkacc[2], dvacc[2];
#pragma unroll
    for (int cb = 0; cb < 2; ++cb)
#pragma unroll
        for (int i = 0; i < 16; ++i) dkacc[cb][i] = dvacc[cb][i] = 0.f;

    const int lo = window < 0 ? INT_MIN : key - window, hi = window < 0 ? INT_MAX : key + window;
    const int w_lo = window < 0 ? 0 : max(0, k0 - window), w_hi = window < 0 ? sq.len - 1 : min(sq.len - 1, k0 + 31 + window);
    const bool wave_live = k0 < sq.len;
    // the slots whose positions the band of keys K0 .. K0 + 127 can touch
    int s_lo = 0, s_hi = sq.nq - 1;
    if (window >= 0 && sq.nq > 0) {
        s_lo = lower_slot(qrows, sq, sq.row0 + max(0, K0 - window));
        s_hi = lower_slot(qrows, sq, sq.row0 + (int64_t)min(sq.len - 1, K0 + kBlock - 1 + window) + 1) - 1;
    }
    const bool any = s_lo <= s_hi;
    const int t_lo = any ? s_lo / kTile : 1, t_hi = any ? s_hi / kTile : 0;

    uint4 qr, gr;
    float lreg = 0.f, dreg = 0.f;
    int preg = 0;
    auto gload = [&](int t) {  // thread = (slot t * 32 + (tid >> 3), chunk tid & 7)
        const int slot = t * kTile + (tid >> 3), ch = tid & 7;
        const bool valid = slot < sq.nq;
        const int sc = min(slot, sq.nq - 1);
        const int pos = slot_pos(qrows, sq, sc);
        const int64_t gi = (int64_t)sq.q_lo + sc;
        uint4 orow = uint4{0u, 0u, 0u, 0u};
        qr = gr = orow;
        if (valid) {
            qr = *reinterpret_cast<const uint4*>(qbase + (int64_t)pos * ld + ch * 8);
            gr = *reinterpret_cast<const uint4*>(d_o + gi * ldo + head * 64 + ch * 8);
            orow = *reinterpret_cast<const uint4*>(o_rows + gi * ldo + head * 64 + ch * 8);
        }
        float d = chunk_dot(*reinterpret_cast<const bf16x8*>(&gr), *reinterpret_cast<const bf16x8*>(&orow));
        d += __shfl_xor(d, 1, 64);  // c(2 s) + c(2 s + 1)
        d += __shfl_xor(d, 2, 64);
        d += __shfl_xor(d, 4, 64);
        dreg = d;
        lreg = valid ? lse[(int64_t)head * n + gi] * kLog2e : __builtin_huge_valf();  // slots past the list: p = 0
        preg = pos;
    };
    auto lstore = [&](int stage) {
        qr_lstore(Ts[stage][0], qr, tid);
        qr_lstore(Ts[stage][1], gr, tid);
        if ((tid & 7) == 0) {
            Ls[stage][tid >> 3] = lreg;
            Ds[stage][tid >> 3] = dreg;
            Ps[stage][tid >> 3] = preg;
        }
    };

    if (any) {
        gload(t_lo);
        lstore(0);
    }
    __syncthreads();

    for (int t = t_lo; t <= t_hi; ++t) {
        const int stage = (t - t_lo) & 1;
        const bool more = t < t_hi;
        if (more) gload(t + 1);
        const int qt0 = t * kTile;
        const int p_first = Ps[stage][0], p_last = Ps[stage][min(kTile - 1, sq.nq - 1 - qt0)];  // ascending: they bound the tile's positions
        if (wave_live && p_first <= w_hi && p_last >= w_lo) {
            const char* Qt = Ts[stage][0];
            const char* Gt = Ts[stage][1];
            f32x16 sacc, dpacc;
#pragma unroll
            for (int i = 0; i < 16; ++i) sacc[i] = dpacc[i] = 0.f;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                sacc = mfma32(qr_frag_R(Qt, s, lane), kf[s], sacc);    // S = Q K^T
                dpacc = mfma32(qr_frag_R(Gt, s, lane), vf[s], dpacc);  // dP = dO V^T
            }
            // accumulator register 4 gg + r is slot qt0 + 8 gg + 4 hh + r against this lane's key
#pragma unroll
            for (int gg = 0; gg < 4; ++gg) {
                const f32x4 l4 = *reinterpret_cast<const f32x4*>(&Ls[stage][8 * gg + 4 * hh]);
                const f32x4 d4 = *reinterpret_cast<const f32x4*>(&Ds[stage][8 * gg + 4 * hh]);
                const int4 p4 = *reinterpret_cast<const int4*>(&Ps[stage][8 * gg + 4 * hh]);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int q = r == 0 ? p4.x : (r == 1 ? p4.y : (r == 2 ? p4.z : p4.w));
                    const bool ok = key_ok & (qt0 + 8 * gg + 4 * hh + r < sq.nq) & (q >= lo) & (q <= hi);
                    const float e = PRE ? sacc[4 * gg + r] - l4[r] : __builtin_fmaf(sacc[4 * gg + r], c, -l4[r]);
                    const float p = ok ? __builtin_amdgcn_exp2f(e) : 0.f;
                    sacc[4 * gg + r] = p;
                    dpacc[4 * gg + r] = p * (dpacc[4 * gg + r] - d4[r]);  // dS
                }
            }
            // dV^T += dO^T P, dK^T += Q^T dS
#pragma unroll
            for (int sp = 0; sp < 2; ++sp) {
                const bf16x8 pf = acc_to_frag(sacc, sp), df = acc_to_frag(dpacc, sp);
#pragma unroll
                for (int cb = 0; cb < 2; ++cb) {
                    dvacc[cb] = mfma32(qr_frag_T(Gt, 16 * sp, cb, lane), pf, dvacc[cb]);
                    dkacc[cb] = mfma32(qr_frag_T(Qt, 16 * sp, cb, lane), df, dkacc[cb]);
                }
            }
        }
        if (more) lstore(stage ^ 1);
        __syncthreads();
    }
    if (key < sq.len) {
        uint16_t* dst = dqkv + (sq.row0 + key) * ld + head * 64;
        qr_zero_row(dst, hh);  // the q third: the dQ kernel overwrites the listed rows afterwards
        if (key_ok) {
            const int64_t tr = (cu ? sq.row0 : (int64_t)b * pos_batch_stride) + key;
            qr_store_row<ROPE>(dst + nh * 64, dkacc, PRE ? kLn2 : scale, hh, ROPE ? rope_cos + tr * 32 : nullptr, ROPE ? rope_sin + tr * 32 : nullptr);
            qr_store_row<false>(dst + 2 * nh * 64, dvacc, 1.0f, hh, nullptr, nullptr);
        } else {
            qr_zero_row(dst + nh * 64, hh);
            qr_zero_row(dst + 2 * nh * 64, hh);
        }
    }
}

bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

bool qrows_args_ok(const void* qkv, const void* out, const float* lse, const uint8_t* key_mask, const int* cu, const int* qrows, const int* qcu, int n,
                   int qmax, int B, int S, int64_t total, int nh, float scale) {
    if (!(qkv && qcu && cm3p_aligned16(qkv) && cm3p_aligned16(out) && cm3p_aligned16(lse) && aligned4(cu) && aligned4(qrows) && aligned4(qcu))) return false;
    if (!(B > 0 && S > 0 && nh > 0 && n >= 0 && total > 0 && scale > 0.f) || (key_mask && cu)) return false;
    if (n > 0 && !(qmax > 0 && out && lse && qrows)) return false;
    if (!cu && total != (int64_t)B * S) return false;
    return B <= 65535 && nh <= 65535 && total < (int64_t(1) << 31) && (int64_t)nh * 192 < (int64_t(1) << 31);  // (grid limits; qrows are int32 rows)
}

}  // namespace

extern "C" {

int cm3p_attn_qrows_abi_version(void) { return CM3P_ATTN_QROWS_ABI_VERSION; }

int cm3p_attn_qrows_fwd(const void* qkv, void* out, float* lse, const uint8_t* key_mask, const int* cu_seqlens, const int* qrows, const int* qcu, int n,
                        int qmax, int B, int S, int64_t total, int nh, int window, float scale, int q_prescaled, void* stream) {
    CM3P_REQUIRE(qrows_args_ok(qkv, out, lse, key_mask, cu_seqlens, qrows, qcu, n, qmax, B, S, total, nh, scale));
    if (n == 0) return CM3P_OK;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid((min(qmax, n) + kBlock - 1) / kBlock, nh, B);
    const uint16_t* x = static_cast<const uint16_t*>(qkv);
    uint16_t* o = static_cast<uint16_t*>(out);
    if (q_prescaled) attn_qrows_fwd_kernel<true><<<grid, 256, 0, st>>>(x, o, lse, key_mask, cu_seqlens, total, qrows, qcu, n, S, nh, window, scale);
    else attn_qrows_fwd_kernel<false><<<grid, 256, 0, st>>>(x, o, lse, key_mask, cu_seqlens, total, qrows, qcu, n, S, nh, window, scale);
    CM3P_LAUNCH_CHECK();
    return CM3P_OK;
}

int cm3p_attn_qrows_bwd(const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv, const uint8_t* key_mask, const int* cu_seqlens,
                        const int* qrows, const int* qcu, int n, int qmax, int B, int S, int64_t total, int nh, int window, float scale,
                        const float* cos_tab, const float* sin_tab, int64_t pos_batch_stride, int q_prescaled, void* stream) {
    CM3P_REQUIRE(qrows_args_ok(qkv, out, lse, key_mask, cu_seqlens, qrows, qcu, n, qmax, B, S, total, nh, scale));
    CM3P_REQUIRE(dqkv && cm3p_aligned16(dqkv) && cm3p_aligned16(dout) && (n == 0 || dout));
    CM3P_REQUIRE((cos_tab == nullptr) == (sin_tab == nullptr) && cm3p_aligned16(cos_tab) && cm3p_aligned16(sin_tab));
    CM3P_REQUIRE(pos_batch_stride == 0 || pos_batch_stride == S);
    const hipStream_t st = static_cast<hipStream_t>(stream);
    if (n == 0) {
        if (hipMemsetAsync(dqkv, 0, (size_t)total * 3 * nh * 64 * sizeof(uint16_t), st) != hipSuccess) return CM3P_ERR_LAUNCH;
        return CM3P_OK;
    }
    const dim3 grid_k((S + kBlock - 1) / kBlock, nh, B), grid_q((min(qmax, n) + kBlock - 1) / kBlock, nh, B);
    auto go = [&](auto pre, auto rope) {
        constexpr bool P = decltype(pre)::value, R = decltype(rope)::value;
        const uint16_t* x = static_cast<const uint16_t*>(qkv);
        const uint16_t* o = static_cast<const uint16_t*>(out);
        const uint16_t* g = static_cast<const uint16_t*>(dout);
        uint16_t* d = static_cast<uint16_t*>(dqkv);
        attn_qrows_dkv_kernel<P, R><<<grid_k, 256, 0, st>>>(x, o, g, lse, d, key_mask, cu_seqlens, total, qrows, qcu, n, S, nh, window, scale, cos_tab, sin_tab,
                                                            pos_batch_stride);
        attn_qrows_dq_kernel<P, R><<<grid_q, 256, 0, st>>>(x, o, g, lse, d, key_mask, cu_seqlens, total, qrows, qcu, n, S, nh, window, scale, cos_tab, sin_tab,
                                                           pos_batch_stride);
        return CM3P_OK;
    };
    const int rc = cm3p_with_layout(q_prescaled != 0, cos_tab != nullptr, go);
    if (rc != CM3P_OK) return rc;
    CM3P_LAUNCH_CHECK();
    return CM3P_OK;
}

}  // extern "C"
