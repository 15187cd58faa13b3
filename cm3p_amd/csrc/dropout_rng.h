// The dropout RNG contract shared by every kernel that drops (nn.Dropout at TF:models/modernbert/modeling_modernbert.py:70,91,
// 181/292, 260/300: keep with probability 1 - p, scale the survivors by 1 / (1 - p), only in training mode).
//
// A keep/drop decision is a pure function of (seed, layer, site, sequence, head, query, key or feature).  It depends on no tiling,
// grid, packed or padded layout, nor on which kernel asks, so a forward, its backward, a checkpointed recompute and a test-side
// materialiser (cm3p_dropout_keep) all see the same mask.
//
//   generator   Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; Random123 constants below)
//   key         the 64-bit seed as (low word, high word)
//   counter     c3 = 4 * layer + site          sites: 0 embedding (layer 0), 1 attention probabilities, 2 attention output, 3 MLP
//               c2 = b * nh + h (site 1)  |  b (element sites)
//               c1 = query position (site 1)  |  token position s inside its sequence (element sites)
//               c0 = key >> 3 (site 1)  |  feature >> 3 (element sites)
//   decisions   one call yields 8: decision j (key or feature 8 c0 + j) is the 16-bit half j of the output,
//               u_j = (w[j >> 1] >> (16 (j & 1))) & 0xffff, and the element is kept iff u_j >= thr, thr = round(p * 65536).
//   scale       survivors are multiplied by 65536 / (65536 - thr) (fp32), the inverse of the realised keep probability; thr = 65536
//               (p = 1) keeps nothing and scales by 0.
//
// Positions are sequence-relative: the padded row (b, s) and the packed row of the same token decide alike, so packed == padded holds
// with dropout on.  Sequences of the metadata tower's (B, V, L) batch are numbered by their flattened row.  Torch's own dropout stream
// is not reproduced (it cannot be); nothing depends on it.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define CM3P_DROP_HD __host__ __device__ __forceinline__
#else
#define CM3P_DROP_HD inline
#endif

namespace cm3p_drop {

enum : uint32_t { kSiteEmbed = 0, kSiteAttnProbs = 1, kSiteAttnOut = 2, kSiteMlp = 3 };

constexpr uint32_t kM0 = 0xD2511F53u, kM1 = 0xCD9E8D57u;  // Random123 multipliers
constexpr uint32_t kW0 = 0x9E3779B9u, kW1 = 0xBB67AE85u;  // Weyl key increments

struct U32x4 {
    uint32_t w[4];
};

CM3P_DROP_HD uint32_t mulhi32(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umulhi(a, b);
#else
    return (uint32_t)(((uint64_t)a * b) >> 32);
#endif
}

CM3P_DROP_HD U32x4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        if (r) {
            k0 += kW0;
            k1 += kW1;
        }
        const uint32_t lo0 = kM0 * c0, hi0 = mulhi32(kM0, c0);
        const uint32_t lo1 = kM1 * c2, hi1 = mulhi32(kM1, c2);
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
    }
    return U32x4{{c0, c1, c2, c3}};
}

CM3P_DROP_HD uint32_t site_word(int layer, uint32_t site) { return 4u * (uint32_t)layer + site; }

// survivors' scale for a threshold in [0, 65536]
CM3P_DROP_HD float keep_scale(uint32_t thr) { return thr >= 65536u ? 0.f : 65536.0f / (float)(65536u - thr); }

// bit j set = element 8 c0 + j kept
CM3P_DROP_HD uint32_t keep8(uint64_t seed, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t thr) {
    const U32x4 r = philox4x32_10(c0, c1, c2, c3, (uint32_t)seed, (uint32_t)(seed >> 32));
    uint32_t m = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) m |= (((r.w[j >> 1] >> (16 * (j & 1))) & 0xffffu) >= thr ? 1u : 0u) << j;
    return m;
}

// what a kernel with a dropout site receives: seed, counter word 3, threshold and the survivors' scale
struct DropCfg {
    uint64_t seed;
    uint32_t c3, thr;
    float scale;
};

CM3P_DROP_HD DropCfg make_cfg(int layer, uint32_t site, int thr, uint64_t seed) {
    return DropCfg{seed, site_word(layer, site), (uint32_t)thr, keep_scale((uint32_t)thr)};
}

// the (layer, thr) an entry point may hand to make_cfg: a threshold in [0, 65536], a layer whose counter word fits 32 bits with room
CM3P_DROP_HD bool cfg_args_ok(int layer, int thr) { return thr >= 0 && thr <= 65536 && layer >= 0 && layer < (1 << 29); }

#if defined(__HIPCC__)
// A kernel with an optional dropout site takes a trailing `Drop... drop` pack: {DropCfg} with dropout, {} without - the same kernel with
// the same signature as before it had the site.  This is the configuration either way (unread when the pack is empty).
template <typename... T>
__device__ __forceinline__ DropCfg drop_cfg(T... t) {
    if constexpr (sizeof...(T) > 0) return (t, ...);
    else return DropCfg{};
}

// Row t of an activation -> (sequence b, position s).  Padded: cu == nullptr, rows of S positions.  Packed: cu_seqlens [nseq + 1],
// b = the last sequence whose first row is <= t (alignment rows form a pseudo-sequence of their own and take no gradient).
__device__ __forceinline__ void row_to_seq(int64_t t, int S, const int* __restrict__ cu, int nseq, uint32_t& b, uint32_t& s) {
    if (cu == nullptr) {
        b = (uint32_t)(t / S);
        s = (uint32_t)(t - (int64_t)b * S);
        return;
    }
    int lo = 0, hi = nseq - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if ((int64_t)cu[mid] <= t) lo = mid;
        else hi = mid - 1;
    }
    b = (uint32_t)lo;
    s = (uint32_t)(t - cu[lo]);
}
#endif

}  // namespace cm3p_drop
