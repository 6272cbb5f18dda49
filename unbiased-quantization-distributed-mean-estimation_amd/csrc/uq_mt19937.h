// uq_mt19937.h — ATen's mt19937 on one wave: a 624-word block in registers, its twist, the
// tempering, torch's 24-bit uniform and the (left, next, words) generator state.  Included by
// uq_quicfl_kernels.h (the sender's and receiver's streams) and uq_rand_kernels.h (the stream
// walker of Scalar_quantize and DRIVE_quantize_Hadamard).

#ifndef UQ_MT19937_H
#define UQ_MT19937_H

#include "uq_common.h"

namespace {

constexpr int kMtN = 624;              // MT19937 state words
constexpr int kMtGroups = 10;          // 64-word groups per block (the last one 48 words)
constexpr int kQfStateWords = 2 + kMtN;             // (left, next, words) per generator state

__device__ __forceinline__ uint32_t mt_temper(uint32_t y) {
    y ^= y >> 11;
    y ^= (y << 7) & 0x9D2C5680u;
    y ^= (y << 15) & 0xEFC60000u;
    y ^= y >> 18;
    return y;
}

// new word = c ^ twist(a, b) (ATen mt19937::next_state)
__device__ __forceinline__ uint32_t mt_mix(uint32_t a, uint32_t b, uint32_t c) {
    const uint32_t y = (a & 0x80000000u) | (b & 0x7FFFFFFFu);
    return c ^ (y >> 1) ^ ((y & 1u) ? 0x9908B0DFu : 0u);
}

// torch's uniform in bernoulli: (w & 0xFFFFFF) * 2^-24 (computed in double, then compared with
// the f32 p): both sides are exact f32 values, so the f32 comparison is the same test
__device__ __forceinline__ float u24(uint32_t w) { return (float)(w & 0xFFFFFFu) * 0x1p-24f; }

__device__ __forceinline__ void mt_seed(uint32_t* mt, uint32_t seed) {     // init_genrand, one lane
    mt[0] = seed;
    for (int i = 1; i < kMtN; ++i) mt[i] = 1812433253u * (mt[i - 1] ^ (mt[i - 1] >> 30)) + (uint32_t)i;
}

// A block in registers: word 64 g + lane in s[g] (g = 9: lanes < 48).  One wave twists it into
// the next block (ATen's next_state): word i takes s[i], s[i + 1] (old) and s[(i + 397) % 624],
// which is old for i < 227 and new (227 words back) otherwise.  Operands move between lanes by
// a DPP wave shift (the +1 neighbour) and ds_bpermute (the +13 / +29 lane rotations of the c
// operand); the groups' dependencies (group g >= 4 needs new groups g-4 and g-3) leave four
// levels.  tools/exp/mt_twist_bench.hip: 0.59 us per twist (+ temper) against 1.39 us for the
// LDS in-place form with its wave fences, bit-identical to a host MT19937.
__device__ __forceinline__ uint32_t mt_perm(uint32_t v, int src_lane) {
    return (uint32_t)__builtin_amdgcn_ds_bpermute(src_lane << 2, (int)v);
}
__device__ __forceinline__ void mt_twist_reg(uint32_t (&s)[kMtGroups], int lane) {
    const int r13 = (lane + 13) & 63, r29 = (lane + 29) & 63;
    uint32_t b[kMtGroups], N[kMtGroups];
#pragma unroll
    for (int g = 0; g < kMtGroups; ++g) {                       // b = old word i + 1
        const uint32_t nx = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)s[g], 0x130, 0xF, 0xF, false);  // wave_shl:1
        const uint32_t first = g + 1 < kMtGroups ? (uint32_t)__builtin_amdgcn_readlane((int)s[g + 1], 0) : 0u;
        b[g] = lane == 63 ? first : nx;
    }
#pragma unroll
    for (int g = 0; g < 3; ++g) {                               // i < 192: c = old word i + 397
        const uint32_t t1 = mt_perm(s[g + 6], r13), t2 = mt_perm(s[g + 7], r13);
        N[g] = mt_mix(s[g], b[g], lane < 51 ? t1 : t2);
    }
    {                                                           // i = 192..255: old s[9] below 227, new N[0] above
        const uint32_t t1 = mt_perm(s[9], r13), t2 = mt_perm(N[0], r29);
        N[3] = mt_mix(s[3], b[3], lane < 35 ? t1 : t2);
    }
#pragma unroll
    for (int g = 4; g < kMtGroups; ++g) {                       // c = new word i - 227
        const uint32_t t1 = mt_perm(N[g - 4], r29), t2 = mt_perm(N[g - 3], r29);
        uint32_t bb = b[g];
        if (g == kMtGroups - 1) {                               // word 623 twists with the new word 0
            const uint32_t n0 = (uint32_t)__builtin_amdgcn_readlane((int)N[0], 0);
            bb = lane == 47 ? n0 : bb;
        }
        N[g] = mt_mix(s[g], bb, lane < 35 ? t1 : t2);
    }
#pragma unroll
    for (int g = 0; g < kMtGroups; ++g) s[g] = N[g];
}
__device__ __forceinline__ void mt_load(uint32_t (&s)[kMtGroups], const uint32_t* src, int lane) {
#pragma unroll
    for (int g = 0; g < kMtGroups; ++g) {
        const int i = 64 * g + lane;
        s[g] = src[i < kMtN ? i : 0];
    }
}
__device__ __forceinline__ void mt_store(const uint32_t (&s)[kMtGroups], uint32_t* dst, int lane) {
#pragma unroll
    for (int g = 0; g < kMtGroups; ++g) {
        const int i = 64 * g + lane;
        if (i < kMtN) dst[i] = s[g];
    }
}

// The global generator's state after the message's D draws: the block holding word D - 1
// (sG after the last round) and ATen's (left, next) for it.
__device__ __forceinline__ void qfl_state_out(uint32_t* so, const uint32_t (&sG)[kMtGroups], int64_t D, int32_t gleft,
                                              int32_t gnext, int64_t vG, int lane) {
    uint32_t left1, next1;
    if (D <= (int64_t)gleft - 1) {                               // every draw from the current block
        left1 = (uint32_t)(gleft - D);
        next1 = (uint32_t)(gnext + D);
    } else {
        const int64_t pos = (vG + D - 1) % kMtN;
        next1 = (uint32_t)(pos + 1);
        left1 = (uint32_t)(kMtN - pos);
    }
    mt_store(sG, so + 2, lane);
    if (lane == 0) {
        so[0] = left1;
        so[1] = next1;
    }
}

}  // namespace

#endif  // UQ_MT19937_H
