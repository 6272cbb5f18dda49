// uq_mt_jump_kernels.h — MT19937 jump-ahead on the GPU: the correlation kernel KQ0j and the block a
// run takes from its partial windows.  Included by uq_quicfl_kernels.h (the sender's and receiver's
// jump forms) and uq_randperm_kernels.h (the run starts of a permutation's word stream).
//
// The state 624 b words ahead of a stream is the correlation window_J = XOR_{k : g_k = 1}
// x[k .. k + 623] of g = t^(624 (b - 1)) mod phi (uq_mt_poly.cpp) with the stream's first
// 19937 + 623 words, then one twist (the window's word 0 carries only its top bit).

#ifndef UQ_MT_JUMP_KERNELS_H
#define UQ_MT_JUMP_KERNELS_H

#include "uq_mt19937.h"

namespace {

constexpr int kMjBlocks = 33;                 // x[0 .. 33 * 624) covers k + w <= 19936 + 623 (+ quad tails)
constexpr int kMjX = kMjBlocks * kMtN;        // stream words kept per (message, stream)
constexpr int kMjParts = 4;                   // workgroups per jump, 156 coefficient words each
constexpr int kMjSlice = 39;                  // coefficient words per wave (4 waves x 4 parts x 39 = 624)
constexpr int kMjPartWords = 4 * kMjSlice * 32 + 632;   // LDS words of a part: its coefficients + the window

struct QflJumpArgs {
    const int32_t* prng_seeds;  // local streams: init_genrand(prng_seeds[j])
    const uint32_t* px_state;   // global streams: ATen state (left, next, words) per message, or null
    const int32_t* px_seeds;    //   or fresh generators
    const uint32_t* polyA;      // [R][624]: row r = t^(624 (r L - 1)) mod phi (row 0 unused)
    const uint32_t* polyB;      // [R][624]: row r = t^(624 (qL + r L - 1)) mod phi
    uint32_t* xs;               // [n][nstreams][kMjX]: the local (and the global) stream's first words
    uint32_t* parts;            // [n][R][kinds][kMjParts][624]: partial windows (local r L, local qL + r L, global r L)
    int32_t R;
    int64_t n;
    int32_t nstreams;           // 2: the sender (local + global); 1: the receiver (local)
    int32_t kinds;              // 3: the sender's three blocks per run; 1: the receiver's local block r L
};

// acc[i] ^= XOR over the set bits t of NIB of E[t + i], E = (E0, E1): coefficient k0 + t applied
// to the four window words w0 .. w0 + 3 (x[k0 + t + w0 + i]); two terms per v_bitop3 (XOR3)
__device__ __forceinline__ uint32_t mj_xor3(uint32_t a, uint32_t b, uint32_t c) {
    return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96);
}
template <int NIB>
__device__ __forceinline__ void mj_apply(uint32_t (&acc)[4], const uint4& E0, const uint4& E1) {
    const uint32_t E[8] = {E0.x, E0.y, E0.z, E0.w, E1.x, E1.y, E1.z, E1.w};
    constexpr int t0 = (NIB & 1) ? 0 : (NIB & 2) ? 1 : (NIB & 4) ? 2 : 3;           // lowest set bit
    constexpr int R1 = NIB & (NIB - 1);                                              // the others
    constexpr int t1 = (R1 & 1) ? 0 : (R1 & 2) ? 1 : (R1 & 4) ? 2 : 3;
    constexpr int R2 = R1 & (R1 - 1);
    constexpr int t2 = (R2 & 1) ? 0 : (R2 & 2) ? 1 : (R2 & 4) ? 2 : 3;
    constexpr int R3 = R2 & (R2 - 1);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (R1 == 0) {
            acc[i] ^= E[t0 + i];
        } else {
            acc[i] = mj_xor3(acc[i], E[t0 + i], E[t1 + i]);
            if (R2 != 0 && R3 == 0) acc[i] ^= E[t2 + i];
            if (R3 != 0) acc[i] = mj_xor3(acc[i], E[t2 + i], E[3 + i]);
        }
    }
}
template <int NIB>
__device__ __forceinline__ void mj_apply3(uint32_t (&acc)[3][4], const uint4 (&E0)[3], const uint4 (&E1)[3]) {
#pragma unroll
    for (int g = 0; g < 3; ++g) mj_apply<NIB>(acc[g], E0[g], E1[g]);
}
__device__ __forceinline__ uint4 mj_quad(const uint32_t* p) {      // one ds_read_b128, never split
    typedef uint32_t u32x4v __attribute__((ext_vector_type(4)));
    typedef __attribute__((address_space(3))) const volatile u32x4v lds_q;
    const u32x4v v = *(lds_q*)p;
    return make_uint4(v.x, v.y, v.z, v.w);
}

// KQ0j: one 256-thread workgroup per (message, run, stream, part); part p's wave v takes the
// polynomial's words [156 p + 39 v, + 39) against window words 0..623 (lane quads: w0 = 256 g +
// 4 lane, group 2 lanes < 28), the stream words it reads staged in LDS; the 4 waves' partial
// windows are XORed and written out (the runs XOR the 4 parts and twist once).
__global__ void __launch_bounds__(256)
quicfl_jump_kernel(QflJumpArgs a) {
    __shared__ __attribute__((aligned(16))) uint32_t X[kMjPartWords];
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t bid = blockIdx.x;
    const int p = (int)(bid % kMjParts);
    const int64_t job = bid / kMjParts;
    const int s = (int)(job % a.kinds);
    const int64_t jr = job / a.kinds;
    const int r = (int)(jr % a.R);
    const int64_t j = jr / a.R;
    if (j >= a.n || (r == 0 && s != 1)) return;          // run 0's local-A and global blocks are the bases
    const uint32_t* poly = (s == 1 ? a.polyB : a.polyA) + (size_t)r * kMtN;
    const int wb0 = p * 4 * kMjSlice + wv * kMjSlice;
    const uint32_t pv = lane < kMjSlice ? poly[wb0 + lane] : 0u;           // the wave's coefficient words
    const int k_lo = p * 4 * kMjSlice * 32;
    const uint32_t* x = a.xs + (j * a.nstreams + (s == 2 ? 1 : 0)) * kMjX;
    {                                                    // stage x[k_lo ..): every load in flight at once
        constexpr int kQ = kMjPartWords / 4, kPer = (kQ + 255) / 256;
        typedef uint32_t u32x4v __attribute__((ext_vector_type(4)));
        u32x4v v[kPer];
#pragma unroll
        for (int t = 0; t < kPer; ++t) {
            const int q = threadIdx.x + 256 * t;
            v[t] = q < kQ && k_lo + 4 * q < kMjX ? *(const u32x4v*)(x + k_lo + 4 * q) : u32x4v{0u, 0u, 0u, 0u};
        }
#pragma unroll
        for (int t = 0; t < kPer; ++t) {
            const int q = threadIdx.x + 256 * t;
            if (q < kQ) *(u32x4v*)(X + 4 * q) = v[t];
        }
    }
    __syncthreads();
    uint32_t acc[3][4];
#pragma unroll
    for (int g = 0; g < 3; ++g)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[g][i] = 0u;
    int w0[3];
#pragma unroll
    for (int g = 0; g < 3; ++g) w0[g] = g < 2 || lane < 28 ? 256 * g + 4 * lane : 0;
    for (int wi = 0; wi < kMjSlice; ++wi) {
        const uint32_t pw = (uint32_t)__builtin_amdgcn_readlane((int)pv, wi);
        if (!pw) continue;
        const int k0 = (wb0 + wi) * 32 - k_lo;
        uint4 E0[3], E1[3];
#pragma unroll
        for (int g = 0; g < 3; ++g) E0[g] = mj_quad(X + k0 + w0[g]);
#pragma unroll
        for (int m = 0; m < 8; ++m) {
#pragma unroll
            for (int g = 0; g < 3; ++g) E1[g] = mj_quad(X + k0 + 4 * m + 4 + w0[g]);
            switch ((pw >> (4 * m)) & 15u) {
                case 1: mj_apply3<1>(acc, E0, E1); break;
                case 2: mj_apply3<2>(acc, E0, E1); break;
                case 3: mj_apply3<3>(acc, E0, E1); break;
                case 4: mj_apply3<4>(acc, E0, E1); break;
                case 5: mj_apply3<5>(acc, E0, E1); break;
                case 6: mj_apply3<6>(acc, E0, E1); break;
                case 7: mj_apply3<7>(acc, E0, E1); break;
                case 8: mj_apply3<8>(acc, E0, E1); break;
                case 9: mj_apply3<9>(acc, E0, E1); break;
                case 10: mj_apply3<10>(acc, E0, E1); break;
                case 11: mj_apply3<11>(acc, E0, E1); break;
                case 12: mj_apply3<12>(acc, E0, E1); break;
                case 13: mj_apply3<13>(acc, E0, E1); break;
                case 14: mj_apply3<14>(acc, E0, E1); break;
                case 15: mj_apply3<15>(acc, E0, E1); break;
                default: break;
            }
#pragma unroll
            for (int g = 0; g < 3; ++g) E0[g] = E1[g];
        }
    }
    __syncthreads();                                     // every wave is done with x
    uint32_t* P = X + wv * 640;                          // partial windows, 640 words apart
#pragma unroll
    for (int g = 0; g < 3; ++g) {
        const int w = 256 * g + 4 * lane;
        if (w < kMtN) *(uint4*)(P + w) = make_uint4(acc[g][0], acc[g][1], acc[g][2], acc[g][3]);
    }
    __syncthreads();
    uint32_t* out = a.parts + (((j * a.R + r) * a.kinds + s) * kMjParts + p) * kMtN;
    for (int i = threadIdx.x; i < kMtN; i += 256) out[i] = X[i] ^ X[640 + i] ^ X[1280 + i] ^ X[1920 + i];
}

// A run's block from KQ0j's parts: the window (XOR of the parts), then one twist (block b - 1's
// word 0 carries only its top bit; every word of block b is exact)
__device__ __forceinline__ void mj_block(uint32_t (&st)[kMtGroups], const uint32_t* parts, int lane) {
#pragma unroll
    for (int g = 0; g < kMtGroups; ++g) {
        const int i = 64 * g + lane;
        const int ii = i < kMtN ? i : 0;
        st[g] = parts[ii] ^ parts[kMtN + ii] ^ parts[2 * kMtN + ii] ^ parts[3 * kMtN + ii];
    }
    mt_twist_reg(st, lane);
}

}  // namespace

#endif  // UQ_MT_JUMP_KERNELS_H
