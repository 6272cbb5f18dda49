// uq_rand_kernels.h — the two baselines that draw torch.rand_like from the global CPU
// generator (AS = NMSE_Results/Codes/All_Schemes.py).  Included by uq_rand.hip.
//
// torch.rand_like(v) on CPU takes one MT19937 word per element in index order,
// u = f32(w & 0xFFFFFF) * 2^-24.  The stream is serial (624-word blocks, each twisted from the
// previous), so ONE WAVE per client walks it (rand_walk) from the client's generator state
// (left, next, words) with the block in registers, and hands every tempered word to the
// scheme: lane l of a block's group g holds word 64 g + l, so a group's 64 words belong to 64
// consecutive coordinates.
//   Scalar_quantize, AS:755-790
//     KR1 scalar_minmax_kernel   min / max / has-NaN of slices of each client (partials)
//     KR2 scalar_walk_kernel     the partials folded (den == 0: out = x, no word taken), else the
//                                walk fused with AS:768-788, one f32 operation per step
//   DRIVE_quantize_Hadamard, AS:707-752 (bits_per_dimension unused, chunks of 2048)
//     KR3 drive_bits_kernel      the walk: D = u > 0.5 as one bit per word (a ballot per group)
//     KR4 drive_chunk_kernel     one workgroup per (chunk, client): everything else
// AS:37-59's "transform" writes through aliasing views: each of its log2(P) stages maps every
// adjacent pair (a, b) to (s, s - b), s = a + b, so a thread's four pairs never leave it.

#ifndef UQ_RAND_KERNELS_H
#define UQ_RAND_KERNELS_H

#include "uq_mt19937.h"

namespace {

constexpr int kRwWavesPerWG = 4;           // clients per workgroup of the walkers (one wave each)
constexpr int kDriveChunk = 2048;          // AS:712 batch_size
constexpr int kMinMaxParts = 64;           // slices per client at most (one per lane of KR2's fold)
constexpr int kMinMaxSlice = 4096;         // coordinates per slice at least

struct RandGen {
    const uint32_t* px_state;   // [n][2 + 624] generator state per client, or null
    const int32_t* px_seeds;    // [n] seeds of fresh generators (when px_state is null)
    uint32_t* px_state_out;     // [n][2 + 624] state after the client's words, or null
};

// Client j's generator into registers: ATen's state, or a fresh one (init_genrand by one lane).
__device__ __forceinline__ void rand_gen_init(const RandGen& a, int64_t j, uint32_t (&s)[kMtGroups], uint32_t* scratch,
                                              int32_t& gleft, int32_t& gnext, int lane) {
    gleft = 1;
    gnext = 0;
    if (a.px_state) {
        const uint32_t* st = a.px_state + j * kQfStateWords;
        gleft = __builtin_amdgcn_readfirstlane((int32_t)st[0]);     // scalars: the walk's bounds stay wave-uniform
        gnext = __builtin_amdgcn_readfirstlane((int32_t)st[1]);
        mt_load(s, st + 2, lane);
    } else {
        if (lane == 0) mt_seed(scratch, (uint32_t)a.px_seeds[j]);
        wave_lds_fence();
        mt_load(s, scratch, lane);
    }
}

// The next N words of the stream whose current block is in s: the first left - 1 of them are
// state[next ..], the rest come from twisted blocks.  Slot 0 of block 0 (the state as given) is
// virtual position 0 and word 0 sits at vG.  For every group of every block the walk touches,
// f(i0, lo, hi, w, v, lane): this lane's tempered word w is word i0 + lane, and it is one of the
// N for lo <= lane < hi (wave-uniform bounds, in index order from call to call; lo = hi = 0
// where the group holds none: no branch per group, the walk's edges are two blocks).  v is what
// pre(i0, lo, hi, lane) returned for the same group: the indices do not depend on the words,
// so pre runs one block ahead and what it loads is in flight across a twist and a block of f.
// On return s is the block of word N - 1, which qfl_state_out stores with ATen's (left, next).
struct RandGroup {
    int64_t i0;
    int lo, hi;
};
__device__ __forceinline__ RandGroup rand_group(int64_t base, int g, int64_t N) {
    RandGroup r;
    r.i0 = base + 64 * g;
    const int width = g == kMtGroups - 1 ? kMtN - 64 * g : 64;
    r.lo = r.i0 < 0 ? (int)std::min<int64_t>(-r.i0, 64) : 0;
    r.hi = (int)std::min<int64_t>(width, N - r.i0);
    if (r.hi <= r.lo) r.lo = r.hi = 0;                          // none of the N words: an empty range
    return r;
}
template <class P, class F>
__device__ __forceinline__ void rand_walk(uint32_t (&s)[kMtGroups], int32_t gleft, int32_t gnext, int64_t N, int lane,
                                          P&& pre, F&& f) {
    if (N <= 0) return;
    using T = decltype(pre((int64_t)0, 0, 0, 0));
    const int64_t vG = gleft > 1 ? (int64_t)gnext : (int64_t)kMtN;
    const int64_t b0 = vG / kMtN, b1 = (vG + N - 1) / kMtN;      // b0: block 0 or 1
    T nxt[kMtGroups], cur[kMtGroups];
    auto fetch = [&](int64_t b) {
#pragma unroll
        for (int g = 0; g < kMtGroups; ++g) {
            const RandGroup r = rand_group(b * kMtN - vG, g, N);
            nxt[g] = pre(r.i0, r.lo, r.hi, lane);
        }
    };
    fetch(b0);
    for (int64_t b = b0; b <= b1; ++b) {
        if (b > 0) mt_twist_reg(s, lane);
#pragma unroll
        for (int g = 0; g < kMtGroups; ++g) cur[g] = nxt[g];
        if (b < b1) fetch(b + 1);
#pragma unroll
        for (int g = 0; g < kMtGroups; ++g) {
            const RandGroup r = rand_group(b * kMtN - vG, g, N);   // word index of the block's slot 0, + 64 g
            f(r.i0, r.lo, r.hi, mt_temper(s[g]), cur[g], lane);
        }
    }
}

__device__ __forceinline__ int64_t rand_vg(int32_t gleft, int32_t gnext) {
    return gleft > 1 ? (int64_t)gnext : (int64_t)kMtN;
}

// ---- Scalar_quantize ---------------------------------------------------------------------
// KR1: workgroup (p, j) folds slice p of client j into part[j][p] = (min, max, has NaN).  min
// and max are exact, so the order is free; fminf / fmaxf skip NaN, which the flag carries.
__global__ void __launch_bounds__(kQBlock)
scalar_minmax_kernel(const float* __restrict__ x, int64_t d, int32_t parts, float4* __restrict__ part) {
    __shared__ float sm[3][kQBlock / kWave];
    const int64_t j = blockIdx.x / parts;
    const int p = (int)(blockIdx.x % parts);
    const int64_t len = (d + parts - 1) / parts;
    const int64_t i0 = std::min<int64_t>(d, p * len), i1 = std::min<int64_t>(d, i0 + len);
    const float* xr = x + j * d;
    float mn = INFINITY, mx = -INFINITY, nan = 0.f;
    for (int64_t i = i0 + threadIdx.x; i < i1; i += kQBlock) {
        const float v = xr[i];
        nan = v != v ? 1.f : nan;
        mn = fminf(mn, v);
        mx = fmaxf(mx, v);
    }
    for (int s = 32; s >= 1; s >>= 1) {
        mn = fminf(mn, __shfl_xor(mn, s));
        mx = fmaxf(mx, __shfl_xor(mx, s));
        nan = fmaxf(nan, __shfl_xor(nan, s));
    }
    const int wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        sm[0][wv] = mn;
        sm[1][wv] = mx;
        sm[2][wv] = nan;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kQBlock / kWave; ++w) {
            mn = fminf(mn, sm[0][w]);
            mx = fmaxf(mx, sm[1][w]);
            nan = fmaxf(nan, sm[2][w]);
        }
        part[blockIdx.x] = make_float4(mn, mx, nan, 0.f);
    }
}

// KR2: one wave per client.  x_min, x_max (NaN when the client holds one, as torch's min / max)
// and den = x_max - x_min (AS:759-761); den == 0 (AS:763): out = x, no word taken, the state
// passes through.  Else coordinate i takes word i:
//   q = clamp((x - mn) / den, 0, 1); t = q * nl; fl = floor(t); fr = t - fl;
//   b = fl + (u < fr); out = (b / nl) * den + mn                                  (AS:768-788)
// each a single f32 operation (the unit is built without contraction, with IEEE division).
__global__ void __launch_bounds__(64 * kRwWavesPerWG)
scalar_walk_kernel(const float* __restrict__ x, float* __restrict__ out, int64_t n, int64_t d, float nl,
                   const float4* __restrict__ part, int32_t parts, RandGen gen, int32_t* __restrict__ info) {
    __shared__ uint32_t seed_scratch[kRwWavesPerWG][kMtN];
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // wave-uniform: j, the walk's bounds
    const int64_t j = (int64_t)blockIdx.x * kRwWavesPerWG + wv;
    if (j >= n) return;                                         // whole wave: no barrier below
    float mn = INFINITY, mx = -INFINITY, nan = 0.f;
    if (lane < parts) {
        const float4 t = part[j * parts + lane];
        mn = t.x;
        mx = t.y;
        nan = t.z;
    }
    for (int s = 32; s >= 1; s >>= 1) {
        mn = fminf(mn, __shfl_xor(mn, s));
        mx = fmaxf(mx, __shfl_xor(mx, s));
        nan = fmaxf(nan, __shfl_xor(nan, s));
    }
    if (nan != 0.f) mn = mx = __builtin_nanf("");
    // every lane holds the same two values: as scalars, so that den, the division plans and the
    // constant test are wave-uniform
    mn = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, mn)));
    mx = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, mx)));
    const float den = mx - mn;
    const bool constant = den == 0.0f;
    uint32_t s[kMtGroups];
    int32_t gleft, gnext;
    rand_gen_init(gen, j, s, seed_scratch[wv], gleft, gnext, lane);
    const float* xr = x + j * d;
    float* outr = out + j * d;
    const int64_t N = constant ? 0 : d;
    if (constant)
        for (int64_t i = lane; i < d; i += 64) outr[i] = xr[i];
    // x and out through buffer descriptors (d * 4 <= 2^30 bytes): a lane outside its group's range
    // takes an out-of-range offset (loads 0, its store is dropped), so a block's ten groups are
    // straight-line code and their chains interleave -- one wave has nothing else to hide latency
    const __amdgpu_buffer_rsrc_t rx = make_rsrc(xr, (uint32_t)d * 4u), ro = make_rsrc(outr, (uint32_t)d * 4u);
    auto off = [](int64_t i0, int lo, int hi, int ln) {
        return ln >= lo && ln < hi ? (uint32_t)(i0 + ln) * 4u : 0xFFFFFFFFu;
    };
    auto load = [&](int64_t i0, int lo, int hi, int ln) {
        return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rx, off(i0, lo, hi, ln), 0, kAuxNT));
    };
    rand_walk(s, gleft, gnext, N, lane, load, [&](int64_t i0, int lo, int hi, uint32_t w, float xv, int ln) {
        float q = (xv - mn) / den;
        q = q != q ? q : fminf(fmaxf(q, 0.0f), 1.0f);           // clamp_ keeps NaN
        const float t = q * nl;
        const float fl = floorf(t);
        const float fr = t - fl;
        const float b = fl + (u24(w) < fr ? 1.0f : 0.0f);
        const float r = b / nl;
        const float m = r * den;
        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(m + mn), ro, off(i0, lo, hi, ln), 0, kAuxNT);
    });
    if (gen.px_state_out)
        qfl_state_out(gen.px_state_out + j * kQfStateWords, s, N, gleft, gnext, rand_vg(gleft, gnext), lane);
    if (lane == 0) info[j] = constant ? UQ_SCALAR_CONSTANT : 0;
}

// ---- DRIVE_quantize_Hadamard -------------------------------------------------------------
// Words one client takes: 2048 per whole chunk, the last chunk's length padded to a power of two
// (the padding draws too, AS:735).
__host__ __device__ inline int64_t drive_pow2ceil(int64_t L) {
    int64_t p = 1;
    while (p < L) p <<= 1;
    return p;
}
__host__ __device__ inline int64_t drive_words(int64_t d) {
    const int64_t rem = d % kDriveChunk;
    return d - rem + (rem ? drive_pow2ceil(rem) : 0);
}

// KR3: one wave per client walks its words; bit i of bits[j] = (u_i > 0.5), D = +1 where set
// (AS:735).  Chunk c's first word is word 2048 c, so its bits start at 64-bit word 32 c.  A
// group's ballot is appended to a 64-bit accumulator (the groups follow each other in index
// order) that is stored each time it fills: one 8-byte store per 64 words.
__global__ void __launch_bounds__(64 * kRwWavesPerWG)
drive_bits_kernel(int64_t n, int64_t words, RandGen gen, uint64_t* __restrict__ bits, int64_t row_words) {
    __shared__ uint32_t seed_scratch[kRwWavesPerWG][kMtN];
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // wave-uniform: j, the walk's bounds
    const int64_t j = (int64_t)blockIdx.x * kRwWavesPerWG + wv;
    if (j >= n) return;                                         // whole wave: no barrier below
    uint32_t s[kMtGroups];
    int32_t gleft, gnext;
    rand_gen_init(gen, j, s, seed_scratch[wv], gleft, gnext, lane);
    uint64_t* row = bits + j * row_words;
    const __amdgpu_buffer_rsrc_t rrow = make_rsrc(row, (uint32_t)row_words * 8u);     // <= 2^25 bytes
    uint64_t acc = 0;
    int fill = 0;
    int64_t k = 0;
    auto none = [](int64_t, int, int, int) { return 0; };
    rand_walk(s, gleft, gnext, words, lane, none, [&](int64_t, int lo, int hi, uint32_t w, int, int ln) {
        // u24(w) > 0.5f on the integers (both sides are exact); selects, not branches: the
        // scalars below are wave-uniform and a taken scalar branch per group costs more
        const bool bit = ln >= lo && ln < hi && (w & 0xFFFFFFu) > 0x800000u;
        const uint64_t m = (uint64_t)__ballot(bit) >> lo;       // hi - lo bits, word order
        const int cnt = hi - lo;
        acc |= m << fill;
        const bool full = fill + cnt >= 64;
        const u32x2v av = {(uint32_t)acc, (uint32_t)(acc >> 32)};
        __builtin_amdgcn_raw_buffer_store_b64(av, rrow, full && ln == 0 ? (uint32_t)k * 8u : 0xFFFFFFFFu, 0, 0);
        const uint64_t carry = fill ? m >> ((64 - fill) & 63) : 0;
        acc = full ? carry : acc;
        k += full ? 1 : 0;
        fill = (fill + cnt) & 63;
    });
    if (fill && lane == 0) row[k] = acc;                        // k < row_words: fill bits are left of the words
    if (gen.px_state_out)
        qfl_state_out(gen.px_state_out + j * kQfStateWords, s, words, gleft, gnext, rand_vg(gleft, gnext), lane);
}

// The pair step of AS:37-59, `stages` times, on a thread's four pairs.
__device__ __forceinline__ void drive_pair_steps(float (&r)[8], int stages) {
    for (int st = 0; st < stages; ++st) {
#pragma unroll
        for (int q = 0; q < 8; q += 2) {
            const float sum = r[q] + r[q + 1];
            r[q + 1] = sum - r[q + 1];
            r[q] = sum;
        }
    }
}

// KR4: workgroup (c, j) = chunk c of client j, L coordinates padded with zeros to P (AS:722-732);
// thread t holds elements 8 t .. 8 t + 7 (threads at or beyond P / 8 only join the barriers).
//   Rx = pairstep^log2(P)(D * v)                                              AS:737-738
//   S = f32(nrm * nrm) / (sum|Rx| + 1e-12f)                                   AS:741
//       nrm: torch.norm of the L inputs (8 fma chains over L - L % 8, lanes in order, then the
//       tail: 4 by mul + add when 4 remain, the last 1 to 3 by fma; |x| for L = 1, fma for
//       L = 2), run by 8 lanes of wave 1 from LDS;
//       sum|Rx|: torch's CPU sum of P <= 2048 values (block_torch_sum)
//   out = pairstep^log2(P)(S * sign(Rx)) * D, the first L                      AS:743-750
__global__ void __launch_bounds__(kQBlock)
drive_chunk_kernel(const float* __restrict__ x, float* __restrict__ out, int64_t d, int64_t nchunks,
                   const uint64_t* __restrict__ bits, int64_t row_words, float* __restrict__ S_out) {
    __shared__ float sv[kDriveChunk];                 // the inputs (the norm's chains)
    __shared__ float sabs[kDriveChunk];               // |Rx|
    __shared__ float scr[64 * 32 + 64];               // block_torch_sum's scratch
    __shared__ float snrm;
    const int tid = threadIdx.x;
    const int64_t j = blockIdx.x / nchunks, c = blockIdx.x % nchunks;
    const int L = (int)std::min<int64_t>(kDriveChunk, d - c * kDriveChunk);
    const int P = (int)drive_pow2ceil(L);
    const int stages = 31 - __builtin_clz((unsigned)P);
    const float* xr = x + j * d + c * kDriveChunk;
    float* outr = out + j * d + c * kDriveChunk;
    const int e0 = 8 * tid;
    const uint8_t* brow = reinterpret_cast<const uint8_t*>(bits + j * row_words + c * (kDriveChunk / 64));
    const uint32_t db = e0 < P ? brow[tid] : 0u;      // bits 8 t .. 8 t + 7 of the chunk (little-endian words)
    float v[8], D[8], r[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        v[q] = e0 + q < L ? xr[e0 + q] : 0.0f;
        D[q] = ((db >> q) & 1u) ? 1.0f : -1.0f;
        r[q] = D[q] * v[q];
        sv[e0 + q] = v[q];
    }
    drive_pair_steps(r, stages);
#pragma unroll
    for (int q = 0; q < 8; ++q) sabs[e0 + q] = fabsf(r[q]);
    __syncthreads();
    if (tid >= kWave && tid < 2 * kWave) {            // wave 1: torch.norm(v[:L])
        const int l = tid & 7;
        const int steps = L / 8;
        float acc = 0.f;
        if (tid < kWave + 8) {
            int i = 0;
            for (; i + 8 <= steps; i += 8) {
                float t[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) t[u] = sv[8 * (i + u) + l];
#pragma unroll
                for (int u = 0; u < 8; ++u) acc = fmaf(t[u], t[u], acc);
            }
            for (; i < steps; ++i) acc = fmaf(sv[8 * i + l], sv[8 * i + l], acc);
        }
        float tot = __shfl(acc, 0, kWave);
        for (int u = 1; u < 8; ++u) tot = tot + __shfl(acc, u, kWave);
        if (tid == kWave) {
            if (L == 2) {
                tot = fmaf(sv[1], sv[1], fmaf(sv[0], sv[0], 0.0f));
            } else {                                  // L % 8 left: 4 by mul + add when 4 remain, the rest by fma
                int i = 8 * steps;
                if (L - i >= 4)
                    for (const int e = i + 4; i < e; ++i) {
                        const float p = sv[i] * sv[i];
                        tot = tot + p;
                    }
                for (; i < L; ++i) tot = fmaf(sv[i], sv[i], tot);
            }
            snrm = L == 1 ? fabsf(sv[0]) : sqrtf(tot);
        }
    }
    const float sum = block_torch_sum(sabs, (int64_t)P, scr, [](float a) { return a; });   // ends on a barrier
    const float nrm = snrm;
    const float S = (nrm * nrm) / (sum + 1e-12f);
#pragma unroll
    for (int q = 0; q < 8; ++q) r[q] = S * ((r[q] > 0.0f ? 1.0f : 0.0f) - (r[q] < 0.0f ? 1.0f : 0.0f));   // sign(+-0) = +0
    drive_pair_steps(r, stages);
#pragma unroll
    for (int q = 0; q < 8; ++q)
        if (e0 + q < L) outr[e0 + q] = r[q] * D[q];
    if (S_out && tid == 0) S_out[blockIdx.x] = S;
}

}  // namespace

#endif  // UQ_RAND_KERNELS_H
