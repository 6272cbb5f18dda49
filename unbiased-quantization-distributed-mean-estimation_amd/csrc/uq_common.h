// uq_common.h — device and host code that more than one scheme of the library uses:
//   the constants, the L1 plan (L1Plan / make_plan), the Markstein divisions (DivPlan, div*),
//   the K1 cascade (torch CPU `sum` order: l1_partial_kernel, l1_finalize_kernel,
//   launch_cascade; the element Ops live with the scheme that owns them), the DPP wave scans,
//   the streaming loads / stores and buffer descriptors, and block_torch_sum.
// Everything is in an anonymous namespace on purpose: each translation unit gets its own copy
// of what it uses (there is no device linking), nothing here has state, and the kernels'
// symbols carry these types' names.  A kernel template is instantiated by the one translation
// unit that launches it (the cascade with AbsOp: uq_unbiased.hip, with the Rez ops: uq_biased.hip).
#ifndef UQ_COMMON_H
#define UQ_COMMON_H

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>

#include "uq_internal.h"

namespace {

constexpr int kWave = 64;
constexpr int kGrain = 32768;     // at::internal::GRAIN_SIZE (torch CPU intra-op split)
constexpr int kMaxThreads = 4096; // torch_threads supported by the L1 plan (per-thread buffer in LDS)
constexpr int kQBlock = 256;      // threads per workgroup (4 waves) of the quantize tiles and block_torch_sum
// Every workspace starts with 256 control bytes.  Only u32 word 2 is in use: the sticky
// status uq_check_status reads and clears (2: a torch tie replay found itself inconsistent;
// 1: reserved for an inter-workgroup timeout, which no kernel reports any more).  A new
// workspace must be zero-filled once before first use.
constexpr size_t kCtrlBytes = 256;

// torch CPU `sum` of a contiguous f32 vector with T intra-op threads (ATen
// TensorIteratorBase::parallel_reduce -> two_pass_reduction, SumKernel cascade_sum):
//   d < GRAIN or T == 1: one cascade over the whole vector.
//   else: nt = min(T, ceil(d/GRAIN)) chunks of cs = ceil(d/nt) (ATen invoke_parallel); thread
//   t < nt sums chunk t into buffer[t] (buffer of T zeros), and the result is the SAME cascade
//   sum over the T-element buffer -- not a sequential add of the chunk sums (verified against
//   torch 2.10 for T = 1..39, 47, 63..65, 96, 128, 200, 256 at five sizes; T in {1,2,3,4,8}
//   happen to coincide with sequential order).
// Chunks are uniform except the last, so two geometries describe them all.
struct ChunkGeo {
    int64_t size;                    // chunk length
    int32_t lp;                      // log2(step) of its cascade
    int32_t ng1;                     // full level-1 groups in the chunk
};
struct L1Plan {
    int32_t nchunks;                 // nt
    int32_t nbuf;                    // T (length of the per-thread buffer), 1 in the one-chunk case
    int32_t total_groups;            // level-1 groups per vector, all chunks
    int64_t cs;                      // chunk stride (size of every chunk but the last)
    ChunkGeo full, last;             // chunks 0 .. nt-2, chunk nt-1
    __host__ __device__ int64_t off(int c) const { return (int64_t)c * cs; }
    __host__ __device__ const ChunkGeo& geo(int c) const { return c + 1 < nchunks ? full : last; }
    __host__ __device__ int32_t gbase(int c) const { return c * full.ng1; }
    __host__ __device__ int chunk_of_group(int32_t G) const {
        const int32_t nfull = (nchunks - 1) * full.ng1;
        return G < nfull ? G / full.ng1 : nchunks - 1;
    }
};

__host__ __device__ inline int ceil_log2_i64(int64_t x) {
    if (x <= 1) return 0;
    int r = 0;
    uint64_t v = (uint64_t)(x - 1);
    while (v) { ++r; v >>= 1; }
    return r;
}
__device__ inline int ceil_log2_dev(int64_t x) { return ceil_log2_i64(x); }

inline bool chunk_geo(int64_t s, ChunkGeo* g) {
    const int64_t rows = (s / 8) / 4;   // rows of 32 floats (8 lanes x 4 ILP)
    int lp = ceil_log2_i64(rows) / 4;
    if (lp < 4) lp = 4;
    if (lp > 8) return false;
    const int64_t step = (int64_t)1 << lp;
    const int64_t ng1 = (rows / step) / step;
    if (ng1 > (int64_t)1 << 28) return false;
    g->size = s;
    g->lp = lp;
    g->ng1 = (int32_t)ng1;
    return true;
}

inline bool make_plan(int64_t d, int32_t T, L1Plan* p) {
    std::memset(p, 0, sizeof(*p));
    if (T < 1) T = 1;
    if (T > kMaxThreads) return false;
    int64_t nt = 1, cs = d;
    if (!(d < kGrain || T == 1)) {
        nt = (d + kGrain - 1) / kGrain;
        if (nt > T) nt = T;
        cs = (d + nt - 1) / nt;
        nt = (d + cs - 1) / cs;        // chunks past d are empty (their buffer slots stay 0)
        p->nbuf = T;
    } else {
        p->nbuf = 1;
    }
    p->nchunks = (int32_t)nt;
    p->cs = cs;
    if (!chunk_geo(nt > 1 ? cs : d, &p->full)) return false;
    if (!chunk_geo(d - (nt - 1) * cs, &p->last)) return false;
    const int64_t g = (nt - 1) * (int64_t)p->full.ng1 + p->last.ng1;
    if (g > (int64_t)1 << 30) return false;
    p->total_groups = (int32_t)g;
    return true;
}

// v = x / den (AS:625) without the IEEE division sequence (~10 VALU per element).  den is
// one per client, so y = RN(1/den) is computed once (IEEE) and each quotient takes a
// product and two residual corrections (Markstein):
//     q0 = RN(x*y);  q1 = RN(q0 + RN(x - den*q0)*y)    (faithful)
//                    q2 = RN(q1 + RN(x - den*q1)*y)    (= RN(x/den): y correctly rounded,
//                                                       q1 faithful, no underflow)
// as packed fma pairs.  No underflow: den = L1 + 1e-12 >= 2^-39.9 always and den < 2^40 is
// required per client (else the IEEE division is used throughout), and elements with
// |q2| < 2^-59/den (covers every 0 < |x| < 2^-60) or q2 NaN (x = inf/NaN, overflow) are
// recomputed with the IEEE division.  x = +-0 gives q = +-0 in either sign, which is
// immaterial (only v < 0 and |v| are used).  tools/markstein_check.c checks this exact
// function against IEEE division over every finite f32 x for divisors across the range.
struct DivPlan {
    float den, y, thr;
    bool fast;
};
__device__ __forceinline__ DivPlan div_plan(float L) {
    DivPlan p;
    p.den = L + 1e-12f;                  // AS:625 (f32 add)
    p.fast = p.den < 0x1p40f;            // false for NaN / inf
    p.y = 1.0f / p.den;
    p.thr = 0x1p-59f / p.den;
    return p;
}
// z / nrm of EDEN's bins (AS:329): the Markstein sequence for a divisor in [2^-39, 2^40)
// (tools/markstein_check.c checks every f32 numerator for divisors over that range)
__device__ __forceinline__ DivPlan div_plan_norm(float nv) {
    DivPlan p;
    p.den = nv;
    p.fast = nv >= 0x1p-39f && nv < 0x1p40f;
    p.y = 1.0f / nv;
    p.thr = 0x1p-59f / nv;
    return p;
}
typedef float f32x2 __attribute__((ext_vector_type(2)));
// PZ: no quotient is -0 (a recomputed one has + 0.0f added, which changes nothing else).  The
// Markstein steps themselves never give -0: a quotient that is not recomputed has
// |q2| >= thr > 0, or x = +-0, and then q2 = +0 (x = -0: q0 = -0, r = fma(-den, -0, -0) = +0,
// q1 = fma(+0, y, -0) = +0, r = fma(-den, +0, -0) = -0, q2 = fma(-0, y, +0) = +0; x = +0: +0
// at every step).  tools/pass1_sign_check.c checks this over every f32 x.
template <bool PZ = false>
__device__ __forceinline__ void div4(const float (&xs)[4], const DivPlan& dp, float (&vs)[4]) {
    if (dp.fast) {
        const f32x2 Y = {dp.y, dp.y}, B = {-dp.den, -dp.den};
        // the two pairs step by step side by side: each step's two packed operations are
        // independent, so neither waits a cycle for the result of the one before it
        const f32x2 a0 = {xs[0], xs[1]}, a1 = {xs[2], xs[3]};
        f32x2 q0 = a0 * Y, q1 = a1 * Y;
        f32x2 r0 = __builtin_elementwise_fma(B, q0, a0), r1 = __builtin_elementwise_fma(B, q1, a1);
        q0 = __builtin_elementwise_fma(r0, Y, q0), q1 = __builtin_elementwise_fma(r1, Y, q1);
        r0 = __builtin_elementwise_fma(B, q0, a0), r1 = __builtin_elementwise_fma(B, q1, a1);
        q0 = __builtin_elementwise_fma(r0, Y, q0), q1 = __builtin_elementwise_fma(r1, Y, q1);
        vs[0] = q0.x, vs[1] = q0.y, vs[2] = q1.x, vs[3] = q1.y;
        // one test per four: the smallest |q| (q is finite here: den >= |x| and finite)
        const float mn = fminf(fminf(fabsf(vs[0]), fabsf(vs[1])), fminf(fabsf(vs[2]), fabsf(vs[3])));
        if (__builtin_expect(!(mn >= dp.thr), 0)) {
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (!(fabsf(vs[c]) >= dp.thr) && xs[c] != 0.0f) vs[c] = PZ ? xs[c] / dp.den + 0.0f : xs[c] / dp.den;
        }
    } else {
#pragma unroll
        for (int c = 0; c < 4; ++c) vs[c] = PZ ? xs[c] / dp.den + 0.0f : xs[c] / dp.den;
    }
}
// One quotient, the same operations as div4 (so the same bits).
__device__ __forceinline__ float div1(float x, const DivPlan& dp) {
    if (!dp.fast) return x / dp.den;
    float q = x * dp.y;
    float r = fmaf(-dp.den, q, x);
    q = fmaf(r, dp.y, q);
    r = fmaf(-dp.den, q, x);
    q = fmaf(r, dp.y, q);
    if (__builtin_expect(!(fabsf(q) >= dp.thr) && x != 0.0f, 0)) q = x / dp.den;
    return q;
}
// N quotients with div1's bits and no per-element branch: the Markstein steps on pairs
// (packed fma), one guard test over the lane's N elements and a wave-uniform branch into the
// IEEE division for the rare lane that needs it.  Elements whose bit is set in `skip` are
// left out of the guard (their quotient is discarded by the caller).
template <int N>
__device__ __forceinline__ void div_n(const float (&xs)[N], const DivPlan& dp, float (&vs)[N], uint32_t skip = 0u) {
    static_assert(N % 2 == 0, "pairs");
    if (dp.fast) {
        const f32x2 Y = {dp.y, dp.y}, B = {-dp.den, -dp.den};
#pragma unroll
        for (int h = 0; h < N / 2; ++h) {
            const f32x2 a = {xs[2 * h], xs[2 * h + 1]};
            f32x2 q = a * Y;
            f32x2 r = __builtin_elementwise_fma(B, q, a);
            q = __builtin_elementwise_fma(r, Y, q);
            r = __builtin_elementwise_fma(B, q, a);
            q = __builtin_elementwise_fma(r, Y, q);
            vs[2 * h] = q.x;
            vs[2 * h + 1] = q.y;
        }
        bool bad = false;
#pragma unroll
        for (int c = 0; c < N; ++c) bad |= !(fabsf(vs[c]) >= dp.thr) && xs[c] != 0.0f && !((skip >> c) & 1u);
        if (__builtin_expect(__ballot(bad) != 0ull, 0)) {
#pragma unroll
            for (int c = 0; c < N; ++c)
                if (!(fabsf(vs[c]) >= dp.thr) && xs[c] != 0.0f) vs[c] = xs[c] / dp.den;
        }
    } else {
#pragma unroll
        for (int c = 0; c < N; ++c) vs[c] = xs[c] / dp.den;
    }
}
// RN(k / m) for the dequantize step (m >= 1 is exact in f32 up to 2^24 and below 2^40
// always): the same Markstein sequence with den = m itself (no 1e-12 term).
__device__ __forceinline__ DivPlan div_plan_m(float fm) {
    DivPlan p;
    p.den = fm;
    p.fast = fm >= 1.0f && fm < 0x1p40f;
    p.y = 1.0f / fm;
    p.thr = 0x1p-59f / fm;
    return p;
}

// slots of the biased quantizer's per-client histograms (the cascade's histogram op counts into kFineSlot)
constexpr int kHistSlots = 4;                       // per biased client: key-digit passes 0-2, KB2's fine bins
constexpr int kFineSlot = 3;

// =====================================================================================
// K1a: level-1 block sums of op(x) in torch cascade order.
// One workgroup = one level-1 group = step leaves x step rows x 32 streams.
// Thread (leaf b, quad q) sums rows [b*step, (b+1)*step) of streams 4q..4q+3
// sequentially (ATen level 0); then 32 threads add the step leaves in order (level 1).
// BIG: cascade steps 64-256 (one chunk of more than 2^28 elements, e.g. T = 1 beyond
// d = 2^28): 256 threads, each taking leaves b, b + 32, ...; 32 KB of leaf sums.
// =====================================================================================
// gpw level-1 groups per workgroup, one after the other (the histogram op: its 2048-bin LDS
// histogram is flushed -- one global atomic per nonzero bin, ~1700 per 8192 coordinates of
// Gaussian rows -- once per gpw groups instead of once per group).
template <bool VEC4, class Op, bool BIG = false>
__global__ void __launch_bounds__(256)
l1_partial_kernel(const float* __restrict__ x, int64_t d, L1Plan plan, float* __restrict__ part,
                  const float* __restrict__ l1, float fm, uint32_t* __restrict__ hist_g, uint32_t* __restrict__ zn_g,
                  int gpw = 1) {
    const int64_t vec = blockIdx.y;
    Op op = Op::make(l1, fm, vec);
    __shared__ uint32_t hs[Op::kHist ? 2048 + 2 : 1];
    if (Op::kHist) {
        for (int b = threadIdx.x; b < 2048 + 2; b += blockDim.x) hs[b] = 0u;
        __syncthreads();
        op.h = hs;
        op.zn = hs + 2048;
    }
    __shared__ float leaf[(BIG ? 256 : 32) * 32];   // [leaf][32]
    const int32_t G0 = (int32_t)blockIdx.x * gpw;
    const int32_t G1 = min((int32_t)plan.total_groups, G0 + gpw);
    for (int32_t G = G0; G < G1; ++G) {
    if (G > G0) __syncthreads();              // the previous group's leaf sums are read
    const int c = plan.chunk_of_group(G);
    const int32_t g = G - plan.gbase(c);
    const int lp = plan.geo(c).lp;
    const int step = 1 << lp;
    const int tid = threadIdx.x;
    const int nthreads = 8 * step;            // 8 quads x step leaves
    const float* base = x + vec * d + plan.off(c) + (int64_t)g * step * step * 32;
    for (int b = tid >> 3; BIG ? b < step : tid < nthreads; b += 32) {
        const int q = tid & 7;
        const float* p = base + ((int64_t)b * step) * 32 + 4 * q;
        float a[4] = {0.f, 0.f, 0.f, 0.f};
        for (int r = 0; r < step; ++r) {
            float v[4];
            if (VEC4) {
                typedef float k1x4 __attribute__((ext_vector_type(4)));
                const k1x4 tv = __builtin_nontemporal_load(reinterpret_cast<const k1x4*>(p + (int64_t)r * 32));
                v[0] = tv.x; v[1] = tv.y; v[2] = tv.z; v[3] = tv.w;
            } else {
                const float* pr = p + (int64_t)r * 32;
                v[0] = pr[0]; v[1] = pr[1]; v[2] = pr[2]; v[3] = pr[3];
            }
            op.apply4(v, a);                  // a[c] += op(v[c]), streams 4q..4q+3 in row order
        }
        float* l = leaf + b * 32 + 4 * q;
        l[0] = a[0]; l[1] = a[1]; l[2] = a[2]; l[3] = a[3];
        if (!BIG) break;
    }
    __syncthreads();
    if (tid < 32) {
        float acc = 0.f;
        for (int b = 0; b < step; ++b) acc += leaf[b * 32 + tid];
        part[(vec * plan.total_groups + G) * 32 + tid] = acc;
    }
    }
    if (Op::kHist) {
        const int tid = threadIdx.x;
        __syncthreads();                      // every group's LDS counts are in
        for (int b = tid; b < 2048; b += blockDim.x)
            if (hs[b]) atomicAdd(&hist_g[((size_t)vec * kHistSlots + kFineSlot) * 2048 + b], hs[b]);
        if (tid < 2 && hs[2048 + tid]) atomicAdd(&zn_g[vec * 2 + tid], hs[2048 + tid]);
    }
}

// Sequential sum of `nrows` rows of stream `a` starting at element `start`.
// Loads go out 16 at a time ahead of the (ordered) adds: one memory round trip per 16 rows.
template <class Op>
__device__ float seq_rows(const Op& op, const float* __restrict__ xv, int64_t start, int64_t nrows, int a) {
    float acc = 0.f;
    int64_t r = 0;
    for (; r + 16 <= nrows; r += 16) {
        float t[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) t[u] = xv[start + (r + u) * 32 + a];
#pragma unroll
        for (int u = 0; u < 16; ++u) acc += op(t[u]);
    }
    for (; r < nrows; ++r) acc += op(xv[start + r * 32 + a]);
    return acc;
}

// =====================================================================================
// K1b: finish the cascade for each client (one wave per client).
// Lanes 0..31 own the 32 streams (8 lanes x 4 ILP): level-2/3 accumulation over the
// level-1 block sums, the open level-1 group and the tail rows (ATen multi_row_sum),
// then the ILP/lane/tail combination of ATen row_sum / vectorized_inner_sum, then the
// chunk results in chunk order (torch parallel_reduce).
// =====================================================================================
constexpr int kFinStage = 64;       // level-1 block sums staged in LDS per wave at a time (8 KB)
constexpr int kFinWaves = 8;        // chunks are finished by different waves, summed in order
// LDS written and read back by lanes of the same wave: a wave-level barrier suffices.
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// Column k of ATen multi_row_sum over R rows of width W (row stride W), f32 accumulate
// (the same level structure as the K1a/K1b cascade, walked by one lane).
__device__ float cascade_col(const float* a, int64_t R, int W, int k) {
    int lp = ceil_log2_dev(R) / 4;
    if (lp < 4) lp = 4;
    const int64_t step = (int64_t)1 << lp, mask = step - 1;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    int64_t i = 0;
    for (; i + step <= R;) {
        for (int64_t j = 0; j < step; ++j, ++i) a0 += a[i * W + k];
        a1 += a0; a0 = 0.f;
        if ((i & (mask << lp)) != 0) continue;
        a2 += a1; a1 = 0.f;
        if ((i & (mask << (2 * lp))) != 0) continue;
        a3 += a2; a2 = 0.f;
    }
    for (; i < R; ++i) a0 += a[i * W + k];
    return ((a0 + a1) + a2) + a3;
}
// torch cascade_sum of a[0..s) (ATen vectorized_inner_sum for s >= 8, scalar row_sum below),
// computed by the lanes of one wave; the result is valid in lane 0.  Used on the two-pass
// reduction's per-thread buffer (s = T <= kMaxThreads, so it is cheap).
[[maybe_unused]] __device__ float lds_torch_sum(const float* a, int s, int lane) {   // (only the cascade's users need it)
    if (s < 8) {
        float p[4] = {0.f, 0.f, 0.f, 0.f};
        if (s >= 4)
            for (int k = 0; k < 4; ++k) p[k] = 0.f + a[k];
        for (int k = (s >= 4 ? 4 : 0); k < s; ++k) p[0] += a[k];
        return ((p[0] + p[1]) + p[2]) + p[3];
    }
    const int vs = s / 8, nilp = vs / 4;
    const float col = (lane < 32 && nilp) ? cascade_col(a, nilp, 32, lane) : 0.f;
    float p[32];
#pragma unroll
    for (int j = 0; j < 32; ++j) p[j] = __shfl(col, j, kWave);
    float p0[8];
#pragma unroll
    for (int l = 0; l < 8; ++l) p0[l] = p[l];
    for (int v = nilp * 4; v < vs; ++v)
#pragma unroll
        for (int l = 0; l < 8; ++l) p0[l] += a[v * 8 + l];
#pragma unroll
    for (int k = 1; k < 4; ++k)
#pragma unroll
        for (int l = 0; l < 8; ++l) p0[l] += p[k * 8 + l];
    float acc = 0.f;
    for (int k = vs * 8; k < s; ++k) acc += a[k];
#pragma unroll
    for (int l = 0; l < 8; ++l) acc += p0[l];
    return acc;
}

// WAVES = 1 when there is one torch chunk (T = 1 or d < 32768): the eight waves' staging
// buffers (64 KB of LDS) held two workgroups per CU for one working wave (37 us at
// 1024 x 2^20, T = 1).
// WIDE (one chunk, a few clients: WAVES = 8, host choice): the level-2 group sums
// B_h = sum of `step` level-1 block sums in order are independent of each other, so all eight
// waves form them at once (step loads in flight per thread) and only acc3 = sum of B_h in order
// stays serial: one client's chain of ng1 dependent adds through eight LDS stages took 65 us at
// d = 2^22 (half of the n = 1 call, profiles/r6d_c4_unbiased_kernel_stats.csv).  Same adds in
// the same order.
template <class Op, int WAVES = kFinWaves, bool WIDE = false>
__global__ void __launch_bounds__(64 * WAVES)
l1_finalize_kernel(const float* __restrict__ x, int64_t d, L1Plan plan,
                   const float* __restrict__ part, float* __restrict__ l1_out,
                   const float* __restrict__ l1, float fm, uint32_t* __restrict__ hist_g,
                   uint32_t* __restrict__ zn_g) {
    const int64_t vec = blockIdx.x;
    Op op = Op::make(l1, fm, vec);
    // the elements outside full level-1 groups (open leaves, tail rows) count into an LDS
    // histogram, flushed once: one global atomic per element on the few hot first-digit bins
    // took 74 us per call at d = 172 554 (six torch chunks of 130 such rows)
    __shared__ uint32_t hs[Op::kHist ? 2048 + 2 : 1];
    if (Op::kHist) {
        for (int b = threadIdx.x; b < 2048 + 2; b += blockDim.x) hs[b] = 0u;
        __syncthreads();
        op.h = hs;
        op.zn = hs + 2048;
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const float* xv = x + vec * d;
    __shared__ float fin_w[WAVES][32];
    __shared__ __attribute__((aligned(16))) float s_stage_w[WAVES][kFinStage * 32];
    __shared__ float s_tail_w[WAVES][64];
    // the per-thread buffer of the two-pass reduction: plan.nbuf floats of dynamic LDS (a
    // static kMaxThreads buffer would halve the workgroups per CU for every T)
    extern __shared__ float s_chunk[];
    float* fin = fin_w[wv];
    float* s_stage = s_stage_w[wv];
    float* s_tail = s_tail_w[wv];
    for (int t = plan.nchunks + (int)threadIdx.x; t < plan.nbuf; t += 64 * WAVES) s_chunk[t] = 0.0f;
    float wide_acc3 = 0.f;                            // WIDE: acc3 of chunk 0, lanes < 32 of wave 0
    if (WIDE) {
        const ChunkGeo& geo = plan.geo(0);
        const int64_t step = (int64_t)1 << geo.lp;
        const int64_t ng2 = geo.ng1 / step;
        const float* pc = part + (vec * plan.total_groups + plan.gbase(0)) * 32;
        float* sB = &s_stage_w[0][0];                 // WAVES * kFinStage groups x 32 streams
        constexpr int kG = WAVES * kFinStage;
        for (int64_t h0 = 0; h0 < ng2; h0 += kG) {
            const int nh = (int)std::min<int64_t>(kG, ng2 - h0);
            for (int t = threadIdx.x; t < nh * 32; t += 64 * WAVES) {
                const float* src = pc + ((h0 + t / 32) * step) * 32 + (t & 31);
                float b = 0.f;
                for (int64_t j0 = 0; j0 < step; j0 += 16) {
                    float v[16];
#pragma unroll
                    for (int u = 0; u < 16; ++u) v[u] = src[(j0 + u) * 32];
#pragma unroll
                    for (int u = 0; u < 16; ++u) b += v[u];
                }
                sB[t] = b;
            }
            __syncthreads();
            if (wv == 0 && lane < 32)
                for (int h = 0; h < nh; ++h) wide_acc3 += sB[h * 32 + lane];
            __syncthreads();
        }
    }
    for (int c = wv; c < plan.nchunks; c += WAVES) {
        const int64_t off = plan.off(c);
        const ChunkGeo& geo = plan.geo(c);
        const int64_t s = geo.size;
        float chunk_sum;
        if (s < 8) {
            // ATen scalar row_sum (ILP 4, rows < step -> all rows land in acc0).  Lane 0
            // only: the op may count each element (RezKHistOp's histogram)
            float p[4] = {0.f, 0.f, 0.f, 0.f};
            if (lane == 0) {
                if (s >= 4)
                    for (int k = 0; k < 4; ++k) p[k] = 0.f + op(xv[off + k]);
                for (int64_t k = (s >= 4 ? 4 : 0); k < s; ++k) p[0] += op(xv[off + k]);
            }
            chunk_sum = ((p[0] + p[1]) + p[2]) + p[3];
        } else {
            const int64_t vs = s / 8, rows = vs / 4;
            const int lp = geo.lp;
            const int64_t step = (int64_t)1 << lp;
            const int64_t nleaf = rows / step;
            const int64_t ng1 = geo.ng1;
            const int64_t ng2 = ng1 / step;
            // level-2/3 over the ng1 block sums in order: groups [h*step, (h+1)*step) for
            // h < ng2 into b2 then acc3, the rest into acc2.  The block sums are staged
            // through LDS by the whole wave (coalesced, all loads in flight), so the
            // sequential adds read LDS instead of one dependent global load each.
            const float* pc = part + (vec * plan.total_groups + plan.gbase(c)) * 32;
            float acc3 = 0.f, acc2 = 0.f, b2 = 0.f;
            const int64_t n3 = ng2 * step;
            if (WIDE) {                               // B_h formed above; the rest after n3 in order
                acc3 = wide_acc3;
                if (lane < 32)
                    for (int64_t k = n3; k < ng1; ++k) acc2 += pc[k * 32 + lane];
            }
            for (int64_t k0 = WIDE ? ng1 : 0; k0 < ng1; k0 += kFinStage) {
                const int nk = (int)std::min<int64_t>(kFinStage, ng1 - k0);
                wave_sync();
                const float4* src = reinterpret_cast<const float4*>(pc + k0 * 32);
                float4* dst = reinterpret_cast<float4*>(s_stage);
                for (int i = lane; i < nk * 8; i += 64) dst[i] = src[i];
                wave_sync();
                if (lane < 32) {
                    for (int kk = 0; kk < nk; ++kk) {
                        const int64_t k = k0 + kk;
                        const float v = s_stage[kk * 32 + lane];
                        if (k < n3) {
                            b2 += v;
                            if (((k + 1) & (step - 1)) == 0) {         // step = 2^lp (no 64-bit modulo)
                                acc3 += b2;
                                b2 = 0.f;
                            }
                        } else {
                            acc2 += v;
                        }
                    }
                }
            }
            if (lane < 32) {
                float acc1 = 0.f;
                for (int64_t b = ng1 * step; b < nleaf; ++b)
                    acc1 += seq_rows(op, xv, off + b * step * 32, step, lane);
                float acc0 = seq_rows(op, xv, off + nleaf * step * 32, rows - nleaf * step, lane);
                fin[lane] = ((acc0 + acc1) + acc2) + acc3;
            }
            // the < 40 elements after the 32-stream rows, one load per lane, into LDS
            const int64_t t0 = rows * 32;
            const int nt = (int)(s - t0);
            if (lane < nt) s_tail[lane] = xv[off + t0 + lane];
            wave_sync();
            if (lane == 0) {
                float p0[8];
                for (int l = 0; l < 8; ++l) p0[l] = fin[l];
                for (int64_t v = rows * 4; v < vs; ++v)
                    for (int l = 0; l < 8; ++l) p0[l] += op(s_tail[v * 8 + l - t0]);
                for (int k = 1; k < 4; ++k)
                    for (int l = 0; l < 8; ++l) p0[l] += fin[k * 8 + l];
                float acc = 0.f;
                for (int64_t k = vs * 8; k < s; ++k) acc += op(s_tail[k - t0]);
                for (int l = 0; l < 8; ++l) acc += p0[l];
                fin[0] = acc;
            }
            wave_sync();
            chunk_sum = fin[0];
            wave_sync();
        }
        if (lane == 0) s_chunk[c] = 0.0f + chunk_sum;     // buffer[t] = 0 + (thread t's chunk)
    }
    __syncthreads();
    if (Op::kHist) {
        for (int b = threadIdx.x; b < 2048; b += blockDim.x)
            if (hs[b]) atomicAdd(&hist_g[((size_t)vec * kHistSlots + kFineSlot) * 2048 + b], hs[b]);
        if (threadIdx.x < 2 && hs[2048 + threadIdx.x]) atomicAdd(&zn_g[vec * 2 + threadIdx.x], hs[2048 + threadIdx.x]);
    }
    // second pass of the two-pass reduction: out = 0 + cascade sum of the T-element buffer
    if (wv == 0) {
        const float total = lds_torch_sum(s_chunk, plan.nbuf, lane);
        if (lane == 0) l1_out[vec] = 0.0f + total;
    }
}

// KB2 (the k' sum with the fine-bin histogram): at most this many level-1 groups per
// workgroup, fewer while that would leave fewer than ~4096 workgroups (a few-client call keeps
// one group each).  1024 x 2^20: KB2 1.16 -> 0.97 ms at 4 (torch-tie batch 5.43 -> 5.21 ms,
// lowest-index 4.23 -> 3.97 ms on one box; 8: 5.21 / 3.96), profiles/r5n_biased_gpw.jsonl.
constexpr int kHistGroupsPerWG = 8;

// Launches K1a + K1b with Op; a histogram op (Op::kHist, KB2 of the biased quantizer) with
// kHistGroupsPerWG.
template <class Op>
int launch_cascade(const float* x, int64_t n, int64_t d, const L1Plan& plan, float* part, float* sum_out,
                   const float* l1, float fm, hipStream_t st, uint32_t* hist = nullptr, uint32_t* zn = nullptr) {
    if (plan.total_groups > 0) {
        bool vec4 = aligned16(x) && (d % 4 == 0 || n == 1);
        vec4 = vec4 && (plan.nchunks == 1 || plan.cs % 4 == 0);
        int maxstep = std::max(16, 1 << plan.last.lp);
        if (plan.nchunks > 1) maxstep = std::max(maxstep, 1 << plan.full.lp);
        const int gpw = Op::kHist ? (int)std::max<int64_t>(1, std::min<int64_t>(kHistGroupsPerWG,
                                                                                (int64_t)plan.total_groups * n / 4096))
                                  : 1;
        dim3 grid((unsigned)((plan.total_groups + gpw - 1) / gpw), (unsigned)n);
        if (maxstep > 32) {              // steps 64..256 (chunk_geo stops at 256)
            if (vec4)
                hipLaunchKernelGGL((l1_partial_kernel<true, Op, true>), grid, dim3(256), 0, st, x, d, plan, part, l1, fm,
                                   hist, zn, gpw);
            else
                hipLaunchKernelGGL((l1_partial_kernel<false, Op, true>), grid, dim3(256), 0, st, x, d, plan, part, l1, fm,
                                   hist, zn, gpw);
        } else {
            dim3 block(8 * maxstep);
            if (vec4)
                hipLaunchKernelGGL((l1_partial_kernel<true, Op>), grid, block, 0, st, x, d, plan, part, l1, fm, hist, zn,
                                   gpw);
            else
                hipLaunchKernelGGL((l1_partial_kernel<false, Op>), grid, block, 0, st, x, d, plan, part, l1, fm, hist, zn,
                                   gpw);
        }
        int rc = hip_check(hipGetLastError(), "l1_partial_kernel launch");
        if (rc) return rc;
    }
    if (plan.nchunks == 1 && n <= 128 && plan.last.size >= 8 && plan.last.ng1 >= 64) {
        hipLaunchKernelGGL((l1_finalize_kernel<Op, kFinWaves, true>), dim3((unsigned)n), dim3(64 * kFinWaves),
                           (size_t)plan.nbuf * sizeof(float), st, x, d, plan, part, sum_out, l1, fm, hist, zn);
        return hip_check(hipGetLastError(), "l1_finalize_kernel (wide) launch");
    }
    if (plan.nchunks == 1) {
        hipLaunchKernelGGL((l1_finalize_kernel<Op, 1>), dim3((unsigned)n), dim3(64), (size_t)plan.nbuf * sizeof(float), st,
                           x, d, plan, part, sum_out, l1, fm, hist, zn);
        return hip_check(hipGetLastError(), "l1_finalize_kernel launch");
    }
    hipLaunchKernelGGL(l1_finalize_kernel<Op>, dim3((unsigned)n), dim3(64 * kFinWaves), (size_t)plan.nbuf * sizeof(float), st,
                       x, d, plan, part, sum_out, l1, fm, hist, zn);
    return hip_check(hipGetLastError(), "l1_finalize_kernel launch");
}

// 64-bit DPP move (two 32-bit halves); lanes without a source (or outside ROWMASK) read 0.
template <int CTRL, int ROWMASK>
__device__ __forceinline__ double dpp_d(double v) {
    const uint64_t u = (uint64_t)__double_as_longlong(v);
    const uint32_t lo = __builtin_amdgcn_update_dpp(0u, (uint32_t)u, CTRL, ROWMASK, 0xF, true);
    const uint32_t hi = __builtin_amdgcn_update_dpp(0u, (uint32_t)(u >> 32), CTRL, ROWMASK, 0xF, true);
    return __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
}
// Inclusive wave scan by DPP (row_shr 1/2/4/8, then row_bcast 15/31): no LDS round trips.
// Only used on sums that are exact in any order (multiples of one G below 2^E).
__device__ __forceinline__ double wave_incl_scan(double v, int) {
    v = v + dpp_d<0x111, 0xF>(v);                  // row_shr:1
    v = v + dpp_d<0x112, 0xF>(v);                  // row_shr:2
    v = v + dpp_d<0x114, 0xF>(v);                  // row_shr:4
    v = v + dpp_d<0x118, 0xF>(v);                  // row_shr:8
    v = v + dpp_d<0x142, 0xA>(v);                  // row_bcast:15 -> rows 1, 3
    v = v + dpp_d<0x143, 0xC>(v);                  // row_bcast:31 -> rows 2, 3
    return v;
}
// value of the previous lane (0 in lane 0): wave_shr:1
__device__ __forceinline__ double wave_prev(double v) { return dpp_d<0x138, 0xF>(v); }

// x is read once and q written once per call: non-temporal loads/stores (measured ~4%
// faster on the C2 batch than default-policy accesses).
typedef float f32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 ld_stream(const float4* p) {
    const f32x4 v = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p));
    return make_float4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ void st_stream(float4* p, float4 v) {
    const f32x4 t = {v.x, v.y, v.z, v.w};
    __builtin_nontemporal_store(t, reinterpret_cast<f32x4*>(p));
}

// Buffer descriptors for the stream kernel (guide T8/T20): built from wave-uniform values
// only (readfirstlane on the inputs), 32-bit per-lane byte offsets, hardware range check
// (out-of-range loads return 0, out-of-range stores are dropped: ragged last tiles need no
// branches).  aux = 2: non-temporal (x and q are touched once per call).
typedef float f32x4v __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4v __attribute__((ext_vector_type(4)));
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void* base, uint32_t bytes) {
    const uint64_t b = (uint64_t)(uintptr_t)base;
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)b);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(b >> 32));
    void* p = (void*)(uintptr_t)(((uint64_t)hi << 32) | lo);
    return __builtin_amdgcn_make_buffer_rsrc(p, (short)0, (int)__builtin_amdgcn_readfirstlane(bytes), 0x00020000);
}
constexpr int kAuxNT = 2;
typedef uint32_t u32x2v __attribute__((ext_vector_type(2)));

// Orders one wave's LDS accesses across lanes: the compiler sees single-lane addresses only
// (s[i] and s[i + 1] never alias for ONE lane) and could otherwise move a read past another
// lane's write; the wave's LDS operations themselves execute in program order.
__device__ __forceinline__ void wave_lds_fence() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront", "local");
    __builtin_amdgcn_wave_barrier();
}

// torch CPU `f(x).sum()` of one vector shorter than GRAIN (one cascade, the same for every
// torch thread count; K1a + K1b's arithmetic with step 16) by one 256-thread workgroup, into
// every thread: f = abs for L1 (AS:624), k' for the biased quantizer's m' (AS:648-649).
// scr: >= 64 * 32 + 64 floats of LDS.
template <class F>
__device__ float block_torch_sum(const float* __restrict__ xv, int64_t s, float* scr, F f) {
    const int tid = threadIdx.x;
    float* leaf = scr;                               // [64 leaves][32 streams]
    float* col = scr + 64 * 32;                      // [32] stream results, then [0] the sum
    if (s < 8) {                                     // ATen scalar row_sum
        if (tid == 0) {
            float p[4] = {0.f, 0.f, 0.f, 0.f};
            if (s >= 4)
                for (int k = 0; k < 4; ++k) p[k] = 0.f + f(xv[k]);
            for (int64_t k = (s >= 4 ? 4 : 0); k < s; ++k) p[0] += f(xv[k]);
            col[0] = 0.0f + (((p[0] + p[1]) + p[2]) + p[3]);
        }
        __syncthreads();
        const float r = col[0];
        __syncthreads();
        return r;
    }
    const int64_t vs = s / 8, rows = vs / 4;         // rows of 32 floats (8 lanes x 4 ILP)
    const int nleaf = (int)(rows / 16);              // cascade step 16: rows < 1024
    for (int b = tid >> 3; b < nleaf; b += kQBlock / 8) {     // level 0: leaf b, streams 4q..4q+3
        const int q = tid & 7;
        const float* p = xv + (int64_t)b * 16 * 32 + 4 * q;
        float a[4] = {0.f, 0.f, 0.f, 0.f};
        for (int r = 0; r < 16; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) a[c] += f(p[r * 32 + c]);
#pragma unroll
        for (int c = 0; c < 4; ++c) leaf[b * 32 + 4 * q + c] = a[c];
    }
    __syncthreads();
    if (tid < 32) {                                  // levels 1-2 (a3 never fills below 4096 rows), open rows
        float a1 = 0.f, a2 = 0.f, a0 = 0.f;
        for (int b = 0; b < nleaf; ++b) {
            a1 += leaf[b * 32 + tid];
            if (((b + 1) & 15) == 0) {
                a2 += a1;
                a1 = 0.f;
            }
        }
        for (int64_t r = (int64_t)nleaf * 16; r < rows; ++r) a0 += f(xv[r * 32 + tid]);
        col[tid] = ((a0 + a1) + a2) + 0.f;
    }
    __syncthreads();
    if (tid == 0) {                                  // ILP vectors, leftover 8-vectors, tail (ATen order)
        float p0[8];
        for (int l = 0; l < 8; ++l) p0[l] = col[l];
        for (int64_t v = rows * 4; v < vs; ++v)
            for (int l = 0; l < 8; ++l) p0[l] += f(xv[v * 8 + l]);
        for (int k = 1; k < 4; ++k)
            for (int l = 0; l < 8; ++l) p0[l] += col[k * 8 + l];
        float acc = 0.f;
        for (int64_t k = vs * 8; k < s; ++k) acc += f(xv[k]);
        for (int l = 0; l < 8; ++l) acc += p0[l];
        col[0] = 0.0f + acc;                         // the two-pass reduction's 0 + chunk
    }
    __syncthreads();
    const float r = col[0];
    __syncthreads();
    return r;
}

}  // namespace

#endif  // UQ_COMMON_H
