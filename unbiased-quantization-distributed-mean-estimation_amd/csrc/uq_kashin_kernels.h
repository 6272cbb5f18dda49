// uq_kashin_kernels.h — Kashin_quantize (AS = NMSE_Results/Codes/All_Schemes.py:834-854 with
// 62-91 and 191-274): the kernels around the RHT passes, which uq_kashin.hip runs through
// uq_internal.h (rht_forward_rows, rht_inverse).  Included by uq_kashin.hip.
//
// Per client: the residual r [D] (x, zero beyond dim), the coefficients c [D], the bound M, a
// `done` flag and the number of forward transforms.  A client that is done keeps c, r and M:
// the transforms still run on its scratch rows, KK2-KK4 skip it.
//     KK0 kashin_pad_kernel      r = pad(x, D), c = 0                                   AS:217-223
//     KK1 kashin_norm_kernel     torch.norm of rows of any length (optionally of a - b): 8 fma
//                                chains, lanes in order, the general tail (KR4's), sqrt
//     KK1b kashin_start_kernel   M = norm / f32(sqrt(delta D)), done = 0, iters = niters  AS:220
//     KK2 kashin_clamp_kernel    b_hat = clamp(b, -M, M) in place, c = c + b_hat        AS:227-228
//     KK3 kashin_resid_kernel    r[:dim] -= t[:dim], M = M * f32(eta)                   AS:232-233
//     KK4 kashin_exit_kernel     err = num / den; err < f32(1e-6): done, iters = i + 1  AS:235-237
//     KR1 scalar_minmax_kernel   (uq_rand_kernels.h) min / max / has-NaN of slices of c
//     KK5 kashin_fold_kernel     mn, step = (mx - mn) / f32(nlevels - 1), info = 0        AS:73
//     KK6 kashin_sq_kernel       one wave per (client, run): rand_walk from the run's state;
//                                bins = floor(q) + (u < q - floor(q)), q = (c - mn) / step, as u8,
//                                or mn + bins * step at once                         AS:79-80, 91
//     KK7 kashin_deq_kernel      mn + bins * step of a u8 message                         AS:91
// Every step is one f32 operation (the unit is built without contraction, with IEEE division).

#ifndef UQ_KASHIN_KERNELS_H
#define UQ_KASHIN_KERNELS_H

#include "uq_rand_kernels.h"

namespace {

constexpr int kKnLoaders = 256;
constexpr int kKnThreads = kWave + kKnLoaders;
constexpr int kKnChunk = 2048;                     // floats per chunk and job of KK1 (8 per loader thread)
constexpr int kKnRow = kKnChunk / 8 + 4;           // one torch lane's 256 steps (+4 pad)
constexpr int kKeT = 256;                          // threads of the element-wise kernels
constexpr int kKeQ = 4;                            // ... each with 4 elements 256 apart

// KK0
__global__ void __launch_bounds__(kKeT)
kashin_pad_kernel(const float* __restrict__ x, float* __restrict__ r, float* __restrict__ c, int64_t dim, int64_t D) {
    const int64_t j = blockIdx.y;
#pragma unroll
    for (int q = 0; q < kKeQ; ++q) {
        const int64_t i = ((int64_t)blockIdx.x * kKeQ + q) * kKeT + threadIdx.x;
        if (i < D) {
            r[j * D + i] = i < dim ? x[j * dim + i] : 0.0f;
            c[j * D + i] = 0.0f;
        }
    }
}

// KK1: one workgroup per client, KE2's roles: wave 0 runs the chains and never touches global
// memory -- lane l = tid % 8 of job (tid / 8) % 2, four steps per ds_read_b128, so the two norms
// of the exit test cost one chain's time (lanes 16..63 mirror them); waves 1-4 stream each job's
// row in chunks of 2048 into a double-buffered LDS image laid out [lane l][step i] (element
// 8 i + l), their loads two chunks ahead of the chain.  A job with b: the norm of a - b, each
// difference one f32 subtraction.
struct KashinNormJob {
    const float* a;
    int64_t lda;
    const float* b;             // or null
    int64_t ldb;
    float* out;                 // [n]
};
struct KashinNormJobs {
    KashinNormJob job[2];
};
struct KashinNormSrc {
    const float *a, *b;
    __device__ __forceinline__ float operator()(int64_t i) const { return b ? a[i] - b[i] : a[i]; }
};

__global__ void __launch_bounds__(kKnThreads)
kashin_norm_kernel(KashinNormJobs jobs, int njobs, int64_t dim, const int32_t* __restrict__ done) {
    __shared__ __attribute__((aligned(16))) float s[2][2][8 * kKnRow];
    const int64_t j = blockIdx.x;
    if (done && done[j]) return;                                  // whole workgroup
    const int tid = threadIdx.x;
    KashinNormSrc src[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const KashinNormJob& jb = jobs.job[k < njobs ? k : 0];
        src[k] = KashinNormSrc{jb.a + j * jb.lda, jb.b ? jb.b + j * jb.ldb : nullptr};
    }
    const int64_t nv = dim - dim % 8;
    const int64_t nchunks = (nv + kKnChunk - 1) / kKnChunk;
    constexpr int kQ = kKnChunk / kKnLoaders;
    const bool chain = tid < kWave;
    const int lt = tid - kWave;                                   // loader thread
    // (a and b apart: the subtraction waits for both loads, so it belongs to the store, a chain later)
    float reg[2][kQ], regb[2][kQ];
    auto load = [&](int64_t ch) {
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            if (k >= njobs) break;                                // uniform
#pragma unroll
            for (int q = 0; q < kQ; ++q) {
                const int64_t i = ch * kKnChunk + lt + kKnLoaders * q;
                reg[k][q] = i < nv ? src[k].a[i] : 0.0f;
                regb[k][q] = i < nv && src[k].b ? src[k].b[i] : 0.0f;
            }
        }
    };
    auto store = [&](int buf) {
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            if (k >= njobs) break;
#pragma unroll
            for (int q = 0; q < kQ; ++q) {
                const int e = lt + kKnLoaders * q;
                s[buf][k][(e & 7) * kKnRow + (e >> 3)] = src[k].b ? reg[k][q] - regb[k][q] : reg[k][q];
            }
        }
    };
    if (nchunks > 0 && !chain) {
        load(0);
        store(0);
        if (nchunks > 1) load(1);
    }
    __syncthreads();
    const int ck = (tid >> 3) & 1;                                // the chain lane's job (job 1's rows hold nothing when njobs == 1)
    float acc = 0.0f;
    for (int64_t ch = 0; ch < nchunks; ++ch) {
        if (chain) {
            const int cnt = (int)(std::min<int64_t>(kKnChunk, nv - ch * kKnChunk) / 8);
            const float* row = s[ch & 1][ck < njobs ? ck : 0] + (tid & 7) * kKnRow;
            int i = 0;
            for (; i + 16 <= cnt; i += 16) {
                float4 t[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) t[u] = *reinterpret_cast<const float4*>(row + i + 4 * u);
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    acc = fmaf(t[u].x, t[u].x, acc);
                    acc = fmaf(t[u].y, t[u].y, acc);
                    acc = fmaf(t[u].z, t[u].z, acc);
                    acc = fmaf(t[u].w, t[u].w, acc);
                }
            }
            for (; i < cnt; ++i) acc = fmaf(row[i], row[i], acc);
        } else if (ch + 1 < nchunks) {
            store((int)((ch + 1) & 1));         // chunk ch + 1 (that buffer was read last in iteration ch - 1, before its barrier)
            if (ch + 2 < nchunks) load(ch + 2); // in flight across the next iteration's chain
        }
        __syncthreads();
    }
    if (chain) {
        const int base = tid & 8;
        float tot = __shfl(acc, base, kWave);
        for (int u = 1; u < 8; ++u) tot = tot + __shfl(acc, base + u, kWave);
        if ((tid == 0 || tid == 8) && ck < njobs) {
            // torch's tail: |x| for one element, fma for two; else 4 by mul + add when 4 remain, the
            // last 1 to 3 by fma (KR4, oracle/uq_oracle.c uqo_torch_norm2)
            const KashinNormSrc val = ck ? src[1] : src[0];
            float res;
            if (dim == 1) {
                res = fabsf(val(0));
            } else if (dim == 2) {
                const float v0 = val(0), v1 = val(1);
                res = sqrtf(fmaf(v1, v1, fmaf(v0, v0, 0.0f)));
            } else {
                int64_t i = nv;
                if (dim - i >= 4)
                    for (const int64_t e = i + 4; i < e; ++i) {
                        const float v = val(i);
                        const float p = v * v;
                        tot = tot + p;
                    }
                for (; i < dim; ++i) {
                    const float v = val(i);
                    tot = fmaf(v, v, tot);
                }
                res = sqrtf(tot);
            }
            (ck ? jobs.job[1] : jobs.job[0]).out[j] = res;
        }
    }
}

// KK1b: torch.norm(x) / np.sqrt(delta * D): a 0-dim f32 tensor by a Python double, which torch
// divides as f32 / f32(sd)
__global__ void __launch_bounds__(kKeT)
kashin_start_kernel(const float* __restrict__ nrm, float sd, int32_t niters, int64_t n, float* __restrict__ M,
                    int32_t* __restrict__ done, int32_t* __restrict__ iters) {
    const int64_t j = (int64_t)blockIdx.x * kKeT + threadIdx.x;
    if (j >= n) return;
    M[j] = nrm[j] / sd;
    done[j] = 0;
    iters[j] = niters;
}

// KK2: torch.clamp propagates NaN (of b or of the bound); c starts as zeros and its first += is
// a real addition (-0.0 becomes +0.0)
__global__ void __launch_bounds__(kKeT)
kashin_clamp_kernel(float* __restrict__ b, float* __restrict__ c, const float* __restrict__ M,
                    const int32_t* __restrict__ done, int64_t D) {
    const int64_t j = blockIdx.y;
    if (done[j]) return;
    const float m = M[j];
#pragma unroll
    for (int q = 0; q < kKeQ; ++q) {
        const int64_t i = ((int64_t)blockIdx.x * kKeQ + q) * kKeT + threadIdx.x;
        if (i < D) {
            const float v = b[j * D + i];
            const float h = (v != v || m != m) ? v + m : fminf(fmaxf(v, -m), m);
            b[j * D + i] = h;
            c[j * D + i] = c[j * D + i] + h;
        }
    }
}

// KK3 (t: [n][dim], the inverse transform's output)
__global__ void __launch_bounds__(kKeT)
kashin_resid_kernel(float* __restrict__ r, const float* __restrict__ t, float* __restrict__ M,
                    const int32_t* __restrict__ done, float eta, int64_t D, int64_t dim) {
    const int64_t j = blockIdx.y;
    if (done[j]) return;
#pragma unroll
    for (int q = 0; q < kKeQ; ++q) {
        const int64_t i = ((int64_t)blockIdx.x * kKeQ + q) * kKeT + threadIdx.x;
        if (i < dim) r[j * D + i] = r[j * D + i] - t[j * dim + i];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) M[j] = M[j] * eta;      // (no other thread of this launch reads M)
}

// KK4: num = norm(x - (H(c) * diag)[:dim]), den = norm(r); the comparison in f32, NaN is no exit
__global__ void __launch_bounds__(kKeT)
kashin_exit_kernel(const float* __restrict__ num, const float* __restrict__ den, float err, int32_t it, int64_t n,
                   int32_t* __restrict__ done, int32_t* __restrict__ iters) {
    const int64_t j = (int64_t)blockIdx.x * kKeT + threadIdx.x;
    if (j >= n || done[j]) return;
    const float e = num[j] / den[j];
    if (e < err) {
        done[j] = 1;
        iters[j] = it;
    }
}

// KK5: KR1's partials folded; min / max are NaN when the row holds one (torch's)
__global__ void __launch_bounds__(kKeT)
kashin_fold_kernel(const float4* __restrict__ part, int32_t parts, float nlm1, int64_t n, float* __restrict__ mn_out,
                   float* __restrict__ step_out, int32_t* __restrict__ info) {
    const int64_t j = (int64_t)blockIdx.x * kKeT + threadIdx.x;
    if (j >= n) return;
    float mn = INFINITY, mx = -INFINITY, nan = 0.f;
    for (int p = 0; p < parts; ++p) {
        const float4 t = part[j * parts + p];
        mn = fminf(mn, t.x);
        mx = fmaxf(mx, t.y);
        nan = fmaxf(nan, t.z);
    }
    if (nan != 0.f) mn = mx = __builtin_nanf("");
    mn_out[j] = mn;
    step_out[j] = (mx - mn) / nlm1;
    info[j] = 0;
}

// KK6: wave (j, r) = run r of client j: coordinates r * run_words .. + N take words 0 .. N - 1 of the
// stream that starts at the run's state (left, next, 624 words), coordinate k word k of the
// client's generator.  The draw is QUIC-FL's bernoulli(p): f32(w & 0xFFFFFF) * 2^-24 < p.  A p
// that is NaN or outside [0, 1] flags UQ_KASHIN_BAD_P (torch.bernoulli raises); DEQ = false also
// flags bins outside 0..255 (UQ_KASHIN_BIN_RANGE; stored saturated).  c and the output through
// buffer descriptors as in KR2.
template <bool DEQ>
__global__ void __launch_bounds__(64 * kRwWavesPerWG)
kashin_sq_kernel(const float* __restrict__ c, int64_t D, const float* __restrict__ mn, const float* __restrict__ step,
                 const uint32_t* __restrict__ runs, const int32_t* __restrict__ run_row, int64_t R, int64_t run_words,
                 int64_t n, void* __restrict__ outp, int32_t* __restrict__ info) {
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t w = (int64_t)blockIdx.x * kRwWavesPerWG + wv;
    if (w >= n * R) return;                                       // whole wave
    const int64_t j = w / R, r = w % R;
    const int64_t row = run_row ? (int64_t)run_row[j] : j;
    const uint32_t* st = runs + (row * R + r) * kQfStateWords;
    const int32_t gleft = __builtin_amdgcn_readfirstlane((int32_t)st[0]);
    const int32_t gnext = __builtin_amdgcn_readfirstlane((int32_t)st[1]);
    uint32_t s[kMtGroups];
    mt_load(s, st + 2, lane);
    const int64_t base = r * run_words;
    const int64_t N = std::min<int64_t>(run_words, D - base);
    const float m = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, mn[j])));
    const float sp = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, step[j])));
    const __amdgpu_buffer_rsrc_t rc = make_rsrc(c + j * D + base, (uint32_t)N * 4u);
    const __amdgpu_buffer_rsrc_t ro = DEQ ? make_rsrc((float*)outp + j * D + base, (uint32_t)N * 4u)
                                          : make_rsrc((uint8_t*)outp + j * D + base, (uint32_t)N);
    auto inside = [](int lo, int hi, int ln) { return ln >= lo && ln < hi; };
    auto load = [&](int64_t i0, int lo, int hi, int ln) {
        const uint32_t off = inside(lo, hi, ln) ? (uint32_t)(i0 + ln) * 4u : 0xFFFFFFFFu;
        return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rc, off, 0, kAuxNT));
    };
    bool bad = false, over = false;
    rand_walk(s, gleft, gnext, N, lane, load, [&](int64_t i0, int lo, int hi, uint32_t wd, float cv, int ln) {
        const bool in = inside(lo, hi, ln);
        const float q = (cv - m) / sp;
        const float fl = floorf(q);
        const float p = q - fl;
        bad |= in && !(p >= 0.0f && p <= 1.0f);
        const float bn = fl + (u24(wd) < p ? 1.0f : 0.0f);
        if (DEQ) {
            const float v = bn * sp;
            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(m + v), ro, in ? (uint32_t)(i0 + ln) * 4u : 0xFFFFFFFFu,
                                                  0, kAuxNT);
        } else {
            over |= in && !(bn >= 0.0f && bn <= 255.0f);
            const float sat = fminf(fmaxf(bn, 0.0f), 255.0f);     // (NaN -> 0)
            __builtin_amdgcn_raw_buffer_store_b8((uint8_t)(int)sat, ro, in ? (uint32_t)(i0 + ln) : 0xFFFFFFFFu, 0, 0);
        }
    });
    const int flags = (__any(bad) ? UQ_KASHIN_BAD_P : 0) | (__any(over) ? UQ_KASHIN_BIN_RANGE : 0);
    if (flags && lane == 0) atomicOr(info + j, flags);
}

// KK7: the receiver's min + bins * step (a multiplication, then an addition) of a u8 message
__global__ void __launch_bounds__(kKeT)
kashin_deq_kernel(const uint8_t* __restrict__ bins, const float* __restrict__ mn, const float* __restrict__ step,
                  float* __restrict__ out, int64_t D) {
    const int64_t j = blockIdx.y;
    const float m = mn[j], sp = step[j];
#pragma unroll
    for (int q = 0; q < kKeQ; ++q) {
        const int64_t i = ((int64_t)blockIdx.x * kKeQ + q) * kKeT + threadIdx.x;
        if (i < D) {
            const float v = (float)bins[j * D + i] * sp;
            out[j * D + i] = m + v;
        }
    }
}

}  // namespace

#endif  // UQ_KASHIN_KERNELS_H
