// uq_unbiased_kernels.h — device code of the unbiased L1-ball type quantizer: the tile
// geometry, AbsOp (the K1 cascade's element op), the K2 kernels (quantize small / stream, tile
// sums, prefix, map, fold, out) and the K3 kernels (client mean, codes decode, codes mean,
// nibbles mean).  Included by uq_unbiased.hip, which launches them (its header lists the
// kernels and their forms), and by the measurement sources under tools/exp/.
//
// Reference (AS = NMSE_Results/Codes/All_Schemes.py, ND = NMSE_Results/Codes/Normal_dist.py):
//   AS:609-641  Type_unbiased_quantize
//   ND:137-138  est += Q(v, R) / n   (client mean)

#ifndef UQ_UNBIASED_KERNELS_H
#define UQ_UNBIASED_KERNELS_H

#include "uq_common.h"

namespace {

// ---- quantize tile geometry --------------------------------------------------------
constexpr int kQItems = 16;                // contiguous elements per thread
constexpr int kQTile = kQBlock * kQItems;  // 4096 elements per tile
// LDS tile image: 256 rows of 16 floats (thread t owns row t); float4 column c of row r
// lives at swz(r, c) (XOR swizzle, see there): bank-conflict-free without padding.
constexpr int64_t kStreamMinClients = 256; // >= this many clients: one workgroup per vector
constexpr int64_t kSegMinTiles = 1024;     // fewer clients but >= this many tiles: segmented stream

// Element transforms summed by the K1 cascade.  The cascade itself (order of f32 adds)
// is the torch CPU `sum` order whatever is summed.
struct AbsOp {            // AS:624  input_vector.abs().sum()
    static constexpr bool kHist = false;   // no radix-digit histogram (see RezKHistOp)
    float den, fm;
    uint32_t *h, *zn;
    __device__ static AbsOp make(const float*, float, int64_t) { return AbsOp{0.f, 0.f, nullptr, nullptr}; }
    __device__ float operator()(float v) const { return fabsf(v); }
    __device__ void apply4(const float (&v)[4], float (&a)[4]) const {
#pragma unroll
        for (int c = 0; c < 4; ++c) a[c] += fabsf(v[c]);
    }
};

// =====================================================================================
// K2: fused normalize / floor / fp64 scan / crossing / dequantize.
//
// Scan (AS:635): torch CPU cumsum of f32 accumulates SEQUENTIALLY in fp64 and rounds
// each prefix to f32.  K2 reproduces every fp64 prefix bit-for-bit, in parallel:
//
//   While the running sum S stays in one fp64 binade [2^E, 2^(E+1)) (spacing G =
//   2^(E-52)), the add S + f rounds to a multiple of G, and the result depends on S
//   only through S mod 2G (round-half-even looks at the parity of S/G).  So a thread
//   runs its 16 adds twice, from B0 = 2^E (parity 0) and B1 = 2^E + G (parity 1):
//   T_p = chain_p - B_p is its EXACT increment for a start of parity p.  All T are
//   multiples of G, so the block scan of T0 is exact in any order.  Threads with
//   T0 != T1 ("ties": an element with remainder exactly G/2) are resolved in order
//   from their exact start parity (the lowest mantissa bit of the start).  A tile is
//   "regular" when its exact start P >= 32 and P + total + 1 < 2^(E+1); otherwise
//   (tile 0, binade crossings: about log2(d) tiles per vector) each thread takes the
//   binade of its approximate start, threads near a binade edge add their 16 values
//   one by one, and one lane walks the threads in order.
//
// Forms: the stream kernel carries the exact P from tile to tile (one workgroup per
// client).  Batches of fewer clients fold per client: approximate tile sums ->
// approximate prefixes P' (binade of each tile) -> exact tile maps (T for a start of
// parity 0 / 1, ties resolved for both) -> exact serial fold (irregular tiles are
// recomputed from their exact start) -> outputs from the exact P.  Every form gives
// the sequential cumsum's bits, hence the same bits.
// =====================================================================================
// Chain bases of the binade holding s: b0 = 2^E, b1 = 2^E + G (odd: lowest mantissa bit
// set), top = 2^(E+1).  Below 32 (and for NaN / huge s) the E = 5 bases: such tiles and
// threads are never "regular", the bases then only serve approximate sums.
struct Binade {
    double b0, b1, top;
};
__device__ __forceinline__ Binade binade_of(double s) {
    const uint64_t e = (s >= 32.0 && s < 0x1p1000) ? ((uint64_t)__double_as_longlong(s) >> 52) : (uint64_t)(1023 + 5);
    Binade b;
    b.b0 = __longlong_as_double((long long)(e << 52));
    b.b1 = __longlong_as_double((long long)((e << 52) | 1ull));
    b.top = __longlong_as_double((long long)((e + 1) << 52));
    return b;
}
// A block-uniform double moved to scalar registers (keeps B and P out of VGPRs).
__device__ __forceinline__ double uniform_d(double v) {
    const uint64_t b = (uint64_t)__double_as_longlong(v);
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)b);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(b >> 32));
    return __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
}
// parity of s/G for s in its own binade: the lowest mantissa bit
__device__ __forceinline__ bool lowbit(double s) { return ((uint32_t)__double_as_longlong(s) & 1u) != 0u; }
// relative margin between an approximate prefix and a binade edge (covers the distance
// between the sequential fp64 sum and any approximation of it for d < 2^31)
constexpr double kEdge = 0x1p-20;

// f(r) = ((r >> 2) ^ (r >> 1)) & 3 makes the 16-lane ds_read_b128 groups (banks mod 64)
// AND the 8-lane ds_write_b128 groups (banks mod 32) conflict-free for row accesses,
// staging writes and store reads alike.
__device__ __forceinline__ int swz(int r, int c) { return r * 16 + 4 * (c ^ (((r >> 2) ^ (r >> 1)) & 3)); }
__device__ __forceinline__ int swz_elem(int i) { return swz(i >> 4, (i >> 2) & 3) + (i & 3); }
// The staging writes and the store reads walk the image by float4 index q = tid + j * kQBlock:
// row (q >> 2) = (tid >> 2) + 64 j, column tid & 3.  64 j leaves the low two bits of r >> 2 and
// of r >> 1 alone, hence f(r) too, so swz(q >> 2, q & 3) = swz_q0(tid) + j * kQBlock * 4: one
// address per thread, the rest are immediate offsets.
__device__ __forceinline__ int swz_q0(int tid) { return swz(tid >> 2, tid & 3); }
static_assert((kQBlock / 4) % 4 == 0, "swz_q0: a step of kQBlock float4s must keep f(row)");

// A copy of a per-thread index that the compiler cannot see through.  Inside the stream
// kernels' tile loop every LDS address, byte offset and lane mask derived from tid is loop
// invariant; hoisted, they outnumber the registers and come back from scratch once per tile
// (a scratch reload shares vmcnt with the tile's buffer stores and loads, so waiting for one
// waits for an HBM round trip).  Derived from an opaque copy taken inside the loop body they
// are recomputed where they are used instead: a few VALU ops per tile.
__device__ __forceinline__ int opaque(int v) {
    asm volatile("" : "+v"(v));
    return v;
}

struct TileRegs {
    float4 v[kQItems / 4];   // VEC4: float4 q = tid + j*256; scalar: element tid + 256*(4j+c)
};

template <bool VEC4>
__device__ __forceinline__ void load_tile(TileRegs& r, const float* __restrict__ x, int64_t d, int32_t tiles,
                                          uint32_t ticket, int tid) {
    const int64_t vec = ticket / (uint32_t)tiles;
    const int64_t t0 = (int64_t)(ticket % (uint32_t)tiles) * kQTile;
    const int64_t rem = d - t0;
    const float* xt = x + vec * d + t0;
    if (VEC4 && rem >= kQTile) {
#pragma unroll
        for (int j = 0; j < kQItems / 4; ++j) r.v[j] = ld_stream(reinterpret_cast<const float4*>(xt) + tid + j * kQBlock);
    } else if (VEC4) {
#pragma unroll
        for (int j = 0; j < kQItems / 4; ++j) {
            const int64_t e = (int64_t)(tid + j * kQBlock) * 4;
            if (e + 3 < rem) {
                r.v[j] = reinterpret_cast<const float4*>(xt)[tid + j * kQBlock];
            } else {                              // ragged end of the row: never read past d
                r.v[j].x = e < rem ? xt[e] : 0.f;
                r.v[j].y = e + 1 < rem ? xt[e + 1] : 0.f;
                r.v[j].z = e + 2 < rem ? xt[e + 2] : 0.f;
                r.v[j].w = 0.f;
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < kQItems / 4; ++j) {
            float t[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int64_t e = tid + (int64_t)kQBlock * (4 * j + c);
                t[c] = e < rem ? xt[e] : 0.0f;
            }
            r.v[j] = make_float4(t[0], t[1], t[2], t[3]);
        }
    }
}

template <bool VEC4>
__device__ __forceinline__ void stage_tile(const TileRegs& r, float* s_x, int tid) {
    if (VEC4) {
        float* s0 = s_x + swz_q0(tid);              // float4 index tid + j*kQBlock = row*4 + column
#pragma unroll
        for (int j = 0; j < kQItems / 4; ++j) *reinterpret_cast<float4*>(s0 + j * (kQBlock * 4)) = r.v[j];
    } else {
#pragma unroll
        for (int j = 0; j < kQItems / 4; ++j) {
            const float t[4] = {r.v[j].x, r.v[j].y, r.v[j].z, r.v[j].w};
#pragma unroll
            for (int c = 0; c < 4; ++c) s_x[swz_elem(tid + kQBlock * (4 * j + c))] = t[c];
        }
    }
}

__device__ __forceinline__ void load_tile_buf(TileRegs& r, __amdgpu_buffer_rsrc_t rx, uint32_t t0_bytes, int tid) {
#pragma unroll
    for (int j = 0; j < kQItems / 4; ++j) {
        const f32x4v v = __builtin_amdgcn_raw_buffer_load_b128(rx, t0_bytes + (uint32_t)(tid + j * kQBlock) * 16u, 0,
                                                               kAuxNT);
        r.v[j] = make_float4(v.x, v.y, v.z, v.w);
    }
}

__device__ __forceinline__ void store_tile_buf(const float* s_data, __amdgpu_buffer_rsrc_t ro, uint32_t t0_bytes,
                                               int tid) {
    const float* s0 = s_data + swz_q0(tid);
#pragma unroll
    for (int j = 0; j < kQTile / 4 / kQBlock; ++j) {
        const int q = tid + j * kQBlock;
        const float4 v = *reinterpret_cast<const float4*>(s0 + j * (kQBlock * 4));
        const f32x4v w = {v.x, v.y, v.z, v.w};
        __builtin_amdgcn_raw_buffer_store_b128(w, ro, t0_bytes + (uint32_t)q * 16u, 0, kAuxNT);
    }
}

// Per-tile compute shared by both K2 kernels.  The tile (kQTile elements, zero-padded)
// is staged in LDS as 256 rows of 16 (+4 pad) floats; thread `tid` owns row `tid`.
//   pass 1: x -> v = x/den, p = |v|, mp = fm*p, fl = floor(mp), fr = mp - fl
//           (fl overwrites x in LDS, fr stays in registers, sign(v) as 2-bit codes),
//           thread sums in fp64, then a fixed-tree block exclusive scan.
//   pass 2: from base = P_t + exclusive prefix: c_i = f32(s += fr_i), crossing test,
//           out = ((L1*sign(v)) * (fl + r)) / m  -> LDS (overwrites fl).
// Output table (AS:640).  out = ((L1 * sign(v)) * (fl + r)) / f32(m) with k = fl + r a
// small non-negative integer, so per client the workgroup tabulates
//     tab[k] = RN( RN(L1 * k) / f32(m) )          k = 0 .. kTab-1   (IEEE division)
// and every element with k < kTab reads its |out| from LDS; (-L1)*k = -RN(L1*k) and
// (-a)/m = -(a/m) under round-to-nearest, so the sign is applied afterwards with
// copysign.  k >= kTab (high rates, large coordinates) and NaN take the arithmetic path.
constexpr int kTab = 256;

__device__ __forceinline__ void build_table(float* s_tab, int tid, float L, float fm) {
    for (int k = tid; k < kTab; k += kQBlock) s_tab[k] = (L * (float)k) / fm;
}

// sign(v) is folded into fl: fl_s = v < 0 ? -fl : fl (fl >= 0, so -0.0 marks a negative
// coordinate whose floor is 0).  torch.sign(v) == 0 (v = +-0 or NaN) needs no code of
// its own: v = +-0 gives fr = 0, hence r = 0 and out = (L1*0)*0/m = +0 = tab[0]; v = NaN
// makes fl NaN and out NaN either way (AS:640).
struct TileState {
    double texcl;        // exclusive prefix of t0 over the tile's threads (exact in a regular tile)
    double total;        // sum of t0 over the tile (same value in every thread)
    double t0, t1;       // this thread's increment from a start of parity 0 / 1 in the binade
};

// mp = m*p of this thread's kQItems elements stays in registers between the passes, with
// sign(v) folded in (v < 0 -> -mp; -0.0 marks a negative coordinate whose floor is 0); fl
// and fr are re-derived from it (floor / subtract: the same f32 ops, so the same bits) --
// one register per element instead of two.
struct TileVals {
    float mps[kQItems];
};
__device__ __forceinline__ float fr_of(float mps) {
    const float mp = fabsf(mps);
    return mp - floorf(mp);                     // AS:631
}

// LDS of the tile scan and the exact resolution (besides the scratch slots, see
// resolve_exact)
struct ScanLds {
    double wave[kQBlock / kWave];        // wave sums of t0
    uint64_t tmask[kQBlock / kWave];     // tie threads (pass 1); events (irregular tiles)
    uint64_t kmask[kQBlock / kWave];     // constant parity transfer (pass 1)
    uint64_t vmask[kQBlock / kWave];     // its value, else the flip bit (pass 1)
    uint64_t cmask[kQBlock / kWave];     // clean threads (irregular tiles)
    double rsum[kQBlock / kWave];        // irregular tiles: sum of the run ending the wave
    uint32_t rhead[kQBlock / kWave];     // irregular tiles: that run starts inside the wave
    double misc[2];
    double aux[kQBlock];                 // t1 - t0 of tie threads (pass 1); run sums (irregular)
};

// pass 1.  TIES: run the parity-1 chain too and publish, before the barrier, the tie mask,
// each thread's parity transfer in B's binade and t1 - t0 of tie threads; otherwise
// t1 = t0 (approximate tile sums).
template <bool FULL, bool TIES>
__device__ __forceinline__ void tile_pass1(const float* s_x, TileVals& tv, ScanLds& sl, int tid, int len,
                                           const DivPlan& dp, float fm, const Binade& B, TileState& st) {
    const int lane = tid & (kWave - 1);
    const int wid = tid / kWave;
    const int i0 = tid * kQItems;
    double c0 = B.b0, c1 = B.b1;
#pragma unroll
    for (int k4 = 0; k4 < kQItems / 4; ++k4) {
        const float4 xv4 = *reinterpret_cast<const float4*>(&s_x[swz(tid, k4)]);
        const float xs[4] = {xv4.x, xv4.y, xv4.z, xv4.w};
        float vs[4];
        if (__builtin_expect(dp.fast, 1)) {
            div4<true>(xs, dp, vs);             // AS:625 x / den, correctly rounded; never -0
        } else {
            // the IEEE division (div4's other branch).  Only here can a quotient be NaN (L1 is
            // not finite); it goes on with its sign cleared, as |v| did
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float q = xs[c] / dp.den + 0.0f;
                vs[c] = q != q ? fabsf(q) : q;
            }
        }
        const f32x2 F = {fm, fm};
        const f32x2 pr[2] = {F * f32x2{vs[0], vs[1]}, F * f32x2{vs[2], vs[3]}};    // the quotients' own pairs
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            // mp = fm*|v| (AS:626, AS:629) with sign(v) folded in, as one product: rounding to
            // nearest is symmetric, so RN(fm*v) = -RN(fm*|v|) for v < 0.  v = -0 is not "v < 0"
            // (its mps was +0): the quotients come without it (div4<true>; + 0.0f turns -0 into
            // +0 and changes no other value, a NaN stays that NaN).  |.| below is a source
            // modifier.  tools/pass1_sign_check.c compares this with
            // v < 0 ? -(fm*|v|) : fm*|v| over every f32 v.
            const float mps0 = (c & 1) ? pr[c >> 1].y : pr[c >> 1].x;
            const float mp = fabsf(mps0);
            const float fl = floorf(mp);        // AS:630
            float fr = mp - fl;                 // AS:631
            float mps = mps0;
            if (!FULL && i0 + 4 * k4 + c >= len) fr = mps = 0.0f;
            tv.mps[4 * k4 + c] = mps;
            c0 += (double)fr;                   // AS:635, from a parity-0 start
            if (TIES) c1 += (double)fr;         // ... and from a parity-1 start
        }
    }
    st.t0 = c0 - B.b0;                          // exact (Sterbenz)
    st.t1 = TIES ? c1 - B.b1 : st.t0;
    const double incl_w = wave_incl_scan(st.t0, lane);
    const double wexcl = wave_prev(incl_w);
    if (lane == kWave - 1) sl.wave[wid] = incl_w;
    if (TIES) {
        // parity transfer (regular tiles): a start of parity 0 ends on parity e0 = par(t0),
        // one of parity 1 on e1 = 1 ^ par(t1); par(t) = lowest mantissa bit of t + 2^E
        const bool tie = st.t0 != st.t1;
        const bool e0 = lowbit(st.t0 + B.b0);
        const bool e1 = !lowbit(st.t1 + B.b0);
        const uint64_t tm = __ballot(tie);
        const uint64_t km = __ballot(e0 == e1);
        const uint64_t vm = __ballot(e0);
        if (lane == 0) {
            sl.tmask[wid] = tm;
            sl.kmask[wid] = km;
            sl.vmask[wid] = vm;
        }
        if (tie) sl.aux[tid] = st.t1 - st.t0;
    }
    __syncthreads();
    double wbase = 0.0, total = 0.0;
#pragma unroll
    for (int w = 0; w < kQBlock / kWave; ++w) {
        if (w < wid) wbase += sl.wave[w];
        total += sl.wave[w];
    }
    st.texcl = wbase + wexcl;
    st.total = uniform_d(total);
}

__device__ __forceinline__ double* slot_of(float* s_scr, int t) { return reinterpret_cast<double*>(s_scr + t * kQItems); }

// Cumulative tie correction of the last tie thread before `tid` (slot[3]), 0 if none.
__device__ __forceinline__ double tie_corr(float* s_scr, const ScanLds& sl, int tid) {
    tid = opaque(tid);
    const int lane = tid & (kWave - 1);
    int w = tid / kWave;
    uint64_t mk = sl.tmask[w] & ((1ull << lane) - 1ull);
    while (mk == 0ull && w > 0) mk = sl.tmask[--w];
    if (mk == 0ull) return 0.0;
    return slot_of(s_scr, w * kWave + 63 - __builtin_clzll(mk))[3];
}

__device__ __forceinline__ uint64_t uniform_u64(uint64_t v) {
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
    return ((uint64_t)hi << 32) | lo;
}
constexpr int kFastTies = 32;   // ties per regular tile resolved from the parity transfers

// Parity of the running sum at the start of each thread of a regular tile whose start
// has parity pP: the threads' parity transfers composed in order.  Each is a constant (a
// tie thread whose two chains end on the same parity) or an xor with a fixed bit, so a
// thread's start parity is the last constant before it xor the flips after that.  The
// masks and the four wave-start parities live in scalar registers (built once per tile).
struct ParityCtx {
    uint64_t km[kQBlock / kWave], vm[kQBlock / kWave];
    bool pw[kQBlock / kWave];
};
__device__ __forceinline__ void parity_ctx(const ScanLds& sl, bool pP, ParityCtx& c) {
    bool p = pP;
#pragma unroll
    for (int w = 0; w < kQBlock / kWave; ++w) {
        const uint64_t km = uniform_u64(sl.kmask[w]), vm = uniform_u64(sl.vmask[w]);
        c.km[w] = km;
        c.vm[w] = vm;
        c.pw[w] = p;
        if (km) {
            const int j = 63 - __builtin_clzll(km);
            p = (((vm >> j) & 1ull) != 0ull) != ((__builtin_popcountll(~km & vm & ~((2ull << j) - 1ull)) & 1) != 0);
        } else {
            p = p != ((__builtin_popcountll(vm) & 1) != 0);
        }
    }
}
// start parity of lane b of wave W (W a compile-time index after unrolling)
template <int W>
__device__ __forceinline__ bool parity_in(const ParityCtx& c, int b) {
    const uint64_t lim = (1ull << b) - 1ull;
    const uint64_t cc = c.km[W] & lim;
    const uint64_t x = ~c.km[W] & c.vm[W] & lim;
    if (cc) {
        const int j = 63 - __builtin_clzll(cc);
        return (((c.vm[W] >> j) & 1ull) != 0ull) != ((__builtin_popcountll(x & ~((2ull << j) - 1ull)) & 1) != 0);
    }
    return c.pw[W] != ((__builtin_popcountll(x) & 1) != 0);
}

// Sum of t1 - t0 over the tie threads of wave W whose start is odd: all of them (Dt) and
// those before thread `tid` (Db).
template <int W>
__device__ __forceinline__ void tie_sums(const ScanLds& sl, const ParityCtx& c, int tid, double& Db, double& Dt) {
    uint64_t mk = uniform_u64(sl.tmask[W]);
    while (mk) {
        const int b = __builtin_ctzll(mk);
        mk &= mk - 1ull;
        if (parity_in<W>(c, b)) {
            const double dd = sl.aux[W * kWave + b];
            Dt = Dt + dd;
            if (W * kWave + b < tid) Db = Db + dd;
        }
    }
}

// Irregular tile, up to the walk: each thread takes the binade of its approximate start
// Ps + texcl (Ps: the exact start, or P' when a map kernel records the tile), writes its
// scratch slot (t0, t1 of a clean thread, else its 16 fractions), the event / clean masks
// (tmask / cmask) and its inclusive run sum (aux).
// Events: threads whose increment is not a fixed multiple of their run's G -- not clean
// (added one by one from their exact start) or a clean tie (t0 != t1).  Between events,
// clean threads form runs inside one binade (consecutive clean threads cannot straddle an
// edge: each ends 1 below it); their t0 are multiples of that G and a run sums to less than
// 2^E, so a SEGMENTED scan of t0 (a run starts after each event) is exact in any order.
struct IrrThread {
    bool event;
    double v, x;         // own run value (0 for an event), inclusive run sum
};
__device__ void irregular_prep(double Ps, const TileState& st, const TileVals& tv, float* s_scr, ScanLds& sl, int tid,
                               IrrThread& it) {
    tid = opaque(tid);
    double* slot = slot_of(s_scr, tid);
    const int wid = tid / kWave;
    const int lane = tid & (kWave - 1);
    const double sa = Ps + st.texcl;
    const Binade bt = binade_of(sa);
    const bool clean = sa >= 32.0 && sa >= bt.b0 * (1.0 + kEdge) && (sa + st.t0) + 1.0 < bt.top;
    double t0c = 0.0, t1c = 0.0;
    if (clean) {
        double c0 = bt.b0, c1 = bt.b1;
#pragma unroll
        for (int k = 0; k < kQItems; ++k) {
            const double f = (double)fr_of(tv.mps[k]);
            c0 += f;
            c1 += f;
        }
        t0c = c0 - bt.b0;
        t1c = c1 - bt.b1;
        slot[0] = t0c;
        slot[1] = t1c;
    } else {
#pragma unroll
        for (int k4 = 0; k4 < kQItems / 4; ++k4)
            reinterpret_cast<float4*>(slot)[k4] = make_float4(fr_of(tv.mps[4 * k4]), fr_of(tv.mps[4 * k4 + 1]),
                                                              fr_of(tv.mps[4 * k4 + 2]), fr_of(tv.mps[4 * k4 + 3]));
    }
    const bool event = !clean || t0c != t1c;
    const double v = event ? 0.0 : t0c;
    it.event = event;
    it.v = v;
    const uint64_t em = __ballot(event);
    const uint64_t cm = __ballot(clean);
    bool f = tid == 0 || (lane > 0 && ((em >> (lane - 1)) & 1ull) != 0ull);   // run head, in-wave view
    double x = v;
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {                       // segmented inclusive scan, wave level
        const double xu = __shfl_up(x, o, kWave);
        const int fu = __shfl_up((int)f, o, kWave);
        if (lane >= o) {
            if (!f) x = xu + x;
            f = f || fu != 0;
        }
    }
    if (lane == kWave - 1) {
        sl.rsum[wid] = x;                                      // sum of the run that ends the wave
        sl.rhead[wid] = f ? 1u : 0u;                           // that run starts inside the wave
    }
    if (lane == 0) {
        sl.tmask[wid] = em;
        sl.cmask[wid] = cm;
    }
    __syncthreads();
    if (!f) {                                                  // the run comes from earlier waves
        for (int w = wid - 1; w >= 0; --w) {
            if ((sl.tmask[w] >> (kWave - 1)) & 1ull) break;    // wave w ends with an event
            x = sl.rsum[w] + x;
            if (sl.rhead[w]) break;
        }
    }
    sl.aux[tid] = x;                                           // inclusive run sum
    it.x = x;
    __syncthreads();
}

// Exact thread base (prefix before this thread's first element) and exact P_{t+1}, from
// the exact tile start P.  s_scr: the tile's LDS image after pass 1 (thread t's row =
// floats [16t, 16t+16) is its scratch slot).  Ends with a barrier whenever it used the
// scratch, so the caller may rewrite the image right after.
__device__ double resolve_exact(double P, const Binade& B, const TileState& st, const TileVals& tv, float* s_scr,
                                ScanLds& sl, int tid, double& pnext) {
    tid = opaque(tid);
    double* slot = slot_of(s_scr, tid);
    if (P >= 32.0 && (P + st.total) + 1.0 < B.top) {            // regular (uniform)
        int nt = 0;
#pragma unroll
        for (int w = 0; w < kQBlock / kWave; ++w) nt += __builtin_popcountll(uniform_u64(sl.tmask[w]));
        if (nt == 0) {
            pnext = P + st.total;                                // exact: multiples of G in the binade
            return P + st.texcl;
        }
        if (nt <= kFastTies) {
            // a tie thread adds t1 - t0 when its start is odd: no barrier, no walk
            ParityCtx pc;
            parity_ctx(sl, lowbit(P), pc);
            double Db = 0.0, Dt = 0.0;
            tie_sums<0>(sl, pc, tid, Db, Dt);
            tie_sums<1>(sl, pc, tid, Db, Dt);
            tie_sums<2>(sl, pc, tid, Db, Dt);
            tie_sums<3>(sl, pc, tid, Db, Dt);
            pnext = (P + st.total) + Dt;
            return (P + st.texcl) + Db;
        }
        if (st.t0 != st.t1) {
            slot[0] = st.texcl;
            slot[1] = st.t0;
            slot[2] = st.t1;
        }
        __syncthreads();
        if (tid == 0) {
            double D = 0.0;
            for (int w = 0; w < kQBlock / kWave; ++w) {
                uint64_t mk = sl.tmask[w];
                while (mk) {
                    double* q = slot_of(s_scr, w * kWave + __builtin_ctzll(mk));
                    mk &= mk - 1ull;
                    const double t0 = q[1], t1 = q[2];
                    const double Sk = (P + q[0]) + D;            // exact start of the tie thread
                    D = D + ((lowbit(Sk) ? t1 : t0) - t0);
                    q[3] = D;
                }
            }
            sl.misc[0] = D;
        }
        __syncthreads();
        const double corr = tie_corr(s_scr, sl, tid);
        const double D = sl.misc[0];
        __syncthreads();
        pnext = (P + st.total) + D;
        return (P + st.texcl) + corr;
    }
    // irregular tile: the events walked by one lane from the exact start
    IrrThread it;
    irregular_prep(P, st, tv, s_scr, sl, tid, it);
    const int lane = tid & (kWave - 1);
    const int wid = tid / kWave;
    if (tid == 0) {
        double S = P;                                          // exact value at the current run head
        for (int w = 0; w < kQBlock / kWave; ++w) {
            uint64_t mk = sl.tmask[w];
            while (mk) {
                const int b = __builtin_ctzll(mk);
                const int k = w * kWave + b;
                mk &= mk - 1ull;
                double* q = slot_of(s_scr, k);
                S = S + sl.aux[k];                             // exact start of event k (its own v is 0)
                sl.aux[k] = S;
                if ((sl.cmask[w] >> b) & 1ull) {
                    const double t0 = q[0], t1 = q[1];
                    S = S + (lowbit(S) ? t1 : t0);
                } else {
                    for (int k4 = 0; k4 < kQItems / 4; ++k4) {
                        const float4 f4 = reinterpret_cast<const float4*>(q)[k4];
                        S = (((S + (double)f4.x) + (double)f4.y) + (double)f4.z) + (double)f4.w;
                    }
                }
                q[6] = S;                                      // value at the head of the next run
            }
        }
        const bool last_event = (sl.tmask[kQBlock / kWave - 1] >> (kWave - 1)) & 1ull;
        sl.misc[0] = last_event ? S : S + sl.aux[kQBlock - 1];
    }
    __syncthreads();
    double base;
    if (it.event) {
        base = sl.aux[tid];
    } else {
        int w = wid;                                           // the last event before this thread
        uint64_t mk = sl.tmask[w] & ((1ull << lane) - 1ull);
        while (mk == 0ull && w > 0) mk = sl.tmask[--w];
        const double start = mk ? slot_of(s_scr, w * kWave + 63 - __builtin_clzll(mk))[6] : P;
        base = start + (it.x - it.v);                                // + exclusive run sum (exact)
    }
    pnext = sl.misc[0];
    __syncthreads();
    return base;
}

// Tile map from an APPROXIMATE start Pg (the per-client fold of the small-batch forms):
// if the exact start is certainly in Pg's binade and the tile stays in it, the tile's
// exact increment for a start of parity p is m[p] (ties resolved for both parities).
// Returns false for an irregular tile (resolved later from its exact start).
__device__ bool resolve_map(double Pg, const Binade& B, const TileState& st, float* s_scr, ScanLds& sl, int tid,
                            double& m0, double& m1) {
    if (!(Pg >= 32.0 && Pg >= B.b0 * (1.0 + kEdge) && (Pg + st.total) + 1.0 < B.top)) return false;   // uniform
    int nt = 0;
#pragma unroll
    for (int w = 0; w < kQBlock / kWave; ++w) nt += __builtin_popcountll(uniform_u64(sl.tmask[w]));
    if (nt == 0) {
        m0 = m1 = st.total;
        return true;
    }
    if (nt <= kFastTies) {
        ParityCtx p0, p1;
        parity_ctx(sl, false, p0);
        parity_ctx(sl, true, p1);
        double D0 = 0.0, D1 = 0.0, unused = 0.0;
        tie_sums<0>(sl, p0, 0, unused, D0);
        tie_sums<1>(sl, p0, 0, unused, D0);
        tie_sums<2>(sl, p0, 0, unused, D0);
        tie_sums<3>(sl, p0, 0, unused, D0);
        tie_sums<0>(sl, p1, 0, unused, D1);
        tie_sums<1>(sl, p1, 0, unused, D1);
        tie_sums<2>(sl, p1, 0, unused, D1);
        tie_sums<3>(sl, p1, 0, unused, D1);
        m0 = st.total + D0;
        m1 = st.total + D1;
        return true;
    }
    double* slot = slot_of(s_scr, tid);
    if (st.t0 != st.t1) {
        slot[0] = st.texcl;
        slot[1] = st.t0;
        slot[2] = st.t1;
    }
    __syncthreads();
    if (tid < 2) {
        // start parity p = tid: the parity at a tie thread is p xor parity((texcl + D)/G),
        // read off (texcl + D) + 2^E (exact: texcl + D < 2^E is a multiple of G)
        const bool p = tid != 0;
        double D = 0.0;
        for (int w = 0; w < kQBlock / kWave; ++w) {
            uint64_t mk = sl.tmask[w];
            while (mk) {
                const double* q = slot_of(s_scr, w * kWave + __builtin_ctzll(mk));
                mk &= mk - 1ull;
                const double t0 = q[1], t1 = q[2];
                const bool par = p != lowbit((q[0] + D) + B.b0);
                D = D + ((par ? t1 : t0) - t0);
            }
        }
        sl.misc[tid] = D;
    }
    __syncthreads();
    m0 = st.total + sl.misc[0];
    m1 = st.total + sl.misc[1];
    __syncthreads();
    return true;
}

// Wire code of one coordinate (type codes, see uq_dme.h): k = fl + r ->
// code = k for sign(v) >= 0 and ~k = -k-1 for sign(v) < 0 (keeps the reference's -0.0
// outputs).  kmax tracks the largest k; a client whose kmax > 127 is flagged as
// overflow (its codes are meaningless).  fl is finite whenever L1 is finite, and a
// non-finite L1 flags the client separately (publish_kmax).
__device__ __forceinline__ uint32_t code_of(float mps, float kf) {
    const int mask = (int)__float_as_uint(mps) >> 31;       // 0 or -1: sign(v) < 0
    return (uint32_t)(((int)kf ^ mask) & 0xFF);
}

// pass 2; WQ: outputs into the LDS image s_o, WC: this thread's 16 codes into cw (NIB: as
// 4-bit codes, element e of the thread in bits 4e..4e+3 of cw[0..1]).
//
// The count k = fl + r is kept as an integer: k = (int)fl + (c_i crossed), with the float
// kf = fl + r re-derived only where it can matter.  While kf < 2^24 both are the same number
// ((int) of an integral float and + 1 are exact), so the table index, the code and the
// running max are the same bits; a group of four with any k >= kTab, or a client whose L1 is
// not finite, recomputes its elements from the float kf exactly as before.  That covers every
// case in which the two could differ: fl >= 2^24 (the float sum rounds), fl >= 2^31 (the
// conversion saturates; as unsigned the count stays >= kTab even after + 1) and fl = NaN (only
// when L1 is not finite).  kmax is only ever compared with 127.
//
// The rare path is one rolled loop per group (the element picked by selects on the uniform
// loop counter): unrolled it was most of the loop's code.
__device__ __forceinline__ uint32_t sign_mask(float mps) { return (uint32_t)((int)__float_as_uint(mps) >> 31); }
// The difference as a value of its own: left to itself the compiler pairs two of a group's
// subtractions into one packed add and spends three moves on lining its operands up.
__device__ __forceinline__ float own_f32(float v) {
    asm("" : "+v"(v));
    return v;
}
template <typename T>
__device__ __forceinline__ T pick4(const T (&a)[4], int c) {
    return c == 0 ? a[0] : c == 1 ? a[1] : c == 2 ? a[2] : a[3];
}

template <bool WQ, bool WC, bool NIB = false>
__device__ __forceinline__ void tile_pass2(float* s_o, const TileVals& tv, const float* s_tab, int tid, double base,
                                           float L, float fm, float Xv, uint32_t (&cw)[4], uint32_t& kmax) {
    double s = base;                           // exact prefix before this thread's first element
    float fprev = floorf((float)s - Xv);       // floor(c_{i-1} - X) of this thread's first element
    // k = fl + r can only be NaN when L1 is not finite: such a client takes the arithmetic
    // path for every element; otherwise a running max of k bounds the table reads
    const bool arith = !(fabsf(L) <= 3.40282347e38f);
    constexpr uint32_t kLim = (uint32_t)kTab;
    constexpr int kBits = NIB ? 4 : 8;
    constexpr uint32_t kMask = (1u << kBits) - 1u;
#pragma unroll
    for (int k4 = 0; k4 < kQItems / 4; ++k4) {
        float o[4];
        uint32_t ks[4];
        uint32_t m4 = 0, w = 0;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float mps = tv.mps[4 * k4 + c];
            const float mp = fabsf(mps);
            const float fla = floorf(mp);                      // AS:630
            s += (double)(mp - fla);                           // AS:631, AS:635 fp64 running sum
            const float fcur = floorf((float)s - Xv);          // AS:636 floor(c_i - X)
            const uint32_t k = (uint32_t)(int)fla + (own_f32(fcur - fprev) == 1.0f ? 1u : 0u);   // AS:636-637, fl + r
            fprev = fcur;
            ks[c] = k;
            m4 = max(m4, k);
            // AS:640 via the table, sign(v) from mps; k >= kTab is recomputed below (rare)
            // (k ^ sign mask) & kMask as one three-input bit operation (truth table 0x48 over
            // a, b, c: (a ^ c) & b); padding elements: mps = 0, r = 0
            const uint32_t code = __builtin_amdgcn_bitop3_b32(sign_mask(mps), kMask, k, 0x48);
            if (WQ) o[c] = copysignf(s_tab[k & (kTab - 1)], mps);
            if (WC) w |= code << (kBits * c);
        }
        if (WC) kmax = max(kmax, m4);
        if (__builtin_expect(!(m4 < kLim) || (WQ && arith), 0)) {
            const float ms[4] = {tv.mps[4 * k4], tv.mps[4 * k4 + 1], tv.mps[4 * k4 + 2], tv.mps[4 * k4 + 3]};
#pragma unroll 1
            for (int c = 0; c < 4; ++c) {
                const float mps = pick4(ms, c);
                const uint32_t k = pick4(ks, c);
                if (!(k < kLim) || (WQ && arith)) {
                    const float fla = floorf(fabsf(mps));
                    const float kf = fla + (float)(k - (uint32_t)(int)fla);        // fl + r, r = 0 or 1
                    if (WQ) {
                        const float oc = (copysignf(L, mps) * kf) / fm;             // ((L1*sign)*(fl+r))/m
#pragma unroll
                        for (int e = 0; e < 4; ++e) o[e] = c == e ? oc : o[e];
                    }
                    if (WC) w = (w & ~(kMask << (kBits * c))) | ((code_of(mps, kf) & kMask) << (kBits * c));
                }
            }
        }
        if (WQ) *reinterpret_cast<float4*>(&s_o[swz(tid, k4)]) = make_float4(o[0], o[1], o[2], o[3]);
        if (WC && !NIB) cw[k4] = w;
        if (WC && NIB) cw[k4 >> 1] = (k4 & 1) ? (cw[k4 >> 1] | (w << 16)) : w;
    }
}

template <bool CVEC>
__device__ __forceinline__ void store_codes(int8_t* __restrict__ ct, const uint32_t (&cw)[4], int len, int tid) {
    if (!CVEC) tid = opaque(tid);               // the bytewise form's 16 addresses: not worth registers
    const int i0 = tid * kQItems;
    if (CVEC && i0 + kQItems <= len) {
        const u32x4v v = {cw[0], cw[1], cw[2], cw[3]};
        __builtin_nontemporal_store(v, reinterpret_cast<u32x4v*>(ct + i0));
    } else {
        for (int k = 0; k < kQItems && i0 + k < len; ++k) ct[i0 + k] = (int8_t)((cw[k >> 2] >> (8 * (k & 3))) & 0xFF);
    }
}

// codes of tile t0 (element offset) of one row: one 16-byte buffer store per thread
// (beyond d: dropped by the range check), or bytewise when d % 16 != 0.
template <bool CVEC, bool NIB = false>
__device__ __forceinline__ void store_codes_buf(__amdgpu_buffer_rsrc_t rc, int8_t* __restrict__ crow,
                                                const uint32_t (&cw)[4], uint32_t t0, int64_t d, int tid) {
    if (NIB) {                                   // 4-bit codes: 8 bytes per thread (d % 32 == 0)
        typedef uint32_t u32x2n __attribute__((ext_vector_type(2)));
        const u32x2n v = {cw[0], cw[1]};
        __builtin_amdgcn_raw_buffer_store_b64(v, rc, (t0 + (uint32_t)(tid * kQItems)) / 2u, 0, kAuxNT);
    } else if (CVEC) {
        const u32x4v v = {cw[0], cw[1], cw[2], cw[3]};
        __builtin_amdgcn_raw_buffer_store_b128(v, rc, t0 + (uint32_t)(tid * kQItems), 0, kAuxNT);
    } else {
        const int64_t rem = d - (int64_t)t0;
        store_codes<false>(crow + t0, cw, (int)(rem < kQTile ? rem : kQTile), tid);
    }
}

__device__ __forceinline__ void publish_kmax(uint32_t kmaxu, float L, int32_t* kmaxv, int64_t vec, int tid) {
    int kmax = (kmaxu <= 127u && isfinite(L)) ? (int)kmaxu : 128;     // 128 = overflow / not codable
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) kmax = max(kmax, __shfl_xor(kmax, o, kWave));
    if ((tid & (kWave - 1)) == 0) atomicMax(&kmaxv[vec], kmax);
}
// The whole client in this workgroup (the stream form with nseg == 1): the block's max is
// the client's, stored plainly -- kmax needs no zero-fill before the launch (one memset per
// call less: ~5 us of the bench step).  s_red: kQBlock / kWave ints of LDS.
__device__ __forceinline__ void store_kmax_block(uint32_t kmaxu, float L, int32_t* kmaxv, int64_t vec, int tid,
                                                 int* s_red) {
    int kmax = (kmaxu <= 127u && isfinite(L)) ? (int)kmaxu : 128;
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) kmax = max(kmax, __shfl_xor(kmax, o, kWave));
    if ((tid & (kWave - 1)) == 0) s_red[tid / kWave] = kmax;
    __syncthreads();
    if (tid == 0) {
        int m = s_red[0];
#pragma unroll
        for (int w = 1; w < kQBlock / kWave; ++w) m = max(m, s_red[w]);
        kmaxv[vec] = m;
    }
}

template <bool VEC4>
__device__ __forceinline__ void store_tile(const float* s_data, float* __restrict__ ot, int len, int tid) {
    if (VEC4 && len == kQTile) {
#pragma unroll
        for (int j = 0; j < kQTile / 4 / kQBlock; ++j) {
            const int q = tid + j * kQBlock;
            st_stream(reinterpret_cast<float4*>(ot) + q, *reinterpret_cast<const float4*>(&s_data[swz(q >> 2, q & 3)]));
        }
    } else {
        for (int i = tid; i < len; i += kQBlock) ot[i] = s_data[swz_elem(i)];
    }
}

// K2-stream: one workgroup streams one whole client vector, tiles in order, the next
// tile prefetched into registers; the exact prefix P is carried in the workgroup.  No
// inter-workgroup communication at all.  Used when there are enough clients to fill
// the GPU (batched DME, the bench workload).  Requires d % 4 == 0 and 4*d < 2^31
// (buffer addressing); the host uses the per-tile form otherwise.
//
// Order of the vector-memory operations per iteration t: stores of tile t-1 (q from the LDS
// image s_o, codes from registers), THEN the loads of tile t+1.  vmcnt counts stores too and
// retires in issue order, so with the loads last the waits before staging tile t+1 (vmcnt 3,
// 2, 1, 0: the loop's only waits on vector memory) wait for nothing younger than the loads,
// and stores and loads both overlap the whole compute of tile t.  The loop keeps no scratch
// (tools/k2_codegen.py, tests/test_k2_codegen.py): the per-thread addresses are one swizzled
// base plus immediates (swz_q0), and the rare paths derive theirs from an opaque copy of tid
// instead of holding them across the loop.
//
// The 4-bit form (kCodesEarly) stores the codes of tile t as soon as pass 2 has them, at the
// end of iteration t.  That store is then the youngest operation at the staging waits, so the
// last of them also waits for its acknowledgement, and the q stores and the loads go out
// after it.  Measured, not designed: an earlier build reloaded spilled addresses from scratch
// between the tile's first store and the others and so waited for that store by accident;
// with no store acknowledged before the others go out the step's K2 takes 1.69 ms instead of
// 1.63 ms (every output placement shifts alike); waiting for all the stores, for the second
// q store, or sleeping instead does not help.
//
// Segments: workgroup b takes client b / nseg, tiles [s*seg_tiles, (s+1)*seg_tiles) with
// s = b % nseg, starting from the exact P = pre[first tile] (the per-client fold of the
// small-batch form) -- or from P = 0 over the whole vector when nseg == 1 (pre == nullptr).
// The tile loop of one workgroup (tiles [tb, te) of client `vec` from the exact start P).
template <bool WQ, bool WC, bool CVEC, bool NIB = false>
__device__ __forceinline__ void stream_tiles(const float* __restrict__ x, float* __restrict__ out,
                                             int8_t* __restrict__ codes, int32_t* __restrict__ overflow, int64_t d,
                                             int32_t tb, int32_t te, float fm, float Xv, float L, int32_t nseg,
                                             double P, int64_t ldo, int64_t ldc, int64_t vec, float* s_x, float* s_o,
                                             float* s_tab, ScanLds& sl) {
    const int tid = threadIdx.x;
    const DivPlan dp = div_plan(L);
    const uint32_t row_bytes = (uint32_t)(d * 4);
    const __amdgpu_buffer_rsrc_t rx = make_rsrc(x + vec * d, row_bytes);
    const __amdgpu_buffer_rsrc_t ro = make_rsrc(WQ ? out + vec * ldo : x, row_bytes);
    const __amdgpu_buffer_rsrc_t rc = make_rsrc(WC ? (const void*)(codes + vec * ldc) : (const void*)x,
                                                row_bytes / (NIB ? 8u : 4u));
    TileRegs pre_x;
    load_tile_buf(pre_x, rx, (uint32_t)tb * (uint32_t)(kQTile * 4), tid);
    build_table(s_tab, tid, L, fm);
    uint32_t cw[4] = {0u, 0u, 0u, 0u};
    uint32_t kmax = 0u;
    constexpr bool kCodesEarly = WQ && WC && NIB;   // see above; only the 4-bit form was measured
    for (int32_t tile = tb; tile < te; ++tile) {
        stage_tile<true>(pre_x, s_x, tid);
        __syncthreads();                           // s_x(t) staged; s_o(t-1) complete
        if (tile > tb) {
            const uint32_t tp = (uint32_t)(tile - 1) * (uint32_t)kQTile;
            if (WQ) store_tile_buf(s_o, ro, tp * 4u, tid);      // beyond d: dropped by the range check
            if (WC && !kCodesEarly) store_codes_buf<CVEC, NIB>(rc, codes + vec * ldc, cw, tp, d, tid);
        }
        if (tile + 1 < te) load_tile_buf(pre_x, rx, (uint32_t)(tile + 1) * (uint32_t)(kQTile * 4), tid);
        const int64_t t0 = (int64_t)tile * kQTile;
        const int len = (int)((d - t0) < kQTile ? (d - t0) : kQTile);
        TileState st;
        TileVals tv;
        P = uniform_d(P);
        const Binade B = binade_of(P);
        // pass 1's barrier also orders the s_o reads above before pass 2's s_o writes
        if (len == kQTile)
            tile_pass1<true, true>(s_x, tv, sl, tid, len, dp, fm, B, st);
        else
            tile_pass1<false, true>(s_x, tv, sl, tid, len, dp, fm, B, st);
        double pnext;
        const double base = resolve_exact(P, B, st, tv, s_x, sl, tid, pnext);
        tile_pass2<WQ, WC, NIB>(s_o, tv, s_tab, tid, base, L, fm, Xv, cw, kmax);
        if (kCodesEarly) store_codes_buf<CVEC, NIB>(rc, codes + vec * ldc, cw, (uint32_t)tile * (uint32_t)kQTile, d, tid);
        P = pnext;
    }
    __syncthreads();
    const uint32_t tp = (uint32_t)(te - 1) * (uint32_t)kQTile;
    if (WQ) store_tile_buf(s_o, ro, tp * 4u, tid);
    if (WC) {
        if (!kCodesEarly) store_codes_buf<CVEC, NIB>(rc, codes + vec * ldc, cw, tp, d, tid);
        if (nseg == 1)
            store_kmax_block(kmax, L, overflow, vec, tid, reinterpret_cast<int*>(sl.wave));
        else
            publish_kmax(kmax, L, overflow, vec, tid);
    }
}

template <bool WQ, bool WC, bool CVEC, bool NIB = false>
__global__ void __launch_bounds__(kQBlock, 4)
quantize_stream_kernel(const float* __restrict__ x, float* __restrict__ out, int8_t* __restrict__ codes,
                       int32_t* __restrict__ overflow, int64_t d, int32_t tiles, float fm,
                       const float* __restrict__ Xs, float Xval, const float* __restrict__ l1, int32_t seg_tiles,
                       int32_t nseg, const uint64_t* __restrict__ pre, int64_t ldo, int64_t ldc) {
    __shared__ __attribute__((aligned(16))) float s_x[kQTile];     // input image of tile t (then scratch)
    __shared__ __attribute__((aligned(16))) float s_o[kQTile];     // output image of tile t-1 / t
    __shared__ float s_tab[kTab];
    __shared__ ScanLds sl;
    const int64_t vec = blockIdx.x / (uint32_t)nseg;
    const int32_t tb = (int32_t)(blockIdx.x % (uint32_t)nseg) * seg_tiles;
    const int32_t te = min(tiles, tb + seg_tiles);
    const float Xv = Xs ? Xs[vec] : Xval;            // one vector per call: X passed by value
    const double P = pre ? __longlong_as_double((long long)pre[vec * tiles + tb]) : 0.0;
    stream_tiles<WQ, WC, CVEC, NIB>(x, out, codes, overflow, d, tb, te, fm, Xv, l1[vec], nseg, P, ldo, ldc, vec, s_x,
                                    s_o, s_tab, sl);
}

constexpr int64_t kSmallL1Max = kGrain - 1;
__device__ __forceinline__ float block_torch_l1(const float* __restrict__ xv, int64_t s, float* scr) {
    return block_torch_sum(xv, s, scr, [](float v) { return fabsf(v); });
}

// The whole AS:609-641 for vectors shorter than GRAIN in ONE launch (the reference's own
// harness sizes: d = 1024 in C1, 2048 in Normal_dist.py:40): one workgroup per client computes
// L1 in torch order (or takes l1in), then streams its tiles exactly as quantize_stream_kernel.
template <bool WQ, bool WC, bool CVEC>
__global__ void __launch_bounds__(kQBlock, 4)
quantize_small_kernel(const float* __restrict__ x, float* __restrict__ out, int8_t* __restrict__ codes,
                      int32_t* __restrict__ overflow, int64_t d, int32_t tiles, float fm,
                      const float* __restrict__ Xs, float Xval, const float* __restrict__ l1in,
                      float* __restrict__ l1out, int64_t ldo, int64_t ldc) {
    __shared__ __attribute__((aligned(16))) float s_x[kQTile];
    __shared__ __attribute__((aligned(16))) float s_o[kQTile];
    __shared__ float s_tab[kTab];
    __shared__ ScanLds sl;
    const int64_t vec = blockIdx.x;
    const float L = l1in ? l1in[vec] : block_torch_l1(x + vec * d, d, s_x);     // AS:624
    if (l1out && threadIdx.x == 0) l1out[vec] = L;
    const float Xv = Xs ? Xs[vec] : Xval;
    stream_tiles<WQ, WC, CVEC>(x, out, codes, overflow, d, 0, tiles, fm, Xv, L, 1, 0.0, ldo, ldc, vec, s_x, s_o, s_tab,
                               sl);
}

// ---- small-batch forms (fewer clients than fill the GPU one workgroup per client) ----
// (irregular-tile records, see TileRec below)
constexpr int kRecEvents = 48;          // events per record
constexpr int kRecPerClient = 32;       // records per client
constexpr int kRecClients = 256;        // clients per launch chunk with records
//   approximate tile sums A_t (agg_stream_kernel over segments, or tile_agg_kernel)
//   tile_map_kernel      per tile: P'_t = the sums before it (approximate prefix), then in
//                        the binade of P'_t the exact map (m0, m1), or an irregular tile's
//                        event record
//   exact_fold_kernel    per client, serial: P_0 = 0, P_{t+1} = P_t + m[parity(P_t)];
//                        irregular tiles recomputed from their exact P_t
//   outputs              quantize_stream_kernel over segments / tile_out_kernel from P_t
// Maps and prefixes are stored as raw fp64 bits in u64 arrays.

// Approximate tile sums over a segment, streamed with the stream kernel's prefetch.
__global__ void __launch_bounds__(kQBlock, 4)
agg_stream_kernel(const float* __restrict__ x, int64_t d, int32_t tiles, float fm, const float* __restrict__ l1,
                  int32_t seg_tiles, int32_t nseg, uint64_t* __restrict__ agg, uint32_t* __restrict__ reccnt) {
    __shared__ __attribute__((aligned(16))) float s_x[kQTile];
    __shared__ ScanLds sl;
    const int tid = threadIdx.x;
    const int64_t vec = blockIdx.x / (uint32_t)nseg;
    const int32_t tb = (int32_t)(blockIdx.x % (uint32_t)nseg) * seg_tiles;
    const int32_t te = min(tiles, tb + seg_tiles);
    if (tb == 0 && tid == 0 && vec < kRecClients) reccnt[vec] = 0u;   // tile_map_kernel's record counter
    const DivPlan dp = div_plan(l1[vec]);
    const __amdgpu_buffer_rsrc_t rx = make_rsrc(x + vec * d, (uint32_t)(d * 4));
    const Binade B = binade_of(0.0);
    TileRegs pre_x;
    load_tile_buf(pre_x, rx, (uint32_t)tb * (uint32_t)(kQTile * 4), tid);
    for (int32_t tile = tb; tile < te; ++tile) {
        stage_tile<true>(pre_x, s_x, tid);
        __syncthreads();
        if (tile + 1 < te) load_tile_buf(pre_x, rx, (uint32_t)(tile + 1) * (uint32_t)(kQTile * 4), tid);
        const int64_t t0 = (int64_t)tile * kQTile;
        const int len = (int)((d - t0) < kQTile ? (d - t0) : kQTile);
        TileState st;
        TileVals tv;
        if (len == kQTile)
            tile_pass1<true, false>(s_x, tv, sl, tid, len, dp, fm, B, st);
        else
            tile_pass1<false, false>(s_x, tv, sl, tid, len, dp, fm, B, st);
        if (tid == 0) agg[vec * tiles + tile] = (uint64_t)__double_as_longlong(st.total);
    }
}

// Approximate tile sums, one workgroup per tile (any row alignment).
template <bool VEC4>
__global__ void __launch_bounds__(kQBlock)
tile_agg_kernel(const float* __restrict__ x, int64_t d, int32_t tiles, float fm, const float* __restrict__ l1,
                uint64_t* __restrict__ agg, uint32_t* __restrict__ reccnt) {
    __shared__ __attribute__((aligned(16))) float s_x[kQTile];
    __shared__ ScanLds sl;
    const int tid = threadIdx.x;
    const int32_t tile = blockIdx.x;
    const int64_t vec = blockIdx.y;
    if (tile == 0 && tid == 0 && vec < kRecClients) reccnt[vec] = 0u;   // tile_map_kernel's record counter
    TileRegs r;
    load_tile<VEC4>(r, x, d, tiles, (uint32_t)(vec * tiles + tile), tid);
    stage_tile<VEC4>(r, s_x, tid);
    __syncthreads();
    const int64_t t0 = (int64_t)tile * kQTile;
    const int len = (int)((d - t0) < kQTile ? (d - t0) : kQTile);
    const DivPlan dp = div_plan(l1[vec]);
    const Binade B = binade_of(0.0);
    TileState st;
    TileVals tv;
    if (len == kQTile)
        tile_pass1<true, false>(s_x, tv, sl, tid, len, dp, fm, B, st);
    else
        tile_pass1<false, false>(s_x, tv, sl, tid, len, dp, fm, B, st);
    if (tid == 0) agg[vec * tiles + tile] = (uint64_t)__double_as_longlong(st.total);
}

// Irregular tiles of the small-batch forms are recorded by the map kernel as their event
// list (classified from P', valid for the exact start by the kEdge margin): per event the
// run sum before it, then a clean tie's (t0, t1) or an edge thread's 16 fractions, and the
// run sum after the last event.  The fold walks a record in LDS instead of loading and
// resolving the tile.  Tiles with more events, or beyond a client's record budget, or of
// clients past kRecClients, are resolved from the data as before.
struct EvEntry {
    double run;                         // run sum between the previous event and this one
    double t0, t1;                      // clean tie
    uint32_t tie;                       // 1: clean tie, 0: edge thread (fr)
    uint32_t pad;
    float fr[kQItems];
};
struct TileRec {
    uint32_t count;
    uint32_t pad;
    double last_run;                    // run sum after the last event
    EvEntry ev[kRecEvents];
};

// Exact tile maps in the binade E of P'_t, in units of G = 2^(E-52): map0[t] = m0/G | (E+1023)
// << 53 and map1[t] = m1/G (both < 2^52); an irregular tile has map0 = kIrrMap and map1 = its
// record number + 1 (0: no record).
// The approximate tile sums of each client -> their exclusive prefix P'_t, in place (one
// workgroup per client, fp64; any order would do: P' only picks each tile's binade).  Each
// tile_map workgroup used to sum its predecessors itself: O(tiles^2) loads per client, 4 MB per
// client at d = 2^22 (the map pass 420 us for 101 clients of 2^22, profiles/r6d_*).
__global__ void __launch_bounds__(kQBlock)
tile_prefix_kernel(uint64_t* __restrict__ agg, int32_t tiles) {
    __shared__ double s_w[kQBlock / kWave];
    constexpr int K = 8;
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wid = tid / kWave;
    uint64_t* a = agg + (int64_t)blockIdx.x * tiles;
    double carry = 0.0;
    for (int32_t b0 = 0; b0 < tiles; b0 += kQBlock * K) {
        const int32_t j0 = b0 + tid * K;
        double v[K], s = 0.0;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            v[k] = j0 + k < tiles ? __longlong_as_double((long long)a[j0 + k]) : 0.0;
            s += v[k];
        }
        double inc = s;                                  // inclusive scan over the wave
#pragma unroll
        for (int o = 1; o < kWave; o <<= 1) {
            const double t = __shfl_up(inc, o, kWave);
            if (lane >= o) inc += t;
        }
        if (lane == kWave - 1) s_w[wid] = inc;
        __syncthreads();
        double e = carry + inc - s, tot = 0.0;
#pragma unroll
        for (int w = 0; w < kQBlock / kWave; ++w) {
            if (w < wid) e += s_w[w];
            tot += s_w[w];
        }
#pragma unroll
        for (int k = 0; k < K; ++k) {
            if (j0 + k < tiles) a[j0 + k] = (uint64_t)__double_as_longlong(e);
            e += v[k];
        }
        carry += tot;
        __syncthreads();
    }
}

constexpr uint64_t kIrrMap = ~0ull;
template <bool VEC4>
__global__ void __launch_bounds__(kQBlock)
tile_map_kernel(const float* __restrict__ x, int64_t d, int32_t tiles, float fm, const float* __restrict__ l1,
                const uint64_t* __restrict__ agg, uint64_t* __restrict__ map0, uint64_t* __restrict__ map1,
                TileRec* __restrict__ recs, uint32_t* __restrict__ reccnt, int32_t prefixed) {
    __shared__ __attribute__((aligned(16))) float s_x[kQTile];
    __shared__ ScanLds sl;
    const int tid = threadIdx.x;
    const int32_t tile = blockIdx.x;
    const int64_t vec = blockIdx.y;
    const int64_t idx = vec * tiles + tile;
    TileRegs r;
    load_tile<VEC4>(r, x, d, tiles, (uint32_t)idx, tid);
    // P'_t = the approximate tile sums before t, in any order (it only picks the binade): from
    // tile_prefix_kernel (prefixed), or summed here (a single client: the extra launch costs
    // more than 1024 tiles' predecessors from L2, 0.155 -> 0.171 ms per call at 2^22)
    double Pg;
    if (prefixed) {
        Pg = uniform_d(__longlong_as_double((long long)agg[idx]));
    } else {
        double acc = 0.0;
        for (int32_t j = tid; j < tile; j += kQBlock) acc += __longlong_as_double((long long)agg[vec * tiles + j]);
#pragma unroll
        for (int o = kWave / 2; o > 0; o >>= 1) acc += __shfl_xor(acc, o, kWave);
        if ((tid & (kWave - 1)) == 0) sl.wave[tid / kWave] = acc;
        __syncthreads();
        Pg = uniform_d(((sl.wave[0] + sl.wave[1]) + sl.wave[2]) + sl.wave[3]);
    }
    const Binade B = binade_of(Pg);
    stage_tile<VEC4>(r, s_x, tid);
    __syncthreads();
    const int64_t t0 = (int64_t)tile * kQTile;
    const int len = (int)((d - t0) < kQTile ? (d - t0) : kQTile);
    const DivPlan dp = div_plan(l1[vec]);
    TileState st;
    TileVals tv;
    if (len == kQTile)
        tile_pass1<true, true>(s_x, tv, sl, tid, len, dp, fm, B, st);
    else
        tile_pass1<false, true>(s_x, tv, sl, tid, len, dp, fm, B, st);
    double m0 = 0.0, m1 = 0.0;
    if (resolve_map(Pg, B, st, s_x, sl, tid, m0, m1)) {
        if (tid == 0) {                                        // in units of G, with the binade
            const uint64_t eb = (uint64_t)__double_as_longlong(B.b0) >> 52;
            const int sh = 52 - ((int)eb - 1023);
            map0[idx] = (uint64_t)ldexp(m0, sh) | (eb << 53);
            map1[idx] = (uint64_t)ldexp(m1, sh);
        }
        return;
    }
    // irregular: record the events (classified from P')
    IrrThread it;
    irregular_prep(Pg, st, tv, s_x, sl, tid, it);
    int ne = 0;
#pragma unroll
    for (int w = 0; w < kQBlock / kWave; ++w) ne += __builtin_popcountll(uniform_u64(sl.tmask[w]));
    if (tid == 0) {
        uint32_t rn = 0;
        if (ne <= kRecEvents && vec < kRecClients) {
            const uint32_t slotno = atomicAdd(&reccnt[vec], 1u);
            rn = slotno < (uint32_t)kRecPerClient ? slotno + 1u : 0u;
        }
        sl.misc[0] = (double)rn;
    }
    __syncthreads();
    const uint32_t rno = (uint32_t)sl.misc[0];
    if (tid == 0) {
        map0[idx] = kIrrMap;
        map1[idx] = rno;
    }
    if (rno == 0u) return;
    TileRec* rec = recs + (vec * kRecPerClient + (rno - 1u));
    if (it.event) {
        const int lane = tid & (kWave - 1), wid = tid / kWave;
        int e = __builtin_popcountll(sl.tmask[wid] & ((1ull << lane) - 1ull));
        for (int w = 0; w < wid; ++w) e += __builtin_popcountll(sl.tmask[w]);
        EvEntry& ev = rec->ev[e];
        const double* q = slot_of(s_x, tid);
        ev.run = it.x;                                         // inclusive run sum; own v is 0
        const bool tie = (sl.cmask[wid] >> lane) & 1ull;
        ev.tie = tie ? 1u : 0u;
        if (tie) {
            ev.t0 = q[0];
            ev.t1 = q[1];
        } else {
#pragma unroll
            for (int k = 0; k < kQItems; ++k) ev.fr[k] = reinterpret_cast<const float*>(q)[k];
        }
    }
    if (tid == kQBlock - 1) {
        rec->count = (uint32_t)ne;
        rec->last_run = it.event ? 0.0 : it.x;
    }
}

constexpr int kFoldEvents = 256;   // record events prefetched into LDS (24 KB)
constexpr int kFoldMaps = 1024;    // tile maps prefetched into LDS (16 KB): d <= 2^22 in one go

__device__ __forceinline__ uint64_t shfl_up64(uint64_t v, int o) {
    const uint32_t lo = __shfl_up((uint32_t)v, o, kWave), hi = __shfl_up((uint32_t)(v >> 32), o, kWave);
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t readlane64(uint64_t v, int l) {
    const uint32_t lo = __builtin_amdgcn_readlane((uint32_t)v, l);
    const uint32_t hi = __builtin_amdgcn_readlane((uint32_t)(v >> 32), l);
    return ((uint64_t)hi << 32) | lo;
}

// One workgroup per client: the exact serial fold over its tile maps; irregular tiles are
// walked from their event records, or loaded and resolved from their exact start.
// pre[t] = exact P_t.  A run of regular maps is walked in integer units of its binade's G
// (P stays in the binade): a parity select and a 64-bit add per tile on uniform values,
// maps read 8 ahead.
template <bool VEC4>
__global__ void __launch_bounds__(kQBlock)
exact_fold_kernel(const float* __restrict__ x, int64_t d, int32_t tiles, float fm, const float* __restrict__ l1,
                  const uint64_t* __restrict__ map0, const uint64_t* __restrict__ map1, uint64_t* __restrict__ pre,
                  const TileRec* __restrict__ recs, const uint32_t* __restrict__ reccnt) {
    __shared__ __attribute__((aligned(16))) float s_x[kQTile];
    __shared__ ScanLds sl;
    __shared__ EvEntry s_ev[kFoldEvents];                  // the client's records, prefetched
    __shared__ uint32_t s_roff[kRecPerClient], s_rcnt[kRecPerClient];
    __shared__ double s_rlast[kRecPerClient];
    __shared__ uint64_t s_m0[kFoldMaps], s_m1[kFoldMaps];
    const int tid = threadIdx.x;
    const int64_t vec = blockIdx.x;
    const int64_t base = vec * tiles;
    const DivPlan dp = div_plan(l1[vec]);
    // every map in LDS when they fit: a run restarted after an irregular tile then reads its
    // next 64 maps from LDS instead of waiting a global round trip (the fold at n = 1 is the
    // serial floor of the per-call drop-in)
    const bool mcache = tiles <= kFoldMaps;
    if (mcache)
        for (int i = tid; i < tiles; i += kQBlock) {
            s_m0[i] = map0[base + i];
            s_m1[i] = map1[base + i];
        }
    auto M0 = [&](int32_t t) -> uint64_t { return mcache ? s_m0[t] : map0[base + t]; };
    auto M1 = [&](int32_t t) -> uint64_t { return mcache ? s_m1[t] : map1[base + t]; };
    // prefetch every record of this client that fits (two dependent round trips in all)
    const int nrec = vec < kRecClients ? (int)min(reccnt[vec], (uint32_t)kRecPerClient) : 0;
    if (tid < nrec) {
        s_rcnt[tid] = recs[vec * kRecPerClient + tid].count;
        s_rlast[tid] = recs[vec * kRecPerClient + tid].last_run;
    }
    __syncthreads();
    if (tid == 0) {
        uint32_t off = 0;
        for (int r = 0; r < nrec; ++r) {
            const bool fits = off + s_rcnt[r] <= (uint32_t)kFoldEvents;
            s_roff[r] = fits ? off : ~0u;
            if (fits) off += s_rcnt[r];
        }
    }
    __syncthreads();
    for (int r = 0; r < nrec; ++r) {
        if (s_roff[r] == ~0u) continue;
        const uint32_t* src = reinterpret_cast<const uint32_t*>(recs[vec * kRecPerClient + r].ev);
        uint32_t* dst = reinterpret_cast<uint32_t*>(s_ev + s_roff[r]);
        const int nw = (int)(s_rcnt[r] * (sizeof(EvEntry) / 4));
        for (int i = tid; i < nw; i += kQBlock) dst[i] = src[i];
    }
    __syncthreads();
    constexpr uint64_t kMant = (1ull << 52) - 1ull;
    uint64_t Pb = 0;                                           // bits of the exact P (P_0 = 0)
    int32_t tile = 0;
    while (tile < tiles) {
        // a run of regular maps, 64 tiles at a time: lane l holds the map of tile blk + l
        // (the next 64 are loaded meanwhile).  A map in units of G is P -> P + d[P & 1];
        // two maps compose to the same form, (F then g).d[p] = F.d[p] + g.d[p ^ (F.d[p] & 1)],
        // so a wave scan gives every tile's exact start at once.  The run ends at the first
        // irregular map or map of another binade (P stays in its binade along a run).
        const int lane = tid & (kWave - 1);
        bool go = true;
        int32_t blk = tile;
        uint64_t am = M0(min(blk + lane, tiles - 1)), bm = M1(min(blk + lane, tiles - 1));
        while (go) {
            const int32_t nb = blk + kWave;
            const uint64_t an = M0(min(nb + lane, tiles - 1)), bn = M1(min(nb + lane, tiles - 1));
            const uint64_t E0 = Pb >> 52;
            const bool valid = blk + lane < tiles && am != kIrrMap && (am >> 53) == E0;
            const uint64_t inv = __ballot(!valid);
            const int f = inv ? (int)__builtin_ctzll(inv) : kWave;        // tiles in the run here
            uint64_t d0 = lane < f ? (am & ((1ull << 53) - 1ull)) : 0ull, d1 = lane < f ? bm : 0ull;
#pragma unroll
            for (int o = 1; o < kWave; o <<= 1) {               // inclusive scan of the maps
                const uint64_t f0 = shfl_up64(d0, o), f1 = shfl_up64(d1, o);
                if (lane >= o) {
                    const uint64_t n0 = f0 + ((f0 & 1ull) ? d1 : d0);
                    const uint64_t n1 = f1 + ((f1 & 1ull) ? d0 : d1);
                    d0 = n0;
                    d1 = n1;
                }
            }
            const uint64_t Pi0 = (Pb & kMant) | (1ull << 52);   // P / G
            const bool odd = (Pi0 & 1ull) != 0ull;
            uint64_t e0 = shfl_up64(d0, 1), e1 = shfl_up64(d1, 1);
            if (lane == 0) e0 = e1 = 0ull;
            const uint64_t st = Pi0 + (odd ? e1 : e0);            // exact start of tile blk + lane
            if (tid < f) pre[base + blk + tid] = (st & kMant) | (E0 << 52);   // wave 0, coalesced
            if (f > 0) {
                const uint64_t inc = odd ? readlane64(d1, f - 1) : readlane64(d0, f - 1);
                Pb = ((Pi0 + inc) & kMant) | (E0 << 52);
            }
            tile += f;
            go = f == kWave;
            blk = nb;
            am = an;
            bm = bn;
        }
        if (tile >= tiles) break;
        // an irregular tile (or a map whose binade P is not in: resolved from the data)
        double P = __longlong_as_double((long long)Pb);
        const int64_t idx = base + tile;
        if (tid == 0) pre[idx] = Pb;
        const uint32_t rid = M0(tile) == kIrrMap ? (uint32_t)M1(tile) : 0u;
        if (rid != 0u && s_roff[rid - 1u] != ~0u) {            // recorded and prefetched: walk it
            if (tid == 0) {
                const EvEntry* ev0 = s_ev + s_roff[rid - 1u];
                double S = P;
                for (uint32_t e = 0; e < s_rcnt[rid - 1u]; ++e) {
                    const EvEntry& ev = ev0[e];
                    S = S + ev.run;                            // exact start of the event
                    if (ev.tie) {
                        S = S + (lowbit(S) ? ev.t1 : ev.t0);
                    } else {
                        for (int k = 0; k < kQItems; ++k) S = S + (double)ev.fr[k];
                    }
                }
                sl.misc[0] = S + s_rlast[rid - 1u];
            }
            __syncthreads();
            P = sl.misc[0];
            __syncthreads();
        } else if (rid != 0u) {                                // recorded: copy it, walk it
            const TileRec* rec = recs + (vec * kRecPerClient + (rid - 1u));
            uint32_t* dst = reinterpret_cast<uint32_t*>(s_x);
            const uint32_t* src = reinterpret_cast<const uint32_t*>(rec);
            for (int i = tid; i < (int)(sizeof(TileRec) / 4); i += kQBlock) dst[i] = src[i];
            __syncthreads();
            if (tid == 0) {
                const TileRec* lr = reinterpret_cast<const TileRec*>(s_x);
                double S = P;
                for (uint32_t e = 0; e < lr->count; ++e) {
                    const EvEntry& ev = lr->ev[e];
                    S = S + ev.run;
                    if (ev.tie) {
                        S = S + (lowbit(S) ? ev.t1 : ev.t0);
                    } else {
                        for (int k = 0; k < kQItems; ++k) S = S + (double)ev.fr[k];
                    }
                }
                sl.misc[0] = S + lr->last_run;
            }
            __syncthreads();
            P = sl.misc[0];
            __syncthreads();
        } else {                                               // from the data
            TileRegs r;
            load_tile<VEC4>(r, x, d, tiles, (uint32_t)idx, tid);
            stage_tile<VEC4>(r, s_x, tid);
            __syncthreads();
            const int64_t t0 = (int64_t)tile * kQTile;
            const int len = (int)((d - t0) < kQTile ? (d - t0) : kQTile);
            const Binade B = binade_of(P);
            TileState st;
            TileVals tv;
            if (len == kQTile)
                tile_pass1<true, true>(s_x, tv, sl, tid, len, dp, fm, B, st);
            else
                tile_pass1<false, true>(s_x, tv, sl, tid, len, dp, fm, B, st);
            double pnext;
            (void)resolve_exact(P, B, st, tv, s_x, sl, tid, pnext);
            __syncthreads();                                   // s_x / sl reused by the next irregular tile
            P = pnext;
        }
        Pb = (uint64_t)__double_as_longlong(P);
        ++tile;
    }
}

// Outputs, one workgroup per tile, from the exact tile prefix pre[t] (any row alignment).
template <bool VEC4, bool WQ, bool WC, bool CVEC>
__global__ void __launch_bounds__(kQBlock)
tile_out_kernel(const float* __restrict__ x, float* __restrict__ out, int8_t* __restrict__ codes,
                int32_t* __restrict__ overflow, int64_t d, int32_t tiles, float fm, const float* __restrict__ Xs,
                float Xval, const float* __restrict__ l1, const uint64_t* __restrict__ pre, int64_t ldo, int64_t ldc) {
    __shared__ __attribute__((aligned(16))) float s_x[kQTile];     // input image, scratch, then output image
    __shared__ float s_tab[kTab];
    __shared__ ScanLds sl;
    const int tid = threadIdx.x;
    const int32_t tile = blockIdx.x;
    const int64_t vec = blockIdx.y;
    TileRegs r;
    load_tile<VEC4>(r, x, d, tiles, (uint32_t)(vec * tiles + tile), tid);
    const float L = l1[vec];
    build_table(s_tab, tid, L, fm);                 // read after pass 1's barrier
    stage_tile<VEC4>(r, s_x, tid);
    __syncthreads();
    const int64_t t0 = (int64_t)tile * kQTile;
    const int len = (int)((d - t0) < kQTile ? (d - t0) : kQTile);
    const DivPlan dp = div_plan(L);
    const double P = __longlong_as_double((long long)pre[vec * tiles + tile]);
    const Binade B = binade_of(P);
    TileState st;
    TileVals tv;
    if (len == kQTile)
        tile_pass1<true, true>(s_x, tv, sl, tid, len, dp, fm, B, st);
    else
        tile_pass1<false, true>(s_x, tv, sl, tid, len, dp, fm, B, st);
    double pnext;
    const double base = resolve_exact(P, B, st, tv, s_x, sl, tid, pnext);   // barrier-terminated if it used s_x
    uint32_t cw[4];
    uint32_t kmax = 0u;
    tile_pass2<WQ, WC>(s_x, tv, s_tab, tid, base, L, fm, Xs ? Xs[vec] : Xval, cw, kmax);   // each thread rewrites its own row
    if (WC) {
        store_codes<CVEC>(codes + vec * ldc + t0, cw, len, tid);
        publish_kmax(kmax, L, overflow, vec, tid);
    }
    __syncthreads();
    if (WQ) store_tile<VEC4>(s_x, out + vec * ldo + t0, len, tid);
}

// =====================================================================================
// K3: est[i] (+)= q[j][i] / n_div, j = 0..n-1 in order (ND:137-138).
// Each thread owns 4 consecutive columns; loads for 8 clients are issued ahead.  1024-thread
// workgroups (16 KB of a client row each): 0.85-0.88 -> 0.75-0.78 ms at 1024 x 2^20 against
// 256 (tools/exp/exp_mean.hip, profiles/r03s_exp_mean_variants.jsonl); non-temporal loads (q
// is read once): 0.740-0.754 -> 0.673-0.684 ms (profiles/r05k_exp_mean_q_variants.jsonl).
// =====================================================================================
constexpr int kMeanThreads = 1024;
template <bool VEC4>
__global__ void __launch_bounds__(kMeanThreads)
client_mean_kernel(const float* __restrict__ q, int64_t n, int64_t d, int64_t ld, float n_div, int accumulate,
                   float* __restrict__ est) {
    const int64_t col = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (col >= d) return;
    if (VEC4) {
        float4 e = accumulate ? *reinterpret_cast<const float4*>(est + col) : make_float4(0.f, 0.f, 0.f, 0.f);
        int64_t j = 0;
        for (; j + 8 <= n; j += 8) {
            float4 t[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) t[u] = ld_stream(reinterpret_cast<const float4*>(q + (j + u) * ld + col));
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                e.x += t[u].x / n_div; e.y += t[u].y / n_div;
                e.z += t[u].z / n_div; e.w += t[u].w / n_div;
            }
        }
        for (; j < n; ++j) {
            const float4 t = *reinterpret_cast<const float4*>(q + j * ld + col);
            e.x += t.x / n_div; e.y += t.y / n_div; e.z += t.z / n_div; e.w += t.w / n_div;
        }
        *reinterpret_cast<float4*>(est + col) = e;
    } else {
        const int cnt = (int)((d - col) < 4 ? (d - col) : 4);
        for (int k = 0; k < cnt; ++k) {
            float e = accumulate ? est[col + k] : 0.f;
            for (int64_t j = 0; j < n; ++j) e += q[j * ld + col + k] / n_div;
            est[col + k] = e;
        }
    }
}

// =====================================================================================
// Type codes (the wire format, see uq_dme.h): decode and decode+mean.
// For one client, |q| = tab[k] = RN(RN(L1*k)/f32(m)) and q carries the code's sign, so
// decoding rebuilds q bit-for-bit (including -0.0).  For the mean, (-a)/n = -(a/n), so
// a per-client table tabn[k] = RN(tab[k]/n_div) gives q/n_div exactly.
// =====================================================================================
constexpr int kDecChunk = 4096;   // elements per decode workgroup (256 threads x 16)
constexpr int kMeanClients = 32;  // clients whose tables are staged in LDS at a time

__device__ __forceinline__ float decode_one(int8_t c, const float* tab) {
    const int ci = (int)c;
    const int k = ci ^ (ci >> 31);                 // ci < 0 ? -ci-1 : ci
    return __uint_as_float(__float_as_uint(tab[k]) ^ ((uint32_t)ci & 0x80000000u));
}

// The decode table entry of count k in either form of the type codes (uq_dme.h UQ_FORM_*):
// unbiased |q| = RN(RN(L1*k)/f32(m)) (AS:640); biased |q| = RN(L1*RN(k/f32(m))) (AS:687), the
// quotient by the biased kernels' correctly rounded division (div1 over div_plan_m).
template <bool BIASED>
__device__ __forceinline__ float code_table_entry(float L, int k, float fm) {
    if constexpr (BIASED) return L * div1((float)k, div_plan_m(fm));
    else return (L * (float)k) / fm;
}

template <bool VEC, bool BIASED>
__device__ __forceinline__ void codes_decode_body(const int8_t* __restrict__ codes, const float* __restrict__ l1,
                                                  int64_t d, float fm, float* __restrict__ out) {
    __shared__ float tab[128];
    const int64_t vec = blockIdx.y;
    const int tid = threadIdx.x;
    const float L = l1[vec];
    if (tid < 128) tab[tid] = code_table_entry<BIASED>(L, tid, fm);
    __syncthreads();
    const int64_t i0 = (int64_t)blockIdx.x * kDecChunk + (int64_t)tid * 16;
    const int8_t* cr = codes + vec * d;
    float* orow = out + vec * d;
    if (VEC && i0 + 16 <= d) {
        const uint4 w = *reinterpret_cast<const uint4*>(cr + i0);
        const uint32_t ws[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (int k4 = 0; k4 < 4; ++k4) {
            float o[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) o[c] = decode_one((int8_t)((ws[k4] >> (8 * c)) & 0xFF), tab);
            *reinterpret_cast<float4*>(orow + i0 + 4 * k4) = make_float4(o[0], o[1], o[2], o[3]);
        }
    } else {
        for (int64_t i = i0; i < i0 + 16 && i < d; ++i) orow[i] = decode_one(cr[i], tab);
    }
}

template <bool VEC>
__global__ void __launch_bounds__(256)
codes_decode_kernel(const int8_t* __restrict__ codes, const float* __restrict__ l1, int64_t d, float fm,
                    float* __restrict__ out) {
    codes_decode_body<VEC, false>(codes, l1, d, fm, out);
}

// The biased form's decode (uq_codes_decode_form_f32 with UQ_FORM_BIASED).
template <bool VEC>
__global__ void __launch_bounds__(256)
codes_decode_biased_kernel(const int8_t* __restrict__ codes, const float* __restrict__ l1, int64_t d, float fm,
                           float* __restrict__ out) {
    codes_decode_body<VEC, true>(codes, l1, d, fm, out);
}

// est[i] (+)= q_j[i] / n_div for clients j in order, q decoded from codes.  Each thread
// owns kMeanCpt consecutive columns (one 8-byte code load per client).  Client tables
// tabn[j][k] = RN(RN(RN(L1_j*k)/m)/n_div) for k <= kmax_j are staged kMeanClients at a
// time (kmax_j from the encoder keeps them tiny: ~8 entries at R = 1); each wave builds
// whole clients' tables from wave-uniform SCALAR loads of L1_j and kmax_j, so the table
// build never waits on the vector-memory counter.  Code loads go in batches of
// kMeanUnroll clients, double-buffered: batch b+1 (crossing group boundaries) is in
// flight while batch b is summed.
constexpr int kMeanCpt = 8;
constexpr int kCodesMeanThreads = 512;          // per workgroup: the tables serve 4 K columns
constexpr int kMeanUnroll = 16;
static_assert(kMeanClients == 2 * kMeanUnroll, "two code batches per table group");

__device__ __forceinline__ void mean_load_batch(uint2 (&w)[kMeanUnroll], const int8_t* cp, int64_t ldc) {
#pragma unroll
    for (int u = 0; u < kMeanUnroll; ++u) {
        const u32x2v t = __builtin_nontemporal_load(reinterpret_cast<const u32x2v*>(cp + (int64_t)u * ldc));
        w[u] = make_uint2(t.x, t.y);
    }
}

__device__ __forceinline__ void mean_add_batch(float (&e)[kMeanCpt], const uint2 (&w)[kMeanUnroll],
                                               const float (*tabn)[256], int jj) {
#pragma unroll
    for (int u = 0; u < kMeanUnroll; ++u) {
        const float* tb = tabn[jj + u];
#pragma unroll
        for (int k = 0; k < 4; ++k) e[k] += tb[(w[u].x >> (8 * k)) & 0xFF];
#pragma unroll
        for (int k = 0; k < 4; ++k) e[4 + k] += tb[(w[u].y >> (8 * k)) & 0xFF];
    }
}

// Tables of clients j0 .. j0+nb-1 into tabn (callers bracket it with barriers).
template <bool BIASED = false>
__device__ __forceinline__ void mean_build_tables(float (*tabn)[256], const float* __restrict__ l1,
                                                  const int32_t* __restrict__ kmaxv, int64_t j0, int nb, int wid,
                                                  int lane, float fm, float n_div) {
    for (int jj = wid; jj < nb; jj += kCodesMeanThreads / kWave) {
        const float L = l1[j0 + jj];                // wave-uniform: scalar loads
        const int km = min(127, max(0, kmaxv[j0 + jj]));
        for (int k = lane; k <= km; k += kWave) {
            const float v = code_table_entry<BIASED>(L, k, fm) / n_div;
            tabn[jj][k] = v;                        // code k
            tabn[jj][255 - k] = -v;                 // code ~k = -k-1 -> byte 255-k; (-a)/n = -(a/n)
        }
    }
}

// ragged / unaligned columns: bytewise, clients j0 .. j0+nb-1 in order
__device__ __forceinline__ void mean_add_bytes(float (&e)[kMeanCpt], const int8_t* __restrict__ codes, int64_t ldc,
                                               const float (*tabn)[256], int64_t j0, int nb, int64_t i0, int64_t d) {
    for (int jj = 0; jj < nb; ++jj)
        for (int k = 0; k < kMeanCpt; ++k)
            if (i0 + k < d) e[k] += tabn[jj][(uint8_t)codes[(j0 + jj) * ldc + i0 + k]];
}

// Overflowed clients (kmax > 127: a count saturated its int8 code) among j0 .. j0+nb-1.
__device__ __forceinline__ uint32_t mean_ovf_mask(const int32_t* __restrict__ kmaxv, int64_t j0, int nb) {
    uint32_t mk = 0;
    for (int jj = 0; jj < nb; ++jj) mk |= (kmaxv[j0 + jj] > 127 ? 1u : 0u) << jj;
    return mk;
}

// Clients j0 .. j0+nb-1 in order when some client overflowed: an overflowed client adds
// q[j][i] / n_div read from the dequantized batch (what K2 wrote correctly beside the
// saturated codes; the same bits as its table entry would have had), the others their
// table entries.  Any column alignment.
__device__ __forceinline__ void mean_add_mixed(float (&e)[kMeanCpt], const int8_t* __restrict__ codes, int64_t ldc,
                                            const float* __restrict__ q, int64_t ldq, const float (*tabn)[256],
                                            uint32_t ovf, int64_t j0, int nb, int64_t i0, int64_t d, float n_div) {
    for (int jj = 0; jj < nb; ++jj) {
        const int64_t j = j0 + jj;
        if ((ovf >> jj) & 1u) {
            for (int k = 0; k < kMeanCpt; ++k)
                if (i0 + k < d) e[k] += q[j * ldq + i0 + k] / n_div;
        } else {
            for (int k = 0; k < kMeanCpt; ++k)
                if (i0 + k < d) e[k] += tabn[jj][(uint8_t)codes[j * ldc + i0 + k]];
        }
    }
}

// ALL: every thread's kMeanCpt columns lie inside d (d a multiple of kCodesMeanThreads *
// kMeanCpt), so no
// per-thread `full` test anywhere (a per-thread guard around the adds cost the loads'
// overlap in other kernels here).
template <bool VEC, bool ALL, bool BIASED>
__device__ __forceinline__ void codes_mean_body(const int8_t* __restrict__ codes, int64_t ldc,
                                                const float* __restrict__ l1, const int32_t* __restrict__ kmaxv,
                                                int64_t n, int64_t d, float fm, float n_div, int accumulate,
                                                float* __restrict__ est, const float* __restrict__ q, int64_t ldq) {
    __shared__ float tabn[kMeanClients][256];     // indexed by the raw code byte, sign included
    __shared__ uint32_t s_ovf;
    const int tid = threadIdx.x;
    const int lane = tid & (kWave - 1);
    const int wid = __builtin_amdgcn_readfirstlane(tid / kWave);
    const int64_t i0 = ((int64_t)blockIdx.x * kCodesMeanThreads + tid) * kMeanCpt;
    const bool full = ALL || (VEC && i0 + kMeanCpt <= d);
    float e[kMeanCpt];
#pragma unroll
    for (int k = 0; k < kMeanCpt; ++k) e[k] = (accumulate && i0 + k < d) ? est[i0 + k] : 0.0f;
    // With q: does any client overflow its codes?  (n kmax words per workgroup, L2-served.)
    // Then the whole launch takes the mixed loop below, which reads those clients from q;
    // the common case keeps the straight-line loop untouched (no per-group test in it).
    bool any = false;
    if (q) {
        if (tid == 0) s_ovf = 0u;
        __syncthreads();
        bool a = false;
        for (int64_t j = tid; j < n; j += kCodesMeanThreads) a = a || kmaxv[j] > 127;
        if (a) s_ovf = 1u;
        __syncthreads();
        any = s_ovf != 0u;
    }
    const int64_t groups = n / kMeanClients;
    if (any) {
        for (int64_t j0 = 0; j0 < n; j0 += kMeanClients) {
            const int nb = (int)min((int64_t)kMeanClients, n - j0);
            const uint32_t ovf = mean_ovf_mask(kmaxv, j0, nb);
            __syncthreads();
            mean_build_tables<BIASED>(tabn, l1, kmaxv, j0, nb, wid, lane, fm, n_div);
            __syncthreads();
            mean_add_mixed(e, codes, ldc, q, ldq, tabn, ovf, j0, nb, i0, d, n_div);
        }
    } else {
    // full groups of kMeanClients: straight-line, unconditional loads (the prefetch of the
    // group after the last one is clamped to a valid row and never used), so the waits
    // before each batch cover that batch only
    const int8_t* cbase = codes + (full ? i0 : 0);
    uint2 wa[kMeanUnroll], wb[kMeanUnroll];
    if (VEC && groups > 0) mean_load_batch(wa, cbase, ldc);
    for (int64_t g = 0; g < groups; ++g) {
        const int64_t j0 = g * kMeanClients;
        __syncthreads();                            // previous group's tables no longer read
        mean_build_tables<BIASED>(tabn, l1, kmaxv, j0, kMeanClients, wid, lane, fm, n_div);
        __syncthreads();
        if (VEC) {
            mean_load_batch(wb, cbase + (j0 + kMeanUnroll) * ldc, ldc);
            if (full) mean_add_batch(e, wa, tabn, 0);
            const int64_t jn = (j0 + kMeanClients + kMeanUnroll <= n) ? j0 + kMeanClients : n - kMeanUnroll;
            mean_load_batch(wa, cbase + jn * ldc, ldc);
            if (full) mean_add_batch(e, wb, tabn, kMeanUnroll);
        }
        if (!full) mean_add_bytes(e, codes, ldc, tabn, j0, kMeanClients, i0, d);
    }
    const int64_t jr = groups * kMeanClients;
    const int nr = (int)(n - jr);
    if (nr > 0) {                                   // the last n % kMeanClients clients
        __syncthreads();
        mean_build_tables<BIASED>(tabn, l1, kmaxv, jr, nr, wid, lane, fm, n_div);
        __syncthreads();
        if (full) {
            for (int jj = 0; jj < nr; ++jj) {
                const uint2 w = *reinterpret_cast<const uint2*>(codes + (jr + jj) * ldc + i0);
#pragma unroll
                for (int k = 0; k < 4; ++k) e[k] += tabn[jj][(w.x >> (8 * k)) & 0xFF];
#pragma unroll
                for (int k = 0; k < 4; ++k) e[4 + k] += tabn[jj][(w.y >> (8 * k)) & 0xFF];
            }
        } else {
            mean_add_bytes(e, codes, ldc, tabn, jr, nr, i0, d);
        }
    }
    }
    if (full) {
        *reinterpret_cast<float4*>(est + i0) = make_float4(e[0], e[1], e[2], e[3]);
        *reinterpret_cast<float4*>(est + i0 + 4) = make_float4(e[4], e[5], e[6], e[7]);
    } else {
        for (int k = 0; k < kMeanCpt; ++k)
            if (i0 + k < d) est[i0 + k] = e[k];
    }
}

template <bool VEC, bool ALL = false>
__global__ void __launch_bounds__(kCodesMeanThreads)
codes_mean_kernel(const int8_t* __restrict__ codes, int64_t ldc, const float* __restrict__ l1,
                  const int32_t* __restrict__ kmaxv, int64_t n, int64_t d, float fm, float n_div, int accumulate,
                  float* __restrict__ est, const float* __restrict__ q, int64_t ldq) {
    codes_mean_body<VEC, ALL, false>(codes, ldc, l1, kmaxv, n, d, fm, n_div, accumulate, est, q, ldq);
}

// The biased form's mean (uq_codes_mean_form_f32 with UQ_FORM_BIASED): the same loops over
// tables of L1*RN(k/m).
template <bool VEC, bool ALL = false>
__global__ void __launch_bounds__(kCodesMeanThreads)
codes_mean_biased_kernel(const int8_t* __restrict__ codes, int64_t ldc, const float* __restrict__ l1,
                         const int32_t* __restrict__ kmaxv, int64_t n, int64_t d, float fm, float n_div,
                         int accumulate, float* __restrict__ est, const float* __restrict__ q, int64_t ldq) {
    codes_mean_body<VEC, ALL, true>(codes, ldc, l1, kmaxv, n, d, fm, n_div, accumulate, est, q, ldq);
}

// ---- 4-bit type codes (the bench pipeline "codes4") ------------------------------------
// uq_type_unbiased_nibbles_ld_f32 writes the type codes of K2 as 4-bit fields (element 2i in
// the low nibble of byte i): the byte code's low nibble, i.e. k for sign >= 0 and 15 - k for
// ~k, exact while k <= kNibMax.  At R <= 2 the counts stay below that for all but extreme
// tails (k <= 2 at R = 1 for |x| < 11 sigma), and a client with kmax > kNibMax is read from q.
// Half the code bytes of K2's write and K3's read: K2 1.69 -> 1.66 ms, K3 0.187 -> 0.148 ms on
// the C2 batch (timing probe tools/exp/variants.py, profiles/r5ai_nibble_codes_probe.jsonl).
constexpr int kNibMax = 7;
constexpr int64_t kNibAlign = kCodesMeanThreads * kMeanCpt;   // d % 4096 == 0: whole mean threads

__device__ __forceinline__ void nib_load_batch(uint32_t (&w)[kMeanUnroll], const uint8_t* cp, int64_t ldn) {
#pragma unroll
    for (int u = 0; u < kMeanUnroll; ++u) w[u] = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(cp + (int64_t)u * ldn));
}

__device__ __forceinline__ void nib_add_batch(float (&e)[kMeanCpt], const uint32_t (&w)[kMeanUnroll],
                                              const float (*tab)[16], int jj) {
#pragma unroll
    for (int u = 0; u < kMeanUnroll; ++u) {
        const float* tb = tab[jj + u];
#pragma unroll
        for (int k = 0; k < kMeanCpt; ++k) e[k] += tb[(w[u] >> (4 * k)) & 0xFu];
    }
}

// tab[jj][c]: nibble c of client j0 + jj = RN(RN(RN(L1*k)/m)/n_div) with k = c (c <= 7) and
// its negation at c = 15 - k (the byte table's values, so est keeps K3c's bits).  All nb
// clients of a chunk at once, entries spread over the workgroup: one round of l1 / kmax loads
// per chunk (per 32-client group, those loads' latency and two barriers were most of K3n).
constexpr int kNibChunk = 1024;                 // clients whose tables sit in LDS at a time (64 KB)
__device__ __forceinline__ void nib_build_tables(float (*tab)[16], const float* __restrict__ l1,
                                                 const int32_t* __restrict__ kmaxv, int64_t j0, int nb, float fm,
                                                 float n_div) {
    for (int e = threadIdx.x; e < nb * 8; e += kCodesMeanThreads) {
        const int jj = e >> 3, k = e & 7;
        const float L = l1[j0 + jj];
        const int km = min(kNibMax, max(0, kmaxv[j0 + jj]));
        if (k <= km) {
            const float v = ((L * (float)k) / fm) / n_div;
            tab[jj][k] = v;
            tab[jj][15 - k] = -v;
        }
    }
}

// K3n: est[i] (+)= q_j[i] / n_div, clients in order, from the 4-bit codes (4 bytes per client
// per thread's 8 columns): the tables of up to kNibChunk clients built once, then the code
// loads in double-buffered batches of kMeanUnroll clients with no barrier between them.
// d % 4096 == 0 (every thread's columns inside d).  Any client with kmax > kNibMax sends the
// launch down the mixed loop: those clients add q[j][i] / n_div (q is required).
__global__ void __launch_bounds__(kCodesMeanThreads)
nibbles_mean_kernel(const uint8_t* __restrict__ nib, int64_t ldn, const float* __restrict__ l1,
                    const int32_t* __restrict__ kmaxv, int64_t n, int64_t d, float fm, float n_div, int accumulate,
                    float* __restrict__ est, const float* __restrict__ q, int64_t ldq) {
    __shared__ float tab[kNibChunk][16];
    __shared__ uint32_t s_ovf;
    const int tid = threadIdx.x;
    const int64_t i0 = ((int64_t)blockIdx.x * kCodesMeanThreads + tid) * kMeanCpt;
    float e[kMeanCpt];
    if (accumulate) {
        const float4 a = *reinterpret_cast<const float4*>(est + i0), b = *reinterpret_cast<const float4*>(est + i0 + 4);
        e[0] = a.x; e[1] = a.y; e[2] = a.z; e[3] = a.w; e[4] = b.x; e[5] = b.y; e[6] = b.z; e[7] = b.w;
    } else {
#pragma unroll
        for (int k = 0; k < kMeanCpt; ++k) e[k] = 0.0f;
    }
    if (tid == 0) s_ovf = 0u;
    __syncthreads();
    bool a = false;
    for (int64_t j = tid; j < n; j += kCodesMeanThreads) a = a || kmaxv[j] > kNibMax;
    if (a) s_ovf = 1u;
    __syncthreads();
    const bool any = s_ovf != 0u;
    const uint8_t* cbase = nib + i0 / 2;
    for (int64_t c0 = 0; c0 < n; c0 += kNibChunk) {
        const int nc = (int)min((int64_t)kNibChunk, n - c0);
        __syncthreads();                               // the previous chunk's tables no longer read
        nib_build_tables(tab, l1, kmaxv, c0, nc, fm, n_div);
        __syncthreads();
        const int full = any ? 0 : nc / kMeanClients * kMeanClients;
        if (full > 0) {
            uint32_t wa[kMeanUnroll], wb[kMeanUnroll];
            const uint8_t* cb = cbase + c0 * ldn;
            nib_load_batch(wa, cb, ldn);
            for (int g = 0; g < full; g += kMeanClients) {
                nib_load_batch(wb, cb + (int64_t)(g + kMeanUnroll) * ldn, ldn);
                nib_add_batch(e, wa, tab, g);
                // the next group's first batch (clamped to a row inside the chunk when none)
                const int gn = (g + kMeanClients + kMeanUnroll <= nc) ? g + kMeanClients : nc - kMeanUnroll;
                nib_load_batch(wa, cb + (int64_t)gn * ldn, ldn);
                nib_add_batch(e, wb, tab, g + kMeanUnroll);
            }
        }
        for (int jj = full; jj < nc; ++jj) {           // mixed / the chunk's last clients
            const int64_t j = c0 + jj;
            if (kmaxv[j] > kNibMax) {
                const float4 a4 = *reinterpret_cast<const float4*>(q + j * ldq + i0);
                const float4 b4 = *reinterpret_cast<const float4*>(q + j * ldq + i0 + 4);
                const float qq[kMeanCpt] = {a4.x, a4.y, a4.z, a4.w, b4.x, b4.y, b4.z, b4.w};
#pragma unroll
                for (int k = 0; k < kMeanCpt; ++k) e[k] += qq[k] / n_div;
            } else {
                const uint32_t w = *reinterpret_cast<const uint32_t*>(cbase + j * ldn);
#pragma unroll
                for (int k = 0; k < kMeanCpt; ++k) e[k] += tab[jj][(w >> (4 * k)) & 0xFu];
            }
        }
    }
    *reinterpret_cast<float4*>(est + i0) = make_float4(e[0], e[1], e[2], e[3]);
    *reinterpret_cast<float4*>(est + i0 + 4) = make_float4(e[4], e[5], e[6], e[7]);
}

}  // namespace

#endif  // UQ_UNBIASED_KERNELS_H
