// uq_eden.hip — EDEN and the randomized Hadamard transform: the dispatch plan, the workspace
// layouts, the launchers of uq_eden_kernels.h (KE0-KE4) and the C API uq_rht_* / uq_eden_*.
// QUIC-FL's sender and quantizer run their RHT and norm here (rht_layout, rht_norm_front,
// rht_inverse in uq_internal.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstring>

#include "uq_eden_kernels.h"
#include "uq_internal.h"

// uq_test_set_eden_hooks (include/uq_dme.h); each packed entry point loads it once, into its plan
static std::atomic<int> g_eden_hooks{0};

namespace {

// ---- EDEN host helpers ------------------------------------------------------------------
bool eden_tables(int nbits, EdenTables* t) {
    // AS:302-315: centroids (-c reversed, c) as f32; boundaries = midpoints of neighbours
    static const double kPos[2][2] = {{0.7978845608028654, 0.0}, {0.4527800398860679, 1.5104176087114887}};
    std::memset(t, 0, sizeof(*t));
    if (nbits != 1 && nbits != 2) return false;
    const int np = nbits;
    for (int i = 0; i < np; ++i) { t->c[np - 1 - i] = (float)-kPos[np - 1][i]; t->c[np + i] = (float)kPos[np - 1][i]; }
    // the reference forms the midpoints from the f32 tensor elements, in double, then
    // stores them as f32 (torch.Tensor of Python floats)
    for (int i = 0; i + 1 < 2 * np; ++i) t->b[i] = (float)(((double)t->c[i] + (double)t->c[i + 1]) / 2.0);
    t->nb = 2 * np - 1;
    return true;
}

int ilog2_pow2(int64_t D) { return D <= 1 ? 0 : 64 - __builtin_clzll((uint64_t)D - 1); }      // the least p with D <= 2^p

// ---- dispatch plan -------------------------------------------------------------------
// Every decision of a call, made once on the host from (op, n, dim, nbits, norm mode); DESIGN.md
// §4.3 has the table.  The launchers launch what the plan names and the workspace sizes read
// the same function, so the test hooks (uq_test_eden_plan, uq_test_last_eden_plan) report what
// a call really runs.

// torch.norm of few clients: the segmented chains (KE2a-KE2d) instead of KE2's sequential
// ones.  KE2 keeps batches above kSegNormMaxN: it hides its chains behind the reads there,
// while KE2s reads the vectors twice.
constexpr int64_t kSegNormMaxN = 256;
// ... and the dot's (KE4s): its one-wave-per-client form runs 6-19 VALU per step, so the
// segmented form pays for its second read only with few clients.  KE4's time is one client's
// chain whatever n (2.67 ms at D = 2^22: 44 % of a 101-client EDEN call, profiles/r6z_*), KE4s
// costs ~15 us per client of 2^22 (~4 per client of 2^20): they cross near 170 clients.
constexpr int64_t kDotSegMaxN = 128;

struct EdenPass {
    int32_t lo, k, kernel;    // index bits [lo, lo + k) by UQ_EDEN_PASS_*
    uint32_t gx;              // workgroups per client
};
struct EdenPlan {
    int32_t op = 0, p = 0;
    int64_t D = 1;
    bool seg = false;         // the shape takes the segmented norm: the workspace has its region
    int32_t tab_cap = 0;      // ... with this many tables per client
    int32_t norm = UQ_EDEN_NORM_NONE, dot = UQ_EDEN_DOT_NONE;
    int32_t first_bits = 0, npass = 0;
    EdenPass pass[UQ_EDEN_MAX_PASSES] = {};
    bool copy_back = false;   // forward RHT: the last pass wrote the workspace, not out
    bool frac = false;        // a fractional rate: the mask-aware dot kernels / first receiver pass
    bool sender() const { return op == UQ_EDEN_OP_COMPRESS || op == UQ_EDEN_OP_RHT_FORWARD || op == UQ_EDEN_OP_QFL_FRONT; }
    // MODE of the first pass: 1 sender (pad, * diag), 2 EDEN's receiver (centroids), 0 plain
    int mode0() const { return sender() ? 1 : op == UQ_EDEN_OP_DECOMPRESS ? 2 : 0; }
};

EdenPlan eden_plan(int op, int64_t n, int64_t dim, int32_t nbits, int32_t mode) {
    EdenPlan P;
    P.op = op;
    const bool norm_op = op == UQ_EDEN_OP_NORM;
    P.p = ilog2_pow2(dim);
    const int64_t D = P.D = norm_op ? dim : (int64_t)1 << P.p;
    P.seg = n >= 1 && n <= kSegNormMaxN && D >= kSegMinD && (D & (D - 1)) == 0;
    P.tab_cap = P.seg ? seg_tab_cap(D) : 0;
    if (n < 1 || dim < 1) return P;
    // a fractional rate takes the rows of 2 bits (never KE2+4, which needs the one boundary at 0
    // for every coordinate), with the mask-aware instances of the dot kernels and of the
    // receiver's first pass
    P.frac = nbits == UQ_EDEN_NBITS_FRAC && (op == UQ_EDEN_OP_COMPRESS || op == UQ_EDEN_OP_DECOMPRESS);
    if (op == UQ_EDEN_OP_COMPRESS && !P.seg && nbits == 1 && D % kNormChunk == 0) {
        // 1 bit, many clients: the norm, the bins and the dot in one read (KE2+4), then KE4 for
        // the clients it flags (a norm that is not positive and finite, an underflowing quotient)
        P.norm = UQ_EDEN_NORM_FUSED;
        P.dot = UQ_EDEN_DOT_FUSED_REDO;
    } else if (op == UQ_EDEN_OP_COMPRESS || op == UQ_EDEN_OP_QFL_FRONT || norm_op) {
        const bool seg = norm_op ? mode == 2 || (mode == 0 && P.seg) : P.seg;
        P.norm = seg ? (P.seg ? UQ_EDEN_NORM_SEGMENTED : UQ_EDEN_NORM_NONE)
                     : D % kNormChunk == 0 ? UQ_EDEN_NORM_CHAINS_WHOLE : UQ_EDEN_NORM_CHAINS_GENERIC;
        if (op == UQ_EDEN_OP_COMPRESS) P.dot = P.seg && n <= kDotSegMaxN ? UQ_EDEN_DOT_SEGMENTED : UQ_EDEN_DOT_ONE_WAVE;
    }
    if (norm_op) return P;
    // The passes of one transform of 2^p elements, low bits first: the first takes up to
    // first_bits (contiguous tiles), every later one up to kFwhtHighBits (2^k rows x kFwhtCols
    // columns).  D = 2^22 (config C4) takes 14 bits, then 8: one pass fewer than 12 + 8 + 2.
    // uq_rht_f32's inverse keeps 12 whatever D: another width would launch other kernels.
    P.first_bits = op != UQ_EDEN_OP_RHT_INVERSE && P.p == kFwhtLow16Bits + kFwhtHighBits ? kFwhtLow16Bits : kFwhtLowBits;
    int lo = 0;
    do {
        EdenPass& s = P.pass[P.npass++];
        const int k = std::min(P.p - lo, lo ? kFwhtHighBits : P.first_bits);
        const bool last = lo + k >= P.p;
        const int m = lo ? 0 : P.mode0();
        const int64_t cols = D >> k;
        // the register-radix kernels for the 16384- and 4096-element low pass and the 256 x 64 high
        // pass, a thread per column for a short pass over >= 1024 workgroups (with fewer, e.g. one client
        // of 2^18, the generic kernel's 2^k x 32 tiles use more of the GPU), else the generic LDS kernel
        auto set = [&](int32_t kernel, int64_t gx) { s = {lo, k, kernel, (uint32_t)gx}; };
        if (lo == 0 && k == kFwhtLow16Bits && !last) set(UQ_EDEN_PASS_LOW16K, cols);
        else if (lo == 0 && k == kFwhtLowBits && (m != 2 || D % 16 == 0)) set(UQ_EDEN_PASS_LOW4096, cols);
        else if (lo > 0 && k == kFwhtHighBits && m == 0 && ((int64_t)1 << lo) % kHighCols == 0)
            set(UQ_EDEN_PASS_HIGH256, cols / kHighCols);
        else if (lo > 0 && k <= 6 && m == 0 && n * (cols / 256) >= 1024) set(UQ_EDEN_PASS_SMALL, (cols + 255) / 256);
        else set(UQ_EDEN_PASS_GENERIC, lo == 0 ? cols : cols / kFwhtCols);
        lo += k;
    } while (lo < P.p && P.npass < UQ_EDEN_MAX_PASSES);      // (four passes reach 2^36: no workspace holds more)
    P.copy_back = op == UQ_EDEN_OP_RHT_FORWARD && P.npass % 2 == 1;
    return P;
}

thread_local EdenPlan t_last_plan[UQ_EDEN_OPS];      // uq_test_last_eden_plan, per op
const EdenPlan& record(const EdenPlan& P) { return t_last_plan[P.op] = P; }

// The packed message form (uq_eden_*_packed_f32) of a plan: which kernel writes, or first reads, the payload rows.
// Fused: KE4 (one wave per client) and KE2+4 with its redo KE4 on the sender, the 4096-element first pass on the
// receiver, at 1 and 2 bits.  Everything else -- the segmented dot, the 16k / generic first passes, the fractional
// rates, and every call under test hook bit 0 -- goes through the u8 bins of the workspace and a converter.
struct PackedPlan {
    int32_t kind = 0, form = UQ_EDEN_PACKED_NONE;
    int64_t P = 0, pitch = 0;
};
bool packed_kind_ok(int32_t kind) { return kind == 1 || kind == 2 || kind == UQ_EDEN_NBITS_FRAC; }
PackedPlan packed_plan(const EdenPlan& E, int32_t kind, int hooks) {
    PackedPlan k;
    k.kind = kind;
    k.P = (E.D + 31) / 32;
    k.pitch = kind == 1 ? k.P : 2 * k.P;
    const bool fused = E.op == UQ_EDEN_OP_COMPRESS ? E.dot == UQ_EDEN_DOT_ONE_WAVE || E.dot == UQ_EDEN_DOT_FUSED_REDO
                                                   : E.npass > 0 && E.pass[0].kernel == UQ_EDEN_PASS_LOW4096;
    k.form = fused && kind != UQ_EDEN_NBITS_FRAC && !(hooks & 1) ? UQ_EDEN_PACKED_FUSED : UQ_EDEN_PACKED_CONVERTER;
    return k;
}
thread_local PackedPlan t_last_packed[2];             // uq_test_last_eden_packed_plan: compress, decompress

// ---- workspace layouts ---------------------------------------------------------------
// The segmented region's arrays at address r (0: for `total` alone), each on a 256-byte boundary: KE2s uses
// the first seven; KE4s, after it (the norm is done with them), also its thresholds [n][4] and chain ends [n][64].
struct SegRegion {
    double* segsum;
    float *g, *e;
    int32_t *kind, *cnt, *tseg;
    float *tab, *thr4, *acc64;
    size_t total;
};
SegRegion seg_region(uintptr_t r, int64_t n, const EdenPlan& P) {
    const size_t nk = (size_t)n * 8 * (size_t)(P.D / kSegBlock), nc = (size_t)n * (size_t)P.tab_cap;
    const size_t bytes[9] = {nk * sizeof(double), nk * sizeof(float), nk * sizeof(float), nk * sizeof(int32_t),
                             (size_t)n * sizeof(int32_t), nc * sizeof(int32_t), nc * kSegTab * sizeof(float),
                             (size_t)n * 4 * sizeof(float), (size_t)n * 64 * sizeof(float)};
    uintptr_t a[10] = {r};
    for (int i = 0; i < 9; ++i) a[i + 1] = r + up256(a[i] - r + bytes[i]);
    return {(double*)a[0], (float*)a[1], (float*)a[2], (int32_t*)a[3], (int32_t*)a[4], (int32_t*)a[5], (float*)a[6],
            (float*)a[7], (float*)a[8], (size_t)(a[9] - r)};
}

struct EdenLayout { size_t vec_off, nrm_off, bins_off, scale_off, redo_off, seg_off, total; };
EdenLayout eden_layout(int64_t n, const EdenPlan& P) {
    EdenLayout w{};
    w.vec_off = kCtrlBytes;
    w.nrm_off = up256(w.vec_off + (size_t)n * P.D * sizeof(float));
    w.bins_off = up256(w.nrm_off + (size_t)n * sizeof(float));
    w.scale_off = up256(w.bins_off + (size_t)n * P.D);
    w.redo_off = up256(w.scale_off + (size_t)n * sizeof(float));
    w.seg_off = up256(w.redo_off + (size_t)n * sizeof(int32_t));
    w.total = w.seg_off + (P.seg ? seg_region(0, n, P).total : 0);
    return w;
}

// ---- launchers: what the plan names ----------------------------------------------------
// AS:329 torch.norm, the plan's form (v: n rows of P.D; region: the segmented form's)
int launch_norm(const EdenPlan& P, const float* v, int64_t n, char* region, float* nrm, hipStream_t st) {
    const int64_t D = P.D, K = D / kSegBlock;
    if (P.norm != UQ_EDEN_NORM_SEGMENTED) {
        const dim3 grid((unsigned)((n + kNormClients - 1) / kNormClients));
        if (P.norm == UQ_EDEN_NORM_CHAINS_WHOLE)
            hipLaunchKernelGGL(eden_norm_whole_kernel, grid, dim3(kNormThreads), 0, st, v, n, D, nrm);
        else
            hipLaunchKernelGGL(eden_norm_kernel, grid, dim3(kNormThreads), 0, st, v, n, D, nrm);
        return launched("eden_norm_kernel launch");
    }
    const SegRegion s = seg_region((uintptr_t)region, n, P);
    const int cap = P.tab_cap;
    const dim3 grid((unsigned)(K / kSegPerWG), (unsigned)n);
    hipLaunchKernelGGL(eden_segsum_kernel, grid, dim3(256), 0, st, v, D, s.segsum);
    hipLaunchKernelGGL(eden_segscan_kernel<8>, dim3(8u, (unsigned)n), dim3(256), 0, st, s.segsum, K, s.g, s.cnt);
    hipLaunchKernelGGL(eden_segchain_kernel, grid, dim3(256), 0, st, v, D, s.g, s.e, s.kind, s.cnt, s.tseg, cap);
    hipLaunchKernelGGL(eden_segtab_kernel, dim3((unsigned)cap, (unsigned)n), dim3(256), 0, st, v, D, s.g, s.cnt, s.tseg,
                       s.tab, cap);
    hipLaunchKernelGGL(eden_segwalk_kernel, dim3((unsigned)n), dim3(512), 0, st, v, D, s.g, s.e, s.kind, s.tab, nrm, cap);
    return launched("eden segmented norm launch");
}

// f(FRAC) for a plan's rate: the mask-aware instances of the segmented dot's kernels, or the 1- and 2-bit ones
template <class F>
void select_frac(bool frac, F&& f) {
    if (frac) f(Flag<true>{});
    else f(Flag<false>{});
}

// KE4s (few clients): the bins and the dot's 64 chains in segments, in the segmented norm's
// region; the same bits as eden_dotbins_kernel
int launch_eden_dotseg(const EdenPlan& P, const float* v, int64_t n, float sqrtD, const float* nrm, const EdenTables& tab,
                       const EdenMask& m, uint8_t* bins, float* scale, char* region, hipStream_t st) {
    const SegRegion s = seg_region((uintptr_t)region, n, P);
    const int64_t D = P.D, K = D / kEdenTile;
    const int cap = P.tab_cap;
    hipLaunchKernelGGL(eden_thresh_kernel, dim3((unsigned)n), dim3(64), 0, st, nrm, tab, s.thr4);
    select_frac(P.frac, [&](auto F) {
        hipLaunchKernelGGL(eden_dseg_sum_kernel<F()>, dim3((unsigned)K, (unsigned)n), dim3(256), 0, st, v, D, sqrtD, nrm, s.thr4,
                           tab, bins, s.segsum, m);
        hipLaunchKernelGGL(eden_segscan_kernel<64>, dim3(64u, (unsigned)n), dim3(256), 0, st, s.segsum, K, s.g, s.cnt);
        hipLaunchKernelGGL(eden_dseg_chain_kernel<F()>, dim3((unsigned)(K / kDSegTiles), (unsigned)n), dim3(256), 0, st, v, D,
                           sqrtD, nrm, s.thr4, tab, s.g, s.e, s.kind, s.cnt, s.tseg, cap, m);
        hipLaunchKernelGGL(eden_dseg_tab_kernel<F()>, dim3((unsigned)cap, (unsigned)n), dim3(256), 0, st, v, D, sqrtD, nrm,
                           s.thr4, tab, s.g, s.cnt, s.tseg, s.tab, cap, m);
        hipLaunchKernelGGL(eden_dseg_walk_kernel<F()>, dim3(8u, (unsigned)n), dim3(512), 0, st, v, D, sqrtD, nrm, s.thr4, tab,
                           s.g, s.e, s.kind, s.tab, s.acc64, cap, m);
    });
    hipLaunchKernelGGL(eden_dseg_final_kernel, dim3((unsigned)n), dim3(64), 0, st, s.acc64, nrm, scale);
    return launched("eden segmented dot launch");
}

// AS:329-335: the bins and the scale's dot in MKL sdot's order (KE4), scale = f32(nrm * nrm) / dot.  (Ahead of the
// FWHT launches: kernels are emitted in the order they are named, which tools/kernel_table.py's hashes see.)
int launch_eden_dotbins(const float* v, int64_t n, int64_t D, float sqrtD, const float* nrm, const EdenTables& tab,
                        uint8_t* bins, float* scale, hipStream_t st, const int32_t* redo, const EdenMask* frac = nullptr) {
    const dim3 grid((unsigned)((n + kDotWaves - 1) / kDotWaves)), block(64 * kDotWaves);
    if (frac)
        hipLaunchKernelGGL(eden_dotbins_frac_kernel, grid, block, 0, st, v, D, sqrtD, nrm, tab, bins, scale, n, *frac);
    else if (tab.nb == 1)
        hipLaunchKernelGGL(eden_dotbins_kernel<1>, grid, block, 0, st, v, D, sqrtD, nrm, tab, bins, scale, n, redo);
    else
        hipLaunchKernelGGL(eden_dotbins_kernel<3>, grid, block, 0, st, v, D, sqrtD, nrm, tab, bins, scale, n, redo);
    return launched("eden_dotbins_kernel launch");
}

// The run-time (MODE, LAST, RECV_LAST) of a pass, and the bits of a short one, as compile-time constants.  The
// seven triples a transform can have: MODE 1 and 2 on the first pass only, RECV_LAST on a receiver's last.
template <int V>
using Int = std::integral_constant<int, V>;

template <class F>
void select_pass(int mode, bool last, bool recv_last, F&& f) {
    if (mode == 1) last ? f(Int<1>{}, Flag<true>{}, Flag<false>{}) : f(Int<1>{}, Flag<false>{}, Flag<false>{});
    else if (mode == 2) last ? f(Int<2>{}, Flag<true>{}, Flag<true>{}) : f(Int<2>{}, Flag<false>{}, Flag<false>{});
    else if (recv_last) f(Int<0>{}, Flag<true>{}, Flag<true>{});
    else if (last) f(Int<0>{}, Flag<true>{}, Flag<false>{});
    else f(Int<0>{}, Flag<false>{}, Flag<false>{});
}
template <class F>
void select_small_k(int k, F&& f) {
    k == 1 ? f(Int<1>{}) : k == 2 ? f(Int<2>{}) : k == 3 ? f(Int<3>{}) : k == 4 ? f(Int<4>{}) : k == 5 ? f(Int<5>{}) : f(Int<6>{});
}

// the packed instances' launches (defined after the u8 forms')
int launch_low4096_packed(const FwhtArgs& a, int kind, bool last, dim3 grid, hipStream_t st);
int launch_normdot1_packed(const float* rot, int64_t n, int64_t D, float sqrtD, const EdenTables& tab, float* nrm,
                           uint32_t* payload, float* scale, int32_t* redo, hipStream_t st);
int launch_eden_dotbins_packed(const float* v, int64_t n, int64_t D, float sqrtD, const float* nrm, const EdenTables& tab,
                               uint32_t* payload, float* scale, hipStream_t st, const int32_t* redo);

FwhtArgs fwht_args(const void* in, const int8_t* signs, const int32_t* sign_row, const uint32_t* sbits,
                   const float* scale, int64_t D, int64_t dim, const EdenTables& tab) {
    const float sqrtD = (float)std::sqrt((double)D);         // np.sqrt(d) -> f32 operand
    return FwhtArgs{in, /*out (set per pass)*/ nullptr, signs, sign_row, sbits, scale, D, dim, sqrtD, tab};
}

// Runs the plan's FWHT passes; the first reads a.in.  Receivers (EDEN's, and the inverse of plain
// vectors): in place in `buf`, the last pass into `out`.  Senders: the passes alternate between
// `buf` and `out` (out == buf: in place; the forward RHT passes its output so that a two-pass
// transform needs no copy); *result = the buffer holding the result.
int launch_passes(const EdenPlan& P, FwhtArgs a, int64_t n, float* buf, float* out, hipStream_t st, float** result = nullptr,
                  const EdenMask* frac = nullptr, int packed_kind = 0) {
    float* dst = nullptr;
    for (int i = 0; i < P.npass; ++i) {
        const EdenPass& s = P.pass[i];
        const bool last = i + 1 == P.npass;
        if (i) a.in = dst;
        a.out = dst = P.sender() ? (i % 2 ? out : buf) : (last ? out : buf);
        const dim3 grid(s.gx, (unsigned)n);
        if (i == 0 && packed_kind) {                     // a.in: payload rows (the plan's packed form is the fused one)
            if (const int rc = launch_low4096_packed(a, packed_kind, last, grid, st)) return rc;
            continue;
        }
        if (i == 0 && frac && P.mode0() == 2) {
            // a fractional receiver's first pass: the plan's kernel for MODE 2, its MODE 3 instance
            // (the table of each bin by the mask rows); never a later pass's kernel
            if (s.kernel == UQ_EDEN_PASS_LOW16K) hipLaunchKernelGGL(fwht_low16k_frac_kernel, grid, dim3(1024), 0, st, a, *frac);
            else if (s.kernel == UQ_EDEN_PASS_LOW4096 && last)
                hipLaunchKernelGGL((fwht_low4096_frac_kernel<true, true>), grid, dim3(256), 0, st, a, *frac);
            else if (s.kernel == UQ_EDEN_PASS_LOW4096)
                hipLaunchKernelGGL((fwht_low4096_frac_kernel<false, false>), grid, dim3(256), 0, st, a, *frac);
            else if (last) hipLaunchKernelGGL((fwht_pass_frac_kernel<true, true>), grid, dim3(kFwhtT), 0, st, a, s.lo, s.k, *frac);
            else hipLaunchKernelGGL((fwht_pass_frac_kernel<false, false>), grid, dim3(kFwhtT), 0, st, a, s.lo, s.k, *frac);
            if (const int rc = launched("fwht_pass_frac_kernel launch")) return rc;
            continue;
        }
        select_pass(i ? 0 : P.mode0(), last, last && !P.sender(), [&](auto M, auto L, auto R) {
            constexpr bool l = decltype(L)::value, r = decltype(R)::value;
            switch (s.kernel) {
                case UQ_EDEN_PASS_LOW16K: hipLaunchKernelGGL((fwht_low16k_kernel<M()>), grid, dim3(1024), 0, st, a); break;
                case UQ_EDEN_PASS_LOW4096: hipLaunchKernelGGL((fwht_low4096_kernel<M(), l, r>), grid, dim3(256), 0, st, a); break;
                case UQ_EDEN_PASS_HIGH256: hipLaunchKernelGGL((fwht_high256_kernel<l, r>), grid, dim3(kHighT), 0, st, a, s.lo); break;
                case UQ_EDEN_PASS_SMALL:
                    select_small_k(s.k, [&](auto K) {
                        hipLaunchKernelGGL((fwht_small_kernel<K(), l, r>), grid, dim3(256), 0, st, a, s.lo);
                    });
                    break;
                default: hipLaunchKernelGGL((fwht_pass_kernel<M(), l, r>), grid, dim3(kFwhtT), 0, st, a, s.lo, s.k);
            }
        });
        if (const int rc = launched("fwht_pass_kernel launch")) return rc;
    }
    if (result) *result = dst;
    return UQ_OK;
}

// A uq_eden_* call or QUIC-FL's front: the arguments they share, then what eden_call derives.
struct EdenCall {
    int64_t n, dim;
    int32_t nbits;
    const int8_t* signs;
    const int32_t* sign_row;
    const uint32_t* sbits;
    void* ws;
    size_t ws_bytes;
    void* stream;
    EdenTables tab;
    EdenPlan P;
    EdenLayout w;
    bool frac = false;        // the _frac entry points: the 2-bit tables, the table per coordinate by `mask`
    EdenMask mask{};
    char* at(size_t off) const { return (char*)ws + off; }
};

// The sender up to the norms: RHT (AS:123-141) in the workspace's vector buffer (*rot), then
// torch.norm (AS:329) in the plan's form; the fused form's norm comes with its dot, from the
// caller.  (MODE 1 reads no table: every sender pass gets an empty one.)
int eden_front(const EdenCall& c, const float* x, float** rot) {
    float* vec = (float*)c.at(c.w.vec_off);
    const FwhtArgs a = fwht_args(x, c.signs, c.sign_row, c.sbits, nullptr, c.P.D, c.dim, EdenTables{});
    const int rc = launch_passes(c.P, a, c.n, vec, vec, (hipStream_t)c.stream, rot);
    if (rc || c.P.norm == UQ_EDEN_NORM_FUSED) return rc;
    return launch_norm(c.P, *rot, c.n, c.at(c.w.seg_off), (float*)c.at(c.w.nrm_off), (hipStream_t)c.stream);
}

// The uq_eden_* entry points' checks, in their order; then the plan of `op`, the layout and body().
template <class F>
int eden_call(EdenCall& c, int op, bool null_ptr, F&& body) {
    t_last_plan[op] = EdenPlan{};
    t_last_packed[op == UQ_EDEN_OP_DECOMPRESS] = PackedPlan{};
    if (c.n < 0 || c.dim < 0) return fail(UQ_E_INVALID, "n and dim must be >= 0");
    if (c.n > 65535) return fail(UQ_E_INVALID, "at most 65535 clients per call");
    if (c.dim > ((int64_t)1 << 28)) return fail(UQ_E_INVALID, "dim must be <= 2^28");
    if (!eden_tables(c.nbits, &c.tab)) return fail(UQ_E_INVALID, "EDEN nbits must be 1 or 2 (the reference's tables)");
    if (c.n > 0 && c.dim > 0 && !c.signs) return fail(UQ_E_INVALID, "null signs");
    if (c.n > 0 && c.dim > 0 && c.frac && !c.mask.bits) return fail(UQ_E_INVALID, "null mask_bits");
    if (c.n == 0 || c.dim == 0) return UQ_OK;
    if (null_ptr) return fail(UQ_E_INVALID, "null pointer");
    c.P = eden_plan(op, c.n, c.dim, c.frac ? UQ_EDEN_NBITS_FRAC : c.nbits, 0);
    c.w = eden_layout(c.n, c.P);
    if (!c.ws || c.ws_bytes < c.w.total) return fail(UQ_E_WORKSPACE, "workspace too small");
    return body();
}

// EdenSender.compress: the front, then the bins and the scale's dot in the plan's form (AS:329-335)
// (payload set: the plan's packed form is the fused one, and the kernels that write bins write payload rows)
int eden_compress(const EdenCall& c, const float* x, uint8_t* bins, float* scale, uint32_t* payload = nullptr) {
    const EdenPlan& P = record(c.P);
    hipStream_t st = (hipStream_t)c.stream;
    float* rot = nullptr;
    int rc = eden_front(c, x, &rot);
    if (rc) return rc;
    float* nrm = (float*)c.at(c.w.nrm_off);
    const float sqrtD = (float)std::sqrt((double)P.D);
    if (P.dot == UQ_EDEN_DOT_SEGMENTED)
        return launch_eden_dotseg(P, rot, c.n, sqrtD, nrm, c.tab, c.mask, bins, scale, c.at(c.w.seg_off), st);
    int32_t* redo = nullptr;
    if (P.dot == UQ_EDEN_DOT_FUSED_REDO) {
        redo = (int32_t*)c.at(c.w.redo_off);
        if (payload) {
            if ((rc = launch_normdot1_packed(rot, c.n, P.D, sqrtD, c.tab, nrm, payload, scale, redo, st))) return rc;
            return launch_eden_dotbins_packed(rot, c.n, P.D, sqrtD, nrm, c.tab, payload, scale, st, redo);
        }
        hipLaunchKernelGGL(eden_normdot1_kernel, dim3((unsigned)((c.n + kNormClients - 1) / kNormClients)), dim3(kNDThreads),
                           0, st, rot, c.n, P.D, sqrtD, c.tab, nrm, bins, scale, redo);
        if ((rc = launched("eden_normdot1_kernel launch"))) return rc;
    }
    if (payload) return launch_eden_dotbins_packed(rot, c.n, P.D, sqrtD, nrm, c.tab, payload, scale, st, redo);
    return launch_eden_dotbins(rot, c.n, P.D, sqrtD, nrm, c.tab, bins, scale, st, redo, P.frac ? &c.mask : nullptr);
}

// EdenReceiver.decompress (AS:378-413)
// (packed_kind 1 or 2: `bins` are payload rows, read by the packed instance of the first pass)
int eden_decompress(const EdenCall& c, const void* bins, const float* scale, float* out, int packed_kind = 0) {
    const FwhtArgs a = fwht_args(bins, c.signs, c.sign_row, c.sbits, scale, c.P.D, c.dim, c.tab);
    return launch_passes(record(c.P), a, c.n, (float*)c.at(c.w.vec_off), out, (hipStream_t)c.stream, nullptr,
                         c.P.frac ? &c.mask : nullptr, packed_kind);
}

// The _frac entry points' call: the 2-bit tables, the 1-bit centroids beside the mask rows
EdenCall frac_call(int64_t n, int64_t dim, const int8_t* signs, const int32_t* sign_row, const uint32_t* sign_bits,
                   const uint32_t* mask_bits, const int32_t* mask_row, void* ws, size_t ws_bytes, void* stream) {
    EdenCall c{n, dim, 2, signs, sign_row, sign_bits, ws, ws_bytes, stream};
    EdenTables one;
    eden_tables(1, &one);
    c.frac = true;
    c.mask = EdenMask{mask_bits, mask_row, one.c[0], one.c[1]};
    return c;
}

// compress then decompress on the workspace's bins (uq_eden_f32_sb and its fractional form)
int eden_fused(EdenCall& c, const float* x, float* out, float* scale_out) {
    t_last_plan[UQ_EDEN_OP_DECOMPRESS] = EdenPlan{};
    return eden_call(c, UQ_EDEN_OP_COMPRESS, !x, [&] {
        uint8_t* bins = (uint8_t*)c.at(c.w.bins_off);
        float* scale = scale_out ? scale_out : (float*)c.at(c.w.scale_off);
        const int rc = eden_compress(c, x, bins, scale);
        if (rc) return rc;
        if (!out) return fail(UQ_E_INVALID, "null pointer");       // (the receiver's own check, in its place after the sender)
        c.P = eden_plan(UQ_EDEN_OP_DECOMPRESS, c.n, c.dim, c.frac ? UQ_EDEN_NBITS_FRAC : c.nbits, 0);
        return eden_decompress(c, bins, scale, out);
    });
}

int export_plan(const EdenPlan& P, int64_t* out, int32_t cap) {
    if (!out || cap < 0) return fail(UQ_E_INVALID, "null plan output");
    int64_t f[UQ_EDEN_PLAN_FIELDS] = {P.D, P.p, P.norm, P.dot, P.first_bits, P.npass};
    for (int i = 0; i < UQ_EDEN_MAX_PASSES; ++i) {
        const EdenPass& s = P.pass[i];
        const int64_t v[4] = {s.lo, s.k, s.kernel, s.gx};
        std::copy(v, v + 4, f + 6 + 4 * i);
    }
    f[22] = P.copy_back;
    f[23] = P.tab_cap;
    f[24] = P.frac;
    std::copy(f, f + std::min<int32_t>(cap, UQ_EDEN_PLAN_FIELDS), out);
    return UQ_OK;
}

// ---- the packed message form -----------------------------------------------------------
int launch_low4096_packed(const FwhtArgs& a, int kind, bool last, dim3 grid, hipStream_t st) {
    if (kind == 1 && last) hipLaunchKernelGGL((fwht_low4096_packed_kernel<4, true, true>), grid, dim3(256), 0, st, a);
    else if (kind == 1) hipLaunchKernelGGL((fwht_low4096_packed_kernel<4, false, false>), grid, dim3(256), 0, st, a);
    else if (last) hipLaunchKernelGGL((fwht_low4096_packed_kernel<5, true, true>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((fwht_low4096_packed_kernel<5, false, false>), grid, dim3(256), 0, st, a);
    return launched("fwht_low4096_packed_kernel launch");
}

int launch_normdot1_packed(const float* rot, int64_t n, int64_t D, float sqrtD, const EdenTables& tab, float* nrm,
                           uint32_t* payload, float* scale, int32_t* redo, hipStream_t st) {
    hipLaunchKernelGGL(eden_normdot1_packed_kernel, dim3((unsigned)((n + kNormClients - 1) / kNormClients)), dim3(kNDThreads), 0,
                       st, rot, n, D, sqrtD, tab, nrm, payload, scale, redo);
    return launched("eden_normdot1_packed_kernel launch");
}

int launch_eden_dotbins_packed(const float* v, int64_t n, int64_t D, float sqrtD, const float* nrm, const EdenTables& tab,
                               uint32_t* payload, float* scale, hipStream_t st, const int32_t* redo) {
    const dim3 grid((unsigned)((n + kDotWaves - 1) / kDotWaves)), block(64 * kDotWaves);
    if (tab.nb == 1)
        hipLaunchKernelGGL(eden_dotbins_packed_kernel<1>, grid, block, 0, st, v, D, sqrtD, nrm, tab, payload, scale, n, redo);
    else
        hipLaunchKernelGGL(eden_dotbins_packed_kernel<3>, grid, block, 0, st, v, D, sqrtD, nrm, tab, payload, scale, n, redo);
    return launched("eden_dotbins_packed_kernel launch");
}

template <class F>
void select_kind(int kind, F&& f) {
    kind == 1 ? f(Int<1>{}) : kind == 2 ? f(Int<2>{}) : f(Int<3>{});
}

int launch_payload_bits(int64_t n, int64_t D, int kind, const PackRows& r, int64_t* payload_bits, hipStream_t st) {
    if (!payload_bits) return UQ_OK;
    hipLaunchKernelGGL(eden_payload_bits_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, D,
                       kind == UQ_EDEN_NBITS_FRAC ? 3 : kind, r, payload_bits);
    return launched("eden_payload_bits_kernel launch");
}

int launch_pack(const uint8_t* bins, int64_t n, int64_t D, int kind, const PackRows& r, uint32_t* payload,
                int64_t* payload_bits, hipStream_t st) {
    const int64_t P = (D + 31) / 32, pitch = kind == 1 ? P : 2 * P;
    select_kind(kind, [&](auto K) {
        hipLaunchKernelGGL(eden_pack_bins_kernel<K()>, dim3((unsigned)((pitch + 255) / 256), (unsigned)n), dim3(256), 0, st, bins,
                           D, r, payload);
    });
    if (const int rc = launched("eden_pack_bins_kernel launch")) return rc;
    return launch_payload_bits(n, D, kind, r, payload_bits, st);
}

int launch_unpack(const uint32_t* payload, int64_t n, int64_t D, int kind, const PackRows& r, uint8_t* bins, hipStream_t st) {
    const int64_t P = (D + 31) / 32;
    select_kind(kind, [&](auto K) {
        hipLaunchKernelGGL(eden_unpack_bins_kernel<K()>, dim3((unsigned)((P + 255) / 256), (unsigned)n), dim3(256), 0, st, payload,
                           D, r, bins);
    });
    return launched("eden_unpack_bins_kernel launch");
}

// the converters' checks, in their order; then body()
template <class F>
int pack_call(int64_t n, int64_t D, int32_t kind, const PackRows& r, bool null_ptr, F&& body) {
    if (!packed_kind_ok(kind)) return fail(UQ_E_INVALID, "kind must be 1, 2 or UQ_EDEN_NBITS_FRAC");
    if (n < 0 || D < 0) return fail(UQ_E_INVALID, "n and D must be >= 0");
    if (n > 65535) return fail(UQ_E_INVALID, "at most 65535 clients per call");
    if (D > ((int64_t)1 << 28)) return fail(UQ_E_INVALID, "D must be <= 2^28");
    if (n == 0 || D == 0) return UQ_OK;
    if (null_ptr) return fail(UQ_E_INVALID, "null pointer");
    if (kind == UQ_EDEN_NBITS_FRAC && (!r.mask || !r.ranks)) return fail(UQ_E_INVALID, "null mask_bits or mask_ranks");
    return body();
}

// The packed entry points' call: the integer rates' or the fractional one (frac_call), and the rank rows' check
EdenCall packed_call(int64_t n, int64_t dim, int32_t kind, const int8_t* signs, const int32_t* sign_row,
                     const uint32_t* sign_bits, const uint32_t* mask_bits, const int32_t* mask_row, void* ws, size_t ws_bytes,
                     void* stream) {
    if (kind == UQ_EDEN_NBITS_FRAC) return frac_call(n, dim, signs, sign_row, sign_bits, mask_bits, mask_row, ws, ws_bytes, stream);
    return EdenCall{n, dim, kind, signs, sign_row, sign_bits, ws, ws_bytes, stream};
}

int export_packed(const PackedPlan& k, int64_t* out, int32_t cap) {
    if (!out || cap < 0) return fail(UQ_E_INVALID, "null plan output");
    const int64_t f[UQ_EDEN_PACKED_PLAN_FIELDS] = {k.kind, k.form, k.P, k.pitch};
    std::copy(f, f + std::min<int32_t>(cap, UQ_EDEN_PACKED_PLAN_FIELDS), out);
    return UQ_OK;
}

// ---- the receiver's coordinate drop (AS:413-423) -------------------------------------------
thread_local int32_t t_last_drop_form = UQ_EDEN_DROP_NONE;      // uq_test_last_eden_drop_form

// EdenReceiver.decompress with dropped coordinates, the vector form: KE5d writes the rotated vector
// (0 at a dropped coordinate, else the centroid divided by 1 - pdrop: `cents`, host floats, the
// kind's own table -- 2 entries at 1 bit, 4 else -- then the 1-bit table's two at a fractional rate)
// into the workspace's vector buffer; the inverse transform's plain passes and the receiver's last
// pass (diagonal, scale, [:dim]) follow, as QUIC-FL's receiver runs them.
int eden_decompress_drop(EdenCall& c, int32_t kind, const float* cents, const uint8_t* bins, const float* scale,
                         const uint32_t* drop_bits, float* out) {
    for (int i = 0; i < (kind == 1 ? 2 : 4); ++i) c.tab.c[i] = cents[i];
    if (c.frac) {
        c.mask.lo0 = cents[4];
        c.mask.lo1 = cents[5];
    }
    hipStream_t st = (hipStream_t)c.stream;
    const int64_t D = c.P.D;
    float* vec = (float*)c.at(c.w.vec_off);
    const dim3 grid((unsigned)((D + 255) / 256), (unsigned)c.n);
    if (c.frac) hipLaunchKernelGGL(eden_drop_vec_kernel<true>, grid, dim3(256), 0, st, bins, D, c.tab, c.mask, drop_bits, vec);
    else hipLaunchKernelGGL(eden_drop_vec_kernel<false>, grid, dim3(256), 0, st, bins, D, c.tab, c.mask, drop_bits, vec);
    if (const int rc = launched("eden_drop_vec_kernel launch")) return rc;
    const EdenPlan P = eden_plan(UQ_EDEN_OP_QFL_INVERSE, c.n, D, 0, 0);
    t_last_plan[UQ_EDEN_OP_DECOMPRESS] = P;              // the passes that ran, under the receiver's hook
    t_last_drop_form = UQ_EDEN_DROP_VECTOR;
    return launch_passes(P, fwht_args(vec, c.signs, c.sign_row, c.sbits, scale, D, c.dim, EdenTables{}), c.n, vec, out, st);
}

}  // namespace

// ---- what QUIC-FL's sender and quantizer run here (uq_internal.h) -------------------------
RhtLayout uq_internal::rht_layout(int64_t n, int64_t dim) {
    const EdenPlan P = eden_plan(UQ_EDEN_OP_QFL_FRONT, n, dim, 0, 0);
    const EdenLayout w = eden_layout(n, P);
    return RhtLayout{w.nrm_off, w.total, P.D};
}

int uq_internal::rht_norm_front(const float* x, int64_t n, int64_t dim, const int8_t* signs, const int32_t* sign_row,
                                char* wsb, float** rot, hipStream_t st) {
    EdenCall c{n, dim, 0, signs, sign_row, nullptr, wsb, 0, st};
    c.P = record(eden_plan(UQ_EDEN_OP_QFL_FRONT, n, dim, 0, 0));
    c.w = eden_layout(n, c.P);
    return eden_front(c, x, rot);
}

// AS:533-535: H, then * diag, [:dim]; D = 2^22 as 14 + 8 bits
int uq_internal::rht_inverse(float* rot, float* out, int64_t n, int64_t D, int64_t dim, const int8_t* signs,
                             const int32_t* sign_row, hipStream_t st) {
    const EdenPlan& P = record(eden_plan(UQ_EDEN_OP_QFL_INVERSE, n, D, 0, 0));
    return launch_passes(P, fwht_args(rot, signs, sign_row, nullptr, nullptr, D, dim, EdenTables{}), n, rot, out, st);
}

// AS:123-141 of rows that are a power of two long: QUIC-FL's front without its norm
int uq_internal::rht_forward_rows(const float* x, float* buf, float* out, int64_t n, int64_t D, const int8_t* signs,
                                  const int32_t* sign_row, float** result, hipStream_t st) {
    const EdenPlan& P = record(eden_plan(UQ_EDEN_OP_QFL_FRONT, n, D, 0, 0));
    return launch_passes(P, fwht_args(x, signs, sign_row, nullptr, nullptr, D, D, EdenTables{}), n, buf, out, st, result);
}

extern "C" {

int uq_test_eden_plan(int32_t op, int64_t n, int64_t dim, int32_t nbits, int32_t mode, int64_t* plan_out, int32_t cap) {
    if (op < 0 || op >= UQ_EDEN_OPS) return fail(UQ_E_INVALID, "op must be one of UQ_EDEN_OP_*");
    if (n < 0 || dim < 0) return fail(UQ_E_INVALID, "n and dim must be >= 0");
    if (mode < 0 || mode > 2) return fail(UQ_E_INVALID, "mode must be 0 (auto), 1 (chains) or 2 (segmented)");
    return export_plan(eden_plan(op, n, dim, nbits, mode), plan_out, cap);
}

int uq_test_last_eden_plan(int32_t op, int64_t* plan_out, int32_t cap) {
    if (op < 0 || op >= UQ_EDEN_OPS) return fail(UQ_E_INVALID, "op must be one of UQ_EDEN_OP_*");
    return export_plan(t_last_plan[op], plan_out, cap);
}

// ---- EDEN + RHT ------------------------------------------------------------------------
int uq_rht_signs(const int32_t* seeds, int64_t rows, int64_t D, int8_t* signs, void* stream) {
    if (rows < 0 || D < 0) return fail(UQ_E_INVALID, "rows and D must be >= 0");
    if (rows == 0 || D == 0) return UQ_OK;
    if (rows > 65535) return fail(UQ_E_INVALID, "at most 65535 rows per call");
    if (!seeds || !signs) return fail(UQ_E_INVALID, "null pointer");
    hipLaunchKernelGGL(rht_signs_kernel, dim3((unsigned)rows), dim3(640), 0, (hipStream_t)stream, seeds, D, signs);
    return launched("rht_signs_kernel launch");
}

int uq_rht_f32(const float* x, float* out, int64_t n, int64_t dim, int32_t inverse, const int8_t* signs,
               const int32_t* sign_row, void* ws, size_t ws_bytes, void* stream) {
    const int op = inverse ? UQ_EDEN_OP_RHT_INVERSE : UQ_EDEN_OP_RHT_FORWARD;
    t_last_plan[op] = EdenPlan{};
    if (n < 0 || dim < 0) return fail(UQ_E_INVALID, "n and dim must be >= 0");
    if (n > 65535) return fail(UQ_E_INVALID, "at most 65535 clients per call");
    if (n == 0 || dim == 0) return UQ_OK;
    if (!x || !out || !signs) return fail(UQ_E_INVALID, "null pointer");
    const EdenPlan P = eden_plan(op, n, dim, 0, 0);
    const EdenLayout w = eden_layout(n, P);
    if (inverse && dim != P.D) return fail(UQ_E_INVALID, "inverse RHT input length must be a power of two");
    // (the transform uses the vector region only: no norm, so no segmented-norm region past seg_off)
    if (!ws || ws_bytes < w.seg_off) return fail(UQ_E_WORKSPACE, "workspace too small");
    // forward (AS:123-141): pad, * diag, H; inverse (AS:146-153): H, then * diag, the receiver's last pass with no scale
    const FwhtArgs a = fwht_args(x, signs, sign_row, nullptr, nullptr, P.D, dim, EdenTables{});
    hipStream_t st = (hipStream_t)stream;
    float* buf = (float*)((char*)ws + w.vec_off);
    const int rc = launch_passes(record(P), a, n, buf, out, st);
    if (rc || !P.copy_back) return rc;
    return hip_check(hipMemcpyAsync(out, buf, (size_t)n * P.D * sizeof(float), hipMemcpyDeviceToDevice, st), "copy rht");
}

int uq_eden_workspace_bytes(int64_t n, int64_t dim, size_t* bytes_out) {
    if (!bytes_out) return fail(UQ_E_INVALID, "null bytes_out");
    if (n < 0 || dim < 0) return fail(UQ_E_INVALID, "n and dim must be >= 0");
    *bytes_out = eden_layout(n, eden_plan(UQ_EDEN_OP_COMPRESS, n, dim, 1, 0)).total;
    return UQ_OK;
}

int uq_eden_norm_workspace_bytes(int64_t n, int64_t D, size_t* bytes_out) {
    if (!bytes_out) return fail(UQ_E_INVALID, "null bytes_out");
    if (n < 0 || D < 0) return fail(UQ_E_INVALID, "n and D must be >= 0");
    const EdenPlan P = eden_plan(UQ_EDEN_OP_NORM, n, D, 0, 0);
    *bytes_out = P.seg ? seg_region(0, n, P).total : 0;
    return UQ_OK;
}

int uq_eden_norm_f32(const float* v, int64_t n, int64_t D, int32_t mode, float* nrm, void* ws, size_t ws_bytes,
                     void* stream) {
    t_last_plan[UQ_EDEN_OP_NORM] = EdenPlan{};
    if (n < 0 || D < 0) return fail(UQ_E_INVALID, "n and D must be >= 0");
    if (n > 65535) return fail(UQ_E_INVALID, "at most 65535 clients per call");
    if (mode < 0 || mode > 2) return fail(UQ_E_INVALID, "mode must be 0 (auto), 1 (chains) or 2 (segmented)");
    if (n == 0) return UQ_OK;
    if (!v || !nrm) return fail(UQ_E_INVALID, "null pointer");
    const EdenPlan P = eden_plan(UQ_EDEN_OP_NORM, n, D, 0, mode);
    if (mode == 2 && !P.seg) return fail(UQ_E_INVALID, "segmented norm: 1 <= n <= 256 and D a power of two >= 16384");
    if (D == 0) return hip_check(hipMemsetAsync(nrm, 0, (size_t)n * sizeof(float), (hipStream_t)stream), "norm fill");
    if (P.norm == UQ_EDEN_NORM_SEGMENTED && (!ws || ws_bytes < seg_region(0, n, P).total))
        return fail(UQ_E_WORKSPACE, "workspace too small");
    return launch_norm(record(P), v, n, (char*)ws, nrm, (hipStream_t)stream);
}

int uq_rht_sign_bits(const int8_t* signs, int64_t rows, int64_t D, uint32_t* bits, void* stream) {
    if (rows < 0 || D < 0) return fail(UQ_E_INVALID, "rows and D must be >= 0");
    if (rows == 0 || D == 0) return UQ_OK;
    if (!signs || !bits) return fail(UQ_E_INVALID, "null pointer");
    const int64_t words = rows * ((D + 31) / 32);
    hipLaunchKernelGGL(rht_sign_bits_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       signs, rows, D, bits);
    return launched("rht_sign_bits_kernel launch");
}

int uq_eden_compress_f32_sb(const float* x, int64_t n, int64_t dim, int32_t nbits, const int8_t* signs,
                            const int32_t* sign_row, const uint32_t* sign_bits, uint8_t* bins, float* scale, void* ws,
                            size_t ws_bytes, void* stream) {
    EdenCall c{n, dim, nbits, signs, sign_row, sign_bits, ws, ws_bytes, stream};
    return eden_call(c, UQ_EDEN_OP_COMPRESS, !x || !bins || !scale, [&] { return eden_compress(c, x, bins, scale); });
}

int uq_eden_decompress_f32_sb(const uint8_t* bins, const float* scale, int64_t n, int64_t dim, int32_t nbits,
                              const int8_t* signs, const int32_t* sign_row, const uint32_t* sign_bits, float* out,
                              void* ws, size_t ws_bytes, void* stream) {
    EdenCall c{n, dim, nbits, signs, sign_row, sign_bits, ws, ws_bytes, stream};
    return eden_call(c, UQ_EDEN_OP_DECOMPRESS, !bins || !scale || !out, [&] { return eden_decompress(c, bins, scale, out); });
}

int uq_eden_f32_sb(const float* x, float* out, int64_t n, int64_t dim, int32_t nbits, const int8_t* signs,
                   const int32_t* sign_row, const uint32_t* sign_bits, float* scale_out, void* ws, size_t ws_bytes,
                   void* stream) {
    // compress (RHT, norm, bins + the MKL-order dot) then decompress: the receiver's first
    // pass reads the 1-byte bins KE4 wrote instead of the 4-byte rotated vector
    EdenCall c{n, dim, nbits, signs, sign_row, sign_bits, ws, ws_bytes, stream};
    return eden_fused(c, x, out, scale_out);
}

// ---- fractional rates 1 < nbits < 2 (AS:352-368, AS:401-411) -----------------------------
int uq_eden_mask_bits(const int64_t* seeds, int64_t rows, int64_t D, uint32_t threshold, uint32_t* bits, void* stream) {
    if (rows < 0 || D < 0) return fail(UQ_E_INVALID, "rows and D must be >= 0");
    if (threshold > (1u << 24)) return fail(UQ_E_INVALID, "threshold must be <= 2^24 (ceil(p_high * 2^24), p_high <= 1)");
    if (rows == 0 || D == 0) return UQ_OK;
    if (rows > 65535) return fail(UQ_E_INVALID, "at most 65535 rows per call");
    if (!seeds || !bits) return fail(UQ_E_INVALID, "null pointer");
    hipLaunchKernelGGL(eden_mask_bits_kernel, dim3((unsigned)rows), dim3(640), 0, (hipStream_t)stream, seeds, D, threshold,
                       bits);
    return launched("eden_mask_bits_kernel launch");
}

int uq_eden_compress_frac_f32(const float* x, int64_t n, int64_t dim, const int8_t* signs, const int32_t* sign_row,
                              const uint32_t* sign_bits, const uint32_t* mask_bits, const int32_t* mask_row, uint8_t* bins,
                              float* scale, void* ws, size_t ws_bytes, void* stream) {
    EdenCall c = frac_call(n, dim, signs, sign_row, sign_bits, mask_bits, mask_row, ws, ws_bytes, stream);
    return eden_call(c, UQ_EDEN_OP_COMPRESS, !x || !bins || !scale, [&] { return eden_compress(c, x, bins, scale); });
}

int uq_eden_decompress_frac_f32(const uint8_t* bins, const float* scale, int64_t n, int64_t dim, const int8_t* signs,
                                const int32_t* sign_row, const uint32_t* sign_bits, const uint32_t* mask_bits,
                                const int32_t* mask_row, float* out, void* ws, size_t ws_bytes, void* stream) {
    EdenCall c = frac_call(n, dim, signs, sign_row, sign_bits, mask_bits, mask_row, ws, ws_bytes, stream);
    return eden_call(c, UQ_EDEN_OP_DECOMPRESS, !bins || !scale || !out, [&] { return eden_decompress(c, bins, scale, out); });
}

int uq_eden_frac_f32(const float* x, float* out, int64_t n, int64_t dim, const int8_t* signs, const int32_t* sign_row,
                     const uint32_t* sign_bits, const uint32_t* mask_bits, const int32_t* mask_row, float* scale_out,
                     void* ws, size_t ws_bytes, void* stream) {
    EdenCall c = frac_call(n, dim, signs, sign_row, sign_bits, mask_bits, mask_row, ws, ws_bytes, stream);
    return eden_fused(c, x, out, scale_out);
}

int uq_eden_compress_f32(const float* x, int64_t n, int64_t dim, int32_t nbits, const int8_t* signs,
                         const int32_t* sign_row, uint8_t* bins, float* scale, void* ws, size_t ws_bytes,
                         void* stream) {
    return uq_eden_compress_f32_sb(x, n, dim, nbits, signs, sign_row, nullptr, bins, scale, ws, ws_bytes, stream);
}

int uq_eden_decompress_f32(const uint8_t* bins, const float* scale, int64_t n, int64_t dim, int32_t nbits,
                           const int8_t* signs, const int32_t* sign_row, float* out, void* ws, size_t ws_bytes,
                           void* stream) {
    return uq_eden_decompress_f32_sb(bins, scale, n, dim, nbits, signs, sign_row, nullptr, out, ws, ws_bytes, stream);
}

int uq_eden_f32(const float* x, float* out, int64_t n, int64_t dim, int32_t nbits, const int8_t* signs,
                const int32_t* sign_row, float* scale_out, void* ws, size_t ws_bytes, void* stream) {
    return uq_eden_f32_sb(x, out, n, dim, nbits, signs, sign_row, nullptr, scale_out, ws, ws_bytes, stream);
}

// ---- the bit-packed message form (it replaces nothing of the reference: AS:335-350 keeps int64 bins) ----
int uq_test_set_eden_hooks(int flags) { return g_eden_hooks.exchange(flags & 1); }

int uq_test_eden_packed_plan(int32_t op, int64_t n, int64_t dim, int32_t kind, int64_t* plan_out, int32_t cap) {
    if (op != UQ_EDEN_OP_COMPRESS && op != UQ_EDEN_OP_DECOMPRESS) return fail(UQ_E_INVALID, "op must be compress or decompress");
    if (!packed_kind_ok(kind)) return fail(UQ_E_INVALID, "kind must be 1, 2 or UQ_EDEN_NBITS_FRAC");
    if (n < 0 || dim < 0) return fail(UQ_E_INVALID, "n and dim must be >= 0");
    if (n == 0 || dim == 0) return export_packed(PackedPlan{}, plan_out, cap);
    return export_packed(packed_plan(eden_plan(op, n, dim, kind, 0), kind, g_eden_hooks.load()), plan_out, cap);
}

int uq_test_last_eden_packed_plan(int32_t op, int64_t* plan_out, int32_t cap) {
    if (op != UQ_EDEN_OP_COMPRESS && op != UQ_EDEN_OP_DECOMPRESS) return fail(UQ_E_INVALID, "op must be compress or decompress");
    return export_packed(t_last_packed[op == UQ_EDEN_OP_DECOMPRESS], plan_out, cap);
}

int uq_eden_packed_words(int64_t D, int32_t kind, int64_t* pitch_words) {
    if (!pitch_words) return fail(UQ_E_INVALID, "null pitch_words");
    if (!packed_kind_ok(kind)) return fail(UQ_E_INVALID, "kind must be 1, 2 or UQ_EDEN_NBITS_FRAC");
    if (D < 0) return fail(UQ_E_INVALID, "D must be >= 0");
    const int64_t P = (D + 31) / 32;
    *pitch_words = kind == 1 ? P : 2 * P;
    return UQ_OK;
}

int uq_eden_packed_workspace_bytes(int64_t n, int64_t dim, int32_t kind, size_t* bytes_out) {
    if (!packed_kind_ok(kind)) return fail(UQ_E_INVALID, "kind must be 1, 2 or UQ_EDEN_NBITS_FRAC");
    // (the layout's u8 bins region, which uq_eden_f32 uses between its two halves, serves the converter path)
    return uq_eden_workspace_bytes(n, dim, bytes_out);
}

int uq_eden_mask_ranks(const uint32_t* mask_bits, int64_t rows, int64_t D, uint32_t* ranks, void* stream) {
    if (rows < 0 || D < 0) return fail(UQ_E_INVALID, "rows and D must be >= 0");
    if (rows == 0) return UQ_OK;
    if (rows > 65535) return fail(UQ_E_INVALID, "at most 65535 rows per call");
    if (!ranks || (D > 0 && !mask_bits)) return fail(UQ_E_INVALID, "null pointer");
    hipLaunchKernelGGL(eden_mask_ranks_kernel, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, mask_bits, D, ranks);
    return launched("eden_mask_ranks_kernel launch");
}

int uq_eden_pack_bins(const uint8_t* bins, int64_t n, int64_t D, int32_t kind, const uint32_t* mask_bits,
                      const uint32_t* mask_ranks, const int32_t* mask_row, uint32_t* payload, int64_t* payload_bits,
                      void* stream) {
    const PackRows r{mask_bits, mask_ranks, mask_row};
    return pack_call(n, D, kind, r, !bins || !payload,
                     [&] { return launch_pack(bins, n, D, kind, r, payload, payload_bits, (hipStream_t)stream); });
}

int uq_eden_unpack_bins(const uint32_t* payload, int64_t n, int64_t D, int32_t kind, const uint32_t* mask_bits,
                        const uint32_t* mask_ranks, const int32_t* mask_row, uint8_t* bins, void* stream) {
    const PackRows r{mask_bits, mask_ranks, mask_row};
    return pack_call(n, D, kind, r, !bins || !payload,
                     [&] { return launch_unpack(payload, n, D, kind, r, bins, (hipStream_t)stream); });
}

int uq_eden_compress_packed_f32(const float* x, int64_t n, int64_t dim, int32_t kind, const int8_t* signs,
                                const int32_t* sign_row, const uint32_t* sign_bits, const uint32_t* mask_bits,
                                const uint32_t* mask_ranks, const int32_t* mask_row, uint32_t* payload,
                                int64_t* payload_bits, float* scale, void* ws, size_t ws_bytes, void* stream) {
    const int hooks = g_eden_hooks.load();
    t_last_plan[UQ_EDEN_OP_COMPRESS] = EdenPlan{};
    t_last_packed[0] = PackedPlan{};
    if (!packed_kind_ok(kind)) return fail(UQ_E_INVALID, "kind must be 1, 2 or UQ_EDEN_NBITS_FRAC");
    EdenCall c = packed_call(n, dim, kind, signs, sign_row, sign_bits, mask_bits, mask_row, ws, ws_bytes, stream);
    const bool null_ptr = !x || !payload || !scale || (kind == UQ_EDEN_NBITS_FRAC && !mask_ranks);
    return eden_call(c, UQ_EDEN_OP_COMPRESS, null_ptr, [&] {
        const PackedPlan k = t_last_packed[0] = packed_plan(c.P, kind, hooks);
        const PackRows r{mask_bits, mask_ranks, mask_row};
        hipStream_t st = (hipStream_t)stream;
        if (k.form == UQ_EDEN_PACKED_FUSED) {
            const int rc = eden_compress(c, x, nullptr, scale, payload);
            return rc ? rc : launch_payload_bits(n, c.P.D, kind, r, payload_bits, st);
        }
        uint8_t* bins = (uint8_t*)c.at(c.w.bins_off);
        const int rc = eden_compress(c, x, bins, scale);
        return rc ? rc : launch_pack(bins, n, c.P.D, kind, r, payload, payload_bits, st);
    });
}

int uq_eden_decompress_packed_f32(const uint32_t* payload, const float* scale, int64_t n, int64_t dim, int32_t kind,
                                  const int8_t* signs, const int32_t* sign_row, const uint32_t* sign_bits,
                                  const uint32_t* mask_bits, const uint32_t* mask_ranks, const int32_t* mask_row, float* out,
                                  void* ws, size_t ws_bytes, void* stream) {
    const int hooks = g_eden_hooks.load();
    t_last_plan[UQ_EDEN_OP_DECOMPRESS] = EdenPlan{};
    t_last_packed[1] = PackedPlan{};
    if (!packed_kind_ok(kind)) return fail(UQ_E_INVALID, "kind must be 1, 2 or UQ_EDEN_NBITS_FRAC");
    EdenCall c = packed_call(n, dim, kind, signs, sign_row, sign_bits, mask_bits, mask_row, ws, ws_bytes, stream);
    const bool null_ptr = !payload || !scale || !out || (kind == UQ_EDEN_NBITS_FRAC && !mask_ranks);
    return eden_call(c, UQ_EDEN_OP_DECOMPRESS, null_ptr, [&] {
        const PackedPlan k = t_last_packed[1] = packed_plan(c.P, kind, hooks);
        if (k.form == UQ_EDEN_PACKED_FUSED) return eden_decompress(c, payload, scale, out, kind);
        uint8_t* bins = (uint8_t*)c.at(c.w.bins_off);
        const int rc = launch_unpack(payload, n, c.P.D, kind, PackRows{mask_bits, mask_ranks, mask_row}, bins, (hipStream_t)stream);
        return rc ? rc : eden_decompress(c, bins, scale, out);
    });
}

// ---- the receivers with the coordinate drop (new entry points; the ones above are unchanged) ----
int uq_test_last_eden_drop_form(int32_t* form_out) {
    if (!form_out) return fail(UQ_E_INVALID, "null form_out");
    *form_out = t_last_drop_form;
    return UQ_OK;
}

int uq_eden_decompress_drop_f32(const uint8_t* bins, const float* scale, int64_t n, int64_t dim, int32_t kind,
                                const int8_t* signs, const int32_t* sign_row, const uint32_t* sign_bits,
                                const uint32_t* mask_bits, const int32_t* mask_row, const uint32_t* drop_bits,
                                const float* cents, float* out, void* ws, size_t ws_bytes, void* stream) {
    t_last_plan[UQ_EDEN_OP_DECOMPRESS] = EdenPlan{};
    t_last_drop_form = UQ_EDEN_DROP_NONE;
    if (!packed_kind_ok(kind)) return fail(UQ_E_INVALID, "kind must be 1, 2 or UQ_EDEN_NBITS_FRAC");
    EdenCall c = packed_call(n, dim, kind, signs, sign_row, sign_bits, mask_bits, mask_row, ws, ws_bytes, stream);
    return eden_call(c, UQ_EDEN_OP_DECOMPRESS, !bins || !scale || !out || !drop_bits || !cents,
                     [&] { return eden_decompress_drop(c, kind, cents, bins, scale, drop_bits, out); });
}

int uq_eden_decompress_packed_drop_f32(const uint32_t* payload, const float* scale, int64_t n, int64_t dim, int32_t kind,
                                       const int8_t* signs, const int32_t* sign_row, const uint32_t* sign_bits,
                                       const uint32_t* mask_bits, const uint32_t* mask_ranks, const int32_t* mask_row,
                                       const uint32_t* drop_bits, const float* cents, float* out, void* ws,
                                       size_t ws_bytes, void* stream) {
    t_last_plan[UQ_EDEN_OP_DECOMPRESS] = EdenPlan{};
    t_last_packed[1] = PackedPlan{};
    t_last_drop_form = UQ_EDEN_DROP_NONE;
    if (!packed_kind_ok(kind)) return fail(UQ_E_INVALID, "kind must be 1, 2 or UQ_EDEN_NBITS_FRAC");
    EdenCall c = packed_call(n, dim, kind, signs, sign_row, sign_bits, mask_bits, mask_row, ws, ws_bytes, stream);
    const bool null_ptr = !payload || !scale || !out || !drop_bits || !cents || (kind == UQ_EDEN_NBITS_FRAC && !mask_ranks);
    return eden_call(c, UQ_EDEN_OP_DECOMPRESS, null_ptr, [&] {
        // the payload rows through the converter into the workspace's u8 bins, whatever the kind
        uint8_t* bins = (uint8_t*)c.at(c.w.bins_off);
        const int rc = launch_unpack(payload, n, c.P.D, kind, PackRows{mask_bits, mask_ranks, mask_row}, bins, (hipStream_t)stream);
        return rc ? rc : eden_decompress_drop(c, kind, cents, bins, scale, drop_bits, out);
    });
}

int uq_eden_drop_f32(const float* x, float* out, int64_t n, int64_t dim, int32_t kind, const int8_t* signs,
                     const int32_t* sign_row, const uint32_t* sign_bits, const uint32_t* mask_bits, const int32_t* mask_row,
                     const uint32_t* drop_bits, const float* cents, float* scale_out, void* ws, size_t ws_bytes,
                     void* stream) {
    t_last_plan[UQ_EDEN_OP_DECOMPRESS] = EdenPlan{};
    t_last_drop_form = UQ_EDEN_DROP_NONE;
    if (!packed_kind_ok(kind)) return fail(UQ_E_INVALID, "kind must be 1, 2 or UQ_EDEN_NBITS_FRAC");
    EdenCall c = packed_call(n, dim, kind, signs, sign_row, sign_bits, mask_bits, mask_row, ws, ws_bytes, stream);
    return eden_call(c, UQ_EDEN_OP_COMPRESS, !x, [&] {
        uint8_t* bins = (uint8_t*)c.at(c.w.bins_off);
        float* scale = scale_out ? scale_out : (float*)c.at(c.w.scale_off);
        const int rc = eden_compress(c, x, bins, scale);
        if (rc) return rc;
        if (!out || !drop_bits || !cents) return fail(UQ_E_INVALID, "null pointer");
        c.P = eden_plan(UQ_EDEN_OP_DECOMPRESS, c.n, c.dim, c.frac ? UQ_EDEN_NBITS_FRAC : c.nbits, 0);
        return eden_decompress_drop(c, kind, cents, bins, scale, drop_bits, out);
    });
}

}  // extern "C"
