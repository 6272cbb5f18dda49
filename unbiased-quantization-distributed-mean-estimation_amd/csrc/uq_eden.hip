// uq_eden.hip — EDEN and the randomized Hadamard transform: workspace layouts, the launchers
// of uq_eden_kernels.h (KE0-KE4) and the C API uq_rht_* / uq_eden_*.  QUIC-FL's sender and
// quantizer run their RHT and norm here (rht_layout, rht_norm_front, rht_inverse in
// uq_internal.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>

#include "uq_eden_kernels.h"
#include "uq_internal.h"

namespace {

// ---- EDEN host helpers ------------------------------------------------------------------
bool eden_tables(int nbits, EdenTables* t) {
    // AS:302-315: centroids (-c reversed, c) as f32; boundaries = midpoints of neighbours
    std::memset(t, 0, sizeof(*t));
    double pos[2];
    int np = 0;
    if (nbits == 1) { pos[0] = 0.7978845608028654; np = 1; }
    else if (nbits == 2) { pos[0] = 0.4527800398860679; pos[1] = 1.5104176087114887; np = 2; }
    else return false;
    double c[4];
    for (int i = 0; i < np; ++i) { c[i] = -pos[np - 1 - i]; c[np + i] = pos[i]; }
    for (int i = 0; i < 2 * np; ++i) t->c[i] = (float)c[i];
    // the reference forms the midpoints from the f32 tensor elements, in double, then
    // stores them as f32 (torch.Tensor of Python floats)
    for (int i = 0; i + 1 < 2 * np; ++i) t->b[i] = (float)(((double)t->c[i] + (double)t->c[i + 1]) / 2.0);
    t->nb = 2 * np - 1;
    return true;
}

int ilog2_pow2(int64_t D) {
    int p = 0;
    while (((int64_t)1 << p) < D) ++p;
    return p;
}

// torch.norm of few clients: the segmented chains (KE2a-KE2d) instead of KE2's sequential
// ones.  KE2 keeps batches above kSegNormMaxN: it hides its chains behind the reads there,
// while KE2s reads the vectors twice.
constexpr int64_t kSegNormMaxN = 256;
// ... and the dot's (KE4s): its one-wave-per-client form runs 6-19 VALU per step, so the
// segmented form pays for its second read only with few clients.  KE4's time is one client's
// chain whatever n (2.67 ms at D = 2^22: 44 % of a 101-client EDEN call, profiles/r6z_*), KE4s
// costs ~15 us per client of 2^22 (~4 per client of 2^20): they cross near 170 clients.
constexpr int64_t kDotSegMaxN = 128;

bool segnorm_applies(int64_t n, int64_t D) {
    return n >= 1 && n <= kSegNormMaxN && D >= kSegMinD && (D & (D - 1)) == 0;
}

struct SegNormLayout {
    size_t segsum, g, e, kind, cnt, tseg, tab, thr, acc, total;      // offsets from the region start
};
SegNormLayout segnorm_layout(int64_t n, int64_t D) {
    const size_t nk = (size_t)n * 8 * (size_t)(D / kSegBlock);
    SegNormLayout L{};
    L.segsum = 0;
    L.g = up256(nk * sizeof(double));
    L.e = up256(L.g + nk * sizeof(float));
    L.kind = up256(L.e + nk * sizeof(float));
    L.cnt = up256(L.kind + nk * sizeof(int32_t));
    L.tseg = up256(L.cnt + (size_t)n * sizeof(int32_t));
    const size_t cap = (size_t)seg_tab_cap(D);
    L.tab = up256(L.tseg + (size_t)n * cap * sizeof(int32_t));
    L.thr = up256(L.tab + (size_t)n * cap * kSegTab * sizeof(float));   // KE4s: thresholds [n][4]
    L.acc = up256(L.thr + (size_t)n * 4 * sizeof(float));                 //       chain ends [n][64]
    L.total = up256(L.acc + (size_t)n * 64 * sizeof(float));
    return L;
}

int launch_segnorm(const float* v, int64_t n, int64_t D, char* region, float* nrm, hipStream_t st) {
    const SegNormLayout L = segnorm_layout(n, D);
    double* segsum = (double*)(region + L.segsum);
    float* g = (float*)(region + L.g);
    float* e = (float*)(region + L.e);
    int32_t* kind = (int32_t*)(region + L.kind);
    int32_t* cnt = (int32_t*)(region + L.cnt);
    int32_t* tseg = (int32_t*)(region + L.tseg);
    float* tab = (float*)(region + L.tab);
    const int64_t K = D / kSegBlock;
    const dim3 grid((unsigned)(K / kSegPerWG), (unsigned)n);
    hipLaunchKernelGGL(eden_segsum_kernel, grid, dim3(256), 0, st, v, D, segsum);
    hipLaunchKernelGGL(eden_segscan_kernel, dim3(8u, (unsigned)n), dim3(256), 0, st, segsum, K, g, cnt);
    const int cap = seg_tab_cap(D);
    hipLaunchKernelGGL(eden_segchain_kernel, grid, dim3(256), 0, st, v, D, g, e, kind, cnt, tseg, cap);
    hipLaunchKernelGGL(eden_segtab_kernel, dim3((unsigned)cap, (unsigned)n), dim3(256), 0, st, v, D, g, cnt, tseg, tab, cap);
    hipLaunchKernelGGL(eden_segwalk_kernel, dim3((unsigned)n), dim3(512), 0, st, v, D, g, e, kind, tab, nrm, cap);
    return hip_check(hipGetLastError(), "eden segmented norm launch");
}

// KE4s (few clients): the bins and the dot's 64 chains in segments, in the segmented norm's
// region (the norm is done with it); the same bits as eden_dotbins_kernel
int launch_eden_dotseg(const float* v, int64_t n, int64_t D, float sqrtD, const float* nrm, const EdenTables& tab,
                       uint8_t* bins, float* scale, char* region, hipStream_t st) {
    const SegNormLayout L = segnorm_layout(n, D);
    double* segsum = (double*)(region + L.segsum);
    float* g = (float*)(region + L.g);
    float* e = (float*)(region + L.e);
    int32_t* kind = (int32_t*)(region + L.kind);
    int32_t* cnt = (int32_t*)(region + L.cnt);
    int32_t* tseg = (int32_t*)(region + L.tseg);
    float* tabv = (float*)(region + L.tab);
    float* thr4 = (float*)(region + L.thr);
    float* acc64 = (float*)(region + L.acc);
    const int64_t K = D / kEdenTile;
    const int cap = seg_tab_cap(D);
    hipLaunchKernelGGL(eden_thresh_kernel, dim3((unsigned)n), dim3(64), 0, st, nrm, tab, thr4);
    hipLaunchKernelGGL(eden_dseg_sum_kernel, dim3((unsigned)K, (unsigned)n), dim3(256), 0, st, v, D, sqrtD, nrm, thr4, tab,
                       bins, segsum);
    hipLaunchKernelGGL(eden_segscan_l_kernel<64>, dim3(64u, (unsigned)n), dim3(256), 0, st, segsum, K, g, cnt);
    hipLaunchKernelGGL(eden_dseg_chain_kernel, dim3((unsigned)(K / kDSegTiles), (unsigned)n), dim3(256), 0, st, v, D, sqrtD,
                       nrm, thr4, tab, g, e, kind, cnt, tseg, cap);
    hipLaunchKernelGGL(eden_dseg_tab_kernel, dim3((unsigned)cap, (unsigned)n), dim3(256), 0, st, v, D, sqrtD, nrm, thr4, tab,
                       g, cnt, tseg, tabv, cap);
    hipLaunchKernelGGL(eden_dseg_walk_kernel, dim3(8u, (unsigned)n), dim3(512), 0, st, v, D, sqrtD, nrm, thr4, tab, g, e,
                       kind, tabv, acc64, cap);
    hipLaunchKernelGGL(eden_dseg_final_kernel, dim3((unsigned)n), dim3(64), 0, st, acc64, nrm, scale);
    return hip_check(hipGetLastError(), "eden segmented dot launch");
}

// AS:329-335: the bins and the scale's dot in MKL sdot's order (KE4), scale = f32(nrm * nrm) / dot
int launch_eden_dotbins(const float* v, int64_t n, int64_t D, float sqrtD, const float* nrm, const EdenTables& tab,
                        uint8_t* bins, float* scale, hipStream_t st, const int32_t* redo = nullptr) {
    const dim3 grid((unsigned)((n + kDotWaves - 1) / kDotWaves)), block(64 * kDotWaves);
    if (tab.nb == 1)
        hipLaunchKernelGGL(eden_dotbins_kernel<1>, grid, block, 0, st, v, D, sqrtD, nrm, tab, bins, scale, n, redo);
    else
        hipLaunchKernelGGL(eden_dotbins_kernel<3>, grid, block, 0, st, v, D, sqrtD, nrm, tab, bins, scale, n, redo);
    return hip_check(hipGetLastError(), "eden_dotbins_kernel launch");
}

int launch_chainnorm(const float* v, int64_t n, int64_t D, float* nrm, hipStream_t st) {
    const dim3 grid((unsigned)((n + kNormClients - 1) / kNormClients));
    if (D % kNormChunk == 0)
        hipLaunchKernelGGL(eden_norm_whole_kernel, grid, dim3(kNormThreads), 0, st, v, n, D, nrm);
    else
        hipLaunchKernelGGL(eden_norm_kernel, grid, dim3(kNormThreads), 0, st, v, n, D, nrm);
    return hip_check(hipGetLastError(), "eden_norm_kernel launch");
}

struct EdenLayout {
    size_t vec_off, nrm_off, bins_off, scale_off, redo_off, seg_off, total;
    int64_t D;
    int32_t tiles;
    bool seg;                 // the segmented norm (its region at seg_off)
};

EdenLayout eden_layout(int64_t n, int64_t dim) {
    EdenLayout w{};
    w.D = dim <= 1 ? 1 : ((int64_t)1 << ilog2_pow2(dim));
    w.tiles = (int32_t)((w.D + kEdenTile - 1) / kEdenTile);
    w.vec_off = kCtrlBytes;
    w.nrm_off = up256(w.vec_off + (size_t)n * w.D * sizeof(float));
    w.bins_off = up256(w.nrm_off + (size_t)n * sizeof(float));
    w.scale_off = up256(w.bins_off + (size_t)n * w.D);
    w.redo_off = up256(w.scale_off + (size_t)n * sizeof(float));
    w.seg_off = up256(w.redo_off + (size_t)n * sizeof(int32_t));
    w.seg = segnorm_applies(n, w.D);
    w.total = w.seg_off + (w.seg ? segnorm_layout(n, w.D).total : 0);
    return w;
}

// One FWHT pass: the register-radix kernels for the 4096-element low pass and the
// 256 x 64 high pass, the generic LDS kernel otherwise (same stages, same bits).
template <int M, bool L, bool R>
void fwht_dispatch(dim3 grid, const FwhtArgs& b, int lo, int k, hipStream_t st) {
    if (lo == 0 && k == kFwhtLow16Bits && !L)
        hipLaunchKernelGGL((fwht_low16k_kernel<M>), dim3((unsigned)(b.D >> kFwhtLow16Bits), grid.y), dim3(1024), 0, st, b);
    else if (lo == 0 && k == kFwhtLowBits && (M != 2 || (b.D % 16) == 0))
        hipLaunchKernelGGL((fwht_low4096_kernel<M, L, R>), grid, dim3(256), 0, st, b);
    else if (lo > 0 && k == kFwhtHighBits && M == 0 && ((int64_t)1 << lo) % kHighCols == 0)
        hipLaunchKernelGGL((fwht_high256_kernel<L, R>), dim3(grid.x * kFwhtCols / kHighCols, grid.y), dim3(kHighT), 0, st,
                           b, lo);
    else if (lo > 0 && k <= 6 && M == 0 && (int64_t)grid.y * ((b.D >> k) / 256) >= 1024) {
        // (a thread per column: with fewer than 1024 workgroups, e.g. one client of 2^18,
        // the generic kernel's 2^k x 32 tiles spread the pass over more of the GPU)
        const dim3 g2((unsigned)(((b.D >> k) + 255) / 256), grid.y);
        switch (k) {
            case 1: hipLaunchKernelGGL((fwht_small_kernel<1, L, R>), g2, dim3(256), 0, st, b, lo); break;
            case 2: hipLaunchKernelGGL((fwht_small_kernel<2, L, R>), g2, dim3(256), 0, st, b, lo); break;
            case 3: hipLaunchKernelGGL((fwht_small_kernel<3, L, R>), g2, dim3(256), 0, st, b, lo); break;
            case 4: hipLaunchKernelGGL((fwht_small_kernel<4, L, R>), g2, dim3(256), 0, st, b, lo); break;
            case 5: hipLaunchKernelGGL((fwht_small_kernel<5, L, R>), g2, dim3(256), 0, st, b, lo); break;
            default: hipLaunchKernelGGL((fwht_small_kernel<6, L, R>), g2, dim3(256), 0, st, b, lo); break;
        }
    } else
        hipLaunchKernelGGL((fwht_pass_kernel<M, L, R>), grid, dim3(kFwhtT), 0, st, b, lo, k);
}

// The passes of one transform of 2^p elements, low bits first: the first pass takes up to
// `first` bits (contiguous tiles), every later one up to kFwhtHighBits (2^k rows x kFwhtCols
// columns).  lo0 > 0 resumes a transform whose passes below bit lo0 are done.
struct FwhtPasses {
    int p, lo, k;
    FwhtPasses(int p_, int first, int lo0 = 0) : p(p_), lo(lo0), k(std::min(p_ - lo0, lo0 ? kFwhtHighBits : first)) {}
    bool last() const { return lo + k >= p; }
    int64_t tiles() const { return ((int64_t)1 << (p - k)) / (lo == 0 ? 1 : kFwhtCols); }
    void next() { lo += k; k = std::min(p - lo, kFwhtHighBits); }
};
// First pass of the forward transform and the receivers' inverse: D = 2^22 (config C4) takes 14
// bits, then 8 (one pass fewer than 12 + 8 + 2)
int fwht_first_bits(int p) { return p == kFwhtLow16Bits + kFwhtHighBits ? kFwhtLow16Bits : kFwhtLowBits; }

FwhtArgs fwht_args(const void* in, const int8_t* signs, const int32_t* sign_row, const uint32_t* sbits,
                   const float* scale, int64_t D, int64_t dim, const EdenTables& tab) {
    const float sqrtD = (float)std::sqrt((double)D);         // np.sqrt(d) -> f32 operand
    return FwhtArgs{in, /*out (set per pass)*/ nullptr, signs, sign_row, sbits, scale, D, dim, sqrtD, tab};
}

// Runs the FWHT passes of one transform.  MODE of the first pass: 1 sender, 2 receiver.
// Receiver: passes in place in `buf`, the last into `out`.  Sender: passes alternate
// between `buf` and `out` (out == buf: in place; the forward RHT passes its output so
// that a two-pass transform needs no copy); *result = the buffer holding the result.
// lo0 > 0 (receiver): the passes below bit lo0 are done already, into `buf`.
int launch_fwht(FwhtArgs a, int64_t n, bool receiver, float* buf, float* out, hipStream_t st,
                float** result = nullptr, int lo0 = 0) {
    const int p = ilog2_pow2(a.D);
    float* cur = buf;                              // sender: the buffer the next pass writes
    for (FwhtPasses ps(p, fwht_first_bits(p), lo0);; ps.next()) {
        const int lo = ps.lo, k = ps.k;
        const bool first = lo == 0, last = ps.last();
        FwhtArgs b = a;
        if (receiver) {
            b.out = last ? out : buf;
            if (!first) b.in = buf;
        } else {
            b.out = cur;
            if (!first) b.in = cur == buf ? out : buf;
            if (result) *result = cur;
            cur = cur == buf ? out : buf;
        }
        const dim3 grid((unsigned)ps.tiles(), (unsigned)n);
        if (first && !receiver) {
            if (last) fwht_dispatch<1, true, false>(grid, b, lo, k, st);
            else fwht_dispatch<1, false, false>(grid, b, lo, k, st);
        } else if (first && receiver) {
            if (last) fwht_dispatch<2, true, true>(grid, b, lo, k, st);
            else fwht_dispatch<2, false, false>(grid, b, lo, k, st);
        } else if (last && receiver) {
            fwht_dispatch<0, true, true>(grid, b, lo, k, st);
        } else if (last) {
            fwht_dispatch<0, true, false>(grid, b, lo, k, st);
        } else {
            fwht_dispatch<0, false, false>(grid, b, lo, k, st);
        }
        int rc = hip_check(hipGetLastError(), "fwht_pass_kernel launch");
        if (rc) return rc;
        if (last) break;
    }
    return UQ_OK;
}

// The inverse transform of plain vectors (H, then * diag on the last pass, no scale): the
// first pass reads a.in, the passes run in place in `buf` and the last writes `out`.
int launch_inverse_passes(const FwhtArgs& a, FwhtPasses ps, int64_t n, float* buf, float* out, hipStream_t st) {
    for (;; ps.next()) {
        const bool last = ps.last();
        FwhtArgs b = a;
        if (ps.lo > 0) b.in = buf;
        b.out = last ? out : buf;
        const dim3 grid((unsigned)ps.tiles(), (unsigned)n);
        if (last) fwht_dispatch<0, true, true>(grid, b, ps.lo, ps.k, st);
        else fwht_dispatch<0, false, false>(grid, b, ps.lo, ps.k, st);
        const int rc = hip_check(hipGetLastError(), "fwht_pass_kernel launch");
        if (rc || last) return rc;
    }
}

int eden_check(int64_t n, int64_t dim, int32_t nbits, const int8_t* signs, EdenTables* tab) {
    if (n < 0 || dim < 0) return fail(UQ_E_INVALID, "n and dim must be >= 0");
    if (n > 65535) return fail(UQ_E_INVALID, "at most 65535 clients per call");
    if (dim > ((int64_t)1 << 28)) return fail(UQ_E_INVALID, "dim must be <= 2^28");
    if (!eden_tables(nbits, tab)) return fail(UQ_E_INVALID, "EDEN nbits must be 1 or 2 (the reference's tables)");
    if (n > 0 && dim > 0 && !signs) return fail(UQ_E_INVALID, "null signs");
    return UQ_OK;
}

// The sender up to the norms: RHT (AS:123-141) and torch.norm (AS:329); *rot = the rotated
// vectors (one of the workspace's two vector buffers).
int eden_front(const float* x, int64_t n, int64_t dim, const EdenTables& tab, const int8_t* signs,
               const int32_t* sign_row, const EdenLayout& w, char* wsb, FwhtArgs& a, float** rot, hipStream_t st,
               const uint32_t* sbits = nullptr) {
    float* nrm = (float*)(wsb + w.nrm_off);
    a = fwht_args(x, signs, sign_row, sbits, nullptr, w.D, dim, tab);
    float* vec = (float*)(wsb + w.vec_off);
    int rc = launch_fwht(a, n, false, vec, vec, st, rot);
    if (rc) return rc;
    if (w.seg) return launch_segnorm(*rot, n, w.D, wsb + w.seg_off, nrm, st);       // AS:329 torch.norm
    return launch_chainnorm(*rot, n, w.D, nrm, st);
}

}  // namespace

// ---- what QUIC-FL's sender and quantizer run here (uq_internal.h) -------------------------
RhtLayout uq_internal::rht_layout(int64_t n, int64_t dim) {
    const EdenLayout w = eden_layout(n, dim);
    return RhtLayout{w.nrm_off, w.total, w.D};
}

int uq_internal::rht_norm_front(const float* x, int64_t n, int64_t dim, const int8_t* signs, const int32_t* sign_row,
                                char* wsb, float** rot, hipStream_t st) {
    FwhtArgs a;
    return eden_front(x, n, dim, EdenTables{}, signs, sign_row, eden_layout(n, dim), wsb, a, rot, st);
}

// AS:533-535: H, then * diag, [:dim]; D = 2^22 as 14 + 8 bits
int uq_internal::rht_inverse(float* rot, float* out, int64_t n, int64_t D, int64_t dim, const int8_t* signs,
                             const int32_t* sign_row, hipStream_t st) {
    const FwhtArgs a = fwht_args(rot, signs, sign_row, nullptr, nullptr, D, dim, EdenTables{});
    const int p = ilog2_pow2(D);
    return launch_inverse_passes(a, FwhtPasses(p, fwht_first_bits(p)), n, rot, out, st);
}

extern "C" {

// ---- EDEN + RHT ------------------------------------------------------------------------
int uq_rht_signs(const int32_t* seeds, int64_t rows, int64_t D, int8_t* signs, void* stream) {
    if (rows < 0 || D < 0) return fail(UQ_E_INVALID, "rows and D must be >= 0");
    if (rows == 0 || D == 0) return UQ_OK;
    if (rows > 65535) return fail(UQ_E_INVALID, "at most 65535 rows per call");
    if (!seeds || !signs) return fail(UQ_E_INVALID, "null pointer");
    hipLaunchKernelGGL(rht_signs_kernel, dim3((unsigned)rows), dim3(640), 0, (hipStream_t)stream, seeds, D, signs);
    return hip_check(hipGetLastError(), "rht_signs_kernel launch");
}

int uq_rht_f32(const float* x, float* out, int64_t n, int64_t dim, int32_t inverse, const int8_t* signs,
               const int32_t* sign_row, void* ws, size_t ws_bytes, void* stream) {
    if (n < 0 || dim < 0) return fail(UQ_E_INVALID, "n and dim must be >= 0");
    if (n > 65535) return fail(UQ_E_INVALID, "at most 65535 clients per call");
    if (n == 0 || dim == 0) return UQ_OK;
    if (!x || !out || !signs) return fail(UQ_E_INVALID, "null pointer");
    const EdenLayout w = eden_layout(n, dim);
    if (inverse && dim != w.D) return fail(UQ_E_INVALID, "inverse RHT input length must be a power of two");
    // the transform uses the vector region only (no norm: the segmented-norm tables past
    // seg_off are not needed here)
    if (!ws || ws_bytes < w.seg_off) return fail(UQ_E_WORKSPACE, "workspace too small");
    const FwhtArgs a = fwht_args(x, signs, sign_row, nullptr, nullptr, w.D, inverse ? w.D : dim, EdenTables{});
    hipStream_t st = (hipStream_t)stream;
    float* buf = (float*)((char*)ws + w.vec_off);
    if (!inverse) {                                           // AS:123-141: pad, * diag, H
        float* res = nullptr;
        int rc = launch_fwht(a, n, false, buf, out, st, &res);
        if (rc || res == out) return rc;
        return hip_check(hipMemcpyAsync(out, buf, (size_t)n * w.D * sizeof(float), hipMemcpyDeviceToDevice, st),
                         "copy rht");
    }
    // AS:146-153: H, then * diag (the receiver's last pass with no scale).  This entry's first
    // pass takes 12 bits at most whatever D, so D = 2^22 runs 12 + 8 + 2 here, not the 14 + 8
    // of fwht_first_bits: another width would launch other kernels.
    return launch_inverse_passes(a, FwhtPasses(ilog2_pow2(w.D), kFwhtLowBits), n, buf, out, st);
}

int uq_eden_workspace_bytes(int64_t n, int64_t dim, size_t* bytes_out) {
    if (!bytes_out) return fail(UQ_E_INVALID, "null bytes_out");
    if (n < 0 || dim < 0) return fail(UQ_E_INVALID, "n and dim must be >= 0");
    *bytes_out = eden_layout(n, dim).total;
    return UQ_OK;
}

int uq_eden_norm_workspace_bytes(int64_t n, int64_t D, size_t* bytes_out) {
    if (!bytes_out) return fail(UQ_E_INVALID, "null bytes_out");
    if (n < 0 || D < 0) return fail(UQ_E_INVALID, "n and D must be >= 0");
    *bytes_out = segnorm_applies(n, D) ? segnorm_layout(n, D).total : 0;
    return UQ_OK;
}

int uq_eden_norm_f32(const float* v, int64_t n, int64_t D, int32_t mode, float* nrm, void* ws, size_t ws_bytes,
                     void* stream) {
    if (n < 0 || D < 0) return fail(UQ_E_INVALID, "n and D must be >= 0");
    if (n > 65535) return fail(UQ_E_INVALID, "at most 65535 clients per call");
    if (mode < 0 || mode > 2) return fail(UQ_E_INVALID, "mode must be 0 (auto), 1 (chains) or 2 (segmented)");
    if (n == 0) return UQ_OK;
    if (!v || !nrm) return fail(UQ_E_INVALID, "null pointer");
    const bool seg = mode == 2 || (mode == 0 && segnorm_applies(n, D));
    if (seg && !segnorm_applies(n, D))
        return fail(UQ_E_INVALID, "segmented norm: 1 <= n <= 256 and D a power of two >= 16384");
    if (D == 0) return hip_check(hipMemsetAsync(nrm, 0, (size_t)n * sizeof(float), (hipStream_t)stream), "norm fill");
    if (!seg) return launch_chainnorm(v, n, D, nrm, (hipStream_t)stream);
    if (!ws || ws_bytes < segnorm_layout(n, D).total) return fail(UQ_E_WORKSPACE, "workspace too small");
    return launch_segnorm(v, n, D, (char*)ws, nrm, (hipStream_t)stream);
}

int uq_eden_compress_f32(const float* x, int64_t n, int64_t dim, int32_t nbits, const int8_t* signs,
                         const int32_t* sign_row, uint8_t* bins, float* scale, void* ws, size_t ws_bytes,
                         void* stream) {
    return uq_eden_compress_f32_sb(x, n, dim, nbits, signs, sign_row, nullptr, bins, scale, ws, ws_bytes, stream);
}

int uq_rht_sign_bits(const int8_t* signs, int64_t rows, int64_t D, uint32_t* bits, void* stream) {
    if (rows < 0 || D < 0) return fail(UQ_E_INVALID, "rows and D must be >= 0");
    if (rows == 0 || D == 0) return UQ_OK;
    if (!signs || !bits) return fail(UQ_E_INVALID, "null pointer");
    const int64_t words = rows * ((D + 31) / 32);
    hipLaunchKernelGGL(rht_sign_bits_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       signs, rows, D, bits);
    return hip_check(hipGetLastError(), "rht_sign_bits_kernel launch");
}

int uq_eden_compress_f32_sb(const float* x, int64_t n, int64_t dim, int32_t nbits, const int8_t* signs,
                            const int32_t* sign_row, const uint32_t* sign_bits, uint8_t* bins, float* scale, void* ws,
                            size_t ws_bytes, void* stream) {
    EdenTables tab;
    int rc = eden_check(n, dim, nbits, signs, &tab);
    if (rc) return rc;
    if (n == 0 || dim == 0) return UQ_OK;
    if (!x || !bins || !scale) return fail(UQ_E_INVALID, "null pointer");
    const EdenLayout w = eden_layout(n, dim);
    if (!ws || ws_bytes < w.total) return fail(UQ_E_WORKSPACE, "workspace too small");
    hipStream_t st = (hipStream_t)stream;
    char* wsb = (char*)ws;
    float* nrm = (float*)(wsb + w.nrm_off);
    if (!w.seg && tab.nb == 1 && w.D % kNormChunk == 0) {
        // 1 bit, many clients: the norm, the bins and the dot in one read (KE2+4), then KE4 for
        // the clients it flags (a norm that is not positive and finite, an underflowing quotient)
        const FwhtArgs a = fwht_args(x, signs, sign_row, sign_bits, nullptr, w.D, dim, EdenTables{});
        float* vec = (float*)(wsb + w.vec_off);
        float* rot = nullptr;
        rc = launch_fwht(a, n, false, vec, vec, st, &rot);                          // AS:123-141
        if (rc) return rc;
        int32_t* redo = (int32_t*)(wsb + w.redo_off);
        hipLaunchKernelGGL(eden_normdot1_kernel, dim3((unsigned)((n + kNormClients - 1) / kNormClients)),
                           dim3(kNDThreads), 0, st, rot, n, w.D, a.sqrtD, tab, nrm, bins, scale, redo);
        rc = hip_check(hipGetLastError(), "eden_normdot1_kernel launch");           // AS:329-335
        if (rc) return rc;
        return launch_eden_dotbins(rot, n, w.D, a.sqrtD, nrm, tab, bins, scale, st, redo);
    }
    FwhtArgs a;
    float* vec = nullptr;
    rc = eden_front(x, n, dim, tab, signs, sign_row, w, wsb, a, &vec, st, sign_bits);
    if (rc) return rc;
    if (w.seg && n <= kDotSegMaxN)                                                   // AS:329-335
        return launch_eden_dotseg(vec, n, w.D, a.sqrtD, nrm, tab, bins, scale, wsb + w.seg_off, st);
    return launch_eden_dotbins(vec, n, w.D, a.sqrtD, nrm, tab, bins, scale, st);
}

int uq_eden_decompress_f32(const uint8_t* bins, const float* scale, int64_t n, int64_t dim, int32_t nbits,
                           const int8_t* signs, const int32_t* sign_row, float* out, void* ws, size_t ws_bytes,
                           void* stream) {
    return uq_eden_decompress_f32_sb(bins, scale, n, dim, nbits, signs, sign_row, nullptr, out, ws, ws_bytes, stream);
}

int uq_eden_decompress_f32_sb(const uint8_t* bins, const float* scale, int64_t n, int64_t dim, int32_t nbits,
                              const int8_t* signs, const int32_t* sign_row, const uint32_t* sign_bits, float* out,
                              void* ws, size_t ws_bytes, void* stream) {
    EdenTables tab;
    int rc = eden_check(n, dim, nbits, signs, &tab);
    if (rc) return rc;
    if (n == 0 || dim == 0) return UQ_OK;
    if (!bins || !scale || !out) return fail(UQ_E_INVALID, "null pointer");
    const EdenLayout w = eden_layout(n, dim);
    if (!ws || ws_bytes < w.total) return fail(UQ_E_WORKSPACE, "workspace too small");
    const FwhtArgs a = fwht_args(bins, signs, sign_row, sign_bits, scale, w.D, dim, tab);
    return launch_fwht(a, n, true, (float*)((char*)ws + w.vec_off), out, (hipStream_t)stream);   // AS:378-413
}

int uq_eden_f32(const float* x, float* out, int64_t n, int64_t dim, int32_t nbits, const int8_t* signs,
                const int32_t* sign_row, float* scale_out, void* ws, size_t ws_bytes, void* stream) {
    return uq_eden_f32_sb(x, out, n, dim, nbits, signs, sign_row, nullptr, scale_out, ws, ws_bytes, stream);
}

int uq_eden_f32_sb(const float* x, float* out, int64_t n, int64_t dim, int32_t nbits, const int8_t* signs,
                   const int32_t* sign_row, const uint32_t* sign_bits, float* scale_out, void* ws, size_t ws_bytes,
                   void* stream) {
    // compress (RHT, norm, bins + the MKL-order dot) then decompress: the receiver's first
    // pass reads the 1-byte bins KE4 wrote instead of the 4-byte rotated vector
    const EdenLayout w = eden_layout(n < 0 ? 0 : n, dim < 0 ? 0 : dim);
    uint8_t* bins = (uint8_t*)((char*)ws + w.bins_off);
    float* scale = scale_out ? scale_out : (float*)((char*)ws + w.scale_off);
    int rc = uq_eden_compress_f32_sb(x, n, dim, nbits, signs, sign_row, sign_bits, bins, scale, ws, ws_bytes, stream);
    if (rc) return rc;
    return uq_eden_decompress_f32_sb(bins, scale, n, dim, nbits, signs, sign_row, sign_bits, out, ws, ws_bytes, stream);
}

}  // extern "C"
