// uq_unbiased.hip — the unbiased L1-ball type quantizer (MI355X, gfx950): workspace layout, the
// launchers of uq_unbiased_kernels.h and the C API uq_workspace_bytes, uq_l1_torch_order_f32,
// uq_type_unbiased_*, uq_codes_*, uq_nibbles_* and uq_client_mean_f32.  The biased quantizer
// reaches the L1 cascade here (launch_l1 in uq_internal.h).
//
// Reference path (paths relative to the reference root):
//   NMSE_Results/Codes/All_Schemes.py:609-641   Type_unbiased_quantize
//   NMSE_Results/Codes/Normal_dist.py:137-138    est += Q(v, R) / n   (client mean)
//
// Kernels (one HIP stage per group of reference torch ops):
//   K1a l1_partial_kernel    AS:624 |x|.sum(), torch CPU cascade: level-1 block sums (uq_common.h)
//   K1b l1_finalize_kernel   AS:624 the rest of the cascade tree, one wave per client (uq_common.h)
//   K2  AS:625-640 normalize -> floor/frac -> fp64 scan (cumsum) -> crossing test -> dequantize
//       (and the type codes), every fp64 prefix bit-exact (see "K2" in uq_unbiased_kernels.h),
//       in four forms:
//         stream    quantize_stream_kernel: one workgroup per client carries the exact prefix
//                   from tile to tile (n >= 256); no inter-workgroup communication
//         small     quantize_small_kernel: d < 32768, L1 and the stream in one launch
//         segments  few clients, many tiles: agg_stream_kernel (approximate tile sums) ->
//                   tile_prefix_kernel -> tile_map_kernel (exact tile maps) -> exact_fold_kernel
//                   (exact prefixes) -> quantize_stream_kernel over segments of tiles
//         phased    otherwise: tile_agg_kernel -> tile_prefix_kernel -> tile_map_kernel ->
//                   exact_fold_kernel -> tile_out_kernel, one workgroup per tile
//   K3  client_mean_kernel   ND:137-138 client-ordered f32 mean; from the type codes:
//       codes_decode_kernel, codes_mean_kernel (K3c), nibbles_mean_kernel (K3n, 4-bit codes)
//
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off (no FMA contraction: the
// reference computes m*p then floor then subtract as separate f32 ops), IEEE f32
// division and denormals kept (the reference runs on torch CPU).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <type_traits>

#include "uq_internal.h"
#include "uq_unbiased_kernels.h"

namespace {

// ---- workspace layout (uq_workspace_bytes) -----------------------------------------
// [0,256)            control bytes (kCtrlBytes, uq_common.h): the sticky status word
// [256, ...)         u64 agg[n][tiles]           (small batches: tile sums A_t, then the approximate
//                                                 prefixes P'_t, then the fold's exact P_t)
// then               u64 incl[n][tiles]          (small batches: map m0)
// then               u64 map1[n][tiles]          (small batches: map m1)
// then               TileRec rec[min(n,256)][32] (irregular tiles' event records) and their counts
// then               f32 l1part[n][groups][32]  (level-1 block sums)
// then               f32 l1[n]                  (computed norms)
struct WsLayout {
    size_t agg_off, incl_off, map1_off, rec_off, cnt_off, part_off, l1_off, total;
    int32_t tiles;
    template <class T>
    T* at(void* ws, size_t off) const { return (T*)((char*)ws + off); }
    // client j0's row of one of the u64 [n][tiles] arrays
    uint64_t* tile_row(void* ws, size_t off, int64_t j0) const { return at<uint64_t>(ws, off) + j0 * tiles; }
};

WsLayout layout(int64_t n, int64_t d, const L1Plan& plan) {
    WsLayout w{};
    const int64_t tiles = (d + kQTile - 1) / kQTile;
    w.tiles = (int32_t)tiles;
    w.agg_off = kCtrlBytes;
    w.incl_off = up256(w.agg_off + (size_t)n * tiles * sizeof(uint64_t));
    w.map1_off = up256(w.incl_off + (size_t)n * tiles * sizeof(uint64_t));
    const size_t rec_clients = (size_t)std::min<int64_t>(n, kRecClients);
    w.rec_off = up256(w.map1_off + (size_t)n * tiles * sizeof(uint64_t));
    w.cnt_off = up256(w.rec_off + rec_clients * kRecPerClient * sizeof(TileRec));
    w.part_off = up256(w.cnt_off + rec_clients * sizeof(uint32_t));
    w.l1_off = up256(w.part_off + (size_t)n * plan.total_groups * 32 * sizeof(float));
    w.total = up256(w.l1_off + (size_t)n * sizeof(float));
    return w;
}

int launch_l1(const float* x, int64_t n, int64_t d, const L1Plan& plan, float* part, float* l1_out,
              hipStream_t st) {
    return launch_cascade<AbsOp>(x, n, d, plan, part, l1_out, nullptr, 0.f, st);
}

// Resident stream-kernel workgroups on this device: 4 per CU (launch bounds).
int stream_slots(int* out) {
    int dev = 0;
    int rc = hip_check(hipGetDevice(&dev), "hipGetDevice");
    if (rc) return rc;
    static thread_local int cache_dev = -1, cache_slots = 0;
    if (cache_dev != dev) {
        int cus = 0;
        rc = hip_check(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev), "CU count");
        if (rc) return rc;
        cache_slots = 4 * std::max(1, cus);
        cache_dev = dev;
    }
    *out = cache_slots;
    return UQ_OK;
}

int check_common(const void* x, int64_t n, int64_t d, int32_t T, void* ws, size_t ws_bytes,
                 L1Plan* plan, WsLayout* w) {
    if (n < 0 || d < 0) return fail(UQ_E_INVALID, "n and d must be >= 0");
    if (n > (int64_t)1 << 31 || d > (int64_t)1 << 40) return fail(UQ_E_INVALID, "n or d too large");
    if (T < 1) return fail(UQ_E_INVALID, "torch_threads must be >= 1");
    if (!make_plan(d, T, plan)) return fail(UQ_E_INVALID, "torch_threads > 4096 (or d too large) unsupported by the L1 plan");
    *w = layout(n, d, *plan);
    if ((int64_t)w->tiles * n > 0xFFFFFFFFll) return fail(UQ_E_INVALID, "batch too large for one call");
    if (n > 0 && d > 0) {
        if (!x) return fail(UQ_E_INVALID, "null input pointer");
        if (!ws) return fail(UQ_E_INVALID, "null workspace");
        if (ws_bytes < w->total) return fail(UQ_E_WORKSPACE, "workspace too small");
    }
    return UQ_OK;
}

}  // namespace

// The biased quantizer reaches the L1 cascade through this: the plan is rebuilt
// from (d, T), which the caller has checked (make_plan is a few integer operations).
int uq_internal::launch_l1(const float* x, int64_t n, int64_t d, int32_t T, float* part, float* l1_out,
                           hipStream_t st) {
    L1Plan plan;
    if (!make_plan(d, T, &plan)) return fail(UQ_E_INVALID, "cannot build L1 plan");
    return ::launch_l1(x, n, d, plan, part, l1_out, st);
}

extern "C" {

int uq_workspace_bytes(int64_t n, int64_t d, int32_t T, size_t* bytes_out) {
    if (!bytes_out) return fail(UQ_E_INVALID, "null bytes_out");
    L1Plan plan;
    if (n < 0 || d < 0 || T < 1) return fail(UQ_E_INVALID, "bad n/d/torch_threads");
    if (!make_plan(d, T, &plan)) return fail(UQ_E_INVALID, "cannot build L1 plan");
    *bytes_out = layout(n, d, plan).total;
    return UQ_OK;
}

int uq_l1_torch_order_f32(const float* x, int64_t n, int64_t d, int32_t T, float* l1_out, void* ws,
                          size_t ws_bytes, void* stream) {
    L1Plan plan;
    WsLayout w;
    int rc = check_common(x, n, d, T, ws, ws_bytes, &plan, &w);
    if (rc) return rc;
    if (n == 0) return UQ_OK;
    if (!l1_out) return fail(UQ_E_INVALID, "null l1_out");
    hipStream_t st = (hipStream_t)stream;
    if (d == 0) return hip_check(hipMemsetAsync(l1_out, 0, n * sizeof(float), st), "memset l1");
    return launch_l1(x, n, d, plan, w.at<float>(ws, w.part_off), l1_out, st);
}

}  // extern "C"

namespace {

// Kernel selection: the run-time flags Q (write q), C (write codes) and CV (code rows 16-byte
// aligned) become compile-time constants, and f(Q, C, CV) launches the kernel they name.  Only
// the five combinations a call can reach exist as kernels: something is written, and without
// codes CV is set.  False for any other combination (f is not called).
template <bool B>
using Flag = std::integral_constant<bool, B>;

template <class F>
bool select_qc(bool q, bool c, bool cv, F&& f) {
    constexpr Flag<true> Y{};
    constexpr Flag<false> N{};
    switch ((q ? 4 : 0) | (c ? 2 : 0) | (cv ? 1 : 0)) {
        case 5: f(Y, N, Y); return true;
        case 7: f(Y, Y, Y); return true;
        case 6: f(Y, Y, N); return true;
        case 3: f(N, Y, Y); return true;
        case 2: f(N, Y, N); return true;
        default: return false;
    }
}

// ... with V (rows of x and q 16-byte aligned) in front, for tile_out_kernel: f(V, Q, C, CV)
template <class F>
bool select_vqc(bool v, bool q, bool c, bool cv, F&& f) {
    if (v) return select_qc(q, c, cv, [&](auto Q, auto C, auto CV) { f(Flag<true>{}, Q, C, CV); });
    return select_qc(q, c, cv, [&](auto Q, auto C, auto CV) { f(Flag<false>{}, Q, C, CV); });
}

int bad_selector() { return fail(UQ_E_INVALID, "internal: bad kernel selector"); }

// ---- dispatch plan -------------------------------------------------------------------
// Every decision of unbiased_codes_impl, made on the host from the call's shape alone: which
// K2 form runs, which template instance of it, and how the clients are chunked.  The dispatcher
// launches what the plan names and nothing else decides, so the test hooks
// (uq_test_unbiased_plan, uq_test_last_unbiased_plan) report what a call really runs.
struct PlanIn {
    int64_t n, d, ldo, ldc;
    bool x16, out16, codes16;          // 16-byte alignment of the base pointers
    bool has_out, has_codes, nib, l1_given;
    int slots;                         // resident stream workgroups; 0: ask the device when needed
};
struct ChunkPlan {                     // one chunk of at most kMaxGridY clients (segments / phased)
    int64_t nj;
    bool seg;
    int32_t prefixed, R, nseg;
};
struct UnbiasedPlan {
    int32_t form;                      // UQ_FORM_*
    bool V, Q, C, CV, l1_given;
    int64_t chunks;
    ChunkPlan last;                    // the last chunk (chunked forms; otherwise nj = n, R = tiles)
    int32_t tiles;
    size_t agg_off, map0_off, map1_off, rec_off, cnt_off;
};

int chunk_plan(const PlanIn& in, const UnbiasedPlan& p, int64_t j0, ChunkPlan* c) {
    c->nj = std::min<int64_t>(kMaxGridY, in.n - j0);
    const int64_t total_tiles = c->nj * (int64_t)p.tiles;
    c->seg = p.V && in.d <= ((int64_t)1 << 29) && total_tiles >= kSegMinTiles;
    c->R = 1;
    c->nseg = 1;
    if (c->seg) {
        // segmented stream: runs of R tiles per workgroup, ~4 resident workgroups per CU
        int slots = in.slots;
        if (slots <= 0) {
            const int rc = stream_slots(&slots);
            if (rc) return rc;
        }
        // at most `slots` workgroups in all, so that they run as one wave: ceil(total / slots)
        // tiles each made nj * ceil(tiles / R) > slots workgroups for most nj (101 x 2^22:
        // 1111 of 1024 slots, the last 87 workgroups a second round of R tiles)
        const int64_t segs = std::max<int64_t>(1, slots / c->nj);
        c->R = (int32_t)((p.tiles + segs - 1) / segs);
        c->nseg = (p.tiles + c->R - 1) / c->R;
    }
    c->prefixed = c->nj >= 4 ? 1 : 0;
    return UQ_OK;
}

// in: a call with n > 0 and d > 0 whose pitches were checked; w: its workspace layout.
int plan_unbiased(const PlanIn& in, const WsLayout& w, UnbiasedPlan* p) {
    *p = UnbiasedPlan{};
    if (!in.has_out && !in.has_codes) return fail(UQ_E_INVALID, "nothing to write: out and codes are both NULL");
    const int64_t n = in.n, d = in.d;
    p->tiles = w.tiles;
    p->agg_off = w.agg_off;
    p->map0_off = w.incl_off;
    p->map1_off = w.map1_off;
    p->rec_off = w.rec_off;
    p->cnt_off = w.cnt_off;
    p->Q = in.has_out;
    p->C = in.has_codes;
    p->l1_given = in.l1_given;
    // rows are 16-byte aligned when d % 4 == 0, or when there is only one row
    p->V = in.x16 && (!in.has_out || in.out16) && ((d % 4 == 0 && in.ldo % 4 == 0) || n == 1);
    p->CV = !in.has_codes || (in.codes16 && d % 16 == 0 && (in.ldc % 16 == 0 || n == 1));
    p->chunks = 1;
    p->last = ChunkPlan{n, false, 0, w.tiles, 1};
    if (!in.nib && d <= kSmallL1Max && p->V && n <= 0x7FFFFFFF) {
        p->form = UQ_FORM_SMALL;
        return UQ_OK;
    }
    const bool stream_form = n >= kStreamMinClients && p->V && d <= ((int64_t)1 << 29);
    if (in.nib) {
        if (!stream_form || !in.has_out || !in.has_codes)
            return fail(UQ_E_INVALID, "internal: 4-bit codes outside the stream form");
        p->form = UQ_FORM_STREAM_NIBBLES;
        p->CV = true;
        return UQ_OK;
    }
    if (stream_form) {
        p->form = UQ_FORM_STREAM;
        return UQ_OK;
    }
    // Small batches: clients go in chunks of at most kMaxGridY.
    p->chunks = (n + kMaxGridY - 1) / kMaxGridY;
    const int rc = chunk_plan(in, *p, (p->chunks - 1) * kMaxGridY, &p->last);
    if (rc) return rc;
    p->form = p->last.seg ? UQ_FORM_SEGMENTS : UQ_FORM_PHASED;
    return UQ_OK;
}

bool bad_pitches(bool has_out, int64_t ldo, bool has_codes, int64_t ldc, int64_t d, bool nib) {
    return (has_out && ldo < d) || (has_codes && ldc < (nib ? d / 2 : d));
}

// 4-bit codes exist in the stream form only, whole mean threads per row
bool bad_nibble_shape(int64_t n, int64_t d) {
    return n < kStreamMinClients || d % kNibAlign != 0 || d > ((int64_t)1 << 29);
}
int nibble_shape_error() {
    return fail(UQ_E_INVALID, "4-bit codes need n >= 256 and d a multiple of 4096 (<= 2^29)");
}

thread_local UnbiasedPlan t_last_plan{};     // uq_test_last_unbiased_plan

int export_plan(const UnbiasedPlan& p, int64_t* out, int32_t cap) {
    if (!out || cap < 0) return fail(UQ_E_INVALID, "null plan output");
    const int64_t f[UQ_PLAN_FIELDS] = {
        p.form, p.V, p.Q, p.C, p.CV, p.l1_given, p.chunks, p.last.nj, p.last.prefixed, p.last.R, p.last.nseg,
        p.tiles, (int64_t)p.agg_off, (int64_t)p.map0_off, (int64_t)p.map1_off, (int64_t)p.rec_off, (int64_t)p.cnt_off,
        (int64_t)sizeof(TileRec), kRecPerClient, kRecClients, kRecEvents, kFoldEvents};
    for (int i = 0; i < std::min<int32_t>(cap, UQ_PLAN_FIELDS); ++i) out[i] = f[i];
    return UQ_OK;
}

// AS:609-641 for a batch.  X: per-client draws (device), or nullptr with n == 1 and the one
// draw passed by value in Xval (the per-call drop-in: no host-to-device copy of X).
// Row j of q at out + j*ldo, of the codes at codes + j*ldc (ldo, ldc >= d: row pitches let the
// caller stagger the rows' physical placement, see DMEPipeline).
// nib: codes as 4-bit fields (uq_type_unbiased_nibbles_ld_f32; the caller checked the stream
// form's conditions and ldc is then the row pitch in bytes of the packed rows).
int unbiased_codes_impl(const float* x, float* out, int64_t ldo, int8_t* codes, int64_t ldc, int32_t* overflow,
                        int64_t n, int64_t d, int64_t m, const float* X, float Xval, const float* l1, float* l1_out,
                        int32_t T, void* ws, size_t ws_bytes, void* stream, bool nib = false) {
    L1Plan plan;
    WsLayout w;
    int rc = check_common(x, n, d, T, ws, ws_bytes, &plan, &w);
    if (rc) return rc;
    t_last_plan = UnbiasedPlan{};
    if (m < 0) return fail(UQ_E_INVALID, "m must be >= 0");
    if (bad_pitches(out, ldo, codes, ldc, d, nib)) return fail(UQ_E_INVALID, "row pitches must be >= d");
    if (n == 0 || d == 0) return UQ_OK;
    if (!X && n != 1) return fail(UQ_E_INVALID, "null X");
    const PlanIn in{n, d, ldo, ldc, aligned16(x), aligned16(out), aligned16(codes), out != nullptr, codes != nullptr,
                    nib, l1 != nullptr, 0};
    UnbiasedPlan P;
    rc = plan_unbiased(in, w, &P);
    if (rc) return rc;
    if (codes && !overflow) return fail(UQ_E_INVALID, "codes need a kmax[n] array");
    t_last_plan = P;
    hipStream_t st = (hipStream_t)stream;
    const float* l1use = l1;
    const float fm = (float)m;   // torch casts the Python int to f32 for `m * p` and `/ m`
    const bool vec4 = P.V, cvec = P.CV;
    if (P.form == UQ_FORM_SMALL) {
        // shorter than GRAIN: L1 (one torch cascade for any thread count) and the exact scan
        // in one workgroup per client, one launch
        if (!select_qc(out, codes, cvec, [&](auto Q, auto C, auto CV) {
                hipLaunchKernelGGL((quantize_small_kernel<Q(), C(), CV()>), dim3((unsigned)n), dim3(kQBlock), 0, st, x,
                                   out, codes, overflow, d, w.tiles, fm, X, Xval, l1, l1_out, ldo, ldc);
            }))
            return bad_selector();
        return hip_check(hipGetLastError(), "quantize_small_kernel launch");      // (l1_out written there)
    }
    if (!l1use) {
        float* l1buf = w.at<float>(ws, w.l1_off);
        rc = launch_l1(x, n, d, plan, w.at<float>(ws, w.part_off), l1buf, st);
        if (rc) return rc;
        l1use = l1buf;
    }
    if (l1_out && l1_out != l1use) {
        rc = hip_check(hipMemcpyAsync(l1_out, l1use, n * sizeof(float), hipMemcpyDeviceToDevice, st), "copy l1");
        if (rc) return rc;
    }
    const bool stream_form = P.form == UQ_FORM_STREAM || P.form == UQ_FORM_STREAM_NIBBLES;
    if (codes && !stream_form) {          // the stream form stores each client's kmax itself
        rc = hip_check(hipMemsetAsync(overflow, 0, n * sizeof(int32_t), st), "memset kmax");
        if (rc) return rc;
    }
    if (P.form == UQ_FORM_STREAM_NIBBLES) {
        hipLaunchKernelGGL((quantize_stream_kernel<true, true, true, true>), dim3((unsigned)n), dim3(kQBlock), 0, st, x,
                           out, codes, overflow, d, w.tiles, fm, X, Xval, l1use, w.tiles, 1, nullptr, ldo, ldc);
        return hip_check(hipGetLastError(), "quantize_stream_kernel (4-bit codes) launch");
    }
    if (P.form == UQ_FORM_STREAM) {
        // enough clients to fill the GPU: one workgroup per client vector
        if (!select_qc(out, codes, cvec, [&](auto Q, auto C, auto CV) {
                hipLaunchKernelGGL((quantize_stream_kernel<Q(), C(), CV()>), dim3((unsigned)n), dim3(kQBlock), 0, st, x,
                                   out, codes, overflow, d, w.tiles, fm, X, Xval, l1use, w.tiles, 1, nullptr, ldo, ldc);
            }))
            return bad_selector();
        return hip_check(hipGetLastError(), "quantize_stream_kernel launch");
    }
    // Small batches: approximate sums -> approximate prefixes -> exact maps -> exact fold
    // -> outputs (see "small-batch forms").  Clients go in chunks of at most kMaxGridY.
    for (int64_t j0 = 0; j0 < n; j0 += kMaxGridY) {
        ChunkPlan ck;
        rc = chunk_plan(in, P, j0, &ck);
        if (rc) return rc;
        const int64_t nj = ck.nj;
        const float* xj = x + j0 * d;
        float* outj = out ? out + j0 * ldo : nullptr;
        int8_t* codesj = codes ? codes + j0 * ldc : nullptr;
        int32_t* ovj = codes ? overflow + j0 : nullptr;
        const float* Xj = X ? X + j0 : nullptr;
        const float* l1j = l1use + j0;
        uint64_t* agg = w.tile_row(ws, w.agg_off, j0);
        uint64_t* pre = w.tile_row(ws, w.incl_off, j0);
        uint64_t* map1 = w.tile_row(ws, w.map1_off, j0);
        TileRec* recs = w.at<TileRec>(ws, w.rec_off);
        uint32_t* reccnt = w.at<uint32_t>(ws, w.cnt_off);     // zeroed by the tile-sum kernels
        const bool seg = ck.seg;
        const dim3 tgrid((unsigned)w.tiles, (unsigned)nj);
        const int32_t R = ck.R, nseg = ck.nseg;
        if (seg) {
            hipLaunchKernelGGL(agg_stream_kernel, dim3((unsigned)(nj * nseg)), dim3(kQBlock), 0, st, xj, d, w.tiles, fm,
                               l1j, R, nseg, agg, reccnt);
        } else if (vec4) {
            hipLaunchKernelGGL(tile_agg_kernel<true>, tgrid, dim3(kQBlock), 0, st, xj, d, w.tiles, fm, l1j, agg, reccnt);
        } else {
            hipLaunchKernelGGL(tile_agg_kernel<false>, tgrid, dim3(kQBlock), 0, st, xj, d, w.tiles, fm, l1j, agg, reccnt);
        }
        rc = hip_check(hipGetLastError(), "tile sums launch");
        if (rc) return rc;
        const int32_t prefixed = ck.prefixed;
        if (prefixed) {
            hipLaunchKernelGGL(tile_prefix_kernel, dim3((unsigned)nj), dim3(kQBlock), 0, st, agg, w.tiles);
            rc = hip_check(hipGetLastError(), "tile_prefix_kernel launch");
            if (rc) return rc;
        }
        const auto map_and_fold = [&](auto V) {
            hipLaunchKernelGGL((tile_map_kernel<V()>), tgrid, dim3(kQBlock), 0, st, xj, d, w.tiles, fm, l1j, agg, pre, map1,
                               recs, reccnt, prefixed);
            const int e = hip_check(hipGetLastError(), "tile_map_kernel launch");
            if (e) return e;
            hipLaunchKernelGGL((exact_fold_kernel<V()>), dim3((unsigned)nj), dim3(kQBlock), 0, st, xj, d, w.tiles, fm, l1j,
                               pre, map1, agg, recs, reccnt);
            return hip_check(hipGetLastError(), "exact_fold_kernel launch");
        };
        rc = vec4 ? map_and_fold(Flag<true>{}) : map_and_fold(Flag<false>{});
        if (rc) return rc;
        pre = agg;                                             // the fold's exact prefixes
        if (seg) {
            if (!select_qc(out, codes, cvec, [&](auto Q, auto C, auto CV) {
                    hipLaunchKernelGGL((quantize_stream_kernel<Q(), C(), CV()>), dim3((unsigned)(nj * nseg)),
                                       dim3(kQBlock), 0, st, xj, outj, codesj, ovj, d, w.tiles, fm, Xj, Xval, l1j, R, nseg,
                                       pre, ldo, ldc);
                }))
                return bad_selector();
            rc = hip_check(hipGetLastError(), "quantize_stream_kernel (segments) launch");
            if (rc) return rc;
            continue;
        }
        if (!select_vqc(vec4, out, codes, cvec, [&](auto V, auto Q, auto C, auto CV) {
                hipLaunchKernelGGL((tile_out_kernel<V(), Q(), C(), CV()>), tgrid, dim3(kQBlock), 0, st, xj, outj, codesj,
                                   ovj, d, w.tiles, fm, Xj, Xval, l1j, pre, ldo, ldc);
            }))
            return bad_selector();
        rc = hip_check(hipGetLastError(), "tile_out_kernel launch");
        if (rc) return rc;
    }
    return UQ_OK;
}

}  // namespace

extern "C" {

int uq_type_unbiased_codes_ld_f32(const float* x, float* out, int64_t ldq, int8_t* codes, int64_t ldc,
                                  int32_t* overflow, int64_t n, int64_t d, int64_t m, const float* X, const float* l1,
                                  float* l1_out, int32_t T, void* ws, size_t ws_bytes, void* stream) {
    if (n > 0 && d > 0 && !X) return fail(UQ_E_INVALID, "null X");
    return unbiased_codes_impl(x, out, ldq, codes, ldc, overflow, n, d, m, X, 0.0f, l1, l1_out, T, ws, ws_bytes,
                               stream);
}

int uq_type_unbiased_nibbles_ld_f32(const float* x, float* out, int64_t ldq, uint8_t* nib, int64_t ldn,
                                    int32_t* kmax, int64_t n, int64_t d, int64_t m, const float* X, const float* l1,
                                    float* l1_out, int32_t T, void* ws, size_t ws_bytes, void* stream) {
    if (n < 0 || d < 0) return fail(UQ_E_INVALID, "n and d must be >= 0");
    if (n == 0 || d == 0) return UQ_OK;
    if (!x || !out || !nib || !kmax || !X) return fail(UQ_E_INVALID, "null pointer (x, out, codes, kmax and X are required)");
    if (bad_nibble_shape(n, d)) return nibble_shape_error();
    if (ldq < d || ldq % 4 != 0 || ldn < d / 2 || ldn % 16 != 0 || !aligned16(x) || !aligned16(out) || !aligned16(nib))
        return fail(UQ_E_INVALID, "4-bit codes need 16-byte aligned rows: ldq >= d, ldq % 4 == 0, ldn >= d/2, ldn % 16 == 0");
    return unbiased_codes_impl(x, out, ldq, (int8_t*)nib, ldn, kmax, n, d, m, X, 0.0f, l1, l1_out, T, ws, ws_bytes,
                               stream, true);
}

int uq_nibbles_q_mean_ld_f32(const uint8_t* nib, int64_t ldn, const float* q, int64_t ldq, const float* l1,
                             const int32_t* kmax, int64_t n, int64_t d, int64_t m, float n_div, int32_t accumulate,
                             float* est, void* stream) {
    if (n < 0 || d < 0 || m < 0) return fail(UQ_E_INVALID, "n, d and m must be >= 0");
    if (d == 0) return UQ_OK;
    if (!est || (n > 0 && (!nib || !l1 || !kmax || !q))) return fail(UQ_E_INVALID, "null pointer (q is required)");
    if (d % kNibAlign != 0 || ldq < d || ldq % 4 != 0 || ldn < d / 2 || ldn % 4 != 0 || !aligned16(est) ||
        (n > 0 && (!aligned16(q) || ((uintptr_t)nib & 3u))))
        return fail(UQ_E_INVALID, "4-bit code mean: d % 4096 == 0, ldq >= d (multiple of 4), ldn >= d/2 (multiple of 4), "
                                  "16-byte aligned est and q");
    const int64_t blocks = d / (kCodesMeanThreads * kMeanCpt);
    if (blocks > 0x7FFFFFFF) return fail(UQ_E_INVALID, "d too large");
    hipLaunchKernelGGL(nibbles_mean_kernel, dim3((unsigned)blocks), dim3(kCodesMeanThreads), 0, (hipStream_t)stream, nib,
                       ldn, l1, kmax, n, d, (float)m, n_div, accumulate, est, q, ldq);
    return hip_check(hipGetLastError(), "nibbles_mean_kernel launch");
}

int uq_type_unbiased_codes_f32(const float* x, float* out, int8_t* codes, int32_t* overflow, int64_t n, int64_t d,
                               int64_t m, const float* X, const float* l1, float* l1_out, int32_t T, void* ws,
                               size_t ws_bytes, void* stream) {
    return uq_type_unbiased_codes_ld_f32(x, out, d, codes, d, overflow, n, d, m, X, l1, l1_out, T, ws, ws_bytes,
                                         stream);
}

int uq_type_unbiased_vec_f32(const float* x, float* out, int64_t d, int64_t m, float X, int32_t T, void* ws,
                             size_t ws_bytes, void* stream) {
    if (d > 0 && !out) return fail(UQ_E_INVALID, "null out");
    return unbiased_codes_impl(x, out, d, nullptr, d, nullptr, 1, d, m, nullptr, X, nullptr, nullptr, T, ws, ws_bytes,
                               stream);
}

int uq_type_unbiased_f32(const float* x, float* out, int64_t n, int64_t d, int64_t m, const float* X,
                         const float* l1, float* l1_out, int32_t T, void* ws, size_t ws_bytes,
                         void* stream) {
    if (n > 0 && d > 0 && !out) return fail(UQ_E_INVALID, "null out");
    return uq_type_unbiased_codes_f32(x, out, nullptr, nullptr, n, d, m, X, l1, l1_out, T, ws, ws_bytes, stream);
}

int uq_codes_decode_f32(const int8_t* codes, const float* l1, int64_t n, int64_t d, int64_t m, float* out,
                        void* stream) {
    return uq_codes_decode_form_f32(codes, l1, n, d, m, UQ_FORM_UNBIASED, out, stream);
}

int uq_codes_decode_form_f32(const int8_t* codes, const float* l1, int64_t n, int64_t d, int64_t m, int32_t form,
                             float* out, void* stream) {
    if (n < 0 || d < 0 || m < 0) return fail(UQ_E_INVALID, "n, d and m must be >= 0");
    if (form != UQ_FORM_UNBIASED && form != UQ_FORM_BIASED) return fail(UQ_E_INVALID, "unknown codes form");
    if (form == UQ_FORM_BIASED && m < 1) return fail(UQ_E_INVALID, "m must be >= 1 for biased codes");
    if (n == 0 || d == 0) return UQ_OK;
    if (!codes || !l1 || !out) return fail(UQ_E_INVALID, "null pointer");
    hipStream_t st = (hipStream_t)stream;
    const int64_t chunks = (d + kDecChunk - 1) / kDecChunk;
    if (chunks > 0x7FFFFFFF) return fail(UQ_E_INVALID, "d too large");
    const bool vec = aligned16(codes) && aligned16(out) && d % 16 == 0;
    dim3 grid((unsigned)chunks, (unsigned)n);
    if (form == UQ_FORM_BIASED) {
        if (vec)
            hipLaunchKernelGGL(codes_decode_biased_kernel<true>, grid, dim3(256), 0, st, codes, l1, d, (float)m, out);
        else
            hipLaunchKernelGGL(codes_decode_biased_kernel<false>, grid, dim3(256), 0, st, codes, l1, d, (float)m, out);
    } else if (vec)
        hipLaunchKernelGGL(codes_decode_kernel<true>, grid, dim3(256), 0, st, codes, l1, d, (float)m, out);
    else
        hipLaunchKernelGGL(codes_decode_kernel<false>, grid, dim3(256), 0, st, codes, l1, d, (float)m, out);
    return hip_check(hipGetLastError(), "codes_decode_kernel launch");
}

int uq_codes_q_mean_ld_f32(const int8_t* codes, int64_t ldc, const float* q, int64_t ldq, const float* l1,
                           const int32_t* kmax, int64_t n, int64_t d, int64_t m, float n_div, int32_t accumulate,
                           float* est, void* stream) {
    return uq_codes_mean_form_f32(codes, ldc, q, ldq, l1, kmax, n, d, m, UQ_FORM_UNBIASED, n_div, accumulate, est, stream);
}

int uq_codes_mean_form_f32(const int8_t* codes, int64_t ldc, const float* q, int64_t ldq, const float* l1,
                           const int32_t* kmax, int64_t n, int64_t d, int64_t m, int32_t form, float n_div,
                           int32_t accumulate, float* est, void* stream) {
    if (n < 0 || d < 0 || m < 0) return fail(UQ_E_INVALID, "n, d and m must be >= 0");
    if (form != UQ_FORM_UNBIASED && form != UQ_FORM_BIASED) return fail(UQ_E_INVALID, "unknown codes form");
    if (form == UQ_FORM_BIASED && m < 1) return fail(UQ_E_INVALID, "m must be >= 1 for biased codes");
    if (d == 0) return UQ_OK;
    if (!est || (n > 0 && (!codes || !l1 || !kmax))) return fail(UQ_E_INVALID, "null pointer");
    if (q && ldq < d) return fail(UQ_E_INVALID, "ldq must be >= d");
    if (ldc < d) return fail(UQ_E_INVALID, "ldc must be >= d");
    hipStream_t st = (hipStream_t)stream;
    const bool vec = (n == 0 || aligned16(codes)) && aligned16(est) && d % 16 == 0 && ldc % 16 == 0;
    const int64_t blocks = (d + kCodesMeanThreads * kMeanCpt - 1) / (kCodesMeanThreads * kMeanCpt);
    if (blocks > 0x7FFFFFFF) return fail(UQ_E_INVALID, "d too large");
    const dim3 tb(kCodesMeanThreads);
    if (form == UQ_FORM_BIASED) {
        if (vec && d % (kCodesMeanThreads * kMeanCpt) == 0)
            hipLaunchKernelGGL((codes_mean_biased_kernel<true, true>), dim3((unsigned)blocks), tb, 0, st, codes, ldc, l1, kmax,
                               n, d, (float)m, n_div, accumulate, est, q, ldq);
        else if (vec)
            hipLaunchKernelGGL(codes_mean_biased_kernel<true>, dim3((unsigned)blocks), tb, 0, st, codes, ldc, l1, kmax, n, d,
                               (float)m, n_div, accumulate, est, q, ldq);
        else
            hipLaunchKernelGGL(codes_mean_biased_kernel<false>, dim3((unsigned)blocks), tb, 0, st, codes, ldc, l1, kmax, n, d,
                               (float)m, n_div, accumulate, est, q, ldq);
        return hip_check(hipGetLastError(), "codes_mean_biased_kernel launch");
    }
    if (vec && d % (kCodesMeanThreads * kMeanCpt) == 0)
        hipLaunchKernelGGL((codes_mean_kernel<true, true>), dim3((unsigned)blocks), tb, 0, st, codes, ldc, l1, kmax, n,
                           d, (float)m, n_div, accumulate, est, q, ldq);
    else if (vec)
        hipLaunchKernelGGL(codes_mean_kernel<true>, dim3((unsigned)blocks), tb, 0, st, codes, ldc, l1, kmax, n, d,
                           (float)m, n_div, accumulate, est, q, ldq);
    else
        hipLaunchKernelGGL(codes_mean_kernel<false>, dim3((unsigned)blocks), tb, 0, st, codes, ldc, l1, kmax, n, d,
                           (float)m, n_div, accumulate, est, q, ldq);
    return hip_check(hipGetLastError(), "codes_mean_kernel launch");
}

int uq_codes_q_mean_f32(const int8_t* codes, const float* q, int64_t ldq, const float* l1, const int32_t* kmax,
                        int64_t n, int64_t d, int64_t m, float n_div, int32_t accumulate, float* est, void* stream) {
    return uq_codes_q_mean_ld_f32(codes, d, q, ldq, l1, kmax, n, d, m, n_div, accumulate, est, stream);
}

int uq_codes_mean_f32(const int8_t* codes, const float* l1, const int32_t* kmax, int64_t n, int64_t d, int64_t m,
                      float n_div, int32_t accumulate, float* est, void* stream) {
    return uq_codes_q_mean_f32(codes, nullptr, d, l1, kmax, n, d, m, n_div, accumulate, est, stream);
}

int uq_client_mean_f32(const float* q, int64_t n, int64_t d, int64_t ld, float n_div, int32_t accumulate,
                       float* est, void* stream) {
    if (n < 0 || d < 0) return fail(UQ_E_INVALID, "n and d must be >= 0");
    if (ld < d) return fail(UQ_E_INVALID, "ld must be >= d");
    if (d == 0) return UQ_OK;
    if (!est || (n > 0 && !q)) return fail(UQ_E_INVALID, "null pointer");
    hipStream_t st = (hipStream_t)stream;
    const bool vec4 = (n == 0 || aligned16(q)) && aligned16(est) && (d % 4 == 0) && (ld % 4 == 0);
    const int64_t threads = (d + 3) / 4;
    dim3 grid((unsigned)((threads + kMeanThreads - 1) / kMeanThreads));
    if (vec4)
        hipLaunchKernelGGL(client_mean_kernel<true>, grid, dim3(kMeanThreads), 0, st, q, n, d, ld, n_div, accumulate, est);
    else
        hipLaunchKernelGGL(client_mean_kernel<false>, grid, dim3(kMeanThreads), 0, st, q, n, d, ld, n_div, accumulate, est);
    return hip_check(hipGetLastError(), "client_mean_kernel launch");
}

int uq_type_unbiased_mean_f32(const float* x, float* out, int64_t n, int64_t d, int64_t m, const float* X,
                              const float* l1, int32_t T, float n_div, int32_t accumulate, float* est,
                              void* ws, size_t ws_bytes, void* stream) {
    if (!out) return fail(UQ_E_INVALID, "out must be non-NULL in this version");
    int rc = uq_type_unbiased_f32(x, out, n, d, m, X, l1, nullptr, T, ws, ws_bytes, stream);
    if (rc) return rc;
    return uq_client_mean_f32(out, n, d, d, n_div, accumulate, est, stream);
}

int uq_test_unbiased_plan(int64_t n, int64_t d, int64_t ldq, int64_t ldc, int32_t x_aligned, int32_t out_aligned,
                          int32_t codes_aligned, int32_t has_out, int32_t has_codes, int32_t nib, int32_t l1_given,
                          int32_t slots, int64_t* plan_out, int32_t cap) {
    L1Plan l1plan;
    if (n < 0 || d < 0) return fail(UQ_E_INVALID, "n and d must be >= 0");
    if (n > (int64_t)1 << 31 || d > (int64_t)1 << 40) return fail(UQ_E_INVALID, "n or d too large");
    if (slots < 0) return fail(UQ_E_INVALID, "slots must be >= 0");
    if (!make_plan(d, 1, &l1plan)) return fail(UQ_E_INVALID, "cannot build L1 plan");
    const WsLayout w = layout(n, d, l1plan);       // (the offsets reported do not depend on torch_threads)
    if ((int64_t)w.tiles * n > 0xFFFFFFFFll) return fail(UQ_E_INVALID, "batch too large for one call");
    if (bad_pitches(has_out, ldq, has_codes, ldc, d, nib)) return fail(UQ_E_INVALID, "row pitches must be >= d");
    UnbiasedPlan P{};
    if (n > 0 && d > 0) {
        if (nib && bad_nibble_shape(n, d)) return nibble_shape_error();
        const PlanIn in{n, d, ldq, ldc, x_aligned != 0, out_aligned != 0, codes_aligned != 0, has_out != 0,
                        has_codes != 0, nib != 0, l1_given != 0, slots};
        const int rc = plan_unbiased(in, w, &P);
        if (rc) return rc;
    }
    return export_plan(P, plan_out, cap);
}

int uq_test_last_unbiased_plan(int64_t* plan_out, int32_t cap) { return export_plan(t_last_plan, plan_out, cap); }

}  // extern "C"
