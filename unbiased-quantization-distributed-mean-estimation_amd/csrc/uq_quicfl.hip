// uq_quicfl.hip — QUIC-FL: the jump plans, the launchers of uq_quicfl_kernels.h and the C API
// of the sender (uq_quicfl_compress_f32, uq_quicfl_quantize_f32) and the receiver
// (uq_quicfl_receive_*), and uq_xxh64 (the sender's prng seed).  The RHT and the norm run in
// uq_eden.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <map>
#include <mutex>
#include <tuple>
#include <vector>

#include "uq_internal.h"
#include "uq_quicfl_kernels.h"

// test hooks of the QUIC-FL kernels (never set by the library itself): bit 0 makes every run
// of the few-message team kernels skip its waits and report UQ_QFL_TIMEOUT; bit 1 sends every
// call to the one-wave-per-message kernels (so a test can compare both forms on one message)
static std::atomic<int> g_quicfl_hooks{0};

// The jump path (KQ0s + KQ0j + KQ1j + KQ1f, uq_quicfl_kernels.h) for few messages: R runs of L
// rounds per message, R from a cost model of the phases (measured round-5 constants): the
// streams (~20 us), the jumps (~tJ of the whole GPU per jump) and a round of passes A + B on one
// wave (~tR; a run wave per SIMD).  The one-wave kernel when the model gives the jumps no gain.
struct QflJumpPlan {
    bool use = false;
    int32_t R = 0;
    int64_t L = 0, qL = 0;
};

// Up to 1024 run waves a wave per SIMD; up to 2048 two (quicfl_send_runs_kernel<., true>), a
// round then costing ~1.3 tR (round 6, profiles/r6k_* .. r6x_*: 512 x 2^20 compress 12.0 -> 7.6
// ms, 1024 x 2^20 14.4 -> 12.9 with R = 2 once the runs' pass A moved to the side stream and the
// counting pass went; 256 x 2^22 round trip 24.2 -> 17.5).
constexpr int64_t kQfJumpMaxN = 1024;
constexpr int64_t kQfRunWaves1 = 1024, kQfRunWaves2 = 2048;
static QflJumpPlan qfl_jump_plan(int64_t n, int64_t D) {
    QflJumpPlan p;
    const int64_t nch = (D + kMtN - 1) / kMtN;
    if (n < 1 || n > kQfJumpMaxN || nch < 8 || D > ((int64_t)1 << 28)) return p;
    const double tS = 20.0, tJ = 0.12, tR = 7.5, f2 = 1.3;
    double best = 1e300;
    for (int64_t R = 1; R <= 1024 && R <= nch; ++R) {
        const int64_t L = (nch + R - 1) / R, Ru = (nch + L - 1) / L;
        if (Ru != R || n * R > kQfRunWaves2) continue;
        const double t = tS + (double)(n * (3 * R - 2)) * tJ + (double)L * tR * (n * R > kQfRunWaves1 ? f2 : 1.0);
        if (t < best) {
            best = t;
            p.R = (int32_t)R;
            p.L = L;
        }
    }
    // against: up to 128 messages the team kernel as round 5 measured it; 129-256 the team kernel
    // at ~2.85 us per round, the model ~1.4x optimistic (r6l: 256 x 2^20 team 5.5 / jump 5.9 ms,
    // 2^21 11.3 / 10.3, 2^22 round trip 24.3 / 18.7); above, a wave per message
    if (n <= 128 || n > kQfTeamMaxN)
        p.use = best < 0.8 * (double)((n + 1023) / 1024) * (double)nch * tR;
    else
        p.use = best < 2.0 * (double)nch;
    p.qL = ((int64_t)kMtN + D) / kMtN;               // block of the first pass-B local word (qfl_ctx)
    return p;
}

// The receiver's jump path: one stream, one jump per run; a round (one wave: the h word, the
// table gather, X, the mask and the exact value) ~tR, ~1.3 tR at two waves per SIMD (more than
// 1024 run waves; 512 x 2^20 decompress 5.60 -> 3.53 ms, 1024 x 2^20 7.4 -> 6.4, profiles/r6r_*,
// r6w_*, r6x_*).  Taken when it beats the team kernel (~1 us per round of the h scout's twists
// and the runs behind it).
static QflJumpPlan qfl_recv_jump_plan(int64_t n, int64_t D) {
    QflJumpPlan p;
    const int64_t nch = (D + kMtN - 1) / kMtN;
    if (n < 1 || n > kQfJumpMaxN || nch < 8 || D > ((int64_t)1 << 28)) return p;
    const double tS = 20.0, tJ = 0.12, tR = 3.0;
    double best = 1e300;
    for (int64_t R = 1; R <= 1024 && R <= nch; ++R) {
        const int64_t L = (nch + R - 1) / R, Ru = (nch + L - 1) / L;
        if (Ru != R || n * R > kQfRunWaves2) continue;                 // (its kernels fit 2 waves per SIMD)
        const double t = tS + (double)(n * (R - 1)) * tJ + (double)L * tR * (n * R > kQfRunWaves1 ? 1.3 : 1.0);
        if (t < best) {
            best = t;
            p.R = (int32_t)R;
            p.L = L;
        }
    }
    // against the team kernel (~1 us per round) up to 256 messages, a wave per message (~tR per
    // round, one wave per SIMD) above
    p.use = best < 0.8 * (double)nch * (n <= kQfTeamMaxN ? 1.0 : tR);
    return p;
}

extern "C" {

int uq_mtpoly_progression(int64_t b0, int64_t step, int32_t count, uint32_t* out);   // uq_mt_poly.cpp

int uq_test_set_quicfl_hooks(int flags) { return g_quicfl_hooks.exchange(flags & 7); }

// t^(624 b) mod phi for the plan's run starts, on the device, cached per (device, qL, L, R):
// rows [0, R) = polyA (row r: b = r L - 1; row 0 unused), rows [R, 2R) = polyB (b = qL + r L - 1)
static int qfl_jump_polys(const QflJumpPlan& p, bool a_only, const uint32_t** out) {
    static std::mutex mu;
    static std::map<std::tuple<int, int64_t, int64_t, int32_t>, uint32_t*> cache;
    int dev = 0;
    int rc = hip_check(hipGetDevice(&dev), "hipGetDevice");
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(mu);
    const auto key = std::make_tuple(dev, a_only ? (int64_t)-1 : p.qL, p.L, p.R);   // (A rows only: no qL)
    auto it = cache.find(key);
    if (it != cache.end()) {
        *out = it->second;
        return UQ_OK;
    }
    std::vector<uint32_t> h((size_t)2 * p.R * kMtN, 0u);
    if ((p.R > 1 && uq_mtpoly_progression(p.L - 1, p.L, p.R - 1, h.data() + kMtN)) ||
        (!a_only && uq_mtpoly_progression(p.qL - 1, p.L, p.R, h.data() + (size_t)p.R * kMtN)))
        return fail(UQ_E_INVALID, "MT19937 jump polynomials unavailable");
    // Entries live for the life of the process: a pointer handed out above may still be waiting
    // to be launched on another thread's stream, so nothing here is ever freed.  The key space is
    // one entry per (device, layout) in use -- 2 R * 624 words each, a few KB to ~1 MB.
    uint32_t* d = nullptr;
    rc = hip_check(hipMalloc(&d, h.size() * sizeof(uint32_t)), "hipMalloc jump polynomials");
    if (rc) return rc;
    rc = hip_check(hipMemcpy(d, h.data(), h.size() * sizeof(uint32_t), hipMemcpyHostToDevice), "copy jump polynomials");
    if (rc) {
        (void)hipFree(d);
        return rc;
    }
    cache.emplace(key, d);
    *out = d;
    return UQ_OK;
}

static int quicfl_recv_jump(const QflRecvArgs& r, int32_t x_kind, const QflJumpPlan& jp, char* wsb, hipStream_t st);

int uq_quicfl_receive_f32(const void* X, int32_t x_kind, int64_t n, int64_t D, const float* recv_table,
                          int32_t table_rows, int32_t h_len, const int32_t* prng_seeds, const uint8_t* exact_mask,
                          const float* exact_vals, int32_t exact_layout, const int32_t* exact_count, const float* scale,
                          float* out, int32_t* info, void* stream) {
    return uq_quicfl_receive_ws_f32(X, x_kind, n, D, recv_table, table_rows, h_len, prng_seeds, exact_mask, exact_vals,
                                    exact_layout, exact_count, scale, out, info, nullptr, 0, stream);
}

int uq_quicfl_receive_workspace_bytes(int64_t n, int64_t D, size_t* bytes_out) {
    if (!bytes_out) return fail(UQ_E_INVALID, "null bytes_out");
    if (n < 0 || D < 0) return fail(UQ_E_INVALID, "n and D must be >= 0");
    const QflJumpPlan p = qfl_recv_jump_plan(n, D);
    *bytes_out = p.use ? ((size_t)n * kMjX + (size_t)n * p.R * (kMjParts * kMtN + 2)) * sizeof(uint32_t) : 0;
    return UQ_OK;
}

int uq_quicfl_receive_ws_f32(const void* X, int32_t x_kind, int64_t n, int64_t D, const float* recv_table,
                             int32_t table_rows, int32_t h_len, const int32_t* prng_seeds, const uint8_t* exact_mask,
                             const float* exact_vals, int32_t exact_layout, const int32_t* exact_count,
                             const float* scale, float* out, int32_t* info, void* ws, size_t ws_bytes, void* stream) {
    if (n < 0 || D < 0) return fail(UQ_E_INVALID, "n and D must be >= 0");
    if (n > 65535) return fail(UQ_E_INVALID, "at most 65535 clients per call");
    if (D > ((int64_t)1 << 28)) return fail(UQ_E_INVALID, "at most 2^28 coordinates per message");
    if (x_kind < 0 || x_kind > 2) return fail(UQ_E_INVALID, "x_kind must be 0 (int64), 1 (uint8) or 2 (int32)");
    if (exact_layout != 0 && exact_layout != 1) return fail(UQ_E_INVALID, "exact_layout must be 0 (dense) or 1 (compact)");
    if (n == 0 || D == 0) return UQ_OK;
    if (!X || !recv_table || !prng_seeds || !scale || !out) return fail(UQ_E_INVALID, "null pointer");
    if ((exact_mask == nullptr) != (exact_vals == nullptr)) return fail(UQ_E_INVALID, "exact_mask and exact_vals go together");
    if (h_len < 1 || table_rows < 1 || (int64_t)h_len * table_rows > kQflTab)
        return fail(UQ_E_INVALID, "receiver table must hold 1..1024 entries");
    hipStream_t st = (hipStream_t)stream;
    QflRecvArgs r{};
    r.X = X;
    r.n = n;
    r.D = D;
    r.table = recv_table;
    r.tab_n = table_rows * h_len;
    r.h_len = h_len;
    r.prng_seeds = prng_seeds;
    r.exact_mask = exact_mask;
    r.exact_vals = exact_vals;
    r.compact = exact_layout;
    r.exact_count = exact_count;
    r.scale = scale;
    r.out = out;
    r.info = info;
    const int hooks = g_quicfl_hooks.load();
    r.force_timeout = hooks & 1;
    // few messages: every run at once from jumped blocks of the h stream (given a workspace), or
    // a workgroup per message (the h stream's scout + 7 runs); batches: a wave each
    const QflJumpPlan jp = qfl_recv_jump_plan(n, D);
    size_t need = 0;
    (void)uq_quicfl_receive_workspace_bytes(n, D, &need);
    if (!(hooks & 7) && jp.use && ws && ws_bytes >= need) return quicfl_recv_jump(r, x_kind, jp, (char*)ws, st);
    if (!(hooks & 2) && n <= kQfTeamMaxN && D >= (int64_t)kMtN * kQrRuns && D <= kQfTeamMaxD) {
        const dim3 grid((unsigned)n), block(64 * kQfTeamWaves);
        if (x_kind == 0) hipLaunchKernelGGL(quicfl_recv_team_kernel<0>, grid, block, 0, st, r);
        else if (x_kind == 1) hipLaunchKernelGGL(quicfl_recv_team_kernel<1>, grid, block, 0, st, r);
        else hipLaunchKernelGGL(quicfl_recv_team_kernel<2>, grid, block, 0, st, r);
        return hip_check(hipGetLastError(), "quicfl_recv_team_kernel launch");
    }
    const dim3 grid((unsigned)((n + kQfWavesPerWG - 1) / kQfWavesPerWG)), block(64 * kQfWavesPerWG);
    if (x_kind == 0) hipLaunchKernelGGL(quicfl_recv_wave_kernel<0>, grid, block, 0, st, r);
    else if (x_kind == 1) hipLaunchKernelGGL(quicfl_recv_wave_kernel<1>, grid, block, 0, st, r);
    else hipLaunchKernelGGL(quicfl_recv_wave_kernel<2>, grid, block, 0, st, r);
    return hip_check(hipGetLastError(), "quicfl_recv_wave_kernel launch");
}

// KQ0s + KQ0j (the h stream, one block per run) + KQ2c + KQ2j + KQ2f
static int quicfl_recv_jump(const QflRecvArgs& r, int32_t x_kind, const QflJumpPlan& jp, char* wsb, hipStream_t st) {
    const int64_t n = r.n;
    const uint32_t* polys = nullptr;
    int rc = qfl_jump_polys(jp, true, &polys);
    if (rc) return rc;
    uint32_t* xs = (uint32_t*)wsb;
    uint32_t* parts = xs + (size_t)n * kMjX;
    QflJumpArgs ja{};
    ja.prng_seeds = r.prng_seeds;
    ja.polyA = polys;
    ja.polyB = polys;                                    // (unused: one kind)
    ja.xs = xs;
    ja.parts = parts;
    ja.R = jp.R;
    ja.n = n;
    ja.nstreams = 1;
    ja.kinds = 1;
    hipLaunchKernelGGL(quicfl_stream_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, ja);
    if ((rc = hip_check(hipGetLastError(), "quicfl_stream_kernel launch"))) return rc;
    hipLaunchKernelGGL(quicfl_jump_kernel, dim3((unsigned)(n * jp.R * kMjParts)), dim3(256), 0, st, ja);
    if ((rc = hip_check(hipGetLastError(), "quicfl_jump_kernel launch"))) return rc;
    QflRunArgs ra{};
    ra.parts = parts;
    ra.runinfo = (int32_t*)(parts + (size_t)n * jp.R * kMjParts * kMtN);
    ra.R = jp.R;
    ra.L = jp.L;
    const dim3 rgrid((unsigned)((n * jp.R + kQfWavesPerWG - 1) / kQfWavesPerWG)), blk(64 * kQfWavesPerWG);
    hipLaunchKernelGGL(quicfl_recv_count_kernel, rgrid, blk, 0, st, r, ra);
    if ((rc = hip_check(hipGetLastError(), "quicfl_recv_count_kernel launch"))) return rc;
    if (x_kind == 0) hipLaunchKernelGGL(quicfl_recv_runs_kernel<0>, rgrid, blk, 0, st, r, ra);
    else if (x_kind == 1) hipLaunchKernelGGL(quicfl_recv_runs_kernel<1>, rgrid, blk, 0, st, r, ra);
    else hipLaunchKernelGGL(quicfl_recv_runs_kernel<2>, rgrid, blk, 0, st, r, ra);
    if ((rc = hip_check(hipGetLastError(), "quicfl_recv_runs_kernel launch"))) return rc;
    hipLaunchKernelGGL(quicfl_recv_fin_kernel, dim3((unsigned)((n + kQfWavesPerWG - 1) / kQfWavesPerWG)), blk, 0, st, r,
                       ra);
    return hip_check(hipGetLastError(), "quicfl_recv_fin_kernel launch");
}

int uq_quicfl_prepare_f32(const int32_t* X, int64_t n, int64_t D, const float* recv_table, int32_t table_rows,
                          int32_t h_len, const int32_t* prng_seeds, const uint8_t* exact_mask, const float* exact_vals,
                          const float* scale, float* out, void* stream) {
    return uq_quicfl_receive_f32(X, 2, n, D, recv_table, table_rows, h_len, prng_seeds, exact_mask, exact_vals, 0, nullptr,
                                 scale, out, nullptr, stream);
}

// ---- QUIC-FL sender ----------------------------------------------------------------------
// Workspace: the EDEN layout (rotated vectors, norms, segmented-norm region) + h [n][D] u8 +
// the jump path's blocks [n][R][3][624] u32 and run records [n][R][2] i32.
static size_t quicfl_h_off(int64_t n, int64_t dim) {
    return up256(rht_layout(n, dim).total);
}
static size_t quicfl_jump_off(int64_t n, int64_t dim) {
    return up256(quicfl_h_off(n, dim) + (size_t)n * (size_t)rht_layout(n, dim).D);
}
// jump region: streams [n][2][kMjX], parts [n][R][3][kMjParts][624], run records [n][R][2]
// (without the jump path: the local blocks after KQ1a, [n][624])
static size_t quicfl_ws_total(int64_t n, int64_t dim) {
    const QflJumpPlan p = qfl_jump_plan(n, rht_layout(n, dim).D);
    const size_t jb = p.use ? ((size_t)n * 2 * kMjX + (size_t)n * p.R * (3 * kMjParts * kMtN + 2)) * sizeof(uint32_t)
                            : (size_t)n * kMtN * sizeof(uint32_t);
    return quicfl_jump_off(n, dim) + jb;
}

int uq_quicfl_workspace_bytes(int64_t n, int64_t dim, size_t* bytes_out) {
    if (!bytes_out) return fail(UQ_E_INVALID, "null bytes_out");
    if (n < 0 || dim < 0) return fail(UQ_E_INVALID, "n and dim must be >= 0");
    *bytes_out = quicfl_ws_total(n, dim);
    return UQ_OK;
}

// The jump path's first two phases (KQ0s + KQ0j) depend only on the generators, so they are
// issued first, on the side stream, and run beside the RHT and the norm on the caller's stream
// (~80 us of small kernels for one 2^20 message); the runs wait for them.
struct QflJumpLaunch {
    bool use = false;
    bool passa = false;             // KQ1a runs on the side stream instead (the one-wave form)
    bool passa_runs = false;        // KQ1ar ran every run's pass A on the side stream (the jump path)
    QflJumpPlan jp;
    uint32_t* parts = nullptr;
    uint32_t* lstate = nullptr;     // KQ1a's local blocks
    SideStream* sb = nullptr;
};
// Which sender form a call takes (launch_quicfl_send): 0 the jump path, 1 the team kernel
// (KQ1t), 2 the one-wave kernel (KQ1).
static int qfl_send_form(int64_t n, int64_t D, bool jump_use) {
    const int hooks = g_quicfl_hooks.load();
    if (jump_use) return 0;
    const QflJumpPlan jp = qfl_jump_plan(n, D);
    if (!(hooks & 2) && ((hooks & 5) || !jp.use) && n <= kQfTeamMaxN && D >= (int64_t)kMtN * kQfRuns &&
        D <= kQfTeamMaxD)
        return 1;
    return 2;
}
static int quicfl_jump_fork(int64_t n, int64_t D, int64_t dim, const int32_t* prng_seeds, const uint32_t* px_state,
                            const int32_t* px_seeds, int32_t h_len, char* wsb, hipStream_t st, QflJumpLaunch* jl) {
    *jl = QflJumpLaunch{};
    const int hooks = g_quicfl_hooks.load();
    const QflJumpPlan jp = qfl_jump_plan(n, D);
    if ((hooks & 7) || !jp.use) {
        if (qfl_send_form(n, D, false) != 2) return UQ_OK;
        // the one-wave form: its pass A (h from the message seeds) beside the RHT and the norm
        SideStream* sb = nullptr;
        int rc = side_stream(&sb);
        if (rc) return rc;
        if ((rc = hip_check(hipEventRecord(sb->fork, st), "record fork"))) return rc;
        if ((rc = hip_check(hipStreamWaitEvent(sb->s, sb->fork, 0), "wait fork"))) return rc;
        QflSendArgs qa{};
        qa.prng_seeds = prng_seeds;
        qa.hbuf = (uint8_t*)(wsb + quicfl_h_off(n, dim));
        qa.h_len = h_len;
        qa.D = D;
        qa.n = n;
        uint32_t* ls = (uint32_t*)(wsb + quicfl_jump_off(n, dim));
        hipLaunchKernelGGL(quicfl_pass_a_kernel, dim3((unsigned)((n + kQfWavesPerWG - 1) / kQfWavesPerWG)),
                           dim3(64 * kQfWavesPerWG), 0, sb->s, qa, ls);
        rc = hip_check(hipGetLastError(), "quicfl_pass_a_kernel launch");
        const int rj = hip_check(hipEventRecord(sb->join, sb->s), "record join");
        if (!rj) {
            jl->passa = true;                   // the guard and the wave launch wait on the join
            jl->lstate = ls;
            jl->sb = sb;
        } else if (hipEventRecord(sb->join, sb->s) == hipSuccess) {
            (void)hipStreamWaitEvent(st, sb->join, 0);
        }
        return rc ? rc : rj;
    }
    const uint32_t* polys = nullptr;
    int rc = qfl_jump_polys(jp, false, &polys);
    if (rc) return rc;
    SideStream* sb = nullptr;
    if ((rc = side_stream(&sb))) return rc;
    if ((rc = hip_check(hipEventRecord(sb->fork, st), "record fork"))) return rc;
    if ((rc = hip_check(hipStreamWaitEvent(sb->s, sb->fork, 0), "wait fork"))) return rc;
    auto join_on_error = [&](int err) {      // whatever reached the side stream finishes before st moves on
        if (hipEventRecord(sb->join, sb->s) == hipSuccess) (void)hipStreamWaitEvent(st, sb->join, 0);
        return err;
    };
    uint32_t* xs = (uint32_t*)(wsb + quicfl_jump_off(n, dim));
    uint32_t* parts = xs + (size_t)n * 2 * kMjX;
    QflJumpArgs ja{};
    ja.prng_seeds = prng_seeds;
    ja.px_state = px_state;
    ja.px_seeds = px_seeds;
    ja.polyA = polys;
    ja.polyB = polys + (size_t)jp.R * kMtN;
    ja.xs = xs;
    ja.parts = parts;
    ja.R = jp.R;
    ja.n = n;
    ja.nstreams = 2;
    ja.kinds = 3;
    hipLaunchKernelGGL(quicfl_stream_kernel, dim3((unsigned)((2 * n + 3) / 4)), dim3(256), 0, sb->s, ja);
    if ((rc = hip_check(hipGetLastError(), "quicfl_stream_kernel launch"))) return join_on_error(rc);
    hipLaunchKernelGGL(quicfl_jump_kernel, dim3((unsigned)(n * jp.R * 3 * kMjParts)), dim3(256), 0, sb->s, ja);
    if ((rc = hip_check(hipGetLastError(), "quicfl_jump_kernel launch"))) return join_on_error(rc);
    {   // KQ1ar: the runs' pass A (h) beside the RHT and the norm
        QflSendArgs qa{};
        qa.prng_seeds = prng_seeds;
        qa.hbuf = (uint8_t*)(wsb + quicfl_h_off(n, dim));
        qa.h_len = h_len;
        qa.D = D;
        qa.n = n;
        QflRunArgs ra{};
        ra.parts = parts;
        ra.R = jp.R;
        ra.L = jp.L;
        hipLaunchKernelGGL(quicfl_pass_a_runs_kernel, dim3((unsigned)((n * jp.R + kQfWavesPerWG - 1) / kQfWavesPerWG)),
                           dim3(64 * kQfWavesPerWG), 0, sb->s, qa, ra);
        if ((rc = hip_check(hipGetLastError(), "quicfl_pass_a_runs_kernel launch"))) return join_on_error(rc);
    }
    if ((rc = hip_check(hipEventRecord(sb->join, sb->s), "record join"))) return join_on_error(rc);
    jl->use = true;
    jl->passa_runs = true;
    jl->jp = jp;
    jl->parts = parts;
    jl->sb = sb;
    return UQ_OK;
}

static int launch_quicfl_send(QflSendArgs& q, int32_t x_kind, const QflJumpLaunch& jl, hipStream_t st);

// Once the fork has happened, the caller's stream waits on the side stream's join on every exit
// path: KQ0s / KQ0j write into the caller's workspace, which may be freed or reused after an
// early error return.  (Waiting twice on the join is harmless.)
namespace {
struct QflJoinGuard {
    const QflJumpLaunch& jl;
    hipStream_t st;
    ~QflJoinGuard() {
        if (jl.use || jl.passa) (void)hipStreamWaitEvent(st, jl.sb->join, 0);
    }
};
}  // namespace

int uq_quicfl_compress_f32(const float* x, int64_t n, int64_t dim, const int8_t* signs, const int32_t* sign_row,
                           const float* table_xp, const uint32_t* table_packed, int64_t table_numel, int32_t h_len,
                           float delta, const int32_t* prng_seeds, const uint32_t* px_state, const int32_t* px_seeds,
                           uint32_t* px_state_out, void* X, int32_t x_kind, uint8_t* exact_mask, float* exact_vals,
                           int32_t* exact_count, float* scale, int32_t* info, void* ws, size_t ws_bytes,
                           void* stream) {
    if (n < 0 || dim < 0) return fail(UQ_E_INVALID, "n and dim must be >= 0");
    if (n > 65535) return fail(UQ_E_INVALID, "at most 65535 messages per call");
    if (dim > ((int64_t)1 << 28)) return fail(UQ_E_INVALID, "dim must be <= 2^28");
    if (h_len < 1 || h_len > 256) return fail(UQ_E_INVALID, "h_len must be 1..256");
    if (table_numel < h_len || table_numel % h_len) return fail(UQ_E_INVALID, "table_numel must be a multiple of h_len");
    if (table_numel >= ((int64_t)1 << 24)) return fail(UQ_E_INVALID, "table_numel must be below 2^24");
    if (x_kind != 0 && x_kind != 1) return fail(UQ_E_INVALID, "x_kind must be 0 (int64) or 1 (uint8)");
    if (n == 0 || dim == 0) return UQ_OK;
    if (!x || !signs || !table_xp || !prng_seeds || !X || !exact_mask || !exact_vals || !exact_count || !scale || !info)
        return fail(UQ_E_INVALID, "null pointer");
    if (!px_state && !px_seeds) return fail(UQ_E_INVALID, "px_state or px_seeds is required");
    const RhtLayout w = rht_layout(n, dim);
    const size_t hoff = quicfl_h_off(n, dim);
    if (!ws || ws_bytes < quicfl_ws_total(n, dim)) return fail(UQ_E_WORKSPACE, "workspace too small");
    hipStream_t st = (hipStream_t)stream;
    char* wsb = (char*)ws;
    QflJumpLaunch jl;
    int rc = quicfl_jump_fork(n, w.D, dim, prng_seeds, px_state, px_seeds, h_len, wsb, st, &jl);
    if (rc) return rc;
    const QflJoinGuard join_guard{jl, st};
    float* rot = nullptr;
    rc = rht_norm_front(x, n, dim, signs, sign_row, wsb, &rot, st);                     // AS:460-470
    if (rc) return rc;
    QflSendArgs q{};
    q.rot = rot;
    q.nrm = (const float*)(wsb + w.nrm_off);
    q.tab = (const float2*)table_xp;
    q.tabp = table_packed;
    q.numel = table_numel;
    q.half = ((table_numel / h_len) - 1) * h_len / 2;                                        // AS:443
    q.h_len = h_len;
    q.delta = delta;
    q.sqrtD = (float)std::sqrt((double)w.D);                                                  // np.sqrt(D) -> f32
    q.prng_seeds = prng_seeds;
    q.px_state = px_state;
    q.px_seeds = px_seeds;
    q.px_state_out = px_state_out;
    q.hbuf = (uint8_t*)(wsb + hoff);
    q.X = X;
    q.x_kind = x_kind;
    q.mask = exact_mask;
    q.ev = exact_vals;
    q.ecount = exact_count;
    q.scale = scale;
    q.info = info;
    q.D = w.D;
    q.n = n;
    return launch_quicfl_send(q, x_kind, jl, st);
}

// By batch size and the plan's cost model: the jump path (KQ0s + KQ0j + KQ1j + KQ1f: every run
// of every message at once from jumped stream blocks) when it beats a wave per message, else up
// to 256 the team kernel KQ1t (scouts + runs in one workgroup per message), batches a wave per
// message (KQ1).  Test hooks: bit 1 the
// one-wave kernel, bit 2 (or bit 0, whose timeouts only the team's runs can report) KQ1t.
static int launch_quicfl_send(QflSendArgs& q, int32_t x_kind, const QflJumpLaunch& jl, hipStream_t st) {
    const int hooks = g_quicfl_hooks.load();
    q.force_timeout = hooks & 1;
    const int64_t n = q.n;
    const QflJumpPlan jp = qfl_jump_plan(n, q.D);
    if (jl.use) {
        int rc = hip_check(hipStreamWaitEvent(st, jl.sb->join, 0), "wait join");   // KQ0s + KQ0j done
        if (rc) return rc;
        QflRunArgs ra{};
        ra.parts = jl.parts;
        ra.runinfo = (int32_t*)(jl.parts + (size_t)n * jl.jp.R * 3 * kMjParts * kMtN);
        ra.R = jl.jp.R;
        ra.L = jl.jp.L;
        ra.passa_done = jl.passa_runs ? 1 : 0;
        const dim3 rgrid((unsigned)((n * jl.jp.R + kQfWavesPerWG - 1) / kQfWavesPerWG)), blk(64 * kQfWavesPerWG);
        const bool w2 = n * jl.jp.R > kQfRunWaves1;
#define UQ_QRUNS(XK)                                                                                        \
    if (w2) hipLaunchKernelGGL((quicfl_send_runs_kernel<XK, true>), rgrid, blk, 0, st, q, ra);               \
    else hipLaunchKernelGGL((quicfl_send_runs_kernel<XK, false>), rgrid, blk, 0, st, q, ra);
        if (x_kind == 2) { UQ_QRUNS(2) } else if (x_kind == 0) { UQ_QRUNS(0) } else { UQ_QRUNS(1) }
#undef UQ_QRUNS
        rc = hip_check(hipGetLastError(), "quicfl_send_runs_kernel launch");
        if (rc) return rc;
        hipLaunchKernelGGL(quicfl_send_fin_kernel, dim3((unsigned)((n + kQfWavesPerWG - 1) / kQfWavesPerWG)), blk, 0, st,
                           q, ra);
        return hip_check(hipGetLastError(), "quicfl_send_fin_kernel launch");
    }
    if (!(hooks & 2) && ((hooks & 5) || !jp.use) && n <= kQfTeamMaxN && q.D >= (int64_t)kMtN * kQfRuns &&
        q.D <= kQfTeamMaxD) {
        if (x_kind == 2)
            hipLaunchKernelGGL(quicfl_send_team_kernel<2>, dim3((unsigned)n), dim3(64 * kQfTeamWaves), 0, st, q);
        else if (x_kind == 0)
            hipLaunchKernelGGL(quicfl_send_team_kernel<0>, dim3((unsigned)n), dim3(64 * kQfTeamWaves), 0, st, q);
        else
            hipLaunchKernelGGL(quicfl_send_team_kernel<1>, dim3((unsigned)n), dim3(64 * kQfTeamWaves), 0, st, q);
        return hip_check(hipGetLastError(), "quicfl_send_team_kernel launch");
    }
    const dim3 grid((unsigned)((n + kQfWavesPerWG - 1) / kQfWavesPerWG));
    if (jl.passa) {                                  // KQ1a (pass A) ran on the side stream
        const int rc = hip_check(hipStreamWaitEvent(st, jl.sb->join, 0), "wait join");
        if (rc) return rc;
        q.lstate = jl.lstate;
    }
    if (x_kind == 2)
        hipLaunchKernelGGL(quicfl_send_wave_kernel<2>, grid, dim3(64 * kQfWavesPerWG), 0, st, q);
    else if (x_kind == 0)
        hipLaunchKernelGGL(quicfl_send_wave_kernel<0>, grid, dim3(64 * kQfWavesPerWG), 0, st, q);
    else
        hipLaunchKernelGGL(quicfl_send_wave_kernel<1>, grid, dim3(64 * kQfWavesPerWG), 0, st, q);
    return hip_check(hipGetLastError(), "quicfl_send_wave_kernel launch");
}

// QUICFL_quantize (AS:814-832) for a batch: the sender as uq_quicfl_compress_f32 with the
// receiver fused into its stage 2 (no second h stream, no message in HBM), then the receiver's
// inverse RHT into out [n][dim].
int uq_quicfl_quantize_f32(const float* x, int64_t n, int64_t dim, const int8_t* signs, const int32_t* sign_row,
                           const float* table_xp, const uint32_t* table_packed, int64_t table_numel, int32_t h_len,
                           float delta, const float* recv_table, int32_t recv_numel, const int32_t* prng_seeds,
                           const uint32_t* px_state, const int32_t* px_seeds, uint32_t* px_state_out, float* out,
                           float* scale, int32_t* info, void* ws, size_t ws_bytes, void* stream) {
    if (n < 0 || dim < 0) return fail(UQ_E_INVALID, "n and dim must be >= 0");
    if (n > 65535) return fail(UQ_E_INVALID, "at most 65535 messages per call");
    if (dim > ((int64_t)1 << 28)) return fail(UQ_E_INVALID, "dim must be <= 2^28");
    if (h_len < 1 || h_len > 256) return fail(UQ_E_INVALID, "h_len must be 1..256");
    if (table_numel < h_len || table_numel % h_len) return fail(UQ_E_INVALID, "table_numel must be a multiple of h_len");
    if (table_numel >= ((int64_t)1 << 24)) return fail(UQ_E_INVALID, "table_numel must be below 2^24");
    if (recv_numel < 1 || recv_numel > kQflRecvTab) return fail(UQ_E_INVALID, "receiver table must hold 1..1024 entries");
    if (n == 0 || dim == 0) return UQ_OK;
    if (!x || !signs || !table_xp || !recv_table || !prng_seeds || !out || !info)
        return fail(UQ_E_INVALID, "null pointer");
    if (!px_state && !px_seeds) return fail(UQ_E_INVALID, "px_state or px_seeds is required");
    const RhtLayout w = rht_layout(n, dim);
    const size_t hoff = quicfl_h_off(n, dim);
    if (!ws || ws_bytes < quicfl_ws_total(n, dim)) return fail(UQ_E_WORKSPACE, "workspace too small");
    hipStream_t st = (hipStream_t)stream;
    char* wsb = (char*)ws;
    QflJumpLaunch jl;
    int rc = quicfl_jump_fork(n, w.D, dim, prng_seeds, px_state, px_seeds, h_len, wsb, st, &jl);
    if (rc) return rc;
    const QflJoinGuard join_guard{jl, st};
    float* rot = nullptr;
    rc = rht_norm_front(x, n, dim, signs, sign_row, wsb, &rot, st);                     // AS:460-470
    if (rc) return rc;
    QflSendArgs q{};
    q.rot = rot;
    q.nrm = (const float*)(wsb + w.nrm_off);
    q.tab = (const float2*)table_xp;
    q.tabp = table_packed;
    q.numel = table_numel;
    q.half = ((table_numel / h_len) - 1) * h_len / 2;                                        // AS:443
    q.h_len = h_len;
    q.delta = delta;
    q.sqrtD = (float)std::sqrt((double)w.D);
    q.prng_seeds = prng_seeds;
    q.px_state = px_state;
    q.px_seeds = px_seeds;
    q.px_state_out = px_state_out;
    q.hbuf = (uint8_t*)(wsb + hoff);
    q.scale = scale;
    q.info = info;
    q.D = w.D;
    q.n = n;
    q.rtab = recv_table;
    q.rtab_n = recv_numel;
    q.pre = rot;                       // in place: a coordinate's rot is loaded a round before its value is stored
    rc = launch_quicfl_send(q, 2, jl, st);              // (2: the fused instances)                 AS:455-503, 526-532
    if (rc) return rc;
    return rht_inverse(rot, out, n, w.D, dim, signs, sign_row, st);                           // AS:533-535
}

// xxHash64 (the public XXH64 algorithm), for AS:457's prng seed
static inline uint64_t xxh_rotl(uint64_t x, int r) { return (x << r) | (x >> (64 - r)); }
static inline uint64_t xxh_read64(const uint8_t* p) { uint64_t v; std::memcpy(&v, p, 8); return v; }
static inline uint32_t xxh_read32(const uint8_t* p) { uint32_t v; std::memcpy(&v, p, 4); return v; }

uint64_t uq_xxh64(const void* data, size_t len, uint64_t seed) {
    const uint64_t P1 = 0x9E3779B185EBCA87ull, P2 = 0xC2B2AE3D27D4EB4Full, P3 = 0x165667B19E3779F9ull,
                   P4 = 0x85EBCA77C2B2AE63ull, P5 = 0x27D4EB2F165667C5ull;
    auto round = [&](uint64_t acc, uint64_t lane) { return xxh_rotl(acc + lane * P2, 31) * P1; };
    const uint8_t* p = (const uint8_t*)data;
    const uint8_t* end = p + len;
    uint64_t h;
    if (len >= 32) {
        uint64_t v1 = seed + P1 + P2, v2 = seed + P2, v3 = seed, v4 = seed - P1;
        while (p + 32 <= end) {
            v1 = round(v1, xxh_read64(p));
            v2 = round(v2, xxh_read64(p + 8));
            v3 = round(v3, xxh_read64(p + 16));
            v4 = round(v4, xxh_read64(p + 24));
            p += 32;
        }
        h = xxh_rotl(v1, 1) + xxh_rotl(v2, 7) + xxh_rotl(v3, 12) + xxh_rotl(v4, 18);
        for (uint64_t v : {v1, v2, v3, v4}) h = (h ^ round(0, v)) * P1 + P4;
    } else {
        h = seed + P5;
    }
    h += (uint64_t)len;
    for (; p + 8 <= end; p += 8) h = xxh_rotl(h ^ round(0, xxh_read64(p)), 27) * P1 + P4;
    if (p + 4 <= end) {
        h = xxh_rotl(h ^ ((uint64_t)xxh_read32(p) * P1), 23) * P2 + P3;
        p += 4;
    }
    for (; p < end; ++p) h = xxh_rotl(h ^ ((uint64_t)*p * P5), 11) * P1;
    h ^= h >> 33;
    h *= P2;
    h ^= h >> 29;
    h *= P3;
    h ^= h >> 32;
    return h;
}

}  // extern "C"
