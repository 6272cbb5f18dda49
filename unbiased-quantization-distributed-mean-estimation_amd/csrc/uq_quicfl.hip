// uq_quicfl.hip — QUIC-FL: the dispatch plan, the launchers of uq_quicfl_kernels.h and the C API
// of the sender (uq_quicfl_compress_f32, uq_quicfl_quantize_f32) and the receiver
// (uq_quicfl_receive_*), the packed message form of both (uq_quicfl_*_packed_f32, uq_quicfl_pack_x /
// uq_quicfl_unpack_x), and uq_xxh64 (the sender's prng seed).  The RHT and the norm run in
// uq_eden.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <map>
#include <mutex>
#include <optional>
#include <tuple>
#include <type_traits>
#include <vector>

#include "uq_internal.h"
#include "uq_quicfl_kernels.h"

// uq_test_set_quicfl_hooks (include/uq_dme.h); each entry point loads it once, into its plan
static std::atomic<int> g_quicfl_hooks{0};
// uq_test_set_quicfl_packed_hooks; each packed entry point loads it once
static std::atomic<int> g_quicfl_packed_hooks{0};

namespace {

// ---- dispatch plan -------------------------------------------------------------------
// Every decision of a sender or receiver call, made once on the host from (side, n, D, hooks,
// workspace); DESIGN.md §4.4 has the table.  The launchers launch what the plan names and the
// workspace sizes read the same function, so the test hooks (uq_test_quicfl_plan,
// uq_test_last_quicfl_plan) report what a call really runs.
struct QflPlan {
    int32_t form = UQ_QFL_FORM_NONE;
    int32_t R = 0;                  // jump form: R runs of L rounds per message
    int64_t L = 0, qL = 0;          // qL: block of the sender's first pass-B local word (qfl_ctx)
    bool w2 = false;                // jump form: more than kQfRunWaves1 run waves, two per SIMD
    int32_t force_timeout = 0;      // hook bit 0
    int32_t side = UQ_QFL_SIDE_NONE;   // the sender's work on the side stream
    size_t jump_bytes = 0;          // the workspace's jump region, whatever the hooks say
};

// What differs between the two sides in the plan: a round of one run wave costs ~tR us, a message
// takes jmul R - jsub jumps (sender: three blocks per run but run 0's two local ones; receiver:
// one), the team kernel has `team_runs` run waves, and the jump region holds `streams` streams
// and `kinds` blocks per run (the sender without the jump form: KQ1a's local blocks, [n][624]).
struct QflSide {
    double tR;
    int64_t jmul, jsub, team_runs;
    size_t streams, kinds;
};
constexpr QflSide kQflSides[2] = {{7.5, 3, 2, kQfRuns, 2, 3}, {3.0, 1, 1, kQrRuns, 1, 1}};

// Up to 1024 run waves a wave per SIMD; up to 2048 two, a round then costing ~1.3 tR.
constexpr int64_t kQfJumpMaxN = 1024;
constexpr int64_t kQfRunWaves1 = 1024, kQfRunWaves2 = 2048;

// The jump form's R from a cost model of its phases (measured round-5 / round-6 constants, us):
// the streams (~20), the jumps (~0.12 of the whole GPU each) and L rounds on one wave.  True
// when the model beats what the call would run otherwise:
//   sender    up to 128 messages and above 256 the one-wave kernel (~tR per round, 1024 waves at
//             a time); 129-256 the team kernel at ~2.85 us per round, the model ~1.4x optimistic
//   receiver  up to 256 messages the team kernel (~1 us per round), above the one-wave kernel
bool qfl_jump_search(int side, int64_t n, int64_t D, int32_t* R_out, int64_t* L_out) {
    const QflSide& s = kQflSides[side];
    const int64_t nch = (D + kMtN - 1) / kMtN;
    if (n < 1 || n > kQfJumpMaxN || nch < 8 || D > ((int64_t)1 << 28)) return false;
    const double tS = 20.0, tJ = 0.12, tR = s.tR, f2 = 1.3;
    double best = 1e300;
    for (int64_t R = 1; R <= 1024 && R <= nch; ++R) {
        const int64_t L = (nch + R - 1) / R, Ru = (nch + L - 1) / L;
        if (Ru != R || n * R > kQfRunWaves2) continue;
        const double t = tS + (double)(n * (s.jmul * R - s.jsub)) * tJ + (double)L * tR * (n * R > kQfRunWaves1 ? f2 : 1.0);
        if (t < best) {
            best = t;
            *R_out = (int32_t)R;
            *L_out = L;
        }
    }
    if (side == UQ_QFL_RECEIVER) return best < 0.8 * (double)nch * (n <= kQfTeamMaxN ? 1.0 : tR);
    if (n <= 128 || n > kQfTeamMaxN) return best < 0.8 * (double)((n + 1023) / 1024) * (double)nch * tR;
    return best < 2.0 * (double)nch;
}

// ws_avail: bytes the caller gives the jump region.  The receiver runs without one; the sender's
// entry points refuse a workspace smaller than the plan's, so they plan with SIZE_MAX.
QflPlan qfl_plan(int side, int64_t n, int64_t D, int hooks, size_t ws_avail) {
    const QflSide& s = kQflSides[side];
    QflPlan p;
    const bool wins = qfl_jump_search(side, n, D, &p.R, &p.L);
    if (wins)
        p.jump_bytes = ((size_t)n * s.streams * kMjX + (size_t)n * p.R * (s.kinds * kMjParts * kMtN + 2)) * sizeof(uint32_t);
    else if (side == UQ_QFL_SENDER)
        p.jump_bytes = (size_t)std::max<int64_t>(n, 0) * kMtN * sizeof(uint32_t);
    if (n < 1 || D < 1) return p;
    p.force_timeout = hooks & 1;
    if (wins && !(hooks & 7) && ws_avail >= p.jump_bytes) {
        p.form = UQ_QFL_FORM_JUMP;
        p.qL = ((int64_t)kMtN + D) / kMtN;
        p.w2 = n * p.R > kQfRunWaves1;
    } else {
        const bool team = !(hooks & 2) && n <= kQfTeamMaxN && D >= (int64_t)kMtN * s.team_runs && D <= kQfTeamMaxD;
        p.form = team ? UQ_QFL_FORM_TEAM : UQ_QFL_FORM_ONE_WAVE;
        p.R = 0;
        p.L = 0;
    }
    if (side == UQ_QFL_SENDER)
        p.side = p.form == UQ_QFL_FORM_JUMP ? UQ_QFL_SIDE_JUMP
                                             : p.form == UQ_QFL_FORM_ONE_WAVE ? UQ_QFL_SIDE_PASS_A : UQ_QFL_SIDE_NONE;
    return p;
}

thread_local QflPlan t_last_plan[2];         // uq_test_last_quicfl_plan, per side

int export_plan(const QflPlan& p, int64_t* out, int32_t cap) {
    if (!out || cap < 0) return fail(UQ_E_INVALID, "null plan output");
    const int64_t f[UQ_QFL_PLAN_FIELDS] = {p.form, p.R, p.L, p.w2, p.force_timeout, p.side};
    for (int i = 0; i < std::min<int32_t>(cap, UQ_QFL_PLAN_FIELDS); ++i) out[i] = f[i];
    return UQ_OK;
}

// ---- kernel selection and launch shapes ------------------------------------------------
// The run-time x_kind (0 int64, 1 uint8, 2 int32 / the sender's fused instances) becomes a
// compile-time constant: f(XK) launches the instance it names; with W2 behind it for the
// sender's runs.  (2, 0, 1 is the order the sender's instances have always been emitted in;
// another order moves the padding between kernels, and with it tools/kernel_table.py's hashes.)
// 3: the packed message's instances (internal: no entry point takes it as an x_kind), emitted in front of them:
// the last instance of the unit has no padding behind it, and stays the last.
template <int K>
using Xk = std::integral_constant<int, K>;

template <class F>
void select_xk(int32_t x_kind, F&& f) {
    if (x_kind == 3) f(Xk<3>{});
    else if (x_kind == 2) f(Xk<2>{});
    else if (x_kind == 0) f(Xk<0>{});
    else f(Xk<1>{});
}
template <class F>
void select_xk_w2(int32_t x_kind, bool w2, F&& f) {
    if (w2) select_xk(x_kind, [&](auto XK) { f(XK, Flag<true>{}); });
    else select_xk(x_kind, [&](auto XK) { f(XK, Flag<false>{}); });
}

const dim3 kWaveBlock(64 * kQfWavesPerWG), kTeamBlock(64 * kQfTeamWaves);
dim3 wave_grid(int64_t waves) { return dim3((unsigned)((waves + kQfWavesPerWG - 1) / kQfWavesPerWG)); }

}  // namespace

extern "C" {

int uq_mtpoly_progression(int64_t b0, int64_t step, int32_t count, uint32_t* out);   // uq_mt_poly.cpp

int uq_test_set_quicfl_hooks(int flags) { return g_quicfl_hooks.exchange(flags & 7); }

int uq_test_quicfl_plan(int32_t side, int64_t n, int64_t D, int32_t hooks, int32_t has_ws, int64_t* plan_out,
                        int32_t cap) {
    if (side != UQ_QFL_SENDER && side != UQ_QFL_RECEIVER) return fail(UQ_E_INVALID, "side must be 0 (sender) or 1 (receiver)");
    if (n < 0 || D < 0) return fail(UQ_E_INVALID, "n and D must be >= 0");
    return export_plan(qfl_plan(side, n, D, hooks & 7, has_ws ? SIZE_MAX : 0), plan_out, cap);
}

int uq_test_last_quicfl_plan(int32_t side, int64_t* plan_out, int32_t cap) {
    if (side != UQ_QFL_SENDER && side != UQ_QFL_RECEIVER) return fail(UQ_E_INVALID, "side must be 0 (sender) or 1 (receiver)");
    return export_plan(t_last_plan[side], plan_out, cap);
}

// t^(624 b) mod phi for the plan's run starts, on the device, cached per (device, qL, L, R):
// rows [0, R) = polyA (row r: b = r L - 1; row 0 unused), rows [R, 2R) = polyB (b = qL + r L - 1)
static int qfl_jump_polys(const QflPlan& p, bool a_only, const uint32_t** out) {
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

// ---- QUIC-FL receiver --------------------------------------------------------------------
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
    *bytes_out = qfl_plan(UQ_QFL_RECEIVER, n, D, 0, 0).jump_bytes;
    return UQ_OK;
}

// KQ0s + KQ0j (the h stream, one block per run) + KQ2c + KQ2j + KQ2f
static int quicfl_recv_jump(const QflRecvArgs& r, int32_t x_kind, const QflPlan& P, char* wsb, hipStream_t st) {
    const int64_t n = r.n;
    const uint32_t* polys = nullptr;
    int rc = qfl_jump_polys(P, true, &polys);
    if (rc) return rc;
    uint32_t* xs = (uint32_t*)wsb;
    uint32_t* parts = xs + (size_t)n * kMjX;
    QflJumpArgs ja{};
    ja.prng_seeds = r.prng_seeds;
    ja.polyA = polys;
    ja.polyB = polys;                                    // (unused: one kind)
    ja.xs = xs;
    ja.parts = parts;
    ja.R = P.R;
    ja.n = n;
    ja.nstreams = 1;
    ja.kinds = 1;
    hipLaunchKernelGGL(quicfl_stream_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, ja);
    if ((rc = launched("quicfl_stream_kernel launch"))) return rc;
    hipLaunchKernelGGL(quicfl_jump_kernel, dim3((unsigned)(n * P.R * kMjParts)), dim3(256), 0, st, ja);
    if ((rc = launched("quicfl_jump_kernel launch"))) return rc;
    QflRunArgs ra{};
    ra.parts = parts;
    ra.runinfo = (int32_t*)(parts + (size_t)n * P.R * kMjParts * kMtN);
    ra.R = P.R;
    ra.L = P.L;
    if (x_kind != 3) {                                   // (a packed message has no mask to count)
        hipLaunchKernelGGL(quicfl_recv_count_kernel, wave_grid(n * P.R), kWaveBlock, 0, st, r, ra);
        if ((rc = launched("quicfl_recv_count_kernel launch"))) return rc;
    }
    select_xk(x_kind, [&](auto XK) {
        hipLaunchKernelGGL(quicfl_recv_runs_kernel<XK()>, wave_grid(n * P.R), kWaveBlock, 0, st, r, ra);
    });
    if ((rc = launched("quicfl_recv_runs_kernel launch"))) return rc;
    hipLaunchKernelGGL(quicfl_recv_fin_kernel, wave_grid(n), kWaveBlock, 0, st, r, ra);
    return launched("quicfl_recv_fin_kernel launch");
}

// The receiver of every entry point.  x_kind 3 (the packed entry point only: nbits planes per payload
// row in X, no mask and no exact values in the rounds, no counting pass).
static int quicfl_receive(const void* X, int32_t x_kind, int32_t nbits, int64_t n, int64_t D, const float* recv_table,
                          int32_t table_rows, int32_t h_len, const int32_t* prng_seeds, const uint8_t* exact_mask,
                          const float* exact_vals, int32_t exact_layout, const int32_t* exact_count,
                          const float* scale, float* out, int32_t* info, void* ws, size_t ws_bytes, void* stream) {
    const int hooks = g_quicfl_hooks.load();
    t_last_plan[UQ_QFL_RECEIVER] = QflPlan{};
    if (n < 0 || D < 0) return fail(UQ_E_INVALID, "n and D must be >= 0");
    if (n > 65535) return fail(UQ_E_INVALID, "at most 65535 clients per call");
    if (D > ((int64_t)1 << 28)) return fail(UQ_E_INVALID, "at most 2^28 coordinates per message");
    if (x_kind < 0 || x_kind > 2 + (nbits > 0)) return fail(UQ_E_INVALID, "x_kind must be 0 (int64), 1 (uint8) or 2 (int32)");
    if (exact_layout != 0 && exact_layout != 1) return fail(UQ_E_INVALID, "exact_layout must be 0 (dense) or 1 (compact)");
    if (n == 0 || D == 0) return UQ_OK;
    if (!X || !recv_table || !prng_seeds || !scale || !out) return fail(UQ_E_INVALID, "null pointer");
    if ((exact_mask == nullptr) != (exact_vals == nullptr)) return fail(UQ_E_INVALID, "exact_mask and exact_vals go together");
    if (h_len < 1 || table_rows < 1 || (int64_t)h_len * table_rows > kQflTab)
        return fail(UQ_E_INVALID, "receiver table must hold 1..1024 entries");
    hipStream_t st = (hipStream_t)stream;
    const QflPlan P = qfl_plan(UQ_QFL_RECEIVER, n, D, hooks, ws ? ws_bytes : 0);
    t_last_plan[UQ_QFL_RECEIVER] = P;
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
    r.nbits = nbits;
    r.exact_count = exact_count;
    r.scale = scale;
    r.out = out;
    r.info = info;
    r.force_timeout = P.force_timeout;
    if (P.form == UQ_QFL_FORM_JUMP) return quicfl_recv_jump(r, x_kind, P, (char*)ws, st);
    if (P.form == UQ_QFL_FORM_TEAM) {
        select_xk(x_kind, [&](auto XK) {
            hipLaunchKernelGGL(quicfl_recv_team_kernel<XK()>, dim3((unsigned)n), kTeamBlock, 0, st, r);
        });
        return launched("quicfl_recv_team_kernel launch");
    }
    select_xk(x_kind, [&](auto XK) { hipLaunchKernelGGL(quicfl_recv_wave_kernel<XK()>, wave_grid(n), kWaveBlock, 0, st, r); });
    return launched("quicfl_recv_wave_kernel launch");
}

int uq_quicfl_receive_ws_f32(const void* X, int32_t x_kind, int64_t n, int64_t D, const float* recv_table,
                             int32_t table_rows, int32_t h_len, const int32_t* prng_seeds, const uint8_t* exact_mask,
                             const float* exact_vals, int32_t exact_layout, const int32_t* exact_count,
                             const float* scale, float* out, int32_t* info, void* ws, size_t ws_bytes, void* stream) {
    return quicfl_receive(X, x_kind, 0, n, D, recv_table, table_rows, h_len, prng_seeds, exact_mask, exact_vals, exact_layout,
                          exact_count, scale, out, info, ws, ws_bytes, stream);
}

int uq_quicfl_prepare_f32(const int32_t* X, int64_t n, int64_t D, const float* recv_table, int32_t table_rows,
                          int32_t h_len, const int32_t* prng_seeds, const uint8_t* exact_mask, const float* exact_vals,
                          const float* scale, float* out, void* stream) {
    return uq_quicfl_receive_f32(X, 2, n, D, recv_table, table_rows, h_len, prng_seeds, exact_mask, exact_vals, 0, nullptr,
                                 scale, out, nullptr, stream);
}

// ---- QUIC-FL sender ----------------------------------------------------------------------
// Workspace: the EDEN layout (rotated vectors, norms, segmented-norm region) + h [n][D] u8 + the
// plan's jump region: streams [n][2][kMjX], parts [n][R][3][kMjParts][624], run records
// [n][R][2] (without the jump form: the local blocks after KQ1a, [n][624]).
static size_t quicfl_h_off(int64_t n, int64_t dim) {
    return up256(rht_layout(n, dim).total);
}
static size_t quicfl_jump_off(int64_t n, int64_t dim) {
    return up256(quicfl_h_off(n, dim) + (size_t)n * (size_t)rht_layout(n, dim).D);
}

int uq_quicfl_workspace_bytes(int64_t n, int64_t dim, size_t* bytes_out) {
    if (!bytes_out) return fail(UQ_E_INVALID, "null bytes_out");
    if (n < 0 || dim < 0) return fail(UQ_E_INVALID, "n and dim must be >= 0");
    *bytes_out = quicfl_jump_off(n, dim) + qfl_plan(UQ_QFL_SENDER, n, rht_layout(n, dim).D, 0, 0).jump_bytes;
    return UQ_OK;
}

// What the plan sends to the side stream, to run beside the RHT and the norm on the caller's
// stream: the one-wave form's pass A (KQ1a: h from the message seeds, leaving each local block
// in the jump region), or the jump form's phases that depend only on the generators (KQ0s +
// KQ0j, ~80 us of small kernels for one 2^20 message, then KQ1ar: every run's pass A).
// q: the generators, hbuf, h_len, D and n are set.
static int quicfl_send_side(const QflSendArgs& q, const QflPlan& P, const uint32_t* polys, uint32_t* jump,
                            hipStream_t side) {
    const int64_t n = q.n;
    QflSendArgs qa{};                                    // what pass A reads
    qa.prng_seeds = q.prng_seeds;
    qa.hbuf = q.hbuf;
    qa.h_len = q.h_len;
    qa.D = q.D;
    qa.n = n;
    if (P.side == UQ_QFL_SIDE_PASS_A) {
        hipLaunchKernelGGL(quicfl_pass_a_kernel, wave_grid(n), kWaveBlock, 0, side, qa, jump);
        return launched("quicfl_pass_a_kernel launch");
    }
    QflJumpArgs ja{};
    ja.prng_seeds = q.prng_seeds;
    ja.px_state = q.px_state;
    ja.px_seeds = q.px_seeds;
    ja.polyA = polys;
    ja.polyB = polys + (size_t)P.R * kMtN;
    ja.xs = jump;
    ja.parts = jump + (size_t)n * 2 * kMjX;
    ja.R = P.R;
    ja.n = n;
    ja.nstreams = 2;
    ja.kinds = 3;
    hipLaunchKernelGGL(quicfl_stream_kernel, dim3((unsigned)((2 * n + 3) / 4)), dim3(256), 0, side, ja);
    int rc = launched("quicfl_stream_kernel launch");
    if (rc) return rc;
    hipLaunchKernelGGL(quicfl_jump_kernel, dim3((unsigned)(n * P.R * 3 * kMjParts)), dim3(256), 0, side, ja);
    if ((rc = launched("quicfl_jump_kernel launch"))) return rc;
    QflRunArgs ra{};
    ra.parts = ja.parts;
    ra.R = P.R;
    ra.L = P.L;
    hipLaunchKernelGGL(quicfl_pass_a_runs_kernel, wave_grid(n * P.R), kWaveBlock, 0, side, qa, ra);
    return launched("quicfl_pass_a_runs_kernel launch");
}

// The plan's form on the caller's stream, after the join: KQ1j + KQ1f (every run of every message
// at once from the jumped blocks), KQ1t (scouts + runs in one workgroup per message) or KQ1 (a
// wave per message).  x_kind 2: the fused instances.
static int launch_quicfl_form(QflSendArgs& q, int32_t x_kind, const QflPlan& P, uint32_t* jump, hipStream_t st);
// ... and, behind a packed form (x_kind 3), KQ1p: the jump form's indices into index order, payload_bits
static int launch_quicfl_send(QflSendArgs& q, int32_t x_kind, const QflPlan& P, uint32_t* jump, int64_t* payload_bits,
                              hipStream_t st) {
    int rc = launch_quicfl_form(q, x_kind, P, jump, st);
    if (rc || x_kind != 3) return rc;
    QflRunArgs ra{};
    if (P.form == UQ_QFL_FORM_JUMP) {
        ra.runinfo = (int32_t*)(jump + (size_t)q.n * 2 * kMjX + (size_t)q.n * P.R * 3 * kMjParts * kMtN);
        ra.R = P.R;
        ra.L = P.L;
    }
    hipLaunchKernelGGL(quicfl_send_fin_packed_kernel, wave_grid(q.n), kWaveBlock, 0, st, q, ra, payload_bits);
    return launched("quicfl_send_fin_packed_kernel launch");
}
static int launch_quicfl_form(QflSendArgs& q, int32_t x_kind, const QflPlan& P, uint32_t* jump, hipStream_t st) {
    const int64_t n = q.n;
    if (P.form == UQ_QFL_FORM_JUMP) {
        QflRunArgs ra{};
        ra.parts = jump + (size_t)n * 2 * kMjX;
        ra.runinfo = (int32_t*)(ra.parts + (size_t)n * P.R * 3 * kMjParts * kMtN);
        ra.R = P.R;
        ra.L = P.L;
        ra.passa_done = 1;                               // KQ1ar, on the side stream
        select_xk_w2(x_kind, P.w2, [&](auto XK, auto W2) {
            hipLaunchKernelGGL((quicfl_send_runs_kernel<XK(), W2()>), wave_grid(n * P.R), kWaveBlock, 0, st, q, ra);
        });
        const int rc = launched("quicfl_send_runs_kernel launch");
        if (rc) return rc;
        hipLaunchKernelGGL(quicfl_send_fin_kernel, wave_grid(n), kWaveBlock, 0, st, q, ra);
        return launched("quicfl_send_fin_kernel launch");
    }
    if (P.form == UQ_QFL_FORM_TEAM) {
        select_xk(x_kind, [&](auto XK) {
            hipLaunchKernelGGL(quicfl_send_team_kernel<XK()>, dim3((unsigned)n), kTeamBlock, 0, st, q);
        });
        return launched("quicfl_send_team_kernel launch");
    }
    q.lstate = jump;                                     // KQ1a's local blocks
    select_xk(x_kind, [&](auto XK) { hipLaunchKernelGGL(quicfl_send_wave_kernel<XK()>, wave_grid(n), kWaveBlock, 0, st, q); });
    return launched("quicfl_send_wave_kernel launch");
}

// The arguments uq_quicfl_compress_f32 and uq_quicfl_quantize_f32 share.
struct QflSendCall {
    const float* x;
    int64_t n, dim;
    const int8_t* signs;
    const int32_t* sign_row;
    const float* table_xp;
    const uint32_t* table_packed;
    int64_t table_numel;
    int32_t h_len;
    float delta;
    const int32_t* prng_seeds;
    const uint32_t* px_state;
    const int32_t* px_seeds;
    uint32_t* px_state_out;
    float* scale;
    int32_t* info;
    void* ws;
    size_t ws_bytes;
    void* stream;
    size_t ws_extra = 0;        // bytes the entry point keeps behind the sender's own workspace
};

// The sender of both entry points: the shared checks, the plan, the side-stream work, the RHT
// and the norm (AS:460-470), and the plan's form.  q arrives with the entry point's own fields;
// own_error / own_null: its own argument check and null pointers, reported in the entry points'
// order.  *rot: the rotated vectors (null when nothing ran), into which a fused call
// (q.rtab set) also writes the receiver's values.
static int quicfl_send(const QflSendCall& c, const char* own_error, bool own_null, QflSendArgs q, int32_t x_kind,
                       float** rot, int64_t* payload_bits = nullptr) {
    const int hooks = g_quicfl_hooks.load();
    t_last_plan[UQ_QFL_SENDER] = QflPlan{};
    *rot = nullptr;
    const int64_t n = c.n, dim = c.dim;
    if (n < 0 || dim < 0) return fail(UQ_E_INVALID, "n and dim must be >= 0");
    if (n > 65535) return fail(UQ_E_INVALID, "at most 65535 messages per call");
    if (dim > ((int64_t)1 << 28)) return fail(UQ_E_INVALID, "dim must be <= 2^28");
    if (c.h_len < 1 || c.h_len > 256) return fail(UQ_E_INVALID, "h_len must be 1..256");
    if (c.table_numel < c.h_len || c.table_numel % c.h_len) return fail(UQ_E_INVALID, "table_numel must be a multiple of h_len");
    if (c.table_numel >= ((int64_t)1 << 24)) return fail(UQ_E_INVALID, "table_numel must be below 2^24");
    if (own_error) return fail(UQ_E_INVALID, own_error);
    if (n == 0 || dim == 0) return UQ_OK;
    if (own_null || !c.x || !c.signs || !c.table_xp || !c.prng_seeds || !c.info) return fail(UQ_E_INVALID, "null pointer");
    if (!c.px_state && !c.px_seeds) return fail(UQ_E_INVALID, "px_state or px_seeds is required");
    const RhtLayout w = rht_layout(n, dim);
    const size_t joff = quicfl_jump_off(n, dim);
    const QflPlan P = qfl_plan(UQ_QFL_SENDER, n, w.D, hooks, SIZE_MAX);
    if (!c.ws || c.ws_bytes < joff + P.jump_bytes + c.ws_extra) return fail(UQ_E_WORKSPACE, "workspace too small");
    t_last_plan[UQ_QFL_SENDER] = P;
    hipStream_t st = (hipStream_t)c.stream;
    char* wsb = (char*)c.ws;
    uint32_t* jump = (uint32_t*)(wsb + joff);
    q.tab = (const float2*)c.table_xp;
    q.tabp = c.table_packed;
    q.numel = c.table_numel;
    q.half = ((c.table_numel / c.h_len) - 1) * c.h_len / 2;                                   // AS:443
    q.h_len = c.h_len;
    q.delta = c.delta;
    q.sqrtD = (float)std::sqrt((double)w.D);                                                  // np.sqrt(D) -> f32
    q.prng_seeds = c.prng_seeds;
    q.px_state = c.px_state;
    q.px_seeds = c.px_seeds;
    q.px_state_out = c.px_state_out;
    q.hbuf = (uint8_t*)(wsb + quicfl_h_off(n, dim));
    q.scale = c.scale;
    q.info = c.info;
    q.D = w.D;
    q.n = n;
    q.force_timeout = P.force_timeout;
    q.nrm = (const float*)(wsb + w.nrm_off);
    int rc = UQ_OK;
    const uint32_t* polys = nullptr;
    if (P.side == UQ_QFL_SIDE_JUMP && (rc = qfl_jump_polys(P, false, &polys))) return rc;
    std::optional<SideFork> fk;
    if (P.side != UQ_QFL_SIDE_NONE) {
        fk.emplace(st, &rc);
        if (rc || (rc = quicfl_send_side(q, P, polys, jump, fk->side()))) return rc;
    }
    if ((rc = rht_norm_front(c.x, n, dim, c.signs, c.sign_row, wsb, rot, st))) return rc;     // AS:460-470
    if (fk && (rc = fk->join())) return rc;
    q.rot = *rot;
    if (q.rtab) q.pre = *rot;                // in place: a coordinate's rot is loaded a round before its value is stored
    return launch_quicfl_send(q, x_kind, P, jump, payload_bits, st);
}

int uq_quicfl_compress_f32(const float* x, int64_t n, int64_t dim, const int8_t* signs, const int32_t* sign_row,
                           const float* table_xp, const uint32_t* table_packed, int64_t table_numel, int32_t h_len,
                           float delta, const int32_t* prng_seeds, const uint32_t* px_state, const int32_t* px_seeds,
                           uint32_t* px_state_out, void* X, int32_t x_kind, uint8_t* exact_mask, float* exact_vals,
                           int32_t* exact_count, float* scale, int32_t* info, void* ws, size_t ws_bytes,
                           void* stream) {
    const QflSendCall c{x, n, dim, signs, sign_row, table_xp, table_packed, table_numel, h_len, delta, prng_seeds,
                        px_state, px_seeds, px_state_out, scale, info, ws, ws_bytes, stream};
    QflSendArgs q{};
    q.X = X;
    q.x_kind = x_kind;
    q.mask = exact_mask;
    q.ev = exact_vals;
    q.ecount = exact_count;
    float* rot = nullptr;
    return quicfl_send(c, x_kind != 0 && x_kind != 1 ? "x_kind must be 0 (int64) or 1 (uint8)" : nullptr,
                       !X || !exact_mask || !exact_vals || !exact_count || !scale, q, x_kind, &rot);
}

// QUICFL_quantize (AS:814-832) for a batch: the sender as uq_quicfl_compress_f32 with the
// receiver fused into its stage 2 (no second h stream, no message in HBM), then the receiver's
// inverse RHT into out [n][dim].
int uq_quicfl_quantize_f32(const float* x, int64_t n, int64_t dim, const int8_t* signs, const int32_t* sign_row,
                           const float* table_xp, const uint32_t* table_packed, int64_t table_numel, int32_t h_len,
                           float delta, const float* recv_table, int32_t recv_numel, const int32_t* prng_seeds,
                           const uint32_t* px_state, const int32_t* px_seeds, uint32_t* px_state_out, float* out,
                           float* scale, int32_t* info, void* ws, size_t ws_bytes, void* stream) {
    const QflSendCall c{x, n, dim, signs, sign_row, table_xp, table_packed, table_numel, h_len, delta, prng_seeds,
                        px_state, px_seeds, px_state_out, scale, info, ws, ws_bytes, stream};
    QflSendArgs q{};
    q.rtab = recv_table;
    q.rtab_n = recv_numel;
    float* rot = nullptr;
    const int rc = quicfl_send(c, recv_numel < 1 || recv_numel > kQflRecvTab ? "receiver table must hold 1..1024 entries" : nullptr,
                               !recv_table || !out, q, 2, &rot);        // (2: the fused instances)  AS:455-503, 526-532
    if (rc || !rot) return rc;
    return rht_inverse(rot, out, n, rht_layout(n, dim).D, dim, signs, sign_row, (hipStream_t)stream);   // AS:533-535
}

// ---- the packed message (it replaces nothing of the reference: AS:494-503 keeps X and the mask) ----
// Form of a packed call: the sender's and the receiver's own rounds write / read the planes (fused), or
// the u8 kernels run on X and mask rows in the workspace and the converters stand between them and the
// message (packed hook bit 0).  DESIGN §4.4 has the measurement behind "fused everywhere".
#define UQ_QFL_PACKED_FUSED 1
#define UQ_QFL_PACKED_CONVERTER 2
extern "C++" {
namespace {
struct QflPackedPlan {
    int32_t nbits = 0, form = 0;
    int64_t P = 0, pitch = 0;
};
thread_local QflPackedPlan t_last_qpacked[2];        // uq_test_last_quicfl_packed_plan, per side

// nbits and D of a packed row (host only): the message of the first failed check, or null
const char* qfl_packed_shape_error(int64_t D, int32_t nbits) {
    if (nbits < 1 || nbits > 4) return "nbits must be 1..4";
    if (D < 1 || (D & (D - 1))) return "D must be a power of two";
    if (D > ((int64_t)1 << 28)) return "at most 2^28 coordinates per message";
    return nullptr;
}
QflPackedPlan qfl_packed_plan(int64_t D, int32_t nbits, int hooks) {
    QflPackedPlan k;
    k.nbits = nbits;
    k.form = (hooks & 1) ? UQ_QFL_PACKED_CONVERTER : UQ_QFL_PACKED_FUSED;
    k.P = (D + 31) / 32;
    k.pitch = nbits * k.P;
    return k;
}
// the converter path's rows behind a u8 call's own workspace: X [n][D] u8, mask [n][D] u8, flags [n]
size_t qfl_conv_bytes(int64_t n, int64_t D) { return up256(2 * (size_t)n * (size_t)D) + up256((size_t)n * sizeof(int32_t)); }
}  // namespace
}  // extern "C++"

int uq_test_set_quicfl_packed_hooks(int flags) { return g_quicfl_packed_hooks.exchange(flags & 1); }

int uq_test_last_quicfl_packed_plan(int32_t side, int64_t* plan_out, int32_t cap) {
    if (side != UQ_QFL_SENDER && side != UQ_QFL_RECEIVER) return fail(UQ_E_INVALID, "side must be 0 (sender) or 1 (receiver)");
    if (!plan_out || cap < 0) return fail(UQ_E_INVALID, "null plan output");
    const QflPackedPlan& k = t_last_qpacked[side];
    const int64_t f[4] = {k.nbits, k.form, k.P, k.pitch};
    for (int i = 0; i < std::min<int32_t>(cap, 4); ++i) plan_out[i] = f[i];
    return UQ_OK;
}

int uq_quicfl_packed_words(int64_t D, int32_t nbits, int64_t* pitch_words) {
    if (!pitch_words) return fail(UQ_E_INVALID, "null pitch_words");
    if (const char* e = qfl_packed_shape_error(D, nbits)) return fail(UQ_E_INVALID, e);
    *pitch_words = nbits * ((D + 31) / 32);
    return UQ_OK;
}

int uq_quicfl_pack_x(const void* X, int32_t x_kind, int64_t n, int64_t D, int32_t nbits, const uint8_t* exact_mask,
                     uint32_t* payload, int32_t* exact_index, int32_t* exact_count, int64_t* payload_bits, int32_t* info,
                     void* stream) {
    if (n < 0) return fail(UQ_E_INVALID, "n must be >= 0");
    if (n > 65535) return fail(UQ_E_INVALID, "at most 65535 messages per call");
    if (x_kind < 0 || x_kind > 2) return fail(UQ_E_INVALID, "x_kind must be 0 (int64), 1 (uint8) or 2 (int32)");
    if (const char* e = qfl_packed_shape_error(D, nbits)) return fail(UQ_E_INVALID, e);
    if (n == 0) return UQ_OK;
    if (!X || !payload || !exact_index || !exact_count) return fail(UQ_E_INVALID, "null pointer");
    hipLaunchKernelGGL(quicfl_pack_x_kernel, dim3((unsigned)n), dim3(256), 0, (hipStream_t)stream, X, x_kind, D, nbits, exact_mask,
                       payload, exact_index, exact_count, payload_bits, info, 0);
    return launched("quicfl_pack_x_kernel launch");
}

int uq_quicfl_unpack_x(const uint32_t* payload, int64_t n, int64_t D, int32_t nbits, const int32_t* exact_index,
                       const int32_t* exact_count, uint8_t* X_u8, uint8_t* exact_mask, int32_t* info, void* stream) {
    if (n < 0) return fail(UQ_E_INVALID, "n must be >= 0");
    if (n > 65535) return fail(UQ_E_INVALID, "at most 65535 messages per call");
    if (const char* e = qfl_packed_shape_error(D, nbits)) return fail(UQ_E_INVALID, e);
    if (n == 0) return UQ_OK;
    if (!payload || !X_u8 || !exact_mask) return fail(UQ_E_INVALID, "null pointer");
    if ((exact_index == nullptr) != (exact_count == nullptr)) return fail(UQ_E_INVALID, "exact_index and exact_count go together");
    hipLaunchKernelGGL(quicfl_unpack_x_kernel, dim3((unsigned)n), dim3(256), 0, (hipStream_t)stream, payload, D, nbits, exact_index,
                       exact_count, X_u8, exact_mask, info);
    return launched("quicfl_unpack_x_kernel launch");
}

int uq_quicfl_packed_workspace_bytes(int64_t n, int64_t dim, size_t* bytes_out) {
    const int rc = uq_quicfl_workspace_bytes(n, dim, bytes_out);
    if (rc) return rc;
    *bytes_out = up256(*bytes_out) + qfl_conv_bytes(n, rht_layout(n, dim).D);
    return UQ_OK;
}

int uq_quicfl_compress_packed_f32(const float* x, int64_t n, int64_t dim, const int8_t* signs, const int32_t* sign_row,
                                  const float* table_xp, const uint32_t* table_packed, int64_t table_numel, int32_t h_len,
                                  float delta, const int32_t* prng_seeds, const uint32_t* px_state, const int32_t* px_seeds,
                                  uint32_t* px_state_out, uint32_t* payload, int32_t nbits, int32_t* exact_index,
                                  float* exact_vals, int32_t* exact_count, int64_t* payload_bits, float* scale, int32_t* info,
                                  void* ws, size_t ws_bytes, void* stream) {
    const int hooks = g_quicfl_packed_hooks.load();
    t_last_qpacked[UQ_QFL_SENDER] = QflPackedPlan{};
    t_last_plan[UQ_QFL_SENDER] = QflPlan{};
    const char* own_error = nbits < 1 || nbits > 4 ? "nbits must be 1..4" : nullptr;
    const bool own_null = !payload || !exact_index || !exact_vals || !exact_count || !payload_bits || !scale;
    // the u8 call's workspace, then the converter path's rows (whichever form runs: one size per shape)
    size_t base0 = 0, base = 0;
    int64_t D = 0;
    if (n > 0 && dim > 0 && n <= 65535 && dim <= ((int64_t)1 << 28)) {
        if (const int rc = uq_quicfl_workspace_bytes(n, dim, &base0)) return rc;
        base = up256(base0);
        D = rht_layout(n, dim).D;
    }
    const QflSendCall c{x, n, dim, signs, sign_row, table_xp, table_packed, table_numel, h_len, delta, prng_seeds,
                        px_state, px_seeds, px_state_out, scale, info, ws, ws_bytes, stream,
                        base - base0 + qfl_conv_bytes(n > 0 ? n : 0, D)};
    const QflPackedPlan k = qfl_packed_plan(D, nbits, hooks);
    float* rot = nullptr;
    QflSendArgs q{};
    q.ev = exact_vals;
    q.ecount = exact_count;
    if (k.form == UQ_QFL_PACKED_FUSED) {
        q.X = payload;
        q.x_kind = 3;
        q.nbits = nbits;
        q.eidx = exact_index;
        const int rc = quicfl_send(c, own_error, own_null, q, 3, &rot, payload_bits);
        if (!rc && rot) t_last_qpacked[UQ_QFL_SENDER] = k;
        return rc;
    }
    // the converter path: the u8 sender into the workspace's rows, then the converter (info ORed into)
    uint8_t* Xu = (uint8_t*)ws + base;
    uint8_t* mk = Xu + (size_t)(n > 0 ? n : 0) * D;
    q.X = Xu;
    q.x_kind = 1;
    q.mask = mk;
    int rc = quicfl_send(c, own_error, own_null, q, 1, &rot);
    if (rc || !rot) return rc;
    hipLaunchKernelGGL(quicfl_pack_x_kernel, dim3((unsigned)n), dim3(256), 0, (hipStream_t)stream, (const void*)Xu, 1, D, nbits,
                       (const uint8_t*)mk, payload, exact_index, exact_count, payload_bits, info, 1);
    if ((rc = launched("quicfl_pack_x_kernel launch"))) return rc;
    t_last_qpacked[UQ_QFL_SENDER] = k;
    return UQ_OK;
}

int uq_quicfl_receive_packed_workspace_bytes(int64_t n, int64_t D, size_t* bytes_out) {
    const int rc = uq_quicfl_receive_workspace_bytes(n, D, bytes_out);
    if (rc) return rc;
    *bytes_out = up256(*bytes_out) + qfl_conv_bytes(n, D);
    return UQ_OK;
}

int uq_quicfl_receive_packed_f32(const uint32_t* payload, int32_t nbits, int64_t n, int64_t D, const float* recv_table,
                                 int32_t table_rows, int32_t h_len, const int32_t* prng_seeds, const int32_t* exact_index,
                                 const float* exact_vals, const int32_t* exact_count, const float* scale, float* out,
                                 int32_t* info, void* ws, size_t ws_bytes, void* stream) {
    const int hooks = g_quicfl_packed_hooks.load();
    t_last_qpacked[UQ_QFL_RECEIVER] = QflPackedPlan{};
    t_last_plan[UQ_QFL_RECEIVER] = QflPlan{};
    if (n < 0) return fail(UQ_E_INVALID, "n must be >= 0");
    if (n > 65535) return fail(UQ_E_INVALID, "at most 65535 clients per call");
    if (const char* e = qfl_packed_shape_error(D, nbits)) return fail(UQ_E_INVALID, e);
    if (n == 0) return UQ_OK;
    if (!payload || !recv_table || !prng_seeds || !scale || !out) return fail(UQ_E_INVALID, "null pointer");
    if ((exact_index == nullptr) != (exact_vals == nullptr) || (exact_index == nullptr) != (exact_count == nullptr))
        return fail(UQ_E_INVALID, "exact_index, exact_vals and exact_count go together");
    size_t base = 0;
    if (const int rc = uq_quicfl_receive_workspace_bytes(n, D, &base)) return rc;
    base = up256(base);
    if (!ws || ws_bytes < base + qfl_conv_bytes(n, D)) return fail(UQ_E_WORKSPACE, "workspace too small");
    hipStream_t st = (hipStream_t)stream;
    const QflPackedPlan k = qfl_packed_plan(D, nbits, hooks);
    int rc;
    if (k.form == UQ_QFL_PACKED_FUSED) {
        // the rounds on the planes (no mask, no exact values), then the exact coordinates from their list
        if ((rc = quicfl_receive(payload, 3, nbits, n, D, recv_table, table_rows, h_len, prng_seeds, nullptr, nullptr, 0, nullptr,
                                 scale, out, info, ws, base, stream)))
            return rc;
        if (exact_index) {
            hipLaunchKernelGGL(quicfl_exact_scatter_kernel, dim3((unsigned)n), dim3(256), 0, st, exact_index, exact_vals,
                               exact_count, scale, out, info, D);
            if ((rc = launched("quicfl_exact_scatter_kernel launch"))) return rc;
        }
    } else {
        // the converter path: X and the mask rebuilt in the workspace, the u8 receiver on them; the list's
        // own check (order included, which a mask cannot show) joins the receiver's flags
        char* conv = (char*)ws + base;
        uint8_t* Xu = (uint8_t*)conv;
        uint8_t* mk = Xu + (size_t)n * D;
        int32_t* linfo = (int32_t*)(conv + up256(2 * (size_t)n * (size_t)D));
        hipLaunchKernelGGL(quicfl_unpack_x_kernel, dim3((unsigned)n), dim3(256), 0, st, payload, D, nbits, exact_index, exact_count,
                           Xu, mk, linfo);
        if ((rc = launched("quicfl_unpack_x_kernel launch"))) return rc;
        if ((rc = quicfl_receive(Xu, 1, 0, n, D, recv_table, table_rows, h_len, prng_seeds, exact_index ? mk : nullptr,
                                 exact_index ? exact_vals : nullptr, 1, exact_count, scale, out, info, ws, base, stream)))
            return rc;
        if (info) {
            hipLaunchKernelGGL(quicfl_or_info_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, info, (const int32_t*)linfo, n);
            if ((rc = launched("quicfl_or_info_kernel launch"))) return rc;
        }
    }
    t_last_qpacked[UQ_QFL_RECEIVER] = k;
    return UQ_OK;
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
