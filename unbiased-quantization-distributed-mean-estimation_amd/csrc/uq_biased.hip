// uq_biased.hip — the biased type quantizer (Reznik rounding): the dispatch plan, the workspace
// layout, the torch tie replay's host code (KB7 / KB7a with its captured level graphs) and the C
// API uq_type_biased_f32 over uq_biased_kernels.h and uq_biased_torch_ties.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <tuple>
#include <type_traits>

#include "uq_biased_torch_ties.h"
#include "uq_internal.h"

namespace {

// test hook (uq_test_force_replay_failure): every torch-tie replay takes its failure path
std::atomic<int> g_force_replay_failure{0};

// batches of at most this many clients run the candidate digits (KB4d) over many workgroups
// per client (one workgroup per client walks up to d/8 keys twice)
constexpr int64_t kCandMultiMaxN = 16;

// ---- dispatch plan -------------------------------------------------------------------
// Every decision of a call, made once on the host from (n, d, tie_policy, alignment of x, out
// and, in a codes call, the codes rows); DESIGN.md §4.2 has the table.  The launchers launch what the plan names and the
// workspace layout reads its sizes, so the test hooks (uq_test_biased_plan,
// uq_test_last_biased_plan) report what a call really runs.
struct BiasedPlan {
    int32_t front = UQ_BIASED_FRONT_NONE;
    int32_t ties = UQ_BIASED_TIES_LOWEST;   // the tail after the selection (small-checked: if a row is ambiguous)
    int32_t levels = 0, lsplit = 0;         // KB7a's levels, lsplit of them before KB6; 0: one rez_ties_kernel launch
    uint32_t lgrid = 0;                     // workgroups of KB7a's per-level launches
    bool vec4 = false;                      // 16-byte accesses to x and out, 4-byte ones to the codes
    bool cand_multi = false;                // KB4d over cspans workgroups per client
    bool clear_bits = false;                // a memset clears the tie bits (KB7a's level-0 kt_count does it otherwise)
    uint32_t cspans = 0;
    uint32_t cap = 0;       // candidate region per client in u32 (KB6f lists cap / 2 (index, key) pairs)
    uint32_t capf = 0;      // listed pairs per client at most: a larger fine bucket takes the full-row passes
    int32_t tiles = 0;      // output tiles per client
    int32_t slots = 0;      // KB7's workgroups and scratch slots, S = min(n, kTieSlots)
    int32_t ran = -1;       // uq_test_last_biased_plan's outcome field
};

// The entry point's checks of its shape and policy, in its order (the hook passes m = 0, T = 1).
int biased_check(int64_t n, int64_t d, int64_t m, int32_t T, int32_t tie_policy) {
    if (n < 0 || d < 0) return fail(UQ_E_INVALID, "n and d must be >= 0");
    if (m < 0) return fail(UQ_E_INVALID, "m must be >= 0");
    if (d >= ((int64_t)1 << 31)) return fail(UQ_E_INVALID, "d must be < 2^31");
    if (n > 65535) return fail(UQ_E_INVALID, "at most 65535 clients per call");
    if (T < 1) return fail(UQ_E_INVALID, "torch_threads must be >= 1");
    tie_policy &= ~UQ_TIES_HOST_CHECK;
    if (tie_policy != UQ_TIES_LOWEST_INDEX && tie_policy != UQ_TIES_TORCH)
        return fail(UQ_E_INVALID, "unknown tie_policy");
    return UQ_OK;
}

// out_aligned: true where a codes call writes no out; codes_aligned: the codes rows start on
// 4-byte boundaries (true where the call writes no codes)
BiasedPlan biased_plan(int64_t n, int64_t d, int32_t tie_policy, bool x_aligned, bool out_aligned,
                       bool codes_aligned = true) {
    BiasedPlan p;
    p.tiles = (int32_t)((d + kSelTile - 1) / kSelTile);
    p.slots = (int32_t)std::min<int64_t>(n, kTieSlots);
    p.cap = (uint32_t)std::min<int64_t>(std::max<int64_t>(d, 1), std::max<int64_t>(4096, d / 8));
    p.capf = p.cap / 2;
    p.cspans = (p.capf + kCandSpan - 1) / kCandSpan;
    if (n == 0 || d == 0) return p;
    const bool host_check = (tie_policy & UQ_TIES_HOST_CHECK) != 0;
    const bool torch = (tie_policy & ~UQ_TIES_HOST_CHECK) == UQ_TIES_TORCH;
    // vectors shorter than GRAIN: one launch (KB-small) with the lowest-index rule; with torch
    // ties only under UQ_TIES_HOST_CHECK, which reads the clients' flags back and runs the
    // multi-kernel path when a threshold tie needs torch's choice
    const bool small = d <= kSmallBiasedMax && (!torch || (host_check && n <= kSmallCheckMaxN));
    p.front = !small ? UQ_BIASED_FRONT_FULL : torch ? UQ_BIASED_FRONT_SMALL_CHECKED : UQ_BIASED_FRONT_SMALL;
    p.vec4 = x_aligned && out_aligned && codes_aligned && d % 4 == 0;
    p.cand_multi = n <= kCandMultiMaxN && p.cspans > 1;
    if (!torch) return p;
    // KB7a pays ~85 short launches whether or not any client is listed (the host does not
    // know): worth it for batches, where ~3 % of Gaussian clients are ambiguous at R = 1 and
    // several replays would share one workgroup each, and for vectors of 2^21 and more, whose
    // one-workgroup replay takes milliseconds; a few-client call at smaller d (the per-vector
    // drop-ins) replays in one kernel when it has to
    const bool kb7a = d > kTieLevelMin && (n >= kTieLevelMinClients || d >= kTieLevelBigD);
    // (the host check pays only where the replay would be KB7a's level chain; a one-kernel
    // replay costs less than the synchronisation)
    p.ties = host_check && kb7a ? UQ_BIASED_TIES_CHECKED : UQ_BIASED_TIES_FORK;
    p.clear_bits = !kb7a;
    if (!kb7a) return p;
    // a level keeps the side of the cut that holds nth, half the range on average; an idle
    // level costs four ~6 us launches, and a range still longer continues in part 1's workgroup
    p.levels = kTieLevelMargin;
    for (int64_t r = d; r > kTieLevelStop; r = (r + 1) / 2) ++p.levels;
    p.lsplit = std::min(kTieHeavyLevels, p.levels);
    // the per-level launches take (active slot, segment) items, one per wave: S slots need at
    // most S * kTieSegs / 4 workgroups (a one-client call launched 2048, 1984 of them idle)
    p.lgrid = (uint32_t)std::min<int64_t>(kTieGrid, (int64_t)p.slots * kTieSegs / 4);
    return p;
}

thread_local BiasedPlan t_last_plan;         // uq_test_last_biased_plan

int export_plan(const BiasedPlan& p, int64_t* out, int32_t cap) {
    if (!out || cap < 0) return fail(UQ_E_INVALID, "null plan output");
    const int replay = p.ties == UQ_BIASED_TIES_LOWEST ? UQ_BIASED_REPLAY_NONE
                       : p.levels                      ? UQ_BIASED_REPLAY_LEVELS
                                                       : UQ_BIASED_REPLAY_ONE_KERNEL;
    const int64_t f[UQ_BIASED_PLAN_FIELDS] = {p.front, p.ties, replay, p.levels, p.lsplit, p.lgrid, p.slots, p.vec4,
                                              p.cand_multi, p.cspans, p.cap, p.capf, p.tiles, p.clear_bits, p.ran};
    for (int i = 0; i < std::min<int32_t>(cap, UQ_BIASED_PLAN_FIELDS); ++i) out[i] = f[i];
    return UQ_OK;
}

// Biased-quantizer workspace: [ctrl 256][K1 parts][l1 n][m' n][state n x 32B]
// [hist n x 3 x 2048 u32][zero/NaN counts n x 2][candidate counts n][candidates n x cap u32]
// [tie counts n x tiles u32][tie bits n x ceil(d/32) u32]
// [KB7 slots: keys + indices S x 2d u32][KB7 positions S x 2d u32], S = the plan's slots
// ... [codes calls: the largest coded count per output tile, n x tiles i32]
struct BiasedLayout {
    size_t part_off, l1_off, msum_off, st_off, hist_off, zn_off, cn_off, fl_off, cand_off, tcnt_off, bits_off,
        pairs_off, pos_off, list_off, tls_off, tcnt2_off, alist_off, kmt_off, total;
};

// codes: the layout of a codes call (uq_biased_codes_workspace_bytes), with the tile maxima at the end
BiasedLayout biased_layout(int64_t n, int64_t d, const L1Plan& plan, const BiasedPlan& P, bool codes = false) {
    BiasedLayout w{};
    w.part_off = kCtrlBytes;
    w.l1_off = up256(w.part_off + (size_t)n * plan.total_groups * 32 * sizeof(float));
    w.msum_off = up256(w.l1_off + (size_t)n * sizeof(float));
    w.st_off = up256(w.msum_off + (size_t)n * sizeof(float));
    w.hist_off = up256(w.st_off + (size_t)n * sizeof(RezState));
    w.zn_off = up256(w.hist_off + (size_t)n * kHistSlots * kRadixBins * sizeof(uint32_t));
    w.cn_off = w.zn_off + (size_t)n * 2 * sizeof(uint32_t);           // zn and cand_n adjacent
    w.fl_off = w.cn_off + (size_t)n * sizeof(uint32_t);               // the full clients' list (zeroed count)
    w.cand_off = up256(w.fl_off + (size_t)(n + 1) * sizeof(uint32_t));
    w.tcnt_off = up256(w.cand_off + (size_t)n * P.cap * sizeof(uint32_t));
    w.bits_off = up256(w.tcnt_off + (size_t)n * P.tiles * sizeof(uint32_t));
    w.pairs_off = up256(w.bits_off + (size_t)n * ((d + 31) / 32) * sizeof(uint32_t));
    w.pos_off = up256(w.pairs_off + (size_t)P.slots * 2 * ((d + 3) & ~(int64_t)3) * sizeof(uint32_t) + 16);
    w.list_off = up256(w.pos_off + (size_t)P.slots * 2 * d * sizeof(uint32_t));
    w.tls_off = up256(w.list_off + (size_t)(n + 1) * sizeof(uint32_t));    // KB7's client list
    w.tcnt2_off = up256(w.tls_off + (size_t)P.slots * sizeof(TieLevelState));
    w.alist_off = up256(w.tcnt2_off + (size_t)P.slots * kTieSegs * 2 * sizeof(uint32_t));
    w.kmt_off = up256(w.alist_off + (size_t)(kTieSlots + 1) * sizeof(uint32_t));    // KB7a's active slots
    w.total = codes ? up256(w.kmt_off + (size_t)n * P.tiles * sizeof(int32_t)) : w.kmt_off;
    return w;
}

// What the launchers of one call share: its arguments, plan, and workspace regions.
struct BiasedCall {
    const float* x;
    float* out;
    int64_t n, d;
    float fm;
    const BiasedPlan& P;
    const BiasedLayout& w;
    char* wsb;
    hipStream_t st;                     // the caller's stream
    int8_t* codes = nullptr;            // a codes call (uq_type_biased_codes_f32): the codes [n][d] and kmax [n];
    int32_t* kmax = nullptr;            // out may then be null (codes only)
    int32_t* kmt = (int32_t*)(wsb + w.kmt_off);         // the writers' per-tile maxima, folded into kmax at the end
    float* l1buf = (float*)(wsb + w.l1_off);
    RezState* state = (RezState*)(wsb + w.st_off);
    uint32_t* hist = (uint32_t*)(wsb + w.hist_off);
    uint32_t* zn = (uint32_t*)(wsb + w.zn_off);
    uint32_t* cand_n = (uint32_t*)(wsb + w.cn_off);
    uint32_t* flist = (uint32_t*)(wsb + w.fl_off);      // KB4a's list of the full clients ([0] = count)
    uint2* fcand = (uint2*)(wsb + w.cand_off);
    uint32_t* tcnt = (uint32_t*)(wsb + w.tcnt_off);
    uint32_t* bits = (uint32_t*)(wsb + w.bits_off);
    uint32_t* list = (uint32_t*)(wsb + w.list_off);     // KB7's list of the ambiguous clients ([0] = count)
    unsigned listed_y = (unsigned)std::min<int64_t>(n, kListedGridY);   // y extent of the list-strided grids
};

// f(V4) launches the float4 (true) or scalar (false) instance it names, f(D) for D = 0, 1, 2
// the instances of a radix digit.  (true before false, digit by digit: the order the instances
// have always been emitted in, which tools/kernel_table.py's hashes depend on.)
template <int D>
using Digit = std::integral_constant<int, D>;
template <class F>
void select_vec4(bool vec4, F&& f) {
    if (vec4) f(Flag<true>{});
    else f(Flag<false>{});
}
// f(CM) for the codes mode of a codes call: kOutCodes, or kCodesOnly without out.
template <int M>
using Mode = std::integral_constant<int, M>;
template <class F>
void select_codes(const float* out, F&& f) {
    if (out) f(Mode<kOutCodes>{});
    else f(Mode<kCodesOnly>{});
}
template <class F>
void each_digit(F&& f) {
    f(Digit<0>{});
    f(Digit<1>{});
    f(Digit<2>{});
}

// KB7's replay kernel on ts, one workgroup per slot.  part 0 (tls null): every listed client,
// start to end.  After KB7a's levels (tls): part 1 the replays' LDS tails in small workgroups,
// part 2 the heap-path clients and the list entries beyond the slots.
int launch_replay(const BiasedCall& c, hipStream_t ts, const TieLevelState* tls, int part) {
    hipLaunchKernelGGL(rez_ties_kernel<kTieThreads>, dim3((unsigned)c.P.slots), dim3(kTieThreads), 0, ts, c.x, c.d, c.l1buf,
                       c.fm, c.state, c.bits, (uint32_t*)(c.wsb + c.w.pairs_off), (uint32_t*)(c.wsb + c.w.pos_off), c.list,
                       (uint32_t*)c.wsb, tls, part, c.tcnt, c.P.tiles, g_force_replay_failure.load());
    return launched("rez_ties_kernel launch");
}

// KB7's client list, and cleared tie bits where the plan says so, before launch_torch_ties and
// the tie counts.
int torch_ties_prepare(const BiasedCall& c) {
    if (c.P.clear_bits) {
        const int rc = hip_check(hipMemsetAsync(c.bits, 0, (size_t)c.n * ((c.d + 31) / 32) * sizeof(uint32_t), c.st),
                                 "memset tie bits");
        if (rc) return rc;
    }
    hipLaunchKernelGGL(rez_tie_list_kernel, dim3(1), dim3(1024), 0, c.st, c.state, c.n, c.list);
    return launched("rez_tie_list_kernel launch");
}

// Captured KB7a level chains, per thread (streams and workspaces are per thread in practice):
// keyed by (device, every pointer the chain's kernels take, d, slots, levels).  *exec =
// nullptr when capture is unavailable (then the caller launches the chain directly).
struct LevelKey {
    int dev;                            // (level_graph fills it in)
    const void *qbuf, *list, *tls, *cnt, *pos, *alist;
    int64_t d;
    unsigned S;
    int levels;                         // lv0 * 256 + lv1: the captured range of levels
    auto tied() const { return std::tie(dev, qbuf, list, tls, cnt, pos, alist, d, S, levels); }
};
template <class F>
int level_graph(LevelKey key, hipStream_t st, F&& launch, hipGraphExec_t* exec) {
    struct Entry {
        LevelKey key;
        hipGraphExec_t exec;
    };
    static thread_local Entry cache[8] = {};
    static thread_local int next = 0;
    int rc = hip_check(hipGetDevice(&key.dev), "hipGetDevice");
    if (rc) return rc;
    for (const Entry& e : cache)
        if (e.exec && e.key.tied() == key.tied()) {
            *exec = e.exec;
            return UQ_OK;
        }
    *exec = nullptr;
    if (hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal) != hipSuccess) {
        (void)hipGetLastError();
        return UQ_OK;                                   // not capturable here: launch directly
    }
    const int lrc = launch(st);
    hipGraph_t g = nullptr;
    const hipError_t ec = hipStreamEndCapture(st, &g);
    if (lrc) {
        if (g) (void)hipGraphDestroy(g);
        return lrc;
    }
    if ((rc = hip_check(ec, "end KB7a capture"))) return rc;
    hipGraphExec_t ex = nullptr;
    rc = hip_check(hipGraphInstantiate(&ex, g, nullptr, nullptr, 0), "instantiate KB7a graph");
    (void)hipGraphDestroy(g);
    if (rc) return rc;
    Entry& slot = cache[next];
    next = (next + 1) % 8;
    if (slot.exec) (void)hipGraphExecDestroy(slot.exec);
    slot = Entry{key, ex};
    *exec = ex;
    return UQ_OK;
}

// KB7 on stream `ts`.  Without KB7a (the plan has no levels) one launch replays every listed
// client.  With KB7a, the replay's LDS tails run here in small workgroups (part 1) and
// *tls_out is set: the caller then runs launch_replay's part 2 (heap-path clients and list
// entries beyond the slots) once the output kernel on its own stream is done.
// mid(): called once KB7a's first lsplit levels are enqueued on `ts` (with KB7a; before
// anything else otherwise) -- the fork makes KB6 part 1 wait there, so the bandwidth-heavy
// first levels (the listed clients' full rows) do not share HBM with KB6 and KB6 runs beside
// the later, latency-bound levels instead.
template <class Mid>
int launch_torch_ties(const BiasedCall& c, hipStream_t ts, const TieLevelState** tls_out, Mid&& mid) {
    *tls_out = nullptr;
    const BiasedPlan& P = c.P;
    int rc = UQ_OK;
    if (!P.levels) return (rc = mid()) ? rc : launch_replay(c, ts, nullptr, 0);
    // KB7a: introselect's levels over (segments x slots) workgroups, level by level, down to
    // ranges that fit the LDS tail
    const int64_t d = c.d;
    const unsigned S = (unsigned)P.slots, lgrid = P.lgrid;
    uint32_t* qbuf = (uint32_t*)(c.wsb + c.w.pairs_off);
    uint32_t* pos = (uint32_t*)(c.wsb + c.w.pos_off);
    TieLevelState* tls = (TieLevelState*)(c.wsb + c.w.tls_off);
    uint32_t* cnt = (uint32_t*)(c.wsb + c.w.tcnt2_off);
    uint32_t* alist = (uint32_t*)(c.wsb + c.w.alist_off);
    // level 0's pivot and counts with the queue fill from x (x, l1 and the states are
    // per-call arguments: launched directly, not captured)
    hipLaunchKernelGGL(kt_count_kernel, dim3(lgrid), dim3(256), 0, ts, c.x, d, c.l1buf, c.fm, (const RezState*)c.state, qbuf,
                       c.list, tls, cnt, alist, c.bits, (int)S, kTieLevelStop, 1);
    if ((rc = launched("kt_count_kernel launch"))) return rc;
    auto levels_on = [&](hipStream_t ls, int lv0, int lv1) {
        for (int lv = lv0; lv < lv1; ++lv) {
            if (lv > 0)
                hipLaunchKernelGGL(kt_count_kernel, dim3(lgrid), dim3(256), 0, ls, (const float*)nullptr, d,
                                   (const float*)nullptr, c.fm, (const RezState*)nullptr, qbuf, c.list, tls, cnt, alist,
                                   (uint32_t*)nullptr, (int)S, kTieLevelStop, 0);
            hipLaunchKernelGGL(kt_list_kernel, dim3(lgrid), dim3(256), 0, ls, d, qbuf, pos, tls, cnt, alist);
            hipLaunchKernelGGL(kt_jcut_kernel, dim3(S), dim3(kJcutThreads), 0, ls, d, qbuf, pos, tls, cnt, alist);
            hipLaunchKernelGGL(kt_swap_kernel, dim3(lgrid), dim3(256), 0, ls, d, qbuf, pos, tls, alist);
        }
        return launched("KB7a level launch");
    };
    // The rest of the level chain (4 dependent launches per level, whether or not a client is
    // listed) is replayed as a captured HIP graph: its arguments are workspace pointers, d, S
    // and the stop only, so one capture serves every call on the same workspace (per-call
    // host cost was ~65 launches, more than the chain's GPU time for a few-client call).
    auto run_levels = [&](int a, int b) {
        if (a >= b) return (int)UQ_OK;
        hipGraphExec_t exec = nullptr;
        int grc = level_graph(LevelKey{0, qbuf, c.list, tls, cnt, pos, alist, d, S, a * 256 + b}, ts,
                              [&](hipStream_t ls) { return levels_on(ls, a, b); }, &exec);
        if (grc) return grc;
        if (exec) return hip_check(hipGraphLaunch(exec, ts), "KB7a level graph launch");
        return levels_on(ts, a, b);
    };
    if ((rc = run_levels(0, P.lsplit))) return rc;
    if ((rc = mid())) return rc;
    if ((rc = run_levels(P.lsplit, P.levels))) return rc;
    hipLaunchKernelGGL(kt_mark_kernel, dim3(kTieMarkSegs, S), dim3(256), 0, ts, d, qbuf, c.list, c.state, tls, c.bits);
    if ((rc = launched("kt_mark_kernel launch"))) return rc;
    *tls_out = tls;
    return launch_replay(c, ts, tls, 1);
}

// KB-small: the whole op in one launch, one workgroup per client.
int launch_small(const BiasedCall& c) {
    static std::atomic<uint64_t> attr_set{0};             // per device (bit = device index < 64)
    int dev = 0;
    if (hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < 64 && !((attr_set.load() >> dev) & 1u)) {
        (void)hipFuncSetAttribute((const void*)biased_small_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)(kSmallBiasedMax * sizeof(uint32_t)));
        attr_set.fetch_or(1ull << dev);
    }
    if (c.codes) {
        static std::atomic<uint64_t> cattr_set{0};            // per device, both codes instances
        if (dev >= 0 && dev < 64 && !((cattr_set.load() >> dev) & 1u)) {
            (void)hipFuncSetAttribute((const void*)biased_small_codes_kernel<kOutCodes>,
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)(kSmallBiasedMax * sizeof(uint32_t)));
            (void)hipFuncSetAttribute((const void*)biased_small_codes_kernel<kCodesOnly>,
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)(kSmallBiasedMax * sizeof(uint32_t)));
            cattr_set.fetch_or(1ull << dev);
        }
        select_codes(c.out, [&](auto CM) {
            hipLaunchKernelGGL(biased_small_codes_kernel<CM()>, dim3((unsigned)c.n), dim3(256), (size_t)c.d * sizeof(uint32_t),
                               c.st, c.x, c.out, c.d, c.fm, (const float*)nullptr, c.l1buf, c.state, c.codes, c.kmt, c.P.tiles);
        });
        return launched("biased_small_codes_kernel launch");
    }
    hipLaunchKernelGGL(biased_small_kernel, dim3((unsigned)c.n), dim3(256), (size_t)c.d * sizeof(uint32_t), c.st, c.x, c.out,
                       c.d, c.fm, (const float*)nullptr, c.l1buf, c.state);
    return launched("biased_small_kernel launch");
}

// The small-checked front's host check: *tie = some client's threshold tie needs torch's choice.
int small_has_tie(const BiasedCall& c, int32_t* tie) {
    SideStream* sb = nullptr;
    int rc = side_stream(&sb);                          // (its pinned states)
    if (rc) return rc;
    rc = hip_check(hipMemcpyAsync(sb->states, c.state, (size_t)c.n * sizeof(RezState), hipMemcpyDeviceToHost, c.st),
                   "copy states");
    if (rc || (rc = hip_check(hipStreamSynchronize(c.st), "sync"))) return rc;
    *tie = 0;
    for (int64_t i = 0; i < c.n; ++i) *tie |= (((const RezState*)sb->states)[i].flags & kRezAmbiguous) != 0;
    return UQ_OK;
}

// The full front up to the selection: KB1, KB2 (with KB4's first histogram), KB3, KB4a, then the
// key digits of the full clients (KB4c) and of the fine ones (KB6f + KB4d).
int launch_select(const BiasedCall& c, int32_t T, const L1Plan& plan) {
    const BiasedPlan& P = c.P;
    const int64_t n = c.n, d = c.d;
    float* part = (float*)(c.wsb + c.w.part_off);
    float* msum = (float*)(c.wsb + c.w.msum_off);
    int rc = launch_l1(c.x, n, d, T, part, c.l1buf, c.st);                                  // AS:680
    if (rc) return rc;
    rc = hip_check(hipMemsetAsync(c.hist, 0, c.w.cand_off - c.w.hist_off, c.st), "memset hist/zn/cand_n");
    if (rc) return rc;
    // AS:648-649 m' = sum k' in torch order, with the first radix digit's histogram (KB2 + KB4 pass 0)
    rc = launch_cascade<RezKHistOp>(c.x, n, d, plan, part, msum, c.l1buf, c.fm, c.st, c.hist, c.zn);
    if (rc) return rc;
    hipLaunchKernelGGL(rez_setup_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c.st, msum, c.fm, d, n, c.state);
    if ((rc = launched("rez_setup_kernel launch"))) return rc;
    // KB4a: the threshold's fine bin; a small bucket makes the client "fine", a large one "full"
    // full clients are listed by KB4a (flist[0] = count, in the zeroed range): the key-digit
    // passes below stride over the list, not over n x spans workgroups that mostly exit
    hipLaunchKernelGGL((rez_select_kernel<0, true>), dim3((unsigned)n), dim3(256), 0, c.st, c.state, c.hist, c.zn, P.capf,
                       c.flist);
    // full clients (tie-heavy rows): the key digits by three full-row histogram passes
    const dim3 hlgrid((unsigned)((d + kHistSpan - 1) / kHistSpan), c.listed_y);
    each_digit([&](auto D) {
        select_vec4(P.vec4, [&](auto V4) {
            hipLaunchKernelGGL((rez_hist_kernel<D(), V4()>), hlgrid, dim3(256), 0, c.st, c.x, d, c.l1buf, c.fm, c.state, c.hist,
                               c.flist);
        });
        hipLaunchKernelGGL((rez_select_kernel<D(), false>), dim3((unsigned)P.slots), dim3(256), 0, c.st, c.state, c.hist, c.zn,
                           P.capf, c.flist);
    });
    // fine clients: KB6f writes every output and lists the bucket, KB4d finds the threshold
    // key among the listed keys, KB6p patches the selected listed coordinates (tie-free clients)
    select_vec4(P.vec4, [&](auto V4) {
        if (c.codes)
            select_codes(c.out, [&](auto CM) {
                hipLaunchKernelGGL((rez_output_fine_codes_kernel<V4(), CM()>), dim3((unsigned)P.tiles, (unsigned)n), dim3(256), 0,
                                   c.st, c.x, c.out, d, c.l1buf, c.fm, c.state, c.fcand, c.cand_n, P.capf, c.codes, c.kmt);
            });
        else
            hipLaunchKernelGGL(rez_output_fine_kernel<V4()>, dim3((unsigned)P.tiles, (unsigned)n), dim3(256), 0, c.st, c.x, c.out, d,
                               c.l1buf, c.fm, c.state, c.fcand, c.cand_n, P.capf);
    });
    if (P.cand_multi) {                          // few clients: the passes over many workgroups
        each_digit([&](auto D) {
            hipLaunchKernelGGL(rez_cand_hist_kernel<D()>, dim3(P.cspans, (unsigned)n), dim3(256), 0, c.st, c.state, c.fcand,
                               c.cand_n, P.capf, c.hist);
            hipLaunchKernelGGL(rez_cand_pick_kernel<D()>, dim3((unsigned)n), dim3(256), 0, c.st, c.state, c.hist);
        });
    } else {
        hipLaunchKernelGGL(rez_cand_select_kernel, dim3((unsigned)n), dim3(256), 0, c.st, c.state, c.fcand, c.cand_n, P.capf);
    }
    return launched("radix select launch");
}

// KB6p: the tie-free fine clients' selected bin coordinates (independent of KB7: with the
// torch-tie fork it runs on the caller's stream beside the replay chain, off its path)
int launch_fine_patch(const BiasedCall& c) {
    if (c.codes)
        select_codes(c.out, [&](auto CM) {
            hipLaunchKernelGGL(rez_fine_patch_codes_kernel<CM()>, dim3(kPatchBlocks, (unsigned)c.n), dim3(256), 0, c.st, c.x,
                               c.out, c.d, c.l1buf, c.fm, c.state, c.fcand, c.cand_n, c.P.capf, c.codes, c.kmt, c.P.tiles);
        });
    else
        hipLaunchKernelGGL(rez_fine_patch_kernel, dim3(kPatchBlocks, (unsigned)c.n), dim3(256), 0, c.st, c.x, c.out, c.d, c.l1buf,
                           c.fm, c.state, c.fcand, c.cand_n, c.P.capf);
    return launched("rez_fine_patch_kernel launch");
}

// KB6 for the clients of a list (list-strided grid): part 0 / 1 over KB4a's list (the full
// clients and those without a selection -- every client KB6f did not write), part 2 over KB7's
// list after the replay, part 3 over the ambiguous ones (their fine clients)
// ol == nullptr: the n x tiles grid (part 1 beside the torch-tie chain: the list-strided
// form was 0.01-0.02 ms slower there, profiles/r5aw_*; the lowest-index batch gains 0.075 ms
// from it, its launches being on the critical path)
int launch_output(const BiasedCall& c, int part, const uint32_t* ol) {
    const dim3 ogrid((unsigned)c.P.tiles, ol ? c.listed_y : (unsigned)c.n);
    select_vec4(c.P.vec4, [&](auto V4) {
        if (c.codes)
            select_codes(c.out, [&](auto CM) {
                hipLaunchKernelGGL((rez_output_codes_kernel<V4(), CM()>), ogrid, dim3(256), 0, c.st, c.x, c.out, c.d, c.l1buf,
                                   c.fm, c.state, c.tcnt, c.P.tiles, c.bits, part, ol, c.codes, c.kmt);
            });
        else
            hipLaunchKernelGGL(rez_output_kernel<V4()>, ogrid, dim3(256), 0, c.st, c.x, c.out, c.d, c.l1buf, c.fm, c.state, c.tcnt,
                               c.P.tiles, c.bits, part, ol);
    });
    return launched("rez_output_kernel launch");
}

// after KB7: its listed clients only (a list-strided grid, not n x tiles workgroups that
// mostly exit): full rows for index-order ranks and full clients, KB6t's patch of the
// listed threshold bin for the replayed fine clients
int launch_output_listed(const BiasedCall& c) {
    const int rc = launch_output(c, 2, c.list);
    if (rc) return rc;
    if (c.codes)
        select_codes(c.out, [&](auto CM) {
            hipLaunchKernelGGL(rez_tie_patch_codes_kernel<CM()>, dim3(kPatchBlocks, c.listed_y), dim3(256), 0, c.st, c.x, c.out,
                               c.d, c.l1buf, c.fm, c.state, c.fcand, c.cand_n, c.P.capf, c.bits, c.list, c.codes, c.kmt, c.P.tiles);
        });
    else
        hipLaunchKernelGGL(rez_tie_patch_kernel, dim3(kPatchBlocks, c.listed_y), dim3(256), 0, c.st, c.x, c.out, c.d, c.l1buf,
                           c.fm, c.state, c.fcand, c.cand_n, c.P.capf, c.bits, c.list);
    return launched("rez_tie_patch_kernel launch");
}

// ---- the three tie tails ---------------------------------------------------------------
// The lowest-index rule: the ambiguous clients' list (rez_tie_list_kernel), their index-order
// tie ranks, then KB6 over the full / no-selection clients and over the ambiguous fine ones.
int tail_lowest(const BiasedCall& c) {
    int rc = launch_fine_patch(c);
    if (rc || (rc = torch_ties_prepare(c))) return rc;
    select_vec4(c.P.vec4, [&](auto V4) {
        hipLaunchKernelGGL(rez_tiecount_kernel<V4()>, dim3((unsigned)c.P.tiles, c.listed_y), dim3(256), 0, c.st, c.x, c.d,
                           c.l1buf, c.fm, c.state, c.tcnt, c.P.tiles, c.list);
    });
    if ((rc = launched("rez_tiecount_kernel launch"))) return rc;
    if ((rc = launch_output(c, 0, c.flist))) return rc;
    return launch_output(c, 3, c.list);
}

// UQ_TIES_HOST_CHECK (synchronous few-client callers): one stream; after the tie list is built,
// wait for it and skip the replay chain -- KB7a's ~65 level launches -- when no client is
// listed; then every client's output in one launch (no tie counts: every ambiguous client is
// listed and replayed; a failed replay counts its own tiles).  *ran: the chain ran.
int tail_checked(const BiasedCall& c, int32_t* ran) {
    int rc = launch_fine_patch(c);
    if (rc || (rc = torch_ties_prepare(c))) return rc;
    SideStream* sb = nullptr;
    if ((rc = side_stream(&sb))) return rc;               // (its pinned word)
    rc = hip_check(hipMemcpyAsync(sb->count, c.list, sizeof(uint32_t), hipMemcpyDeviceToHost, c.st), "copy tie list length");
    if (rc || (rc = hip_check(hipStreamSynchronize(c.st), "sync"))) return rc;
    *ran = *sb->count != 0u;
    if (*ran) {
        const TieLevelState* tls = nullptr;
        if ((rc = launch_torch_ties(c, c.st, &tls, [] { return (int)UQ_OK; }))) return rc;
        if (tls && (rc = launch_replay(c, c.st, tls, 2))) return rc;
        if ((rc = launch_output_listed(c))) return rc;
    }
    return launch_output(c, 1, nullptr);
}

// The fork: KB7 (few workgroups, latency-bound) on the side stream while KB6 writes the clients
// without a threshold tie on the caller's stream; join, then the rest.
int tail_fork(const BiasedCall& c) {
    // the tie list (and, without KB7a, cleared tie bits) before the fork: both streams read it
    int rc = torch_ties_prepare(c);
    if (rc) return rc;
    SideFork fk(c.st, &rc);
    if (rc) return rc;
    // KB6 for the clients without a tie waits for KB7a's first (bandwidth-heavy) levels
    // and then runs beside the later, latency-bound ones (the chain is the critical path).
    // No tie counts: every ambiguous client is listed and replayed (a failed replay counts
    // its own tiles; the launch was 66 us of early-exit workgroups beside the chain)
    const TieLevelState* tls = nullptr;
    rc = launch_torch_ties(c, fk.side(), &tls, [&] {
        int mrc = fk.wait_mid();
        if (!mrc) mrc = launch_output(c, 1, nullptr);
        return mrc ? mrc : launch_fine_patch(c);
    });
    if (rc || (rc = fk.join())) return rc;
    // replays KB7a did not take (full 1024-thread replays)
    if (tls && (rc = launch_replay(c, c.st, tls, 2))) return rc;
    return launch_output_listed(c);
}

int biased_impl(const float* x, float* out, int8_t* codes, int32_t* kmax, int64_t n, int64_t d, int64_t m, int32_t T,
                int32_t tie_policy, float* l1_out, int32_t* info, void* ws, size_t ws_bytes, void* stream);

}  // namespace

extern "C" {

int uq_test_force_replay_failure(int on) { return g_force_replay_failure.exchange(on ? 1 : 0); }

int uq_test_biased_plan(int64_t n, int64_t d, int32_t tie_policy, int32_t x_aligned, int32_t out_aligned,
                        int64_t* plan_out, int32_t cap) {
    const int rc = biased_check(n, d, 0, 1, tie_policy);
    return rc ? rc : export_plan(biased_plan(n, d, tie_policy, x_aligned != 0, out_aligned != 0), plan_out, cap);
}

int uq_test_last_biased_plan(int64_t* plan_out, int32_t cap) { return export_plan(t_last_plan, plan_out, cap); }

int uq_biased_workspace_bytes(int64_t n, int64_t d, int32_t T, size_t* bytes_out) {
    if (!bytes_out) return fail(UQ_E_INVALID, "null bytes_out");
    L1Plan plan;
    if (n < 0 || d < 0 || T < 1) return fail(UQ_E_INVALID, "bad n/d/torch_threads");
    if (!make_plan(d, T, &plan)) return fail(UQ_E_INVALID, "cannot build L1 plan");
    *bytes_out = biased_layout(n, d, plan, biased_plan(n, d, UQ_TIES_TORCH, false, false)).total;   // (sizes: any policy)
    return UQ_OK;
}

int uq_biased_codes_workspace_bytes(int64_t n, int64_t d, int32_t T, size_t* bytes_out) {
    if (!bytes_out) return fail(UQ_E_INVALID, "null bytes_out");
    L1Plan plan;
    if (n < 0 || d < 0 || T < 1) return fail(UQ_E_INVALID, "bad n/d/torch_threads");
    if (!make_plan(d, T, &plan)) return fail(UQ_E_INVALID, "cannot build L1 plan");
    *bytes_out = biased_layout(n, d, plan, biased_plan(n, d, UQ_TIES_TORCH, false, false), true).total;
    return UQ_OK;
}

int uq_type_biased_f32(const float* x, float* out, int64_t n, int64_t d, int64_t m, int32_t T,
                       int32_t tie_policy, float* l1_out, int32_t* info, void* ws, size_t ws_bytes,
                       void* stream) {
    return biased_impl(x, out, nullptr, nullptr, n, d, m, T, tie_policy, l1_out, info, ws, ws_bytes, stream);
}

int uq_type_biased_codes_f32(const float* x, float* out, int8_t* codes, int32_t* kmax, int64_t n, int64_t d, int64_t m,
                             int32_t T, int32_t tie_policy, float* l1_out, int32_t* info, void* ws, size_t ws_bytes,
                             void* stream) {
    t_last_plan = BiasedPlan{};
    const int rc = biased_check(n, d, m, T, tie_policy);
    if (rc) return rc;
    if (m < 1) return fail(UQ_E_INVALID, "m must be >= 1 for type codes");
    if (n == 0 || d == 0) return UQ_OK;
    if (!codes || !kmax) return fail(UQ_E_INVALID, "null codes or kmax");
    if (!l1_out) return fail(UQ_E_INVALID, "null l1_out (the codes are decoded with it)");
    return biased_impl(x, out, codes, kmax, n, d, m, T, tie_policy, l1_out, info, ws, ws_bytes, stream);
}

}  // extern "C"

namespace {

// uq_type_biased_f32 (codes null), and uq_type_biased_codes_f32 after its own checks (codes and
// kmax given, out may be null).
int biased_impl(const float* x, float* out, int8_t* codes, int32_t* kmax, int64_t n, int64_t d, int64_t m, int32_t T,
                int32_t tie_policy, float* l1_out, int32_t* info, void* ws, size_t ws_bytes, void* stream) {
    t_last_plan = BiasedPlan{};
    int rc = biased_check(n, d, m, T, tie_policy);
    if (rc) return rc;
    L1Plan plan;
    if (!make_plan(d, T, &plan)) return fail(UQ_E_INVALID, "cannot build L1 plan for this d/torch_threads");
    const BiasedPlan P = biased_plan(n, d, tie_policy, aligned16(x), !out || aligned16(out),
                                     ((uintptr_t)codes & 3u) == 0);
    const BiasedLayout w = biased_layout(n, d, plan, P, codes != nullptr);
    if (n == 0) return UQ_OK;
    hipStream_t st = (hipStream_t)stream;
    if (d == 0) {
        if (l1_out) rc = hip_check(hipMemsetAsync(l1_out, 0, n * sizeof(float), st), "memset l1");
        if (!rc && info) rc = hip_check(hipMemsetAsync(info, 0, n * 2 * sizeof(int32_t), st), "memset info");
        return rc;
    }
    if (!x || (!out && !codes)) return fail(UQ_E_INVALID, "null x or out");
    if (!ws) return fail(UQ_E_INVALID, "null workspace");
    if (ws_bytes < w.total) return fail(UQ_E_WORKSPACE, "workspace too small");
    t_last_plan = P;
    const BiasedCall c{x, out, n, d, (float)m, P, w, (char*)ws, st, codes, kmax};
    auto clear_kmax = [&]() {                 // the per-tile maxima: the writers raise them with atomicMax
        return codes ? hip_check(hipMemsetAsync(c.kmt, 0, (size_t)n * P.tiles * sizeof(int32_t), st), "memset tile kmax")
                     : (int)UQ_OK;
    };
    if ((rc = clear_kmax())) return rc;
    auto finish = [&]() {                     // kmax's flagged rows, l1_out and the info pairs
        int frc = UQ_OK;
        if (codes) {
            hipLaunchKernelGGL(rez_kmax_finish_kernel, dim3((unsigned)n), dim3(256), 0, st, kmax, c.kmt, P.tiles, c.l1buf,
                               c.state);
            if ((frc = launched("rez_kmax_finish_kernel launch"))) return frc;
        }
        if (l1_out) frc = hip_check(hipMemcpyAsync(l1_out, c.l1buf, n * sizeof(float), hipMemcpyDeviceToDevice, st), "copy l1");
        if (!frc && info)
            frc = hip_check(hipMemcpy2DAsync(info, 2 * sizeof(int32_t), c.state, sizeof(RezState), 2 * sizeof(int32_t), n,
                                             hipMemcpyDeviceToDevice, st), "copy info");
        return frc;
    };
    if (P.front != UQ_BIASED_FRONT_FULL) {
        if ((rc = launch_small(c))) return rc;
        if (P.front == UQ_BIASED_FRONT_SMALL_CHECKED && (rc = small_has_tie(c, &t_last_plan.ran))) return rc;
        if (t_last_plan.ran <= 0) return finish();       // the lowest-index rule, or no ambiguous row
        if ((rc = clear_kmax())) return rc;              // the multi-kernel path writes every row again
    }
    if ((rc = launch_select(c, T, plan))) return rc;
    if (P.ties == UQ_BIASED_TIES_LOWEST) rc = tail_lowest(c);
    else if (P.ties == UQ_BIASED_TIES_CHECKED) rc = tail_checked(c, &t_last_plan.ran);
    else rc = tail_fork(c);
    return rc ? rc : finish();
}

}  // namespace
