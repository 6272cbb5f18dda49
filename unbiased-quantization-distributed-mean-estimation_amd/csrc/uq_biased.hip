// uq_biased.hip — the biased type quantizer (Reznik rounding): workspace layout, the torch
// tie replay's host code (KB7 / KB7a with its captured level graphs) and the C API
// uq_type_biased_f32 over uq_biased_kernels.h and uq_biased_torch_ties.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdlib>
#include <functional>

#include "uq_biased_torch_ties.h"
#include "uq_internal.h"

namespace {

// test hook (uq_test_force_replay_failure): every torch-tie replay takes its failure path
std::atomic<int> g_force_replay_failure{0};

// KB2 (the k' sum with the fine-bin histogram): at most this many level-1 groups per
// workgroup, fewer while that would leave fewer than ~4096 workgroups (a few-client call keeps
// one group each).  1024 x 2^20: KB2 1.16 -> 0.97 ms at 4 (torch-tie batch 5.43 -> 5.21 ms,
// lowest-index 4.23 -> 3.97 ms on one box; 8: 5.21 / 3.96), profiles/r5n_biased_gpw.jsonl.
// Env UQDME_HIST_GPW overrides the cap (measurements).
static const int kHistGroupsPerWG = [] {
    const char* e = std::getenv("UQDME_HIST_GPW");
    const int v = e ? std::atoi(e) : 8;
    return v >= 1 && v <= 64 ? v : 8;
}();

}  // namespace

int uq_internal::hist_groups_per_wg() { return kHistGroupsPerWG; }

namespace {

// Biased-quantizer workspace: [ctrl 256][K1 parts][l1 n][m' n][state n x 32B]
// [hist n x 3 x 2048 u32][zero/NaN counts n x 2][candidate counts n][candidates n x cap u32]
// [tie counts n x tiles u32][tie bits n x ceil(d/32) u32]
// [KB7 slots: keys + indices S x 2d u32][KB7 positions S x 2d u32], S = min(n, kTieSlots)
struct BiasedLayout {
    size_t part_off, l1_off, msum_off, st_off, hist_off, zn_off, cn_off, fl_off, cand_off, tcnt_off, bits_off,
        pairs_off, pos_off, list_off, tls_off, tcnt2_off, alist_off, total;
    int32_t tiles;
    int32_t slots;
    uint32_t cap;      // candidate region per client in u32 (KB6f lists cap / 2 (index, key) pairs)
    uint32_t capf;     // listed pairs per client at most: a larger fine bucket takes the full-row passes
};

BiasedLayout biased_layout(int64_t n, int64_t d, const L1Plan& plan) {
    BiasedLayout w{};
    w.tiles = (int32_t)((d + kSelTile - 1) / kSelTile);
    w.part_off = kCtrlBytes;
    w.l1_off = up256(w.part_off + (size_t)n * plan.total_groups * 32 * sizeof(float));
    w.msum_off = up256(w.l1_off + (size_t)n * sizeof(float));
    w.st_off = up256(w.msum_off + (size_t)n * sizeof(float));
    w.hist_off = up256(w.st_off + (size_t)n * sizeof(RezState));
    w.cap = (uint32_t)std::min<int64_t>(std::max<int64_t>(d, 1), std::max<int64_t>(4096, d / 8));
    w.capf = w.cap / 2;
    w.zn_off = up256(w.hist_off + (size_t)n * kHistSlots * kRadixBins * sizeof(uint32_t));
    w.cn_off = w.zn_off + (size_t)n * 2 * sizeof(uint32_t);           // zn and cand_n adjacent
    w.fl_off = w.cn_off + (size_t)n * sizeof(uint32_t);               // the full clients' list (zeroed count)
    w.cand_off = up256(w.fl_off + (size_t)(n + 1) * sizeof(uint32_t));
    w.tcnt_off = up256(w.cand_off + (size_t)n * w.cap * sizeof(uint32_t));
    w.bits_off = up256(w.tcnt_off + (size_t)n * w.tiles * sizeof(uint32_t));
    w.slots = (int32_t)std::min<int64_t>(n, kTieSlots);
    w.pairs_off = up256(w.bits_off + (size_t)n * ((d + 31) / 32) * sizeof(uint32_t));
    w.pos_off = up256(w.pairs_off + (size_t)w.slots * 2 * ((d + 3) & ~(int64_t)3) * sizeof(uint32_t) + 16);
    w.list_off = up256(w.pos_off + (size_t)w.slots * 2 * d * sizeof(uint32_t));
    w.tls_off = up256(w.list_off + (size_t)(n + 1) * sizeof(uint32_t));    // KB7's client list
    w.tcnt2_off = up256(w.tls_off + (size_t)w.slots * sizeof(TieLevelState));
    w.alist_off = up256(w.tcnt2_off + (size_t)w.slots * kTieSegs * 2 * sizeof(uint32_t));
    w.total = up256(w.alist_off + (size_t)(kTieSlots + 1) * sizeof(uint32_t));    // KB7a's active slots
    return w;
}

// biased quantizer: batches of at most this many clients run the candidate digits (KB4d) over
// many workgroups per client (one workgroup per client walks up to d/8 keys twice)
constexpr int64_t kCandMultiMaxN = 16;

// KB7 on stream `st`.  Without KB7a (d <= kTieLevelMin) one launch replays every listed
// client.  With KB7a, the replay's LDS tails run here in small workgroups (part 1) and
// *tls_out is set: the caller then runs launch_torch_ties_rest (part 2: heap-path clients
// and list entries beyond the slots) once the output kernel on its own stream is done.
// KB7's client list and cleared tie bits (before launch_torch_ties and the tie counts).
// KB7 replays through KB7a's multi-workgroup levels (else one rez_ties_kernel launch)
inline bool kb7a_path(int64_t n, int64_t d) {
    return !(d <= kTieLevelMin || (n < kTieLevelMinClients && d < kTieLevelBigD));
}

// clear_bits: without KB7a (whose level-0 kt_count clears the listed clients' rows) every row here.
int torch_ties_prepare(int64_t n, int64_t d, RezState* state, uint32_t* bits, char* wsb, const BiasedLayout& w,
                       hipStream_t st, bool clear_bits) {
    if (clear_bits) {
        const int rc = hip_check(hipMemsetAsync(bits, 0, (size_t)n * ((d + 31) / 32) * sizeof(uint32_t), st),
                                 "memset tie bits");
        if (rc) return rc;
    }
    hipLaunchKernelGGL(rez_tie_list_kernel, dim3(1), dim3(1024), 0, st, state, n, (uint32_t*)(wsb + w.list_off));
    return hip_check(hipGetLastError(), "rez_tie_list_kernel launch");
}

// Captured KB7a level chains, per thread (streams and workspaces are per thread in practice):
// keyed by (device, every pointer the chain's kernels take, d, slots, levels).  *exec =
// nullptr when capture is unavailable (then the caller launches the chain directly).
struct LevelPtrs {
    const void *qbuf, *list, *tls, *cnt, *pos, *alist;
    bool operator==(const LevelPtrs& o) const {
        return qbuf == o.qbuf && list == o.list && tls == o.tls && cnt == o.cnt && pos == o.pos && alist == o.alist;
    }
};
template <class F>
int level_graph(const LevelPtrs& wsb, int64_t d, unsigned S, int levels, hipStream_t st, F&& launch,
                hipGraphExec_t* exec) {
    struct Entry {
        int dev;
        LevelPtrs wsb;
        int64_t d;
        unsigned S;
        int levels;                     // lv0 * 256 + lv1: the captured range of levels
        hipGraphExec_t exec;
    };
    static thread_local Entry cache[8] = {};
    static thread_local int next = 0;
    int dev = 0;
    int rc = hip_check(hipGetDevice(&dev), "hipGetDevice");
    if (rc) return rc;
    for (const Entry& e : cache)
        if (e.exec && e.dev == dev && e.wsb == wsb && e.d == d && e.S == S && e.levels == levels) {
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
    slot = Entry{dev, wsb, d, S, levels, ex};
    *exec = ex;
    return UQ_OK;
}

// mid (may be empty): called once KB7a's first kTieHeavyLevels levels are enqueued on `st`
// (with KB7a; before anything else otherwise) -- the fork records an event there and lets KB6
// part 1 wait for it, so the bandwidth-heavy first levels (the listed clients' full rows)
// do not share HBM with KB6 and KB6 runs beside the later, latency-bound levels instead.
int launch_torch_ties(const float* x, int64_t n, int64_t d, const float* l1, float fm, RezState* state,
                      uint32_t* bits, char* wsb, const BiasedLayout& w, hipStream_t st, const TieLevelState** tls_out,
                      const std::function<int()>& mid) {
    *tls_out = nullptr;
    int rc = UQ_OK;
    uint32_t* list = (uint32_t*)(wsb + w.list_off);
    uint32_t* qbuf = (uint32_t*)(wsb + w.pairs_off);
    uint32_t* pos = (uint32_t*)(wsb + w.pos_off);
    // KB7a pays ~85 short launches whether or not any client is listed (the host does not
    // know): worth it for batches, where ~3 % of Gaussian clients are ambiguous at R = 1 and
    // several replays would share one workgroup each, and for vectors of 2^21 and more, whose
    // one-workgroup replay takes milliseconds; a few-client call at smaller d (the per-vector
    // drop-ins) replays in one kernel when it has to
    if (!kb7a_path(n, d)) {
        if (mid && (rc = mid())) return rc;
        hipLaunchKernelGGL(rez_ties_kernel<kTieThreads>, dim3((unsigned)w.slots), dim3(kTieThreads), 0, st, x, d, l1, fm,
                           state, bits, qbuf, pos, list, (uint32_t*)wsb, (const TieLevelState*)nullptr, 0,
                           (uint32_t*)(wsb + w.tcnt_off), w.tiles, g_force_replay_failure.load());
        return hip_check(hipGetLastError(), "rez_ties_kernel launch");
    }
    // KB7a: introselect's levels over (segments x slots) workgroups, level by level, down to
    // ranges that fit the LDS tail
    TieLevelState* tls = (TieLevelState*)(wsb + w.tls_off);
    uint32_t* cnt = (uint32_t*)(wsb + w.tcnt2_off);
    const unsigned S = (unsigned)w.slots;
    // a level keeps the side of the cut that holds nth, half the range on average; an idle
    // level costs four ~6 us launches, and a range still longer continues in part 1's
    // workgroup (UQDME_TIE_STOP / UQDME_TIE_MARGIN: experiments only)
    static const int64_t tie_stop = [] {
        const char* e = std::getenv("UQDME_TIE_STOP");
        const long long v = e ? std::atoll(e) : 0;
        return v >= kTieLevelMin ? (int64_t)v : kTieLevelStop;
    }();
    static const int tie_margin = [] {
        const char* e = std::getenv("UQDME_TIE_MARGIN");
        const int v = e ? std::atoi(e) : -1;
        return v >= 0 && v <= 8 ? v : kTieLevelMargin;
    }();
    int levels = tie_margin;
    for (int64_t r = d; r > tie_stop; r = (r + 1) / 2) ++levels;
    levels = std::max(levels, 1);
    uint32_t* alist = (uint32_t*)(wsb + w.alist_off);
    // the per-level launches take (active slot, segment) items, one per wave: S slots need at
    // most S * kTieSegs / 4 workgroups (a one-client call launched 2048, 1984 of them idle)
    const unsigned lgrid = (unsigned)std::min<int64_t>(kTieGrid, (int64_t)S * kTieSegs / 4);
    // level 0's pivot and counts with the queue fill from x (x, l1 and the states are
    // per-call arguments: launched directly, not captured)
    hipLaunchKernelGGL(kt_count_kernel, dim3(lgrid), dim3(256), 0, st, x, d, l1, fm, (const RezState*)state, qbuf, list,
                       tls, cnt, alist, bits, (int)S, tie_stop, 1);
    if ((rc = hip_check(hipGetLastError(), "kt_count_kernel launch"))) return rc;
    static const int heavy = [] {
        const char* e = std::getenv("UQDME_TIE_HEAVY");
        const int v = e ? std::atoi(e) : -1;
        return v >= 0 && v <= 16 ? v : kTieHeavyLevels;
    }();
    const int lsplit = std::min(heavy, levels);
    int lv0 = 0, lv1 = levels;                  // the range levels_on enqueues
    auto levels_on = [&](hipStream_t ls) {
        for (int lv = lv0; lv < lv1; ++lv) {
            if (lv > 0)
                hipLaunchKernelGGL(kt_count_kernel, dim3(lgrid), dim3(256), 0, ls, (const float*)nullptr, d,
                                   (const float*)nullptr, fm, (const RezState*)nullptr, qbuf, list, tls, cnt, alist,
                                   (uint32_t*)nullptr, (int)S, tie_stop, 0);
            hipLaunchKernelGGL(kt_list_kernel, dim3(lgrid), dim3(256), 0, ls, d, qbuf, pos, tls, cnt, alist);
            hipLaunchKernelGGL(kt_jcut_kernel, dim3(S), dim3(kJcutThreads), 0, ls, d, qbuf, pos, tls, cnt, alist);
            hipLaunchKernelGGL(kt_swap_kernel, dim3(lgrid), dim3(256), 0, ls, d, qbuf, pos, tls, alist);
        }
        return hip_check(hipGetLastError(), "KB7a level launch");
    };
    // The rest of the level chain (4 dependent launches per level, whether or not a client is
    // listed) is replayed as a captured HIP graph: its arguments are workspace pointers, d, S
    // and the stop only, so one capture serves every call on the same workspace (per-call
    // host cost was ~65 launches, more than the chain's GPU time for a few-client call).
    auto run_levels = [&](int a, int b) {
        if (a >= b) return (int)UQ_OK;
        lv0 = a;
        lv1 = b;
        hipGraphExec_t exec = nullptr;
        int grc = level_graph(LevelPtrs{qbuf, list, tls, cnt, pos, alist}, d, S, a * 256 + b, st, levels_on, &exec);
        if (grc) return grc;
        if (exec) return hip_check(hipGraphLaunch(exec, st), "KB7a level graph launch");
        return levels_on(st);
    };
    if ((rc = run_levels(0, lsplit))) return rc;
    if (mid && (rc = mid())) return rc;
    if ((rc = run_levels(lsplit, levels))) return rc;
    hipLaunchKernelGGL(kt_mark_kernel, dim3(kTieMarkSegs, S), dim3(256), 0, st, d, qbuf, list, state, tls, bits);
    if ((rc = hip_check(hipGetLastError(), "kt_mark_kernel launch"))) return rc;
    hipLaunchKernelGGL(rez_ties_kernel<kTieThreads>, dim3(S), dim3(kTieThreads), 0, st, x, d, l1, fm, state, bits,
                       qbuf, pos, list, (uint32_t*)wsb, (const TieLevelState*)tls, 1, (uint32_t*)(wsb + w.tcnt_off),
                       w.tiles, g_force_replay_failure.load());
    *tls_out = tls;
    return hip_check(hipGetLastError(), "rez_ties_kernel launch");
}

int launch_torch_ties_rest(const float* x, int64_t d, const float* l1, float fm, RezState* state, uint32_t* bits,
                           char* wsb, const BiasedLayout& w, const TieLevelState* tls, hipStream_t st) {
    hipLaunchKernelGGL(rez_ties_kernel<kTieThreads>, dim3((unsigned)w.slots), dim3(kTieThreads), 0, st, x, d, l1, fm,
                       state, bits, (uint32_t*)(wsb + w.pairs_off), (uint32_t*)(wsb + w.pos_off),
                       (const uint32_t*)(wsb + w.list_off), (uint32_t*)wsb, tls, 2, (uint32_t*)(wsb + w.tcnt_off),
                       w.tiles, g_force_replay_failure.load());
    return hip_check(hipGetLastError(), "rez_ties_kernel launch");
}

}  // namespace

extern "C" {

int uq_test_force_replay_failure(int on) { return g_force_replay_failure.exchange(on ? 1 : 0); }

int uq_biased_workspace_bytes(int64_t n, int64_t d, int32_t T, size_t* bytes_out) {
    if (!bytes_out) return fail(UQ_E_INVALID, "null bytes_out");
    L1Plan plan;
    if (n < 0 || d < 0 || T < 1) return fail(UQ_E_INVALID, "bad n/d/torch_threads");
    if (!make_plan(d, T, &plan)) return fail(UQ_E_INVALID, "cannot build L1 plan");
    *bytes_out = biased_layout(n, d, plan).total;
    return UQ_OK;
}

int uq_type_biased_f32(const float* x, float* out, int64_t n, int64_t d, int64_t m, int32_t T,
                       int32_t tie_policy, float* l1_out, int32_t* info, void* ws, size_t ws_bytes,
                       void* stream) {
    if (n < 0 || d < 0) return fail(UQ_E_INVALID, "n and d must be >= 0");
    if (m < 0) return fail(UQ_E_INVALID, "m must be >= 0");
    if (d >= ((int64_t)1 << 31)) return fail(UQ_E_INVALID, "d must be < 2^31");
    if (n > 65535) return fail(UQ_E_INVALID, "at most 65535 clients per call");
    if (T < 1) return fail(UQ_E_INVALID, "torch_threads must be >= 1");
    const bool host_check = (tie_policy & UQ_TIES_HOST_CHECK) != 0;
    tie_policy &= ~UQ_TIES_HOST_CHECK;
    if (tie_policy != UQ_TIES_LOWEST_INDEX && tie_policy != UQ_TIES_TORCH)
        return fail(UQ_E_INVALID, "unknown tie_policy");
    L1Plan plan;
    if (!make_plan(d, T, &plan)) return fail(UQ_E_INVALID, "cannot build L1 plan for this d/torch_threads");
    const BiasedLayout w = biased_layout(n, d, plan);
    if (n == 0) return UQ_OK;
    hipStream_t st = (hipStream_t)stream;
    if (d == 0) {
        int rc = UQ_OK;
        if (l1_out) rc = hip_check(hipMemsetAsync(l1_out, 0, n * sizeof(float), st), "memset l1");
        if (!rc && info) rc = hip_check(hipMemsetAsync(info, 0, n * 2 * sizeof(int32_t), st), "memset info");
        return rc;
    }
    if (!x || !out) return fail(UQ_E_INVALID, "null x or out");
    if (!ws) return fail(UQ_E_INVALID, "null workspace");
    if (ws_bytes < w.total) return fail(UQ_E_WORKSPACE, "workspace too small");
    char* wsb = (char*)ws;
    float* part = (float*)(wsb + w.part_off);
    float* l1buf = (float*)(wsb + w.l1_off);
    float* msum = (float*)(wsb + w.msum_off);
    RezState* state = (RezState*)(wsb + w.st_off);
    auto finish = [&]() {                     // l1_out and the info pairs
        int frc = UQ_OK;
        if (l1_out) frc = hip_check(hipMemcpyAsync(l1_out, l1buf, n * sizeof(float), hipMemcpyDeviceToDevice, st), "copy l1");
        if (!frc && info)
            frc = hip_check(hipMemcpy2DAsync(info, 2 * sizeof(int32_t), state, sizeof(RezState), 2 * sizeof(int32_t), n,
                                             hipMemcpyDeviceToDevice, st), "copy info");
        return frc;
    };
    // vectors shorter than GRAIN: one launch (KB-small) with the lowest-index rule; with torch
    // ties only under UQ_TIES_HOST_CHECK, which reads the clients' flags back and runs the
    // multi-kernel path below when a threshold tie needs torch's choice
    if (d <= kSmallBiasedMax &&
        (tie_policy == UQ_TIES_LOWEST_INDEX || (host_check && n <= kSmallCheckMaxN))) {
        static std::atomic<uint64_t> attr_set{0};             // per device (bit = device index < 64)
        int dev = 0;
        if (hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < 64 && !((attr_set.load() >> dev) & 1u)) {
            (void)hipFuncSetAttribute((const void*)biased_small_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)(kSmallBiasedMax * sizeof(uint32_t)));
            attr_set.fetch_or(1ull << dev);
        }
        hipLaunchKernelGGL(biased_small_kernel, dim3((unsigned)n), dim3(256), (size_t)d * sizeof(uint32_t), st, x, out, d,
                           (float)m, (const float*)nullptr, l1buf, state);
        int rc = hip_check(hipGetLastError(), "biased_small_kernel launch");
        if (rc) return rc;
        if (tie_policy == UQ_TIES_LOWEST_INDEX) return finish();
        SideStream* sb = nullptr;
        if ((rc = side_stream(&sb))) return rc;
        rc = hip_check(hipMemcpyAsync(sb->states, state, (size_t)n * sizeof(RezState), hipMemcpyDeviceToHost, st),
                       "copy states");
        if (rc) return rc;
        if ((rc = hip_check(hipStreamSynchronize(st), "sync"))) return rc;
        bool tie = false;
        for (int64_t i = 0; i < n; ++i) tie |= (((const RezState*)sb->states)[i].flags & kRezAmbiguous) != 0;
        if (!tie) return finish();
    }
    uint32_t* hist = (uint32_t*)(wsb + w.hist_off);
    uint32_t* tcnt = (uint32_t*)(wsb + w.tcnt_off);
    uint32_t* bits = (uint32_t*)(wsb + w.bits_off);
    const float fm = (float)m;
    int rc = launch_l1(x, n, d, T, part, l1buf, st);                                      // AS:680
    if (rc) return rc;
    uint32_t* zn = (uint32_t*)(wsb + w.zn_off);
    uint32_t* cand_n = (uint32_t*)(wsb + w.cn_off);
    uint32_t* cand = (uint32_t*)(wsb + w.cand_off);
    rc = hip_check(hipMemsetAsync(hist, 0, w.cand_off - w.hist_off, st), "memset hist/zn/cand_n");
    if (rc) return rc;
    // AS:648-649 m' = sum k' in torch order, with the first radix digit's histogram (KB2 + KB4 pass 0)
    rc = launch_cascade<RezKHistOp>(x, n, d, plan, part, msum, l1buf, fm, st, hist, zn);
    if (rc) return rc;
    hipLaunchKernelGGL(rez_setup_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, msum, fm, d, n, state);
    rc = hip_check(hipGetLastError(), "rez_setup_kernel launch");
    if (rc) return rc;
    const bool vec4 = aligned16(x) && aligned16(out) && d % 4 == 0;
    const dim3 fgrid((unsigned)((d + kSelTile - 1) / kSelTile), (unsigned)n);
    uint2* fcand = (uint2*)cand;
    // KB4a: the threshold's fine bin; a small bucket makes the client "fine", a large one "full"
    // full clients are listed by KB4a (flist[0] = count, in the zeroed range): the key-digit
    // passes below stride over the list, not over n x spans workgroups that mostly exit
    uint32_t* flist = (uint32_t*)(wsb + w.fl_off);
    hipLaunchKernelGGL((rez_select_kernel<0, true>), dim3((unsigned)n), dim3(256), 0, st, state, hist, zn, w.capf, flist);
    const unsigned fy = (unsigned)std::min<int64_t>(n, kListedGridY);
    const dim3 hlgrid((unsigned)((d + kHistSpan - 1) / kHistSpan), fy);
    // full clients (tie-heavy rows): the key digits by three full-row histogram passes
#define UQ_RADIX(P)                                                                                          \
    if (vec4)                                                                                                \
        hipLaunchKernelGGL((rez_hist_kernel<P, true>), hlgrid, dim3(256), 0, st, x, d, l1buf, fm, state, hist, flist); \
    else                                                                                                     \
        hipLaunchKernelGGL((rez_hist_kernel<P, false>), hlgrid, dim3(256), 0, st, x, d, l1buf, fm, state, hist, flist); \
    hipLaunchKernelGGL((rez_select_kernel<P, false>), dim3((unsigned)std::min<int64_t>(n, kTieSlots)), dim3(256), 0, st, \
                       state, hist, zn, w.capf, flist);
    UQ_RADIX(0) UQ_RADIX(1) UQ_RADIX(2)
#undef UQ_RADIX
    // fine clients: KB6f writes every output and lists the bucket, KB4d finds the threshold
    // key among the listed keys, KB6p patches the selected listed coordinates (tie-free clients)
    if (vec4)
        hipLaunchKernelGGL(rez_output_fine_kernel<true>, fgrid, dim3(256), 0, st, x, out, d, l1buf, fm, state, fcand,
                           cand_n, w.capf);
    else
        hipLaunchKernelGGL(rez_output_fine_kernel<false>, fgrid, dim3(256), 0, st, x, out, d, l1buf, fm, state, fcand,
                           cand_n, w.capf);
    const unsigned cspans = (unsigned)((w.capf + kCandSpan - 1) / kCandSpan);
    if (n <= kCandMultiMaxN && cspans > 1) {         // few clients: the passes over many workgroups
#define UQ_CAND(P)                                                                                           \
        hipLaunchKernelGGL(rez_cand_hist_kernel<P>, dim3(cspans, (unsigned)n), dim3(256), 0, st, state, fcand, cand_n, \
                           w.capf, hist);                                                                    \
        hipLaunchKernelGGL(rez_cand_pick_kernel<P>, dim3((unsigned)n), dim3(256), 0, st, state, hist);
        UQ_CAND(0) UQ_CAND(1) UQ_CAND(2)
#undef UQ_CAND
    } else {
        hipLaunchKernelGGL(rez_cand_select_kernel, dim3((unsigned)n), dim3(256), 0, st, state, fcand, cand_n, w.capf);
    }
    rc = hip_check(hipGetLastError(), "radix select launch");
    if (rc) return rc;
    // KB6p: the tie-free fine clients' selected bin coordinates (independent of KB7: with the
    // torch-tie fork it runs on the caller's stream beside the replay chain, off its path)
    auto fine_patch = [&](hipStream_t ps) {
        hipLaunchKernelGGL(rez_fine_patch_kernel, dim3(kPatchBlocks, (unsigned)n), dim3(256), 0, ps, x, out, d, l1buf,
                           fm, state, fcand, cand_n, w.capf);
        return hip_check(hipGetLastError(), "rez_fine_patch_kernel launch");
    };
    const bool fork_ties = tie_policy == UQ_TIES_TORCH && !(host_check && kb7a_path(n, d));
    if (!fork_ties && (rc = fine_patch(st))) return rc;
    // KB6 for the clients of a list (list-strided grid): part 0 / 1 over KB4a's list (the full
    // clients and those without a selection -- every client KB6f did not write), part 3 over
    // the ambiguous ones (their fine clients)
    // ol == nullptr: the n x tiles grid (part 1 beside the torch-tie chain: the list-strided
    // form was 0.01-0.02 ms slower there, profiles/r5aw_*; the lowest-index batch gains 0.075 ms
    // from it, its launches being on the critical path)
    const dim3 lgrid((unsigned)w.tiles, (unsigned)std::min<int64_t>(n, kListedGridY));
    auto output = [&](hipStream_t os, int part, const uint32_t* ol) {
        const dim3 ogrid((unsigned)w.tiles, (unsigned)(ol ? std::min<int64_t>(n, kListedGridY) : n));
        if (vec4)
            hipLaunchKernelGGL(rez_output_kernel<true>, ogrid, dim3(256), 0, os, x, out, d, l1buf, fm, state, tcnt,
                               w.tiles, bits, part, ol);
        else
            hipLaunchKernelGGL(rez_output_kernel<false>, ogrid, dim3(256), 0, os, x, out, d, l1buf, fm, state, tcnt,
                               w.tiles, bits, part, ol);
        return hip_check(hipGetLastError(), "rez_output_kernel launch");
    };
    // after KB7: its listed clients only (a list-strided grid, not n x tiles workgroups that
    // mostly exit): full rows for index-order ranks and full clients, KB6t's patch of the
    // listed threshold bin for the replayed fine clients
    auto output_listed = [&](hipStream_t os) {
        const uint32_t* list = (const uint32_t*)(wsb + w.list_off);
        if (vec4)
            hipLaunchKernelGGL(rez_output_kernel<true>, lgrid, dim3(256), 0, os, x, out, d, l1buf, fm, state, tcnt,
                               w.tiles, bits, 2, list);
        else
            hipLaunchKernelGGL(rez_output_kernel<false>, lgrid, dim3(256), 0, os, x, out, d, l1buf, fm, state, tcnt,
                               w.tiles, bits, 2, list);
        int orc = hip_check(hipGetLastError(), "rez_output_kernel launch");
        if (orc) return orc;
        hipLaunchKernelGGL(rez_tie_patch_kernel, dim3(kPatchBlocks, (unsigned)std::min<int64_t>(n, kListedGridY)),
                           dim3(256), 0, os, x, out, d, l1buf, fm, state, fcand, cand_n, w.capf, bits, list);
        return hip_check(hipGetLastError(), "rez_tie_patch_kernel launch");
    };
    auto tiecount = [&](hipStream_t ts, const uint32_t* list) {
        // index-order tie ranks of the listed (ambiguous) clients
        if (vec4)
            hipLaunchKernelGGL(rez_tiecount_kernel<true>, lgrid, dim3(256), 0, ts, x, d, l1buf, fm, state, tcnt, w.tiles,
                               list);
        else
            hipLaunchKernelGGL(rez_tiecount_kernel<false>, lgrid, dim3(256), 0, ts, x, d, l1buf, fm, state, tcnt, w.tiles,
                               list);
        return hip_check(hipGetLastError(), "rez_tiecount_kernel launch");
    };
    // (the check pays only where the replay would be KB7a's level chain; a one-kernel replay
    // costs less than the synchronisation)
    const bool kb7a = kb7a_path(n, d);
    if (tie_policy == UQ_TIES_TORCH && host_check && kb7a) {
        // UQ_TIES_HOST_CHECK (synchronous few-client callers): one stream; after the tie list
        // is built, wait for it and skip the replay chain -- KB7a's ~65 level launches --
        // when no client is listed; then every client's output in one launch
        // (no tie counts: every ambiguous client is listed and replayed; a failed replay
        // counts its own tiles)
        rc = torch_ties_prepare(n, d, state, bits, wsb, w, st, false);
        if (rc) return rc;
        SideStream* sb = nullptr;
        rc = side_stream(&sb);                            // (its pinned word)
        if (rc) return rc;
        rc = hip_check(hipMemcpyAsync(sb->count, wsb + w.list_off, sizeof(uint32_t), hipMemcpyDeviceToHost, st),
                       "copy tie list length");
        if (rc) return rc;
        rc = hip_check(hipStreamSynchronize(st), "sync");
        if (rc) return rc;
        if (*sb->count != 0u) {
            const TieLevelState* tls = nullptr;
            rc = launch_torch_ties(x, n, d, l1buf, fm, state, bits, wsb, w, st, &tls, nullptr);
            if (rc) return rc;
            if (tls && (rc = launch_torch_ties_rest(x, d, l1buf, fm, state, bits, wsb, w, tls, st))) return rc;
            if ((rc = output_listed(st))) return rc;
        }
        rc = output(st, 1, nullptr);
        if (rc) return rc;
    } else if (tie_policy == UQ_TIES_TORCH) {
        // fork: KB7 (few workgroups, latency-bound) on the side stream while KB6 writes the
        // clients without a threshold tie on the caller's stream; join, then the rest
        SideStream* sb = nullptr;
        rc = side_stream(&sb);
        if (rc) return rc;
        // the tie list (and, without KB7a, cleared tie bits) before the fork: both streams read it
        rc = torch_ties_prepare(n, d, state, bits, wsb, w, st, !kb7a);
        if (rc) return rc;
        rc = hip_check(hipEventRecord(sb->fork, st), "record fork");
        if (rc) return rc;
        rc = hip_check(hipStreamWaitEvent(sb->s, sb->fork, 0), "wait fork");
        if (rc) return rc;
        // KB6 for the clients without a tie waits for KB7a's first (bandwidth-heavy) levels
        // and then runs beside the later, latency-bound ones (the chain is the critical path).
        // No tie counts: every ambiguous client is listed and replayed (a failed replay counts
        // its own tiles; the launch was 66 us of early-exit workgroups beside the chain)
        const TieLevelState* tls = nullptr;
        rc = launch_torch_ties(x, n, d, l1buf, fm, state, bits, wsb, w, sb->s, &tls, [&]() {
            int mrc = hip_check(hipEventRecord(sb->mid, sb->s), "record mid");
            if (!mrc) mrc = hip_check(hipStreamWaitEvent(st, sb->mid, 0), "wait mid");
            if (!mrc) mrc = output(st, 1, nullptr);
            if (!mrc) mrc = fine_patch(st);
            return mrc;
        });
        if (rc) return rc;
        rc = hip_check(hipEventRecord(sb->join, sb->s), "record join");
        if (rc) return rc;
        rc = hip_check(hipStreamWaitEvent(st, sb->join, 0), "wait join");
        if (rc) return rc;
        if (tls) {                       // replays KB7a did not take (full 1024-thread replays)
            rc = launch_torch_ties_rest(x, d, l1buf, fm, state, bits, wsb, w, tls, st);
            if (rc) return rc;
        }
        rc = output_listed(st);
        if (rc) return rc;
    } else {
        // the lowest-index rule: the ambiguous clients' list (rez_tie_list_kernel), their tie
        // counts, then KB6 over the full / no-selection clients and over the ambiguous fine ones
        rc = torch_ties_prepare(n, d, state, bits, wsb, w, st, false);
        if (rc) return rc;
        const uint32_t* amb = (const uint32_t*)(wsb + w.list_off);
        if ((rc = tiecount(st, amb))) return rc;
        if ((rc = output(st, 0, flist))) return rc;
        if ((rc = output(st, 3, amb))) return rc;
    }
    return finish();
}

}  // extern "C"
