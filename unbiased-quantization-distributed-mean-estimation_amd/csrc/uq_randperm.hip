// uq_randperm.hip — torch.randperm(D)[:k] of the CPU generator on the GPU (EDEN's receiver-side
// coordinate drop, AS:419-423): the plan, the workspace layout, the launchers of
// uq_randperm_kernels.h and the C API uq_randperm_prefix*.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <map>
#include <mutex>
#include <tuple>
#include <vector>

#include "uq_internal.h"
#include "uq_randperm_kernels.h"

extern "C" int uq_mtpoly_progression(int64_t b0, int64_t step, int32_t count, uint32_t* out);   // uq_mt_poly.cpp

namespace {

constexpr int64_t kRpMaxD = 0xFFFFFFFFll / 20;        // torch's randperm takes another algorithm from here on
constexpr int64_t kRpWalkBlocks = 16;                 // streams of up to this many blocks: one wave per client
constexpr int64_t kRpRunBlocks = 16;                  // jump form: blocks per run at least
constexpr int64_t kRpMaxRuns = 1024;                  // ... and runs per client at most
constexpr int64_t kRpRunWaves = 4096;                 // ... and about this many run waves per call
constexpr size_t kRpWorkspaceCap = (size_t)1 << 30;   // uq_randperm_prefix_workspace_bytes asks for no more (one client aside)
constexpr int64_t kRpMaxTestWords = 65536;            // uq_test_randperm_from_words: one list may hold every step

struct RpPlan {
    int32_t form = UQ_RANDPERM_FORM_NONE, R = 0;
    int64_t L = 0, G = 0, K = 0, groups = 0;
};
thread_local RpPlan t_last_plan;

// Stage 1 of a call: the stream of K words may start anywhere in its first block, so it touches
// blocks 0 .. B - 1 at most.  Few blocks: one wave walks them.  Else runs of L blocks from jumped
// states, L chosen so that a call has about kRpRunWaves run waves and a client at most kRpMaxRuns.
RpPlan rp_plan(int64_t n, int64_t D, int64_t k, bool from_words) {
    RpPlan p;
    if (n < 1 || k < 1) return p;
    p.K = std::min(k, D - 1);
    if (from_words) {
        p.form = UQ_RANDPERM_FORM_WORDS;
        return p;
    }
    const int64_t B = (kMtN + p.K - 1) / kMtN + 1;
    if (B <= kRpWalkBlocks) {
        p.form = UQ_RANDPERM_FORM_WALK;
        p.R = 1;
        p.L = B;
        return p;
    }
    p.form = UQ_RANDPERM_FORM_JUMP;
    const int64_t per = (n * B + kRpRunWaves - 1) / kRpRunWaves;
    p.L = std::max({kRpRunBlocks, (B + kRpMaxRuns - 1) / kRpMaxRuns, std::min(per, B)});
    p.R = (int32_t)((B + p.L - 1) / p.L);
    return p;
}

// The workspace of a group of G clients: the control block every workspace of the library starts
// with (untouched here), the round flags, then one array per region.
constexpr size_t kRpFlagsOff = 256;
struct RpLayout {
    size_t h, next, a, head, xs, parts, total;
};
RpLayout rp_layout(const RpPlan& p, int64_t G, int64_t D, int64_t k) {
    RpLayout l;
    size_t off = kRpFlagsOff + 256;
    auto take = [&](size_t bytes) {
        const size_t at = off;
        off += up256(bytes);
        return at;
    };
    const bool jump = p.form == UQ_RANDPERM_FORM_JUMP;
    l.h = take((size_t)G * p.K * 4);
    l.next = take((size_t)G * k * 4);
    l.a = take((size_t)G * k * 4);
    l.head = take((size_t)G * D * 4);
    l.xs = take(jump ? (size_t)G * kMjX * 4 : 0);
    l.parts = take(jump ? (size_t)G * p.R * kMjParts * kMtN * 4 : 0);
    l.total = off;
    return l;
}

// The largest group (at most n clients, one grid row each) whose workspace fits `bytes`; 0: not even one
int64_t rp_group(const RpPlan& p, int64_t n, int64_t D, int64_t k, size_t bytes) {
    int64_t lo = 0, hi = std::min<int64_t>(n, kMaxGridY);
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) / 2;
        if (rp_layout(p, mid, D, k).total <= bytes) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

int rp_check(int64_t n, int64_t D, int64_t k) {
    if (n < 0 || D < 0 || k < 0) return fail(UQ_E_INVALID, "randperm: n, D and k must be >= 0");
    if (k > D) return fail(UQ_E_INVALID, "randperm: k must be <= D");
    if (D >= kRpMaxD) return fail(UQ_E_INVALID, "randperm: D must be below 2^32 / 20 (torch.randperm changes algorithm there)");
    return UQ_OK;
}

// t^(624 (r L - 1)) mod phi for r = 1 .. R - 1 on the device (row 0 unused), cached per (device, L, R)
// for the life of the process, as QUIC-FL's jump form keeps its own: a pointer handed out may still
// be waiting in a stream, so nothing is freed.  R * 2496 bytes per entry.
int rp_polys(const RpPlan& p, const uint32_t** out) {
    static std::mutex mu;
    static std::map<std::tuple<int, int64_t, int32_t>, uint32_t*> cache;
    int dev = 0;
    int rc = hip_check(hipGetDevice(&dev), "hipGetDevice");
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(mu);
    const auto key = std::make_tuple(dev, p.L, p.R);
    auto it = cache.find(key);
    if (it != cache.end()) {
        *out = it->second;
        return UQ_OK;
    }
    std::vector<uint32_t> h((size_t)p.R * kMtN, 0u);
    if (p.R > 1 && uq_mtpoly_progression(p.L - 1, p.L, p.R - 1, h.data() + kMtN))
        return fail(UQ_E_INVALID, "MT19937 jump polynomials unavailable");
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

dim3 step_grid(int64_t k, int64_t G) { return dim3((unsigned)((k + kRpBlock - 1) / kRpBlock), (unsigned)G); }
dim3 wave_grid(int64_t waves) { return dim3((unsigned)((waves + kRpWaves - 1) / kRpWaves)); }

int rp_run(const uint32_t* states, const uint32_t* words, int64_t n, int64_t D, int64_t k, int64_t* index_out,
           uint32_t* drop_bits, void* ws, size_t ws_bytes, hipStream_t st) {
    t_last_plan = RpPlan{};
    int rc = rp_check(n, D, k);
    if (rc) return rc;
    if (n == 0) return UQ_OK;
    const int64_t W = (D + 31) / 32;
    if (drop_bits && W) {                                // an empty set when k = 0
        if ((rc = hip_check(hipMemsetAsync(drop_bits, 0, (size_t)n * W * 4, st), "zero drop_bits"))) return rc;
    }
    if (k == 0) return UQ_OK;
    RpPlan P = rp_plan(n, D, k, words != nullptr);
    if (P.K > 0 && !states && !words) return fail(UQ_E_INVALID, "randperm: null states");
    if (words && P.K > kRpMaxTestWords) return fail(UQ_E_INVALID, "uq_test_randperm_from_words: at most 65536 words per client");
    if (!ws) return fail(UQ_E_INVALID, "randperm: null workspace");
    P.G = rp_group(P, n, D, k, ws_bytes);
    if (P.G < 1) return fail(UQ_E_WORKSPACE, "workspace too small (uq_randperm_prefix_workspace_bytes)");
    P.groups = (n + P.G - 1) / P.G;
    const uint32_t* polys = nullptr;
    if (P.form == UQ_RANDPERM_FORM_JUMP && (rc = rp_polys(P, &polys))) return rc;
    const RpLayout l = rp_layout(P, P.G, D, k);
    char* wsb = (char*)ws;
    int rounds = 1;
    while (((int64_t)1 << (rounds - 1)) < k) ++rounds;   // ceil(log2 k) + 1: the last finds nothing to move
    rounds = std::min(rounds, kRpMaxRounds);
    for (int64_t g0 = 0; g0 < n; g0 += P.G) {
        const int64_t G = std::min(P.G, n - g0);
        RpArgs a{};
        a.states = states ? states + g0 * kQfStateWords : nullptr;
        a.words = words ? words + g0 * P.K : nullptr;
        a.parts = (const uint32_t*)(wsb + l.parts);
        a.n = G;
        a.D = D;
        a.k = k;
        a.K = P.K;
        a.R = std::max(P.R, 1);
        a.L = P.L;
        a.h = (uint32_t*)(wsb + l.h);
        a.head = (int32_t*)(wsb + l.head);
        a.next = (int32_t*)(wsb + l.next);
        a.a = (int32_t*)(wsb + l.a);
        a.flags = (int32_t*)(wsb + kRpFlagsOff);
        a.index_out = index_out ? index_out + g0 * k : nullptr;
        a.drop_bits = drop_bits ? drop_bits + g0 * W : nullptr;
        a.W = W;
        if ((rc = hip_check(hipMemsetAsync(a.flags, 0, 256, st), "zero flags"))) return rc;
        if ((rc = hip_check(hipMemsetAsync(a.head, 0xFF, (size_t)G * D * 4, st), "reset heads"))) return rc;
        if (P.K > 0) {
            if (P.form == UQ_RANDPERM_FORM_WORDS) {
                hipLaunchKernelGGL(randperm_words_kernel, step_grid(P.K, G), dim3(kRpBlock), 0, st, a);
                if ((rc = launched("randperm_words_kernel launch"))) return rc;
            } else {
                if (P.form == UQ_RANDPERM_FORM_JUMP) {
                    uint32_t* xs = (uint32_t*)(wsb + l.xs);
                    hipLaunchKernelGGL(randperm_stream_kernel, wave_grid(G), dim3(64 * kRpWaves), 0, st, a, xs);
                    if ((rc = launched("randperm_stream_kernel launch"))) return rc;
                    QflJumpArgs ja{};
                    ja.polyA = polys;
                    ja.polyB = polys;                    // (unused: one kind)
                    ja.xs = xs;
                    ja.parts = (uint32_t*)(wsb + l.parts);
                    ja.R = P.R;
                    ja.n = G;
                    ja.nstreams = 1;
                    ja.kinds = 1;
                    hipLaunchKernelGGL(quicfl_jump_kernel, dim3((unsigned)(G * P.R * kMjParts)), dim3(256), 0, st, ja);
                    if ((rc = launched("quicfl_jump_kernel launch"))) return rc;
                }
                hipLaunchKernelGGL(randperm_targets_kernel, wave_grid(G * a.R), dim3(64 * kRpWaves), 0, st, a);
                if ((rc = launched("randperm_targets_kernel launch"))) return rc;
            }
        }
        const dim3 grid = step_grid(k, G);
        hipLaunchKernelGGL(randperm_link_kernel, grid, dim3(kRpBlock), 0, st, a);
        if ((rc = launched("randperm_link_kernel launch"))) return rc;
        hipLaunchKernelGGL(randperm_par_kernel, grid, dim3(kRpBlock), 0, st, a);
        if ((rc = launched("randperm_par_kernel launch"))) return rc;
        for (int t = 0; t < rounds; ++t) {
            hipLaunchKernelGGL(randperm_root_kernel, grid, dim3(kRpBlock), 0, st, a, t);
            if ((rc = launched("randperm_root_kernel launch"))) return rc;
        }
        hipLaunchKernelGGL(randperm_out_kernel, grid, dim3(kRpBlock), 0, st, a);
        if ((rc = launched("randperm_out_kernel launch"))) return rc;
    }
    t_last_plan = P;
    return UQ_OK;
}

}  // namespace

extern "C" {

int uq_randperm_prefix_workspace_bytes(int64_t n, int64_t D, int64_t k, size_t* bytes_out) {
    if (!bytes_out) return fail(UQ_E_INVALID, "null bytes_out");
    if (const int rc = rp_check(n, D, k)) return rc;
    *bytes_out = 0;
    if (n == 0 || k == 0) return UQ_OK;
    const RpPlan P = rp_plan(n, D, k, false);
    const int64_t G = std::max<int64_t>(1, rp_group(P, n, D, k, kRpWorkspaceCap));
    *bytes_out = rp_layout(P, G, D, k).total;
    return UQ_OK;
}

int uq_randperm_prefix(const uint32_t* states, int64_t n, int64_t D, int64_t k, int64_t* index_out, uint32_t* drop_bits,
                       void* ws, size_t ws_bytes, void* stream) {
    return rp_run(states, nullptr, n, D, k, index_out, drop_bits, ws, ws_bytes, (hipStream_t)stream);
}

int uq_test_randperm_from_words(const uint32_t* words, int64_t n, int64_t D, int64_t k, int64_t* index_out,
                                uint32_t* drop_bits, void* ws, size_t ws_bytes, void* stream) {
    if (!words && n > 0 && k > 0 && D > 1) return fail(UQ_E_INVALID, "uq_test_randperm_from_words: null words");
    static const uint32_t none = 0;                      // (D = 1 takes no word: any non-null pointer selects the form)
    return rp_run(nullptr, words ? words : &none, n, D, k, index_out, drop_bits, ws, ws_bytes, (hipStream_t)stream);
}

int uq_test_last_randperm_plan(int64_t* plan_out, int32_t cap) {
    if (!plan_out || cap < 0) return fail(UQ_E_INVALID, "null plan output");
    const RpPlan& p = t_last_plan;
    const int64_t f[UQ_RANDPERM_PLAN_FIELDS] = {p.form, p.R, p.L, p.G, p.K, p.groups};
    std::copy(f, f + std::min<int32_t>(cap, UQ_RANDPERM_PLAN_FIELDS), plan_out);
    return UQ_OK;
}

}  // extern "C"
