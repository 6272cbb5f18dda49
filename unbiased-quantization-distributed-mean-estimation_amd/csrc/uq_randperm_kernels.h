// uq_randperm_kernels.h — torch.randperm(D)[:k] of the CPU generator, per client.  Included by
// uq_randperm.hip.
//
// torch's CPU randperm (D < 2^32 / 20) is a forward Fisher-Yates shuffle: step i = 0 .. D - 2 swaps
// r[i] with r[h_i], h_i = i + w_i % (D - i), w_i the generator's i-th 32-bit word.  The first k
// entries are final after K = min(k, D - 1) steps; for k = D the entry D - 1 is a step that hits
// itself (h = D - 1, no word).  Without the serial chain:
//   W(p, i) = the largest step j < i with h_j = p, or none
//   par(j)  = W(j, j);  root(j) follows par until there is none (par(j) < j, so it ends): what
//             position j holds when step j begins
//   r[i]    = root(i) if h_i = i, else with q = W(h_i, i): h_i if q is none, else root(q)
// Kernels (one client per grid row, a thread per step unless said otherwise):
//   KP0s randperm_stream_kernel   jump form: the first 33 blocks of each client's stream, one wave each
//   KQ0j quicfl_jump_kernel       jump form: each run's starting block (uq_mt_jump_kernels.h)
//   KP1  randperm_targets_kernel  one wave per (client, run) walks the run's blocks: h_i
//   KP1w randperm_words_kernel    the test entry: h_i from words given by the caller
//   KP2  randperm_link_kernel     the writers of each position as a linked list (head per position,
//                                 next per step): atomic exchanges place them in arrival order, and
//                                 every reader takes a maximum over the whole list, which is the
//                                 same in any order
//   KP3  randperm_par_kernel      a[i] = par(i), or i
//   KP4  randperm_root_kernel     one round of pointer doubling, a[i] = a[a[i]], in place: a[i] only
//                                 ever moves towards its root, so a round that reads a value another
//                                 thread has just advanced is only further on; ceil(log2 k) rounds
//                                 reach every root, and a round in which nothing moved ends the rest
//   KP5  randperm_out_kernel      q by the list of h_i, r[i] as int64 and as a bit of the drop row
// Every list walk is bounded: a list's members are distinct steps, all below i in the list of
// position i (h_j = i needs j <= i, which is par(j) < j), and at most k in any list.

#ifndef UQ_RANDPERM_KERNELS_H
#define UQ_RANDPERM_KERNELS_H

#include "uq_mt_jump_kernels.h"

namespace {

constexpr int kRpWaves = 4;                  // waves per workgroup of KP0s / KP1
constexpr int kRpBlock = 256;                // threads per workgroup of the per-step kernels
constexpr int kRpMaxRounds = 32;             // doubling rounds at most (k < 2^28)

struct RpArgs {
    const uint32_t* states;     // [n][626] (left, next, words) per client
    const uint32_t* words;      // the test entry: [n][K] words, else null
    const uint32_t* parts;      // jump form: KQ0j's partial windows [n][R][kMjParts][624]
    int64_t n, D, k, K;         // clients of this group; K = min(k, D - 1) words per client
    int32_t R;                  // runs per client
    int64_t L;                  // blocks per run
    uint32_t* h;                // [n][K]
    int32_t* head;              // [n][D]: the last arrival among the steps that hit the position, or -1
    int32_t* next;              // [n][k]: the arrival before this step at its position, or -1
    int32_t* a;                 // [n][k]: par, then the ancestor the doubling has reached, at last root
    int32_t* flags;             // [kRpMaxRounds + 1]: flags[t] != 0: round t still has work
    int64_t* index_out;         // [n][k] or null
    uint32_t* drop_bits;        // [n][W] or null (zeroed before KP5)
    int64_t W;
};

// KP0s: x[0 .. kMjX) of each client's stream (the state's block as given, then 32 twists)
__global__ void __launch_bounds__(64 * kRpWaves)
randperm_stream_kernel(RpArgs a, uint32_t* xs) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t j = (int64_t)blockIdx.x * kRpWaves + wv;
    if (j >= a.n) return;
    uint32_t st[kMtGroups];
    mt_load(st, a.states + j * kQfStateWords + 2, lane);
    uint32_t* x = xs + j * kMjX;
    mt_store(st, x, lane);
    for (int b = 1; b < kMjBlocks; ++b) {
        mt_twist_reg(st, lane);
        mt_store(st, x + b * kMtN, lane);
    }
}

// KP1: wave (client j, run r) walks blocks [r L, r L + L) of the client's stream, block 0 being
// the state as given: word i sits at slot (vG + i) % 624 of block (vG + i) / 624, vG = next (624
// when the block is used up: left = 1).  Run 0 starts from the state, run r >= 1 from its jumped block.
__global__ void __launch_bounds__(64 * kRpWaves)
randperm_targets_kernel(RpArgs a) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t id = (int64_t)blockIdx.x * kRpWaves + wv;
    const int64_t j = id / a.R;
    const int r = (int)(id % a.R);
    if (j >= a.n) return;
    const uint32_t* state = a.states + j * kQfStateWords;
    const int32_t gleft = __builtin_amdgcn_readfirstlane((int32_t)state[0]);
    const int32_t gnext = __builtin_amdgcn_readfirstlane((int32_t)state[1]);
    const int64_t vG = gleft > 1 ? (int64_t)gnext : (int64_t)kMtN;
    const int64_t b1 = (vG + a.K - 1) / kMtN;
    const int64_t c0 = (int64_t)r * a.L, c1 = min(b1, c0 + a.L - 1);
    if (c0 > c1) return;
    uint32_t s[kMtGroups];
    if (r == 0) mt_load(s, state + 2, lane);
    else mj_block(s, a.parts + (j * a.R + r) * kMjParts * kMtN, lane);
    uint32_t* h = a.h + j * a.K;
    for (int64_t b = c0; b <= c1; ++b) {
        if (b > c0) mt_twist_reg(s, lane);
#pragma unroll
        for (int g = 0; g < kMtGroups; ++g) {
            const int slot = 64 * g + lane;
            const int64_t i = b * kMtN + slot - vG;
            if (slot < kMtN && i >= 0 && i < a.K) h[i] = (uint32_t)i + mt_temper(s[g]) % (uint32_t)(a.D - i);
        }
    }
}

// KP1w: the same from words the caller gives
__global__ void __launch_bounds__(kRpBlock)
randperm_words_kernel(RpArgs a) {
    const int64_t j = blockIdx.y, i = (int64_t)blockIdx.x * kRpBlock + threadIdx.x;
    if (i >= a.K) return;
    a.h[j * a.K + i] = (uint32_t)i + a.words[j * a.K + i] % (uint32_t)(a.D - i);
}

// h_i of client j (i < k): the virtual step D - 1 of k = D hits itself
// (a value outside [i, D) can only come from a state that breaks ATen's (left, next) invariant, whose
// walk leaves words unwritten: it is read as a self-hit, so that no index below leaves its array)
__device__ __forceinline__ int32_t rp_target(const RpArgs& a, int64_t j, int64_t i) {
    if (i >= a.K) return (int32_t)i;
    const uint32_t v = a.h[j * a.K + i];
    return v >= (uint32_t)i && v < (uint32_t)a.D ? (int32_t)v : (int32_t)i;
}

// The largest member below i of position p's list, or -1 (members are distinct steps: at most
// `bound` of them, whatever the memory holds)
__device__ __forceinline__ int32_t rp_last_below(const int32_t* head, const int32_t* next, int64_t p, int32_t i,
                                                 int64_t bound) {
    int32_t best = -1;
    int32_t e = head[p];
    for (int64_t t = 0; t < bound && e >= 0; ++t) {
        if (e < i) best = max(best, e);
        e = next[e];
    }
    return best;
}

// KP2
__global__ void __launch_bounds__(kRpBlock)
randperm_link_kernel(RpArgs a) {
    const int64_t j = blockIdx.y, i = (int64_t)blockIdx.x * kRpBlock + threadIdx.x;
    if (i >= a.k) return;
    const int32_t hi = rp_target(a, j, i);
    int32_t prev = -1;
    if (hi != (int32_t)i) prev = atomicExch(a.head + j * a.D + hi, (int32_t)i);    // (a self-hit writes nothing)
    a.next[j * a.k + i] = prev;
}

// KP3
__global__ void __launch_bounds__(kRpBlock)
randperm_par_kernel(RpArgs a) {
    const int64_t j = blockIdx.y, i = (int64_t)blockIdx.x * kRpBlock + threadIdx.x;
    if (i >= a.k) return;
    if (i == 0 && j == 0) a.flags[0] = 1;                                 // (zeroed before the group: round 0 runs)
    const int32_t p = rp_last_below(a.head + j * a.D, a.next + j * a.k, i, (int32_t)i, i);
    a.a[j * a.k + i] = p >= 0 ? p : (int32_t)i;
}

// KP4, round t
__global__ void __launch_bounds__(kRpBlock)
randperm_root_kernel(RpArgs a, int32_t t) {
    if (!a.flags[t]) return;
    const int64_t j = blockIdx.y, i = (int64_t)blockIdx.x * kRpBlock + threadIdx.x;
    if (i >= a.k) return;
    int32_t* row = a.a + j * a.k;
    const int32_t x = __hip_atomic_load(row + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (x < 0 || x > (int32_t)i) return;                                  // (never: par(i) <= i)
    const int32_t y = __hip_atomic_load(row + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (y != x && y >= 0 && y < x) {
        __hip_atomic_store(row + i, y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(a.flags + t + 1, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// KP5
__global__ void __launch_bounds__(kRpBlock)
randperm_out_kernel(RpArgs a) {
    const int64_t j = blockIdx.y, i = (int64_t)blockIdx.x * kRpBlock + threadIdx.x;
    if (i >= a.k) return;
    const int32_t* root = a.a + j * a.k;
    const int32_t hi = rp_target(a, j, i);
    int32_t r;
    if (hi == (int32_t)i) {
        r = root[i];
    } else {
        const int32_t q = rp_last_below(a.head + j * a.D, a.next + j * a.k, hi, (int32_t)i, a.k);   // (later steps too)
        r = q < 0 ? hi : root[q];
    }
    if (r < 0 || r >= a.D) return;                                        // (never)
    if (a.index_out) a.index_out[j * a.k + i] = r;
    if (a.drop_bits) atomicOr(a.drop_bits + j * a.W + (r >> 5), 1u << (r & 31));
}

}  // namespace

#endif  // UQ_RANDPERM_KERNELS_H
