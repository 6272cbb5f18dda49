// uq_internal.h — host functions and state that cross the library's translation units.
//
// Each scheme is one .hip (uq_unbiased.hip, uq_biased.hip, uq_eden.hip, uq_quicfl.hip, uq_rand.hip,
// uq_kashin.hip, uq_codec.hip) beside the host core, uq_core.hip.  What they share on the host is declared
// here and defined in exactly one of them, so every piece of state (the error string, the side
// streams) exists once in the library.  Nothing here is exported: the
// namespace has hidden visibility.  Signatures use plain types only: the kernels' argument
// structs live in anonymous namespaces (their names are part of the kernels' symbols), so they
// cannot cross.
#ifndef UQ_INTERNAL_H
#define UQ_INTERNAL_H

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <string>
#include <type_traits>

#include "../../include/uq_dme.h"

namespace uq_internal __attribute__((visibility("hidden"))) {

constexpr int64_t kMaxGridY = 65535;       // clients per launch of the kernels with one grid row per client

// Workspace regions start on 256-byte boundaries: v rounded up to the next one.
constexpr size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

// ---- uq_core.hip ---------------------------------------------------------------------
// Records msg as the calling thread's uq_last_error() and returns code.
int fail(int code, const std::string& msg);
int hip_check(hipError_t e, const char* what);
bool aligned16(const void* p);
// After a kernel launch: hip_check of the launch's error.
inline int launched(const char* what) { return hip_check(hipGetLastError(), what); }
// A run-time flag as a compile-time constant, for the selectors of template instances.
template <bool B>
using Flag = std::integral_constant<bool, B>;

// A second stream per device and thread (plus fork / join events) for work that can run
// beside the caller's stream inside one call; joined back before the call returns.
struct SideStream {
    hipStream_t s;
    hipEvent_t fork, join, mid;         // mid: KB7a's bandwidth-heavy first levels done
    uint32_t* count;            // pinned host word (UQ_TIES_HOST_CHECK reads the tie list's length)
    void* states;               // pinned host RezStates (the small-vector path's flags), kSmallCheckMaxN
};
constexpr int64_t kSmallCheckMaxN = 64;    // clients per host-checked small-vector biased call
int side_stream(SideStream** out);

// Forks the thread's side stream from st; join() records the side stream's end and makes st
// wait for it.  The destructor joins if that has not happened, so once forked the caller's
// stream waits on every exit path: the side kernels write into the caller's workspace, which
// may be freed or reused after an early error return.
class SideFork {
public:
    SideFork(hipStream_t st, int* rc) : st_(st) {
        if ((*rc = side_stream(&sb_))) return;
        if ((*rc = hip_check(hipEventRecord(sb_->fork, st), "record fork"))) return;
        if ((*rc = hip_check(hipStreamWaitEvent(sb_->s, sb_->fork, 0), "wait fork"))) return;
        open_ = true;
    }
    SideFork(const SideFork&) = delete;
    SideFork& operator=(const SideFork&) = delete;
    ~SideFork() { (void)join(); }
    hipStream_t side() const { return sb_->s; }
    // The reverse wait, before the join: st waits for what the side stream holds so far.
    int wait_mid() {
        const int rc = hip_check(hipEventRecord(sb_->mid, sb_->s), "record mid");
        return rc ? rc : hip_check(hipStreamWaitEvent(st_, sb_->mid, 0), "wait mid");
    }
    int join() {
        if (!open_) return UQ_OK;
        open_ = false;
        const int rc = hip_check(hipEventRecord(sb_->join, sb_->s), "record join");
        return rc ? rc : hip_check(hipStreamWaitEvent(st_, sb_->join, 0), "wait join");
    }

private:
    hipStream_t st_;
    SideStream* sb_ = nullptr;
    bool open_ = false;
};

// ---- uq_unbiased.hip -----------------------------------------------------------------
// AS:624 |x|.sum() of n rows in torch CPU order for T intra-op threads (K1a + K1b with AbsOp).
// part: n * total_groups * 32 floats of the plan make_plan(d, T) gives; the caller has checked
// that the plan exists.
int launch_l1(const float* x, int64_t n, int64_t d, int32_t T, float* part, float* l1_out, hipStream_t st);

// ---- uq_eden.hip: the RHT and the norm as QUIC-FL's sender uses them -------------------
// The EDEN workspace layout of (n, dim): D = dim padded to a power of two, the norms at
// nrm_off, `total` bytes in all (QUIC-FL's own regions follow).
struct RhtLayout {
    size_t nrm_off, total;
    int64_t D;
};
RhtLayout rht_layout(int64_t n, int64_t dim);
// RHT (AS:123-141) and torch.norm (AS:329) of n rows in the workspace wsb; *rot = the rotated
// vectors (one of the workspace's two vector buffers), the norms at rht_layout's nrm_off.
int rht_norm_front(const float* x, int64_t n, int64_t dim, const int8_t* signs, const int32_t* sign_row, char* wsb,
                   float** rot, hipStream_t st);
// The receiver's inverse RHT (H, then * diag) of rot [n][D], in place but for the last pass,
// which writes out [n][dim].
int rht_inverse(float* rot, float* out, int64_t n, int64_t D, int64_t dim, const int8_t* signs,
                const int32_t* sign_row, hipStream_t st);
// The sender's RHT of rows that are D = 2^p long already (Kashin's padded residual, AS:222-224): the
// passes alternate between buf and out [n][D] each, x is only read; *result = the one holding the result.
int rht_forward_rows(const float* x, float* buf, float* out, int64_t n, int64_t D, const int8_t* signs,
                     const int32_t* sign_row, float** result, hipStream_t st);

}  // namespace uq_internal

// (only the library's own translation units include this header)
using namespace uq_internal;

#endif  // UQ_INTERNAL_H
