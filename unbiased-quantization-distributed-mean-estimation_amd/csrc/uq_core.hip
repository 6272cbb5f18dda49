// uq_core.hip — the library's host core, no kernels: the per-thread error string (fail /
// hip_check / uq_last_error), aligned16, the side streams, uq_version, uq_build_id,
// uq_rate_to_m and uq_check_status.  What the schemes' translation units (uq_unbiased.hip,
// uq_biased.hip, uq_eden.hip, uq_quicfl.hip, uq_codec.hip) share on the host, declared in
// uq_internal.h.  A .hip only for the HIP runtime header: the build compiles .cpp with g++.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "uq_internal.h"

namespace {

thread_local std::string g_err;

}  // namespace

int uq_internal::fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

int uq_internal::hip_check(hipError_t e, const char* what) {
    if (e != hipSuccess) return fail(UQ_E_HIP, std::string(what) + ": " + hipGetErrorString(e));
    return UQ_OK;
}

bool uq_internal::aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

// The side stream of this device and thread (SideStream: uq_internal.h), created on first use.
int uq_internal::side_stream(SideStream** out) {
    int dev = 0;
    int rc = hip_check(hipGetDevice(&dev), "hipGetDevice");
    if (rc) return rc;
    static thread_local SideStream cache[64];
    static thread_local bool made[64] = {};
    if (dev < 0 || dev >= 64) return fail(UQ_E_INVALID, "device index out of range");
    if (!made[dev]) {
        // the side stream carries short dependent chains (KB7) beside a bandwidth-bound kernel on
        // the caller's stream: give it the highest priority so its workgroups dispatch first
        int least = 0, greatest = 0;
        rc = hip_check(hipDeviceGetStreamPriorityRange(&least, &greatest), "stream priority range");
        if (rc) return rc;
        rc = hip_check(hipStreamCreateWithPriority(&cache[dev].s, hipStreamNonBlocking, greatest), "create side stream");
        if (rc) return rc;
        rc = hip_check(hipEventCreateWithFlags(&cache[dev].fork, hipEventDisableTiming), "create event");
        if (rc) return rc;
        rc = hip_check(hipEventCreateWithFlags(&cache[dev].join, hipEventDisableTiming), "create event");
        if (rc) return rc;
        rc = hip_check(hipEventCreateWithFlags(&cache[dev].mid, hipEventDisableTiming), "create event");
        if (rc) return rc;
        rc = hip_check(hipHostMalloc((void**)&cache[dev].count, sizeof(uint32_t), hipHostMallocDefault), "pinned word");
        if (rc) return rc;
        rc = hip_check(hipHostMalloc(&cache[dev].states, kSmallCheckMaxN * 32, hipHostMallocDefault), "pinned states");
        if (rc) return rc;
        made[dev] = true;
    }
    *out = &cache[dev];
    return UQ_OK;
}

extern "C" {

int uq_version(void) { return 103; }

#ifndef UQ_BUILD_ID
#define UQ_BUILD_ID "unknown"
#endif
const char* uq_build_id(void) { return UQ_BUILD_ID; }

const char* uq_last_error(void) { return g_err.c_str(); }

int uq_rate_to_m(double bits, int64_t d, int64_t* m_out) {
    // AS:614-620
    static const double keys[20] = {0.5, 1, 1.5, 2, 2.5, 3, 3.5, 4, 4.5, 5,
                                    5.5, 6, 6.5, 7, 7.5, 8, 8.5, 9, 9.5, 10};
    static const double vals[20] = {0.08282, 0.21403, 0.39443, 0.63752, 0.96656, 1.41725, 2.04187,
                                    2.91504, 4.14217, 5.87195, 8.31416, 11.76507, 16.64332, 23.54075,
                                    33.29414, 47.0868, 66.59204, 94.17625, 133.18596, 188.35383};
    if (!m_out) return fail(UQ_E_INVALID, "null m_out");
    if (d < 0) return fail(UQ_E_INVALID, "d must be >= 0");
    for (int i = 0; i < 20; ++i)
        if (bits == keys[i]) {
            *m_out = (int64_t)(vals[i] * (double)d);   // AS:623 int(l * d), truncation
            return UQ_OK;
        }
    return fail(UQ_E_INVALID, "bits_per_dimension not in the rate table (reference raises KeyError)");
}

int uq_check_status(void* ws, void* stream) {
    if (!ws) return fail(UQ_E_INVALID, "null workspace");
    hipStream_t st = (hipStream_t)stream;
    uint32_t status = 0;
    int rc = hip_check(hipMemcpyAsync(&status, (char*)ws + 8, 4, hipMemcpyDeviceToHost, st), "read status");
    if (rc) return rc;
    rc = hip_check(hipStreamSynchronize(st), "sync");
    if (rc) return rc;
    if (status) {
        (void)hipMemsetAsync((char*)ws + 8, 0, 4, st);
        (void)hipStreamSynchronize(st);
        if (status == 2) return fail(UQ_E_TIMEOUT, "torch tie replay inconsistent (internal error)");
        return fail(UQ_E_TIMEOUT, "inter-workgroup wait timed out");
    }
    return UQ_OK;
}

}  // extern "C"
