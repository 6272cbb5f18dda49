// uq_rand.hip — Scalar_quantize and DRIVE_quantize_Hadamard (the baselines that draw
// torch.rand_like from the global CPU generator): the launchers of uq_rand_kernels.h and their
// C API (uq_rand_workspace_bytes, uq_drive_words, uq_scalar_quantize_f32, uq_drive_hadamard_f32).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "uq_internal.h"
#include "uq_rand_kernels.h"

namespace {

constexpr int64_t kRandMaxD = (int64_t)1 << 28;
constexpr int64_t kRandMaxGrid = 0x7FFFFFFFll;

// Workspace of a call on (n, d): Scalar's partials, then DRIVE's sign bits (either call fits).
struct RandLayout {
    int32_t parts;              // KR1 slices per client
    int64_t words, row_words;   // DRIVE: generator words and 64-bit words of sign bits per client
    int64_t nchunks;
    size_t part_off, bits_off, total;
};

RandLayout rand_layout(int64_t n, int64_t d) {
    RandLayout l;
    l.parts = (int32_t)std::max<int64_t>(1, std::min<int64_t>(kMinMaxParts, (d + kMinMaxSlice - 1) / kMinMaxSlice));
    l.words = drive_words(d);
    l.row_words = (l.words + 63) / 64;
    l.nchunks = (d + kDriveChunk - 1) / kDriveChunk;
    l.part_off = 0;
    l.bits_off = up256((size_t)n * l.parts * sizeof(float4));
    l.total = l.bits_off + up256((size_t)n * l.row_words * sizeof(uint64_t));
    return l;
}

// The checks both schemes share; *run = false for the empty batch (a no-op).
int rand_check(const char* who, const float* x, float* out, int64_t n, int64_t d, const uint32_t* px_state,
               const int32_t* px_seeds, void* ws, size_t ws_bytes, RandLayout* l, bool* run) {
    const std::string w(who);
    *run = false;
    if (n < 0 || d < 0) return fail(UQ_E_INVALID, w + ": n and d must be >= 0");
    if (d > kRandMaxD) return fail(UQ_E_INVALID, w + ": d above 2^28");
    if (n == 0 || d == 0) return UQ_OK;
    if (!x || !out) return fail(UQ_E_INVALID, w + ": null x or out");
    if (!px_state && !px_seeds) return fail(UQ_E_INVALID, w + ": px_state or px_seeds is required");
    if (!ws) return fail(UQ_E_INVALID, w + ": null workspace");
    *l = rand_layout(n, d);
    if (n > kRandMaxGrid / kMinMaxParts || n * l->nchunks > kRandMaxGrid)
        return fail(UQ_E_INVALID, w + ": batch too large for one call");
    if (ws_bytes < l->total) return fail(UQ_E_WORKSPACE, w + ": workspace too small (uq_rand_workspace_bytes)");
    *run = true;
    return UQ_OK;
}

}  // namespace

extern "C" {

int uq_rand_workspace_bytes(int64_t n, int64_t d, size_t* bytes_out) {
    if (!bytes_out) return fail(UQ_E_INVALID, "null bytes_out");
    if (n < 0 || d < 0) return fail(UQ_E_INVALID, "n and d must be >= 0");
    if (d > kRandMaxD) return fail(UQ_E_INVALID, "d above 2^28");
    *bytes_out = rand_layout(n, d).total;
    return UQ_OK;
}

int uq_drive_words(int64_t d, int64_t* words_out) {
    if (!words_out) return fail(UQ_E_INVALID, "null words_out");
    if (d < 0 || d > kRandMaxD) return fail(UQ_E_INVALID, "d must be in 0..2^28");
    *words_out = drive_words(d);
    return UQ_OK;
}

int uq_scalar_quantize_f32(const float* x, float* out, int64_t n, int64_t d, float nlevels, const uint32_t* px_state,
                           const int32_t* px_seeds, uint32_t* px_state_out, int32_t* info, void* ws, size_t ws_bytes,
                           void* stream) {
    if (!(nlevels >= 1.0f) || std::isinf(nlevels))
        return fail(UQ_E_INVALID, "uq_scalar_quantize_f32: nlevels must be finite and >= 1 (below, the reference returns its input)");
    RandLayout l;
    bool run;
    if (int rc = rand_check("uq_scalar_quantize_f32", x, out, n, d, px_state, px_seeds, ws, ws_bytes, &l, &run)) return rc;
    if (!run) return UQ_OK;
    if (!info) return fail(UQ_E_INVALID, "uq_scalar_quantize_f32: null info");
    hipStream_t st = (hipStream_t)stream;
    float4* part = reinterpret_cast<float4*>((char*)ws + l.part_off);
    scalar_minmax_kernel<<<dim3((unsigned)(n * l.parts)), dim3(kQBlock), 0, st>>>(x, d, l.parts, part);
    if (int rc = launched("scalar_minmax_kernel launch")) return rc;
    const RandGen gen{px_state, px_seeds, px_state_out};
    scalar_walk_kernel<<<dim3((unsigned)((n + kRwWavesPerWG - 1) / kRwWavesPerWG)), dim3(64 * kRwWavesPerWG), 0, st>>>(
        x, out, n, d, nlevels, part, l.parts, gen, info);
    return launched("scalar_walk_kernel launch");
}

int uq_drive_hadamard_f32(const float* x, float* out, int64_t n, int64_t d, const uint32_t* px_state,
                          const int32_t* px_seeds, uint32_t* px_state_out, float* S_out, void* ws, size_t ws_bytes,
                          void* stream) {
    RandLayout l;
    bool run;
    if (int rc = rand_check("uq_drive_hadamard_f32", x, out, n, d, px_state, px_seeds, ws, ws_bytes, &l, &run)) return rc;
    if (!run) return UQ_OK;
    hipStream_t st = (hipStream_t)stream;
    uint64_t* bits = reinterpret_cast<uint64_t*>((char*)ws + l.bits_off);
    const RandGen gen{px_state, px_seeds, px_state_out};
    drive_bits_kernel<<<dim3((unsigned)((n + kRwWavesPerWG - 1) / kRwWavesPerWG)), dim3(64 * kRwWavesPerWG), 0, st>>>(
        n, l.words, gen, bits, l.row_words);
    if (int rc = launched("drive_bits_kernel launch")) return rc;
    drive_chunk_kernel<<<dim3((unsigned)(n * l.nchunks)), dim3(kQBlock), 0, st>>>(x, out, d, l.nchunks, bits,
                                                                                  l.row_words, S_out);
    return launched("drive_chunk_kernel launch");
}

}  // extern "C"
