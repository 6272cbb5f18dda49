// uq_kashin.hip — Kashin_quantize (AS:834-854): the loop of KashinSender.kashin_coefficients
// (AS:212-239) on the device with no host wait, the stochastic quantizer of its coefficients
// (AS:67-82) and the receiver (AS:269-274); the launchers of uq_kashin_kernels.h and the C API
// uq_kashin_*.  The transforms are EDEN's passes (rht_forward_rows, rht_inverse in uq_internal.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "uq_internal.h"
// (uq_rand_kernels.h comes with the walker and KR1; its other kernels are not launched here)
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunused-function"
#include "uq_kashin_kernels.h"
#pragma clang diagnostic pop

namespace {

constexpr int64_t kKashinMaxD = (int64_t)1 << 28;
constexpr int64_t kKashinMaxGrid = 0x7FFFFFFFll;

// Workspace of a call on (n, D): the residual, two transform buffers and the coefficients, [n][D]
// f32 each; then the per-client scalars and KR1's partials.
struct KashinLayout {
    int32_t parts;              // KR1 slices per client
    size_t r_off, a_off, b_off, c_off, nrm_off, M_off, done_off, iters_off, mn_off, step_off, part_off, total;
};

KashinLayout kashin_layout(int64_t n, int64_t D) {
    KashinLayout l;
    l.parts = (int32_t)std::max<int64_t>(1, std::min<int64_t>(kMinMaxParts, (D + kMinMaxSlice - 1) / kMinMaxSlice));
    const size_t vec = up256((size_t)n * D * sizeof(float)), sc = up256((size_t)n * sizeof(float));
    l.r_off = kCtrlBytes;
    l.a_off = l.r_off + vec;
    l.b_off = l.a_off + vec;
    l.c_off = l.b_off + vec;
    l.nrm_off = l.c_off + vec;              // [3][n]: norm(x), then the exit test's numerator and denominator
    l.M_off = l.nrm_off + 3 * sc;
    l.done_off = l.M_off + sc;
    l.iters_off = l.done_off + sc;
    l.mn_off = l.iters_off + sc;
    l.step_off = l.mn_off + sc;
    l.part_off = l.step_off + sc;
    l.total = l.part_off + up256((size_t)n * l.parts * sizeof(float4));
    return l;
}

struct KashinCall {
    int64_t n, dim, D;
    const int8_t* signs;
    const int32_t* sign_row;
    void* ws;
    size_t ws_bytes;
    void* stream;
    KashinLayout w;
    template <class T>
    T* at(size_t off) const { return reinterpret_cast<T*>((char*)ws + off); }
    dim3 egrid(int64_t len) const { return dim3((unsigned)((len + kKeT * kKeQ - 1) / (kKeT * kKeQ)), (unsigned)n); }
    dim3 cgrid() const { return dim3((unsigned)((n + kKeT - 1) / kKeT)); }
};

// The checks every entry shares, before any launch; *run = false for the empty batch (a no-op).
int kashin_check(KashinCall& c, bool null_ptr, bool* run) {
    *run = false;
    if (c.n < 0 || c.dim < 0) return fail(UQ_E_INVALID, "kashin: n and dim must be >= 0");
    if (c.n > kMaxGridY) return fail(UQ_E_INVALID, "kashin: at most 65535 clients per call");
    if (c.n == 0 || c.dim == 0) return UQ_OK;
    if (c.D < 2 || (c.D & (c.D - 1)) != 0 || c.D < c.dim)
        return fail(UQ_E_INVALID, "kashin: D must be a power of two >= max(2, dim) (uq_kashin_padded_dim)");
    if (c.D > kKashinMaxD) return fail(UQ_E_INVALID, "kashin: D above 2^28");
    if (null_ptr || !c.signs) return fail(UQ_E_INVALID, "kashin: null pointer");
    c.w = kashin_layout(c.n, c.D);
    if (!c.ws || c.ws_bytes < c.w.total) return fail(UQ_E_WORKSPACE, "kashin: workspace too small (uq_kashin_workspace_bytes)");
    *run = true;
    return UQ_OK;
}

struct KashinParams {
    int32_t niters;
    double eta, delta, err;
    int32_t nlevels;
    const uint32_t* runs;
    const int32_t* run_row;
    int64_t run_words;
};

int kashin_check_params(const KashinCall& c, const KashinParams& p) {
    if (p.niters < 1) return fail(UQ_E_INVALID, "kashin: niters must be >= 1");
    if (p.nlevels < 2 || p.nlevels > 256) return fail(UQ_E_INVALID, "kashin: nlevels must be in 2..256");
    if (!(p.delta > 0.0)) return fail(UQ_E_INVALID, "kashin: delta must be > 0");
    // AS:236 at i = 0 compares 1.0 (or NaN) with the bound; kashin_coefficients skips that test
    if ((float)p.err > 1.0f)
        return fail(UQ_E_INVALID, "kashin: err must be <= 1 as f32 (above it the reference exits after the first transform, "
                                  "a test this loop does not evaluate)");
    if (p.run_words < 1 || p.run_words > kKashinMaxD) return fail(UQ_E_INVALID, "kashin: run_words must be in 1..2^28");
    if (c.n > 0 && c.dim > 0 && c.D >= 2 && c.n * ((c.D + p.run_words - 1) / p.run_words) > kKashinMaxGrid)
        return fail(UQ_E_INVALID, "kashin: too many runs for one call");
    return UQ_OK;
}

// AS:212-239 into c (at w.c_off); iters [n]: the forward transforms each client ran
int kashin_coefficients(const KashinCall& k, const KashinParams& p, const float* x, int32_t* iters) {
    hipStream_t st = (hipStream_t)k.stream;
    const int64_t n = k.n, dim = k.dim, D = k.D;
    float *r = k.at<float>(k.w.r_off), *A = k.at<float>(k.w.a_off), *B = k.at<float>(k.w.b_off), *c = k.at<float>(k.w.c_off);
    float *nrm = k.at<float>(k.w.nrm_off), *num = nrm + n, *den = num + n, *M = k.at<float>(k.w.M_off);
    int32_t* done = k.at<int32_t>(k.w.done_off);
    int rc;
    kashin_pad_kernel<<<k.egrid(D), dim3(kKeT), 0, st>>>(x, r, c, dim, D);
    if ((rc = launched("kashin_pad_kernel launch"))) return rc;
    KashinNormJobs jobs{};
    jobs.job[0] = KashinNormJob{x, dim, nullptr, 0, nrm};
    kashin_norm_kernel<<<dim3((unsigned)n), dim3(kKnThreads), 0, st>>>(jobs, 1, dim, nullptr);
    if ((rc = launched("kashin_norm_kernel launch"))) return rc;
    const float sd = (float)std::sqrt(p.delta * (double)D);        // np.sqrt(delta * D) -> the f32 operand
    kashin_start_kernel<<<k.cgrid(), dim3(kKeT), 0, st>>>(nrm, sd, p.niters, n, M, done, iters);
    if ((rc = launched("kashin_start_kernel launch"))) return rc;
    for (int32_t i = 0; i < p.niters; ++i) {
        float* b = nullptr;
        if ((rc = rht_forward_rows(r, A, B, n, D, k.signs, k.sign_row, &b, st))) return rc;      // AS:222-224
        float* other = b == A ? B : A;
        kashin_clamp_kernel<<<k.egrid(D), dim3(kKeT), 0, st>>>(b, c, M, done, D);               // AS:227-228
        if ((rc = launched("kashin_clamp_kernel launch"))) return rc;
        if (i + 1 >= p.niters) break;            // the last iteration's test changes nothing
        if ((rc = rht_inverse(b, other, n, D, dim, k.signs, k.sign_row, st))) return rc;        // AS:231
        kashin_resid_kernel<<<k.egrid(dim), dim3(kKeT), 0, st>>>(r, other, M, done, (float)p.eta, D, dim);
        if ((rc = launched("kashin_resid_kernel launch"))) return rc;
        if (i == 0) continue;                    // err is num / num there: 1.0 or NaN, never below a bound <= 1 (kashin_check_params)
        // AS:235-237: H(c.clone()) * diag, the two norms side by side in one chain wave, the exit test
        if ((rc = hip_check(hipMemcpyAsync(A, c, (size_t)n * D * sizeof(float), hipMemcpyDeviceToDevice, st), "copy c")))
            return rc;
        if ((rc = rht_inverse(A, B, n, D, dim, k.signs, k.sign_row, st))) return rc;
        jobs.job[0] = KashinNormJob{x, dim, B, dim, num};
        jobs.job[1] = KashinNormJob{r, D, nullptr, 0, den};
        kashin_norm_kernel<<<dim3((unsigned)n), dim3(kKnThreads), 0, st>>>(jobs, 2, dim, done);
        if ((rc = launched("kashin_norm_kernel launch"))) return rc;
        kashin_exit_kernel<<<k.cgrid(), dim3(kKeT), 0, st>>>(num, den, (float)p.err, i + 1, n, done, iters);
        if ((rc = launched("kashin_exit_kernel launch"))) return rc;
    }
    return UQ_OK;
}

// AS:67-82 of c: min, max and step, then the runs' walks (DEQ: AS:91 fused, into `outp` f32 [n][D])
template <bool DEQ>
int kashin_sq(const KashinCall& k, const KashinParams& p, void* outp, float* mn, float* step, int32_t* info) {
    hipStream_t st = (hipStream_t)k.stream;
    const int64_t n = k.n, D = k.D;
    const float* c = k.at<float>(k.w.c_off);
    float4* part = k.at<float4>(k.w.part_off);
    int rc;
    scalar_minmax_kernel<<<dim3((unsigned)(n * k.w.parts)), dim3(kQBlock), 0, st>>>(c, D, k.w.parts, part);
    if ((rc = launched("scalar_minmax_kernel launch"))) return rc;
    kashin_fold_kernel<<<k.cgrid(), dim3(kKeT), 0, st>>>(part, k.w.parts, (float)(p.nlevels - 1), n, mn, step, info);
    if ((rc = launched("kashin_fold_kernel launch"))) return rc;
    const int64_t R = (D + p.run_words - 1) / p.run_words;
    const dim3 grid((unsigned)((n * R + kRwWavesPerWG - 1) / kRwWavesPerWG));
    kashin_sq_kernel<DEQ><<<grid, dim3(64 * kRwWavesPerWG), 0, st>>>(c, D, mn, step, p.runs, p.run_row, R, p.run_words, n,
                                                                     outp, info);
    return launched("kashin_sq_kernel launch");
}

}  // namespace

extern "C" {

int uq_kashin_padded_dim(int64_t dim, int64_t* D_out) {
    if (!D_out) return fail(UQ_E_INVALID, "null D_out");
    if (dim < 0 || dim > kKashinMaxD / 2) return fail(UQ_E_INVALID, "uq_kashin_padded_dim: dim must be in 0..2^27");
    int64_t D = 2 * dim;                                           // AS:209: a power of two doubles
    if (dim & (dim - 1)) {
        D = 1;
        while (D < dim) D <<= 1;
        if ((double)dim / (double)D > 0.85) D *= 2;                // AS:206 pad_threshold, in doubles
    }
    *D_out = D;
    return UQ_OK;
}

int uq_kashin_workspace_bytes(int64_t n, int64_t D, size_t* bytes_out) {
    if (!bytes_out) return fail(UQ_E_INVALID, "null bytes_out");
    if (n < 0 || D < 0) return fail(UQ_E_INVALID, "n and D must be >= 0");
    if (D > kKashinMaxD) return fail(UQ_E_INVALID, "D above 2^28");
    *bytes_out = kashin_layout(n, D).total;
    return UQ_OK;
}

int uq_kashin_compress_f32(const float* x, int64_t n, int64_t dim, int64_t D, int32_t niters, double eta, double delta,
                           double err, int32_t nlevels, const int8_t* signs, const int32_t* sign_row,
                           const uint32_t* runs, const int32_t* run_row, int64_t run_words, uint8_t* bins, float* mn,
                           float* step, int32_t* info, int32_t* iters, void* ws, size_t ws_bytes, void* stream) {
    KashinCall k{n, dim, D, signs, sign_row, ws, ws_bytes, stream};
    const KashinParams p{niters, eta, delta, err, nlevels, runs, run_row, run_words};
    if (int rc = kashin_check_params(k, p)) return rc;
    bool run;
    if (int rc = kashin_check(k, !x || !runs || !bins || !mn || !step || !info || !iters, &run)) return rc;
    if (!run) return UQ_OK;
    if (int rc = kashin_coefficients(k, p, x, iters)) return rc;
    return kashin_sq<false>(k, p, bins, mn, step, info);
}

int uq_kashin_decompress_f32(const uint8_t* bins, const float* mn, const float* step, int64_t n, int64_t dim, int64_t D,
                             const int8_t* signs, const int32_t* sign_row, float* out, void* ws, size_t ws_bytes,
                             void* stream) {
    KashinCall k{n, dim, D, signs, sign_row, ws, ws_bytes, stream};
    bool run;
    if (int rc = kashin_check(k, !bins || !mn || !step || !out, &run)) return rc;
    if (!run) return UQ_OK;
    hipStream_t st = (hipStream_t)stream;
    float* A = k.at<float>(k.w.a_off);
    kashin_deq_kernel<<<k.egrid(D), dim3(kKeT), 0, st>>>(bins, mn, step, A, D);
    if (int rc = launched("kashin_deq_kernel launch")) return rc;
    return rht_inverse(A, out, n, D, dim, signs, sign_row, st);                                   // AS:274
}

int uq_kashin_f32(const float* x, float* out, int64_t n, int64_t dim, int64_t D, int32_t niters, double eta, double delta,
                  double err, int32_t nlevels, const int8_t* signs, const int32_t* sign_row, const uint32_t* runs,
                  const int32_t* run_row, int64_t run_words, float* mn, float* step, int32_t* info, int32_t* iters,
                  void* ws, size_t ws_bytes, void* stream) {
    KashinCall k{n, dim, D, signs, sign_row, ws, ws_bytes, stream};
    const KashinParams p{niters, eta, delta, err, nlevels, runs, run_row, run_words};
    if (int rc = kashin_check_params(k, p)) return rc;
    bool run;
    if (int rc = kashin_check(k, !x || !out || !runs || !info, &run)) return rc;
    if (!run) return UQ_OK;
    if (int rc = kashin_coefficients(k, p, x, iters ? iters : k.at<int32_t>(k.w.iters_off))) return rc;
    float* A = k.at<float>(k.w.a_off);
    if (int rc = kashin_sq<true>(k, p, A, mn ? mn : k.at<float>(k.w.mn_off), step ? step : k.at<float>(k.w.step_off), info))
        return rc;
    return rht_inverse(A, out, n, D, dim, signs, sign_row, (hipStream_t)stream);
}

}  // extern "C"
