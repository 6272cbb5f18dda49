/* uq_dme.h — C-ABI of the MI355X-native unbiased L1-ball type quantizer.
 *
 * The reference (Ritesh622/Unbiased-Quantization-Distributed-Mean-Estimation) is pure
 * Python/PyTorch and has no FFI; every entry point below replaces one group of torch
 * ops inside `Type_unbiased_quantize` (NMSE_Results/Codes/All_Schemes.py:609-641) or
 * the DME client-mean around it (NMSE_Results/Codes/Normal_dist.py:137-138).  The
 * Python binding that calls these through ctypes is the drop-in; INTEGRATION.md shows
 * the binding a maintainer of the reference would add.
 *
 * Conventions
 *   - All buffers are DEVICE pointers, caller-allocated, row-major [n][d] f32 for
 *     client vectors.  `stream` is a hipStream_t passed as void* (NULL = default stream).
 *   - The library never allocates, never synchronises, and is stream-ordered.
 *   - Return 0 on success, a negative UQ_E* code on error; uq_last_error() gives a
 *     thread-local message.  Launch errors are reported; kernel-side protocol
 *     timeouts are reported by uq_check_status() after the stream is synchronised.
 *   - No hidden RNG: the per-client uniform X of AS:634 is an input.
 *   - m (lattice sum, AS:622-623) is passed explicitly; uq_rate_to_m() reproduces the
 *     reference's rate table for callers that want it.
 *   - torch_threads selects the f32 summation order of torch CPU `sum` (AS:624) for a
 *     given intra-op thread count, so results are bit-identical to the CPU reference
 *     run with that many threads.
 */
#ifndef UQ_DME_H
#define UQ_DME_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UQ_OK 0
#define UQ_E_INVALID (-1)   /* bad argument */
#define UQ_E_HIP (-2)       /* HIP runtime error */
#define UQ_E_WORKSPACE (-3) /* workspace too small */
#define UQ_E_TIMEOUT (-4)   /* inter-workgroup protocol timed out (see uq_check_status) */

/* Library ABI version (major*100 + minor). */
int uq_version(void);
/* SHA-256 (hex) of the sources and flags the library was built from (build_ext.build_id()). */
const char* uq_build_id(void);
/* Test hook, process-wide: on != 0 makes every later torch-tie replay (biased quantizer,
 * UQ_TIES_TORCH) take its failure path, so the defined fallback (lowest-index order plus the
 * internal-error status) can be tested.  Returns the previous setting.  Never set by the
 * library; production callers leave it at 0. */
int uq_test_force_replay_failure(int on);
/* Test hooks of the QUIC-FL kernels, process-wide (never set by the library): bit 0 makes the
 * runs of the few-message team kernels (sender KQ1t, receiver KQ2t) skip their waits and report
 * UQ_QFL_TIMEOUT, so the callers' timeout handling can be tested (the sender then takes KQ1t);
 * bit 1 sends every call to the one-wave-per-message kernels (KQ1 / KQ2); bit 2 sends the
 * sender's few-message calls to the team kernel KQ1t instead of the jump path (KQ0j + KQ1j), so
 * the forms can be compared on the same message.  Returns the previous flags. */
int uq_test_set_quicfl_hooks(int flags);
/* Test hooks of the QUIC-FL dispatch (each sender or receiver call computes one plan and launches
 * what it names; DESIGN.md 4.4 has the table).  A plan is UQ_QFL_PLAN_FIELDS int64 values, of
 * which min(cap, UQ_QFL_PLAN_FIELDS) are written:
 *   [0] form (UQ_QFL_FORM_*)   jump form: [1] R runs per message of [2] L rounds, [3] two run
 *   waves per SIMD (more than 1024 run waves); else 0   [4] force_timeout (hook bit 0)
 *   [5] the sender's work on the side stream (UQ_QFL_SIDE_*: nothing, KQ1a, KQ0s + KQ0j + KQ1ar)
 * uq_test_quicfl_plan: host only, launches nothing: the plan of side (UQ_QFL_SENDER /
 * UQ_QFL_RECEIVER) for n messages of D (padded) coordinates under `hooks`, with (has_ws != 0) or
 * without a workspace of the size the side's *_workspace_bytes gives (the sender's entry points
 * refuse a call without one).  Form 0 for n == 0 or D == 0.
 * uq_test_last_quicfl_plan: the plan of this thread's last call of that side (form 0 when it
 * launched nothing). */
#define UQ_QFL_PLAN_FIELDS 6
#define UQ_QFL_SENDER 0
#define UQ_QFL_RECEIVER 1
#define UQ_QFL_FORM_NONE 0
#define UQ_QFL_FORM_ONE_WAVE 1
#define UQ_QFL_FORM_TEAM 2
#define UQ_QFL_FORM_JUMP 3
#define UQ_QFL_SIDE_NONE 0
#define UQ_QFL_SIDE_PASS_A 1
#define UQ_QFL_SIDE_JUMP 2
int uq_test_quicfl_plan(int32_t side, int64_t n, int64_t D, int32_t hooks, int32_t has_ws, int64_t* plan_out,
                        int32_t cap);
int uq_test_last_quicfl_plan(int32_t side, int64_t* plan_out, int32_t cap);
/* Test hooks of the unbiased quantizer's dispatch (every uq_type_unbiased_* entry point runs one
 * dispatcher, and the dispatcher launches what its plan names).
 * A plan is UQ_PLAN_FIELDS int64 values, of which min(cap, UQ_PLAN_FIELDS) are written:
 *   [0] form (UQ_FORM_*)   [1] V: float4 lanes for x and q   [2] Q: q written   [3] C: codes written
 *   [4] CV: 16-byte code rows   [5] l1 supplied by the caller   [6] chunks of at most 65535 clients
 *   of the last chunk: [7] clients   [8] prefixed (the approximate-prefix launch)   [9] tiles per
 *   segment   [10] segments per client
 *   [11] tiles per client   byte offsets in the workspace of [12] the u64 [n][tiles] array that
 *   holds the fold's exact tile starts P_t after a segments / phased call, [13] map0, [14] map1,
 *   [15] the irregular tiles' records ([min(n, [19])][[18]] of [17] bytes, the event count in the
 *   first 32-bit word), [16] their u32 counters (the last chunk's, one per client)
 *   [17] sizeof(TileRec)   [18] records per client   [19] clients with records   [20] events per
 *   record   [21] events the fold prefetches
 * uq_test_unbiased_plan: host only, the plan of a call of that shape (alignment and presence of
 * the pointers as flags; slots = resident stream workgroups, 0 asks the current device when the
 * plan needs it); UQ_E_INVALID where the call would be refused for its shape.
 * uq_test_last_unbiased_plan: the plan of this thread's last unbiased call (form 0 when it
 * launched nothing). */
#define UQ_PLAN_FIELDS 22
#define UQ_FORM_NONE 0
#define UQ_FORM_SMALL 1
#define UQ_FORM_STREAM 2
#define UQ_FORM_STREAM_NIBBLES 3
#define UQ_FORM_SEGMENTS 4
#define UQ_FORM_PHASED 5
int uq_test_unbiased_plan(int64_t n, int64_t d, int64_t ldq, int64_t ldc, int32_t x_aligned, int32_t out_aligned,
                          int32_t codes_aligned, int32_t has_out, int32_t has_codes, int32_t nib, int32_t l1_given,
                          int32_t slots, int64_t* plan_out, int32_t cap);
int uq_test_last_unbiased_plan(int64_t* plan_out, int32_t cap);
/* Test hooks of the biased quantizer's dispatch (uq_type_biased_f32 computes one plan from n, d,
 * tie_policy and the alignment of x and out, and launches what it names; DESIGN.md 4.2 has the
 * table).  A plan is UQ_BIASED_PLAN_FIELDS int64 values, of which min(cap, UQ_BIASED_PLAN_FIELDS)
 * are written:
 *   [0] front (UQ_BIASED_FRONT_*)   [1] tie mode (UQ_BIASED_TIES_*; for the small-checked front:
 *   the mode the call takes when a row is ambiguous)   [2] replay form (UQ_BIASED_REPLAY_*)
 *   KB7a's levels (0 without them): [3] levels, [4] of which before KB6 starts, [5] workgroups
 *   per level launch   [6] S: replay slots, min(n, 256)   [7] vec4: 16-byte accesses to x and out
 *   (in a codes call also 4-byte ones to the codes rows)
 *   [8] cand_multi: the candidate digits over [9] cspans workgroups per client   [10] cap: u32 of
 *   the candidate region per client   [11] capf = cap / 2: listed pairs per client at most
 *   [12] output tiles per client   [13] clear_bits: the tie bits are cleared by a memset
 *   [14] outcome, known after the host check of the small-checked front and the checked tie mode:
 *   1 when the multi-kernel path / the replay chain ran, 0 when it was skipped; -1 in every
 *   other mode and from uq_test_biased_plan.
 * uq_test_biased_plan: host only, launches nothing: the plan of a call of that shape and policy
 * (alignment as flags), with uq_type_biased_f32's own checks of n, d and tie_policy.  Front 0
 * for n == 0 or d == 0.
 * uq_test_last_biased_plan: the plan of this thread's last uq_type_biased_f32 or
 * uq_type_biased_codes_f32 call (front 0
 * when it launched nothing). */
#define UQ_BIASED_PLAN_FIELDS 15
#define UQ_BIASED_FRONT_NONE 0
#define UQ_BIASED_FRONT_SMALL 1         /* KB-small alone (lowest-index rule) */
#define UQ_BIASED_FRONT_SMALL_CHECKED 2 /* KB-small, then the multi-kernel path if a row is ambiguous */
#define UQ_BIASED_FRONT_FULL 3          /* the multi-kernel path */
#define UQ_BIASED_TIES_LOWEST 0         /* lowest-index rule: no replay */
#define UQ_BIASED_TIES_FORK 1           /* torch ties, the replay on the side stream beside KB6 */
#define UQ_BIASED_TIES_CHECKED 2        /* torch ties, one stream, the replay skipped when no row is listed */
#define UQ_BIASED_REPLAY_NONE 0
#define UQ_BIASED_REPLAY_ONE_KERNEL 1
#define UQ_BIASED_REPLAY_LEVELS 2
int uq_test_biased_plan(int64_t n, int64_t d, int32_t tie_policy, int32_t x_aligned, int32_t out_aligned,
                        int64_t* plan_out, int32_t cap);
int uq_test_last_biased_plan(int64_t* plan_out, int32_t cap);
/* Test hooks of the EDEN / RHT dispatch (every uq_eden_* and uq_rht_f32 call, and QUIC-FL's RHT
 * front and inverse, computes one plan per op and launches what it names; DESIGN.md 4.3 has the
 * table).  A plan is UQ_EDEN_PLAN_FIELDS int64 values, of which min(cap, UQ_EDEN_PLAN_FIELDS) are
 * written:
 *   [0] D: dim padded to a power of two (the norm op: dim itself)   [1] p: D <= 2^p
 *   [2] norm form (UQ_EDEN_NORM_*)   [3] dot form (UQ_EDEN_DOT_*)   [4] bits of the first FWHT pass
 *   [5] FWHT passes, then for each of UQ_EDEN_MAX_PASSES passes (0 past [5]): [6 + 4 i] lo, its
 *   lowest index bit   [7 + 4 i] k, its bits   [8 + 4 i] kernel (UQ_EDEN_PASS_*)   [9 + 4 i]
 *   workgroups per client (grid x; grid y is n)
 *   [22] the forward RHT copies its result from the workspace into out   [23] tables per client
 *   of the segmented norm (0 where the shape has no segmented region)
 *   [24] 1 for a fractional rate (the uq_eden_*_frac_f32 entry points): the forms above name the
 *   mask-aware instances of KE4 / KE4s and of the receiver's first pass
 * uq_test_eden_plan: host only, launches nothing: the plan of op (UQ_EDEN_OP_*) for n clients of
 * dim coordinates; nbits matters to compress and decompress (1, 2, or UQ_EDEN_NBITS_FRAC for
 * 1 < nbits < 2, which takes the rows of 2 bits), mode (uq_eden_norm_f32's) to the norm op,
 * whose norm form is 0 when mode 2 is asked for a shape the segmented norm does not take.  No
 * forms and no passes for n == 0 or dim == 0.
 * uq_test_last_eden_plan: the plan of this thread's last call of that op (no passes and no forms
 * when it launched nothing); a uq_eden_f32 call records a compress and a decompress plan. */
#define UQ_EDEN_PLAN_FIELDS 25
#define UQ_EDEN_NBITS_FRAC 12           /* the plan hook's nbits for a fractional rate, 1 < nbits < 2 */
#define UQ_EDEN_MAX_PASSES 4            /* three up to D = 2^28 (12 + 8 + 8), the quantizers' limit */
#define UQ_EDEN_OP_COMPRESS 0
#define UQ_EDEN_OP_DECOMPRESS 1
#define UQ_EDEN_OP_RHT_FORWARD 2
#define UQ_EDEN_OP_RHT_INVERSE 3        /* uq_rht_f32's inverse: first pass 12 bits whatever D */
#define UQ_EDEN_OP_NORM 4
#define UQ_EDEN_OP_QFL_FRONT 5          /* QUIC-FL's sender: RHT + norm */
#define UQ_EDEN_OP_QFL_INVERSE 6        /* uq_quicfl_quantize_f32's inverse RHT */
#define UQ_EDEN_OPS 7
#define UQ_EDEN_NORM_NONE 0
#define UQ_EDEN_NORM_CHAINS_WHOLE 1     /* KE2, D a multiple of its 2048-float chunk */
#define UQ_EDEN_NORM_CHAINS_GENERIC 2   /* KE2, any D */
#define UQ_EDEN_NORM_SEGMENTED 3        /* KE2a-KE2d */
#define UQ_EDEN_NORM_FUSED 4            /* KE2+4: norm, bins and dot in one read */
#define UQ_EDEN_DOT_NONE 0
#define UQ_EDEN_DOT_ONE_WAVE 1          /* KE4 */
#define UQ_EDEN_DOT_SEGMENTED 2         /* KE4s */
#define UQ_EDEN_DOT_FUSED_REDO 3        /* KE2+4, then KE4 for the clients it flags */
#define UQ_EDEN_PASS_LOW16K 1
#define UQ_EDEN_PASS_LOW4096 2
#define UQ_EDEN_PASS_HIGH256 3
#define UQ_EDEN_PASS_SMALL 4
#define UQ_EDEN_PASS_GENERIC 5
int uq_test_eden_plan(int32_t op, int64_t n, int64_t dim, int32_t nbits, int32_t mode, int64_t* plan_out, int32_t cap);
int uq_test_last_eden_plan(int32_t op, int64_t* plan_out, int32_t cap);
/* Test hooks of the packed message form (uq_eden_compress_packed_f32 / uq_eden_decompress_packed_f32): beside
 * the EDEN plan above, which such a call records as the u8 call of the same shape does, a packed call names
 * which kernel writes (compress) or first reads (decompress) the payload rows.  UQ_EDEN_PACKED_PLAN_FIELDS
 * int64 values, of which min(cap, UQ_EDEN_PACKED_PLAN_FIELDS) are written:
 *   [0] kind (1, 2, UQ_EDEN_NBITS_FRAC; 0: the op's last call was not a packed one or launched nothing)
 *   [1] form: UQ_EDEN_PACKED_FUSED (KE4 / KE2+4 and its redo KE4 write payload words; the 4096-element first
 *       pass reads them) or UQ_EDEN_PACKED_CONVERTER (u8 bins in the workspace and uq_eden_pack_bins' /
 *       uq_eden_unpack_bins' kernel: the segmented dot, the 16k / generic first passes, every fractional rate)
 *   [2] P = ceil(D / 32), the words of a plane   [3] the row pitch in words
 * uq_test_eden_packed_plan: host only (op: UQ_EDEN_OP_COMPRESS or UQ_EDEN_OP_DECOMPRESS), under the current
 * hooks; uq_test_last_eden_packed_plan: of this thread's last call of that op.
 * uq_test_set_eden_hooks: process-wide; bit 0 sends every packed call through the u8 bins and the converter,
 * so that the fused and the fallback form can be compared on the same input.  Returns the previous flags. */
#define UQ_EDEN_PACKED_PLAN_FIELDS 4
#define UQ_EDEN_PACKED_NONE 0
#define UQ_EDEN_PACKED_FUSED 1
#define UQ_EDEN_PACKED_CONVERTER 2
int uq_test_set_eden_hooks(int flags);
int uq_test_eden_packed_plan(int32_t op, int64_t n, int64_t dim, int32_t kind, int64_t* plan_out, int32_t cap);
int uq_test_last_eden_packed_plan(int32_t op, int64_t* plan_out, int32_t cap);
/* Host-only, for tests and tools: the MT19937 state (ATen's 624-word array, block-aligned) that
 * `blocks` twists ahead of state624, computed the way the QUIC-FL sender's jump path does it
 * (t^(624 (blocks - 1)) mod phi, phi from Berlekamp-Massey; the correlation with the stream's
 * first 19937 + 623 words; one twist) -- see uq_mt_poly.cpp.  Replaces nothing in the
 * reference: its generators (All_Schemes.py:457, 465, 484, 489) are walked word by word. */
int uq_mt_jump_host(const uint32_t* state624, int64_t blocks, uint32_t* out624);

/* Host-only: the NMSE drivers' input vectors, bit-identical to numpy's legacy RandomState and
 * multi-threaded (uq_legacy_rng.cpp).  Replaces the per-vector draws of
 * NMSE_Results/Codes/Normal_dist.py:88-91 (np.random.normal(0, 1, size=d)), Laplace_dist.py:89,
 * Gamma_dist.py:86, Bernoulli_dist.py:90 (choice(arange(2), p)) and Lognormal_dist.py:90:
 * n successive size-d calls on the state (key624, pos, has_gauss, gauss) -- numpy's
 * get_state() tuple, advanced in place -- into out [n][d] as f32 (the drivers' cast to a f32
 * tensor), and norm2[i] = np.linalg.norm(v_i) ** 2 summed in f64 in a fixed order.
 * dist / (a, b): 0 normal (loc, scale), 1 laplace (loc, scale), 2 gamma (shape > 1, scale),
 * 3 choice of {0, 1} (the normalised cdf), 4 lognormal (mean, sigma), 5 uniform (low,
 * high - low).  threads: host threads (1 = sequential).  Returns 0, -1 bad arguments, -2 jump
 * unavailable, -3 internal inconsistency.  Does not set uq_last_error. */
int uq_legacy_draw_f32(uint32_t* key624, int32_t* pos, int32_t* has_gauss, double* gauss, int32_t dist,
                       double a, double b, int64_t n, int64_t d, float* out, double* norm2, int32_t threads);
/* Test hook: set the parallel draw's chunking (words per chunk, words of overlap; 0 keeps) and
 * read-and-reset its counters (waves run, chunk meetings missed). */
int uq_legacy_test_params(int64_t min_chunk, int64_t overlap, int64_t* waves, int64_t* misses);

/* Thread-local description of the last error returned on this thread. */
const char* uq_last_error(void);

/* AS:614-623: m = int(table[bits] * d).  Unknown `bits` -> UQ_E_INVALID (the
 * reference raises KeyError). */
int uq_rate_to_m(double bits_per_dimension, int64_t d, int64_t* m_out);

/* Bytes of device workspace needed by the calls below for a batch of n vectors of
 * length d summed in torch order for `torch_threads`.  The workspace also holds the
 * status word read by uq_check_status().  A workspace must be zero-filled once before
 * its first use (later calls re-initialise what they need themselves). */
int uq_workspace_bytes(int64_t n, int64_t d, int32_t torch_threads, size_t* bytes_out);

/* AS:624 — l1_out[j] = sum_i |x[j][i]| in torch CPU cascade order (f32 accumulate). */
int uq_l1_torch_order_f32(const float* x, int64_t n, int64_t d, int32_t torch_threads,
                          float* l1_out, void* ws, size_t ws_bytes, void* stream);

/* AS:609-641 for a batch — out[j] = Type_unbiased_quantize(x[j], ·) with uniform X[j].
 *   m       lattice sum (AS:623)
 *   X       [n] device f32, the AS:634 draw per client
 *   l1      [n] device f32 L1 norms, or NULL to compute them here (torch order)
 *   l1_out  [n] device f32 or NULL: receives the L1 norms used */
int uq_type_unbiased_f32(const float* x, float* out, int64_t n, int64_t d, int64_t m,
                         const float* X, const float* l1, float* l1_out,
                         int32_t torch_threads, void* ws, size_t ws_bytes, void* stream);

/* AS:609-641 for ONE vector per call, the form the reference's callers use (Normal_dist.py:137,
 * Type_unbiased.py:160): out = Type_unbiased_quantize(x, ·) with the AS:634 draw X passed by
 * value (no device copy of it), L1 computed here (torch order).  Same bits as
 * uq_type_unbiased_f32 with n = 1. */
int uq_type_unbiased_vec_f32(const float* x, float* out, int64_t d, int64_t m, float X, int32_t torch_threads,
                             void* ws, size_t ws_bytes, void* stream);

/* Normal_dist.py:137-138 — est[i] (+)= q[j][i] / n_div for j = 0..n-1 in client order
 * (f32 IEEE division, f32 add).  Row j starts at q + j*ld (ld >= d, so a column block
 * of a wider batch can be folded in).  accumulate=0 starts from zeros; accumulate=1
 * continues from `est`, which makes the sum over a sequence of calls bit-identical
 * to one call over all rows in the same order. */
int uq_client_mean_f32(const float* q, int64_t n, int64_t d, int64_t ld, float n_div,
                       int32_t accumulate, float* est, void* stream);

/* Quantize a batch and fold it into the client mean in one call:
 *   q = Type_unbiased_quantize(x[j]) for all j (into `out`, which must be non-NULL),
 *   then est (+)= q[j] / n_div in client order.  Bit-identical to the two calls above. */
int uq_type_unbiased_mean_f32(const float* x, float* out, int64_t n, int64_t d, int64_t m,
                              const float* X, const float* l1, int32_t torch_threads,
                              float n_div, int32_t accumulate, float* est,
                              void* ws, size_t ws_bytes, void* stream);

/* Type codes (wire format; see unbiased-quantization-distributed-mean-estimation_amd/codes.py).
 * Per coordinate one int8: k = fl + r (the lattice count, 0..127) for sign(v) >= 0 and
 * -k-1 for sign(v) < 0.  With the client's L1 and m, q is rebuilt bit-for-bit:
 * q = +-RN(RN(L1*k)/f32(m)).  kmax[j] = the client's largest count; 128 means some count
 * exceeded 127 and saturated (overflow: send that client as floats).
 *
 * uq_type_unbiased_codes_f32: as uq_type_unbiased_f32, writing q (out, may be NULL)
 * and/or codes [n][d] int8 (may be NULL; then kmax may be NULL too).  kmax [n] int32 is
 * zeroed by the call. */
int uq_type_unbiased_codes_f32(const float* x, float* out, int8_t* codes, int32_t* kmax,
                               int64_t n, int64_t d, int64_t m, const float* X, const float* l1,
                               float* l1_out, int32_t torch_threads, void* ws, size_t ws_bytes,
                               void* stream);

/* As uq_type_unbiased_codes_f32 with row pitches: q row j at out + j*ldq (floats, ldq >= d),
 * codes row j at codes + j*ldc (bytes, ldc >= d), e.g. rows of wider caller buffers.  Same
 * bits as the dense call; nothing is written between rows. */
int uq_type_unbiased_codes_ld_f32(const float* x, float* out, int64_t ldq, int8_t* codes, int64_t ldc,
                                  int32_t* kmax, int64_t n, int64_t d, int64_t m, const float* X,
                                  const float* l1, float* l1_out, int32_t torch_threads, void* ws,
                                  size_t ws_bytes, void* stream);

/* 4-bit type codes (the bench pipeline "codes4"): as uq_type_unbiased_codes_ld_f32 writing q
 * (required) and the codes as 4-bit fields, two per byte (element 2i in the low nibble of byte
 * i of row j at nib + j*ldn, ldn >= d/2 bytes): the low nibble of the int8 code, i.e. k for
 * sign >= 0 and 15-k for -k-1, exact while k <= 7.  kmax as for the int8 codes (the largest
 * count, 128 above 127); a client with kmax > 7 is read from q by uq_nibbles_q_mean_ld_f32.
 * Stream form only: n >= 256, d % 4096 == 0, d <= 2^29, 16-byte aligned rows (UQ_E_INVALID
 * otherwise).  Internal format between K2 and the mean; no wire format (the UQR1 codec takes
 * the int8 codes). */
int uq_type_unbiased_nibbles_ld_f32(const float* x, float* out, int64_t ldq, uint8_t* nib, int64_t ldn,
                                    int32_t* kmax, int64_t n, int64_t d, int64_t m, const float* X,
                                    const float* l1, float* l1_out, int32_t torch_threads, void* ws,
                                    size_t ws_bytes, void* stream);

/* est[i] (+)= q[j][i] / n_div, clients in order, from the 4-bit codes above: bit-identical to
 * uq_client_mean_f32(q); clients with kmax[j] > 7 add q[j][i] / n_div (q required).
 * d % 4096 == 0, ldq >= d, ldn >= d/2, 16-byte aligned est and q. */
int uq_nibbles_q_mean_ld_f32(const uint8_t* nib, int64_t ldn, const float* q, int64_t ldq, const float* l1,
                             const int32_t* kmax, int64_t n, int64_t d, int64_t m, float n_div,
                             int32_t accumulate, float* est, void* stream);

/* q[j][i] = decode(codes[j][i]; l1[j], m). */
int uq_codes_decode_f32(const int8_t* codes, const float* l1, int64_t n, int64_t d, int64_t m,
                        float* out, void* stream);

/* Normal_dist.py:137-138 from codes: est[i] (+)= q[j][i] / n_div, clients in order,
 * bit-identical to uq_client_mean_f32 on the decoded batch (reads d bytes per client).
 * kmax [n] as produced by the encoder (sizes the per-client decode tables). */
int uq_codes_mean_f32(const int8_t* codes, const float* l1, const int32_t* kmax, int64_t n, int64_t d,
                      int64_t m, float n_div, int32_t accumulate, float* est, void* stream);

/* As uq_codes_mean_f32, with the dequantized batch q (row j at q + j*ldq, ldq >= d) beside
 * the codes: a client whose counts overflowed its codes (kmax[j] > 127, saturated) adds
 * q[j][i] / n_div instead, so est is always bit-identical to uq_client_mean_f32(q).
 * q == NULL is uq_codes_mean_f32 (overflowed clients then add their saturated codes).
 * Clients without overflow read only their codes. */
int uq_codes_q_mean_f32(const int8_t* codes, const float* q, int64_t ldq, const float* l1, const int32_t* kmax,
                        int64_t n, int64_t d, int64_t m, float n_div, int32_t accumulate, float* est,
                        void* stream);

/* As uq_codes_q_mean_f32 with the codes' row pitch: codes row j at codes + j*ldc (ldc >= d). */
int uq_codes_q_mean_ld_f32(const int8_t* codes, int64_t ldc, const float* q, int64_t ldq, const float* l1,
                           const int32_t* kmax, int64_t n, int64_t d, int64_t m, float n_div,
                           int32_t accumulate, float* est, void* stream);

/* The two forms of type codes (not the UQ_FORM_* plan forms above).  Both are lattice types
 * k/m with the same int8 code (k for sign > 0 or >= 0, -k-1 for sign < 0), but the dequantized
 * value groups its products differently, so each form has its own decode and mean tables:
 *   UQ_FORM_UNBIASED  |q| = RN(RN(L1*k) / f32(m))     (AS:640; uq_type_unbiased_codes_f32)
 *   UQ_FORM_BIASED    |q| = RN(L1 * RN(k / f32(m)))   (AS:687; uq_type_biased_codes_f32), m >= 1
 * uq_codes_decode_form_f32 / uq_codes_mean_form_f32: as uq_codes_decode_f32 /
 * uq_codes_q_mean_ld_f32 (q may be NULL) for codes of `form`; UQ_FORM_UNBIASED gives the bits
 * of those entries, any other value of form is UQ_E_INVALID.  With UQ_FORM_BIASED the mean is
 * bit-identical to uq_client_mean_f32 over uq_type_biased_f32's output for clients with
 * kmax[j] <= 127; a client with kmax[j] == 128 is read from q (required for such a batch). */
#define UQ_FORM_UNBIASED 0
#define UQ_FORM_BIASED 1
int uq_codes_decode_form_f32(const int8_t* codes, const float* l1, int64_t n, int64_t d, int64_t m, int32_t form,
                             float* out, void* stream);
int uq_codes_mean_form_f32(const int8_t* codes, int64_t ldc, const float* q, int64_t ldq, const float* l1,
                           const int32_t* kmax, int64_t n, int64_t d, int64_t m, int32_t form, float n_div,
                           int32_t accumulate, float* est, void* stream);

/* ---- type messages "UQR1": entropy-coded type codes ---------------
 * The reference has no wire format (parity unpinned); its client output is AS:640's
 * dequantized vector, fully described by (L1, m, signed counts k) = the int8 codes above.
 * One message per client: rANS over symbols s = 2k + neg with a per-client static model
 * (frequencies quantized to 2^12), 32-bit states, 16-bit words, W = min(64, ceil(d/1024))
 * interleaved states per chunk of W*1024 symbols, so ~R bits per coordinate at rate R.
 * flags bit 0 (UQ_TC_EXACT_ZERO_SIGNS): keep the sign of zero counts (neg for k = 0), so
 * the decoded q is bit-identical to AS:640 (-0.0 included); without it the sign of a zero
 * count is dropped and q is value-identical (+0.0 where the reference has -0.0), at ~R bits.
 * flags bit 1 (UQ_TC_BIASED_FORM): the codes are of UQ_FORM_BIASED; the bit is written into the
 * header's flags half-word (byte 6) beside bit 0 and changes nothing else of the message: the
 * coder does not depend on it and uq_tc_decode accepts either value (the receiver reads the
 * form from the header).  Messages without it are byte for byte what they have always been.
 * Byte layout: oracle/uq_codec.c (the CPU restatement the tests compare against).
 *
 * uq_tc_bound: the largest message of a client of length d (bytes).
 * uq_tc_encode: codes [n][d] int8, l1 [n] f32 (device) -> messages packed back to back in
 *   msgs (device, msgs_bytes >= n * bound), offsets [n+1] u64 (device): client j's message is
 *   msgs[offsets[j] .. offsets[j+1]).  Workspace: uq_tc_workspace_bytes (no zero-fill needed).
 * uq_tc_decode: messages (device buffer of msgs_bytes, offsets [n+1]) -> codes [n][d], l1 [n],
 *   kmax [n]; status [n] int32 (device) is 0 for a well-formed message, else bit 0 bad header,
 *   d mismatch or offsets outside [0, msgs_bytes] / not increasing / unaligned (nothing is read
 *   outside the buffer), bit 1 bad frequency table, bit 2 word stream overrun or underrun,
 *   bit 3 wrong final state, bit 4 the header's m differs from `m` (m < 0: any m). */
#define UQ_TC_EXACT_ZERO_SIGNS 1
#define UQ_TC_BIASED_FORM 2
int uq_tc_bound(int64_t d, size_t* bytes_out);
int uq_tc_workspace_bytes(int64_t n, int64_t d, size_t* bytes_out);
int uq_tc_encode(const int8_t* codes, const float* l1, int64_t n, int64_t d, int64_t m, int32_t flags,
                 uint8_t* msgs, size_t msgs_bytes, uint64_t* offsets, void* ws, size_t ws_bytes, void* stream);
int uq_tc_decode(const uint8_t* msgs, size_t msgs_bytes, const uint64_t* offsets, int64_t n, int64_t d, int64_t m,
                 int8_t* codes, float* l1, int32_t* kmax, int32_t* status, void* stream);

/* ---- biased type quantizer (Reznik rounding) ------------------------------------------
 * NMSE_Results/Codes/All_Schemes.py:669-687 Type_biased_quantize and :644-666 Reznik for
 * a batch: out[j] = Type_biased_quantize(x[j], ·) with m = the lattice sum (AS:684).
 *   k' = floor(m p + 0.5), m' = sum k' (torch CPU order for torch_threads), Delta = int(m' - m);
 *   the |Delta| coordinates with the largest delta' = k' - m p (Delta > 0: k' -= 1) or the
 *   smallest (Delta < 0: k' += 1) are adjusted; out = (L1 * sign(x)) * (k' / m).
 * tie_policy decides which of several coordinates with the same delta' at the selection
 * threshold are taken (torch.topk compares values only):
 *   UQ_TIES_TORCH         the coordinates torch CPU's topk returns (libstdc++
 *                         nth_element / partial_sort replayed on the GPU): bit-identical
 *                         to the reference on every input
 *   UQ_TIES_LOWEST_INDEX  the lowest indices (cheaper; identical whenever no tie straddles
 *                         the threshold, i.e. info flag 1 is clear)
 * l1_out [n] f32 or NULL.  info [n][2] int32 or NULL: {Delta, flags}; flags bit0 = a tie
 * straddled the threshold, bit1 = m' not finite (the reference raises; output is NaN-laden),
 * bit2 = |Delta| > d (the reference's topk raises), bit3 = torch tie choice replayed,
 * bit4 = threshold digits 2-3 found on the compacted first-digit bucket (informational).
 * Workspace: uq_biased_workspace_bytes; zero-filled once before first use (it holds the
 * status word of uq_check_status, which reports an inconsistent tie replay).  The tests
 * exercise the replay's index-order fallback through uq_test_force_replay_failure, not
 * through the workspace: no workspace content changes which path a replay takes. */
#define UQ_TIES_TORCH 0
#define UQ_TIES_LOWEST_INDEX 1
/* OR'd into UQ_TIES_TORCH: the call synchronises `stream` once, to read the number of clients
 * whose tie choice needs the replay, and skips the replay's kernels when it is zero -- for
 * synchronous few-client callers (the per-vector drop-in); results are the same bits either
 * way. */
#define UQ_TIES_HOST_CHECK 4
int uq_biased_workspace_bytes(int64_t n, int64_t d, int32_t torch_threads, size_t* bytes_out);
int uq_type_biased_f32(const float* x, float* out, int64_t n, int64_t d, int64_t m,
                       int32_t torch_threads, int32_t tie_policy, float* l1_out, int32_t* info,
                       void* ws, size_t ws_bytes, void* stream);

/* uq_type_biased_f32 that also (out given) or only (out == NULL: no float output is written at
 * all) writes the type codes of the same k'': codes [n][d] int8 of UQ_FORM_BIASED, kmax [n] int32
 * (written by the call) and l1_out [n] (required: the codes are decoded with it).  Same tie
 * policies, host-check bit and info pairs as uq_type_biased_f32, and the same bits in out.
 * Workspace: uq_biased_codes_workspace_bytes (uq_biased_workspace_bytes plus one int32 per
 * 4096 coordinates and client, where the writers gather the largest coded count); the same
 * buffer serves both calls.  m >= 1.
 *   code = k''      for x > 0
 *   code = -k''-1   for x < 0  (a negative coordinate with k'' = 0 is -0.0 and round-trips)
 *   code = 0        for x == 0 (sign 0: the output is +0.0 whatever k'' the Delta < 0 adjustment
 *                   gave the coordinate; so the counts of the codes sum to <= m, to m when no
 *                   coordinate is zero)
 * For a client with kmax[j] <= 127, uq_codes_decode_form_f32(UQ_FORM_BIASED) of (codes, l1_out, m)
 * is out bit for bit.  kmax[j] is >= every coded count of the row and <= the largest + 1 (a
 * count written provisionally and lowered by a patch may leave it one high); it is 128 for a
 * client whose codes must not be decoded: a count above 127 at any stage (saturated to 127 in
 * the code), L1 not finite, or info flag bit 1 (m' not finite) or bit 2 (|Delta| > d).  Such
 * rows are still correct in out when out is given.
 * Errors (UQ_E_INVALID with a uq_last_error text): m < 1; codes, kmax or l1_out NULL with
 * n, d > 0.  n == 0 or d == 0 is a no-op.  16-byte accesses need x and out 16-byte aligned, the
 * codes 4-byte aligned and d % 4 == 0 (the plan's vec4; any alignment gives the same bits).
 * uq_test_last_biased_plan reports this call's plan too. */
int uq_biased_codes_workspace_bytes(int64_t n, int64_t d, int32_t torch_threads, size_t* bytes_out);
int uq_type_biased_codes_f32(const float* x, float* out, int8_t* codes, int32_t* kmax, int64_t n, int64_t d,
                             int64_t m, int32_t torch_threads, int32_t tie_policy, float* l1_out, int32_t* info,
                             void* ws, size_t ws_bytes, void* stream);

/* ---- EDEN with the randomized Hadamard transform (baseline) -------
 * NMSE_Results/Codes/All_Schemes.py:95-153 (RHT), :324-413 (EdenSender / EdenReceiver),
 * :792-811 (EDEN_quantize_Hadamard).  D = dim rounded up to a power of two.
 *
 * uq_rht_signs: the RHT diagonal of AS:117-120 for each seed: signs[r][i] = +-1 (int8) as
 *   2 * torch.bernoulli(1/2, generator seeded with seeds[r]) - 1 on torch's CPU generator
 *   (MT19937).  Callers cache rows per (seed, D); seeds is a device int32 [rows].
 * uq_eden_compress_f32: bins [n][D] u8 and scale [n] f32 of EdenSender.compress for integer
 *   nbits (1 or 2, the tables the reference defines); client j uses diagonal row
 *   sign_row[j] (device int32 [n]).  Rotation, norm (torch CPU order) and bins are
 *   bit-identical to the reference, and so is the scale: its torch.dot is summed in MKL sdot's
 *   order on the fixtures' host (oracle/uq_eden.py torch_dot).
 * uq_eden_decompress_f32: out [n][dim] = scale * RHT^-1(centroids[bins])[:dim].
 * uq_eden_f32: both (EDEN_quantize_Hadamard for a batch); scale_out [n] or NULL.
 * Workspace: uq_eden_workspace_bytes. */
int uq_rht_signs(const int32_t* seeds, int64_t rows, int64_t D, int8_t* signs, void* stream);
/* The randomized Hadamard transform itself, for a batch (workspace: uq_eden_workspace_bytes):
 *   inverse = 0: out [n][D] = H(pad(x[j], D) * diag) (HadamardSender.randomized_hadamard_transform,
 *                AS:123-141); x rows have length dim
 *   inverse = 1: out [n][D] = H(x[j]) * diag (HadamardReceiver, AS:146-153); dim must be D
 * bit-identical to the reference (f32 butterflies a + b, (a + b) - 2b; / f32(sqrt(D))).
 * (It uses only the vector part of that workspace, not the norm's tables, so a smaller
 * buffer passes the size check; uq_eden_workspace_bytes is always enough.) */
int uq_rht_f32(const float* x, float* out, int64_t n, int64_t dim, int32_t inverse, const int8_t* signs,
               const int32_t* sign_row, void* ws, size_t ws_bytes, void* stream);
/* uq_quicfl_prepare_f32: QuicFLReceiver.decompress (AS:526-532) up to its inverse RHT, for a
 * batch: out [n][D] = (exact ? exact_vals : recv_table[X * h_len + h]) / scale[j], with
 * h = torch.randint(0, h_len, (D,)) of a CPU generator seeded with prng_seeds[j] (MT19937
 * word % h_len).  X [n][D] int32 in [0, table_rows); recv_table [table_rows][h_len] f32
 * (<= 1024 entries: the reference tables <b>_X_<s>_h_256_q_recv_table.pt); exact_mask u8 [n][D] and
 * exact_vals f32 [n][D] (dense) or both NULL; scale [n] f32.  The inverse RHT is uq_rht_f32
 * (inverse = 1). */
int uq_quicfl_prepare_f32(const int32_t* X, int64_t n, int64_t D, const float* recv_table, int32_t table_rows,
                          int32_t h_len, const int32_t* prng_seeds, const uint8_t* exact_mask, const float* exact_vals,
                          const float* scale, float* out, void* stream);
/* uq_quicfl_receive_f32: the same for messages as they come (uq_quicfl_compress_f32's or the
 * reference's dict): X [n][D] int64 (x_kind 0), uint8 (1) or int32 (2), read in place; the
 * index X * h_len + h is taken like torch.take (AS:530): -numel <= index < numel, negatives
 * wrap, any other index sets UQ_QFL_BAD_INDEX in info[j] (that coordinate's output is 0; the
 * reference raises IndexError).  exact_mask u8/bool [n][D] or NULL; exact_vals f32 [n][D]
 * dense (exact_layout 0: the value at its coordinate) or compact (exact_layout 1: row j's
 * exact values in index order in its first entries, as uq_quicfl_compress_f32 writes them;
 * exact_vals rows are still D entries long).  exact_count [n] or NULL (compact only): a row
 * whose mask does not hold exactly exact_count[j] coordinates gets UQ_QFL_BAD_EXACT (the
 * reference's `vec[exact_indeces] = exact_values` raises).  info [n] int32 or NULL.
 * D <= 2^28.  uq_quicfl_prepare_f32 = x_kind 2, dense, no info. */
#define UQ_QFL_BAD_EXACT 32
int uq_quicfl_receive_f32(const void* X, int32_t x_kind, int64_t n, int64_t D, const float* recv_table,
                          int32_t table_rows, int32_t h_len, const int32_t* prng_seeds, const uint8_t* exact_mask,
                          const float* exact_vals, int32_t exact_layout, const int32_t* exact_count, const float* scale,
                          float* out, int32_t* info, void* stream);
/* uq_quicfl_receive_ws_f32: uq_quicfl_receive_f32 with a device workspace of
 * uq_quicfl_receive_workspace_bytes(n, D) bytes (0 means none is used; NULL is accepted then):
 * with it, few-message calls start every run of the h stream at once from jumped generator
 * blocks (MT19937 jump-ahead, uq_mt_poly.cpp) instead of walking the stream; same results. */
int uq_quicfl_receive_workspace_bytes(int64_t n, int64_t D, size_t* bytes_out);
int uq_quicfl_receive_ws_f32(const void* X, int32_t x_kind, int64_t n, int64_t D, const float* recv_table,
                             int32_t table_rows, int32_t h_len, const int32_t* prng_seeds, const uint8_t* exact_mask,
                             const float* exact_vals, int32_t exact_layout, const int32_t* exact_count,
                             const float* scale, float* out, int32_t* info, void* ws, size_t ws_bytes, void* stream);

/* ---- QUIC-FL sender (baseline) --------------------------------------
 * QuicFLSender.compress (NMSE_Results/Codes/All_Schemes.py:455-503) for a batch of n messages,
 * bit-identical to the reference's CPU run (tests/golden/quicfl_sender_vectors.*):
 *   rotation: the sender RHT of uq_rht_f32 (diagonal row sign_row[j] of signs [rows][D]);
 *   scale[j] = f32(1 / torch.norm(rot)) * f32(sqrt(D))       (AS:466/470, Tensor.__rtruediv__)
 *   v = rot * scale; exact = |v| > f32(norm.ppf(1 - 2^-9));   (AS:472-478)
 *   q = v / delta (0 where exact); p = q - floor(q);           (AS:480-483)
 *   h = randint(0, h_len, (D,)) and bernoulli(p) from MT19937 seeded with prng_seeds[j]
 *       (= xxh64(str(seed)) % 2^16, uq_xxh64), the D randint words first;
 *   idx = ((floor(q) + b) * h_len + h) + half_table in f32, truncated (torch.take wraps
 *       negatives), half_table = ((table_numel / h_len) - 1) * h_len / 2   (AS:443, AS:486);
 *   X = table[idx].X + bernoulli(table[idx].p) from a second generator, truncated (AS:489-490).
 * table_xp: device f32 [table_numel][2] = (sender_table_X, sender_table_p) pairs; table_packed
 *   (or NULL): the same table as u32 (X << 25) | ceil(p * 2^24), valid when every X is an integer
 *   in 0..127 and every p in [0, 1] (the caller checks): one 4-byte gather per coordinate instead
 *   of 8 -- bernoulli(p) draws low24(w) * 2^-24 < p, i.e. low24(w) < ceil(p * 2^24), the same bits.
 * The second generator (the reference's global torch generator): px_state [n][626] u32 =
 *   (left, next, state[624]) of ATen's mt19937 per message (next = 625 - left unless left = 1),
 *   or px_state = NULL and px_seeds [n] (fresh generators, manual_seed(px_seeds[j]));
 *   px_state_out [n][626] (or NULL) receives the state after the message's D draws.
 * Outputs: X [n][D] int64 (x_kind 0, the reference's X.long()) or uint8 (x_kind 1; values
 *   outside 0..255 flag UQ_QFL_X_RANGE); exact_mask [n][D] u8; exact_vals [n][D] f32 with
 *   message j's exact values compacted in index order in its first exact_count[j] entries;
 *   scale [n] f32; info [n] int32 flags: UQ_QFL_BAD_P (some p outside [0, 1]: the reference's
 *   bernoulli raises RuntimeError, e.g. an all-zero vector), UQ_QFL_BAD_INDEX (an index outside
 *   [-numel, numel): torch.take raises IndexError), UQ_QFL_BAD_PX (a table p outside [0, 1]),
 *   UQ_QFL_X_RANGE.  h_len must be 1..256; workspace: uq_quicfl_workspace_bytes. */
#define UQ_QFL_BAD_P 1
#define UQ_QFL_BAD_INDEX 2
#define UQ_QFL_BAD_PX 4
#define UQ_QFL_X_RANGE 8
#define UQ_QFL_TIMEOUT 16   /* internal: a wait of the few-message kernel ran out (never expected) */
#define UQ_QFL_STATE_WORDS 626
int uq_quicfl_workspace_bytes(int64_t n, int64_t dim, size_t* bytes_out);
int uq_quicfl_compress_f32(const float* x, int64_t n, int64_t dim, const int8_t* signs, const int32_t* sign_row,
                           const float* table_xp, const uint32_t* table_packed, int64_t table_numel, int32_t h_len,
                           float delta,
                           const int32_t* prng_seeds, const uint32_t* px_state, const int32_t* px_seeds,
                           uint32_t* px_state_out, void* X, int32_t x_kind, uint8_t* exact_mask, float* exact_vals,
                           int32_t* exact_count, float* scale, int32_t* info, void* ws, size_t ws_bytes, void* stream);
/* uq_quicfl_quantize_f32: QUICFL_quantize (All_Schemes.py:814-832) for a batch: the sender of
 * uq_quicfl_compress_f32 (same arguments, same generators, px_state_out likewise) with the
 * receiver QuicFLReceiver.decompress (AS:526-535) on each message fused into it: out[j][:dim]
 * = inverse RHT of (exact ? v : recv_table[X * h_len + h]) / scale, where h is the sender's
 * own randint stream (the receiver regenerates the same words from the same prng seed).  No
 * message is written.  recv_table: device f32 [recv_numel] (<= 1024; torch.take's flat index
 * range, negatives wrap, others flag UQ_QFL_RECV_INDEX: the reference's receiver raises
 * IndexError after its sender returned).  scale [n] (or NULL) = the messages' scales.  info as
 * uq_quicfl_compress_f32 plus UQ_QFL_RECV_INDEX.  Workspace: uq_quicfl_workspace_bytes. */
#define UQ_QFL_RECV_INDEX 64
int uq_quicfl_quantize_f32(const float* x, int64_t n, int64_t dim, const int8_t* signs, const int32_t* sign_row,
                           const float* table_xp, const uint32_t* table_packed, int64_t table_numel, int32_t h_len,
                           float delta, const float* recv_table, int32_t recv_numel, const int32_t* prng_seeds,
                           const uint32_t* px_state, const int32_t* px_seeds, uint32_t* px_state_out, float* out,
                           float* scale, int32_t* info, void* ws, size_t ws_bytes, void* stream);
/* QUIC-FL messages at their rate: X bit-packed, the exact coordinates as an index list.  These entry points
 * replace nothing of the reference, whose message dict keeps X and a mask (AS:494-503).  D: the padded
 * power-of-two dimension (<= 2^28), nbits 1..4, P = ceil(D / 32).
 *   payload [n][nbits * P] u32, one row per message (row pitch: uq_quicfl_packed_words): plane b is words
 *     [b P, (b + 1) P); bit i % 32 of word i / 32 of plane b is bit b of X_i (uq_rht_sign_bits' numbering);
 *     every bit that names no coordinate is 0 (bits >= D when D < 32).  X must lie in [0, 2^nbits): a value
 *     outside sets UQ_QFL_X_RANGE in info[j] and is stored as 0.
 *   exact_index [n][D] int32: row j's exact coordinates, ascending, in its first exact_count[j] entries, beside
 *     the compact exact_vals [n][D] f32 (exact_layout 1) and exact_count [n]; a packed message has no mask.
 *   payload_bits [n] int64 = nbits D + 64 exact_count[j].
 * uq_quicfl_packed_words: host only; D not a power of two, D > 2^28 or nbits outside 1..4 return UQ_E_INVALID.
 * uq_quicfl_pack_x: X [n][D] int64 / uint8 / int32 (x_kind 0 / 1 / 2) and exact_mask [n][D] u8 (or NULL: no
 *   exact coordinate) -> payload, exact_index, exact_count, payload_bits (or NULL), info (or NULL; written).
 * uq_quicfl_unpack_x: payload and the list (exact_index and exact_count, or both NULL) -> X_u8 [n][D] and
 *   exact_mask [n][D] u8; a malformed list (below) sets UQ_QFL_BAD_EXACT in info[j] (or NULL; written).
 * uq_quicfl_compress_packed_f32: uq_quicfl_compress_f32 with payload (nbits planes), exact_index and payload_bits
 *   in place of X, x_kind and exact_mask: the same generators, px_state_out, flags, side stream and dispatch
 *   plan, exact_vals / exact_count / scale the same bits.  Workspace: uq_quicfl_packed_workspace_bytes.
 * uq_quicfl_receive_packed_f32: uq_quicfl_receive_ws_f32 on such a message (the list: all three or all NULL);
 *   out the same bits.  A row whose list is malformed -- exact_count outside 0..D, an index outside 0..D-1, or
 *   indices not strictly ascending -- gets UQ_QFL_BAD_EXACT in info[j]; nothing is written outside its row.
 *   Workspace (required): uq_quicfl_receive_packed_workspace_bytes.
 * Test hooks: uq_test_set_quicfl_packed_hooks, process-wide, bit 0 sends every packed call through the u8
 *   kernels on rows in the workspace and the converters (returns the previous flags);
 *   uq_test_last_quicfl_packed_plan: of this thread's last packed call of that side, 4 int64 of which
 *   min(cap, 4) are written: [0] nbits (0: it launched nothing) [1] form: 1 the rounds write / read the planes
 *   themselves, 2 the converter path [2] P [3] the row pitch.  The QUIC-FL plan (uq_test_last_quicfl_plan) of a
 *   packed call is the u8 call's of its shape. */
int uq_test_set_quicfl_packed_hooks(int flags);
int uq_test_last_quicfl_packed_plan(int32_t side, int64_t* plan_out, int32_t cap);
int uq_quicfl_packed_words(int64_t D, int32_t nbits, int64_t* pitch_words);
int uq_quicfl_pack_x(const void* X, int32_t x_kind, int64_t n, int64_t D, int32_t nbits, const uint8_t* exact_mask,
                     uint32_t* payload, int32_t* exact_index, int32_t* exact_count, int64_t* payload_bits, int32_t* info,
                     void* stream);
int uq_quicfl_unpack_x(const uint32_t* payload, int64_t n, int64_t D, int32_t nbits, const int32_t* exact_index,
                       const int32_t* exact_count, uint8_t* X_u8, uint8_t* exact_mask, int32_t* info, void* stream);
int uq_quicfl_packed_workspace_bytes(int64_t n, int64_t dim, size_t* bytes_out);
int uq_quicfl_compress_packed_f32(const float* x, int64_t n, int64_t dim, const int8_t* signs, const int32_t* sign_row,
                                  const float* table_xp, const uint32_t* table_packed, int64_t table_numel, int32_t h_len,
                                  float delta, const int32_t* prng_seeds, const uint32_t* px_state, const int32_t* px_seeds,
                                  uint32_t* px_state_out, uint32_t* payload, int32_t nbits, int32_t* exact_index,
                                  float* exact_vals, int32_t* exact_count, int64_t* payload_bits, float* scale, int32_t* info,
                                  void* ws, size_t ws_bytes, void* stream);
int uq_quicfl_receive_packed_workspace_bytes(int64_t n, int64_t D, size_t* bytes_out);
int uq_quicfl_receive_packed_f32(const uint32_t* payload, int32_t nbits, int64_t n, int64_t D, const float* recv_table,
                                 int32_t table_rows, int32_t h_len, const int32_t* prng_seeds, const int32_t* exact_index,
                                 const float* exact_vals, const int32_t* exact_count, const float* scale, float* out,
                                 int32_t* info, void* ws, size_t ws_bytes, void* stream);
/* xxHash64 of `len` bytes (AS:457 hashes str(seed) with seed 0); host-only, no GPU. */
uint64_t uq_xxh64(const void* data, size_t len, uint64_t seed);
int uq_eden_workspace_bytes(int64_t n, int64_t dim, size_t* bytes_out);
int uq_eden_compress_f32(const float* x, int64_t n, int64_t dim, int32_t nbits, const int8_t* signs,
                         const int32_t* sign_row, uint8_t* bins, float* scale, void* ws, size_t ws_bytes,
                         void* stream);
int uq_eden_decompress_f32(const uint8_t* bins, const float* scale, int64_t n, int64_t dim, int32_t nbits,
                           const int8_t* signs, const int32_t* sign_row, float* out, void* ws, size_t ws_bytes,
                           void* stream);
int uq_eden_f32(const float* x, float* out, int64_t n, int64_t dim, int32_t nbits, const int8_t* signs,
                const int32_t* sign_row, float* scale_out, void* ws, size_t ws_bytes, void* stream);
/* The same three with the diagonal rows also as bits: sign_bits [rows][ceil(D / 32)] u32, bit
 * i % 32 of word i / 32 set where signs[row][i] is -1 (uq_rht_sign_bits makes them from the
 * int8 rows); the passes that apply the diagonal (the sender's first, the receiver's last) read
 * 1/8 byte per coordinate instead of 1.  sign_bits NULL: the int8 rows, as above.  Same results. */
int uq_rht_sign_bits(const int8_t* signs, int64_t rows, int64_t D, uint32_t* bits, void* stream);
int uq_eden_compress_f32_sb(const float* x, int64_t n, int64_t dim, int32_t nbits, const int8_t* signs,
                            const int32_t* sign_row, const uint32_t* sign_bits, uint8_t* bins, float* scale, void* ws,
                            size_t ws_bytes, void* stream);
int uq_eden_decompress_f32_sb(const uint8_t* bins, const float* scale, int64_t n, int64_t dim, int32_t nbits,
                              const int8_t* signs, const int32_t* sign_row, const uint32_t* sign_bits, float* out,
                              void* ws, size_t ws_bytes, void* stream);
int uq_eden_f32_sb(const float* x, float* out, int64_t n, int64_t dim, int32_t nbits, const int8_t* signs,
                   const int32_t* sign_row, const uint32_t* sign_bits, float* scale_out, void* ws, size_t ws_bytes,
                   void* stream);
/* Fractional rates 1 < nbits < 2 (EdenSender.stochastic_quantize, AS:352-368; the receiver,
 * AS:401-411), bit-identical to the reference: p_high = nbits - 1, and coordinate k of the padded
 * row takes the 2-bit table where mask[k] = torch.bernoulli(p_high) of a CPU generator seeded with
 * 7 * seed + 13 is set, the 1-bit table elsewhere; bins and centroids are mixed accordingly and the
 * scale is f32(nrm * nrm) / torch.dot(mixed centroids, vec) in the same order as above.
 * uq_eden_mask_bits: the mask rows, bits [rows][ceil(D / 32)] u32 in uq_rht_sign_bits's layout: bit
 *   i % 32 of word i / 32 of row r set where word i of MT19937 seeded with the low 32 bits of
 *   7 * seeds[r] + 13 (seeds: device int64 [rows], the ROTATION seeds; 64-bit arithmetic) has
 *   low24(w) < threshold, threshold = ceil(f32(p_high) * 2^24) <= 2^24 -- the draw f32(low24) * 2^-24
 *   < f32(p_high).  A pure function of (seed, D, threshold): callers cache the rows.
 * uq_eden_compress_frac_f32 / uq_eden_decompress_frac_f32 / uq_eden_frac_f32: the three _sb entry
 *   points for such a rate: no nbits; client j reads mask row mask_row[j] (device int32 [n], or
 *   NULL: row 0) of mask_bits.  bins are 0..3 where the mask is set and 0..1 elsewhere; of a
 *   message with another bin the receiver reads the bin's low two bits (its low bit where the mask
 *   is clear), where the reference's torch.take raises.  Dispatch, workspace (uq_eden_workspace_bytes) and every other argument as
 *   for nbits = 2. */
int uq_eden_mask_bits(const int64_t* seeds, int64_t rows, int64_t D, uint32_t threshold, uint32_t* bits, void* stream);
int uq_eden_compress_frac_f32(const float* x, int64_t n, int64_t dim, const int8_t* signs, const int32_t* sign_row,
                              const uint32_t* sign_bits, const uint32_t* mask_bits, const int32_t* mask_row, uint8_t* bins,
                              float* scale, void* ws, size_t ws_bytes, void* stream);
int uq_eden_decompress_frac_f32(const uint8_t* bins, const float* scale, int64_t n, int64_t dim, const int8_t* signs,
                                const int32_t* sign_row, const uint32_t* sign_bits, const uint32_t* mask_bits,
                                const int32_t* mask_row, float* out, void* ws, size_t ws_bytes, void* stream);
int uq_eden_frac_f32(const float* x, float* out, int64_t n, int64_t dim, const int8_t* signs, const int32_t* sign_row,
                     const uint32_t* sign_bits, const uint32_t* mask_bits, const int32_t* mask_row, float* scale_out,
                     void* ws, size_t ws_bytes, void* stream);
/* EDEN messages at their rate: the bins bit-packed.  These entry points replace nothing of the reference, which
 * keeps a message's bins as an int64 tensor (AS:335-350, 352-368; read back at AS:398-411); scale and outputs
 * are the bits of the u8 entry points above, and the payload is the packing of their bins.
 * Layout: a client's payload is a row of u32 words, coordinate i of the padded row (D, a power of two) at bit
 * i % 32 of word i / 32 of a plane (uq_rht_sign_bits' numbering), P = ceil(D / 32) words per plane.
 *   plane H, words [0, P): the bin (kind 1), bin >> 1 (kind 2), or for kind UQ_EDEN_NBITS_FRAC bin >> 1 where
 *     the client's mask bit is set and the 1-bit bin where it is clear: above the middle boundary at every rate;
 *   plane L: none (kind 1); words [P, 2 P) = bin & 1 (kind 2); for a fractional rate the low bits of the
 *     mask-set coordinates only, in index order: the r-th set bit of the mask row (r from 0) at bit r % 32 of
 *     word P + r / 32, so the message is D + cnt bits, cnt = popcount(mask row[:D]).
 * Every bit that names no coordinate is written as 0 (bits >= D of the word when D < 32, bits >= cnt of plane
 * L's last word, words of the pitch past it).  Row pitch: uq_eden_packed_words (P for kind 1, else 2 P);
 * payload_bits [n] int64 (or NULL) receives D, 2 D or D + cnt_j.
 * uq_eden_mask_ranks: ranks [rows][P + 1] u32, the exclusive rank (set bits before it) of each word of a mask row
 *   (uq_eden_mask_bits) and cnt in the last entry: a pure function of the row, cached with it by callers.
 * uq_eden_pack_bins / uq_eden_unpack_bins: u8 bins [n][D] <-> payload rows, for any D >= 0; mask_bits,
 *   mask_ranks and mask_row (NULL: row 0) are read for the fractional kind only.  Unpacking a fractional
 *   message gives the bins uq_eden_compress_frac_f32 writes (0..3 where the mask is set, 0..1 elsewhere).
 * uq_eden_compress_packed_f32 / uq_eden_decompress_packed_f32: the _sb / _frac entry points by `kind`, with the
 *   payload rows in place of bins.  Workspace: uq_eden_packed_workspace_bytes.  One wave per client (KE4), KE2+4
 *   and the receiver's 4096-element first pass write / read the words themselves at kinds 1 and 2; other shapes
 *   and the fractional kind go through u8 bins in the workspace and the converters (uq_test_last_eden_packed_plan). */
int uq_eden_packed_words(int64_t D, int32_t kind, int64_t* pitch_words);
int uq_eden_packed_workspace_bytes(int64_t n, int64_t dim, int32_t kind, size_t* bytes_out);
int uq_eden_mask_ranks(const uint32_t* mask_bits, int64_t rows, int64_t D, uint32_t* ranks, void* stream);
int uq_eden_pack_bins(const uint8_t* bins, int64_t n, int64_t D, int32_t kind, const uint32_t* mask_bits,
                      const uint32_t* mask_ranks, const int32_t* mask_row, uint32_t* payload, int64_t* payload_bits,
                      void* stream);
int uq_eden_unpack_bins(const uint32_t* payload, int64_t n, int64_t D, int32_t kind, const uint32_t* mask_bits,
                        const uint32_t* mask_ranks, const int32_t* mask_row, uint8_t* bins, void* stream);
int uq_eden_compress_packed_f32(const float* x, int64_t n, int64_t dim, int32_t kind, const int8_t* signs,
                                const int32_t* sign_row, const uint32_t* sign_bits, const uint32_t* mask_bits,
                                const uint32_t* mask_ranks, const int32_t* mask_row, uint32_t* payload,
                                int64_t* payload_bits, float* scale, void* ws, size_t ws_bytes, void* stream);
int uq_eden_decompress_packed_f32(const uint32_t* payload, const float* scale, int64_t n, int64_t dim, int32_t kind,
                                  const int8_t* signs, const int32_t* sign_row, const uint32_t* sign_bits,
                                  const uint32_t* mask_bits, const uint32_t* mask_ranks, const int32_t* mask_row, float* out,
                                  void* ws, size_t ws_bytes, void* stream);
/* The receivers with EDEN's coordinate drop (AS:413-423: `ri = torch.randperm(D)[:round(D * pdrop)];
 * vec[ri] = 0; vec /= (1 - pdrop)` on the rotated vector, at rates below 1 bit and for the message
 * field pdrop).  New entry points; the ones above are unchanged and a message without a drop takes
 * them.  One entry per message form, every rate by `kind` (1, 2, UQ_EDEN_NBITS_FRAC: mask_bits /
 * mask_row as the _frac entries take them, NULL at 1 and 2 bits):
 *   drop_bits [n][ceil(D / 32)]: client j's dropped coordinates (uq_randperm_prefix's drop_bits);
 *   cents: HOST floats, the centroids divided by 1 - pdrop by the caller (the binding divides the
 *     reference's f32 table with torch itself, so the quotient is the reference's own): the kind's
 *     table, 2 entries at 1 bit and 4 else (ascending, as AS:309 builds it), then at a fractional
 *     rate the 1-bit table's two.  The kernels select 0 or a table value; no division runs on the GPU.
 * uq_eden_decompress_drop_f32: a u8 message; uq_eden_decompress_packed_drop_f32: a packed one (the
 * payload rows go through uq_eden_unpack_bins' kernel into the workspace's bins); uq_eden_drop_f32:
 * sender and receiver fused on the workspace's bins, as uq_eden_f32_sb / uq_eden_frac_f32.
 * Form (uq_test_last_eden_drop_form, this thread's last call of the three): UQ_EDEN_DROP_VECTOR: KE5d
 * writes the rotated f32 vector [n][D] into the workspace, then the inverse transform's plain passes
 * and the receiver's last pass run on it (uq_test_last_eden_plan(UQ_EDEN_OP_DECOMPRESS) names them).
 * No first pass reads the drop rows itself yet; UQ_EDEN_DROP_NONE after a call that launched nothing.
 * Workspace: uq_eden_workspace_bytes(n, dim).  No host synchronisation. */
#define UQ_EDEN_DROP_NONE 0
#define UQ_EDEN_DROP_VECTOR 1
int uq_test_last_eden_drop_form(int32_t* form_out);
int uq_eden_decompress_drop_f32(const uint8_t* bins, const float* scale, int64_t n, int64_t dim, int32_t kind,
                                const int8_t* signs, const int32_t* sign_row, const uint32_t* sign_bits,
                                const uint32_t* mask_bits, const int32_t* mask_row, const uint32_t* drop_bits,
                                const float* cents, float* out, void* ws, size_t ws_bytes, void* stream);
int uq_eden_decompress_packed_drop_f32(const uint32_t* payload, const float* scale, int64_t n, int64_t dim, int32_t kind,
                                       const int8_t* signs, const int32_t* sign_row, const uint32_t* sign_bits,
                                       const uint32_t* mask_bits, const uint32_t* mask_ranks, const int32_t* mask_row,
                                       const uint32_t* drop_bits, const float* cents, float* out, void* ws,
                                       size_t ws_bytes, void* stream);
int uq_eden_drop_f32(const float* x, float* out, int64_t n, int64_t dim, int32_t kind, const int8_t* signs,
                     const int32_t* sign_row, const uint32_t* sign_bits, const uint32_t* mask_bits, const int32_t* mask_row,
                     const uint32_t* drop_bits, const float* cents, float* scale_out, void* ws, size_t ws_bytes,
                     void* stream);
/* torch.norm(v[j], 2) of each row of v [n][D] f32 in torch's CPU order (AS:329: 8 lanes of
 * fma chains, lanes added in order, sqrt), the norm the EDEN entry points use:
 *   mode 1: the sequential chains (one chain per torch lane; what batches above 256 rows use)
 *   mode 2: the segmented chains (1 <= n <= 256, D a power of two >= 16384; workspace
 *           uq_eden_norm_workspace_bytes): the same bits, the chains cut into segments that
 *           are resolved in parallel (include/../DESIGN.md §4, EDEN)
 *   mode 0: mode 2 where it applies, else mode 1 (the choice the EDEN entry points make).
 * nrm [n] f32. */
int uq_eden_norm_workspace_bytes(int64_t n, int64_t D, size_t* bytes_out);
int uq_eden_norm_f32(const float* v, int64_t n, int64_t D, int32_t mode, float* nrm, void* ws, size_t ws_bytes,
                     void* stream);

/* ---- Scalar and DRIVE baselines: torch.rand_like from the global generator ---------------
 * Scalar_quantize (All_Schemes.py:755-790) and DRIVE_quantize_Hadamard (AS:707-752) for n
 * clients [n][d], bit-identical to the reference on torch CPU (tests/golden/rand_schemes_vectors.*).
 * torch.rand_like takes one MT19937 word per element in index order, u = f32(w & 0xFFFFFF) *
 * 2^-24.  px_state / px_seeds / px_state_out are uq_quicfl_compress_f32's: client j's generator
 * as [n][UQ_QFL_STATE_WORDS] states or as seeds of fresh generators, and the state after the
 * client's words.  d <= 2^28; n = 0 or d = 0 is a no-op.  Workspace: uq_rand_workspace_bytes.
 *
 * uq_scalar_quantize_f32: mn = min(x), mx = max(x) (NaN if x holds one), den = mx - mn.
 *   den == 0: out = x, info[j] = UQ_SCALAR_CONSTANT, no word taken (px_state_out[j] is the input
 *   state).  Else d words: q = clamp((x - mn) / den, 0, 1); t = q * nlevels; fl = floor(t);
 *   out = ((fl + (u < t - fl)) / nlevels) * den + mn, every step one f32 operation.  nlevels is
 *   the f32 of 2^bits - 1; below 1 the reference returns its input, so the call is refused.
 * uq_drive_hadamard_f32: chunks of 2048; a chunk of L coordinates is zero-padded to P, the next
 *   power of two, and takes P words: D = (u > 0.5) * 2 - 1.  The reference's "Hadamard" maps each
 *   adjacent pair (a, b) to (a + b, (a + b) - b), log2(P) times (its views alias).  S =
 *   f32(norm(x)^2) / (sum|Rx| + 1e-12f) with torch's norm and sum orders; out = pairsteps(S *
 *   sign(Rx)) * D.  S_out [n][ceil(d / 2048)] (or NULL) receives each chunk's S.
 *   uq_drive_words(d): the words one client takes, (d / 2048) * 2048 + pow2ceil(d % 2048)
 *   (no last term when d % 2048 == 0); host only. */
#define UQ_SCALAR_CONSTANT 1
int uq_rand_workspace_bytes(int64_t n, int64_t d, size_t* bytes_out);
int uq_drive_words(int64_t d, int64_t* words_out);
int uq_scalar_quantize_f32(const float* x, float* out, int64_t n, int64_t d, float nlevels, const uint32_t* px_state,
                           const int32_t* px_seeds, uint32_t* px_state_out, int32_t* info, void* ws, size_t ws_bytes,
                           void* stream);
int uq_drive_hadamard_f32(const float* x, float* out, int64_t n, int64_t d, const uint32_t* px_state,
                          const int32_t* px_seeds, uint32_t* px_state_out, float* S_out, void* ws, size_t ws_bytes,
                          void* stream);

/* ---- Kashin baseline: Kashin_quantize (All_Schemes.py:834-854) ----------------------------
 * KashinStochasticQuantizationSender.compress (AS:249-261) and its receiver (AS:269-274) for n
 * clients [n][dim], bit-identical to the reference on torch CPU (tests/golden/kashin_vectors.*).
 * D = uq_kashin_padded_dim(dim) (AS:202-210, host only): a power of two doubles, another length
 *   goes to the next power of two, doubled when dim / D > 0.85.  The entries take D and check it
 *   (a power of two >= max(2, dim), <= 2^28).
 * The loop (AS:212-239) runs on the device, nothing waits on the host: M = torch.norm(x) /
 *   f32(sqrt(delta * D)); iteration i: b = RHT(residual padded to D) with diagonal row sign_row[j]
 *   of signs [rows][D] (uq_rht_signs; the reference's rotation seed is 123), c += clamp(b, -M, M);
 *   for i < niters - 1 the residual loses the clamped part's inverse transform and M *= f32(eta);
 *   then err = norm(x - inverse(c)[:dim]) / norm(residual) and the client is done when err <
 *   f32(err).  At i = 0 the two norms are the same bits and at i = niters - 1 the test changes
 *   nothing, so it is evaluated for 0 < i < niters - 1 only.  That needs f32(err) <= 1: the quotient
 *   at i = 0 is 1.0 or NaN, below a larger bound only, where the reference exits after its first
 *   transform; f32(err) > 1 is refused with UQ_E_INVALID.  Every norm is torch's CPU order for
 *   one thread.  iters [n] = the forward transforms each client ran.
 * The stochastic quantizer (AS:67-82) of c: mn = min(c), step = (max(c) - mn) / f32(nlevels - 1),
 *   q = (c - mn) / step, bins = floor(q) + bernoulli(q - floor(q)); coordinate k takes word k of a
 *   CPU generator seeded with xxh64(str(seed)) % 2^16 (uq_xxh64), the draw being f32(w & 0xFFFFFF)
 *   * 2^-24 < p.  The stream is cut into runs of run_words coordinates, R = ceil(D / run_words) per
 *   client, each walked by one wave from its own state: runs [rows][R][UQ_QFL_STATE_WORDS] u32 =
 *   (left, next, state[624]) of the generator at each run's start, client j reading row run_row[j]
 *   (run_row NULL: row j), so clients with one seed share a row.
 * Outputs: bins [n][D] u8, mn [n], step [n], iters [n] and info [n] int32 flags: UQ_KASHIN_BAD_P
 *   (some p is NaN or outside [0, 1], where the reference's torch.bernoulli raises RuntimeError: an
 *   all-zero vector, a NaN or an inf, every vector of dim 1) and UQ_KASHIN_BIN_RANGE (a bin above
 *   255, stored saturated; only nlevels = 256 can reach it).
 * uq_kashin_decompress_f32: out [n][dim] = (H(mn + bins * step) * diag)[:dim], the product and
 *   the sum rounded apart.  uq_kashin_f32: both fused, no message written; mn, step and iters may
 *   be NULL there.  niters >= 1, nlevels in 2..256, delta > 0; n = 0 or dim = 0 is a no-op.
 *   Workspace: uq_kashin_workspace_bytes(n, D). */
#define UQ_KASHIN_BAD_P 1
#define UQ_KASHIN_BIN_RANGE 2
int uq_kashin_padded_dim(int64_t dim, int64_t* D_out);
int uq_kashin_workspace_bytes(int64_t n, int64_t D, size_t* bytes_out);
int uq_kashin_compress_f32(const float* x, int64_t n, int64_t dim, int64_t D, int32_t niters, double eta, double delta,
                           double err, int32_t nlevels, const int8_t* signs, const int32_t* sign_row,
                           const uint32_t* runs, const int32_t* run_row, int64_t run_words, uint8_t* bins, float* mn,
                           float* step, int32_t* info, int32_t* iters, void* ws, size_t ws_bytes, void* stream);
int uq_kashin_decompress_f32(const uint8_t* bins, const float* mn, const float* step, int64_t n, int64_t dim, int64_t D,
                             const int8_t* signs, const int32_t* sign_row, float* out, void* ws, size_t ws_bytes,
                             void* stream);
int uq_kashin_f32(const float* x, float* out, int64_t n, int64_t dim, int64_t D, int32_t niters, double eta, double delta,
                  double err, int32_t nlevels, const int8_t* signs, const int32_t* sign_row, const uint32_t* runs,
                  const int32_t* run_row, int64_t run_words, float* mn, float* step, int32_t* info, int32_t* iters,
                  void* ws, size_t ws_bytes, void* stream);

/* ---- torch.randperm(D)[:k] of the CPU generator (EDEN's coordinate drop, All_Schemes.py:419-423) ----
 * The reference drops round(D * pdrop) coordinates of the rotated vector by
 * `torch.randperm(D)[:k]` on the global CPU generator.  For D < 2^32 / 20 that is a forward
 * Fisher-Yates shuffle, step i = 0 .. D - 2 swapping r[i] with r[i + w_i % (D - i)], w_i the
 * generator's i-th word: D - 1 words whatever k, of which the prefix depends on the first
 * K = min(k, D - 1).  uq_randperm_prefix computes the prefix of n clients without the serial chain
 * (csrc/uq_randperm_kernels.h has the algorithm), bit for bit:
 *   states [n][UQ_QFL_STATE_WORDS] u32 = (left, next, state[624]) of each client's generator where
 *     its permutation starts (may be NULL when no word is taken: D <= 1 or k = 0).  The generator
 *     after a permutation is D - 1 words on: the caller advances it (uq_mt_jump_host).
 *   index_out [n][k] int64 (or NULL) = torch.randperm(D)[:k] per client.
 *   drop_bits [n][ceil(D / 32)] u32 (or NULL): the same set, coordinate i at bit i % 32 of word
 *     i / 32 (uq_rht_sign_bits' numbering); the rows are written whole, so every bit that names no
 *     dropped coordinate, at or above D included, is 0 (k = 0: all of them).
 * k = 0 writes no index; k = D is the whole permutation (every coordinate dropped); D >= 2^32 / 20
 * (torch takes another algorithm), k > D and negative sizes return UQ_E_INVALID.
 * Workspace: uq_randperm_prefix_workspace_bytes(n, D, k), at most about 1 GiB (or one client's
 * need, 4 (3 k + D) bytes and the jump form's blocks, if that is more); a batch that does not fit
 * the workspace it is given is processed in groups of clients inside the call, so any size from one
 * client's up is accepted.  Stream-ordered, no host synchronisation.  The one allocation is the
 * jump form's table of polynomials, made once per (device, run layout) like QUIC-FL's.
 * Test hooks: uq_test_last_randperm_plan writes min(cap, UQ_RANDPERM_PLAN_FIELDS) int64 values of
 * this thread's last call: [0] form of the words stage (UQ_RANDPERM_FORM_*: nothing launched, one
 * wave per client walks the stream, runs from jumped states, words given by the caller)
 * [1] runs per client  [2] blocks of 624 words per run  [3] clients per group  [4] K
 * [5] groups.  uq_test_randperm_from_words runs the same stages on words [n][K] (device) given by
 * the caller instead of a generator's, for word patterns no generator draws; K <= 65536 there, since
 * one position's list may then hold every step and each step reads it whole. */
#define UQ_RANDPERM_PLAN_FIELDS 6
#define UQ_RANDPERM_FORM_NONE 0
#define UQ_RANDPERM_FORM_WALK 1
#define UQ_RANDPERM_FORM_JUMP 2
#define UQ_RANDPERM_FORM_WORDS 3
int uq_randperm_prefix_workspace_bytes(int64_t n, int64_t D, int64_t k, size_t* bytes_out);
int uq_randperm_prefix(const uint32_t* states, int64_t n, int64_t D, int64_t k, int64_t* index_out, uint32_t* drop_bits,
                       void* ws, size_t ws_bytes, void* stream);
int uq_test_randperm_from_words(const uint32_t* words, int64_t n, int64_t D, int64_t k, int64_t* index_out,
                                uint32_t* drop_bits, void* ws, size_t ws_bytes, void* stream);
int uq_test_last_randperm_plan(int64_t* plan_out, int32_t cap);

/* After the stream has been synchronised: UQ_OK, or UQ_E_TIMEOUT if any
 * inter-workgroup wait in a previous call on this workspace gave up. Clears it. */
int uq_check_status(void* ws, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* UQ_DME_H */
