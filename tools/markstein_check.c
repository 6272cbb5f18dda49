/* Exhaustive check of the division x / den in the stream and look-back kernels' pass 1
 * (csrc/uq_common.h: div_plan / div4).  Tool, not shipped.
 *
 *   den = L1 + 1e-12 (>= 2^-39.9);  fast path only while den < 2^40
 *   y   = RN(1/den)                              one IEEE division per client
 *   q0  = RN(x*y)
 *   q1  = RN(q0 + RN(x - den*q0)*y)              faithful
 *   q2  = RN(q1 + RN(x - den*q1)*y)              Markstein: = RN(x/den)
 *   guard: !(|q2| >= 2^-59/den) && x != 0  ->  q2 = x/den (IEEE)
 *          (every 0 < |x| < 2^-60, and q2 NaN: x = inf/NaN or overflow)
 *
 * For each divisor, EVERY non-negative finite f32 x and its negation are checked
 * against the IEEE quotient bit for bit (x = +-0 may differ only in the sign of a zero
 * quotient, which the kernel never observes: it uses v < 0 and |v| only).
 * Divisors: 1e-12 (L1 = 0), 2^40 - ulp, 1e-12 + tiny, then random significands at random
 * exponents in [-39, 39].
 *
 *   gcc -O2 -mfma -fopenmp -ffp-contract=off tools/markstein_check.c -o /tmp/mk -lm
 *   /tmp/mk [n_divisors=14]        # ~13 s per divisor on 8 cores
 *   /tmp/mk 13 m                   # the biased dequantize divisors m (div_plan_m)
 *   /tmp/mk 6 q                    # QUIC-FL's q = v / delta (quicfl_send_wave_kernel, div_plan_norm):
 *                                  # the deltas of the reference's four data.txt (AS:480) and the tests' 0.06, 0.05
 * Round-1 run: 14 divisors, 59,894,661,120 quotients, 0 mismatches.  An earlier variant
 * without the guard showed the failures it removes: |x| <= 2^-87 (residual underflow).
 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static float fbits(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static uint32_t ubits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

static inline float kernel_div(float a, float den, float y, float thr) {
    float q = a * y;
    float r = fmaf(-den, q, a);
    q = fmaf(r, y, q);
    r = fmaf(-den, q, a);
    q = fmaf(r, y, q);
    if (!(fabsf(q) >= thr) && a != 0.0f) q = a / den;
    return q;
}

/* "m" mode: the biased dequantize step k''/m (div_plan_m: den = f32(m), no 1e-12 term)
 * for the m values of the configs (C1, C2/C3, C4, C5, CIFAR-10 at R=1,2) plus
 * 1, 3 and f32(2^24+1), every finite x as above. */
static const float kM[] = {219.f, 652.f, 224426.f, 668488.f, 897706.f, 2673952.f, 36931.f, 110006.f,
                           26245.f, 78176.f, 1.f, 3.f, 16777217.f};

int main(int argc, char** argv) {
    const int mmode = argc > 2 && strcmp(argv[2], "m") == 0;
    const int qmode = argc > 2 && strcmp(argv[2], "q") == 0;
    static const double kDelta[] = {0.0006194538156387708, 0.0006194538156392149, 0.0006194538156414353, 0.06, 0.05,
                                    0.0006194538156414353 * 4096};
    const int nb = argc > 1 ? atoi(argv[1]) : 14;
    uint64_t s = 12345;
    long long bad = 0, total = 0;
    for (int ib = 0; ib < nb; ++ib) {
        s ^= s << 13; s ^= s >> 7; s ^= s << 17;
        const int e = -39 + (int)((s >> 30) % 79u);
        float den = fbits(((uint32_t)(127 + e) << 23) | (uint32_t)(s & 0x7FFFFF));
        if (ib == 0) den = 1e-12f;
        if (ib == 1) den = nextafterf(0x1p40f, 0.0f);
        if (ib == 2) den = 1e-12f + 1e-12f * 0x1p-20f;
        if (mmode) {
            if (ib >= (int)(sizeof kM / sizeof kM[0])) break;
            den = kM[ib];
        }
        if (qmode) {
            if (ib >= (int)(sizeof kDelta / sizeof kDelta[0])) break;
            den = (float)kDelta[ib];
        }
        const float y = 1.0f / den, thr = 0x1p-59f / den;
        long long lb = 0;
#pragma omp parallel for reduction(+ : lb) schedule(static, 1 << 16)
        for (uint32_t u = 0; u < 0x7F800000u; ++u) {
            const float a = fbits(u);
            for (int sg = 0; sg < 2; ++sg) {
                const float x = sg ? -a : a;
                const float want = x / den, got = kernel_div(x, den, y, thr);
                if (ubits(want) != ubits(got) && !(want == 0.0f && got == 0.0f)) ++lb;
            }
        }
        printf("den=%a: %lld mismatches\n", (double)den, lb);
        fflush(stdout);
        bad += lb;
        total += 2LL * 0x7F800000u;
    }
    printf("%d divisors, %lld quotients, %lld mismatches\n", nb, total, bad);
    return bad != 0;
}
