/* Exhaustive check of pass 1's signed product (csrc/uq_unbiased_kernels.h: tile_pass1, and
 * div4<true> in csrc/uq_common.h).  Tool, not shipped.
 *
 * Before:  p = |v|;  mp = fm*p;  fl = floor(mp);  fr = mp - fl;  mps = v < 0 ? -mp : mp
 * Now:     mps = fm*v;  mp = |mps|;  fl = floor(mp);  fr = mp - fl
 *          where v is never -0 (part B) and a NaN v comes with its sign cleared (only the IEEE
 *          division of a client whose L1 is not finite gives one; tile_pass1 clears it there).
 *
 * Part A: for each fm, EVERY f32 bit pattern v (finite, +-0, +-inf, every NaN): v is brought
 * in as the kernel brings it (v + 0.0f, the sign of a NaN cleared) and mps, fl, fr of the two
 * forms are compared bit for bit.  v + 0.0f is applied to every v, which also shows that it
 * changes no value but -0.
 * fm: m of the configs and of the tests' shapes (R = 1 .. 10), 1, 3, 2^24 + 2 and 2^31.
 *
 * Part B: for each divisor den (as tools/markstein_check.c draws them), EVERY finite f32 x of
 * either sign: a Markstein quotient that the guard does not recompute is never -0, and a
 * recomputed one is x / den + 0.0f: the IEEE quotient, except +0 for -0.
 *
 *   gcc -O2 -mfma -fopenmp -ffp-contract=off tools/pass1_sign_check.c -o /tmp/p1 -lm
 *   /tmp/p1 [n_fm=10] [n_divisors=6]
 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static float fbits(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static uint32_t ubits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

static const float kFm[] = {224426.f, 2629.f, 7833.f, 204513.f, 49373626.f, 219.f, 1.f, 3.f, 16777218.f, 0x1p31f};

static inline float markstein(float a, float den, float y) {
    float q = a * y;
    float r = fmaf(-den, q, a);
    q = fmaf(r, y, q);
    r = fmaf(-den, q, a);
    return fmaf(r, y, q);
}

int main(int argc, char** argv) {
    const int nfm = argc > 1 ? atoi(argv[1]) : (int)(sizeof kFm / sizeof kFm[0]);
    const int nb = argc > 2 ? atoi(argv[2]) : 6;
    long long bad = 0;
    for (int i = 0; i < nfm && i < (int)(sizeof kFm / sizeof kFm[0]); ++i) {
        const float fm = kFm[i];
        long long lb = 0;
#pragma omp parallel for reduction(+ : lb) schedule(static, 1 << 16)
        for (int64_t w = 0; w < (int64_t)1 << 32; ++w) {
            const float v = fbits((uint32_t)w);
            /* before */
            const float p = fabsf(v);
            const float mp0 = fm * p;
            const float fl0 = floorf(mp0);
            const float fr0 = mp0 - fl0;
            const float mps0 = v < 0.0f ? -mp0 : mp0;
            /* now */
            volatile float zero = 0.0f;
            float vz = v + zero;
            if (vz != vz) vz = fabsf(vz);
            if (ubits(vz) != ubits(v) && !(ubits(v) == 0x80000000u && ubits(vz) == 0u) && v == v) ++lb;   /* + 0 changed a value */
            const float mps1 = fm * vz;
            const float mp1 = fabsf(mps1);
            const float fl1 = floorf(mp1);
            const float fr1 = mp1 - fl1;
            if (ubits(mps0) != ubits(mps1) || ubits(fl0) != ubits(fl1) || ubits(fr0) != ubits(fr1)) ++lb;
        }
        printf("A fm=%a: %lld mismatches\n", (double)fm, lb);
        fflush(stdout);
        bad += lb;
    }
    uint64_t s = 12345;
    for (int ib = 0; ib < nb; ++ib) {
        s ^= s << 13; s ^= s >> 7; s ^= s << 17;
        const int e = -39 + (int)((s >> 30) % 79u);
        float den = fbits(((uint32_t)(127 + e) << 23) | (uint32_t)(s & 0x7FFFFF));
        if (ib == 0) den = 1e-12f;
        if (ib == 1) den = nextafterf(0x1p40f, 0.0f);
        if (ib == 2) den = 1e-12f + 1e-12f * 0x1p-20f;
        const float y = 1.0f / den, thr = 0x1p-59f / den;
        long long lb = 0;
#pragma omp parallel for reduction(+ : lb) schedule(static, 1 << 16)
        for (uint32_t u = 0; u < 0x7F800000u; ++u) {
            for (int sg = 0; sg < 2; ++sg) {
                const float x = sg ? -fbits(u) : fbits(u);
                float q = markstein(x, den, y);
                if (!(fabsf(q) >= thr) && x != 0.0f) {
                    volatile float zero = 0.0f;
                    const float want = x / den;
                    q = want + zero;
                    if (ubits(q) != ubits(want) && !(ubits(want) == 0x80000000u && ubits(q) == 0u)) ++lb;
                }
                if (ubits(q) == 0x80000000u) ++lb;
            }
        }
        printf("B den=%a: %lld quotients of -0 or changed by + 0\n", (double)den, lb);
        fflush(stdout);
        bad += lb;
    }
    printf("%lld mismatches\n", bad);
    return bad != 0;
}
