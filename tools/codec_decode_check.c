/* Stand-alone check that uqc_decode (oracle/uq_codec.c) reads nothing outside the message it
 * is given: every message is decoded from a heap copy of exactly its size, so a sanitizer build
 * reports any read past it.  Host code only, no GPU.
 *
 *   gcc -O1 -g -std=c11 -fsanitize=address,undefined -fno-omit-frame-pointer \
 *       -o codec_decode_check tools/codec_decode_check.c oracle/uq_codec.c && ./codec_decode_check
 *
 * Prints each verdict and "done"; exit status 0 when the good message decodes and every
 * structural corruption is refused.  2000 single-bit corruptions follow, whatever their verdict.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

uint64_t uqc_bound(int64_t d);
uint64_t uqc_encode(const int8_t* codes, int64_t d, int64_t m, float l1, int exact, uint8_t* out);
int uqc_decode(const uint8_t* msg, uint64_t size, int8_t* codes, int64_t d_expect, float* l1, int64_t* m);

static int run(const uint8_t* src, uint64_t n, int64_t d) {
    uint8_t* msg = malloc(n);
    int8_t* codes = malloc((size_t)d);
    float l1;
    int64_t m;
    memcpy(msg, src, n);
    const int rc = uqc_decode(msg, n, codes, d, &l1, &m);
    free(msg);
    free(codes);
    return rc;
}

int main(void) {
    const int64_t d = 70001;                         /* one full chunk and a ragged one */
    int8_t* codes = malloc((size_t)d);
    uint32_t s = 12345;
    for (int64_t i = 0; i < d; ++i) {                /* mostly 0, the rest in -4..3 */
        s = s * 1664525u + 1013904223u;
        codes[i] = (s >> 24) < 200 ? 0 : (int8_t)((int)((s >> 16) % 8) - 4);
    }
    uint8_t* good = malloc(uqc_bound(d));
    const uint64_t n = uqc_encode(codes, d, 7, 1.5f, 0, good);
    uint8_t* b = malloc(n);
    int fails = 0;
    int rc = run(good, n, d);
    printf("good: %d (size %llu)\n", rc, (unsigned long long)n);
    fails += rc != 0;
    uint16_t nsym;
    memcpy(&nsym, good + 28, 2);
    const uint64_t wend = (40 + 2 * (uint64_t)nsym + 3) & ~(uint64_t)3;
    const struct { const char* what; uint64_t off; uint32_t v; int bytes; } bad[] = {
        {"words_end[1] = 2^32 - 1", wend + 4, 0xFFFFFFFFu, 4}, {"words_end[0] = 2^31 - 1", wend, 0x7FFFFFFFu, 4},
        {"nchunks = 2^30", 32, 1u << 30, 4},                   {"nchunks = 3", 32, 3, 4},
        {"nsym = 256", 28, 256, 2},                            {"nsym = 1", 28, 1, 2},
        {"size + 4", 36, (uint32_t)n + 4, 4},
    };
    for (size_t k = 0; k < sizeof bad / sizeof bad[0]; ++k) {
        memcpy(b, good, n);
        memcpy(b + bad[k].off, &bad[k].v, (size_t)bad[k].bytes);
        rc = run(b, n, d);
        printf("%s: %d\n", bad[k].what, rc);
        fails += rc == 0;
    }
    const uint32_t cut = (uint32_t)(wend + 8 + 16);  /* ends inside the states, size field consistent */
    memcpy(b, good, n);
    memcpy(b + 36, &cut, 4);
    rc = run(b, cut, d);
    printf("cut inside the states: %d\n", rc);
    fails += rc == 0;
    for (int k = 0; k < 2000; ++k) {
        memcpy(b, good, n);
        s = s * 1664525u + 1013904223u;
        b[(s >> 8) % n] ^= (uint8_t)(1u << (s & 7));
        run(b, n, d);
    }
    free(b);
    free(good);
    free(codes);
    puts("done");
    return fails != 0;
}
