// count_centroid_check.cpp - the host build of pyrecode_amd/csrc/rc_count.h as a stand-alone program (tests/test_count_centroid_cpu.py builds
// it, also under AddressSanitizer / UBSan): cnt_rhe against 128-bit arithmetic, cnt_finish's three methods and its weight-0 fallback.
// Prints one line per group of checks and "ok"; the exit status is the number of failed groups.
#include <stdint.h>
#include <stdio.h>

#include "../../pyrecode_amd/csrc/rc_count.h"

typedef unsigned __int128 u128;

// nearest integer of S / w, ties to even, in 128 bits: floor((2 S + w) / (2 w)), minus one where that is an odd result of an exact tie
static uint64_t rhe128(uint64_t S, uint64_t w)
{
    const u128 num = (u128)2 * S + w, den = (u128)2 * w;
    u128 q = num / den;
    if (num % den == 0 && (q & 1)) --q;
    return (uint64_t)q;
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t next64()
{
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static int failures = 0;
static void group(const char *name, uint64_t bad, uint64_t n)
{
    printf("%-28s %llu checks, %llu wrong\n", name, (unsigned long long)n, (unsigned long long)bad);
    if (bad) ++failures;
}
static uint64_t differs(uint64_t S, uint64_t w) { return rc::cnt_rhe(S, w) != rhe128(S, w) ? 1u : 0u; }

int main()
{
    uint64_t bad = 0, n = 0;
    for (uint64_t S = 0; S < 4096; ++S, ++n) bad += differs(S, 1);
    bad += differs(~0ull, 1); ++n;
    group("weight 1", bad, n);

    bad = n = 0;
    for (uint64_t w = 1; w < 4096; ++w, ++n) bad += differs(0, w);
    bad += differs(0, 1ull << 48); ++n;
    group("S = 0", bad, n);

    // ties: S = (2 q + 1) * h over w = 2 h, for even and odd q - and their neighbours on both sides
    bad = n = 0;
    for (uint64_t h = 1; h < 200; ++h)
        for (uint64_t q = 0; q < 200; ++q) {
            const uint64_t S = (2 * q + 1) * h, w = 2 * h;
            if (rc::cnt_rhe(S, w) != q + (q & 1)) ++bad;
            bad += differs(S, w) + differs(S + 1, w) + (S ? differs(S - 1, w) : 0);
            n += 4;
        }
    group("ties of both parities", bad, n);

    // the largest operands: S just below 2^64, weight 2^48 (area 2^32 pixels of 65 535) and around it
    bad = n = 0;
    const uint64_t big_w[] = {1ull << 48, (1ull << 48) - 1, (1ull << 48) + 1, 65535ull * 0xFFFFFFFFull, 0xFFFFFFFFull, ~0ull, (1ull << 63), (1ull << 63) + 1};
    for (uint64_t w : big_w)
        for (uint64_t k = 0; k < 64; ++k) {
            bad += differs(~0ull - k, w) + differs((1ull << 63) + k, w) + differs(w / 2 + k, w) + differs(w / 2 - k, w) + differs(w + w / 2 + (w > (1ull << 62) ? 0 : k), w);
            n += 5;
        }
    group("operands at their maxima", bad, n);

    bad = n = 0;
    for (int i = 0; i < 4000000; ++i, ++n) {
        const uint64_t a = next64(), b = next64();
        const uint64_t w = (b >> (a & 63)) | 1u;               // every magnitude
        const uint64_t S = a >> ((b >> 8) & 63);
        bad += differs(S, w);
        if ((i & 7) == 0) { bad += differs(w / 2 * (2 * (a & 1023) + 1), w & ~1ull ? w & ~1ull : 2); ++n; }      // near ties
    }
    group("seeded pairs", bad, n);

    // cnt_finish: the three methods, and the weighted average of a component that weighs nothing
    bad = n = 0;
    int32_t r, c;
    rc::CntSums s{};
    s.a = 25; s.b = 3; s.w = 14; s.area = 5; s.za = 99; s.zb = 99;                    // the L of the Python model's hand-worked case
    rc::cnt_finish(rc::CNT_WEIGHTED, s, 4, &r, &c);
    bad += !(r == 2 && c == 0); ++n;
    s = rc::CntSums{}; s.a = 7; s.b = 3; s.w = 14; s.area = 5;
    rc::cnt_finish(rc::CNT_UNWEIGHTED, s, 4, &r, &c);
    bad += !(r == 1 && c == 1); ++n;
    s = rc::CntSums{}; s.w = 0; s.area = 3; s.za = 3; s.zb = 6;                        // three zeros at (1, 1..3)
    rc::cnt_finish(rc::CNT_WEIGHTED, s, 6, &r, &c);
    bad += !(r == 1 && c == 2); ++n;
    s = rc::CntSums{}; s.w = 0; s.area = 2; s.za = 5; s.zb = 7;                        // ties in both axes: 2.5 -> 2, 3.5 -> 4
    rc::cnt_finish(rc::CNT_WEIGHTED, s, 9, &r, &c);
    bad += !(r == 2 && c == 4); ++n;
    // maximum: the larger value wins; among equal values the earlier pixel; a key is never 0
    const uint64_t k1 = rc::cnt_max_key(9, 1 * 6 + 2), k2 = rc::cnt_max_key(9, 1 * 6 + 3), k3 = rc::cnt_max_key(10, 2 * 6 + 5), k0 = rc::cnt_max_key(0, 0xFFFFFFFEu);
    bad += !(k1 > k2 && k3 > k1 && k0 != 0 && k0 < k2); n += 1;
    s = rc::CntSums{}; s.a = k1 > k2 ? k1 : k2; s.w = 18; s.area = 2;
    rc::cnt_finish(rc::CNT_MAX, s, 6, &r, &c);
    bad += !(r == 1 && c == 2); ++n;
    s.a = rc::cnt_max_key(65535, 65534u * 65535u + 65534u);                            // the last pixel of the largest frame
    rc::cnt_finish(rc::CNT_MAX, s, 65535, &r, &c);
    bad += !(r == 65534 && c == 65534); ++n;
    group("cnt_finish", bad, n);

    if (!failures) printf("ok\n");
    return failures;
}
