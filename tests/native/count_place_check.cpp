// count_place_check.cpp - the host build of pyrecode_amd/csrc/rc_count.h's placement on a finer grid as a stand-alone program
// (tests/test_counted_view_cpu.py builds it, also under AddressSanitizer / UBSan): cnt_place against 128-bit arithmetic on its whole domain
// (1 <= s <= 16, 1 <= w < 2^48, S <= 65535 w), and cnt_finish_fine's three methods and its weight-0 fallback.
// Prints one line per group of checks and "ok"; the exit status is the number of failed groups.
#include <stdint.h>
#include <stdio.h>

#include "../../pyrecode_amd/csrc/rc_count.h"

typedef unsigned __int128 u128;

// (2 s S + (s - 1) w) / (2 w) to the nearest integer, ties to even, in 128 bits; *tie: whether it was one
static uint64_t place128(uint64_t S, uint64_t w, uint32_t s, bool *tie = nullptr)
{
    const u128 num = (u128)2 * s * S + (u128)(s - 1) * w, den = (u128)2 * w;
    u128 q = num / den;
    const u128 rem = num % den;
    if (tie) *tie = 2 * rem == den;
    if (2 * rem > den || (2 * rem == den && (q & 1))) ++q;
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
static uint64_t differs(uint64_t S, uint64_t w, uint32_t s) { return rc::cnt_place(S, w, s) != place128(S, w, s) ? 1u : 0u; }

static const uint64_t W_MAX = (1ull << 48) - 1, V_MAX = 65535;

int main()
{
    uint64_t bad = 0, n = 0;
    // s = 1 is cnt_rhe
    for (uint64_t w = 1; w < 64; ++w)
        for (uint64_t S = 0; S < 64 * w; ++S, ++n) bad += rc::cnt_place(S, w, 1) != rc::cnt_rhe(S, w);
    for (int i = 0; i < 200000; ++i, ++n) {
        const uint64_t w = (next64() >> (16 + next64() % 48)) | 1u, S = next64() % (V_MAX * w + 1);
        bad += rc::cnt_place(S, w, 1) != rc::cnt_rhe(S, w);
    }
    group("s = 1 is cnt_rhe", bad, n);

    // every s on small operands, exhaustively; the result stays inside [0, s * n - 1] for a centroid in [0, n - 1]
    bad = n = 0;
    for (uint32_t s = 1; s <= 16; ++s)
        for (uint64_t w = 1; w <= 48; ++w)
            for (uint64_t S = 0; S <= 9 * w; ++S, ++n) {
                bad += differs(S, w, s);
                if (rc::cnt_place(S, w, s) > (uint64_t)s * 10 - 1) ++bad;
            }
    group("every s, small operands", bad, n);

    // hand-written ties.  s even: every integer centroid q is one (u = s q + (s - 1) / 2): t = s q + s / 2 - 1, even or odd by s / 2.
    // s odd: a centroid q + 1 / 2 is one (u = s q + s - 1 / 2): its floor t = s q + s - 1 has the parity of s q.
    bad = n = 0;
    uint64_t ties_odd_sq = 0, ties_even_sq = 0;
    for (uint32_t s = 1; s <= 16; ++s)
        for (uint64_t q = 0; q < 40; ++q)
            for (uint64_t h = 1; h < 12; ++h) {
                bool tie = false;
                uint64_t S, w;
                if (s & 1) { S = (2 * q + 1) * h; w = 2 * h; }       // q + 1 / 2
                else { S = q * h; w = h; }                           // q
                const uint64_t want = place128(S, w, s, &tie);
                if (!tie) ++bad;
                const uint64_t fl = (s & 1) ? s * q + (s - 1) : s * q + s / 2 - 1;       // the floor of u
                if (want != fl + (fl & 1)) ++bad;
                if (rc::cnt_place(S, w, s) != want) ++bad;
                ((s * q) & 1 ? ties_odd_sq : ties_even_sq) += 1;
                bad += differs(S + 1, w, s) + (S ? differs(S - 1, w, s) : 0);
                n += 5;
            }
    // the case that tells the parity of the total from the parity of qq: s = 3, S / w = 3 / 2 -> u = 3 * 1.5 + 1 = 5.5; q = 1, s q = 3 (odd),
    // qq = 2 (even): the total 5 is odd -> 6; qq's parity would say 5
    bad += rc::cnt_place(3, 2, 3) != 6; ++n;
    bad += rc::cnt_place(1, 2, 3) != 2; ++n;           // u = 2.5 -> 2 (s q = 0, even)
    bad += rc::cnt_place(5, 1, 2) != 10; ++n;          // u = 10.5 -> 10
    bad += rc::cnt_place(5, 1, 4) != 22; ++n;          // u = 21.5 -> 22
    bad += !(ties_odd_sq > 1000 && ties_even_sq > 1000); ++n;
    group("ties, s q odd and even", bad, n);

    // the domain's corners: w = 2^48 - 1, S = 65535 w, S = 0, and their neighbours, for every s
    bad = n = 0;
    const uint64_t ws[] = {1, 2, 3, W_MAX, W_MAX - 1, W_MAX / 2, W_MAX / 2 + 1, (1ull << 47), 65535ull * 0xFFFFFFFFull, 0xFFFFFFFFull};
    for (uint32_t s = 1; s <= 16; ++s)
        for (uint64_t w : ws)
            for (uint64_t k = 0; k < 48; ++k) {
                const uint64_t top = V_MAX * w;
                const uint64_t Ss[] = {0 + (k < top ? k : 0), top - (k < top ? k : 0), w / 2 + k, (w - 1) / 2 * (2 * k + 1), V_MAX / 2 * w + k, (top / 2 > k ? top / 2 - k : 0)};
                for (uint64_t S : Ss) {
                    if (S > top) continue;
                    bad += differs(S, w, s);
                    if (rc::cnt_place(S, w, s) > (uint64_t)s * 65536 - 1) ++bad;      // centroid in [0, 65535]
                    ++n;
                }
            }
    bad += rc::cnt_place(V_MAX * W_MAX, W_MAX, 16) != 16 * V_MAX + 8; ++n;           // u = 16 * 65535 + 7.5 -> the even neighbour
    bad += rc::cnt_place(0, W_MAX, 16) != 8; ++n;                                      // u = 7.5 -> 8
    bad += rc::cnt_place(0, W_MAX, 15) != 7; ++n;
    group("corners of the domain", bad, n);

    // seeded pairs over every magnitude of w, S anywhere in [0, 65535 w], and near ties
    bad = n = 0;
    uint64_t ties = 0;
    for (int i = 0; i < 1500000; ++i) {
        const uint64_t a = next64(), b = next64();
        const uint32_t s = 1 + (uint32_t)(a % 16);
        uint64_t w = (b >> (16 + (a >> 8) % 48));
        if (w == 0) w = 1;
        const uint64_t S = next64() % (V_MAX * w + 1);
        bad += differs(S, w, s);
        ++n;
        if ((i & 3) == 0) {                                        // an exact tie, then its neighbours: S / w = q (s even) or q + 1 / 2 (s odd)
            const uint64_t q = (a >> 16) % V_MAX;
            uint64_t w2 = (s & 1) ? (w & ~1ull) : w;
            if (w2 == 0) w2 = 2;
            const uint64_t S2 = (s & 1) ? q * w2 + w2 / 2 : q * w2;
            bool tie = false;
            (void)place128(S2, w2, s, &tie);
            ties += tie;
            bad += differs(S2, w2, s) + differs(S2 + 1, w2, s) + (S2 ? differs(S2 - 1, w2, s) : 0);
            n += 3;
        }
    }
    bad += !(ties > 300000);
    group("seeded pairs", bad, n);

    // cnt_finish_fine: the choice between (a, w), (za, area) and the rest is cnt_finish's; at upsample 1 it IS cnt_finish
    bad = n = 0;
    for (int i = 0; i < 200000; ++i) {
        rc::CntSums s{};
        const uint32_t nx = 1 + (uint32_t)(next64() % 65535), ny = 1 + (uint32_t)(next64() % 65535);
        s.area = 1 + (uint32_t)(next64() % 1000);
        s.w = (i % 5 == 0) ? 0 : 1 + next64() % (65535ull * s.area);
        const uint32_t method = (uint32_t)(i % 3);
        if (method == rc::CNT_MAX) s.a = rc::cnt_max_key((uint32_t)(next64() % 65536), (uint32_t)(next64() % ((uint64_t)nx * ny)));
        else {
            s.a = next64() % ((ny - 1) * (method == rc::CNT_WEIGHTED ? s.w : (uint64_t)s.area) + 1);
            s.b = next64() % ((nx - 1) * (method == rc::CNT_WEIGHTED ? s.w : (uint64_t)s.area) + 1);
            s.za = next64() % ((ny - 1) * (uint64_t)s.area + 1);
            s.zb = next64() % ((nx - 1) * (uint64_t)s.area + 1);
        }
        int32_t r, c;
        uint32_t fr, fc;
        rc::cnt_finish(method, s, nx, &r, &c);
        rc::cnt_finish_fine(method, s, nx, 1, &fr, &fc);
        bad += !((int64_t)fr == r && (int64_t)fc == c); ++n;
        const uint32_t up = 1 + (uint32_t)(next64() % 16);
        rc::cnt_finish_fine(method, s, nx, up, &fr, &fc);
        uint64_t wr, wc;
        if (method == rc::CNT_MAX) { const uint32_t p = 0xFFFFFFFFu - (uint32_t)s.a; wr = place128(p / nx, 1, up); wc = place128(p % nx, 1, up); }
        else if (method == rc::CNT_WEIGHTED && s.w) { wr = place128(s.a, s.w, up); wc = place128(s.b, s.w, up); }
        else if (method == rc::CNT_WEIGHTED) { wr = place128(s.za, s.area, up); wc = place128(s.zb, s.area, up); }
        else { wr = place128(s.a, s.area, up); wc = place128(s.b, s.area, up); }
        bad += !(fr == wr && fc == wc && fr < (uint64_t)up * ny && fc < (uint64_t)up * nx); ++n;
    }
    // by hand: the L of the Python model's worked case (25 / 14, 3 / 14) at upsample 4: 4 * 25 / 14 + 1.5 = 8.64 -> 9, 4 * 3 / 14 + 1.5 = 2.36 -> 2
    uint32_t fr, fc;
    rc::CntSums s{};
    s.a = 25; s.b = 3; s.w = 14; s.area = 5; s.za = 99; s.zb = 99;
    rc::cnt_finish_fine(rc::CNT_WEIGHTED, s, 4, 4, &fr, &fc);
    bad += !(fr == 9 && fc == 2); ++n;
    s = rc::CntSums{}; s.w = 0; s.area = 2; s.za = 5; s.zb = 7;                        // weight 0: (2.5, 3.5) at upsample 2 -> 5.5 -> 6, 7.5 -> 8
    rc::cnt_finish_fine(rc::CNT_WEIGHTED, s, 9, 2, &fr, &fc);
    bad += !(fr == 6 && fc == 8); ++n;
    s = rc::CntSums{}; s.a = rc::cnt_max_key(9, 1 * 6 + 2); s.w = 18; s.area = 2;      // maximum at (1, 2), upsample 3: the centre cells 4 and 7
    rc::cnt_finish_fine(rc::CNT_MAX, s, 6, 3, &fr, &fc);
    bad += !(fr == 4 && fc == 7); ++n;
    s.a = rc::cnt_max_key(65535, 65534u * 65535u + 65534u);                            // the last pixel of the largest frame, upsample 2: 131068.5 -> 131068
    rc::cnt_finish_fine(rc::CNT_MAX, s, 65535, 2, &fr, &fc);
    bad += !(fr == 131068 && fc == 131068); ++n;
    group("cnt_finish_fine", bad, n);

    if (!failures) printf("ok\n");
    return failures;
}
