// shift_window_check.cpp - the host build of pyrecode_amd/csrc/rc_shift.h as a stand-alone program (tests/test_aligned_sum_cpu.py builds it,
// also under AddressSanitizer / UBSan): for every case the output words a shifted frame becomes - two source words funnel-shifted, the column
// mask applied, as k_sum_shift forms them - against a loop over the output pixels that looks the source pixel up by row and column.
// Shapes (nx x ny) 1x1, 21x3, 64x2, 65x2, 130x127; every dx in [-nx - 1, nx + 1] and the int32 extremes; a spread of dy with +-ny and the
// extremes.  Prints one line per case - the offset, the funnel, whether anything survives, the masks of four words: what
// tests/aligned_sum_model.py restates - and "ok"; the exit status is 1 when a case was wrong.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../../pyrecode_amd/csrc/rc_shift.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t next64()
{
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// the frame's bitmap as the kernels read it: word a, zero outside the frame (a signed index: a window may start before it)
static uint64_t word_at(const std::vector<uint64_t> &bm, int64_t a) { return a < 0 || a >= (int64_t)bm.size() ? 0 : bm[(size_t)a]; }

static int check_case(const std::vector<uint64_t> &bm, uint32_t nx, uint32_t ny, int32_t dy, int32_t dx)
{
    const uint64_t N = (uint64_t)nx * ny, words = (N + 63) / 64;
    const int64_t s = rc::shift_offset(dy, dx, nx);
    int64_t q;
    uint32_t sh;
    rc::shift_funnel(s, &q, &sh);
    const bool in = rc::shift_in_view(dy, dx, nx, ny);
    int bad = 0;
    if (sh >= 64 || 64 * q + (int64_t)sh != -s) bad = 1;
    for (uint64_t i = 0; i < words; ++i) {
        const int64_t a = (int64_t)i + q;
        const uint64_t win = rc::shift_window(word_at(bm, a), word_at(bm, a + 1), sh);
        const uint64_t got = in ? win & rc::shift_col_mask((uint32_t)((i * 64) % nx), nx, dx) : 0;
        uint64_t want = 0;
        for (uint32_t j = 0; j < 64; ++j) {
            const uint64_t p = i * 64 + j;
            if (p >= N) break;
            const int64_t r = (int64_t)(p / nx) - dy, c = (int64_t)(p % nx) - dx;
            if (r < 0 || r >= (int64_t)ny || c < 0 || c >= (int64_t)nx) continue;
            const uint64_t src = (uint64_t)r * nx + (uint64_t)c;
            want |= ((bm[src >> 6] >> (src & 63)) & 1ull) << j;
        }
        const uint64_t live = N - i * 64 >= 64 ? ~0ull : (1ull << (N - i * 64)) - 1ull;     // (output pixels at or past N are dropped by the flush)
        if ((got & live) != want) bad = 1;
    }
    const uint64_t picks[4] = {0, words > 1 ? 1u : 0u, words / 2, words - 1};
    printf("%u %u %d %d %lld %lld %u %d", nx, ny, dy, dx, (long long)s, (long long)q, sh, in ? 1 : 0);
    for (uint64_t i : picks) printf(" %016llx", (unsigned long long)rc::shift_col_mask((uint32_t)((i * 64) % nx), nx, dx));
    printf("\n");
    return bad;
}

int main()
{
    const uint32_t shapes[5][2] = {{1, 1}, {21, 3}, {64, 2}, {65, 2}, {130, 127}};
    int failures = 0;
    for (const auto &shape : shapes) {
        const uint32_t nx = shape[0], ny = shape[1];
        const uint64_t N = (uint64_t)nx * ny, words = (N + 63) / 64;
        // a dense random frame (every second pixel), the bits at or past N clear - as expand_word hands them out
        std::vector<uint64_t> bm(words);
        for (uint64_t i = 0; i < words; ++i) bm[i] = next64();
        if (N % 64) bm[words - 1] &= (1ull << (N % 64)) - 1ull;
        const int64_t cand[15] = {0, 1, -1, 2, -3, (int64_t)ny - 1, -((int64_t)ny - 1), ny, -(int64_t)ny, (int64_t)ny + 1, -(int64_t)ny - 5, 64, -64, INT32_MIN, INT32_MAX};
        std::vector<int64_t> dys;
        for (int64_t dy : cand) {
            bool seen = false;
            for (int64_t e : dys) seen = seen || e == dy;
            if (!seen) dys.push_back(dy);
        }
        for (int64_t dy : dys) {
            for (int64_t dx = -(int64_t)nx - 1; dx <= (int64_t)nx + 1; ++dx) failures += check_case(bm, nx, ny, (int32_t)dy, (int32_t)dx);
            failures += check_case(bm, nx, ny, (int32_t)dy, INT32_MIN);
            failures += check_case(bm, nx, ny, (int32_t)dy, INT32_MAX);
        }
    }
    if (failures) { printf("%d cases wrong\n", failures); return 1; }
    printf("ok\n");
    return 0;
}
