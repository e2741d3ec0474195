// dense_region_check.cpp - the host build of pyrecode_amd/csrc/rc_dense.h as a stand-alone program (tests/test_dense_plan_cpu.py builds it,
// also under AddressSanitizer / UBSan): dense_cell, dense_block_range and dense_is_linear against a double loop over the region's cells.
// Every region of the small shapes with steps 1..4, a seeded sample of the two shapes that span blocks.
// Prints one line per shape and "ok"; the exit status is the number of shapes with a wrong answer.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../../pyrecode_amd/csrc/rc_dense.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t next64()
{
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static std::vector<int64_t> want;

// 1 if anything about this region is wrong
static uint64_t region_differs(uint32_t ny, uint32_t nx, const rc::DenseRegion &r)
{
    want.assign((size_t)ny * nx, -1);
    uint64_t p_min = ~0ull, p_max = 0;
    for (uint32_t j = 0; j < r.h; ++j)
        for (uint32_t i = 0; i < r.w; ++i) {
            const uint64_t p = (uint64_t)(r.y0 + j * r.step_y) * nx + r.x0 + i * r.step_x;
            want[p] = (int64_t)j * r.w + i;
            if (p < p_min) p_min = p;
            if (p > p_max) p_max = p;
        }
    uint64_t bad = 0;
    for (uint32_t row = 0; row < ny; ++row)
        for (uint32_t col = 0; col < nx; ++col)
            if (rc::dense_cell(r, row, col) != want[(size_t)row * nx + col]) bad = 1;
    uint32_t first = 0, last = 0;
    rc::dense_block_range(nx, r, &first, &last);
    if (first != p_min / rc::DENSE_BLOCK_PIXELS || last != p_max / rc::DENSE_BLOCK_PIXELS) bad = 1;
    const bool linear = rc::dense_is_linear(nx, r);
    if (linear != (r.x0 == 0 && r.w == nx && r.step_x == 1 && r.step_y == 1)) bad = 1;
    if (linear)      // the frame's output is the linear range [y0 * nx, (y0 + h) * nx) of its pixels, in order
        for (uint64_t p = 0; p < (uint64_t)ny * nx; ++p) {
            const uint64_t a = (uint64_t)r.y0 * nx, b = a + (uint64_t)r.w * r.h;
            if (want[p] != (p >= a && p < b ? (int64_t)(p - a) : -1)) bad = 1;
        }
    return bad;
}

static int failures = 0;
static void report(uint32_t ny, uint32_t nx, const char *how, uint64_t bad, uint64_t n)
{
    printf("(%u, %u) %-14s %llu regions, %llu wrong\n", ny, nx, how, (unsigned long long)n, (unsigned long long)bad);
    if (bad) ++failures;
}

static void all_regions(uint32_t ny, uint32_t nx)
{
    uint64_t bad = 0, n = 0;
    for (uint32_t sy = 1; sy <= 4; ++sy)
        for (uint32_t sx = 1; sx <= 4; ++sx)
            for (uint32_t y0 = 0; y0 < ny; ++y0)
                for (uint32_t h = 1; y0 + (h - 1) * sy < ny; ++h)
                    for (uint32_t x0 = 0; x0 < nx; ++x0)
                        for (uint32_t w = 1; x0 + (w - 1) * sx < nx; ++w, ++n) bad += region_differs(ny, nx, rc::DenseRegion{x0, y0, w, h, sx, sy});
    report(ny, nx, "all regions", bad, n);
}

static void sampled_regions(uint32_t ny, uint32_t nx, uint32_t count)
{
    uint64_t bad = 0, n = 0;
    for (uint32_t k = 0; k < count; ++k, ++n) {
        rc::DenseRegion r;
        r.step_y = 1 + (uint32_t)(next64() % 4);
        r.step_x = 1 + (uint32_t)(next64() % 4);
        r.y0 = (uint32_t)(next64() % ny);
        r.x0 = k % 3 == 0 ? 0u : (uint32_t)(next64() % nx);
        const uint32_t h_max = (ny - 1 - r.y0) / r.step_y + 1, w_max = (nx - 1 - r.x0) / r.step_x + 1;
        r.h = 1 + (uint32_t)(next64() % h_max);
        r.w = k % 3 == 0 ? w_max : 1 + (uint32_t)(next64() % w_max);      // (a third: whole rows - linear where the steps are 1)
        if (k % 6 == 0) r.step_x = r.step_y = 1, r.w = nx, r.h = 1 + (uint32_t)(next64() % (ny - r.y0));
        bad += region_differs(ny, nx, r);
    }
    report(ny, nx, "seeded sample", bad, n);
}

int main()
{
    all_regions(1, 1);
    all_regions(3, 21);
    all_regions(5, 64);
    all_regions(5, 65);
    sampled_regions(127, 130, 600);
    sampled_regions(2, 20000, 300);
    if (!failures) printf("ok\n");
    return failures;
}
