// rc_calib.h - the per-column logic of the calibration kernels (rc_calib.hip), host and device: order statistics of one pixel's
// column of uint16 values by bitwise bisection, and its exact-integer moments.  Compiles as plain C++ (tests/native/calib_select_check.cpp
// runs it under the sanitizers); `Col` is anything with `uint32_t operator()(uint32_t i) const` returning value i of the column.
//
// Reference: pyrecode/utils/calibration.py - _median_std_nb (:48-57: np.median and np.std of every pixel over the frames) and
// _get_pixel_thresh_2 (:26-45: the mean of the (k+1)-th and k-th largest of the values above the pixel's median).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RC_CALIB_HD __host__ __device__ inline
#else
#define RC_CALIB_HD inline
#endif

namespace rc {

constexpr uint32_t CALIB_MAX_FRAMES = 65535;   // n * S2 - S1^2 fits 64 bits up to here (S2 <= n * 65535^2)

// The values of ascending ranks r and r + 1 (0-based; r < n) of a column of n uint16 values.  16 passes settle the bits of the rank-r
// value v from the top: among the values that share the prefix settled so far, those with the next bit clear come first.  What is left
// of r is then v's rank among the values EQUAL to v, `same` of them: rank r + 1 is v again while r + 1 < same, otherwise the smallest
// value above v (one more pass).  With r + 1 == n there is no second rank: hi = lo.
template <class Col>
RC_CALIB_HD void calib_select_pair(const Col &col, uint32_t n, uint32_t r, uint32_t &lo, uint32_t &hi)
{
    uint32_t prefix = 0, same = n;
    for (int b = 15; b >= 0; --b) {
        const uint32_t want = prefix >> b;           // (bit b still clear)
        uint32_t c = 0;
        for (uint32_t i = 0; i < n; ++i) c += ((col(i) >> b) == want) ? 1u : 0u;
        if (r < c) same = c;
        else { r -= c; same -= c; prefix |= 1u << b; }
    }
    lo = hi = prefix;
    if (r + 1 < same) return;
    uint32_t above = 0x10000u;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t v = col(i);
        if (v > prefix && v < above) above = v;
    }
    if (above != 0x10000u) hi = above;
}

// np.median of the column as 2 * median (an integer below 2^17): the middle value twice (odd n) or the sum of the two middle values
template <class Col>
RC_CALIB_HD uint32_t calib_median2(const Col &col, uint32_t n)
{
    uint32_t lo, hi;
    calib_select_pair(col, n, (n - 1) / 2, lo, hi);
    return (n & 1u) ? 2u * lo : lo + hi;
}

// np.std of the column (population) from exact integers: sqrt(n * S2 - S1^2) / n, one square root in double precision
template <class Col>
RC_CALIB_HD float calib_std(const Col &col, uint32_t n)
{
    uint64_t s1 = 0, s2 = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const uint64_t v = col(i);
        s1 += v;
        s2 += v * v;
    }
    const uint64_t num = (uint64_t)n * s2 - s1 * s1;
    return (float)(__builtin_sqrt((double)num) / (double)n);
}

// _get_pixel_thresh_2 for one pixel: the mean of the (k+1)-th and k-th largest values, defined when at least k + 1 values lie above the
// pixel's median `med` (the values above the median ARE the largest ones, so ranks among them are ranks of the column counted from the
// top: ascending ranks n - k - 1 and n - k).  Returns false - and leaves `acc` alone - where the reference's result is undefined.
template <class Col>
RC_CALIB_HD bool calib_top_pair(const Col &col, uint32_t n, float med, uint32_t k, float &acc)
{
    uint32_t above = 0;
    for (uint32_t i = 0; i < n; ++i) above += ((float)col(i) > med) ? 1u : 0u;
    if (k == 0 || k + 1 > above) return false;
    uint32_t lo, hi;
    calib_select_pair(col, n, n - k - 1, lo, hi);
    acc = ((float)lo + (float)hi) / 2.0f;
    return true;
}

}  // namespace rc
