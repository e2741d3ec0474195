// rc_shift.h - aligned views (rc_sum_add_frames_shifted, rc_expand.hip: k_sum_shift): the arithmetic of a frame that is added somewhere
// other than where it was recorded - host and device.  The arithmetic compiles as plain C++ (tests/native/shift_window_check.cpp runs it
// under the sanitizers against a loop over the pixels).
//
// Frame f carries (dy, dx): what the unshifted add puts into cell (r, c) goes to (r + dy, c + dx), and is dropped when that lies outside
// the view.  In the linear, row-major pixel index a translation is ONE constant offset s = dy * nx + dx, so the 64 output pixels of output
// word i are the 64 source bits that start at bit 64 * i - s of the frame's bitmap: two neighbouring source words, funnel-shifted.  What the
// offset cannot know is the row a bit came from - an output bit whose column c' fails dx <= c' < nx + dx holds a pixel of the neighbouring
// source row and is masked off.  With the column valid the source row is in range exactly when the source index is one of the frame's
// (0 <= p < ny * nx), and bits outside the frame read as zero anyway.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RC_SHIFT_HD __host__ __device__ inline
#else
#define RC_SHIFT_HD inline
#endif

namespace rc {

// s = dy * nx + dx: nx <= 65535 and both shifts are int32, so |s| < 2^48
RC_SHIFT_HD int64_t shift_offset(int32_t dy, int32_t dx, uint32_t nx) { return (int64_t)dy * (int64_t)nx + (int64_t)dx; }

// whether anything of a frame of ny x nx survives the shift
RC_SHIFT_HD bool shift_in_view(int32_t dy, int32_t dx, uint32_t nx, uint32_t ny)
{
    return (int64_t)dy < (int64_t)ny && (int64_t)dy > -(int64_t)ny && (int64_t)dx < (int64_t)nx && (int64_t)dx > -(int64_t)nx;
}

// Output word i starts at source bit 64 * i - s = 64 * (i + *word) + *bit with 0 <= *bit < 64: floor division and a non-negative
// modulus of -s (C++'s own round towards zero)
RC_SHIFT_HD void shift_funnel(int64_t s, int64_t *word, uint32_t *bit)
{
    const int64_t m = -s;
    int64_t q = m / 64, r = m % 64;
    if (r < 0) { r += 64; --q; }
    *word = q;
    *bit = (uint32_t)r;
}

// 64 bits from bit `bit` of the pair (w0 = the word the window starts in, w1 = the one behind it)
RC_SHIFT_HD uint64_t shift_window(uint64_t w0, uint64_t w1, uint32_t bit) { return bit ? (w0 >> bit) | (w1 << (64u - bit)) : w0; }

// The output bits of a word whose column survives: bit j is output pixel 64 * i + j, c0 = (64 * i) % nx the column of bit 0; kept iff
// max(dx, 0) <= column < min(nx, nx + dx).  A word spans 64 / nx + 2 rows at most, and the mask is built per row segment.
RC_SHIFT_HD uint64_t shift_col_mask(uint32_t c0, uint32_t nx, int32_t dx)
{
    const int64_t lo = dx > 0 ? (int64_t)dx : 0, hi = dx < 0 ? (int64_t)nx + (int64_t)dx : (int64_t)nx;
    if (lo >= hi) return 0;
    uint64_t mask = 0;
    uint32_t pos = 0, c = c0;
    while (pos < 64) {
        const uint32_t seg = (nx - c) < (64u - pos) ? (nx - c) : (64u - pos);     // bits pos .. pos + seg - 1 are columns c .. c + seg - 1
        const int64_t a = lo > (int64_t)c ? lo : (int64_t)c, b = hi < (int64_t)c + seg ? hi : (int64_t)c + seg;
        if (b > a) {
            const uint32_t len = (uint32_t)(b - a), at = pos + (uint32_t)(a - (int64_t)c);
            mask |= (len >= 64 ? ~0ull : ((1ull << len) - 1ull)) << at;
        }
        pos += seg;
        c = 0;
    }
    return mask;
}

}  // namespace rc
