// rc_trace.h - frame traces (rc_trace.hip): the no-wrap rule of rc_trace_frames - whether a column of a frame's trace can pass 2^63 - 1 -
// host and device, and the launchers of the kernels.  The arithmetic compiles as plain C++ (tests/native/trace_bound_check.cpp runs it
// under the sanitizers against a restatement in Python integers).
//
// Reference: the dose rate the converter prints per frame (pyrecode/utils/converters.py:108-111) and the loop a caller writes around
// ReCoDeReader.get_frame for anything else per frame; there the sums are Python / numpy integers on the host.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RC_TRACE_HD __host__ __device__ inline
#else
#define RC_TRACE_HD inline
#endif

namespace rc {

constexpr uint32_t TRACE_MAX_PLANES = 16;
constexpr uint32_t TRACE_MOMENTS = 4;                  // count, sum v, sum v * row, sum v * col: the columns in front of the weighted ones
constexpr uint64_t TRACE_LIMIT = 0x7FFFFFFFFFFFFFFFull;   // what an int64 cell holds

// |w| of an int32 as uint32: INT32_MIN counts as 2^31
RC_TRACE_HD uint32_t trace_abs(int32_t w) { return w < 0 ? 0u - (uint32_t)w : (uint32_t)w; }

// the largest value a set pixel stores: the d-bit field at level 1 (1 <= d <= 16 here), 1 at levels 2 and 3
RC_TRACE_HD uint64_t trace_vmax(uint32_t level, uint32_t bit_depth) { return level == 1 ? (1ull << bit_depth) - 1ull : 1ull; }

// the set pixels a frame can hold: all of them - at level 1 no more than its packed value stream has fields for (k_expand_bases refuses a
// frame with more)
RC_TRACE_HD uint64_t trace_frame_pixels(uint32_t nx, uint32_t ny, uint32_t level, uint32_t bit_depth, uint32_t packed_bytes)
{
    const uint64_t N = (uint64_t)nx * ny;
    if (level != 1) return N;
    const uint64_t fields = 8ull * packed_bytes / bit_depth;
    return fields < N ? fields : N;
}

// a * vmax * pixels <= 2^63 - 1, by division: no product here can wrap
RC_TRACE_HD bool trace_column_fits(uint64_t a, uint64_t vmax, uint64_t pixels)
{
    if (a == 0 || vmax == 0 || pixels == 0) return true;
    if (a > TRACE_LIMIT / vmax) return false;
    return pixels <= TRACE_LIMIT / (a * vmax);
}

// the largest weight of any column: 1 (count, sum), ny - 1 (rows), nx - 1 (columns), maxabs of every plane
RC_TRACE_HD uint64_t trace_largest_weight(uint32_t nx, uint32_t ny, uint32_t k, const uint32_t *plane_bound)
{
    uint64_t a = 1;
    if (ny - 1 > a) a = ny - 1;
    if (nx - 1 > a) a = nx - 1;
    for (uint32_t m = 0; m < k; ++m)
        if (plane_bound[m] > a) a = plane_bound[m];
    return a;
}

// Whether every column of every frame of a batch stays within an int64: the rule is monotone in the weight and in the pixels, so the largest
// weight against the fullest frame decides.  sizes: uint32[n][3] as rc_expand_frames takes them ([3 f + 2] = bytes of the packed values).
RC_TRACE_HD bool trace_batch_fits(uint32_t nx, uint32_t ny, uint32_t level, uint32_t bit_depth, uint32_t k, const uint32_t *plane_bound,
                                  const uint32_t *sizes, uint32_t n)
{
    const uint64_t a = trace_largest_weight(nx, ny, k, plane_bound), vmax = trace_vmax(level, bit_depth);
    uint64_t pixels = 0;
    for (uint32_t f = 0; f < n; ++f) {
        const uint64_t p = trace_frame_pixels(nx, ny, level, bit_depth, sizes[3 * (uint64_t)f + 2]);
        if (p > pixels) pixels = p;
    }
    return trace_column_fits(a, vmax, pixels);
}

// planes of the interleaved copy of the weights: k rounded up to whole 16-byte vectors of int32
RC_TRACE_HD uint32_t trace_padded_planes(uint32_t k) { return (k + 3u) & ~3u; }

}  // namespace rc

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
namespace rc {
// bytes of the partial sums launch_expand_batch_trace needs at `partials`: int64[n][blocks][4 + k]
uint64_t trace_workspace_bytes(uint64_t nb8, uint32_t n, uint32_t k);
// Behind launch_expand_batch_count on the same stream (blk_off, and *err as the gate: nothing is written once it is set): out[f][0 .. 4 + k)
// = set pixels, sum v, sum v * row, sum v * col, sum v * W_m[row][col] of frame f (level 1: v = the pixel's d-bit field, d <= 16; other
// levels 1).  weights: int32[ny * nx][trace_padded_planes(k)], pixel-major (NULL when k == 0).  Every cell of out is written exactly once.
void launch_expand_batch_trace(const uint8_t *bm, uint64_t bm_stride, uint64_t nb8, uint64_t N, uint32_t nx, uint32_t n, const uint32_t *blk_off,
                               const uint8_t *pv, uint64_t pv_stride, const uint32_t *pv_bytes, uint32_t d, uint32_t level, const int32_t *weights,
                               uint32_t k, int64_t *partials, int64_t *out, const int *err, hipStream_t s);
// plane m of a handle's weights, int32[N] in device memory, into the interleaved copy
void launch_trace_interleave(const int32_t *plane, uint64_t N, uint32_t m, uint32_t kp, int32_t *weights, hipStream_t s);
// *bound = max(*bound, maxabs(plane)) as uint32 (the caller clears it first)
void launch_trace_maxabs(const int32_t *plane, uint64_t N, uint32_t *bound, hipStream_t s);
}  // namespace rc
#endif
