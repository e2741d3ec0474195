// rc_dense.h - dense frame batches (rc_dense.hip): the arithmetic of a region - which blocks of a frame hold its pixels, and which output cell
// a source pixel goes to - host and device, and the launcher of the kernel.  The arithmetic compiles as plain C++
// (tests/native/dense_region_check.cpp runs it under the sanitizers against a double loop).
//
// Reference: ReCoDeReader.get_sub_volume is a stub there (pyrecode/recode_reader.py:185-186); what callers do instead is frame.toarray()
// per frame on the host (pyrecode/utils/viewer.py:65-68).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RC_DENSE_HD __host__ __device__ inline
#else
#define RC_DENSE_HD inline
#endif

namespace rc {

constexpr uint32_t DENSE_BLOCK_PIXELS = 256 * 64;      // pixels, in linear row-major order, a workgroup of the expand kernels owns (WG words)

// Output cell (j, i), j < h, i < w, is source pixel (y0 + j * step_y, x0 + i * step_x).  Checked by the entry points: steps and sizes are
// not 0, x0 + (w - 1) * step_x < nx, y0 + (h - 1) * step_y < ny; nx, ny <= 65535 (a pixel's linear index fits 32 bits).
struct DenseRegion {
    uint32_t x0, y0, w, h, step_x, step_y;
};

// the blocks that hold the region's first and its last pixel: every pixel of the region lies in a block of [*first, *last], and both ends
// hold one (the blocks in between may hold none: a region narrower than the frame)
RC_DENSE_HD void dense_block_range(uint32_t nx, const DenseRegion &r, uint32_t *first, uint32_t *last)
{
    const uint64_t p_first = (uint64_t)r.y0 * nx + r.x0;
    const uint64_t p_last = ((uint64_t)r.y0 + (uint64_t)(r.h - 1) * r.step_y) * nx + r.x0 + (uint64_t)(r.w - 1) * r.step_x;
    *first = (uint32_t)(p_first / DENSE_BLOCK_PIXELS);
    *last = (uint32_t)(p_last / DENSE_BLOCK_PIXELS);
}

// source pixel (row, col) -> its cell j * w + i of a frame's output, or -1: off the region or off the step lattice
RC_DENSE_HD int64_t dense_cell(const DenseRegion &r, uint32_t row, uint32_t col)
{
    if (row < r.y0 || col < r.x0) return -1;
    const uint32_t dy = row - r.y0, dx = col - r.x0;
    const uint32_t j = r.step_y == 1 ? dy : dy / r.step_y, i = r.step_x == 1 ? dx : dx / r.step_x;
    if (j >= r.h || i >= r.w || j * r.step_y != dy || i * r.step_x != dx) return -1;
    return (int64_t)j * r.w + i;
}

// whole rows at steps of 1: a frame's output is ONE linear range of its pixels, [y0 * nx, (y0 + h) * nx), in the same order
RC_DENSE_HD bool dense_is_linear(uint32_t nx, const DenseRegion &r) { return r.x0 == 0 && r.w == nx && r.step_x == 1 && r.step_y == 1; }

}  // namespace rc

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
namespace rc {
// Behind launch_expand_batch_count on the same stream (blk_off, and *err as the gate: nothing is written once it is set): out[f][j][i],
// f < n, cells of cell_bytes (1, 2 or 4) bytes, frames back to back - level 1: the pixel's d-bit field (d <= 8 * cell_bytes), other levels 1
// per set pixel; an unset pixel's cell is 0.  Every cell is written exactly once.  out is cell-aligned, no more.
void launch_expand_batch_dense(const uint8_t *bm, uint64_t bm_stride, uint64_t nb8, uint64_t N, uint32_t nx, uint32_t n, const uint32_t *blk_off,
                               const uint8_t *pv, uint64_t pv_stride, const uint32_t *pv_bytes, uint32_t d, uint32_t level, const DenseRegion &region,
                               uint32_t cell_bytes, void *out, const int *err, hipStream_t s);
}  // namespace rc
#endif
