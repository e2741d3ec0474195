// rc_corr.h - per-frame correlation surfaces (rc_corr.hip): the window, the zero-bordered copy of the reference, the accumulators a lane
// keeps and the workspace of rc_corr_frames - host and device -, and the launchers of the kernels.  The no-wrap rule is rc_trace.h's
// (trace_column_fits), asked here with the reference's maxabs as the one weight.  The arithmetic compiles as plain C++
// (tests/native/corr_index_check.cpp runs it under the sanitizers against a restatement in Python integers).
//
// Reference: none in pyrecode - the caller's drift estimation around ReCoDeReader.get_frame (a whole-frame FFT per fraction); here the
// frames are sparse and the drift is a few pixels, so the surface is summed directly over a window of (2 R + 1)^2 offsets.
#pragma once
#include <stdint.h>
#include "rc_trace.h"

namespace rc {

constexpr uint32_t CORR_MAX_RADIUS = 16;
constexpr uint32_t CORR_TARGET_WGS = 4096;   // workgroups a launch aims for: the partial rows grow with THIS, not with the frame
constexpr uint32_t CORR_XCDS = 8;            // chunks c and c + 8 go to workgroups 8 apart in launch order (one XCD's L2 under round-robin dealing: speed only)

// side and cells of the window of radius R
RC_TRACE_HD uint32_t corr_side(uint32_t radius) { return 2u * radius + 1u; }
RC_TRACE_HD uint32_t corr_cells(uint32_t radius) { return corr_side(radius) * corr_side(radius); }
// int64 accumulators a lane keeps when a wave's 64 lanes own the cells: ceil(S^2 / 64) - 1 up to R = 3, 5 at R = 8, 18 at R = 16 (1089 cells)
RC_TRACE_HD uint32_t corr_lane_cells(uint32_t radius) { return (corr_cells(radius) + 63u) / 64u; }

// the reference as the handle keeps it: (ny + 2 R) x (nx + 2 R) with a border of R zeros, so a set pixel's whole window is inside it
RC_TRACE_HD uint32_t corr_padded_nx(uint32_t nx, uint32_t radius) { return nx + 2u * radius; }
RC_TRACE_HD uint64_t corr_padded_cells(uint32_t nx, uint32_t ny, uint32_t radius) { return (uint64_t)(nx + 2u * radius) * (ny + 2u * radius); }
// where the window of the pixel (row, col) starts in the padded copy: T[row - R][col - R] sits at padded (row, col)
RC_TRACE_HD uint64_t corr_window_base(uint32_t row, uint32_t col, uint32_t nx, uint32_t radius) { return (uint64_t)row * corr_padded_nx(nx, radius) + col; }
// ... and cell c = (dy + R) * S + (dx + R) of that window, from the base
RC_TRACE_HD uint32_t corr_cell_offset(uint32_t cell, uint32_t nx, uint32_t radius)
{
    const uint32_t S = corr_side(radius);
    return (cell / S) * corr_padded_nx(nx, radius) + cell % S;
}

// A workgroup walks `blocks per chunk` consecutive blocks of WG bitmap words of ONE frame with its accumulators in registers and stores one
// row of S^2 partial sums: chunks = ceil(nblk / ceil(nblk / want)), want = min(nblk, ceil(CORR_TARGET_WGS / n)) - at most
// ceil(CORR_TARGET_WGS / n) of them, whatever the frame's size
RC_TRACE_HD uint32_t corr_blocks_per_chunk(uint32_t nblk, uint32_t n)
{
    uint32_t want = (CORR_TARGET_WGS + n - 1u) / n;
    if (want > nblk) want = nblk;
    if (want == 0) want = 1;
    return nblk ? (nblk + want - 1u) / want : 1u;
}
RC_TRACE_HD uint32_t corr_chunks(uint32_t nblk, uint32_t n)
{
    const uint32_t bpc = corr_blocks_per_chunk(nblk, n);
    return nblk ? (nblk + bpc - 1u) / bpc : 1u;
}
// bytes of the partial sums launch_expand_batch_corr needs at `partials`: int64[n][chunks][S^2] <= (n + CORR_TARGET_WGS) * S^2 * 8.
// wg: the workgroup's threads (rc_device.h: WG)
RC_TRACE_HD uint64_t corr_workspace_bytes(uint64_t nb8, uint32_t n, uint32_t radius, uint32_t wg = 256)
{
    const uint32_t nblk = (uint32_t)((nb8 + wg - 1) / wg);
    return (uint64_t)n * corr_chunks(nblk, n) * corr_cells(radius) * 8ull;
}

// Whether every cell of every frame's surface stays within an int64: |cell| <= max|T| * vmax * P_f, the trace rule with one weight
RC_TRACE_HD bool corr_batch_fits(uint32_t nx, uint32_t ny, uint32_t level, uint32_t bit_depth, uint32_t bound, const uint32_t *sizes, uint32_t n)
{
    uint64_t pixels = 0;
    for (uint32_t f = 0; f < n; ++f) {
        const uint64_t p = trace_frame_pixels(nx, ny, level, bit_depth, sizes[3 * (uint64_t)f + 2]);
        if (p > pixels) pixels = p;
    }
    return trace_column_fits(bound, trace_vmax(level, bit_depth), pixels);
}

}  // namespace rc

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
namespace rc {
// Behind launch_expand_batch_count on the same stream (blk_off, and *err as the gate: nothing is written once it is set):
// out[f][dy + R][dx + R] = sum over frame f's set pixels (row, col) of v * T[row + dy][col + dx] (level 1: v = the pixel's d-bit field,
// d <= 16; other levels 1; T outside the image 0).  padded: the handle's zero-bordered int32[ny + 2 R][nx + 2 R].  partials:
// corr_workspace_bytes.  Every cell of out is written exactly once.
void launch_expand_batch_corr(const uint8_t *bm, uint64_t bm_stride, uint64_t nb8, uint64_t N, uint32_t nx, uint32_t n, const uint32_t *blk_off,
                              const uint8_t *pv, uint64_t pv_stride, const uint32_t *pv_bytes, uint32_t d, uint32_t level, const int32_t *padded,
                              uint32_t radius, int64_t *partials, int64_t *out, const int *err, hipStream_t s);
// k_corr_reduce on its own: out[f][c] = sum over the chunks of partials[f][chunk][c] for n frames of rows of `ncells` cells, nothing once
// *err is set (rc_bins.hip's rows are added by it too)
void launch_rows_reduce(const int64_t *partials, uint32_t nchunk, uint32_t ncells, uint32_t n, int64_t *out, const int *err, hipStream_t s);
}  // namespace rc
#endif
