// rc_bins.h - binned frame traces (rc_bins.hip): per frame and bin of a label map the number of set pixels and the sum of their values -
// the bins, the histogram a workgroup keeps in LDS, the chunking and the workspace of rc_bins_frames - host and device -, and the launchers
// of the kernels.  The arithmetic compiles as plain C++ (tests/native/bins_index_check.cpp runs it under the sanitizers against a
// restatement in Python integers).
//
// Reference: none in pyrecode - a caller's loop around ReCoDeReader.get_frame and np.bincount over labels[rows, cols] (a radial profile, an
// annular or segmented detector, an ROI grid).
#pragma once
#include <stdint.h>
#include "rc_corr.h"

namespace rc {

constexpr uint32_t BINS_MAX = 4096;          // bins a handle may have
constexpr uint16_t BINS_IGNORE = 0xFFFF;     // the label of a pixel in no bin
constexpr uint32_t BINS_PLANES = 2;          // per frame: plane 0 the set pixels of every bin, plane 1 the sum of their values
constexpr uint32_t BINS_TARGET_WGS = CORR_TARGET_WGS;   // workgroups a launch aims for while the partial rows allow it
// What the partial rows of the workgroups AIMED FOR may take: 32 MiB.  A row is 2 B int64, 64 KiB at B = 4096, so the target falls from
// 4096 workgroups (B <= 512) to 512 (B = 4096) - still two for each of the 256 CUs, which hold three of the largest histogram each.
// 32 MiB is what the neighbouring kinds already keep in the same workspace at 4096 x 4096 and 64 frames (the correlations' rows at R = 16
// are 35.7 MB, the traces' with 16 planes 10.5 MB), an eighth of the 256 MiB last-level cache, so a row that is written once and read once
// need not go to memory in between; 4096 workgroups at B = 4096 would be 272 MB.
constexpr uint64_t BINS_PARTIAL_BUDGET = 32ull << 20;

// No batch is refused for wrap: a cell is at most vmax * (set pixels of a frame) <= 65535 * 65535 * 65535 < 2^48, far inside an int64 -
// and a workgroup's uint32 count at most nx * ny < 2^32.
static_assert(65535ull * 65535ull * 65535ull < (1ull << 48), "a bin's sum fits 48 bits");
static_assert(65535ull * 65535ull < (1ull << 32), "a bin's count fits a uint32");

// The histogram tiers: the kernel is instantiated for 256, 1024 and 4096 bins, so that a handle of few bins keeps the occupancy
RC_TRACE_HD uint32_t bins_tier(uint32_t B) { return B <= 256u ? 256u : B <= 1024u ? 1024u : BINS_MAX; }
// LDS bytes of the histogram of a workgroup whose handle has B bins: a uint32 count per bin of its tier and, at level 1 alone, a uint64
// sum (levels 2 and 3: the sum IS the count) - 48 KiB at B = 4096 and level 1.  (The scan's 20 bytes come on top.)
RC_TRACE_HD uint32_t bins_lds_bytes(uint32_t B, uint32_t level) { return bins_tier(B) * (level == 1 ? 12u : 4u); }

// workgroups a launch aims for: BINS_TARGET_WGS, or as many rows of 2 B int64 as fit the budget
RC_TRACE_HD uint32_t bins_target_wgs(uint32_t B)
{
    const uint64_t rows = BINS_PARTIAL_BUDGET / ((uint64_t)BINS_PLANES * B * 8ull);      // (1 <= B <= 4096: at least 512)
    return rows < BINS_TARGET_WGS ? (uint32_t)rows : BINS_TARGET_WGS;
}
// rc_corr.h's chunking with that target: a workgroup walks `blocks per chunk` consecutive blocks of WG bitmap words of ONE frame with its
// histogram in LDS and stores one row of 2 B partial sums - at most ceil(bins_target_wgs(B) / n) chunks a frame, whatever the frame's size
RC_TRACE_HD uint32_t bins_blocks_per_chunk(uint32_t nblk, uint32_t n, uint32_t B)
{
    const uint32_t target = bins_target_wgs(B);
    uint32_t want = (target + n - 1u) / n;
    if (want > nblk) want = nblk;
    if (want == 0) want = 1;
    return nblk ? (nblk + want - 1u) / want : 1u;
}
RC_TRACE_HD uint32_t bins_chunks(uint32_t nblk, uint32_t n, uint32_t B)
{
    const uint32_t bpc = bins_blocks_per_chunk(nblk, n, B);
    return nblk ? (nblk + bpc - 1u) / bpc : 1u;
}
// bytes of the partial sums launch_expand_batch_bins needs at `partials`: int64[n][chunks][2][B]
//   <= (n + bins_target_wgs(B)) * 2 B * 8 <= n * 16 B + BINS_PARTIAL_BUDGET
// - the output's own size plus the budget, whatever the frame's size.  wg: the workgroup's threads (rc_device.h: WG)
RC_TRACE_HD uint64_t bins_workspace_bytes(uint64_t nb8, uint32_t n, uint32_t B, uint32_t wg = 256)
{
    const uint32_t nblk = (uint32_t)((nb8 + wg - 1) / wg);
    return (uint64_t)n * bins_chunks(nblk, n, B) * BINS_PLANES * B * 8ull;
}

}  // namespace rc

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
namespace rc {
// Behind launch_expand_batch_count on the same stream (blk_off, and *err as the gate: nothing is written once it is set):
// out[f][0][b] = frame f's set pixels with labels[row * nx + col] == b, out[f][1][b] = the sum of their values (level 1: the pixel's d-bit
// field, d <= 16; other levels 1).  labels: the handle's uint16[ny * nx], every one below B or BINS_IGNORE.  partials:
// bins_workspace_bytes.  Every cell of out is written exactly once.
void launch_expand_batch_bins(const uint8_t *bm, uint64_t bm_stride, uint64_t nb8, uint64_t N, uint32_t n, const uint32_t *blk_off, const uint8_t *pv,
                              uint64_t pv_stride, const uint32_t *pv_bytes, uint32_t d, uint32_t level, const uint16_t *labels, uint32_t B,
                              int64_t *partials, int64_t *out, const int *err, hipStream_t s);
// *top = max(*top, the largest label that is not BINS_IGNORE) (the caller clears it first)
void launch_bins_label_max(const uint16_t *labels, uint64_t N, uint32_t *top, hipStream_t s);
}  // namespace rc
#endif
