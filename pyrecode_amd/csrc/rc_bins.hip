// rc_bins.hip - binned frame traces (rc_bins_frames): a batch's decoded bitmaps and value streams and a label map -> out[n][2][B], per
// frame and bin the number of set pixels and the sum of their values (gfx950).
//
//   radial profiles, annular / segmented detectors, ROI grids per frame
//                                     nothing in pyrecode: a caller's loop around ReCoDeReader.get_frame (pyrecode/recode_reader.py:379-471)
//                                     and np.bincount over labels[rows, cols]
#include "rc_bins.h"
#include "rc_expand.h"

#include <algorithm>

namespace rc {

// A workgroup owns a CHUNK of consecutive blocks of WG bitmap words of ONE frame - the shape of k_expand_corr_b; the launch is the plain
// one, workgroup L on chunk L % nchunk of frame L / nchunk: k_expand_corr_b's dealing ties chunk c to XCD c % 8, which measured SLOWER
// here - a pixel reads 2 bytes of the label map, not a window, and a frame of 12 chunks (B = 2896) left half the XCDs with half the work:
// 403 against 227 us a batch (profiles/bins_kernel_stats.md) - and keeps the chunk's histogram in LDS:
// a uint32 count per bin and, with SUMS (level 1), a uint64 sum; at levels 2 and 3 every value is 1 and the sum is the count.  TIER bins
// are reserved (256, 1024, 4096: the instantiation sizes the LDS, so a handle of few bins keeps the occupancy); B <= TIER of them are
// cleared, added to and stored.
//   Per block a thread does what k_expand_trace_b does - the word, with the next block's in flight; with SUMS block_excl_scan of the
//   popcounts and blk_off for its rank in the value stream (without: no scan, no barrier in the loop) - and walks the word's set pixels:
//   pixel k0 + bit costs ONE 2-byte load, labels[k0 + bit] - no row, no column.  Consecutive pixels of one label are summed in registers
//   (a run: label, count, sum) and a run that ends goes to LDS with non-returning integer adds.  Integer adds commute: the result is exact
//   whatever the order.  (Reducing a wave whose lanes all hold ONE bin first - B = 1, a large ROI - and adding once was built and measured:
//   no faster, with every pixel of 4096 x 4096 frames in one bin either; the lanes add for themselves.)
//   A label at or above B adds nothing: BINS_IGNORE, and - the handle has checked that there is no other - the bound of the LDS index.
//   At the end the workgroup stores its row partials[f][chunk][2][B] - every cell, also of an empty chunk: nobody clears anything -, and
//   k_corr_reduce adds a frame's rows.  No global atomics, no scratch.
// LDS: TIER * 4 (+ TIER * 8 with SUMS) + the scan's 20 B: 48 KiB + 20 B at most.  Writes nothing once *err is set.
template <uint32_t TIER, bool SUMS>
__global__ __launch_bounds__(WG) void k_expand_bins_b(const uint8_t *__restrict__ bm, uint64_t bm_stride, uint64_t nb8, uint64_t N, uint32_t nblk, uint32_t bpc,
                                                        uint32_t nchunk, const uint32_t *__restrict__ blk_off, const uint8_t *__restrict__ pv,
                                                        uint64_t pv_stride, const uint32_t *__restrict__ pv_bytes, uint32_t d, const uint16_t *__restrict__ labels,
                                                        uint32_t B, uint64_t *__restrict__ partials, const int *__restrict__ err)
{
    __shared__ uint32_t sm[WAVES + 1];
    __shared__ uint32_t s_cnt[TIER];
    __shared__ unsigned long long s_sum[SUMS ? TIER : 1];
    if (*err) return;   // (workgroup-uniform, as in k_expand_emit_b)
    const uint32_t t = threadIdx.x, f = blockIdx.x / nchunk, chunk = blockIdx.x - f * nchunk;
    if (B > TIER) return;                                               // (never: the launcher picks the tier)
    for (uint32_t b = t; b < B; b += WG) {
        s_cnt[b] = 0;
        if (SUMS) s_sum[b] = 0;
    }
    __syncthreads();
    const uint32_t dmask = SUMS ? (1u << d) - 1u : 0u;                   // (level 1: 1 <= d <= 16)
    const uint8_t *bmf = bm + f * bm_stride, *pix = pv + f * pv_stride;
    const uint64_t pix_bytes = SUMS ? pv_bytes[f] : 0;
    const uint32_t b0 = chunk * bpc, b1 = min(nblk, b0 + bpc);

    auto add = [&](uint32_t bin, uint32_t c, uint32_t sv) {             // (bin < B; non-returning LDS adds)
        (void)atomicAdd(&s_cnt[bin], c);
        if (SUMS) (void)atomicAdd(&s_sum[bin], (unsigned long long)sv);
    };

    uint64_t next = b0 < b1 ? expand_word(bmf, nb8, N, (uint64_t)b0 * WG + t) : 0;
    for (uint32_t b = b0; b < b1; ++b) {
        const uint64_t i = (uint64_t)b * WG + t;
        uint64_t bits = next;
        if (b + 1 < b1) next = expand_word(bmf, nb8, N, i + WG);         // (in flight across this block's barriers)
        uint32_t local = 0, tot;
        if (SUMS) local = block_excl_scan((uint32_t)__builtin_popcountll(bits), sm, &tot);   // (uniform)
        uint32_t cur = BINS_IGNORE, c = 0, sv = 0;                       // the run in hand: label, pixels, sum (<= 64 * 65535)
        if (bits) {
            uint64_t rank = SUMS ? (uint64_t)blk_off[(uint64_t)f * nblk + b] + local : 0;
            const uint16_t *lab = labels + i * 64;                       // (bits != 0: i < nb8, and every set bit is a pixel below N)
            for (; bits; bits &= bits - 1, ++rank) {
                const uint32_t l = lab[__builtin_ctzll(bits)];
                const uint32_t v = SUMS ? expand_field16(pix, pix_bytes, rank, d, dmask) : 1u;
                if (l != cur) {
                    if (c && cur < B) add(cur, c, sv);
                    cur = l; c = 0; sv = 0;
                }
                ++c;
                sv += v;
            }
        }
        if (c && cur < B) add(cur, c, sv);
    }
    __syncthreads();
    uint64_t *row = partials + ((uint64_t)f * nchunk + chunk) * BINS_PLANES * B;
    for (uint32_t b = t; b < B; b += WG) {
        const uint64_t cnt = s_cnt[b];
        row[b] = cnt;
        row[B + b] = SUMS ? (uint64_t)s_sum[b] : cnt;
    }
}

void launch_expand_batch_bins(const uint8_t *bm, uint64_t bm_stride, uint64_t nb8, uint64_t N, uint32_t n, const uint32_t *blk_off, const uint8_t *pv,
                              uint64_t pv_stride, const uint32_t *pv_bytes, uint32_t d, uint32_t level, const uint16_t *labels, uint32_t B,
                              int64_t *partials, int64_t *out, const int *err, hipStream_t s)
{
    const uint32_t nblk = (uint32_t)((nb8 + WG - 1) / WG);
    const uint32_t bpc = bins_blocks_per_chunk(nblk, n, B), nchunk = bins_chunks(nblk, n, B), tier = bins_tier(B);
    uint64_t *part = reinterpret_cast<uint64_t *>(partials);
    const dim3 grid(n * nchunk);                                        // (at most n + bins_target_wgs(B) workgroups)
    auto go = [&](auto c, auto sums) {
        hipLaunchKernelGGL((k_expand_bins_b<(uint32_t)decltype(c)::value, decltype(sums)::value != 0>), grid, dim3(WG), 0, s, bm, bm_stride, nb8, N, nblk, bpc,
                           nchunk, blk_off, pv, pv_stride, pv_bytes, d, labels, B, part, err);
    };
    auto pick = [&](auto sums) {
        if (tier == 256u) go(int_c<256>{}, sums);
        else if (tier == 1024u) go(int_c<1024>{}, sums);
        else go(int_c<(int)BINS_MAX>{}, sums);
    };
    if (level == 1) pick(int_c<1>{});
    else pick(int_c<0>{});
    launch_rows_reduce(partials, nchunk, BINS_PLANES * B, n, out, err, s);
}

// ---- a handle's labels (rc_bins_create) -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(WG) void k_bins_label_max(const uint16_t *__restrict__ labels, uint64_t N, uint32_t *__restrict__ top)
{
    const uint64_t stride = (uint64_t)gridDim.x * WG;
    uint32_t a = 0;
    for (uint64_t p = (uint64_t)blockIdx.x * WG + threadIdx.x; p < N; p += stride) {
        const uint32_t l = labels[p];
        if (l != BINS_IGNORE) a = max(a, l);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) a = max(a, (uint32_t)__shfl_xor((int)a, d));
    if ((threadIdx.x & 63u) == 0 && a) (void)atomicMax(top, a);
}
void launch_bins_label_max(const uint16_t *labels, uint64_t N, uint32_t *top, hipStream_t s)
{
    hipLaunchKernelGGL(k_bins_label_max, dim3((uint32_t)std::min<uint64_t>(2048, (N + WG - 1) / WG)), dim3(WG), 0, s, labels, N, top);
}

}  // namespace rc
