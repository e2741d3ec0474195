// rc_corr.hip - per-frame correlation surfaces (rc_corr_frames): a batch's decoded bitmaps and value streams and a reference image T ->
// out[n][S][S], S = 2 R + 1: per frame the overlap of its set pixels with T at every offset of the window (gfx950).
//
//   drift estimation per frame        nothing in pyrecode: a caller's loop around ReCoDeReader.get_frame (pyrecode/recode_reader.py:379-471)
//                                     and a whole-frame FFT per fraction
#include "rc_corr.h"
#include "rc_expand.h"

#include <algorithm>

namespace rc {

constexpr uint32_t CORR_STAGE = 2048;   // set pixels a workgroup collects in LDS before its waves walk them (16 KiB)

// A workgroup owns a CHUNK of consecutive blocks of WG bitmap words of ONE frame and keeps the window's S^2 sums across all of
// them.  Per block it does what k_expand_trace_b does - the word, with the next block's in flight; block_excl_scan of the popcounts; a
// thread's rank in the value stream = blk_off + its exclusive prefix (level 1) - but instead of summing, a thread writes its set pixels as
// (row << 16 | col, value) into an LDS stage at the same exclusive prefix.  Once the stage could not take the next block (or the chunk
// ends) the four waves walk it, wave w the entries w, w + 4, ..: the entry is wave-uniform (one LDS broadcast, then scalar registers),
// the 64 LANES own the window's cells - lane l the cells l, l + 64, .. < S^2, NACC = ceil(S^2 / 64) int64 accumulators, 18 at R = 16 -
// and cell (dy, dx) of pixel (row, col) is one dword of the zero-bordered reference at base(row, col) + (dy + R) * (nx + 2 R) + (dx + R):
// no bounds test, and for a fixed dy the lanes of consecutive dx read consecutive dwords (a wave instruction touches ceil(64 / S) + 1 rows
// of T, each S dwords wide).  A pixel costs a lane one load and one 64-bit multiply-add per accumulator.  The per-lane offsets are
// registers (NACC of them), the accumulators are indexed by constants only: no scratch.
//   A block with more set pixels than the stage holds (a full frame has 16384) goes through it in passes of CORR_STAGE ranks.
//   At the end the four waves' sums meet in LDS, one accumulator at a time (two buffers that alternate: one barrier each), and wave j & 3
//   stores cells 64 j .. 64 j + 63 of partials[f][chunk][S^2]; k_corr_reduce adds a frame's rows.  No atomics; every row is written, also
//   an all-zero one, so nobody clears anything.
// LDS: 16 KiB stage + 4 KiB hand-over + the scan's 20 B.  Writes nothing once *err is set.
template <uint32_t NACC>
__global__ __launch_bounds__(WG) void k_expand_corr_b(const uint8_t *__restrict__ bm, uint64_t bm_stride, uint64_t nb8, uint64_t N, uint32_t nx, uint32_t nblk,
                                                        uint32_t bpc, uint32_t nchunk, uint32_t n, const uint32_t *__restrict__ blk_off, const uint8_t *__restrict__ pv, uint64_t pv_stride,
                                                        const uint32_t *__restrict__ pv_bytes, uint32_t d, uint32_t level, const int32_t *__restrict__ padded,
                                                        uint32_t radius, uint64_t *__restrict__ partials, const int *__restrict__ err)
{
    __shared__ uint32_t sm[WAVES + 1];
    __shared__ u32x2 s_px[CORR_STAGE];
    __shared__ uint64_t s_red[2][WAVES][64];
    if (*err) return;   // (workgroup-uniform, as in k_expand_emit_b)
    const uint32_t t = threadIdx.x, wave = t >> 6, lane = t & 63u;
    // Workgroup L of the launch takes frame (L / 8) % n of chunk (L / (8 n)) * 8 + L % 8: workgroups are dealt round-robin over the 8 XCDs,
    // so ONE XCD's L2 serves the workgroups of chunks c, c + 8, .. - of every frame in turn - and holds the rows of T under the few chunks
    // that are resident at a time, not all of T.  Placement is speed only; a chunk past the last one (the launch is padded to whole
    // eights) has no row to write and leaves.
    const uint32_t q = blockIdx.x / CORR_XCDS, f = q % n, chunk = (q / n) * CORR_XCDS + blockIdx.x % CORR_XCDS;
    if (chunk >= nchunk) return;
    const uint32_t S = corr_side(radius), S2 = S * S, nacc = (S2 + 63u) >> 6, nxp = corr_padded_nx(nx, radius);
    const uint32_t dmask = level == 1 ? (1u << d) - 1u : 0u;          // (level 1: 1 <= d <= 16)
    uint32_t off[NACC];
    int64_t acc[NACC];
#pragma unroll
    for (uint32_t j = 0; j < NACC; ++j) {
        const uint32_t cell = 64u * j + lane;
        off[j] = cell < S2 ? corr_cell_offset(cell, nx, radius) : 0u;   // (a lane past the window reads the base and stores nothing)
        acc[j] = 0;
    }
    const uint8_t *bmf = bm + f * bm_stride, *pix = pv + f * pv_stride;
    const uint64_t pix_bytes = level == 1 ? pv_bytes[f] : 0;
    const uint32_t b0 = chunk * bpc, b1 = min(nblk, b0 + bpc);

    // the waves walk the first `fill` entries of the stage (between two barriers of the caller's)
    auto add = [&](u32x2 px) {
        const uint32_t rc = (uint32_t)__builtin_amdgcn_readfirstlane((int)px[0]);
        const int32_t v = __builtin_amdgcn_readfirstlane((int)px[1]);              // (below 2^16)
        const int32_t *w = padded + ((uint64_t)(rc >> 16) * nxp + (rc & 0xFFFFu));
#pragma unroll
        for (uint32_t j = 0; j < NACC; ++j)
            if (j < nacc) acc[j] += (int64_t)w[off[j]] * (int64_t)v;              // (uniform)
    };
    auto walk = [&](uint32_t fill) {      // (two entries a turn: the second one's loads do not wait for the first one's sums)
        uint32_t e = wave;
        for (; e + (uint32_t)WAVES < fill; e += 2u * WAVES) {
            const u32x2 p0 = s_px[e], p1 = s_px[e + (uint32_t)WAVES];
            add(p0);
            add(p1);
        }
        if (e < fill) add(s_px[e]);
    };

    uint32_t fill = 0;                                                   // entries staged and not walked (uniform)
    uint64_t next = b0 < b1 ? expand_word(bmf, nb8, N, (uint64_t)b0 * WG + t) : 0;
    for (uint32_t b = b0; b < b1; ++b) {
        const uint64_t i = (uint64_t)b * WG + t;
        const uint64_t word = next;
        if (b + 1 < b1) next = expand_word(bmf, nb8, N, i + WG);         // (in flight across this block's barriers)
        const uint32_t cnt = (uint32_t)__builtin_popcountll(word);
        uint32_t tot;
        const uint32_t local = block_excl_scan(cnt, sm, &tot);           // (uniform)
        if (tot == 0) continue;
        const bool whole = tot <= CORR_STAGE;
        if (fill && fill + tot > CORR_STAGE) {                           // no room behind what is staged: walk that first
            __syncthreads();
            walk(fill);
            __syncthreads();
            fill = 0;
        }
        const uint32_t k0 = i < nb8 ? (uint32_t)(i * 64) : 0u;           // the word's first pixel (frames have fewer than 2^32 pixels)
        const uint32_t row0 = k0 / nx, col0 = k0 - row0 * nx;
        const uint64_t rank0 = level == 1 ? (uint64_t)blk_off[(uint64_t)f * nblk + b] + local : 0;
        // ranks [lo, lo + CORR_STAGE) of the block go to the stage at `fill`: one pass unless the block alone overflows it
        for (uint32_t lo = 0; lo < tot; lo += CORR_STAGE) {
            uint64_t bits = word;
            uint32_t row = row0, col = col0, prev = 0, r = local;
            for (; bits; bits &= bits - 1, ++r) {
                const uint32_t bit = (uint32_t)__builtin_ctzll(bits);
                col += bit - prev;
                prev = bit;
                while (col >= nx) { col -= nx; ++row; }
                if (r - lo < CORR_STAGE) {                               // (r < lo wraps to a large number)
                    const uint32_t v = level == 1 ? expand_field16(pix, pix_bytes, rank0 + (r - local), d, dmask) : 1u;
                    u32x2 px;
                    px[0] = row << 16 | col; px[1] = v;
                    s_px[fill + (r - lo)] = px;
                }
            }
            if (whole) { fill += tot; break; }
            __syncthreads();
            walk(min(tot - lo, CORR_STAGE));
            __syncthreads();
        }
    }
    if (fill) {
        __syncthreads();
        walk(fill);
    }
    // the four waves' sums of accumulator j meet in s_red[j & 1]; wave j & 3 adds them and stores the cells 64 j + lane
    uint64_t *rowp = partials + ((uint64_t)f * nchunk + chunk) * S2;
#pragma unroll
    for (uint32_t j = 0; j < NACC; ++j) {
        if (j < nacc) {                                                  // (uniform)
            s_red[j & 1u][wave][lane] = (uint64_t)acc[j];
            __syncthreads();
            const uint32_t cell = 64u * j + lane;
            if (wave == (j & 3u) && cell < S2) {
                uint64_t x = 0;
#pragma unroll
                for (uint32_t w = 0; w < (uint32_t)WAVES; ++w) x += s_red[j & 1u][w][lane];
                rowp[cell] = x;
            }
        }
    }
}

// out[f][c] = sum over the chunks of partials[f][chunk][c]: a thread per cell, consecutive threads on consecutive words of every row.
// (k_trace_reduce's job for rows wider than a workgroup; that kernel and its callers are as they were.)  The only writer of `out`, every
// cell once; nothing once *err is set.  launch_rows_reduce is its launch on its own: rc_bins.hip's rows of 2 B cells are added by it too.
__global__ __launch_bounds__(WG) void k_corr_reduce(const uint64_t *__restrict__ partials, uint32_t nchunk, uint32_t ncells, int64_t *__restrict__ out,
                                                      const int *__restrict__ err)
{
    if (*err) return;
    const uint32_t f = blockIdx.x, c = blockIdx.y * WG + threadIdx.x;
    if (c >= ncells) return;
    const uint64_t *p = partials + (uint64_t)f * nchunk * ncells + c;
    uint64_t x = 0;
    for (uint32_t k = 0; k < nchunk; ++k) x += p[(uint64_t)k * ncells];
    out[(uint64_t)f * ncells + c] = (int64_t)x;
}

void launch_expand_batch_corr(const uint8_t *bm, uint64_t bm_stride, uint64_t nb8, uint64_t N, uint32_t nx, uint32_t n, const uint32_t *blk_off,
                              const uint8_t *pv, uint64_t pv_stride, const uint32_t *pv_bytes, uint32_t d, uint32_t level, const int32_t *padded,
                              uint32_t radius, int64_t *partials, int64_t *out, const int *err, hipStream_t s)
{
    const uint32_t nblk = (uint32_t)((nb8 + WG - 1) / WG);
    const uint32_t bpc = corr_blocks_per_chunk(nblk, n), nchunk = corr_chunks(nblk, n), S2 = corr_cells(radius), nacc = corr_lane_cells(radius);
    uint64_t *part = reinterpret_cast<uint64_t *>(partials);
    auto go = [&](auto c) {
        hipLaunchKernelGGL(k_expand_corr_b<(uint32_t)decltype(c)::value>, dim3(n * ((nchunk + CORR_XCDS - 1) / CORR_XCDS) * CORR_XCDS), dim3(WG), 0, s, bm, bm_stride, nb8, N, nx, nblk, bpc, nchunk, n, blk_off, pv,
                           pv_stride, pv_bytes, d, level, padded, radius, part, err);
    };
    // (the instantiation bounds the registers; the kernel skips the accumulators past ceil(S^2 / 64))
    if (nacc <= 1) go(int_c<1>{});            // R <= 3
    else if (nacc <= 2) go(int_c<2>{});       // R = 4, 5
    else if (nacc <= 5) go(int_c<5>{});       // R = 6 .. 8
    else if (nacc <= 9) go(int_c<9>{});       // R = 9 .. 11
    else go(int_c<18>{});                     // R = 12 .. 16
    launch_rows_reduce(partials, nchunk, S2, n, out, err, s);
}

void launch_rows_reduce(const int64_t *partials, uint32_t nchunk, uint32_t ncells, uint32_t n, int64_t *out, const int *err, hipStream_t s)
{
    hipLaunchKernelGGL(k_corr_reduce, dim3(n, (ncells + WG - 1) / WG), dim3(WG), 0, s, reinterpret_cast<const uint64_t *>(partials), nchunk, ncells, out, err);
}

}  // namespace rc
