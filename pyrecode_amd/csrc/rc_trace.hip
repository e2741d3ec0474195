// rc_trace.hip - frame traces (rc_trace_frames): a batch's decoded bitmaps and value streams -> out[n][4 + k], per frame the number of set
// pixels, the sum of their values, the sums weighted by row and by column, and the sums under k int32 weight planes (gfx950).
//
//   dose rate per frame              pyrecode/utils/converters.py:108-111 (the set pixels of every frame, printed by l1_to_l4_converter)
//   anything else per frame          a host loop around ReCoDeReader.get_frame (pyrecode/recode_reader.py:379-471) and numpy
#include "rc_trace.h"
#include "rc_expand.h"

#include <algorithm>

namespace rc {

constexpr uint32_t TRACE_COLS_MAX = TRACE_MOMENTS + TRACE_MAX_PLANES;
constexpr uint32_t TRACE_TARGET_WGS = 2048;   // workgroups a launch aims for, as k_expand_sum_b's: four rounds of the 512 resident on 256 CUs
constexpr uint32_t TRACE_MIN_GROUP = 4;       // ... but no group of fewer frames: the word's row / column division is paid once per group

// the sum over the wave's 64 lanes, in every lane (sums are modulo 2^64: signed values add as their two's complements)
__device__ __forceinline__ uint64_t wave_sum64(uint64_t x)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) x += __shfl_xor(x, d);
    return x;
}

// A workgroup owns ONE block of WG bitmap words for a GROUP of consecutive frames, as in k_expand_sum_b, with the next frame's word in
// flight across this frame's barriers; a thread's rank in the value stream is blk_off + block_excl_scan (level 1 only: the other levels
// have no values to rank, and no scan).  The word index is the same for every frame of the group, so row and column of its first pixel come
// from ONE division per thread and group; the pixels behind it step the column, as in k_expand_emit_b.  Instead of cells per pixel a thread
// keeps the frame's 4 + k sums in registers (uint64, exact modulo 2^64; the no-wrap rule of rc_trace.h makes the modulus moot), the
// weighted ones in a fully unrolled array of TRACE_MAX_PLANES that is indexed by constants only: no scratch.
//   Weights: int32[N][kp], pixel-major, kp = k rounded up to a multiple of 4 - a set pixel's k weights are kp / 4 consecutive 16-byte
//   vectors, one to four lines' worth of ONE address instead of k loads 4 N bytes apart.  HAS_W = false touches no weight memory.
//   The partials meet without atomics: a wave with a set pixel reduces its sums across its lanes (DPP for the two that fit 32 bits, xor
//   shuffles for the 64-bit ones), lane 0 leaves them in LDS - two buffers that alternate by frame, so ONE barrier per frame orders both
//   the hand-over and the buffer's reuse two frames later -, and threads 0 .. 4 + k - 1 add the four waves' and store the block's row of
//   partials[f][block][4 + k].  k_trace_reduce then adds a frame's rows.  1024 blocks of a 4096 x 4096 frame adding into the same
//   4 + k addresses is the one-row shape global atomics are slowest at; the rows cost 160 bytes per (frame, block) at most, written and
//   read once, and the result is written exactly once per cell without anybody clearing `out`.
// LDS: the scan's 20 bytes + 2 x 4 x 20 x 8 = 1300 B.  Writes nothing once *err is set (a decoder, or k_expand_bases: value stream too short).
template <bool HAS_W>
__global__ __launch_bounds__(WG) void k_expand_trace_b(const uint8_t *__restrict__ bm, uint64_t bm_stride, uint64_t nb8, uint64_t N, uint32_t nx,
                                                         uint32_t nblk, const uint32_t *__restrict__ blk_off, const uint8_t *__restrict__ pv,
                                                         uint64_t pv_stride, const uint32_t *__restrict__ pv_bytes, uint32_t d, uint32_t level, uint32_t n,
                                                         uint32_t per_group, const u32x4 *__restrict__ weights, uint32_t k, uint64_t *__restrict__ partials,
                                                         const int *__restrict__ err)
{
    __shared__ uint32_t sm[WAVES + 1];
    __shared__ uint64_t s_w[2][WAVES][TRACE_COLS_MAX];
    if (*err) return;   // (workgroup-uniform, as in k_expand_emit_b)
    const uint32_t t = threadIdx.x, wave = t >> 6, lane = t & 63u;
    const uint32_t ncols = TRACE_MOMENTS + k, kv = (k + 3u) >> 2;     // columns of a row; 16-byte vectors of a pixel's weights
    const uint32_t f0 = blockIdx.y * per_group, f1 = min(n, f0 + per_group);
    const uint64_t i = (uint64_t)blockIdx.x * WG + t;
    const uint32_t dmask = level == 1 ? (1u << d) - 1u : 0u;          // (level 1: 1 <= d <= 16)
    const uint32_t k0 = i < nb8 ? (uint32_t)(i * 64) : 0u;            // the word's first pixel (frames have fewer than 2^32 pixels)
    const uint32_t row0 = k0 / nx, col0 = k0 - row0 * nx;
    uint64_t next = f0 < f1 ? expand_word(bm + f0 * bm_stride, nb8, N, i) : 0;
    for (uint32_t f = f0; f < f1; ++f) {
        uint64_t bits = next;
        if (f + 1 < f1) next = expand_word(bm + (f + 1) * bm_stride, nb8, N, i);   // (in flight across this frame's barriers)
        const uint32_t cnt = (uint32_t)__builtin_popcountll(bits);
        uint32_t local = 0, tot;
        if (level == 1) local = block_excl_scan(cnt, sm, &tot);                    // (uniform)
        uint32_t a_sum = 0;                                                        // <= 64 * 65535
        uint64_t a_row = 0, a_col = 0, a_w[TRACE_MAX_PLANES];
#pragma unroll
        for (uint32_t m = 0; m < TRACE_MAX_PLANES; ++m) a_w[m] = 0;
        if (bits) {
            uint64_t rank = level == 1 ? (uint64_t)blk_off[(uint64_t)f * nblk + blockIdx.x] + local : 0;
            const uint8_t *pix = pv + f * pv_stride;
            const uint64_t pix_bytes = level == 1 ? pv_bytes[f] : 0;
            uint32_t row = row0, col = col0, prev = 0;
            for (; bits; bits &= bits - 1, ++rank) {
                const uint32_t b = (uint32_t)__builtin_ctzll(bits);
                col += b - prev;
                prev = b;
                while (col >= nx) { col -= nx; ++row; }
                const uint32_t v = level == 1 ? expand_field16(pix, pix_bytes, rank, d, dmask) : 1u;
                a_sum += v;
                a_row += (uint64_t)v * row;
                a_col += (uint64_t)v * col;
                if (HAS_W) {
                    const u32x4 *w = weights + (uint64_t)(k0 + b) * kv;
#pragma unroll
                    for (uint32_t g = 0; g < TRACE_MAX_PLANES / 4; ++g) {
                        if (g < kv) {                                              // (uniform)
                            const u32x4 q = w[g];
#pragma unroll
                            for (uint32_t j = 0; j < 4; ++j) a_w[4 * g + j] += (uint64_t)((int64_t)(int32_t)q[j] * (int64_t)v);
                        }
                    }
                }
            }
        }
        uint64_t *mine = s_w[(f - f0) & 1u][wave];
        if (__ballot(cnt != 0)) {                                                  // (wave-uniform)
            const uint32_t w_cnt = wave_last(wave_incl_scan(cnt)), w_sum = wave_last(wave_incl_scan(a_sum));   // <= 4096, <= 4096 * 65535
            const uint64_t w_row = wave_sum64(a_row), w_col = wave_sum64(a_col);
            if (lane == 0) { mine[0] = w_cnt; mine[1] = w_sum; mine[2] = w_row; mine[3] = w_col; }
            if (HAS_W) {
#pragma unroll
                for (uint32_t m = 0; m < TRACE_MAX_PLANES; ++m) {
                    if (m < k) {                                                   // (uniform)
                        const uint64_t x = wave_sum64(a_w[m]);
                        if (lane == 0) mine[TRACE_MOMENTS + m] = x;
                    }
                }
            }
        } else if (lane < ncols)
            mine[lane] = 0;
        __syncthreads();
        if (t < ncols) {
            const uint64_t(*b)[TRACE_COLS_MAX] = s_w[(f - f0) & 1u];
            uint64_t x = 0;
#pragma unroll
            for (uint32_t w = 0; w < (uint32_t)WAVES; ++w) x += b[w][t];
            partials[((uint64_t)f * nblk + blockIdx.x) * ncols + t] = x;
        }
    }
}

// One workgroup per frame: out[f][c] = sum over the blocks of partials[f][block][c].  A frame's rows are one array of nblk * ncols words
// whose element j belongs to column j % ncols: the first S = (WG / ncols) * ncols threads walk it S apart - consecutive lanes on consecutive
// words, every thread inside one column -, then thread c adds the threads of its column.  The only writer of `out`, every cell once;
// nothing once *err is set.
__global__ __launch_bounds__(WG) void k_trace_reduce(const uint64_t *__restrict__ partials, uint32_t nblk, uint32_t ncols, int64_t *__restrict__ out,
                                                       const int *__restrict__ err)
{
    __shared__ uint64_t s[WG];
    if (*err) return;
    const uint32_t f = blockIdx.x, t = threadIdx.x, S = ((uint32_t)WG / ncols) * ncols;
    const uint64_t total = (uint64_t)nblk * ncols;
    const uint64_t *p = partials + (uint64_t)f * total;
    uint64_t a = 0;
    if (t < S)
        for (uint64_t j = t; j < total; j += S) a += p[j];
    s[t] = a;
    __syncthreads();
    if (t < ncols) {
        uint64_t x = 0;
        for (uint32_t j = t; j < S; j += ncols) x += s[j];
        out[(uint64_t)f * ncols + t] = (int64_t)x;
    }
}

uint64_t trace_workspace_bytes(uint64_t nb8, uint32_t n, uint32_t k)
{
    const uint64_t nblk = (nb8 + WG - 1) / WG;
    return (uint64_t)n * nblk * (TRACE_MOMENTS + k) * 8;
}

void launch_expand_batch_trace(const uint8_t *bm, uint64_t bm_stride, uint64_t nb8, uint64_t N, uint32_t nx, uint32_t n, const uint32_t *blk_off,
                               const uint8_t *pv, uint64_t pv_stride, const uint32_t *pv_bytes, uint32_t d, uint32_t level, const int32_t *weights,
                               uint32_t k, int64_t *partials, int64_t *out, const int *err, hipStream_t s)
{
    const uint32_t nblk = (uint32_t)((nb8 + WG - 1) / WG);
    const uint32_t want = std::max(1u, std::min((TRACE_TARGET_WGS + nblk - 1) / nblk, (n + TRACE_MIN_GROUP - 1) / TRACE_MIN_GROUP));
    const uint32_t per_group = (n + want - 1) / want, groups = (n + per_group - 1) / per_group;      // (no empty group)
    uint64_t *part = reinterpret_cast<uint64_t *>(partials);
    const u32x4 *w = reinterpret_cast<const u32x4 *>(weights);
    if (k)
        hipLaunchKernelGGL(k_expand_trace_b<true>, dim3(nblk, groups), dim3(WG), 0, s, bm, bm_stride, nb8, N, nx, nblk, blk_off, pv, pv_stride, pv_bytes, d, level,
                           n, per_group, w, k, part, err);
    else
        hipLaunchKernelGGL(k_expand_trace_b<false>, dim3(nblk, groups), dim3(WG), 0, s, bm, bm_stride, nb8, N, nx, nblk, blk_off, pv, pv_stride, pv_bytes, d, level,
                           n, per_group, w, 0u, part, err);
    hipLaunchKernelGGL(k_trace_reduce, dim3(n), dim3(WG), 0, s, part, nblk, TRACE_MOMENTS + k, out, err);
}

// ---- a handle's weights (rc_trace_create) -----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(WG) void k_trace_interleave(const int32_t *__restrict__ plane, uint64_t N, uint32_t m, uint32_t kp, int32_t *__restrict__ weights)
{
    const uint64_t stride = (uint64_t)gridDim.x * WG;
    for (uint64_t p = (uint64_t)blockIdx.x * WG + threadIdx.x; p < N; p += stride) weights[p * kp + m] = plane[p];
}
__global__ __launch_bounds__(WG) void k_trace_maxabs(const int32_t *__restrict__ plane, uint64_t N, uint32_t *__restrict__ bound)
{
    const uint64_t stride = (uint64_t)gridDim.x * WG;
    uint32_t a = 0;
    for (uint64_t p = (uint64_t)blockIdx.x * WG + threadIdx.x; p < N; p += stride) a = max(a, trace_abs(plane[p]));
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) a = max(a, (uint32_t)__shfl_xor((int)a, d));
    if ((threadIdx.x & 63u) == 0 && a) (void)atomicMax(bound, a);
}
static uint32_t trace_plane_grid(uint64_t N) { return (uint32_t)std::min<uint64_t>(2048, (N + WG - 1) / WG); }
void launch_trace_interleave(const int32_t *plane, uint64_t N, uint32_t m, uint32_t kp, int32_t *weights, hipStream_t s)
{
    hipLaunchKernelGGL(k_trace_interleave, dim3(trace_plane_grid(N)), dim3(WG), 0, s, plane, N, m, kp, weights);
}
void launch_trace_maxabs(const int32_t *plane, uint64_t N, uint32_t *bound, hipStream_t s)
{
    hipLaunchKernelGGL(k_trace_maxabs, dim3(trace_plane_grid(N)), dim3(WG), 0, s, plane, N, bound);
}

}  // namespace rc
