// rc_dense.hip - dense frame batches (rc_expand_frames_dense): a batch's decoded bitmaps and value streams -> out[n][h][w], a region of
// every frame as an array of cells, written on the device (gfx950).
//
//   ReCoDeReader.get_sub_volume      pyrecode/recode_reader.py:185-186 (a NotImplementedError stub there)
//   frame.toarray() per frame        pyrecode/utils/viewer.py:65-68 (what callers do instead: a memset and a scatter on the host)
#include "rc_dense.h"
#include "rc_expand.h"

namespace rc {

static_assert(DENSE_BLOCK_PIXELS == (uint32_t)WG * 64u, "a block is WG bitmap words");

// A workgroup owns ONE block of WG bitmap words (16 384 pixels in linear row-major order) of ONE frame, as in k_expand_sum_b, and builds the
// block's cells in LDS: the image is zeroed by all threads (16-byte stores, lanes on consecutive vectors), then thread t expands its word's
// set pixels into it - it is the only writer of its 64 cells: no atomics -, and after one barrier the workgroup flushes the image, lanes on
// consecutive output cells.  Every cell of `out` the block is responsible for is written exactly once, zeros included; nothing is read
// from `out`.  The image is in pixel order, cell (word t, bit b) at 64 t + b, so that the flush reads 16 bytes per lane (ds_read_b128,
// conflict-free) - the price is the expansion of a DENSE frame, whose lanes walk b in lockstep 64 cells apart and share banks; the
// expansion's cost follows the set pixels, a few per word in the frames this format is for, the flush's the cells.
//   Whole rows at steps of 1 (dense_is_linear): the block's cells are one contiguous range of `out`.  They leave as 16-byte stores with a
//   cell-by-cell head and tail: out + f * h * w cells is only cell-aligned (3 x 21 uint16 frames are 126 bytes each), and a frame's last
//   block ends mid-vector when N % 8 != 0.  The image is shifted by the range's misalignment (sh cells), so that LDS vector v IS global
//   vector v: one aligned LDS read per aligned store.
//   Otherwise pixel -> (row, col) -> cell (dense_cell): one division per thread, then the column steps by WG; cells off the region or off
//   the step lattice are dropped.
// LDS: the image is PIX + one vector of cells, PIX = 16 384 for uint8 (16 KiB + 16 B) and uint16 (32 KiB + 16 B) cells; uint32 cells would
// need 64 KiB, which with the scan's words is over the static limit: that instantiation runs its block in two passes of 8192 pixels
// (32 KiB + 16 B; the words of the other half wait).  With the scan's 20 bytes that leaves room for 9 (uint8) and 4 (uint16, uint32)
// workgroups in a CU's 160 KiB; 8 workgroups of 4 waves fill a CU's wave slots.
// Writes nothing once *err is set (a decoder, or k_expand_bases: value stream too short).
template <class CT>
__global__ __launch_bounds__(WG) void k_expand_dense_b(const uint8_t *__restrict__ bm, uint64_t bm_stride, uint64_t nb8, uint64_t N, uint32_t nx,
                                                         uint32_t nblk, uint32_t blk0, const uint32_t *__restrict__ blk_off,
                                                         const uint8_t *__restrict__ pv, uint64_t pv_stride, const uint32_t *__restrict__ pv_bytes,
                                                         uint32_t d, uint32_t level, DenseRegion R, uint32_t linear, CT *__restrict__ out,
                                                         const int *__restrict__ err)
{
    constexpr uint32_t PASSES = sizeof(CT) == 4 ? 2 : 1;
    constexpr uint32_t WORDS = WG / PASSES;           // bitmap words of a pass
    constexpr uint32_t PIX = WORDS * 64;              // pixels of a pass = cells of the image
    constexpr uint32_t VEC = 16 / sizeof(CT);         // cells of a 16-byte vector
    __shared__ uint32_t sm[WAVES + 1];
    __shared__ __attribute__((aligned(16))) CT cell[PIX + VEC];
    if (*err) return;   // (workgroup-uniform, as in k_expand_emit_b)
    const uint32_t t = threadIdx.x, f = blockIdx.y, blk = blk0 + blockIdx.x;
    uint64_t bits = expand_word(bm + f * bm_stride, nb8, N, (uint64_t)blk * WG + t);
    uint64_t rank = 0;
    if (level == 1) {   // (uniform) ranks inside the value stream; other levels write 1
        uint32_t tot;
        rank = (uint64_t)blk_off[(uint64_t)f * nblk + blk] + block_excl_scan((uint32_t)__builtin_popcountll(bits), sm, &tot);
    }
    const uint8_t *pix = pv + f * pv_stride;
    const uint64_t pix_bytes = level == 1 ? pv_bytes[f] : 0;
    const uint64_t frame_cells = (uint64_t)R.w * R.h;
    CT *o = out + (uint64_t)f * frame_cells;
    u32x4 *cv = reinterpret_cast<u32x4 *>(cell);
    // the frame's pixels that are cells, as a linear range (linear form) - or everything (the mapping decides)
    const uint64_t ra = linear ? (uint64_t)R.y0 * nx : 0, rb = linear ? ra + frame_cells : N;
    for (uint32_t pass = 0; pass < PASSES; ++pass) {
        const uint64_t p0 = (uint64_t)blk * DENSE_BLOCK_PIXELS + (uint64_t)pass * PIX;     // the pass's first pixel
        const uint64_t a = p0 > ra ? p0 : ra, b = p0 + PIX < rb ? p0 + PIX : rb;           // [a, b): its pixels that are cells
        if (a >= b) continue;                                                              // (uniform)
        // sh: image index of pixel p is sh + (p - p0); in the linear form chosen so that the image and `out` agree modulo a vector
        const uint32_t sh = linear ? (uint32_t)((reinterpret_cast<uintptr_t>(o + (a - ra)) / sizeof(CT) - (a - p0)) & (VEC - 1)) : 0u;
        if (pass) __syncthreads();                                                         // (the flush before has read the image)
        for (uint32_t v = t; v < (PIX + VEC) / VEC; v += WG) cv[v] = u32x4{0u, 0u, 0u, 0u};
        __syncthreads();
        if (bits && t / WORDS == pass) {
            CT *mine = cell + sh + (t % WORDS) * 64;
            for (; bits; bits &= bits - 1, ++rank)
                mine[__builtin_ctzll(bits)] = level == 1 ? (CT)expand_field32(pix, pix_bytes, rank, d) : (CT)1;
        }
        __syncthreads();
        if (linear) {
            // image indices [s0, s1) go to o[c + shift_out]: whole vectors as vectors, the two ragged ends cell by cell
            const uint32_t s0 = sh + (uint32_t)(a - p0), s1 = sh + (uint32_t)(b - p0);
            CT *og = o + (a - ra) - s0;                       // image index c <-> og + c; 16-byte aligned by the choice of sh
            for (uint32_t v = s0 / VEC + t; v * VEC < s1; v += WG) {
                const uint32_t lo = v * VEC;
                if (lo >= s0 && lo + VEC <= s1) reinterpret_cast<u32x4 *>(og)[v] = cv[v];
                else
                    for (uint32_t c = lo > s0 ? lo : s0; c < lo + VEC && c < s1; ++c) og[c] = cell[c];
            }
        } else {
            // pixel q of the pass: one division for a thread's first pixel, then the column steps by WG (rows shorter than that: divide)
            const uint32_t p = (uint32_t)p0 + t;
            uint32_t row = p / nx, col = p - row * nx;
            for (uint32_t q = t; q < PIX && p0 + q < N; q += WG) {
                const int64_t idx = dense_cell(R, row, col);
                if (idx >= 0) o[idx] = cell[q];
                if (nx >= (uint32_t)WG) {
                    col += WG;
                    if (col >= nx) { col -= nx; ++row; }
                } else {
                    const uint32_t pn = p + (q - t) + WG;
                    row = pn / nx;
                    col = pn - row * nx;
                }
            }
        }
    }
}

void launch_expand_batch_dense(const uint8_t *bm, uint64_t bm_stride, uint64_t nb8, uint64_t N, uint32_t nx, uint32_t n, const uint32_t *blk_off,
                               const uint8_t *pv, uint64_t pv_stride, const uint32_t *pv_bytes, uint32_t d, uint32_t level, const DenseRegion &region,
                               uint32_t cell_bytes, void *out, const int *err, hipStream_t s)
{
    const uint32_t nblk = (uint32_t)((nb8 + WG - 1) / WG);
    // only the blocks between the region's first and last pixel: a block offset in the grid (the count pass before covered the frame)
    uint32_t first, last;
    dense_block_range(nx, region, &first, &last);
    const dim3 grid(last - first + 1, n);
    const uint32_t linear = dense_is_linear(nx, region) ? 1u : 0u;
    if (cell_bytes == 1)
        hipLaunchKernelGGL(k_expand_dense_b<uint8_t>, grid, dim3(WG), 0, s, bm, bm_stride, nb8, N, nx, nblk, first, blk_off, pv, pv_stride, pv_bytes, d, level,
                           region, linear, static_cast<uint8_t *>(out), err);
    else if (cell_bytes == 2)
        hipLaunchKernelGGL(k_expand_dense_b<uint16_t>, grid, dim3(WG), 0, s, bm, bm_stride, nb8, N, nx, nblk, first, blk_off, pv, pv_stride, pv_bytes, d, level,
                           region, linear, static_cast<uint16_t *>(out), err);
    else
        hipLaunchKernelGGL(k_expand_dense_b<uint32_t>, grid, dim3(WG), 0, s, bm, bm_stride, nb8, N, nx, nblk, first, blk_off, pv, pv_stride, pv_bytes, d, level,
                           region, linear, static_cast<uint32_t *>(out), err);
}

}  // namespace rc
