// rc_expand.h - launchers of rc_expand.hip
#pragma once
#include "rc_device.h"
#include "rc_shift.h"

namespace rc {
// ---- what the kernels of rc_expand.hip and rc_count.hip read a decoded frame with ----------------------------------------------------
// bitmap is padded with zero bytes to a multiple of 8 by the host wrapper, so 8-byte loads are always in bounds.
// 64 bitmap bits of word i with the bits of pixels at or past N cleared: a well-formed bitmap has them zero, a foreign or
// damaged file may not, and the count pass and the emit pass must agree on what they see
__device__ __forceinline__ uint64_t expand_word(const uint8_t *__restrict__ bitmap, uint64_t nb8, uint64_t N, uint64_t i)
{
    if (i >= nb8) return 0;
    const u32x2 v = reinterpret_cast<const u32x2 *>(bitmap)[i];
    uint64_t bits = (uint64_t)v[0] | ((uint64_t)v[1] << 32);
    const uint64_t k0 = i * 64;
    if (k0 + 64 > N) bits = k0 >= N ? 0 : bits & ((1ull << (N - k0)) - 1);
    return bits;
}

// d-bit LSB-first field number `idx` of a packed stream of `nbytes` bytes (bytes past the end read as zero)
__device__ __forceinline__ uint64_t read_field(const uint8_t *__restrict__ p, uint64_t nbytes, uint64_t idx, uint32_t d)
{
    const uint64_t bit = idx * d;
    uint64_t byte = bit >> 3;
    const uint32_t sh = (uint32_t)(bit & 7);
    const uint32_t need = (sh + d + 7) >> 3;  // <= 9 bytes for d <= 64
    uint64_t lo = 0, hi = 0;
    for (uint32_t k = 0; k < need && k < 8; ++k)
        if (byte + k < nbytes) lo |= (uint64_t)p[byte + k] << (8 * k);
    if (need > 8 && byte + 8 < nbytes) hi = p[byte + 8];
    uint64_t v = lo >> sh;
    if (sh && need > 8) v |= hi << (64 - sh);
    return d >= 64 ? v : (v & ((1ull << d) - 1));
}

// field `rank` of a frame's decoded value stream, 1 <= d <= 16 (dmask = 2^d - 1): d = 16 is the uint16 itself; a narrower field that ends
// inside the stream lies in the two dwords at its bit position, the second of which ends before pix_bytes + 8 - inside the frame's slot,
// zeroed behind the stream (rc_reader.hip: pv_stride; slots are 16-byte aligned); anything else goes byte by byte with every byte
// checked (read_field)
__device__ __forceinline__ uint32_t expand_field16(const uint8_t *__restrict__ pix, uint64_t pix_bytes, uint64_t rank, uint32_t d, uint32_t dmask)
{
    if (d == 16 && 2 * rank + 2 <= pix_bytes) return reinterpret_cast<const uint16_t *>(pix)[rank];
    if (d < 16 && rank * d + d <= 8 * pix_bytes) {
        const uint64_t bit = rank * d;
        const uint32_t *p = reinterpret_cast<const uint32_t *>(pix) + (bit >> 5);
        return (uint32_t)((((uint64_t)p[0] | ((uint64_t)p[1] << 32)) >> (bit & 31u))) & dmask;
    }
    return (uint32_t)read_field(pix, pix_bytes, rank, d);
}

// the same for 17 <= d <= 32, from dwords (value streams are 16-byte aligned): d = 32 is the dword itself; a narrower field that ends inside
// the stream lies inside the two dwords at its bit position.  Its last bit is below 8 * pix_bytes, so the first dword starts below pix_bytes
// and the second one ends before pix_bytes + 8 - inside the frame's slot, which is the longest stream rounded up to 16 bytes plus 16 more,
// zeroed behind the stream (rc_reader.hip: pv_stride, out_bytes; as k_stats_unpack).
__device__ __forceinline__ uint32_t expand_field_wide(const uint8_t *__restrict__ pix, uint64_t pix_bytes, uint64_t rank, uint32_t d)
{
    if (d == 32 && 4 * rank + 4 <= pix_bytes) return reinterpret_cast<const uint32_t *>(pix)[rank];
    if (d < 32 && rank * d + d <= 8 * pix_bytes) {
        const uint64_t bit = rank * d;
        const uint32_t *p = reinterpret_cast<const uint32_t *>(pix) + (bit >> 5);
        return (uint32_t)((((uint64_t)p[0] | ((uint64_t)p[1] << 32)) >> (bit & 31u)) & ((1u << d) - 1u));
    }
    return (uint32_t)read_field(pix, pix_bytes, rank, d);
}
// any 1 <= d <= 32
__device__ __forceinline__ uint32_t expand_field32(const uint8_t *__restrict__ pix, uint64_t pix_bytes, uint64_t rank, uint32_t d)
{
    return d <= 16 ? expand_field16(pix, pix_bytes, rank, d, (1u << d) - 1u) : expand_field_wide(pix, pix_bytes, rank, d);
}

void launch_expand_count(const uint8_t *bitmap_pad8, uint64_t nb8, uint64_t N, uint32_t *blk_cnt, uint32_t *blk_off,
                         uint64_t *nnz_dev, hipStream_t s);
void launch_expand_emit(const uint8_t *bitmap_pad8, uint64_t nb8, uint64_t N, uint32_t nx, const uint32_t *blk_off,
                        const uint8_t *pix, uint64_t pix_bytes, uint32_t d, uint32_t level, uint64_t cap, uint64_t *out,
                        hipStream_t s);
void launch_expand_batch_count(const uint8_t *bm, uint64_t bm_stride, uint64_t nb8, uint64_t N, uint32_t n, uint32_t *blk_cnt, uint32_t *blk_off,
                               uint64_t *frame_nnz, uint64_t *frame_base, hipStream_t s, const uint32_t *pv_bytes = nullptr, uint32_t d = 0,
                               uint32_t level = 0, uint64_t cap = 0, int *err = nullptr);
void launch_expand_batch_scan(const uint32_t *cnt, uint32_t *off, uint64_t nb8, uint32_t n, uint64_t *frame_nnz, uint64_t *frame_base, uint64_t cap,
                              int *err, hipStream_t s);
// coo_value_bytes: 0 = uint64 (row, col, value) rows; 2 / 4 = int32 rows[cap] | int32 columns[cap] | uint16 / uint32 values[cap]
void launch_expand_batch_emit(const uint8_t *bm, uint64_t bm_stride, uint64_t nb8, uint64_t N, uint32_t nx, uint32_t n, const uint32_t *blk_off,
                              const uint64_t *frame_base, const uint8_t *pv, uint64_t pv_stride, const uint32_t *pv_bytes, uint32_t d,
                              uint32_t level, uint64_t cap, void *out, hipStream_t s, const int *err = nullptr, uint32_t coo_value_bytes = 0);
// acc[ny * nx] += the frames' pixel values (level 1: the d-bit fields, d <= 16; other levels: 1 per set pixel), behind
// launch_expand_batch_count on the same stream (blk_off, and *err as the gate: nothing is added once it is set)
void launch_expand_batch_sum(const uint8_t *bm, uint64_t bm_stride, uint64_t nb8, uint64_t N, uint32_t n, const uint32_t *blk_off, const uint8_t *pv,
                             uint64_t pv_stride, const uint32_t *pv_bytes, uint32_t d, uint32_t level, uint32_t *acc, const int *err, hipStream_t s);
// the same with frame f added (shifts[2 * f], shifts[2 * f + 1]) = (dy, dx) pixels away, what leaves the ny x nx view dropped (k_sum_shift; shifts:
// device memory, frame_nnz: the count pass's per-frame totals)
void launch_expand_batch_sum_shifted(const uint8_t *bm, uint64_t bm_stride, uint64_t nb8, uint64_t N, uint32_t nx, uint32_t ny, uint32_t n,
                                     const uint32_t *blk_off, const uint64_t *frame_nnz, const uint8_t *pv, uint64_t pv_stride, const uint32_t *pv_bytes,
                                     uint32_t d, uint32_t level, const int32_t *shifts, uint32_t *acc, const int *err, hipStream_t s);
// rc_zstd_dec.hip: block decoders of the batched reader
void launch_block_decode(int codec, int row, const uint8_t *data, const void *frame_lists, uint32_t nframes, uint32_t max_blocks_per_frame,
                         const void *tables, const void *predef, uint8_t *out, const uint64_t *out_base, int *err, hipStream_t s,
                         uint32_t *produced_out = nullptr);
void launch_bitmap_decode_compact(int codec, const uint8_t *data, const void *frame_lists, const uint64_t *src_base, uint32_t nframes,
                                  uint32_t max_blocks_per_frame, const void *tables, const void *predef, uint8_t *out, const uint64_t *out_base,
                                  uint64_t nb, int *err, hipStream_t s);
void launch_block_copy(const uint8_t *data, const void *lists, uint32_t nlists, uint32_t nblocks, uint32_t max_regen, uint8_t *out,
                       const uint64_t *out_base, hipStream_t s);
// rc_blosc.hip: the blocks of blosc1 chunks (entries: rc::ZdBlock, seq_tables = the chunk's shuffle flag)
void launch_blosc_decode_blocks(const uint8_t *data, const void *frame_lists, uint32_t nframes, uint32_t max_blocks_per_frame, uint8_t *out,
                                const uint64_t *out_base, int *err, hipStream_t s);
// level-2 statistics: d-bit fields of every frame's decoded stream -> uint16 (8 <= d <= 16)
void launch_stats_unpack(const uint8_t *pv, uint64_t pv_stride, const uint32_t *pv_bytes, const uint64_t *st_base, uint32_t n, uint32_t max_count,
                         uint32_t d, uint16_t *out, const int *err, hipStream_t s);
size_t zd_tables_bytes();
size_t zd_block_bytes();
void zd_predefined_tables(void *dst);
void launch_bit_pack(const uint16_t *vals, uint64_t n, uint32_t d, uint8_t *out, uint64_t out_n, hipStream_t s);
void launch_bit_unpack(const uint8_t *packed, uint64_t nbytes, uint64_t n, uint32_t d, uint64_t *out, hipStream_t s);
void launch_synth_dark(uint32_t seed, uint64_t N, uint16_t *dark, hipStream_t s);
void launch_synth_frames_clustered(uint32_t seed, uint32_t first_frame, uint32_t nframes, uint32_t nx, uint32_t ny, uint32_t seed_ppm,
                                   const uint16_t *dark, uint16_t *frames, hipStream_t s);
void launch_synth_frames(uint32_t seed, uint32_t first_frame, uint32_t nframes, uint64_t N, uint32_t sparsity_ppm,
                         const uint16_t *dark, uint16_t *frames, hipStream_t s);
}  // namespace rc
