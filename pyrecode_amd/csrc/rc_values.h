// rc_values.h - device code the two formats of the value stage share (rc_launch.h; rc_pix_huff.hip: zstd blocks, rc_pix_deflate.hip: DEFLATE
// blocks).  A wavefront takes a chunk of the flat stream, 16 bytes per lane: the bytes' codes from an LDS table, four groups per lane, are ORed
// into an LDS window at scanned bit offsets; a wavefront per chunk then copies the image behind the record's binary-map stream.
#pragma once
#include "rc_record.h"

namespace rc {

__host__ __device__ __forceinline__ uint32_t value_chunks(uint32_t npk, uint32_t chunk) { return npk ? (npk + chunk - 1) / chunk : 1u; }   // (empty stream: one empty block)

// Codes (code | length << 12) of the first vb of a lane's 16 bytes, in groups of four bytes: g[k] the group's bits (<= 48), gb[k] how many;
// returns the lane's sum.  LAST_LOW: inside a group the LAST byte is lowest (zstd: a stream is read from its end), else the FIRST (DEFLATE).
template <bool LAST_LOW>
__device__ __forceinline__ uint32_t value_codes(const u32x4 &v, int vb, const uint16_t *s_code, uint64_t (&g)[4], uint32_t (&gb)[4])
{
    uint32_t nb = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        uint64_t a = 0;
        uint32_t b = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int j = LAST_LOW ? 3 - i : i;
            if (4 * k + j < vb) {
                const uint32_t cd = s_code[(v[k] >> (8 * j)) & 0xFFu];
                a |= (uint64_t)(cd & 0xFFFu) << b;
                b += cd >> 12;
            }
        }
        g[k] = a; gb[k] = b; nb += b;
    }
    return nb;
}

// OR a group of up to 48 bits into the wavefront's zeroed LDS window at bit `bit` (up to three dwords; the lanes' groups share dwords)
__device__ __forceinline__ void window_or(uint32_t *win, uint32_t bit, uint64_t g)
{
    const uint32_t wd = bit >> 5, s = bit & 31u;
    const uint64_t a = g << s;
    const uint32_t top = s ? (uint32_t)(g >> (64 - s)) : 0u;
    __hip_atomic_fetch_or(&win[wd], (uint32_t)a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
    if (a >> 32) __hip_atomic_fetch_or(&win[wd + 1], (uint32_t)(a >> 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
    if (top) __hip_atomic_fetch_or(&win[wd + 2], top, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}

// size bytes from src (4-byte aligned, readable up to the next dword boundary behind src + size + 4) to dst (any alignment), by one wavefront:
// destination dword j = source bytes [head + 4j, +4) = the byte funnel of source dwords j, j + 1
__device__ __forceinline__ void wave_copy_unaligned(uint8_t *dst, const uint8_t *src, uint32_t size, uint32_t lane)
{
    const uint32_t head = min(size, (uint32_t)((4u - (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 3u)) & 3u));
    const uint32_t nd = (size - head) >> 2, tail = (size - head) & 3u;
    const uint32_t *s32 = reinterpret_cast<const uint32_t *>(src);
    for (uint32_t j = lane; j < nd; j += 64)
        reinterpret_cast<uint32_t *>(dst + head)[j] = __builtin_amdgcn_alignbyte(s32[j + 1], s32[j], head);
    if (lane < head) dst[lane] = src[lane];
    if (lane < tail) dst[head + 4 * nd + lane] = src[head + 4 * nd + lane];
}

// host side: the zstd format's half of launch_values_encode / _scan / _gather (rc_launch.h; they dispatch on the kind in rc_pix_deflate.hip)
void launch_pix_huff(const Scratch &sc, uint32_t B, uint32_t depth, hipStream_t s);
void launch_pix_scan(const Scratch &sc, uint32_t B, uint32_t depth, hipStream_t s);   // (rc_reduce.hip: it shares the tile scans' helpers)
void launch_pix_gather(const Scratch &sc, uint32_t B, uint32_t depth, uint32_t rec_hdr, uint8_t *out, const uint64_t *rec_off, hipStream_t s);

}  // namespace rc
