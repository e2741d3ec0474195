// rc_blosc.hip - blosc1 chunk (bit-shuffle + LZ4, compression_scheme 8) block encoding on the GPU.
//
// Replaces `blosc.compress(data, clevel, cname='lz4', shuffle=blosc.BITSHUFFLE)` on the packed binary map
// (pyrecode/recode_compressors.py:108, called from recode_writer.py:503-505).  python-blosc is not a pinned dependency of
// the reference and is absent from the build image: the contract is a well-formed blosc1 chunk
// (c-blosc 1.x README_CHUNK_FORMAT / blosc.h) whose blocks are LZ4 blocks of the bit-shuffled data:
//   header 16 B: version 2 | versionlz 1 | flags | typesize 8 | nbytes | blocksize | cbytes   (little-endian int32s)
//   flags = 0x04 bit-shuffle | 0x10 blocks not split | 0x20 LZ4 format;   then int32 bstarts[nblocks];   then per block
//   int32 csize + csize bytes (csize == block bytes means "stored").
// One 512-byte tile = one block = 64 elements of typesize 8 (python-blosc's default typesize, the reference passes none).
//
// Bit-shuffle of a block (bitshuffle's bshuf_trans_bit_elem, little-endian bit order): with S elements, output row r
// (r = 0..63, bit r%8 of byte r/8 of every element) is S/8 bytes whose bit i is that bit of element i.  A lane owns one
// element (8 consecutive bytes), so row r IS the wave ballot of bit r.  S is rounded down to a multiple of 8; the bytes
// behind the shuffled part are copied unchanged (c-blosc's blosc_internal_bitshuffle).
#include "rc_launch.h"
#include "rc_lz4_block.h"
#include "rc_zstd_dec.h"

namespace rc {


// grid (ceil(ntiles/WAVES), B): wave w encodes block t = blockIdx.x*WAVES + w of frame blockIdx.y from the raw bitmap row.
__global__ __launch_bounds__(WG) void k_blosc_blocks(Scratch sc)
{
    __shared__ Lz4Lds s_lz[WAVES];
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = lane_id();
    const uint32_t t = blockIdx.x * WAVES + w;
    const uint32_t f = blockIdx.y;
    if (t >= sc.ntiles) return;
    const uint64_t b0 = (uint64_t)t * TILE_BM;
    const uint32_t n = (uint32_t)min((uint64_t)TILE_BM, sc.nb - b0);
    const u32x2 v = reinterpret_cast<const u32x2 *>(sc.bitmap + (uint64_t)f * sc.nb_stride + b0)[lane];  // rows are padded
    const uint64_t elem = (uint64_t)v[0] | ((uint64_t)v[1] << 32);
    Lz4Lds &L = s_lz[w];
    reinterpret_cast<u32x2 *>(L.raw)[lane] = v;
    const uint64_t own = bitshuffle_block(elem, n, L);
    const uint32_t csize = lz4_encode_block(own, n, L);
    const uint64_t ft = (uint64_t)f * sc.ntiles + t;
    uint8_t *slot = sc.blk_slots + ft * sc.blk_stride;
    const uint32_t used = lz4_store_block(slot, own, n, csize, L, true);   // (blosc marks a stored block by csize == size)
    if (lane == 0) sc.blk_size[ft] = used;
}

void launch_blosc_encode_blocks(const Scratch &sc, uint32_t B, hipStream_t s)
{
    hipLaunchKernelGGL(k_blosc_blocks, dim3((sc.ntiles + WAVES - 1) / WAVES, B), dim3(WG), 0, s, sc);
}

// Stand-alone chunk of an arbitrary buffer (seam 2): header + bstarts + blocks.  One wavefront per block copy.
__global__ __launch_bounds__(WG) void k_blosc_gather(Scratch sc, uint8_t *__restrict__ out)
{
    const uint32_t t = blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (t >= sc.ntiles) return;
    const uint32_t tab = 16 + 4 * sc.ntiles;
    if (t == 0 && lane_id() == 0) {
        const uint32_t nbytes = (uint32_t)sc.nb, bs = nbytes < (uint32_t)TILE_BM ? nbytes : (uint32_t)TILE_BM, cb = tab + sc.frame_cbytes[0];
        out[0] = 2; out[1] = 1; out[2] = 0x34; out[3] = 8;
        for (int k = 0; k < 4; ++k) { out[4 + k] = (uint8_t)(nbytes >> (8 * k)); out[8 + k] = (uint8_t)(bs >> (8 * k)); out[12 + k] = (uint8_t)(cb >> (8 * k)); }
    }
    const uint32_t off = tab + sc.blk_off[t];
    if (lane_id() == 0) for (int k = 0; k < 4; ++k) out[16 + 4 * t + k] = (uint8_t)(off >> (8 * k));
    const uint8_t *src = sc.blk_slots + (uint64_t)t * BLK_SLOT;
    const uint32_t n = sc.blk_size[t];
    for (uint32_t i = lane_id(); i < n; i += 64) out[off + i] = src[i];
}
void launch_blosc_gather(const Scratch &sc, uint8_t *out, hipStream_t s)
{
    hipLaunchKernelGGL(k_blosc_gather, dim3((sc.ntiles + WAVES - 1) / WAVES), dim3(WG), 0, s, sc, out);
}

// ---- decode side (seam 2: de_compress, recode_compressors.py:61-76): the blocks' LZ4 streams are decoded by k_lz4_decode
// (rc_lz4.hip) into a scratch image of the shuffled chunk; this kernel undoes the shuffle.  One thread per output byte.
// shuffle: 0 none, 1 byte shuffle, 4 bit shuffle (the header's flag bits).
__global__ void k_blosc_unshuffle(const uint8_t *__restrict__ in, uint8_t *__restrict__ out, uint64_t nbytes, uint32_t blocksize,
                                  uint32_t typesize, uint32_t shuffle)
{
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= nbytes) return;
    const uint64_t b0 = (g / blocksize) * blocksize;
    const uint32_t bsize = (uint32_t)min((uint64_t)blocksize, nbytes - b0);
    const uint32_t p = (uint32_t)(g - b0);
    const uint8_t *blk = in + b0;
    uint32_t v = blk[p];
    if (shuffle == 4 && bsize >= typesize) {
        const uint32_t S = (bsize / typesize) & ~7u;
        if (p < S * typesize) {
            const uint32_t i = p / typesize, k = p % typesize, rowb = S >> 3;
            v = 0;
            for (uint32_t b = 0; b < 8; ++b) v |= ((blk[(8 * k + b) * rowb + (i >> 3)] >> (i & 7)) & 1u) << b;
        }
    } else if (shuffle == 1 && typesize > 1) {
        const uint32_t ne = bsize / typesize;
        if (p < ne * typesize) v = blk[(p % typesize) * ne + p / typesize];
    }
    out[g] = (uint8_t)v;
}
void launch_blosc_unshuffle(const uint8_t *in, uint8_t *out, uint64_t nbytes, uint32_t blocksize, uint32_t typesize,
                            uint32_t shuffle, hipStream_t s)
{
    if (!nbytes) return;
    hipLaunchKernelGGL(k_blosc_unshuffle, dim3((uint32_t)((nbytes + 255) / 256)), dim3(256), 0, s, in, out, nbytes, blocksize,
                       typesize, shuffle);
}

// ---- decode side, batched reader (rc_expand_frames & co., scheme 8): ONE WAVEFRONT decodes ONE BLOCK of one frame's chunk - LZ4 block
// (or stored bytes) -> LDS, bit-unshuffle inside the wave, tile -> its place in the frame's decoded image.  Replaces, for every block of
// every frame of a batch at once, blosc.decompress on the frame's streams (pyrecode/recode_compressors.py:61-76, called from
// recode_reader.py:393-411).  The host walk (rc_reader.hip::blosc_index_stream) has checked every block's place and size: csize is at
// most the LZ4 bound of 512 bytes, so the compressed bytes always fit the wave's stage.
constexpr uint32_t BLOSC_IN_DW = 136;   // dwords staged per block: LZ4 bound of TILE_BM (530 bytes) + up to 3 bytes of misalignment in front

// One LZ4 block (lz4_Block_format.md), n bytes at `in`, into out[0 .. cap), both in the wave's LDS; returns the bytes produced.  The
// sequence headers are read by all lanes alike (wave-uniform, through readfirstlane), literals and matches are copied by the lanes side by
// side: a match's byte i is byte i % offset of the `offset` bytes in front of it, which are complete before the copy starts.
__device__ __forceinline__ uint32_t lz4_block_decode_wave(const uint8_t *in, uint32_t n, uint8_t *out, uint32_t cap, uint32_t lane, int *err)
{
    auto byte = [&](uint32_t i) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)in[i]); };
    uint32_t ip = 0, op = 0;
    while (ip < n) {
        const uint32_t token = byte(ip++);
        uint32_t lit = token >> 4;
        if (lit == 15) { uint32_t x; do { if (ip >= n) { *err = 1; return op; } x = byte(ip++); lit += x; } while (x == 255); }
        if (ip + lit > n || op + lit > cap) { *err = 1; return op; }
        for (uint32_t i = lane; i < lit; i += 64) out[op + i] = in[ip + i];
        ip += lit;
        op += lit;
        if (ip >= n) break;
        if (ip + 2 > n) { *err = 1; return op; }
        const uint32_t off = byte(ip) | (byte(ip + 1) << 8);
        ip += 2;
        uint32_t ml = token & 15u;
        if (ml == 15) { uint32_t x; do { if (ip >= n) { *err = 1; return op; } x = byte(ip++); ml += x; } while (x == 255); }
        ml += 4;
        if (off == 0 || off > op || op + ml > cap) { *err = 1; return op; }
        __builtin_amdgcn_wave_barrier();
        for (uint32_t i = lane; i < ml; i += 64) out[op + i] = out[op - off + i % off];
        __builtin_amdgcn_wave_barrier();
        op += ml;
    }
    return op;
}

// grid (ceil(max blocks per frame / WAVES), frames): wave w takes entry blockIdx.x * WAVES + w of lists[blockIdx.y] (ZdBlock: src / csize =
// the block's bytes behind its int32 size word, dst / regen = its place and size in the decoded stream, type 0 stored / 2 LZ4,
// seq_tables = the chunk's shuffle flag: 0 none, 4 bit-shuffle).  `out` is zeroed by the caller: only what is not zero is stored.
// The shuffled block is 64 rows of S/8 bytes, row r = bit r of the S elements (see the head of this file): lane i gathers bit i of every
// row - a 64 x 64 bit transpose out of LDS.
__global__ __launch_bounds__(WG) void k_blosc_decode_blocks(const uint8_t *__restrict__ data, const ZdFrameList *__restrict__ lists,
                                                              uint8_t *__restrict__ out, const uint64_t *__restrict__ out_base, int *__restrict__ err)
{
    __shared__ uint32_t s_in[WAVES][BLOSC_IN_DW];
    __shared__ uint64_t s_out[WAVES][TILE_BM / 8];
    const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = (uint32_t)lane_id();
    const uint32_t f = blockIdx.y, bi = blockIdx.x * WAVES + w;
    if (bi >= lists[f].n) return;
    const ZdBlock b = lists[f].p[bi];
    const uint32_t n = b.regen;
    int e = 0;
    if (n == 0 || n > (uint32_t)TILE_BM || b.csize == 0 || b.csize > n + n / 255u + 16u || (b.type != 2 && b.csize != n)) e = 1;   // (the host walk's own rules)
    uint8_t *raw = reinterpret_cast<uint8_t *>(s_out[w]);
    if (!e) {
        const uint64_t src0 = b.src & ~3ull;
        const uint32_t mis = (uint32_t)(b.src - src0), ndw = (mis + b.csize + 3u) >> 2;        // <= BLOSC_IN_DW
        const uint32_t *g = reinterpret_cast<const uint32_t *>(data + src0);                    // (data is 16-byte aligned and padded behind its end)
        for (uint32_t i = lane; i < ndw; i += 64) s_in[w][i] = g[i];
        __builtin_amdgcn_wave_barrier();
        const uint8_t *in = reinterpret_cast<const uint8_t *>(s_in[w]) + mis;
        if (b.type == 2) {
            if (lz4_block_decode_wave(in, b.csize, raw, n, lane, &e) != n) e = 1;
        } else
            for (uint32_t i = lane; i < n; i += 64) raw[i] = in[i];
        __builtin_amdgcn_wave_barrier();
    }
    if (e) {
        if (lane == 0) *err = 1;
        return;
    }
    uint8_t *dst = out + out_base[b.frame] + b.dst;                                          // 8-byte aligned: frame slots and tiles are
    const uint32_t S = b.seq_tables == 4 ? (n >> 3) & ~7u : 0u, whole = n >> 3;                 // elements shuffled / whole elements
    if (lane < whole) {
        uint64_t v;
        if (lane < S) {
            const uint32_t rowb = S >> 3, col = lane >> 3, sh = lane & 7u;
            uint32_t lo = 0, hi = 0;
#pragma unroll
            for (uint32_t r = 0; r < 32; ++r) {
                lo |= (((uint32_t)raw[r * rowb + col] >> sh) & 1u) << r;
                hi |= (((uint32_t)raw[(r + 32) * rowb + col] >> sh) & 1u) << r;
            }
            v = (uint64_t)lo | ((uint64_t)hi << 32);
        } else
            v = s_out[w][lane];
        if (v) reinterpret_cast<uint64_t *>(dst)[lane] = v;
    }
    const uint32_t tail = whole * 8u + lane;                                                  // the bytes behind the last whole element (< 8)
    if (tail < n && raw[tail]) dst[tail] = raw[tail];
}
void launch_blosc_decode_blocks(const uint8_t *data, const void *frame_lists, uint32_t nframes, uint32_t max_blocks_per_frame, uint8_t *out,
                                const uint64_t *out_base, int *err, hipStream_t s)
{
    if (!max_blocks_per_frame) return;
    hipLaunchKernelGGL(k_blosc_decode_blocks, dim3((max_blocks_per_frame + WAVES - 1) / WAVES, nframes), dim3(WG), 0, s, data,
                       reinterpret_cast<const ZdFrameList *>(frame_lists), out, out_base, err);
}

}  // namespace rc
