// rc_pix_deflate.hip - Huffman coding of the residual-intensity stream for the device DEFLATE encoder at compression_level >= 2 (gfx950).
//
// Replaces the second `compress()` of the reference's per-frame step for compression_scheme 0, zlib.compress(packed_residuals, level)
// (pyrecode/recode_writer.py:507-511 -> recode_compressors.py:84-85).  The packed stream has no repeats worth finding, so every 32 KiB
// chunk of it (the grid of the stored blocks, rc_record.h) becomes one dynamic-Huffman block of literals under the ctx's table
// (rc_deflate_model.h), or stays the stored block it was when that would not be smaller.  Serial statement of the stream:
// tests/deflate_values_model.py::encode_values, judged by stock zlib in tests/test_deflate_values_cpu.py.
//
//   k_pd_hist     byte histogram of a sample's flat residual streams (the table is fitted to it on the host)
//   k_pd_encode   one wavefront per chunk of the flat stream (Scratch::pixraw, k_gather's PIX_MODE_FLAT pass).  First a sizing pass - the
//                 chunk's bit count under the table and its Adler-32 partials -, which decides coded / stored; a coded chunk is then built
//                 in windows of 1024 bytes: 16 bytes per lane, code lookups in an LDS copy of the table, one wave scan of the bit sizes, LDS
//                 ORs into a zeroed window, whole dwords flushed to the chunk's slot, the open dword and the bit position carried on
//   k_pd_scan     per frame: chunk sizes -> offsets, the stream's length and its Adler-32
//   k_pd_gather   a wavefront per chunk: the coded image from its slot, or the stored block straight from the flat stream, behind the
//                 binary-map stream; chunk 0's wavefront also writes the two header bytes and the trailer
#include <algorithm>

#include "rc_values.h"
#include "rc_deflate_block.h"
#include "rc_deflate_model.h"

namespace rc {

constexpr int PD_WG_PER_FRAME = 16;             // at most: x WAVES wavefronts loop over a frame's chunks (11 chunks per 4096^2 frame at 1 %, d = 16)
constexpr uint32_t PD_WIN = 1024;               // bytes per window: 16 per lane
constexpr int PD_DW = 392;                      // LDS dwords per wavefront: the open dword + 1024 * 12 bits + slack for the OR of a straddling group
constexpr uint32_t PD_CODED = 0x80000000u;      // chunk_size: the slot holds a coded image (otherwise the chunk is a stored block of the flat stream)

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) { return wave_last(wave_incl_scan(v)); }
// the wavefront's LDS window passes from one phase to the next (all lanes' accesses of the phase before are ordered in front)
__device__ __forceinline__ void pd_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

__global__ __launch_bounds__(WG) void k_pd_hist(Scratch sc, uint32_t depth, uint32_t *__restrict__ hist)
{
    __shared__ uint32_t s_hist[256];
    s_hist[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t f = blockIdx.y, npk = packed_bytes(sc.frame_nnz[f], depth);
    const uint8_t *src = sc.pixraw + (uint64_t)f * sc.pixraw_stride;
    for (uint32_t o = 16u * (blockIdx.x * WG + threadIdx.x); o < npk; o += 16u * WG * gridDim.x) {
        const u32x4 v = *reinterpret_cast<const u32x4 *>(src + o);   // rows are 16-byte aligned and padded
        const uint32_t vb = min(16u, npk - o);
        for (uint32_t i = 0; i < vb; ++i) atomicAdd(&s_hist[(v[i >> 2] >> (8 * (i & 3))) & 0xFFu], 1u);
    }
    __syncthreads();
    if (s_hist[threadIdx.x]) atomicAdd(&hist[threadIdx.x], s_hist[threadIdx.x]);
}

void launch_pd_hist(const Scratch &sc, uint32_t B, uint32_t depth, uint32_t *hist, hipStream_t s)
{
    static_assert(WG == 256, "k_pd_hist: a thread per byte value");
    hipLaunchKernelGGL(k_pd_hist, dim3(16, B), dim3(WG), 0, s, sc, depth, hist);
}

// the lane's 16 bytes of a window (zero beyond the chunk's end) and how many of them are valid
__device__ __forceinline__ u32x4 pd_load(const uint8_t *src, uint32_t n, uint32_t off, int &vb)
{
    vb = off < n ? (int)min(16u, n - off) : 0;
    u32x4 v = {0u, 0u, 0u, 0u};
    if (vb > 0) v = *reinterpret_cast<const u32x4 *>(src + off);   // rows and chunks are 16-byte aligned, rows padded
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int nb = vb - 4 * k;
        if (nb < 4) v[k] = nb <= 0 ? 0u : v[k] & ((1u << (8 * nb)) - 1u);
    }
    return v;
}

__global__ __launch_bounds__(WG) void k_pd_encode(Scratch sc, uint32_t B, uint32_t depth)
{
    __shared__ uint16_t s_code[DM_SYMS + 3];
    __shared__ uint32_t s_hdr[DM_HDR_WORDS];
    __shared__ __attribute__((aligned(16))) uint32_t s_out[WAVES][PD_DW];
    const DeflateModel *M = sc.dz_model;
    if (threadIdx.x < (DM_SYMS + 3) / 2) reinterpret_cast<uint32_t *>(s_code)[threadIdx.x] = reinterpret_cast<const uint32_t *>(M->code)[threadIdx.x];
    if (threadIdx.x < DM_HDR_WORDS) s_hdr[threadIdx.x] = M->hdr[threadIdx.x];
    __syncthreads();
    const uint32_t f = blockIdx.y;
    if (f >= B) return;
    const uint32_t lane = (uint32_t)lane_id();
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t npk = packed_bytes(sc.frame_nnz[f], depth);
    const uint32_t nch = value_chunks(npk, PD_CHUNK);
    const uint32_t hdr_bits = M->hdr_bits, usable = M->usable;
    const uint32_t eob = s_code[DM_EOB] & 0xFFFu, eob_len = s_code[DM_EOB] >> 12;
    uint32_t *o = s_out[w];
    for (uint32_t c = blockIdx.x * WAVES + w; c < nch; c += gridDim.x * WAVES) {
        const uint32_t n = min(PD_CHUNK, npk - c * PD_CHUNK);   // (npk == 0: one empty stored block)
        const bool last = c + 1 == nch;
        const uint8_t *src = sc.pixraw + (uint64_t)f * sc.pixraw_stride + (uint64_t)c * PD_CHUNK;
        // ---- sizing pass: bits under the table; Adler-32 partials A = sum of the bytes, W = sum of stream position * byte (mod 65521) ----
        uint32_t lbits = 0, lA = 0, lW = 0;
        for (uint32_t w0 = 0; w0 < n; w0 += PD_WIN) {
            int vb;
            const uint32_t off = w0 + 16u * lane;
            const u32x4 v = pd_load(src, n, off, vb);
            uint32_t a = 0, q = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (4 * k + j < vb) lbits += s_code[(v[k] >> (8 * j)) & 0xFFu] >> 12;
                a = __builtin_amdgcn_sad_u8(v[k], 0u, a);
                q = __builtin_amdgcn_udot4(v[k], 0x03020100u + 0x04040404u * (uint32_t)k, q, false);
            }
            lA += a;                                                                    // <= 32 windows * 4080
            lW = (lW + ((c * PD_CHUNK + off) % ADLER_P) * a + q) % ADLER_P;             // < 65521 * 4080 + 30600 + 65521 < 2^32
        }
        const uint32_t bits = hdr_bits + wave_sum(lbits) + eob_len;
        const uint32_t size = last ? (bits + 7) >> 3 : ((bits + 3 + 7) >> 3) + 4;
        const bool coded = usable && n && size < n + 5;
        const uint32_t A = wave_sum(lA % ADLER_P) % ADLER_P, W = wave_sum(lW) % ADLER_P;
        const uint64_t fc = (uint64_t)f * sc.nchunk_max + c;
        if (lane == 0) {
            sc.chunk_size[fc] = coded ? size | PD_CODED : n + 5;
            sc.chunk_aux[2 * ((uint64_t)f * (sc.nchunk_max + 1) + c)] = A;
            sc.chunk_aux[2 * ((uint64_t)f * (sc.nchunk_max + 1) + c) + 1] = W;
        }
        if (!coded) continue;   // (wave-uniform)
        // ---- the image: header bits, literals window by window, end of block, sync marker or padding --------------------------------------
        uint32_t *slot = reinterpret_cast<uint32_t *>(sc.pix_chunks + fc * PD_SLOT);
        uint32_t gpos = 0;      // dwords of the slot written
        // whole dwords of the window's first `tb` bits -> the slot; the open dword moves to the window's front, the rest is zeroed
        auto flush = [&](uint32_t tb) {
            const uint32_t nfull = tb >> 5;
            for (uint32_t i = lane; i < nfull; i += 64) slot[gpos + i] = o[i];
            const uint32_t open = o[nfull];
            pd_sync();
            for (uint32_t i = lane; i < (uint32_t)PD_DW; i += 64) o[i] = i == 0 ? open : 0u;
            pd_sync();
            gpos += nfull;
            return tb & 31u;
        };
        pd_sync();
        for (uint32_t i = lane; i < (uint32_t)PD_DW; i += 64) o[i] = i < (uint32_t)DM_HDR_WORDS ? (s_hdr[i] | (i == 0 && last ? 1u : 0u)) : 0u;   // (hdr is zero behind its bits)
        pd_sync();
        uint32_t carry = flush(hdr_bits);
        for (uint32_t w0 = 0; w0 < n; w0 += PD_WIN) {
            int vb;
            const u32x4 v = pd_load(src, n, w0 + 16u * lane, vb);
            uint64_t g[4];
            uint32_t gb[4];
            const uint32_t nb = value_codes<false>(v, vb, s_code, g, gb);
            const uint32_t binc = wave_incl_scan(nb);
            const uint32_t tot = wave_last(binc);
            uint32_t bit = carry + binc - nb;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (gb[k]) {
                    window_or(o, bit, g[k]);
                    bit += gb[k];
                }
            pd_sync();
            carry = flush(carry + tot);
        }
        // end of block at bit `carry` (< 32) of the window; then, unless this is the stream's last block, an empty stored block (000, pad,
        // LEN 0, NLEN FFFF: the next chunk starts on a byte), else padding to the byte
        uint32_t bit = carry + eob_len;
        uint32_t mark = 0;
        if (!last) { bit = (bit + 3 + 7) & ~7u; mark = bit; bit += 32; }
        else bit = (bit + 7) & ~7u;
        if (lane == 0) {
            const uint64_t e = (uint64_t)eob << carry;
            o[0] |= (uint32_t)e;
            o[1] |= (uint32_t)(e >> 32);
            if (!last) {
                const uint64_t m = 0xFFFF0000ull << (mark & 31u);
                o[mark >> 5] |= (uint32_t)m;
                o[(mark >> 5) + 1] |= (uint32_t)(m >> 32);
            }
        }
        pd_sync();
        for (uint32_t i = lane; i < (bit + 31) >> 5; i += 64) slot[gpos + i] = o[i];   // (4 * gpos + bit / 8 == size <= n + 4: inside the slot)
        pd_sync();
    }
}

// (DEFLATE: at most PD_WG_PER_FRAME workgroups per frame, fewer where a frame cannot have that many chunks)
static dim3 pd_grid(const Scratch &sc, uint32_t B) { return dim3(std::min((sc.nchunk_max + WAVES - 1) / WAVES, (uint32_t)PD_WG_PER_FRAME), B); }

void launch_values_encode(ValueStage kind, const Scratch &sc, uint32_t B, uint32_t depth, hipStream_t s)
{
    if (kind == VALUES_ZSTD_HUFF) return launch_pix_huff(sc, B, depth, s);
    if (kind == VALUES_DEFLATE_HUFF) hipLaunchKernelGGL(k_pd_encode, pd_grid(sc, B), dim3(WG), 0, s, sc, B, depth);   // (VALUES_NONE: no table, no flat stream - nothing to launch)
}

// per frame: the chunks' sizes -> offsets behind the stream's two header bytes; frame_pbytes = images + trailer; the Adler-32 from the partials
__global__ __launch_bounds__(WG) void k_pd_scan(Scratch sc, uint32_t depth)
{
    __shared__ uint32_t s_sz[WG], s_A[WG], s_W[WG];
    const uint32_t f = blockIdx.x, t = threadIdx.x;
    const uint32_t npk = packed_bytes(sc.frame_nnz[f], depth);
    const uint32_t nch = value_chunks(npk, PD_CHUNK);
    const uint32_t per = (nch + WG - 1) / WG, lo = min(t * per, nch), hi = min(lo + per, nch);
    const uint32_t *size = sc.chunk_size + (uint64_t)f * sc.nchunk_max;
    uint32_t *aux = sc.chunk_aux + 2 * (uint64_t)f * (sc.nchunk_max + 1);
    uint32_t sum = 0, A = 0, W = 0;
    for (uint32_t c = lo; c < hi; ++c) {
        sum += size[c] & ~PD_CODED;
        A = (A + aux[2 * c]) % ADLER_P;
        W = (W + aux[2 * c + 1]) % ADLER_P;
    }
    s_sz[t] = sum; s_A[t] = A; s_W[t] = W;
    __syncthreads();
    uint32_t base = 0;
    for (uint32_t i = 0; i < t; ++i) base += s_sz[i];
    for (uint32_t c = lo; c < hi; ++c) {
        sc.chunk_off[(uint64_t)f * sc.nchunk_max + c] = base;
        base += size[c] & ~PD_CODED;
    }
    if (t == WG - 1) {
        uint32_t tA = 0, tW = 0;
        for (uint32_t i = 0; i < (uint32_t)WG; ++i) { tA = (tA + s_A[i]) % ADLER_P; tW = (tW + s_W[i]) % ADLER_P; }
        sc.frame_pbytes[f] = base + 4;
        aux[2 * sc.nchunk_max] = adler_from_sums(npk, tA, tW);
    }
}

void launch_values_scan(ValueStage kind, const Scratch &sc, uint32_t B, uint32_t depth, hipStream_t s)
{
    if (kind == VALUES_ZSTD_HUFF) return launch_pix_scan(sc, B, depth, s);
    if (kind == VALUES_DEFLATE_HUFF) hipLaunchKernelGGL(k_pd_scan, dim3(B), dim3(WG), 0, s, sc, depth);   // (VALUES_NONE: no table, no flat stream - nothing to launch)
}

__global__ __launch_bounds__(WG) void k_pd_gather(Scratch sc, uint32_t B, uint32_t depth, uint32_t rec_hdr, uint8_t *__restrict__ out,
                                                    const uint64_t *__restrict__ rec_off)
{
    const uint32_t f = blockIdx.y;
    if (f >= B || sc.status->code != 0) return;
    const uint32_t lane = (uint32_t)lane_id();
    const uint32_t w = threadIdx.x >> 6;
    const uint32_t npk = packed_bytes(sc.frame_nnz[f], depth);
    const uint32_t nch = value_chunks(npk, PD_CHUNK);
    const FrameFmt ff = frame_fmt(EMIT_DEFLATE);
    // the residual stream starts behind the record header and the binary-map stream: [78 01][chunk images][Adler-32]
    uint8_t *pf = out + rec_off[f] + rec_hdr + ff.hdr + sc.frame_cbytes[f] + ff.end;
    for (uint32_t c = blockIdx.x * WAVES + w; c < nch; c += gridDim.x * WAVES) {
        const uint64_t fc = (uint64_t)f * sc.nchunk_max + c;
        const uint32_t word = sc.chunk_size[fc], off = sc.chunk_off[fc];
        uint8_t *dst = pf + ff.hdr + off;
        if (word & PD_CODED) wave_copy_unaligned(dst, sc.pix_chunks + fc * PD_SLOT, word & ~PD_CODED, lane);
        else {   // stored block: [BFINAL][LEN][NLEN] and the chunk of the flat stream as it is
            const uint32_t n = word - 5;
            if (lane == 0) {
                dst[0] = c + 1 == nch ? 1 : 0;
                dst[1] = (uint8_t)n; dst[2] = (uint8_t)(n >> 8); dst[3] = (uint8_t)~n; dst[4] = (uint8_t)(~n >> 8);
            }
            wave_copy_unaligned(dst + 5, sc.pixraw + (uint64_t)f * sc.pixraw_stride + (uint64_t)c * PD_CHUNK, n, lane);
        }
        if (c == 0 && lane == 0) {
            pf[0] = 0x78; pf[1] = 0x01;   // CMF, FLG as the binary-map stream's (rc_record.h)
            store_u32_be(pf + ff.hdr + sc.frame_pbytes[f] - 4, sc.chunk_aux[2 * ((uint64_t)f * (sc.nchunk_max + 1) + sc.nchunk_max)]);
        }
    }
}

void launch_values_gather(ValueStage kind, const Scratch &sc, uint32_t B, uint32_t depth, uint32_t rec_hdr, uint8_t *out, const uint64_t *rec_off,
                          hipStream_t s)
{
    if (kind == VALUES_ZSTD_HUFF) return launch_pix_gather(sc, B, depth, rec_hdr, out, rec_off, s);
    if (kind == VALUES_DEFLATE_HUFF) hipLaunchKernelGGL(k_pd_gather, pd_grid(sc, B), dim3(WG), 0, s, sc, B, depth, rec_hdr, out, rec_off);   // (VALUES_NONE: no table, no flat stream - nothing to launch)
}

}  // namespace rc
