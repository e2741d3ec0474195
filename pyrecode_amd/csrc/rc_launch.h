// rc_launch.h - host-side launcher declarations shared by the .hip translation units of librecode_hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/recode_hip.h"
#include "rc_device.h"

namespace rc {

struct ZstdModel;      // rc_zstd_block.h
struct DeflateModel;   // rc_deflate_model.h
struct InfStream;      // rc_inflate.h

// Scratch::comb: where a tile's packed residual stream lives
constexpr uint32_t COMB_OFF = 0u;          // in pix_slots
constexpr uint32_t COMB_BEHIND_BLOCK = 1u; // in the block's slot, at the next 16-byte boundary behind the block image (LZ4 / blosc: the image is
                                           // final when the reduce kernel writes it)
constexpr uint32_t COMB_AT_BLK_SLOT = 2u;  // in the block's slot, at offset BLK_SLOT (zstd: the FSE pass and the frame's definitions still grow
                                           // the block)

// Device scratch of one ctx, laid out for a batch of up to max_batch frames (DESIGN.md "data layout in HBM").
struct Scratch {
    uint64_t N = 0;            // pixels per frame
    uint32_t ntiles = 0;       // ceil(N / TILE_PX)
    uint64_t nb = 0;           // ceil(N / 8) bitmap bytes per frame
    uint64_t nb_stride = 0;    // ntiles * TILE_BM (bitmap rows padded to whole tiles)
    uint32_t max_batch = 0;
    bool guarded_loads = false;        // every tile through the guarded single-load instantiation of the reduce kernel (tests: RC_REDUCE_GUARDED_LOADS=1
                                       // in the environment when the ctx is created; the product reads the switch nowhere else)
    uint16_t *thr = nullptr;           // [N]
    uint8_t *bitmap = nullptr;         // [B][nb_stride]            packed binary maps
    uint16_t *pix_slots = nullptr;     // [B][ntiles][TILE_PX]      per-tile residuals, row-major inside the tile
    uint32_t pix_slot_bytes = SLOT_PX * 2;   // bytes between two tiles' residual slots (uint32 sources, rc_reduce32.hip: TILE_PX * 4)
    uint32_t *tile_cnt = nullptr;      // [B][ntiles]               set pixels per tile
    uint32_t *tile_off = nullptr;      // [B][ntiles]               exclusive prefix of tile_cnt inside the frame
    uint32_t *tile_next = nullptr;     // [B][ntiles]               next tile index > t with tile_cnt > 0 (ntiles if none)
    uint8_t *blk_slots = nullptr;      // [B][ntiles][blk_stride]   encoded bitmap blocks (codec dependent); a ctx's level-1 pipeline keeps the
                                       //                           tile's residual stream in the same slot when both fit (`comb`)
    uint32_t blk_stride = BLK_SLOT;    // bytes between two tiles' block slots
    // Combined slots (a ctx with a device codec at level 1): the tile's packed residual stream sits BEHIND its encoded block in the block's
    // slot (COMB_* forms) whenever block + residual lines fit blk_stride; a tile too dense for that keeps its residuals in pix_slots as before.
    // One run of lines per tile and frame instead of two runs 8 KiB apart: fewer lines written by the reduce kernel and read by k_gather
    // (each run wastes half a line on average).
    uint32_t comb = COMB_OFF;
    uint32_t *blk_size = nullptr;      // [B][ntiles]               bytes used in each slot
    uint32_t *blk_aux = nullptr;       // [B][ntiles]               deflate: the tiles' Adler-32 partials (rc_deflate_block.h::deflate_adler_word)
    uint32_t *zl_acc = nullptr;        // [B][8]                    deflate: per frame {A, W of the map, A, W of the residual stream}
                                       //                           (zeroed by k_layout, summed up by k_gather, turned into the two trailers by k_zlib_finish)
    uint32_t *blk_off = nullptr;       // [B][ntiles]               exclusive prefix of blk_size inside the frame
    uint32_t *frame_nnz = nullptr;     // [B]
    uint32_t *frame_cbytes = nullptr;  // [B]                       sum of blk_size
    uint32_t *scan_part = nullptr;     // [B][nseg][8]              partial results of the segmented scans (frames with > 4096 tiles)
    BatchStatus *status = nullptr;     // [1] of this batch
    BatchStatus *first_err = nullptr;  // [1] shared by both scratch sets: first failed batch since the last rc_ctx_sync
                                       //     (code, frame, total = number of the batch among those enqueued since then)
    // The value stage (ValueStage below): one pipeline, two formats.  Allocated only for a ctx that has the stage.
    uint8_t *pixraw = nullptr;         // [B][pixraw_stride]           the frame's packed stream laid out flat (k_gather, PIX_MODE_FLAT)
    uint64_t pixraw_stride = 0;
    uint8_t *pix_chunks = nullptr;     // [B][nchunk_max][slot]        the encoded image of every chunk of the flat stream (chunk, slot: value_geom)
    uint32_t *chunk_size = nullptr;    // [B][nchunk_max]              the chunk's bytes in the record | the format's flag (ZW_TREE: treeless literals, PD_CODED)
    uint32_t *chunk_off = nullptr;     // [B][nchunk_max]              exclusive prefix of the sizes inside the frame
    uint32_t *frame_pbytes = nullptr;  // [B]                          the encoded stream behind its frame header (DEFLATE: the Adler-32 included)
    uint32_t nchunk_max = 0;           // chunks a frame can have
    // modelled zstd (CODEC_ZSTD_MODELLED, rc_zstd_model.h): the ctx's model on the device and what the block encoders need of it
    const ZstdModel *zm_model = nullptr;
    const void *zm_lit_code = nullptr; // &model->lit_code
    uint32_t zm_valid = 0, zm_budget = 0, zm_seq_bits = 12;
    // level 2 (rc_l2.hip)
    u32x2 *l2_node = nullptr;          // [B][ntiles * TILE_PX] {parent id, accumulator} per set pixel, id = tile * TILE_PX + rank in the tile
    uint64_t l2_ids_per_frame = 0;
    uint16_t *l2_base = nullptr;       // [B][ntiles * 64] set pixels of a word's tile in front of the word (k_l2_dir)
    // the value stage in DEFLATE's format (appended: every older field keeps its kernel-argument offset)
    uint32_t *chunk_aux = nullptr;     // [B][nchunk_max + 1][2]  the chunks' Adler-32 partials {A, W}; last entry: the stream's Adler-32
    const DeflateModel *dz_model = nullptr;   // the ctx's table (rc_deflate_model.h)
};

// RecordParams::emit / rc_ctx::emit: the form of a record's two streams (rc_record.h).  Also the batched decoder's selector (rc_reader.hip,
// rc_zstd_dec.hip).  rc_ctx_create sets emit = compression_scheme for a device codec, so the codecs' values are the scheme codes.
constexpr uint32_t EMIT_RAW = 0u;          // raw pieces (a mode-0 record): NOT compression_scheme 0 (zlib)
constexpr uint32_t EMIT_ZSTD = 1u;         // zstd frames
constexpr uint32_t EMIT_LZ4 = 2u;          // LZ4 frames
constexpr uint32_t EMIT_BLOSC = 8u;        // blosc1 chunks (bit-shuffle + LZ4)
constexpr uint32_t EMIT_DEFLATE = 0x100u;  // zlib streams of the device DEFLATE encoder
static_assert(EMIT_ZSTD == RC_SCHEME_ZSTD && EMIT_LZ4 == RC_SCHEME_LZ4 && EMIT_BLOSC == RC_SCHEME_BLOSC_LZ4 && EMIT_DEFLATE == RC_SCHEME_ZLIB_DEVICE,
              "rc_ctx_create assigns emit = compression_scheme");

// The block encoder fused into the reduce kernel (the CODEC template parameter, launch_reduce / launch_reduce32's codec); a ctx's one is
// chosen by rc_api.hip::fused_codec
constexpr int CODEC_NONE = 0;            // no encoded blocks: the raw binary maps only
constexpr int CODEC_ZSTD_FAST = 1;       // zstd, compression_level 0: raw literals, predefined tables (k_zstd_fse finishes the blocks)
constexpr int CODEC_LZ4_RUNS = 2;        // LZ4, compression_level 0: the run encoder (rc_lz4_block.h)
constexpr int CODEC_ZSTD_MODELLED = 3;   // zstd, compression_level >= 1: Huffman-coded literals, tokens for the ctx's fitted tables (rc_zstd_wave.h)
constexpr int CODEC_LZ4_EVENTS = 4;      // LZ4, compression_level >= 1: the event parser (rc_lz4_block.h)
constexpr int CODEC_DEFLATE = 5;         // a fixed-Huffman block per tile + its Adler-32 partials (rc_deflate_block.h)
constexpr int CODEC_BLOSC = 8;           // blosc1 block: bit-shuffle (typesize 8), then the LZ4 run encoder

// RecordParams::pix_mode: what k_gather / k_layout do with the level-1 residual stream
constexpr uint32_t PIX_MODE_STORED = 0u; // it goes into the record as it is (stored chunks)
constexpr uint32_t PIX_MODE_FLAT = 1u;   // ONLY the residual stream, flat, into Scratch::pixraw (input of the value stage)
constexpr uint32_t PIX_MODE_SKIP = 2u;   // everything but the residual stream, whose encoded size is Scratch::frame_pbytes

struct RecordParams {
    uint32_t level;        // 1 or 3
    uint32_t emit;         // EMIT_*
    uint32_t depth;        // source_bit_depth
    uint32_t packed_slots; // 1: the tiles' slots hold tile-local packed streams - level-1 residuals and, since round 5, level-2 statistics (k_l2_emit);
                           // 0: no value stream is gathered (no caller passes it any more)
    uint32_t first_frame_id;
    uint64_t frame_bytes;  // raw frame size = N * 2 (record upper bound, recode_writer.py:565-566)
    uint32_t pix_mode = PIX_MODE_STORED;
};

// rc_reduce.hip
void launch_threshold(const void *dark, int64_t eps, uint64_t N, uint16_t *thr, hipStream_t s, uint32_t src_bytes = 2);   // dark: uint16, or uint8 for src_bytes 1
// codec: CODEC_*.  level: 1 residuals, 2 raw values of the set pixels (input of launch_l2), 3 bitmap only.  depth < 16 (level 1 only):
// every tile's residuals are left in its slot already bit-packed (tile-local LSB-first stream of depth-bit fields)
// src_bytes: bytes per source pixel - 2 (uint16 frames) or 1 (uint8 frames, source_bit_depth <= 8)
void launch_reduce(const Scratch &sc, const void *frames, uint32_t B, uint32_t level, uint32_t codec, bool keep_bitmap,
                   uint32_t depth, hipStream_t s, hipStream_t s_tail = nullptr, uint32_t src_bytes = 2);
// rc_reduce32.hip: uint32 sources (source_bit_depth > 16) - reduce + d-bit pack, the block encoder of `codec` fused (every CODEC_* but
// CODEC_ZSTD_MODELLED and CODEC_DEFLATE); raw binary maps only with keep_bitmap
void launch_threshold32(const uint32_t *dark, int64_t eps, uint64_t N, uint32_t *thr, hipStream_t s);
void launch_reduce32(const Scratch &sc, const uint32_t *frames, const uint32_t *thr32, uint32_t B, uint32_t level, uint32_t depth, hipStream_t s,
                     uint32_t codec = CODEC_NONE, bool keep_bitmap = true);
// rc_l2.hip
void launch_l2(const Scratch &sc, uint32_t B, uint32_t nx, uint32_t use_sum, uint32_t depth, hipStream_t s);
void launch_scans(const Scratch &sc, uint32_t B, bool with_counts, bool with_blocks, hipStream_t s);
void launch_layout(const Scratch &sc, const RecordParams &rp, uint32_t B, uint64_t out_cap, uint64_t *rec_off,
                   uint32_t *md, hipStream_t s);
void launch_assemble(const Scratch &sc, const RecordParams &rp, uint32_t B, uint8_t *out, const uint64_t *rec_off,
                     uint32_t batch_seq, hipStream_t s);
// rc_gather.hip: k_gather, what launch_assemble runs for everything but level-2 value lists
void launch_gather(const Scratch &sc, const RecordParams &rp, uint32_t B, uint8_t *out, const uint64_t *rec_off, uint32_t hdr_bitmap, uint32_t hdr_pix,
                   uint32_t batch_seq, hipStream_t s);
// The value stage: a ctx's Huffman stage for the level-1 residual stream (uint16 / uint8 sources).  k_gather's flat pass into Scratch::pixraw ->
// encode (a wavefront per chunk) -> scan (sizes -> offsets, per frame) -> gather behind the binary-map stream (rc_values.h, rc_pix_huff.hip,
// rc_pix_deflate.hip), under a table fitted to a sample of the ctx's first batch (rc_api.hip::fit_value_model).
enum ValueStage : uint32_t {
    VALUES_NONE = 0,       // the stream is stored
    VALUES_ZSTD_HUFF,      // modelled zstd: a block of treeless Huffman-coded literals per 1008 bytes
    VALUES_DEFLATE_HUFF,   // device DEFLATE, compression_level >= 2: a dynamic-Huffman block per 32 KiB, the grid of the stored blocks (rc_record.h)
};
inline ValueStage value_stage_of(uint32_t emit, uint32_t clevel, uint32_t level)
{
    if (level == 1 && emit == EMIT_ZSTD && clevel != 0) return VALUES_ZSTD_HUFF;
    return level == 1 && emit == EMIT_DEFLATE && clevel >= 2 ? VALUES_DEFLATE_HUFF : VALUES_NONE;
}
constexpr uint32_t PIX_CHUNK = 1008, PIX_SLOT = 1024, PD_CHUNK = 1u << 15, PD_SLOT = PD_CHUNK + 32;   // (a coded DEFLATE image is < PD_CHUNK + 5 bytes)
struct ValueGeom { uint32_t chunk, slot; };   // bytes of the flat stream per chunk, bytes between two chunks' images in Scratch::pix_chunks
inline ValueGeom value_geom(ValueStage kind) { return kind == VALUES_DEFLATE_HUFF ? ValueGeom{PD_CHUNK, PD_SLOT} : ValueGeom{PIX_CHUNK, PIX_SLOT}; }
void launch_values_encode(ValueStage kind, const Scratch &sc, uint32_t B, uint32_t depth, hipStream_t s);
void launch_values_scan(ValueStage kind, const Scratch &sc, uint32_t B, uint32_t depth, hipStream_t s);
void launch_values_gather(ValueStage kind, const Scratch &sc, uint32_t B, uint32_t depth, uint32_t level1_hdr, uint8_t *out, const uint64_t *rec_off,
                          hipStream_t s);
void launch_pd_hist(const Scratch &sc, uint32_t B, uint32_t depth, uint32_t *hist_dev, hipStream_t s);   // the DEFLATE fit's sample: byte histogram of pixraw
// rc_lz4.hip
struct Lz4Block { uint64_t src_off; uint32_t size; uint32_t raw; };
void launch_lz4_encode_buffer(const Scratch &sc, hipStream_t s, bool events = false);  // sc.bitmap = the buffer, sc.nb = its length
void launch_lz4_encode_rows(const Scratch &sc, uint32_t B, hipStream_t s, bool events);   // B rows of sc.bitmap (a batch's raw binary maps)
void launch_lz4f_gather(const Scratch &sc, uint32_t hdr3, uint8_t *out, hipStream_t s);
void launch_lz4_decode(const uint8_t *src, const Lz4Block *blks, uint32_t nblk, uint32_t *sizes, const uint64_t *dst_off,
                       uint8_t *dst, uint64_t cap, int linked, int *err, hipStream_t s, uint32_t max_stored = 0);
uint32_t lz4f_descriptor(uint8_t bd);
// rc_blosc.hip
void launch_blosc_encode_blocks(const Scratch &sc, uint32_t B, hipStream_t s);
void launch_blosc_gather(const Scratch &sc, uint8_t *out, hipStream_t s);
void launch_blosc_unshuffle(const uint8_t *in, uint8_t *out, uint64_t nbytes, uint32_t blocksize, uint32_t typesize,
                            uint32_t shuffle, hipStream_t s);
// rc_zstd.hip
void launch_zstd_encode_blocks(const Scratch &sc, uint32_t B, const void *tables_dev, hipStream_t s);
void launch_zstd_tokenize_rows(const Scratch &sc, uint32_t B, hipStream_t s);   // the tokenizer half only (launch_zstd_fse finishes the blocks)
void launch_zstd_fse(const Scratch &sc, uint32_t B, const void *tables_dev, bool fitted, hipStream_t s);  // 2nd half of the fused path
// modelled encoder (rc_zstd_model.h): histograms of a sample of plain-tokenized frames -> model (host) -> kernels
void launch_zstd_sample(const Scratch &sc, uint32_t B, bool with_pix, uint32_t depth, void *sample_dev, hipStream_t s);
size_t zstd_model_bytes();
size_t zstd_sample_bytes();
void zstd_model_from_sample(const void *sample_host, void *model_host, uint32_t speed_permille = 0);   // (rc_zstd_model.h::zm_build_model)
void launch_zstd_gather(const Scratch &sc, uint8_t *out, hipStream_t s);
size_t zstd_tables_bytes();
void zstd_tables_host(void *dst);  // rc_reduce.hip: FLG | BD << 8 | HC << 16

// where tile ft's packed residual stream starts (see Scratch::comb); bn: the tile's blk_size word as the reduce kernel wrote it
// (COMB_BEHIND_BLOCK only), cnt: its set pixels, d: bits per value
template <class S>
__host__ __device__ inline const uint8_t *residual_src(const S &sc, uint64_t ft, uint32_t bn, uint32_t cnt, uint32_t d)
{
    if (sc.comb) {
        const uint32_t ro16 = sc.comb == COMB_AT_BLK_SLOT ? (uint32_t)BLK_SLOT / 16 : (bn + 15) >> 4, r16 = (cnt * d + 127) >> 7;
        if (16 * (ro16 + r16) <= sc.blk_stride) return sc.blk_slots + ft * sc.blk_stride + 16 * ro16;
    }
    return reinterpret_cast<const uint8_t *>(sc.pix_slots) + ft * sc.pix_slot_bytes;
}

// rc_inflate.hip: the batched device inflate of rc_expand_frames.  streams: n_map binary-map streams, then n_val value streams; *_cap_max /
// *_units_max: the largest candidate room / unit count among them; cand_pos, link: one entry per candidate room, unit_cand: per unit, ncand: per stream
void launch_inflate(const uint8_t *data, const InfStream *streams, uint32_t n_map, uint32_t n_val, uint32_t map_cap_max, uint32_t map_units_max,
                    uint32_t val_cap_max, uint32_t val_units_max, uint32_t *cand_pos, uint32_t *ncand, uint32_t *link, uint32_t *unit_cand,
                    uint8_t *out, int *err, hipStream_t s);

void launch_roi_components(const void *frames, const void *thr, uint64_t N, uint32_t nx, uint32_t n, uint32_t first_frame_id, uint32_t gap,
                           uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, uint32_t *counts, hipStream_t s, uint32_t src_bytes = 2);

// rc_calib.hip - calibration: per-pixel median / std / range, histogram of frame - median, accurate thresholds
constexpr uint32_t CALIB_LDS_MAX_FRAMES = 512;   // the longest column a one-wave workgroup stages in LDS (512 frames x 128 bytes = 64 KiB)
void launch_calib_stats(const uint16_t *stack, uint32_t n, uint64_t N, uint32_t n_stats, float *median, float *sdev, int32_t *range2, hipStream_t s);
void launch_calib_hist(const uint16_t *frames, uint32_t n_stats, uint64_t N, const float *median, const double *edges, uint32_t n_bins,
                       uint64_t *counts, hipStream_t s);
void launch_calib_top(const uint16_t *stack, uint32_t n, uint64_t N, const float *median, uint32_t k, float *acc, uint64_t *n_undefined, hipStream_t s);
}  // namespace rc
