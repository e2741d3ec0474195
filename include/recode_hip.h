/* recode_hip.h - C ABI of librecode_hip.so: the MI355X (gfx950) implementation of pyReCoDe's per-frame
 * reduce -> bit-pack -> compress hot path and of the reader's sparse expand.
 *
 * This is the drop-in boundary.  Plain C: pointers and sizes only, no torch / HIP types.
 * Every entry point names the reference interface it replaces (paths relative to the reference repo).
 * All kernels behind it are hand-written HIP for gfx950; there is NO CPU fallback in this library: on a
 * machine without a usable GPU every compute entry point returns RC_ERR_DEVICE.
 *
 * Conventions
 *   - Return value: RC_OK (0) or a negative rc_status.  Nothing throws across the ABI.
 *   - Buffers are caller-owned (as in the reference: recode_writer.py:229-230, recode_reader.py:115).
 *     A data pointer may be host memory or device memory of the ctx's GPU; the library detects which
 *     (hipPointerGetAttributes) and stages host buffers itself.  It never allocates or frees caller memory.
 *   - A ctx is bound to one GPU and one HIP stream and is not thread-safe; distinct ctxs are independent
 *     (reference: one ReCoDeWriter per process, recode_server.py:358-363).
 *   - All multi-byte fields the library writes are little-endian (reference uses sys.byteorder on x86).
 *   - Ordering of device pointers: the library works on streams of its own (non-blocking streams: they do not wait for the legacy null
 *     stream or for any stream of the caller).  Device memory handed to a synchronous or stateless entry point must therefore be
 *     COMPLETE when the call is made - the caller synchronises the stream that produced it first (torch: torch.cuda.synchronize(), or
 *     the producing stream's synchronize()) -, and what such a call wrote to device memory is complete when it returns.  Only the
 *     asynchronous ctx entry points order themselves on a stream the caller names (rc_ctx_set_stream, rc_ctx_wait_results).
 */
#ifndef RECODE_HIP_H
#define RECODE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RC_ABI_VERSION 3

typedef enum rc_status {
    RC_OK = 0,
    RC_ERR_BAD_ARG = -1,          /* python shim: ValueError */
    RC_ERR_OUT_TOO_SMALL = -2,    /* caller's output capacity insufficient; nothing useful written */
    RC_ERR_DEVICE = -3,           /* no GPU / HIP error; rc_last_error() has the HIP message; python: RuntimeError */
    RC_ERR_UNSUPPORTED = -4,      /* scheme / level not implemented on device; python: NotImplementedError
                                     (recode_compressors.py:78-79,119-120) */
    RC_ERR_RECORD_TOO_LARGE = -5, /* a record exceeds the raw frame size; python: ValueError('Buffer size smaller
                                     than compressed data size') (recode_writer.py:565-566) */
    RC_ERR_CORRUPT = -6,          /* malformed compressed stream / bitmap-vs-pixvals mismatch on the read side */
    RC_ERR_WORKSPACE = -7         /* the device memory a ctx or a call needs could not be allocated (hipErrorOutOfMemory; rc_last_error
                                     names the allocation): python MemoryError.  A ctx's scratch is sized by its geometry and max_batch
                                     alone - per frame of the batch and scratch set (two sets): 2 * nx * ny bytes of residual slots +
                                     ceil(nx * ny / 4096) * 1.5 KiB of block slots (reduction level 2 adds 8 bytes per pixel and frame
                                     for the labelling nodes, a second copy of them once the ctx is pipelined) - so a ctx that was
                                     created never runs out of memory in a batch */
} rc_status;

/* compression_scheme codes of the reference (recode_compressors.py:3-4, config/README.md). Device codecs:
 * 2 (LZ4 frame), 1 (zstd frame), 8 (blosc1 chunk: bit-shuffle + LZ4, typesize 8).  Every other code: the ctx emits the
 * reduce-only pieces and the host layer runs the reference's own library call (zlib, bz2, lzma, ...).
 * RC_SCHEME_ZLIB_DEVICE is not a code of the reference: a ctx created with it writes compression_scheme 0 records (file header
 * field 0, recode_compressors.py:42-43,84-85) whose two streams are zlib streams (RFC 1950) made by the device's own DEFLATE
 * encoder - a byte-aligned fixed-Huffman block per 512-byte tile of the binary map, stored blocks for the packed values, Adler-32
 * trailers - which `zlib.decompress` (the reference's reader, recode_compressors.py:43) expands to the exact bytes; like every other
 * device codec it promises a VALID stream, not stock zlib's bytes (RC_SCHEME_ZLIB through the host layer keeps those).
 * compression_level: 0 / 1 as above.  From 2 on (reduction level 1) the packed values are Huffman-coded: every 32 KiB chunk that pays
 * becomes a literals-only dynamic-Huffman block (RFC 1951 BTYPE 10) under ONE table per ctx, fitted to (up to two frames of) the ctx's
 * first batch - rc_ctx_refit_model fits it again -, every other chunk stays the stored block it was, so a record never grows; a ctx
 * whose sample the byte-wise code cannot shrink by 3 % (bit-packed depths such as 12) keeps the stored form.  The workspace of such a ctx
 * holds the flat value stream and the chunk images besides (about two raw frames per frame of a batch, per scratch set).  Reduction
 * levels 2 and 3 write at every level what they write at level 1. */
enum { RC_SCHEME_ZLIB = 0, RC_SCHEME_ZSTD = 1, RC_SCHEME_LZ4 = 2, RC_SCHEME_BLOSC_LZ4 = 8, RC_SCHEME_ZLIB_DEVICE = 0x100 };

typedef struct rc_ctx rc_ctx;

/* ---- library ------------------------------------------------------------------------------------- */
int rc_abi_version(void);
const char *rc_strerror(int status);
const char *rc_last_error(void);                 /* thread-local detail of the last failure */
int rc_device_count(int *count);                 /* RC_OK with *count == 0 when no GPU is visible */
int rc_scheme_on_device(uint32_t scheme);        /* 1 if rc_reduce_compress_batch emits this scheme itself */

/* ---- seam 1: the per-frame operator, batched ---------------------------------------------------------
 * Replaces ReCoDeWriter._reduce_compress (pyrecode/recode_writer.py:430-557) and the buffers ReCoDeWriter.start()
 * allocates for it (:212-230).  One ctx == one writer (one node_id).
 *
 *   nx, ny            frame shape (header fields nx, ny; recode_header.py:66-67)
 *   src_bit_depth     source_bit_depth, 1..32: pixvals are bit-packed when it is not a multiple of 8 (recode_writer.py:463-475);
 *                     up to 8 the reference's source dtype is uint8, beyond 16 uint32: rc_ctx_set_source_bytes(ctx, 1 / 4)
 *   reduction_level   1 (binary map + residuals), 2 (binary map + one statistic per 8-connected component, see
 *                     rc_ctx_set_l2_statistics) or 3 (binary map only); 4 -> RC_ERR_UNSUPPORTED
 *   op_mode           rc_operation_mode: 0 reduce only, 1 reduce + compress (recode_writer.py:482,497)
 *   scheme, clevel    compression_scheme / compression_level (recode_writer.py:503-511)
 *   device_id         HIP device ordinal
 *   max_batch         largest n later passed to rc_reduce_compress_batch (1 .. 65535: a batch's frames are a launch's grid.y); sizes the device scratch
 */
rc_ctx *rc_ctx_create(uint32_t nx, uint32_t ny, uint32_t src_bit_depth, uint32_t reduction_level,
                      uint32_t op_mode, uint32_t scheme, uint32_t clevel, int device_id, uint32_t max_batch,
                      int *status);
int rc_ctx_destroy(rc_ctx *ctx);

/* Reduction level 2 only: which statistic of the RAW frame values each connected component contributes (header field
 * L2_statistics, recode_writer.py:358-365): 0 or 1 = maximum, 2 = sum modulo 2^src_bit_depth - the reference casts the
 * statistic to the source dtype and stores it in src_bit_depth bits like every pixel value (recode_writer.py:446,463-475),
 * so a sum that does not fit wraps.
 * Components are listed in scipy.ndimage.label order, i.e. by their first pixel in row-major order
 * (recode_writer.py:443-446, utils/converters.py:262-297 - restated by intent, the reference's own code cannot run). */
int rc_ctx_set_l2_statistics(rc_ctx *ctx, uint32_t l2_statistics);

/* Use a caller-provided hipStream_t (passed as void*) instead of the ctx's own stream, e.g. torch's current
 * stream so that caller-side events bracket the kernels.  NULL restores the ctx's own stream (so the legacy null
 * stream, whose handle is 0, cannot be selected: use a created stream). */
int rc_ctx_set_stream(rc_ctx *ctx, void *hip_stream);

/* Bytes per SOURCE pixel - the reference's Python path takes whatever its map_dtype yields for the source bit depth (misc.py:41-49; only
 * use_c is uint16-only, recode_writer.py:85-87): 2 (default: uint16 frames and dark, 9..16 bits), 1 (uint8, <= 8 bits) or 4 (uint32, 17..32 bits).
 * Call before rc_set_dark and the first batch.  Every `frames` / `dark` pointer below is then of that type, a raw frame is ny*nx*bytes
 * (rc_out_capacity, the record bound of recode_writer.py:565-566).  uint8: a uint8 instantiation of the load path (half the bytes); everything
 * behind the loads is the uint16 path.  uint32 (levels 1 and 3): a kernel of its own for the reduce step (rc_reduce32.hip: uint32 compare,
 * residuals and depth-bit fields - four raw bytes a value when the depth is a multiple of 8, 24 included, as `.tobytes()` gives them,
 * recode_writer.py:463-464) with every device codec's block encoder fused into it as in the uint16 kernel (LZ4, blosc-lz4, zstd in its fast
 * form - the modelled encoder and reduction level 2 are uint16 / uint8 only); scans, record layout and assembly are shared.  rc_set_threshold then takes a uint32 frame. */
int rc_ctx_set_source_bytes(rc_ctx *ctx, uint32_t bytes_per_pixel);
uint32_t rc_ctx_source_bytes(const rc_ctx *ctx);

/* thr = calibration frame + epsilon in the source dtype's arithmetic (wraps mod 2^16 - mod 2^8 for uint8 sources - like NumPy 2):
 * ReCoDeWriter.__init__, recode_writer.py:126-137.  dark: uint16[ny*nx] (uint8[ny*nx] after rc_ctx_set_source_bytes(ctx, 1)), C order. */
int rc_set_dark(rc_ctx *ctx, const void *dark, int64_t epsilon);
/* Or hand over the finished threshold frame (self._calibration_frame_p_threshold). */
int rc_set_threshold(rc_ctx *ctx, const void *thr);   /* uint16[ny*nx] (uint8 and uint16 sources), uint32[ny*nx] (uint32 sources) */

/* Worst-case bytes one batch of n frames can occupy in `out` (n * raw frame size, the reference's own bound,
 * recode_writer.py:217-218,565-566), and the number of u32 metadata fields per frame for this ctx's
 * (level, mode) (structures.py:18-46): L1/mode1 3, L1/mode0 1, L3/mode1 1, L3/mode0 0. */
uint64_t rc_out_capacity(const rc_ctx *ctx, uint32_t n);
uint32_t rc_md_fields(const rc_ctx *ctx);

/* n frames in, n part-file records out.
 *   frames         uint16[n][ny][nx] C order (host or device); uint8[n][ny][nx] after rc_ctx_set_source_bytes(ctx, 1)
 *   first_frame_id absolute_frame_index of frames[0] (recode_writer.py:385); frame i gets first_frame_id + i
 *   out            records back to back, byte-identical in layout to what _write_to_frame_buffer assembles
 *                  (recode_writer.py:485-494,518-525,546-550):
 *                    L1 mode 1: u32 frame_id | u32 n_comp_bitmap | u32 n_comp_pix | u32 n_packed_pix | comp_bitmap | comp_pix
 *                    L1 mode 0: u32 frame_id | u32 n_packed_pix | bitmap[ceil(nx*ny/8)] | packed_pix
 *                    L3 mode 1: u32 frame_id | u32 n_comp_bitmap | comp_bitmap
 *                    L3 mode 0: u32 frame_id | bitmap
 *                  With op_mode 1 and a scheme that is not a device codec the ctx emits the mode-0 record and the
 *                  host layer compresses (see rc_scheme_on_device).
 *   out_cap        capacity of out in bytes
 *   rec_offsets    uint64[n+1]: record i is out[rec_offsets[i] .. rec_offsets[i+1])
 *   md             uint32[n][3]: the record's metadata fields after frame_id, zero padded to 3
 * Synchronous: returns after the records (and offsets, md) are readable by the caller.
 * RC_ERR_RECORD_TOO_LARGE / RC_ERR_OUT_TOO_SMALL leave out undefined. */
int rc_reduce_compress_batch(rc_ctx *ctx, const void *frames, uint32_t n, uint32_t first_frame_id,
                             uint8_t *out, uint64_t out_cap, uint64_t *rec_offsets, uint32_t *md);

/* Asynchronous form for device-resident pipelines: every pointer must be device memory; work is enqueued on the
 * ctx's stream and nothing is read back.  rc_ctx_sync waits for all enqueued batches and returns RC_OK, or the status
 * of the FIRST batch that failed since the previous sync (RC_ERR_RECORD_TOO_LARGE, RC_ERR_OUT_TOO_SMALL;
 * rc_last_error names the batch and frame); later batches are unaffected by an earlier failure. */
int rc_reduce_compress_batch_async(rc_ctx *ctx, const void *frames_dev, uint32_t n, uint32_t first_frame_id,
                                   uint8_t *out_dev, uint64_t out_cap, uint64_t *rec_offsets_dev, uint32_t *md_dev);
int rc_ctx_sync(rc_ctx *ctx);

/* Pipelining across batches (off by default).  A batch is two stages: the reduce kernel on the ctx's stream, then scans,
 * record layout and assembly on an internal stream, over one of two scratch sets.  Off: the ctx's stream waits for the
 * records before anything enqueued later - plain stream order.  On: it does not, so the next batch's reduce kernel
 * overlaps this batch's second stage (small latency-bound kernels that leave most of the GPU idle); a consumer of out /
 * rec_offsets / md orders itself behind the most recent batch with rc_ctx_wait_results(ctx, its_stream) (NULL = the ctx's
 * stream), or calls rc_ctx_sync.  The caller must not reuse a batch's output buffers before that: consecutive batches need their own
 * out / rec_offsets / md (two sets, alternating, are enough - batch i + 2 is ordered behind batch i; at reduction level 2 the second
 * stages of batches i and i + 1 really do run at the same time).  Batches complete in the order they were enqueued.
 * No counterpart in the reference (one frame at a time on one core, recode_writer.py:383-399). */
int rc_ctx_set_pipelined(rc_ctx *ctx, int on);
int rc_ctx_wait_results(rc_ctx *ctx, void *hip_stream);

/* ---- seam 1, host streaming form: the ingest / egress side of the writer's frame loop --------------------------------
 * Replaces the body of ReCoDeWriter.run's loop and its buffered file append (pyrecode/recode_writer.py:383-399, 605-607)
 * for callers whose frames live in host memory: RC_PIPE_SLOTS batches are in flight at once, so that the host-to-device
 * copy of batch i+1, the kernels of batch i, the device-to-host copy of batch i-1's records and the caller's file append
 * of batch i-2 overlap.  A slot owns device input / output buffers and pinned metadata; the caller owns the host buffers.
 * Call order per slot: submit -> [input_done] -> result -> fetch -> fetch_wait -> submit ...
 *
 *   rc_host_alloc / rc_host_free          page-locked host memory (for frames read from a file and for fetched records)
 *   rc_host_register / rc_host_unregister pin caller memory in place (a stack that is already in RAM)
 *   rc_pipe_submit      enqueue copy-in + all kernels of one batch; returns at once.  frames_host must stay untouched until
 *                       rc_pipe_input_done (pinned / registered memory) - pageable memory also works, the copy is then
 *                       synchronous inside the HIP runtime
 *   rc_pipe_result      wait for the batch; rec_offsets[n+1], md[n][3], *total = bytes of the n records.  Returns the batch's
 *                       status (RC_ERR_RECORD_TOO_LARGE, ...)
 *   rc_pipe_fetch       start copying the records (bytes <= *total) into dst_host; rc_pipe_fetch_wait waits for it
 *   rc_ctx_set_validation  validation frames on this path (pyrecode/recode_writer.py:402-415): for every frame of a submitted batch
 *                       whose absolute id is a multiple of `gap`, the 8-connected components of the binary map inside the region
 *                       [x0, x0 + w) x [y0, y0 + h) (<= 128 x 128: the reference's central ROI) are counted on the device, from the
 *                       frame the reduce kernel has just read.  gap 0 switches it off.
 *   rc_pipe_validation  counts[n] of the slot's batch (between rc_pipe_submit and rc_pipe_fetch_wait); 0xFFFFFFFF = not a
 *                       validation frame.  dose rate = count / (w * h), as in the reference */
#define RC_PIPE_SLOTS 3
void *rc_host_alloc(uint64_t bytes);
int rc_host_free(void *p);
int rc_host_register(void *p, uint64_t bytes);
int rc_host_unregister(void *p);
int rc_pipe_submit(rc_ctx *ctx, uint32_t slot, const void *frames_host, uint32_t n, uint32_t first_frame_id);
int rc_pipe_input_done(rc_ctx *ctx, uint32_t slot);
int rc_pipe_result(rc_ctx *ctx, uint32_t slot, uint64_t *rec_offsets, uint32_t *md, uint64_t *total);
int rc_pipe_fetch(rc_ctx *ctx, uint32_t slot, uint8_t *dst_host, uint64_t bytes);
int rc_pipe_fetch_wait(rc_ctx *ctx, uint32_t slot);
int rc_ctx_set_validation(rc_ctx *ctx, uint32_t gap, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h);
int rc_pipe_validation(rc_ctx *ctx, uint32_t slot, uint32_t *counts);

/* zstd, modelled encoder (compression_level >= 1): the ctx fits its entropy tables to a sample of the FIRST batch it sees and
 * keeps them (every frame carries the tables it was coded with, so any model is valid for any data - only the ratio suffers when
 * the data drifts away from the sample).  rc_ctx_refit_model makes the NEXT batch the sample again (one synchronous step), e.g.
 * after a change of dose or detector mode; a no-op for other schemes.  No counterpart in the reference (libzstd adapts per call). */
int rc_ctx_refit_model(rc_ctx *ctx);

/* Packed binary map (ceil(nx*ny/8) bytes, LSB-first) of frame i of the most recent batch: what the third element
 * of _reduce_compress's return value carries for validation frames (recode_writer.py:386,402-415,557). */
int rc_get_binary_map(rc_ctx *ctx, uint32_t i, uint8_t *bitmap_out);
/* The reference only consumes binary_frame for validation frames (recode_writer.py:402-415).  With a device codec the
 * raw maps are an extra HBM write; a caller that never asks for them can switch that off (default: kept).  Without a
 * device codec the raw map is part of the record and always produced. */
int rc_ctx_keep_binary_maps(rc_ctx *ctx, int on);

/* Per-stage device time of the most recent batch in milliseconds (HIP events), keyed like the reference's
 * run metrics (recode_writer.py:451,457,479,506,512,555):
 *   [0] frame_thresholding_and_counting_time + frame_binary_image_packing_time (fused reduce kernel; with LZ4 the
 *       bitmap compression is fused in here as well)
 *   [1] frame_binary_image_compression_time when the codec is a kernel of its own (zstd)   [2] per-frame scans
 *   [3] record layout + frame_pixel_intensity_packing_time + frame_pixel_intensity_compression_time (assemble kernel)
 *   [4] whole batch (frame_time * n)
 * Only filled by the synchronous entry point. */
int rc_get_stage_ms(rc_ctx *ctx, float ms[5]);

/* Stage timing of the ASYNCHRONOUS path: with profiling on, every rc_reduce_compress_batch_async brackets its stages
 * with HIP events on the ctx's stream; rc_ctx_sync folds them into running sums (same 5 slots as rc_get_stage_ms).
 * rc_ctx_set_profiling also clears the sums.  Used by bench.py to measure the dominant kernel inside the timed region.
 * on = k > 1: events around every k-th batch only, starting with the next one (a timing event is a packet of its own on the
 * stream, a few microseconds between two reduce kernels; rc_ctx_get_profile's `batches` counts the bracketed ones). */
int rc_ctx_set_profiling(rc_ctx *ctx, int on);
int rc_ctx_get_profile(rc_ctx *ctx, double sum_ms[5], uint64_t *batches);

/* ---- seam 2: compressor backend -----------------------------------------------------------------------
 * compress()/de_compress() of pyrecode/recode_compressors.py:82-120 / :40-79 for the device codecs.
 * Host or device pointers.  *out_n receives the produced byte count; rc_decompress also sets it to the required size
 * when it returns RC_ERR_OUT_TOO_SMALL (dst may then be NULL with dst_cap 0: a size query).
 * Every scheme rc_scheme_on_device() reports (LZ4, zstd, blosc-lz4) is both encoded and decoded here.  Decoding covers
 * what this library writes and the stock encoders' frames of the same kind: LZ4 frames (independent or linked blocks),
 * blosc1-LZ4 chunks; zstd frames inside the device decoder's subset, whoever wrote them (rc_zstd_dec.h: Raw, RLE and Compressed
 * blocks; raw, RLE or single-stream Huffman literals; predefined / described / repeated sequence tables; repeat-offset matches
 * behind at least one literal; 512 regenerated bytes per block with sequences, at most 1024 per Compressed block) - for a zstd
 * frame outside it (a stock encoder's 4-stream literals, real offsets) rc_decompress returns RC_ERR_UNSUPPORTED before doing any
 * work, and RC_ERR_CORRUPT where only the decoding lanes can see the departure (a sequence without literals, a block with
 * sequences of another size in mid-frame) or the frame is damaged; for both codes the caller uses the stock decoder
 * (pyrecode_amd/recode_compressors.py::de_compress does).
 * Runs on the caller's current GPU, or on `RC_DEVICE` (env) when that is set. */
int rc_compress(uint32_t scheme, uint32_t level, const uint8_t *src, uint64_t n, uint8_t *dst, uint64_t dst_cap,
                uint64_t *out_n);
int rc_decompress(uint32_t scheme, const uint8_t *src, uint64_t n, uint8_t *dst, uint64_t dst_cap, uint64_t *out_n);
uint64_t rc_compress_bound(uint32_t scheme, uint64_t n);

/* ---- seam 3: the native c_recode.Reader methods (pyrecode/pyrecode.cpp:143-150) ---------------------------
 * get_frame_sparse -> _unpack_frame_sparse (pyrecode.cpp:95-119, c_extensions/reader.h:10-68): for every set bit of
 * the bitmap in row-major order write (row, col, val) as three uint64; level 1: val = next d-bit LSB-first field
 * of pixvals; other levels: val = 1.  out must hold 3 * popcount(bitmap) uint64 (the reference sizes it
 * nx*ny*3, recode_reader.py:111-115); out_cap_triplets bounds it.  Returns nnz >= 0 or a negative rc_status.
 * out == NULL with out_cap_triplets == 0 is a counting call: returns popcount(bitmap) and writes nothing. */
int64_t rc_unpack_frame_sparse(uint32_t nx, uint32_t ny, uint32_t bit_depth, const uint8_t *bitmap,
                               const uint8_t *pixvals, uint64_t pixvals_bytes, uint64_t *out,
                               uint64_t out_cap_triplets, uint32_t reduction_level);
/* Batched form of the reader's per-frame work: n stored frames -> decompress both streams -> sparse expand, in one call
 * with no host round trip in between.  Replaces, for n frames at once, ReCoDeReader._get_frame_sparse
 * (pyrecode/recode_reader.py:379-471: de_compress on the binary-map stream and on the value stream,
 * recode_compressors.py:40-79, then c_recode get_frame_sparse, pyrecode.cpp:95-119).
 *   nx, ny, bit_depth, reduction_level (1, 2 or 3), op_mode, scheme    header fields of the file
 *   data          host or device memory: the n frames' data blobs back to back, as they lie in a merged file (per frame: the
 *                 binary-map stream, then the value stream).  Host memory is copied in while the streams' block headers are
 *                 walked (page-locked memory - rc_host_alloc - makes that copy asynchronous); device memory is decoded where it lies
 *   sizes         uint32[n][3]: bytes of the binary-map stream, bytes of the value stream, bytes of the DEcompressed value
 *                 stream (the rows of the file's metadata table; mode 0: {nb, n_packed, n_packed})
 *   nnz_prefix    uint64[n+1] out: exclusive prefix of the frames' set-pixel counts (frame i's triplets are
 *                 [nnz_prefix[i], nnz_prefix[i+1]))
 *   triplets      uint64[cap][3] out (host or device): (row, col, value) in row-major order per frame, frames in order;
 *                 may be NULL with cap 0 (a counting call)
 * Device decoders: mode 0 (stored pieces), LZ4 frames with independent blocks, zstd frames inside the subset rc_zstd_dec.h
 * describes (wider than what this library writes), and blosc1-LZ4 chunks (RC_SCHEME_BLOSC_LZ4; replaces blosc.decompress,
 * recode_compressors.py:61-76) of the shape this library writes: version 2, typesize 8, blocks of 512 bytes that are not split, bit-shuffled
 * or not shuffled, or a "memcpyed" chunk of exactly 16 + nbytes bytes (either stream; the value stream only so).  A chunk whose header's
 * nbytes / cbytes disagree with the frame, or whose block starts / sizes leave the stream or exceed a block's LZ4 bound, is RC_ERR_CORRUPT.
 * scheme RC_SCHEME_ZLIB_DEVICE (op_mode 1, reduction levels 1 and 3; rc_inflate.hip): the zlib streams of a compression_scheme-0 file that
 * this library's device DEFLATE encoder wrote - a fixed-Huffman or stored block per 512 map bytes, a literals-only dynamic-Huffman or
 * stored block per 32 KiB of values, coded blocks closed by an empty stored block.  The host does not walk them: the device finds the
 * blocks' starts itself.  Any other zlib stream (stock zlib's among them) is RC_ERR_UNSUPPORTED - from the call, or, for a stream only
 * the device can tell apart, from rc_expand_frames_wait - with nothing written to the output: use the stock decoder
 * (rc_host_decode_streams).  The Adler-32 trailers are not checked.  scheme 0 itself stays RC_ERR_UNSUPPORTED, as does rc_expand_frames_l2
 * with RC_SCHEME_ZLIB_DEVICE.
 * reduction_level 2: the binary map expands exactly as at level 3 (value 1) and the statistics stream - sizes[i][1] bytes - is stepped
 * over, as the reference's reader does (recode_reader.py:413-440: get_frame_sparse(level, map, None)); with triplets NULL this is the
 * counting call that sizes the buffers of rc_expand_frames_l2.  Anything else returns RC_ERR_UNSUPPORTED before any work is done and the caller falls back to
 * the per-frame path with the stock decoder; a stream that is inside the subset on its face but does not decode to the frame's
 * shape (a foreign encoder's larger blocks, or damage) returns RC_ERR_CORRUPT - callers that can fall back should do so for both
 * codes and let the stock decoder judge.  RC_ERR_OUT_TOO_SMALL: nnz_prefix is valid, triplets untouched.  At reduction level 1
 * sum(8 * sizes[i][2] / bit_depth) bounds the count, so one call with that capacity does (ReCoDeReader.get_frames_triplets).
 * The host walk runs on a small pool of worker threads that stays with the process. */
int rc_expand_frames(uint32_t nx, uint32_t ny, uint32_t bit_depth, uint32_t reduction_level, uint32_t op_mode, uint32_t scheme,
                     const uint8_t *data, const uint32_t *sizes, uint32_t n, uint64_t *nnz_prefix, uint64_t *triplets, uint64_t cap);
/* The same work in two halves, for a reader that streams through a file: _submit queues one batch (host walk of the block headers,
 * copy-in, decoders, count, emit) on one of two slots and returns; _wait(slot) blocks until that batch is done and reports like
 * rc_expand_frames.  With two batches in flight the host walk and copy-in of one run while the device decodes the other.
 *   slot            0 or 1; a slot holds one batch at a time (_submit on a slot with a batch waiting: RC_ERR_BAD_ARG).  The synchronous
 *                   rc_expand_frames owns resources of its own, so it may be called (e.g. to redo ONE batch) while batches are queued
 *   triplets_dev    device memory, or page-locked host memory (rc_host_alloc: staged on the device, then ONE asynchronous copy of all
 *                   cap entries - keep cap tight; contents unspecified when _wait reports an error), cap entries
 *                   (level 1: sum(8 * sizes[i][2] / bit_depth) bounds the count)
 *   data            must stay valid until _wait(slot) returns; sizes is consumed by _submit
 * Streams outside the device decoders' subset are reported by _submit (RC_ERR_UNSUPPORTED / RC_ERR_CORRUPT, nothing left pending);
 * what only the device can see (a block that does not decode to its size, cap too small) by _wait. */
int rc_expand_frames_submit(uint32_t slot, uint32_t nx, uint32_t ny, uint32_t bit_depth, uint32_t reduction_level, uint32_t op_mode,
                            uint32_t scheme, const uint8_t *data, const uint32_t *sizes, uint32_t n, uint64_t *triplets_dev, uint64_t cap);
int rc_expand_frames_wait(uint32_t slot, uint64_t *nnz_prefix);
/* The same two calls with the output laid out as what the reference's reader makes of the triplets - the three arrays of a scipy COO
 * matrix (recode_reader.py:466-469): `coo` = int32 rows[cap] | int32 columns[cap] | uint16 values[cap] (10 * cap bytes; entry i of the
 * batch at index i of each array, frame f's entries at nnz_prefix[f] .. nnz_prefix[f+1]).  10 instead of 24 bytes per set pixel cross
 * the link, and the host has nothing to split.  bit_depth <= 16.  rc_expand_frames_coo_submit is waited for with
 * rc_expand_frames_wait like a triplet batch. */
int rc_expand_frames_coo(uint32_t nx, uint32_t ny, uint32_t bit_depth, uint32_t reduction_level, uint32_t op_mode, uint32_t scheme,
                         const uint8_t *data, const uint32_t *sizes, uint32_t n, uint64_t *nnz_prefix, void *coo, uint64_t cap);
int rc_expand_frames_coo_submit(uint32_t slot, uint32_t nx, uint32_t ny, uint32_t bit_depth, uint32_t reduction_level, uint32_t op_mode,
                                uint32_t scheme, const uint8_t *data, const uint32_t *sizes, uint32_t n, void *coo_dev, uint64_t cap);
/* The COO pair for files whose values do not fit 16 bits (uint32 sources, 17..32-bit fields): the reference's reader gives the matrix the
 * data type target_bit_depth maps to (recode_reader.py:464-471 with misc.py:41-52), uint32 for such files, and so does
 * `coo` = int32 rows[cap] | int32 columns[cap] | uint32 values[cap] (12 * cap bytes, 12 instead of 24 per set pixel over the link).
 * bit_depth 1..32 at reduction level 1 (narrower files come out as the _coo values widened; above 32: RC_ERR_BAD_ARG); levels 3 and 2
 * as for rc_expand_frames_coo, value 1 in the wider array.  Everything else - arguments, host / device / page-locked outputs, status
 * codes, rc_expand_frames_wait for the _submit form - as for the _coo pair. */
int rc_expand_frames_coo32(uint32_t nx, uint32_t ny, uint32_t bit_depth, uint32_t reduction_level, uint32_t op_mode, uint32_t scheme,
                           const uint8_t *data, const uint32_t *sizes, uint32_t n, uint64_t *nnz_prefix, void *coo, uint64_t cap);
int rc_expand_frames_coo32_submit(uint32_t slot, uint32_t nx, uint32_t ny, uint32_t bit_depth, uint32_t reduction_level, uint32_t op_mode,
                                  uint32_t scheme, const uint8_t *data, const uint32_t *sizes, uint32_t n, void *coo_dev, uint64_t cap);
/* A batch of reduction-level-2 frames in full: the set pixels AND every frame's summary statistics.  Replaces, for n frames at once, the
 * level-2 branch of ReCoDeReader._get_frame_sparse (pyrecode/recode_reader.py:413-440 for the pixels, :473-481 for the statistics, whose
 * unpacker is c_extensions/reader.h:74-99 - intended semantics) and the de_compress calls in front of it (:393-411).
 *   rc            int32 rows[cap] | int32 columns[cap] (8 * cap bytes): the COO layout of rc_expand_frames_coo without the value array -
 *                 every value is 1.  Frame i's entries are [nnz_prefix[i], nnz_prefix[i+1]) of both arrays; rc_expand_frames with
 *                 reduction_level 2 and triplets NULL counts them beforehand
 *   stats         uint16[stats_cap] out: the statistics, frame after frame.  Frame i holds floor(8 * sizes[i][2] / bit_depth) of them -
 *                 the caller knows the prefix from the metadata table, so none is returned
 *   bit_depth     8..16: narrower fields leave the count ambiguous (the per-frame reader settles it by labelling) and level 2 does not exist
 *                 for wider sources - RC_ERR_UNSUPPORTED for both
 * op_mode / scheme, data, sizes, nnz_prefix, host or device pointers and the status codes as for rc_expand_frames_coo;
 * RC_ERR_OUT_TOO_SMALL (cap or stats_cap) leaves nnz_prefix valid and writes neither output.  rc_expand_frames_l2_submit queues the batch on
 * a slot like rc_expand_frames_coo_submit (rc_dev and stats_dev: device or page-locked host memory; a stats_cap that is too small is
 * reported at once, nothing left pending) and is waited for with rc_expand_frames_wait. */
int rc_expand_frames_l2(uint32_t nx, uint32_t ny, uint32_t bit_depth, uint32_t op_mode, uint32_t scheme, const uint8_t *data,
                        const uint32_t *sizes, uint32_t n, uint64_t *nnz_prefix, void *rc, uint64_t cap, uint16_t *stats, uint64_t stats_cap);
int rc_expand_frames_l2_submit(uint32_t slot, uint32_t nx, uint32_t ny, uint32_t bit_depth, uint32_t op_mode, uint32_t scheme,
                               const uint8_t *data, const uint32_t *sizes, uint32_t n, void *rc_dev, uint64_t cap, uint16_t *stats_dev,
                               uint64_t stats_cap);
/* ---- summed views: frames added up on the device --------------------------------------------------------------
 * What the reference's ReCoDeViewer (pyrecode/utils/viewer.py:40-75) and its Live View notebooks do with the frames of a window -
 * np.add(view, frame.toarray()) for each of them - without a set pixel crossing the link: a batch is decoded and counted exactly as by
 * rc_expand_frames, and in place of the emit kernel one kernel adds every frame's values to an accumulator in device memory (level 1: the
 * pixel's bit_depth-bit value; levels 2 and 3: 1 per set pixel, a level-2 frame's statistics stream stepped over).
 * The accumulator is an object the caller owns - one uint32 cell per pixel, row-major, ny * nx cells, zeroed, on the caller's current GPU
 * (or RC_DEVICE) - so that several readers, the part files of one run, add into one view.  ONE thread uses a handle at a time.
 *   rc_sum_create            NULL with *status set on failure (RC_ERR_DEVICE without a GPU, like every compute entry point)
 *   rc_sum_add_frames        the synchronous add; bit_depth .. sizes, n, nnz_prefix and the device decoders' subset as for rc_expand_frames
 *                            (nx, ny are the handle's; nnz_prefix may be NULL).  Has resources of its own, like rc_expand_frames
 *   rc_sum_add_frames_submit the same batch queued on slot 0 or 1; rc_expand_frames_wait(slot, nnz_prefix) gives its verdict and the counts.
 *                            Batches on both slots may add into one handle: their decode stages overlap, their sum kernels are ordered
 *   rc_sum_fetch             waits for every add queued so far, then copies the ny * nx cells to dst (host or device memory); reset != 0
 *                            also zeroes the cells and the bound
 *   rc_sum_bound             the largest value any cell can hold so far: the sum over the accepted adds of n * (2^bit_depth - 1) at level 1
 *                            and of n at levels 2 and 3 (a queued batch the device rejects later still counts: an upper bound)
 *   rc_sum_destroy           waits for queued adds, frees the cells
 * A batch the device rejects - RC_ERR_CORRUPT, RC_ERR_UNSUPPORTED, a value stream shorter than its set pixels need (RC_ERR_CORRUPT) - adds
 * NOTHING to the cells; the call, or rc_expand_frames_wait, says which.  No silent wrap: an add that could take a cell past 2^32 - 1
 * (rc_sum_bound() + this batch's share) is refused with RC_ERR_OUT_TOO_SMALL before anything is queued - fetch with reset, fold into a wider
 * image on the host, go on.  RC_ERR_UNSUPPORTED: level 1 with bit_depth > 16 (64-bit cells are not offered), and what rc_expand_frames
 * refuses.  RC_ERR_BAD_ARG: stored frames (op_mode 0) whose binary map is not ceil(nx * ny / 8) bytes - another geometry than the handle's -,
 * a handle of another device. */
typedef struct rc_sum rc_sum;
rc_sum *rc_sum_create(uint32_t nx, uint32_t ny, int *status);
int rc_sum_destroy(rc_sum *s);
int rc_sum_add_frames(rc_sum *s, uint32_t bit_depth, uint32_t reduction_level, uint32_t op_mode, uint32_t scheme, const uint8_t *data,
                      const uint32_t *sizes, uint32_t n, uint64_t *nnz_prefix);
int rc_sum_add_frames_submit(rc_sum *s, uint32_t slot, uint32_t bit_depth, uint32_t reduction_level, uint32_t op_mode, uint32_t scheme,
                             const uint8_t *data, const uint32_t *sizes, uint32_t n);
int rc_sum_fetch(rc_sum *s, uint32_t *dst, int reset);
uint64_t rc_sum_bound(const rc_sum *s);
/* ---- electron counting: one event per connected component ----------------------------------------------------
 * What l1_to_l4_converter (pyrecode/utils/converters.py:59-123) does with the frames of a level-1 file one at a time on the host -
 * scipy.ndimage.label with the 3 x 3 structure (:75, :88), then a centroid per label (_get_centroids_2d_nb_w :167-197, _nb_u :200-226,
 * _nb_m :229-259) - for n frames in one device call: a batch is decoded and counted exactly as by rc_expand_frames, and in place of the
 * emit kernel the kernels of rc_count.hip label the set pixels (8-connected, within a frame, no wrap from a row's last column to the next
 * row's first) and reduce every component.  With v a pixel's stored value (level 1: the bit_depth-bit field; levels 2 and 3: 1, a
 * level-2 frame's statistics stream stepped over): area = pixels, weight = sum v, Sr = sum v * row, Sc = sum v * col - exact integers.
 *   method          0 weighted average: row = rhe(Sr / weight), col = rhe(Sc / weight), rhe = nearest integer of the exact rational, ties
 *                     to the even one (np.round, :92); a component of weight 0 is placed as by method 1
 *                   1 unweighted average: the same with v = 1 for the position (weight stays sum v)
 *                   2 maximum: the pixel with the largest v, the first in raster order among equals (:243, a strict >)
 *   area_threshold  an event is kept iff area > area_threshold (:195, :224, :257: a strict >)
 *   nev_prefix      uint64[n+1] out (host): frame i's events are [nev_prefix[i], nev_prefix[i+1]), ordered by the raster position of
 *                   their component's first pixel (scipy's label order); two events of a frame on one pixel are both kept
 *   events          uint64 weight[cap] | int32 rows[cap] | int32 cols[cap] | uint32 area[cap] (20 * cap bytes; host or device), or NULL
 *                   with cap 0: the counting call.  Events <= set pixels bounds cap
 * Unlike the reference: the sums are exact (it accumulates in float32), positions are (row, col) (it hands (col, row) to coo_matrix as
 * (row, col), :100-101), every method is what its helper computes (it sends all three names to the weighted one, :157-164).
 * nx, ny <= 65535; op_mode / scheme / data / sizes and the device decoders' subset as for rc_expand_frames.  RC_ERR_OUT_TOO_SMALL:
 * nev_prefix is valid, no byte of events written.  RC_ERR_CORRUPT: a value stream shorter than its set pixels need (or a stream that does
 * not decode); nothing written.  RC_ERR_UNSUPPORTED: level 1 with bit_depth > 16, 2^32 set pixels or more in one call, and what
 * rc_expand_frames refuses.  RC_ERR_BAD_ARG: method > 2, NULL / zero arguments.  RC_ERR_DEVICE: no GPU.
 * rc_count_frames_submit queues the batch on slot 0 or 1 (events_dev: device or page-locked host memory, which is filled only once the
 * batch is known to be good); rc_expand_frames_wait(slot, nev_prefix) gives its verdict and the prefix.  At levels 2 and 3 the set
 * pixels are not bounded by the streams' sizes: both forms wait for their count before the workspace is sized. */
int rc_count_frames(uint32_t nx, uint32_t ny, uint32_t bit_depth, uint32_t reduction_level, uint32_t op_mode, uint32_t scheme,
                    const uint8_t *data, const uint32_t *sizes, uint32_t n, uint32_t method, uint32_t area_threshold,
                    uint64_t *nev_prefix, void *events, uint64_t cap);
int rc_count_frames_submit(uint32_t slot, uint32_t nx, uint32_t ny, uint32_t bit_depth, uint32_t reduction_level, uint32_t op_mode,
                           uint32_t scheme, const uint8_t *data, const uint32_t *sizes, uint32_t n, uint32_t method,
                           uint32_t area_threshold, void *events_dev, uint64_t cap);
/* ---- counted views: events summed on the device, with sub-pixel placement ---------------------------------------
 * The two above together: what a caller of l1_to_l4_converter (pyrecode/utils/converters.py:59-123) who wants the counted IMAGE of a dose
 * fraction does next - add the frames' events up, as the viewer adds frames (np.add at pyrecode/utils/viewer.py:65-68) - without an event
 * crossing the link: the batch is decoded, labelled and reduced exactly as by rc_count_frames (method, area_threshold as there), and in the
 * place of the event arrays every kept component adds ONE count to a cell of an rc_sum handle.
 *   upsample  1..16: the view's grid is `upsample` times finer than the frame's, the handle is (upsample * nx) x (upsample * ny) cells.
 *             Pixel centres lie at integers, fine cell k of an axis has its centre at (k - (upsample - 1) / 2) / upsample; the count goes
 *             to the cell whose centre is nearest to the exact centroid S / w: k = (2 s S + (s - 1) w) / (2 w) rounded to the nearest
 *             integer, ties to the even one - integer arithmetic, nothing rounded before.  upsample 1 is rc_count_frames' (row, col).
 *             Method 2 places the winning pixel's centre.  A component of weight 0 is placed by its unweighted sums.
 *   nx, ny    the FRAME's shape
 *   nev_prefix  uint64[n+1] out (host), may be NULL: the frames' EVENT prefix, as rc_count_frames gives it
 * Everything that holds for rc_sum_add_frames holds here: the cells are the caller's handle; the same handle takes plain and counted adds;
 * batches on both slots may add into one handle; rc_expand_frames_wait(slot, nev_prefix) gives a submitted batch's verdict and the event
 * prefix; a batch the device rejects adds NOTHING.  At levels 2 and 3 both forms wait for the set-pixel count before the workspace is sized.
 * No silent wrap: a batch grows rc_sum_bound() by the sum over its frames of
 *     min(ceil(nx / 2) * ceil(ny / 2), floor(8 * sizes[3 f + 2] / bit_depth))       (levels 2 and 3: the first term alone)
 * - the components a frame can hold (an aligned 2 x 2 block of pixels belongs to at most one of them) and the set pixels its value stream
 * has room for; every component is one count and all of them could share a cell - and an add that could take a cell past 2^32 - 1 is refused
 * with RC_ERR_OUT_TOO_SMALL before anything is queued.
 * RC_ERR_BAD_ARG: upsample outside 1..16, method > 2, a slot above 1, NULL / zero arguments, nx or ny above 65535, a handle whose shape is
 * not (upsample * nx, upsample * ny), a handle of another device.  RC_ERR_UNSUPPORTED: level 1 with bit_depth > 16, and what
 * rc_expand_frames and rc_count_frames refuse.  RC_ERR_CORRUPT: as rc_count_frames.  RC_ERR_DEVICE: no GPU. */
int rc_sum_add_counted(rc_sum *s, uint32_t nx, uint32_t ny, uint32_t upsample, uint32_t bit_depth, uint32_t reduction_level,
                       uint32_t op_mode, uint32_t scheme, const uint8_t *data, const uint32_t *sizes, uint32_t n, uint32_t method,
                       uint32_t area_threshold, uint64_t *nev_prefix);
int rc_sum_add_counted_submit(rc_sum *s, uint32_t slot, uint32_t nx, uint32_t ny, uint32_t upsample, uint32_t bit_depth,
                              uint32_t reduction_level, uint32_t op_mode, uint32_t scheme, const uint8_t *data, const uint32_t *sizes,
                              uint32_t n, uint32_t method, uint32_t area_threshold);
/* ---- aligned views: per-frame shifts applied while the device sums frames ------------------------------------
 * A dose-fractionated movie is not summed as it lies: the specimen drifts, and every frame is translated by its measured drift before it is
 * added.  The four calls below are the four adds above with one more argument:
 *   shifts  int32[2 * n] in HOST memory: dy0, dx0, dy1, dx1, ... - frame f's translation.  What the unshifted call adds to cell (r, c) of the
 *           view, the shifted call adds to (r + dy_f, c + dx_f); a contribution whose target lies outside the view is DROPPED - not wrapped,
 *           not clamped, not an error.  Any int32 pair is legal (the cell is computed in 64 bits); a frame shifted wholly out adds nothing.
 *           The array is copied before the call returns, the _submit forms included.  NULL: RC_ERR_BAD_ARG.
 * Plain sums: cells are sensor pixels, shifts whole pixels (fractional shifts of plain sums are not offered: the cells would stop being
 * exact integers).  Counted sums: cells are the fine grid's and shifts are in FINE cells (1 / upsample pixel) - the event is placed as by
 * rc_sum_add_counted and then translated, which makes an integer shift a drift correction at 1 / upsample-pixel resolution.
 * Unchanged by shifts: nnz_prefix / nev_prefix (the decoded set pixels or kept events per frame, placed or not), the growth of
 * rc_sum_bound() (dropping only lowers a sum), every refusal and status code of the unshifted calls, and "a rejected batch adds NOTHING".
 * All-zero shifts give, cell for cell, what the unshifted call gives; one handle takes shifted and unshifted adds. */
int rc_sum_add_frames_shifted(rc_sum *s, uint32_t bit_depth, uint32_t reduction_level, uint32_t op_mode, uint32_t scheme, const uint8_t *data,
                              const uint32_t *sizes, uint32_t n, const int32_t *shifts, uint64_t *nnz_prefix);
int rc_sum_add_frames_shifted_submit(rc_sum *s, uint32_t slot, uint32_t bit_depth, uint32_t reduction_level, uint32_t op_mode, uint32_t scheme,
                                     const uint8_t *data, const uint32_t *sizes, uint32_t n, const int32_t *shifts);
int rc_sum_add_counted_shifted(rc_sum *s, uint32_t nx, uint32_t ny, uint32_t upsample, uint32_t bit_depth, uint32_t reduction_level,
                               uint32_t op_mode, uint32_t scheme, const uint8_t *data, const uint32_t *sizes, uint32_t n, uint32_t method,
                               uint32_t area_threshold, const int32_t *shifts, uint64_t *nev_prefix);
int rc_sum_add_counted_shifted_submit(rc_sum *s, uint32_t slot, uint32_t nx, uint32_t ny, uint32_t upsample, uint32_t bit_depth,
                                      uint32_t reduction_level, uint32_t op_mode, uint32_t scheme, const uint8_t *data, const uint32_t *sizes,
                                      uint32_t n, uint32_t method, uint32_t area_threshold, const int32_t *shifts);
/* ---- dense frame batches: a region of every frame as an array, written on the device ----------------------------
 * What ReCoDeReader.get_sub_volume would return in the reference, where it is a stub (pyrecode/recode_reader.py:185-186), and what its
 * callers do instead with every frame on the host - frame.toarray(), a memset and a scatter (pyrecode/utils/viewer.py:65-68): a batch is
 * decoded and counted exactly as by rc_expand_frames, and in place of the emit kernel one kernel (k_expand_dense_b) writes
 *   out[f][j][i] = the value of source pixel (y0 + j * step_y, x0 + i * step_x) of frame f,   f < n, j < h, i < w,
 * row-major, frames back to back, cells of cell_bytes bytes.  Level 1: a set pixel's bit_depth-bit field; levels 2 and 3: 1 (a level-2
 * frame's statistics stream is stepped over); an unset pixel: 0.  EVERY cell is written exactly once, zeros included: out needs no
 * memset and what it held does not matter.  Levels 2 and 3 need no counting call first.
 *   x0, y0, w, h, step_x, step_y  the region; w and h are the OUTPUT's size.  RC_ERR_BAD_ARG: a step, w or h of 0,
 *                 x0 + (w - 1) * step_x >= nx, y0 + (h - 1) * step_y >= ny, nx or ny above 65535
 *   cell_bytes    1, 2 or 4 (unsigned cells); at level 1 bit_depth > 8 * cell_bytes is RC_ERR_BAD_ARG, bit_depth > 32 RC_ERR_UNSUPPORTED
 *   out           cell_bytes-aligned (no more: frames of 3 x 21 uint16 cells are 126 bytes each), device or host memory: device memory is
 *                 written by the kernel itself, host memory is staged on the device and copied once the batch is known to be good
 *   out_cells     cells out has room for; fewer than n * w * h is RC_ERR_OUT_TOO_SMALL
 *   nnz_prefix    uint64[n+1] out (host), may be NULL: the frames' set-pixel prefix over the WHOLE frames, not the region - what
 *                 rc_expand_frames gives, to cross-check against the COO route
 * All of the above are known from the arguments alone and reported before any device work, in both forms.
 * op_mode / scheme, data (host or device), sizes and the device decoders' subset as for rc_expand_frames.  A batch that is refused - a
 * decoder's RC_ERR_CORRUPT or RC_ERR_UNSUPPORTED, a level-1 value stream shorter than its set pixels need (RC_ERR_CORRUPT) - writes NOTHING
 * to out.  RC_ERR_DEVICE: no GPU.
 * rc_expand_frames_dense_submit queues the batch on slot 0 or 1 (out: device memory, or page-locked host memory, which gets ONE
 * asynchronous copy from the staged cells after the verdict, like rc_count_frames_submit's events; anything else is RC_ERR_BAD_ARG);
 * rc_expand_frames_wait(slot, nnz_prefix) gives its verdict and the prefix. */
int rc_expand_frames_dense(uint32_t nx, uint32_t ny, uint32_t bit_depth, uint32_t reduction_level, uint32_t op_mode, uint32_t scheme,
                           const uint8_t *data, const uint32_t *sizes, uint32_t n, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
                           uint32_t step_x, uint32_t step_y, uint32_t cell_bytes, void *out, uint64_t out_cells, uint64_t *nnz_prefix);
int rc_expand_frames_dense_submit(uint32_t slot, uint32_t nx, uint32_t ny, uint32_t bit_depth, uint32_t reduction_level, uint32_t op_mode,
                                  uint32_t scheme, const uint8_t *data, const uint32_t *sizes, uint32_t n, uint32_t x0, uint32_t y0,
                                  uint32_t w, uint32_t h, uint32_t step_x, uint32_t step_y, uint32_t cell_bytes, void *out,
                                  uint64_t out_cells);
/* ---- frame traces: a few exact integers per frame, reduced on the device -----------------------------------------
 * What a time-resolved or scanned acquisition is first looked at with, and what the reference computes on the host: the dose rate its
 * l1_to_l4_converter prints per frame (pyrecode/utils/converters.py:108-111: the frame's set pixels over its area), and everything
 * else per frame - total intensity, centre of mass, the sum under a mask - by a caller's loop around ReCoDeReader.get_frame
 * (pyrecode/recode_reader.py:379-471) and numpy.  A batch is decoded and counted exactly as by rc_expand_frames, and in place of the
 * emit kernel the kernels of rc_trace.hip write, for frame f and its set pixels (row, col) of stored value v (level 1: the
 * bit_depth-bit field; levels 2 and 3: 1, a level-2 frame's statistics stream is stepped over),
 *   out[f][0] = the number of set pixels      out[f][2] = sum v * row
 *   out[f][1] = sum v                          out[f][3] = sum v * col        out[f][4 + m] = sum v * W_m[row][col],  m < k
 * int64[n][4 + k], row-major, exact.  A frame without a set pixel gives a row of zeros; EVERY cell is written exactly once: out needs
 * no memset.
 *   rc_trace_create   nx, ny: the frames' shape, 1..65535; k <= 16 planes of int32[ny][nx] in C order, host or device memory (NULL
 *                     when k == 0), copied into the handle in the layout its kernel reads (pixel-major) - the caller's may go away.
 *                     Device planes are read on the library's own stream, which is NOT ordered behind the caller's: they lie on the
 *                     handle's GPU and whatever writes them has finished (hipStreamSynchronize / hipDeviceSynchronize) before the call.
 *                     NULL with *status set on failure: RC_ERR_BAD_ARG (k > 16, a shape of 0 or above 65535, planes NULL with k > 0),
 *                     RC_ERR_DEVICE without a GPU.  The handle lives on the caller's current GPU (RC_DEVICE); its weights are read-only
 *                     after create, so batches on both slots may use one handle.  One thread uses a handle at a time.
 *   rc_trace_columns       4 + k
 *   rc_trace_weight_bound  max |W_m| as uint32 (INT32_MIN counts as 2^31); 0 for m >= k
 * No silent wrap: with a = the largest weight of any column (1, ny - 1, nx - 1, the planes' bounds), vmax = 2^bit_depth - 1 at level 1
 * and 1 otherwise, and P_f = the set pixels frame f can hold (nx * ny; at level 1 no more than floor(8 * sizes[3 f + 2] / bit_depth)),
 * a batch with a * vmax * P_f > 2^63 - 1 for any frame is refused with RC_ERR_OUT_TOO_SMALL before any device work.
 *   out           int64-aligned, device or host memory: device memory is written by the kernel itself, host memory is staged on the
 *                 device and copied once the batch is known to be good
 *   out_cells     cells out has room for; fewer than n * (4 + k) is RC_ERR_OUT_TOO_SMALL
 *   nnz_prefix    uint64[n+1] out (host), may be NULL: what rc_expand_frames gives
 * Level 1 with bit_depth > 16 is RC_ERR_UNSUPPORTED, as for the summed views; stored frames (op_mode 0) whose binary map is not
 * ceil(nx * ny / 8) bytes, and a handle of another device, are RC_ERR_BAD_ARG.  Everything known from the arguments alone is reported
 * before any device work, in both forms.  op_mode / scheme, data (host or device), sizes and the device decoders' subset as for
 * rc_expand_frames.  A batch that is refused - the no-wrap rule, a decoder's RC_ERR_CORRUPT or RC_ERR_UNSUPPORTED, a level-1 value stream
 * shorter than its set pixels need (RC_ERR_CORRUPT) - writes NOTHING to out.
 * rc_trace_frames_submit queues the batch on slot 0 or 1 (out: device memory, or page-locked host memory, which gets ONE asynchronous
 * copy after the verdict; anything else is RC_ERR_BAD_ARG); rc_expand_frames_wait(slot, nnz_prefix) gives its verdict and the prefix. */
typedef struct rc_trace rc_trace;
rc_trace *rc_trace_create(uint32_t nx, uint32_t ny, uint32_t k, const int32_t *planes, int *status);
int rc_trace_destroy(rc_trace *t);
uint32_t rc_trace_columns(const rc_trace *t);
uint32_t rc_trace_weight_bound(const rc_trace *t, uint32_t m);
int rc_trace_frames(rc_trace *t, uint32_t bit_depth, uint32_t reduction_level, uint32_t op_mode, uint32_t scheme, const uint8_t *data,
                    const uint32_t *sizes, uint32_t n, int64_t *out, uint64_t out_cells, uint64_t *nnz_prefix);
int rc_trace_frames_submit(rc_trace *t, uint32_t slot, uint32_t bit_depth, uint32_t reduction_level, uint32_t op_mode, uint32_t scheme,
                           const uint8_t *data, const uint32_t *sizes, uint32_t n, int64_t *out, uint64_t out_cells);
/* ---- correlation surfaces: per frame the overlap with a reference image over a window of offsets -----------------------------
 * What drift estimation needs of every frame, and what a caller otherwise computes with a whole-frame FFT per fraction around
 * ReCoDeReader.get_frame (pyrecode/recode_reader.py:379-471).  A batch is decoded and counted exactly as by rc_expand_frames, and in
 * place of the emit kernel the kernels of rc_corr.hip write, for frame f and its set pixels (row, col) of stored value v (level 1: the
 * bit_depth-bit field; levels 2 and 3: 1), with S = 2 * radius + 1 and T the handle's reference (0 outside the image),
 *   out[f][dy + R][dx + R] = sum v * T[row + dy][col + dx],   -R <= dy, dx <= R
 * int64[n][S][S], row-major, exact: the overlap with T of frame f translated by (dy, dx) - the sign convention of the shifted adds
 * (rc_sum_add_frames_shifted), so the argmax is the (dy, dx) to pass there.  The centre cell is rc_trace_frames' column under the
 * plane T; the surface of a smaller radius is the centre crop of a larger one's.  A frame without a set pixel gives zeros; EVERY cell
 * is written exactly once: out needs no memset.
 *   rc_corr_create  nx, ny: the frames' shape, 1..65535; radius 0..16; reference: int32[ny][nx] in C order, host or device memory,
 *                   copied into the handle with a border of `radius` zeros - the caller's may go away.  A device reference is read on the
 *                   library's own stream: the ordering rule of rc_trace_create's planes.  NULL with *status set on failure:
 *                   RC_ERR_BAD_ARG (radius > 16, a shape of 0 or above 65535, reference NULL), RC_ERR_DEVICE without a GPU.  The handle
 *                   lives on the caller's current GPU (RC_DEVICE) and is read-only after create, so batches on both slots may use one
 *                   handle.  One thread uses a handle at a time.
 *   rc_corr_side             2 * radius + 1
 *   rc_corr_reference_bound  max |T| as uint32 (INT32_MIN counts as 2^31)
 * No silent wrap, by the rule of the traces with max |T| as the one weight: a batch with max |T| * vmax * P_f > 2^63 - 1 for any frame
 * is refused with RC_ERR_OUT_TOO_SMALL before any device work.  out, nnz_prefix, the refusals (out_cells < n * S * S is
 * RC_ERR_OUT_TOO_SMALL), their order before any device work, and "a refused batch writes NOTHING to out" are rc_trace_frames';
 * rc_corr_frames_submit queues the batch on slot 0 or 1 as rc_trace_frames_submit does, rc_expand_frames_wait gives the verdict. */
typedef struct rc_corr rc_corr;
rc_corr *rc_corr_create(uint32_t nx, uint32_t ny, uint32_t radius, const int32_t *reference, int *status);
int rc_corr_destroy(rc_corr *c);
uint32_t rc_corr_side(const rc_corr *c);
uint32_t rc_corr_reference_bound(const rc_corr *c);
int rc_corr_frames(rc_corr *c, uint32_t bit_depth, uint32_t reduction_level, uint32_t op_mode, uint32_t scheme, const uint8_t *data,
                   const uint32_t *sizes, uint32_t n, int64_t *out, uint64_t out_cells, uint64_t *nnz_prefix);
int rc_corr_frames_submit(rc_corr *c, uint32_t slot, uint32_t bit_depth, uint32_t reduction_level, uint32_t op_mode, uint32_t scheme,
                          const uint8_t *data, const uint32_t *sizes, uint32_t n, int64_t *out, uint64_t out_cells);
/* ---- binned frame traces: per frame and bin of a label map the set pixels and the sum of their values ---------------------------
 * The per-frame reduction of diffraction and 4D-STEM data that is a PARTITION - radial profiles, annular and segmented detectors, ROI
 * grids -, which a caller otherwise computes with np.bincount over labels[rows, cols] around ReCoDeReader.get_frame
 * (pyrecode/recode_reader.py:379-471).  A batch is decoded and counted exactly as by rc_expand_frames, and in place of the emit kernel the
 * kernels of rc_bins.hip write, for frame f and its set pixels (row, col) of stored value v (level 1: the bit_depth-bit field; levels 2
 * and 3: 1; a level-2 file's statistics stream is stepped over),
 *   out[f][0][b] = the number of set pixels with labels[row][col] == b,   out[f][1][b] = the sum of their v,   0 <= b < n_bins
 * int64[n][2][n_bins], row-major, exact.  Summed over b, plane 0 plus the ignored pixels is rc_trace_frames' count and plane 1 its sum;
 * for n_bins <= 16 plane 1 is its weighted columns under the one-hot planes labels == b.  A frame without a set pixel gives zeros; EVERY
 * cell is written exactly once: out needs no memset.
 *   rc_bins_create  nx, ny: the frames' shape, 1..65535; n_bins 1..4096; labels: uint16[ny][nx] in C order, host or device memory, each
 *                   cell a bin 0 .. n_bins - 1 or 0xFFFF ("in no bin"), copied into the handle - the caller's may go away.  Device
 *                   labels are read on the library's own stream: the ordering rule of rc_trace_create's planes.  NULL with *status set
 *                   on failure: RC_ERR_BAD_ARG (a shape of 0 or above 65535, n_bins 0 or above 4096, labels NULL, a label >= n_bins
 *                   that is not 0xFFFF - host labels are scanned on the host, all of this before the device is asked for; device labels
 *                   by a small kernel), RC_ERR_DEVICE without a GPU.  The handle lives on the caller's current GPU (RC_DEVICE) and is
 *                   read-only after create, so batches on both slots may use one handle.  One thread uses a handle at a time.
 *   rc_bins_count   n_bins
 * No batch is refused for wrap: a cell is at most 65535 * nx * ny < 2^48.  out, nnz_prefix, the refusals (out_cells < n * 2 * n_bins is
 * RC_ERR_OUT_TOO_SMALL; level 1 above 16 bits RC_ERR_UNSUPPORTED; a stored frame of another geometry or a handle of another device
 * RC_ERR_BAD_ARG), their order before any device work, and "a refused batch writes NOTHING to out" are rc_trace_frames';
 * rc_bins_frames_submit queues the batch on slot 0 or 1 as rc_trace_frames_submit does, rc_expand_frames_wait gives the verdict. */
typedef struct rc_bins rc_bins;
rc_bins *rc_bins_create(uint32_t nx, uint32_t ny, uint32_t n_bins, const uint16_t *labels, int *status);
int rc_bins_destroy(rc_bins *b);
uint32_t rc_bins_count(const rc_bins *b);
int rc_bins_frames(rc_bins *b, uint32_t bit_depth, uint32_t reduction_level, uint32_t op_mode, uint32_t scheme, const uint8_t *data,
                   const uint32_t *sizes, uint32_t n, int64_t *out, uint64_t out_cells, uint64_t *nnz_prefix);
int rc_bins_frames_submit(rc_bins *b, uint32_t slot, uint32_t bit_depth, uint32_t reduction_level, uint32_t op_mode, uint32_t scheme,
                          const uint8_t *data, const uint32_t *sizes, uint32_t n, int64_t *out, uint64_t out_cells);
/* The host half of a batch whose streams only a STOCK decoder takes - files the reference's writer produced with zstandard /
 * lz4.frame / zlib (recode_compressors.py:82-120): linked 64 KiB LZ4 blocks, 4-stream Huffman literals and real offsets in zstd,
 * deflate.  Each is one serial chain, which the reference walks with one library call per stream (recode_compressors.py:40-79:
 * zlib.decompress :43, zstd :46, lz4.frame.decompress :49).  rc_host_decode_streams makes the SAME library's call (libzstd.so.1 /
 * liblz4.so.1 / libz.so.1, bound at run time) for n streams at once on worker threads: stream i is src[spans[4i] .. + spans[4i+1])
 * and must decode to exactly spans[4i+3] bytes at dst + spans[4i+2] (host pointers; dst is typically the page-locked stored-pieces
 * image that rc_expand_frames / _submit then takes with op_mode 0).  threads 0 = min(16, cores).  Schemes 1 (zstd), 2 (LZ4), 0 (zlib).
 * RC_ERR_UNSUPPORTED: no such library on this host (rc_host_decoder_available says so beforehand);
 * RC_ERR_CORRUPT: the stock decoder rejected a stream or it decodes to another size.  No GPU is touched. */
int rc_host_decoder_available(uint32_t scheme);     /* 1 / 0 */
int rc_host_decode_streams(uint32_t scheme, const uint8_t *src, uint8_t *dst, const uint64_t *spans, uint32_t n, uint32_t threads);
/* The last step of the reference's get_frame (recode_reader.py:466-469: coo_matrix((data, (row, col)))) for a frame's triplets: its
 * uint64 (row, col, value) rows -> int32 rows, int32 columns and values as unsigned integers of val_bytes (1 / 2 / 4 / 8) bytes, in ONE
 * pass.  Host pointers; no GPU is touched. */
int rc_split_triplets(const uint64_t *triplets, uint64_t n, int32_t *row, int32_t *col, void *val, uint32_t val_bytes);
/* bit_pack_pixel_intensities -> _bit_pack_pixel_intensities (reader.h:105-140) with the intended semantics of
 * the numba _bit_pack (recode_writer.py:637-652): zero, then LSB-first d-bit fields.  out_n = ceil(n*d/8). */
int rc_bit_pack(const uint16_t *pixvals, uint64_t n, uint32_t bit_depth, uint8_t *out, uint64_t out_n);
/* bit_unpack_pixel_intensities -> intended semantics of reader.h:74-99: n d-bit fields -> uint64[n]. */
int rc_bit_unpack(const uint8_t *packed, uint64_t packed_bytes, uint64_t n, uint32_t bit_depth, uint64_t *out);

/* ---- calibration: from a flat-field acquisition to threshold frames --------------------------------------------
 * The per-pixel and per-value loops of pyrecode/utils/calibration.py::make_calibration_frames (:87-138); the Gaussian fit, the thresholds
 * floor(median + sigma * i) and the files stay on the host (pyrecode_amd/utils/calibration.py), the event counts per threshold
 * (_count_events, :19-23) are a reduction-level-2 ctx in reduce-only mode.  Stateless, on the caller's current GPU (or RC_DEVICE);
 * every pointer may be host or device memory.  stack: uint16[n][n_pixels] in C order, 1 <= n <= 65535 (RC_ERR_BAD_ARG beyond: the
 * exact-integer variance n * S2 - S1^2 fits 64 bits up to there); sizes are checked before any device work.
 *
 * rc_calib_stats replaces _median_std_nb (:48-57):
 *   median    float32[n_pixels] out: np.median of every pixel's n values, bit-exact (odd n: the middle value, even n: the mean of the two
 *             middle values - a multiple of 0.5 below 2^17)
 *   std_out   float32[n_pixels] out: np.std (population) as sqrt(n * S2 - S1^2) / n from exact integer sums, one square root in double
 *             precision - within one float32 ulp of numpy's two-pass float64 result
 *   range2    int32[2] out: minimum and maximum of 2 * frame - 2 * median over the LAST n_stats frames (n_stats <= n), i.e. twice the
 *             range of what _get_fit_params (:64-71) histograms; {INT32_MAX, INT32_MIN} when n_stats is 0
 * One read of the stack from HBM while a pixel's column fits LDS (n <= rc_calib_lds_max_frames()); longer columns are read about 17
 * times from global memory by the same per-column code (pyrecode_amd/csrc/rc_calib.h). */
int rc_calib_stats(const uint16_t *stack, uint32_t n, uint64_t n_pixels, uint32_t n_stats, float *median, float *std_out, int32_t *range2);
uint32_t rc_calib_lds_max_frames(void);          /* no GPU needed */
/* np.histogram(frames - median, bins=edges) of _get_fit_params (:71): frames uint16[n_stats][n_pixels] (the frames themselves - for the
 * reference's choice, the address of frame n - n_stats of the stack), edges double[n_bins + 1] ascending (np.histogram_bin_edges on the
 * host), counts uint64[n_bins] out.  A value x = double(frame) - double(median) counts for the bin with edges[i] <= x < edges[i + 1], the
 * last bin closed on the right; values outside the edges count nowhere.  1 <= n_bins <= 1024, 1 <= n_stats <= 65535. */
int rc_calib_histogram(const uint16_t *frames, uint32_t n_stats, uint64_t n_pixels, const float *median, const double *edges,
                       uint32_t n_bins, uint64_t *counts);
/* _get_pixel_thresh_2 (:26-45), the "accurate" per-pixel thresholds: acc float32[n_pixels] out = the mean of the (k + 1)-th and the k-th
 * largest of the pixel's values that exceed median[pixel]; k = expected_n_events >= 1.  Where fewer than k + 1 values exceed the median
 * the reference's result is np.finfo(float32).min cast to an integer - undefined; here such a pixel gets 65535, the source type's
 * maximum, so that it never fires, and *n_undefined (uint64 out) counts those pixels. */
int rc_calib_top_thresholds(const uint16_t *stack, uint32_t n, uint64_t n_pixels, const float *median, uint32_t k, float *acc,
                            uint64_t *n_undefined);

/* ---- synthetic stacks for tests / bench --------------------------------------------------
 * Counter-based integer generator, identical on host (pyrecode_amd/synth.py) and device:
 * dark in [80,120]; Bernoulli(sparsity_ppm / 1e6) events of amplitude [1,2047] above dark; background <= dark. */
int rc_synth_dark(int device_id, uint32_t seed, uint64_t n_pixels, uint16_t *dark_dev);
int rc_synth_frames(int device_id, uint32_t seed, uint32_t first_frame, uint32_t n_frames, uint64_t n_pixels,
                    uint32_t sparsity_ppm, const uint16_t *dark_dev, uint16_t *frames_dev);
/* Detector-like variant: events come in clusters of 1..6 pixels (mean 4.1) inside a 2 x 3 window anchored at a seed pixel;
 * seed_ppm = seeds per million pixels (10 700 gives ~4.3 % set pixels: the real acquisition the reference's notebook records,
 * examples/Reading_ReCoDe_v0.1_Files.ipynb cells 7 / 17).  Same amplitudes and background as rc_synth_frames. */
int rc_synth_frames_clustered(int device_id, uint32_t seed, uint32_t first_frame, uint32_t n_frames, uint32_t nx, uint32_t ny,
                              uint32_t seed_ppm, const uint16_t *dark_dev, uint16_t *frames_dev);

#ifdef __cplusplus
}
#endif
#endif /* RECODE_HIP_H */
