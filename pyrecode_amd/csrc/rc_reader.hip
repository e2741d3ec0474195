// rc_reader.hip - the batched reader behind rc_expand_frames / rc_expand_frames_submit / _wait (include/recode_hip.h, seam 3):
// host walk of the stored frames' block headers on a small thread pool, block lists in page-locked memory, then the device
// decoders (rc_zstd_dec.hip) and the sparse expand (rc_expand.hip) - n frames, both streams, one call, no host round trip in between.
// Replaces ReCoDeReader._get_frame_sparse (pyrecode/recode_reader.py:379-471) for n frames at once.
#include "rc_host.h"
#include "rc_count.h"
#include "rc_dense.h"
#include "rc_inflate.h"
#include "rc_read_plan.h"
#include "rc_trace.h"
#include "rc_corr.h"
#include "rc_bins.h"

// ---- seam 3, batched: decode + expand n stored frames ---------------------------------------------------------------------
namespace {
// LZ4 frame of independent blocks -> block table (compressed blocks in `comp`, stored ones in `raw`); expect: bytes every
// compressed block regenerates (the last one the rest)
template <class VC, class VR>
int lz4_index_frame(const uint8_t *base, uint64_t off, uint64_t n, uint32_t frame_idx, uint32_t expect, uint64_t total_expected,
                    VC &comp, VR &raw, uint64_t *total)
{
    using namespace rc;
    const uint8_t *p = base + off;
    auto rd32 = [&](uint64_t q) { return (uint32_t)p[q] | ((uint32_t)p[q + 1] << 8) | ((uint32_t)p[q + 2] << 16) | ((uint32_t)p[q + 3] << 24); };
    if (n < 11 || rd32(0) != 0x184D2204u) return ZD_CORRUPT;
    const uint32_t flg = p[4], bd = p[5];
    if ((flg >> 6) != 1 || (flg & 2) || (bd & 0x8F)) return ZD_CORRUPT;
    if (!((flg >> 5) & 1)) return ZD_FOREIGN;                          // linked blocks: a serial chain
    const int bsum = (flg >> 4) & 1, csize = (flg >> 3) & 1, csum = (flg >> 2) & 1, dict = flg & 1;
    uint64_t q = 6 + (csize ? 8 : 0) + (dict ? 4 : 0) + 1, out = 0;
    for (;;) {
        if (q + 4 > n) return ZD_CORRUPT;
        uint32_t bs = rd32(q);
        q += 4;
        if (bs == 0) break;
        const bool stored = bs >> 31;
        bs &= 0x7FFFFFFFu;
        if (q + bs > n) return ZD_CORRUPT;
        // the walk is a chain of dependent cache misses (a header per few lines): ask for the lines a few blocks ahead, assuming
        // blocks of about this size
        if (bs < 2048) { __builtin_prefetch(p + q + 4 * (uint64_t)(bs + 4)); __builtin_prefetch(p + q + 4 * (uint64_t)(bs + 4) + 64); }
        ZdBlock b;
        memset(&b, 0, sizeof b);
        b.frame = frame_idx; b.src = off + q; b.csize = bs; b.dst = (uint32_t)out;
        if (stored) { b.type = 0; b.regen = bs; raw.push_back(b); }
        else {
            if (!expect) return ZD_FOREIGN;
            b.type = 2;
            b.regen = (uint32_t)std::min<uint64_t>(expect, total_expected - out);
            comp.push_back(b);
        }
        out += b.regen;
        if (out > total_expected) return ZD_CORRUPT;
        q += bs + (bsum ? 4 : 0);
    }
    if (csum) q += 4;
    if (q != n) return ZD_CORRUPT;
    *total = out;
    return ZD_OK;
}

// One stream of a scheme-8 frame: a blosc1 chunk (rc_blosc.hip's head has the layout) -> one entry per block in `blocks` (type 2: an LZ4
// block, 0: csize == the block's bytes, stored; seq_tables = the chunk's shuffle flag, 0 or 4), or ONE stored entry in `raw` for a
// "memcpyed" chunk.  map: the binary-map stream - the value stream is taken as a memcpyed chunk only (what this library writes and what
// c-blosc itself emits for bytes it cannot compress).  The device subset: version 2, LZ4 format, typesize 8, blocks of TILE_BM bytes, not
// split, bit-shuffled or not shuffled; anything else is ZD_FOREIGN.  Sizes that disagree with the frame, and block positions or sizes
// that leave the stream or exceed the LZ4 bound of a block, are ZD_CORRUPT: the decoding wave stages csize <= bound bytes and relies on it.
template <class V, class VR>
int blosc_index_stream(const uint8_t *base, uint64_t off, uint64_t n, uint32_t frame_idx, uint64_t total_expected, bool map, V &blocks, VR &raw)
{
    using namespace rc;
    const uint8_t *p = base + off;
    auto rd32 = [&](uint64_t q) { return (uint32_t)p[q] | ((uint32_t)p[q + 1] << 8) | ((uint32_t)p[q + 2] << 16) | ((uint32_t)p[q + 3] << 24); };
    if (n < 16) return ZD_CORRUPT;
    const uint32_t version = p[0], versionlz = p[1], flags = p[2], typesize = p[3];
    const uint32_t nbytes = rd32(4), blocksize = rd32(8), cbytes = rd32(12);
    if (version != 2) return ZD_FOREIGN;
    const bool memcpyed = flags & 0x02u;
    if (!memcpyed) {
        if (!map) return ZD_FOREIGN;
        if ((flags >> 5) != 1 || versionlz != 1 || !(flags & 0x10u) || (flags & 0x09u) || typesize != 8) return ZD_FOREIGN;   // codec, split, byte shuffle
        if (blocksize != std::min<uint64_t>((uint64_t)TILE_BM, std::max<uint32_t>(nbytes, 1u))) return ZD_FOREIGN;
    }
    if (nbytes != total_expected || cbytes != n) return ZD_CORRUPT;
    ZdBlock b;
    memset(&b, 0, sizeof b);
    b.frame = frame_idx;
    if (memcpyed) {
        if (n != 16ull + nbytes) return ZD_CORRUPT;
        b.src = off + 16; b.csize = b.regen = nbytes; b.dst = 0; b.type = 0;
        if (nbytes) raw.push_back(b);
        return ZD_OK;
    }
    const uint64_t nblocks = ((uint64_t)nbytes + TILE_BM - 1) / TILE_BM;
    if (16 + 4 * nblocks > n) return ZD_CORRUPT;
    b.seq_tables = (uint8_t)(flags & 0x04u);
    for (uint64_t t = 0; t < nblocks; ++t) {
        const uint64_t bs = rd32(16 + 4 * t);
        const uint32_t bsize = (uint32_t)std::min<uint64_t>((uint64_t)TILE_BM, nbytes - t * TILE_BM);
        if (bs < 16 + 4 * nblocks || bs + 4 > n) return ZD_CORRUPT;
        const uint64_t csize = rd32(bs);
        if (csize == 0 || csize > bsize + bsize / 255u + 16u || bs + 4 + csize > n) return ZD_CORRUPT;
        b.src = off + bs + 4; b.csize = (uint32_t)csize; b.dst = (uint32_t)(t * TILE_BM); b.regen = bsize; b.type = csize == bsize ? 0 : 2;
        blocks.push_back(b);
    }
    return ZD_OK;
}
}  // namespace

// The accumulator of the summed-view calls (rc_sum_*): a uint32 cell per pixel in device memory, owned by the caller's handle - not by the
// utility context, so several readers (the part files of a run) add into one view and a handle is freed when its owner says so.
// ev orders the adds: both streaming slots and the synchronous call may hold an add into the same cells, each on a stream of its own; an add's
// sum kernel waits for ev and records it again, rc_sum_fetch / rc_sum_destroy wait for it.  (Integer adds commute and the kernel adds with
// atomics, so the order is not needed for the sum - it is needed for "everything queued has landed" to be one event.)
struct rc_sum {
    int device = -1;
    uint32_t nx = 0, ny = 0;
    uint32_t *acc = nullptr;
    hipEvent_t ev = nullptr;
    hipStream_t stream = nullptr;      // fetch / reset
    uint64_t bound = 0;                // the largest value a cell can hold: sum over the adds of n * (2^d - 1) (level 1) or n (levels 2, 3);
                                       // a counted add: of the events its frames can hold (counted_admit)
};

// ---- one request: what an entry point asks of expand_run ---------------------------------------------------------------------------------
struct CountReq { uint32_t method, area_threshold, upsample; };
struct DenseReq { rc::DenseRegion region; uint32_t cell_bytes; };
// a per-frame table (trace, corr, bins): the handle's device plane, its parameter (weight planes k, radius R, bins B) and the cells of one
// frame's row; a dense batch names its row - w * h cells - here too, so that every kind of cells has its output's size in one place
struct TableReq { const void *plane; uint32_t param; uint64_t row_cells; };
// slot, submit: the synchronous forms = (RC_READ_SLOTS - their own resources -, false); the _submit forms = (slot, true): they return once
// everything is queued.  kind (rc_read_plan.h) says what out / cap are: entries of the kind's size (cap of them; NULL / 0: the prefix alone),
// the cells of a dense, trace, corr or bins output (the entry points have checked that cap holds them), nothing for the adds into `sum`.  stats /
// stats_cap (RK_L2 alone; otherwise a level-2 file's statistics stream is stepped over): every frame's fields as uint16.  shifts (with sum
// only): the caller's int32 (dy, dx) per frame, copied into the slot's page-locked head before anything is queued - the caller may reuse its
// array once the call has returned.  count.upsample: RK_COUNTED_SUM's grid is that many times finer than the frame (nx, ny: the FRAME's).
struct ReadFrames { uint32_t nx, ny, bit_depth, level, op_mode, scheme; const uint8_t *data; const uint32_t *sizes; uint32_t n; };   // (the ABI's order)
struct ReadRequest {
    ReadFrames in;
    uint32_t slot = RC_READ_SLOTS; bool submit = false;
    uint64_t *nnz_prefix = nullptr;
    rc::ReadKind kind = rc::RK_TRIPLETS; void *out = nullptr; uint64_t cap = 0;
    uint16_t *stats = nullptr; uint64_t stats_cap = 0;
    rc_sum *sum = nullptr; const int32_t *shifts = nullptr;
    CountReq count{}; DenseReq dense{}; TableReq table{};
};

// `p` must be memory a queued copy can fill: RC_ERR_BAD_ARG with `msg` for anything but page-locked host memory
static int need_page_locked(const void *p, const char *msg)
{
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) == hipSuccess && a.type == hipMemoryTypeHost) return RC_OK;
    (void)hipGetLastError();
    return fail(RC_ERR_BAD_ARG, msg);
}

// a staged output's segments from `src` (device) to the caller's `dst`, same offsets on both sides
static int run_copy_plan(const rc::CopyPlan &plan, uint8_t *dst, const uint8_t *src, hipStream_t s)
{
    for (uint32_t i = 0; i < plan.nseg; ++i)
        HIP_TRY(hipMemcpyAsync(dst + plan.seg[i].off, src + plan.seg[i].off, plan.seg[i].bytes, hipMemcpyDeviceToHost, s));
    return RC_OK;
}

// The slot's head: [ZdTables bitmap x n][ZdTables values x n] (zstd) [block lists: bitmap x n, values x n, stored x threads, compact bitmap x n]
// [pv_bytes n] [base2 2n][pv_base n][src_base n][st_base n] [shifts 2n int32] (a shifted add only) - the same layout in page-locked host
// memory and on the device: one copy.  It is what the kernels read.
struct HeadLayout {
    uint64_t n, ntab, o_lists, o_base2, o_shift, bytes;
    HeadLayout(uint64_t n_ = 0, bool zstd = false, bool shifted = false) : n(n_), ntab(zstd ? n_ : 0)
    {
        o_lists = 2 * ntab * sizeof(rc::ZdTables);
        o_base2 = (o_lists + (3 * n + RC_READ_THREADS) * sizeof(rc::ZdFrameList) + n * 4 + 15) & ~15ull;
        o_shift = o_base2 + n * 5 * 8;
        bytes = o_shift + (shifted ? n * 8 : 0);
    }
};
struct HeadView {
    rc::ZdTables *bm_tab, *pv_tab;
    rc::ZdFrameList *bm_list, *pv_list, *raw_list, *cbm_list;
    uint32_t *pv_bytes; uint64_t *base2, *pv_base, *src_base, *st_base; int32_t *shifts;       // (shifts nullptr: not a shifted add)
};
static HeadView head_view(const HeadLayout &L, uint8_t *base)
{
    HeadView v;
    v.bm_tab = reinterpret_cast<rc::ZdTables *>(base); v.pv_tab = v.bm_tab + L.ntab;
    v.bm_list = reinterpret_cast<rc::ZdFrameList *>(base + L.o_lists); v.pv_list = v.bm_list + L.n; v.raw_list = v.pv_list + L.n;
    v.cbm_list = v.raw_list + RC_READ_THREADS;
    v.pv_bytes = reinterpret_cast<uint32_t *>(v.cbm_list + L.n);
    v.base2 = reinterpret_cast<uint64_t *>(base + L.o_base2); v.pv_base = v.base2 + 2 * L.n; v.src_base = v.pv_base + L.n; v.st_base = v.src_base + L.n;
    v.shifts = L.bytes > L.o_shift ? reinterpret_cast<int32_t *>(base + L.o_shift) : nullptr;
    return v;
}

// What the stages of one call hand to each other, on top of the request's frames and the slot's head as the HOST sees it (dev: the device)
struct ReadRun : ReadFrames, HeadView {
    const ReadRequest &q;
    UtilScope scope;
    Util *pU = nullptr; ReadRes *pu = nullptr; hipStream_t s = nullptr;
    uint64_t *h_res = nullptr;                 // page-locked: the prefix (n + 1) and the error word, as the device leaves them
    rc::ReadKindInfo kind;
    uint32_t codec, klevel, nblk, nthr = 1;
    bool vstream, values, l2out;               // the frames carry a value stream (level 1: residuals, level 2: statistics) ... which this call decodes
    uint64_t N, nb, nb8, bm_stride, pv_stride, total_in = 0, out_bytes;
    std::vector<uint64_t> foff, st_off;
    uint64_t stats_total = 0; uint32_t stats_max = 0; bool stats_short = false, stats_staged = false; uint16_t *stats_dev = nullptr;
    void *out; uint64_t cap;                   // the request's output and capacity - none once stats is short: the call still counts
    HeadLayout head; HeadView dev;
    const uint8_t *d_data, *d_bm, *d_pv; uint8_t *d_out; uint32_t *d_blk_cnt, *d_blk_off; uint64_t *d_fnnz, *d_fbase; int *d_err;
    const uint64_t *d_prefix;                  // where the kernels leave the prefix the caller gets
    uint64_t n_bm = 0, n_pv = 0, n_raw = 0;
    uint32_t bm_max = 0, pv_max = 0, raw_max_regen = 0, cbm_max = 0;
    void *target = nullptr;                    // device memory the kernels write the output to: the caller's, or d_triplets (nullptr: nothing yet)
    uint8_t *host_dst = nullptr;               // the caller's host memory, when the output is or will be staged in d_triplets
    uint64_t cell_bytes = 0;                   // bytes of a dense / trace output
    double t[5] = {};                          // RC_READ_TIMING
    explicit ReadRun(const ReadRequest &r) : ReadFrames(r.in), HeadView(), q(r) {}
    int begin(), host_walk(), decode(), route(), results(), finish();      // the stages, in expand_run's order
};
static double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// ---- stage 1: the checks, the sizes known without looking at the streams, the slot and its buffers ------------------------------------------
using namespace rc;      // (the stages below)
int ReadRun::begin()
{
    kind = read_kind_info(q.kind); l2out = kind.stats;
    if (!data || !sizes || (!q.nnz_prefix && !q.submit && !kind.cells) || n == 0 || nx == 0 || ny == 0 || (!q.out && q.cap) || (!q.stats && q.stats_cap))
        return fail(RC_ERR_BAD_ARG, "NULL / zero argument");
    if (level < 1 || level > 3) return fail(RC_ERR_UNSUPPORTED, "rc_expand_frames: reduction level 1, 2 or 3");
    if (level == 1 && (bit_depth == 0 || bit_depth > 64)) return fail(RC_ERR_BAD_ARG, "bit_depth must be 1..64");
    if (l2out && level != 2) return fail(RC_ERR_BAD_ARG, "rc_expand_frames_l2: reduction level 2");
    if (l2out && (bit_depth < 8 || bit_depth > 16))
        return fail(RC_ERR_UNSUPPORTED, "rc_expand_frames_l2: bit_depth 8..16 (narrower fields: the stream's length does not give their count)");
    if (op_mode != 0 && scheme != RC_SCHEME_LZ4 && scheme != RC_SCHEME_ZSTD && scheme != RC_SCHEME_BLOSC_LZ4 && scheme != RC_SCHEME_ZLIB_DEVICE)
        return fail(RC_ERR_UNSUPPORTED, "rc_expand_frames: scheme has no batched device decoder");
    if (op_mode != 0 && scheme == RC_SCHEME_ZLIB_DEVICE && level == 2)
        return fail(RC_ERR_UNSUPPORTED, "rc_expand_frames: the device inflate reads reduction levels 1 and 3");
    codec = op_mode == 0 ? EMIT_RAW : scheme;   // (EMIT_LZ4 / EMIT_ZSTD / EMIT_BLOSC / EMIT_DEFLATE are the scheme codes)
    vstream = level != 3; values = read_kind_values(q.kind, level); klevel = read_kind_klevel(q.kind, level);
    N = (uint64_t)nx * ny; nb = (N + 7) / 8; nb8 = (nb + 7) / 8;
    t[0] = now_ms();
    bm_stride = nb8 * 8 + 8; pv_stride = 16;
    std::vector<uint64_t>(n).swap(foff);
    for (uint32_t f = 0; f < n; ++f) {
        const uint32_t npk = values ? sizes[3 * f + 2] : 0;
        pv_stride = std::max<uint64_t>(pv_stride, ((uint64_t)npk + 15) & ~15ull);
        foff[f] = total_in;
        total_in += (uint64_t)sizes[3 * f] + (vstream ? sizes[3 * f + 1] : 0);
    }
    pv_stride += 16;
    // level-2 statistics: frame f holds floor(8 * sizes[f][2] / bit_depth) of them (exact for fields of a byte or more)
    std::vector<uint64_t>(l2out ? n : 0).swap(st_off);
    for (uint32_t f = 0; f < n && l2out; ++f) {
        const uint32_t c = (uint32_t)(8ull * sizes[3 * f + 2] / bit_depth);
        st_off[f] = stats_total;
        stats_total += c;
        stats_max = std::max(stats_max, c);
    }
    stats_short = stats_total > q.stats_cap;     // the synchronous call still counts (nnz_prefix stays valid), and writes nothing
    if (stats_short && q.submit) return fail(RC_ERR_OUT_TOO_SMALL, "rc_expand_frames_l2_submit: stats holds fewer entries than the frames have statistics");
    out = stats_short ? nullptr : q.out; cap = stats_short ? 0 : q.cap;
    int r = scope.enter();
    if (r != RC_OK) return r;
    Util &U = *(pU = &g_util); ReadRes &u = *(pu = &U.rr[q.slot]);
    if (u.pending) return fail(RC_ERR_BAD_ARG, "rc_expand_frames: this slot holds a submitted batch - rc_expand_frames_wait first");
    if (!u.stream) {
        for (hipStream_t *p : {&u.stream, &u.stream2}) HIP_TRY(hipStreamCreateWithFlags(p, hipStreamNonBlocking));
        for (hipEvent_t *p : {&u.ev_a, &u.ev_b, &u.done}) HIP_TRY(hipEventCreateWithFlags(p, hipEventDisableTiming));
    }
    if ((r = u.h_res.ensure(U.hmem, ((uint64_t)n + 2) * 8)) != RC_OK) return r;
    h_res = u.h_res.as<uint64_t>(); s = u.stream;
    nblk = (uint32_t)((nb8 + WG - 1) / WG);
    out_bytes = (uint64_t)n * (bm_stride + (values ? pv_stride : 0)) + 64;
    head = HeadLayout(n, codec == EMIT_ZSTD, q.shifts != nullptr);
    if ((r = u.d_data.ensure(U.dmem, total_in + 64)) != RC_OK || (r = u.d_streams.ensure(U.dmem, out_bytes)) != RC_OK ||
        (r = u.d_head.ensure(U.dmem, head.bytes)) != RC_OK ||
        (r = u.d_counters.ensure(U.dmem, (uint64_t)n * nblk * 8 + (uint64_t)(2 * n + 2) * 8 + 64)) != RC_OK ||
        (r = u.rd_head.ensure(U.hmem, head.bytes)) != RC_OK || (r = zstd_predefined_tables(U)) != RC_OK)
        return r;
    static_cast<HeadView &>(*this) = head_view(head, u.rd_head.p);
    dev = head_view(head, u.d_head.p);
    d_out = u.d_streams.p; d_bm = d_out; d_pv = d_out + (uint64_t)n * bm_stride;
    d_blk_cnt = u.d_counters.as<uint32_t>(); d_blk_off = d_blk_cnt + (uint64_t)n * nblk;
    d_fnnz = reinterpret_cast<uint64_t *>(d_blk_off + (uint64_t)n * nblk); d_fbase = d_fnnz + n;
    d_prefix = d_fbase; d_err = reinterpret_cast<int *>(d_fbase + n + 1);
    return RC_OK;
}

// ---- stage 2: the copy-in is queued, then the host walks the frames and builds block tables and decoding tables (a few threads, each
// claiming frames one at a time).  The copy-in reads the caller's memory: from here on expand_run does not return without waiting for it.
int ReadRun::host_walk()
{
    Util &U = *pU; ReadRes &u = *pu;
    // The compressed bytes: device memory is used where it lies; host memory is copied in, and the copy runs while the host walks the
    // streams.  (Letting the decoders read page-locked host memory in place - their staging loads as the transfer - was slower: the
    // transfer then sits inside the decoders' critical path, 1.3 ms against 0.7 ms behind a copy that hides under the host walk.)
    d_data = u.d_data.p;
    bool copy_in = true;
    {
        // in place only if the decoders' 16-byte staging loads (and the bit readers' dword loads) can neither be misaligned nor leave
        // the last page of the caller's allocation: they may touch up to 15 bytes behind the last stream
        const uintptr_t end = (uintptr_t)data + total_in;
        const bool usable = ((uintptr_t)data & 15u) == 0 && (end & 4095u) != 0 && (end & 4095u) <= 4096u - 16u;
        if (usable && is_device_ptr(data)) { d_data = data; copy_in = false; }
    }
    // The header walk below runs on the host.  Bytes that lie in device memory are fetched once into page-locked memory for it (the
    // host CAN read device memory through the PCIe aperture, a few hundred MB/s: 187 ms for 34 MB); the decoders read them where they are.
    const uint8_t *walk = data;
    if (is_device_ptr(data)) {
        int r = u.h_blob.ensure(U.hmem, total_in + 64, total_in / 4);
        if (r != RC_OK) return r;
        HIP_TRY(hipMemcpyAsync(u.h_blob.p, data, total_in, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        walk = u.h_blob.p;
    }
    if (copy_in) HIP_TRY(hipMemcpyAsync(u.d_data.p, data, total_in, hipMemcpyDefault, s));
    HIP_TRY(hipMemsetAsync(d_out, 0, out_bytes, s));   // bitmap padding and value-stream tails read as zero
    HIP_TRY(hipMemsetAsync(d_err, 0, 4, s));
    // The block lists stay where the indexing threads wrote them, in page-locked host memory: the decoders read every entry once,
    // over the link (uploading them meant 3 small copies per thread, each a fixed ~15 us of stream time: 0.7 ms per call).
    if (q.shifts) memcpy(shifts, q.shifts, (size_t)n * 8);
    // c0, c_n: the frame's range in its thread's compact offset list (c_n blocks = c_n + 1 offsets); c_skips: tree_skip | seq_skip << 8
    struct FrameIndex { uint32_t bm0 = 0, bm_n = 0, pv0 = 0, pv_n = 0, thread = 0, c0 = 0, c_n = 0, c_skips = 0; int status = ZD_OK; const char *what = nullptr; };
    std::vector<FrameIndex> fi(n);
    const uint32_t hw = usable_cpus();
    static const uint32_t thr_env = getenv("RC_READ_THREADS") ? (uint32_t)atoi(getenv("RC_READ_THREADS")) : 0u;   // (development: 1..16)
    nthr = std::max(1u, std::min<uint32_t>(std::min<uint32_t>(n, thr_env ? std::min<uint32_t>(thr_env, RC_READ_THREADS) : RC_READ_THREADS), hw));
    const int dev_now = U.device;
    // frames are claimed one at a time: the calling thread starts at once, the pool's workers join in as they wake up (their
    // wake-up, not the walk - 30 us per frame - is what a static split waited for)
    std::atomic<uint32_t> next_frame{0};
    uint64_t max_npk = 0;
    if (values) for (uint32_t f = 0; f < n; ++f) max_npk = std::max<uint64_t>(max_npk, sizes[3 * f + 2]);
    auto index_range = [&](uint32_t t) {
        if (t) (void)hipSetDevice(dev_now);   // (a worker thread: page-locked memory it allocates belongs to this device's context)
        auto &BM = u.rd_bm[t]; auto &PV = u.rd_pv[t]; auto &RAW = u.rd_raw[t]; auto &all = u.rd_tmp[t]; auto &OFF = u.rd_off[t];
        BM.clear(); PV.clear(); RAW.clear(); OFF.clear();
        if (codec == EMIT_BLOSC) BM.reserve(std::min<uint64_t>(n, 3ull * ((n + nthr - 1) / nthr)) * ((nb + TILE_BM - 1) / TILE_BM));   // (one entry per block)
        else if (codec) {
            // what this thread is likely to collect (frames are claimed one at a time: up to three times its even share), reserved
            // in one allocation each; anything beyond still grows by doubling
            const uint64_t share = std::min<uint64_t>(n, 3ull * ((n + nthr - 1) / nthr));
            OFF.reserve(share * ((nb + TILE_BM - 1) / TILE_BM + 1));
            if (values && codec == EMIT_ZSTD) PV.reserve(share * (max_npk / 1000 + 2));   // (value-stream chunks: PIX_CHUNK = 1008 bytes each)
        }
        // A binary-map stream whose blocks all regenerate TILE_BM bytes (the last one the rest), lie back to back and keep to one
        // set of sequence tables - what this library's encoders write - leaves one dword per block (k_bitmap_decode_c); any other
        // stream inside the decoders' subset leaves full entries, Compressed blocks and stored ones apart, as before.
        auto route_bitmap = [&](FrameIndex &F, uint64_t o, uint64_t cb, uint32_t hdr, bool one_table_set) {
            bool uniform = one_table_set && !all.empty() && cb < (1ull << 32);
            uint32_t skips = 0;
            for (size_t i = 0; uniform && i < all.size(); ++i) {
                const ZdBlock &b = all[i];
                const uint64_t want = std::min<uint64_t>((uint64_t)TILE_BM, nb - std::min<uint64_t>(nb, (uint64_t)i * TILE_BM));
                uniform = b.regen == want && b.dst == (uint64_t)i * TILE_BM && (i + 1 == all.size() || all[i + 1].src - hdr == b.src + b.csize);
                if (b.tree_skip) skips |= b.tree_skip;
                if (b.seq_skip > 1) skips |= (uint32_t)b.seq_skip << 8;     // (1 = the RLE offset byte of a block with predefined tables)
            }
            if (uniform) {
                F.c0 = (uint32_t)OFF.size(); F.c_n = (uint32_t)all.size(); F.c_skips = skips;
                for (const ZdBlock &b : all) OFF.push_back((uint32_t)(b.src - hdr - o));
                OFF.push_back((uint32_t)(all.back().src + all.back().csize - o));
            } else
                for (const ZdBlock &b : all) { if (b.type == 2) BM.push_back(b); else RAW.push_back(b); }
        };
        for (;;) {
            const uint32_t f = next_frame.fetch_add(1, std::memory_order_relaxed);
            if (f >= n) break;
            FrameIndex &F = fi[f];
            F.thread = t;
            const uint64_t cb = sizes[3 * f], cp = vstream ? sizes[3 * f + 1] : 0, npk = values ? sizes[3 * f + 2] : 0;
            const uint64_t o = foff[f];
            uint64_t got = 0;
            int rr = ZD_OK;
            F.bm0 = (uint32_t)BM.size(); F.pv0 = (uint32_t)PV.size();
            if (codec == EMIT_RAW) {
                if (cb != nb || cp != (vstream ? sizes[3 * f + 2] : 0u)) { F.status = ZD_CORRUPT; F.what = "rc_expand_frames: mode-0 sizes disagree with the frame shape"; continue; }
                ZdBlock b;
                memset(&b, 0, sizeof b);
                b.frame = f; b.src = o; b.csize = b.regen = (uint32_t)nb; b.dst = 0;
                RAW.push_back(b);
                if (npk) { b.src = o + cb; b.csize = b.regen = (uint32_t)npk; b.frame = n + f; RAW.push_back(b); }
            } else if (codec == EMIT_LZ4) {
                all.clear();
                rr = lz4_index_frame(walk, o, cb, f, TILE_BM, nb, all, all, &got);
                if (rr == ZD_OK && got != nb) rr = ZD_CORRUPT;
                if (rr == ZD_OK) route_bitmap(F, o, cb, 4, true);
                if (rr == ZD_OK && values) {
                    all.clear();   // (a value stream holds stored chunks only: a compressed block there is outside the subset)
                    rr = lz4_index_frame(walk, o + cb, cp, n + f, 0, npk, all, RAW, &got);
                    if (rr == ZD_OK && got != npk) rr = ZD_CORRUPT;
                }
            } else if (codec == EMIT_DEFLATE) {
                // No walk: the units' starts are found on the device (rc_inflate.hip).  The host only refuses what is plainly not the
                // device encoder's: another zlib header, or a first block of a type the stream cannot start with.
                auto own = [&](uint64_t at, uint64_t sz, uint32_t coded) {
                    return sz >= 8 && sz < (1ull << 28) && walk[at] == 0x78 && walk[at + 1] == 0x01 && ((walk[at + 2] & 6u) == 0u || (walk[at + 2] & 6u) == coded);
                };
                if (!own(o, cb, 2u) || (values && !own(o + cb, cp, 4u))) rr = ZD_FOREIGN;
            } else if (codec == EMIT_BLOSC) {
                // (every block of the map to the frame's list - stored ones too: they are shuffled like the others; a memcpyed chunk to the copy list)
                rr = blosc_index_stream(walk, o, cb, f, nb, true, BM, RAW);
                if (rr == ZD_OK && values) rr = blosc_index_stream(walk, o + cb, cp, n + f, npk, false, BM, RAW);
            } else {
                // (Compressed blocks to the stream's list, stored / RLE ones to the copy list, as the walk finds them)
                struct Route {
                    PinnedVec<ZdBlock> &comp, &raw;
                    bool values; uint32_t frame; bool too_long = false;
                    void push_back(const ZdBlock &b)
                    {
                        if (b.type != 2) { raw.push_back(b); return; }
                        if (!values) { comp.push_back(b); return; }
                        if (b.regen > 1024) { too_long = true; return; }   // a value-stream block the chunk decoder is not built for
                        ZdBlock c = b;
                        c.frame = frame;
                        comp.push_back(c);
                    }
                };
                Route rp{PV, RAW, true, f};
                all.clear();
                rr = zd_index_frame(walk, o, cb, f, TILE_BM, nb, all, bm_tab[f], &got);
                if (rr == ZD_OK && got != nb) rr = ZD_CORRUPT;
                if (rr == ZD_OK) route_bitmap(F, o, cb, 3, !(bm_tab[f].has & 4u));
                if (rr == ZD_OK && values) {
                    rr = zd_index_frame(walk, o + cb, cp, n + f, 0, npk, rp, pv_tab[f], &got);
                    if (rr == ZD_OK && got != npk) rr = ZD_CORRUPT;
                    if (rr == ZD_OK && rp.too_long) rr = ZD_FOREIGN;
                }
            }
            F.bm_n = (uint32_t)BM.size() - F.bm0; F.pv_n = (uint32_t)PV.size() - F.pv0;
            F.status = rr;
        }
    };
    g_pool->run(nthr, index_range);
    t[1] = now_ms();
    for (uint32_t t = 0; t < nthr; ++t) {
        if (!u.rd_bm[t].ok || !u.rd_pv[t].ok || !u.rd_raw[t].ok || !u.rd_off[t].ok) return fail(RC_ERR_DEVICE, "rc_expand_frames: page-locked host memory exhausted");
        raw_list[t].p = u.rd_raw[t].data(); raw_list[t].n = (uint32_t)u.rd_raw[t].size(); raw_list[t].pad = 0;
        n_raw += u.rd_raw[t].size();
        const ZdBlock *rb = u.rd_raw[t].data();
        for (size_t i = 0; i < u.rd_raw[t].size(); ++i) raw_max_regen = std::max(raw_max_regen, rb[i].regen);
    }
    for (uint32_t f = 0; f < n; ++f) {
        const FrameIndex &F = fi[f];
        const uint32_t t = F.thread;
        if (F.status == ZD_FOREIGN) return fail(RC_ERR_UNSUPPORTED, "rc_expand_frames: stream outside the device decoders' subset (use the stock decoder)");
        if (F.status != ZD_OK) return fail(RC_ERR_CORRUPT, F.what ? F.what : "rc_expand_frames: malformed compressed stream");
        bm_list[f].p = u.rd_bm[t].data() + F.bm0; bm_list[f].n = F.bm_n; bm_list[f].pad = 0;
        pv_list[f].p = u.rd_pv[t].data() + F.pv0; pv_list[f].n = F.pv_n; pv_list[f].pad = 0;
        cbm_list[f].p = reinterpret_cast<const ZdBlock *>(u.rd_off[t].data() + F.c0); cbm_list[f].n = F.c_n; cbm_list[f].pad = F.c_skips;
        src_base[f] = foff[f];
        cbm_max = std::max(cbm_max, F.c_n);
        pv_bytes[f] = values ? sizes[3 * f + 2] : 0;
        st_base[f] = l2out ? st_off[f] : 0;
        base2[f] = (uint64_t)f * bm_stride;                                        // stored blocks: frames 0..n-1 = bitmaps,
        base2[n + f] = pv_base[f] = (uint64_t)n * bm_stride + (uint64_t)f * pv_stride;   // n..2n-1 = value streams (behind the bitmaps)
        bm_max = std::max(bm_max, F.bm_n);
        pv_max = std::max(pv_max, F.pv_n);
        n_bm += F.bm_n; n_pv += F.pv_n;
    }
    if (n_raw >= (1ull << 31)) return fail(RC_ERR_UNSUPPORTED, "rc_expand_frames: too many blocks in one call");
    t[2] = now_ms();
    return RC_OK;
}

// ---- stage 3: the head's one copy, then the decoders ------------------------------------------------------------------------------------------
int ReadRun::decode()
{
    Util &U = *pU; ReadRes &u = *pu;
    const HeadView &d = dev;
    HIP_TRY(hipMemcpyAsync(u.d_head.p, u.rd_head.p, head.bytes, hipMemcpyHostToDevice, s));
    t[3] = now_ms();
    // the value streams' chunks (few, long serial chains) decode next to the binary maps' blocks (many, short), on a second stream
    static const bool serial = getenv("RC_READ_SERIAL") != nullptr;   // development: both decoders on one stream (clean per-kernel times)
    if (n_pv && serial) launch_block_decode(EMIT_ZSTD, 1024, d_data, d.pv_list, n, pv_max, d.pv_tab, U.zd_predef, d_out, d.pv_base, d_err, s);
    else if (n_pv) {
        HIP_TRY(hipEventRecord(u.ev_a, s));
        HIP_TRY(hipStreamWaitEvent(u.stream2, u.ev_a, 0));
        launch_block_decode(EMIT_ZSTD, 1024, d_data, d.pv_list, n, pv_max, d.pv_tab, U.zd_predef, d_out, d.pv_base, d_err, u.stream2);
        HIP_TRY(hipEventRecord(u.ev_b, u.stream2));
    }
    if (codec == EMIT_DEFLATE) {
        // stream descriptors (page-locked, one copy) and the tables of the candidate / chain scheme, all in one device buffer
        const uint32_t ns = values ? 2 * n : n;
        uint64_t cand_total = 0, unit_total = 0;
        uint32_t cap_max[2] = {0, 0}, units_max[2] = {0, 0};
        int r = u.h_inf.ensure(U.hmem, (uint64_t)ns * sizeof(InfStream));
        if (r != RC_OK) return r;
        InfStream *st = u.h_inf.as<InfStream>();
        for (uint32_t j = 0; j < ns; ++j) {
            const uint32_t f = j < n ? j : j - n, v = j < n ? 0u : 1u;
            InfStream &S = st[j];
            S.src = foff[f] + (v ? sizes[3 * f] : 0u);
            S.dst = v ? pv_base[f] : base2[f];
            S.csize = sizes[3 * f + v];
            S.size = v ? sizes[3 * f + 2] : (uint32_t)nb;
            S.unit = v ? INF_VAL_UNIT : INF_MAP_UNIT;
            S.units = inf_units(S.size, S.unit);
            S.cand0 = (uint32_t)cand_total; S.cap = 2 * S.units + INF_CAND_EXTRA;
            S.unit0 = (uint32_t)unit_total; S.pad = 0;
            cand_total += S.cap; unit_total += S.units;
            cap_max[v] = std::max(cap_max[v], S.cap); units_max[v] = std::max(units_max[v], S.units);
        }
        if (cand_total >= (1ull << 31)) return fail(RC_ERR_UNSUPPORTED, "rc_expand_frames: too many blocks in one call");
        const uint64_t o_tab = ((uint64_t)ns * sizeof(InfStream) + 15) & ~15ull;
        if ((r = u.d_inf.ensure(U.dmem, o_tab + (2 * cand_total + unit_total + ns) * 4 + 64)) != RC_OK) return r;
        HIP_TRY(hipMemcpyAsync(u.d_inf.p, st, (uint64_t)ns * sizeof(InfStream), hipMemcpyHostToDevice, s));
        uint32_t *d_cand = reinterpret_cast<uint32_t *>(u.d_inf.p + o_tab), *d_link = d_cand + cand_total, *d_unit = d_link + cand_total, *d_ncand = d_unit + unit_total;
        launch_inflate(d_data, u.d_inf.as<InfStream>(), n, ns - n, cap_max[0], units_max[0], cap_max[1], units_max[1], d_cand, d_ncand, d_link, d_unit, d_out,
                       d_err, s);
    }
    if (cbm_max) launch_bitmap_decode_compact(codec, d_data, d.cbm_list, d.src_base, n, cbm_max, d.bm_tab, U.zd_predef, d_out, d.base2, nb, d_err, s);
    if (n_bm && codec == EMIT_BLOSC) launch_blosc_decode_blocks(d_data, d.bm_list, n, bm_max, d_out, d.base2, d_err, s);
    else if (n_bm) launch_block_decode(codec, TILE_BM, d_data, d.bm_list, n, bm_max, d.bm_tab, U.zd_predef, d_out, d.base2, d_err, s);
    launch_block_copy(d_data, d.raw_list, nthr, (uint32_t)n_raw, raw_max_regen, d_out, d.base2, s);
    if (n_pv && !serial) HIP_TRY(hipStreamWaitEvent(s, u.ev_b, 0));
    return RC_OK;
}

// ---- stage 4: the output route of the kind - where the kernels write, and the count and the kernels behind it.  An output in host memory is
// staged in d_triplets: kinds that are `held` in both forms; entries for a submitted batch too (page-locked memory: one asynchronous copy of
// cap entries follows the emit kernel - the copy engine moves 64 MB in 1.3 ms under the next batch's work; letting the emit kernel write over
// the link itself - 8-byte stores, 24 bytes apart - took 4 ms); the synchronous call's entries are emitted by finish(), their number known.
int ReadRun::route()
{
    Util &U = *pU; ReadRes &u = *pu;
    const HeadView &d = dev; const ReadKindInfo &k = kind;
    int r = RC_OK;
    // level-2 statistics: unpacked where the caller wants them when the device can write there, otherwise staged - a submitted batch's
    // page-locked destination gets ONE asynchronous copy of all of them (their number is known here), the synchronous call copies at its end
    stats_dev = q.stats;
    if (k.stats && !stats_short && stats_total) {
        if (!is_device_ptr(q.stats)) {
            if (q.submit && (r = need_page_locked(q.stats, "rc_expand_frames_l2_submit: stats must be device or page-locked host memory")) != RC_OK) return r;
            if ((r = u.d_stats.ensure(U.dmem, stats_total * 2 + 64)) != RC_OK) return r;
            stats_dev = u.d_stats.as<uint16_t>(); stats_staged = true;
        }
        launch_stats_unpack(d_pv, pv_stride, d.pv_bytes, d.st_base, n, stats_max, bit_depth, stats_dev, d_err, s);
        if (stats_staged && q.submit) HIP_TRY(hipMemcpyAsync(q.stats, stats_dev, stats_total * 2, hipMemcpyDeviceToHost, s));
    }
    // Entries wanted in DEVICE memory: the emit kernel is queued right behind the count - no host round trip in between; the kernel that
    // finishes the count (k_expand_bases) checks what the host otherwise would (total <= cap, value streams long enough) and the emit
    // kernel writes nothing once any check or decoder has raised *d_err.
    if (k.cells) cell_bytes = (uint64_t)n * q.table.row_cells * (q.kind == RK_DENSE ? q.dense.cell_bytes : 8u);      // (a table's cells are int64)
    auto place = [&]() -> int {      // where the kernels write: the caller's device memory, or d_triplets for its host memory
        if (!out || is_device_ptr(out)) { target = out; return RC_OK; }
        host_dst = static_cast<uint8_t *>(out);
        if (q.submit && need_page_locked(out, k.pageable) != RC_OK) return RC_ERR_BAD_ARG;
        if (!k.held && !q.submit) return RC_OK;
        const int e = u.d_triplets.ensure(U.dmem, (k.cells ? cell_bytes : cap * k.esz) + 64);
        if (e == RC_OK) target = u.d_triplets.p;
        return e;
    };
    if (!k.counts && (r = place()) != RC_OK) return r;
    // the count: with a capacity only where entries follow it at once
    const bool emit_now = k.esz && !k.counts && target;
    if (k.esz && !k.counts && !emit_now) launch_expand_batch_count(d_bm, bm_stride, nb8, N, n, d_blk_cnt, d_blk_off, d_fnnz, d_fbase, s);
    else
        launch_expand_batch_count(d_bm, bm_stride, nb8, N, n, d_blk_cnt, d_blk_off, d_fnnz, d_fbase, s, d.pv_bytes, bit_depth, klevel,
                                  emit_now ? cap : ~0ull, d_err);
    if (k.counts) {
        // The workspace is sized by the set pixels the batch can hold.  Level 1: a frame's value stream bounds them (k_expand_bases refuses
        // a frame with more set pixels than its stream has fields), so nothing waits.  Levels 2 and 3: only the frame's size does - the
        // count is fetched first (one synchronisation, in the submit form too).
        uint64_t id_cap = 0;
        if (level == 1)
            for (uint32_t f = 0; f < n; ++f) id_cap += std::min<uint64_t>(N, 8ull * sizes[3 * f + 2] / bit_depth);
        else {
            HIP_TRY(hipMemcpyAsync(h_res, d_fbase + n, 8, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
            id_cap = h_res[0];
        }
        if (id_cap >= 0xFFFFFFFEull) return fail(RC_ERR_UNSUPPORTED, "rc_count_frames: 2^32 set pixels or more in one call (fewer frames per call)");
        id_cap = std::max<uint64_t>(id_cap, 1);
        if ((r = u.d_count.ensure(U.dmem, cnt_workspace_bytes(nb8, n, id_cap, q.count.method) + 64)) != RC_OK || (r = place()) != RC_OK) return r;
        if (k.sums)
            launch_count_place(d_bm, bm_stride, nb8, N, nx, n, d_blk_off, d_fbase, d_pv, pv_stride, d.pv_bytes, bit_depth, klevel, q.count.method,
                               q.count.area_threshold, u.d_count.p, id_cap, q.sum->acc, (uint64_t)q.sum->nx * q.sum->ny, q.count.upsample, q.sum->ev, d_err, s,
                               d.shifts);
        else
            launch_count_events(d_bm, bm_stride, nb8, N, nx, n, d_blk_off, d_fbase, d_pv, pv_stride, d.pv_bytes, bit_depth, klevel, q.count.method,
                                q.count.area_threshold, u.d_count.p, id_cap, target, cap, d_err, s);
        d_prefix = cnt_ev_base(u.d_count.p, n);      // (the frames' EVENT prefix)
    } else if (q.kind == RK_TRACE) {
        // the per-(frame, block) partial sums live in the counting workspace: no counting request shares a batch with a trace
        if ((r = u.d_count.ensure(U.dmem, trace_workspace_bytes(nb8, n, q.table.param) + 64)) != RC_OK) return r;
        launch_expand_batch_trace(d_bm, bm_stride, nb8, N, nx, n, d_blk_off, d_pv, pv_stride, d.pv_bytes, bit_depth, klevel,
                                  static_cast<const int32_t *>(q.table.plane), q.table.param, u.d_count.as<int64_t>(), static_cast<int64_t *>(target), d_err, s);
    } else if (q.kind == RK_CORR) {
        // (its per-(frame, chunk) partial rows live there too: corr_workspace_bytes, bounded by the launch's workgroups, not the frame's blocks)
        if ((r = u.d_count.ensure(U.dmem, corr_workspace_bytes(nb8, n, q.table.param, WG) + 64)) != RC_OK) return r;
        launch_expand_batch_corr(d_bm, bm_stride, nb8, N, nx, n, d_blk_off, d_pv, pv_stride, d.pv_bytes, bit_depth, klevel,
                                 static_cast<const int32_t *>(q.table.plane), q.table.param, u.d_count.as<int64_t>(), static_cast<int64_t *>(target), d_err, s);
    } else if (q.kind == RK_BINS) {
        // (and the per-(frame, chunk) rows of 2 B partials: bins_workspace_bytes, the output's size plus BINS_PARTIAL_BUDGET at most)
        if ((r = u.d_count.ensure(U.dmem, bins_workspace_bytes(nb8, n, q.table.param, WG) + 64)) != RC_OK) return r;
        launch_expand_batch_bins(d_bm, bm_stride, nb8, N, n, d_blk_off, d_pv, pv_stride, d.pv_bytes, bit_depth, klevel,
                                 static_cast<const uint16_t *>(q.table.plane), q.table.param, u.d_count.as<int64_t>(), static_cast<int64_t *>(target), d_err, s);
    } else if (q.kind == RK_DENSE)
        launch_expand_batch_dense(d_bm, bm_stride, nb8, N, nx, n, d_blk_off, d_pv, pv_stride, d.pv_bytes, bit_depth, klevel, q.dense.region,
                                  q.dense.cell_bytes, target, d_err, s);
    else if (k.sums) {
        HIP_TRY(hipStreamWaitEvent(s, q.sum->ev, 0));
        if (d.shifts)
            launch_expand_batch_sum_shifted(d_bm, bm_stride, nb8, N, nx, ny, n, d_blk_off, d_fnnz, d_pv, pv_stride, d.pv_bytes, bit_depth, klevel,
                                            d.shifts, q.sum->acc, d_err, s);
        else
            launch_expand_batch_sum(d_bm, bm_stride, nb8, N, n, d_blk_off, d_pv, pv_stride, d.pv_bytes, bit_depth, klevel, q.sum->acc, d_err, s);
        HIP_TRY(hipEventRecord(q.sum->ev, s));
    } else if (emit_now)
        launch_expand_batch_emit(d_bm, bm_stride, nb8, N, nx, n, d_blk_off, d_fbase, d_pv, pv_stride, d.pv_bytes, bit_depth, klevel, cap, target, s,
                                 d_err, k.coo);
    HIP_TRY(hipGetLastError());
    return RC_OK;
}

// ---- stage 5: finish.  Both forms fetch the prefix and the error word; a submit notes what rc_expand_frames_wait needs and is done ---------------
int ReadRun::results()
{
    ReadRes &u = *pu;
    HIP_TRY(hipMemcpyAsync(h_res, d_prefix, (uint64_t)(n + 1) * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(h_res + n + 1, d_err, 4, hipMemcpyDeviceToHost, s));
    if (!q.submit) return RC_OK;
    const bool late = read_copy_is_late(q.kind, codec == EMIT_DEFLATE);
    const int r = host_dst && !late ? run_copy_plan(read_copy_plan_early(q.kind, cap), host_dst, u.d_triplets.p, s) : RC_OK;
    if (r != RC_OK) return r;
    HIP_TRY(hipEventRecord(u.done, s));
    u.late_dst = late ? host_dst : nullptr;
    u.kind = q.kind; u.n = n; u.cap = cap; u.cell_bytes = cell_bytes; u.pending = true;
    return RC_OK;
}
// ... both forms, once the stream (rc_expand_frames_wait: the event) has been waited for: the prefix out before any refusal, then the verdict
static rc::Verdict read_judge(ReadRes &u, rc::VerdictRoute route, uint32_t n, uint64_t cap, uint64_t *nnz_prefix, rc::VerdictFacts f)
{
    const uint64_t *h_res = u.h_res.as<uint64_t>();
    if (nnz_prefix) memcpy(nnz_prefix, h_res, (size_t)(n + 1) * 8);
    f.err = (uint32_t)h_res[n + 1]; f.total = h_res[n]; f.cap = cap;
    const rc::Verdict v = rc::read_verdict(route, u.kind, f);
    if (v.status != RC_OK) fail(v.status, v.msg);
    return v;
}
// ... and a good batch's output, staged in d_triplets, goes back to the caller
static int read_copy_back(ReadRes &u, uint32_t n, uint64_t cap, uint64_t cell_bytes, uint8_t *dst)
{
    const rc::CopyPlan plan = rc::read_copy_plan(u.kind, cap, u.h_res.as<uint64_t>()[n], cell_bytes);
    if (!plan.nseg) return RC_OK;
    const int r = run_copy_plan(plan, dst, u.d_triplets.p, u.stream);
    if (r != RC_OK) return r;
    HIP_TRY(hipStreamSynchronize(u.stream));
    return RC_OK;
}
int ReadRun::finish()
{
    ReadRes &u = *pu;
    const VerdictRoute route = verdict_route_sync(kind);
    VerdictFacts f{0, 0, 0, out != nullptr, stats_short, false};
    // (level 1: the host checks each frame's share of the prefix against its value stream's bytes, where a waited-for batch has bit 4)
    for (uint32_t i = 0; i < n && route == VR_SYNC_ENTRIES && level == 1; ++i)
        f.values_short = f.values_short || ((h_res[i + 1] - h_res[i]) * bit_depth + 7) / 8 > pv_bytes[i];
    u.kind = q.kind; t[4] = now_ms();
    const Verdict v = read_judge(u, route, n, cap, q.nnz_prefix, f);
    if (stats_staged && v.decoded()) {      // (the statistics of a batch that decoded, whatever becomes of its entries)
        HIP_TRY(hipMemcpyAsync(q.stats, stats_dev, stats_total * 2, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    if (v.status != RC_OK || v.step == VS_NO_OUTPUT) return v.status;
    static const bool timing = getenv("RC_READ_TIMING") != nullptr;   // development: phase times on stderr
    const uint64_t total = h_res[n];
    if (!host_dst) {
        if (timing && route == VR_SYNC_ENTRIES)
            fprintf(stderr, "rc_expand_frames: index %.3f ms, merge %.3f, enqueue copies %.3f, decode+count+emit (to sync) %.3f\n", t[1] - t[0], t[2] - t[1],
                    t[3] - t[2], t[4] - t[3]);
        return RC_OK;
    }
    if (!target && total) {
        // entries for host memory, now that their number is known: the triplets packed, the arrays of a COO output at the caller's stride
        const uint64_t ecap = q.kind == RK_TRIPLETS ? total : cap;
        const int r = u.d_triplets.ensure(pU->dmem, ecap * kind.esz + 64);
        if (r != RC_OK) return r;
        launch_expand_batch_emit(d_bm, bm_stride, nb8, N, nx, n, d_blk_off, d_fbase, d_pv, pv_stride, dev.pv_bytes, bit_depth, klevel, ecap,
                                 u.d_triplets.p, s, nullptr, kind.coo);
        HIP_TRY(hipGetLastError());
    }
    const int r = read_copy_back(u, n, cap, cell_bytes, host_dst);
    if (r == RC_OK && timing && q.kind == RK_TRIPLETS && total)
        fprintf(stderr, "rc_expand_frames: index %.3f ms, merge %.3f, enqueue copies %.3f, decode+count (to sync) %.3f, emit %.3f\n", t[1] - t[0], t[2] - t[1],
                t[3] - t[2], t[4] - t[3], now_ms() - t[4]);
    return r;
}

// The batched reader behind every entry point below.  A stage that fails after the copy-in has been queued returns here, and the copy-in -
// it reads the caller's memory - is waited for before the call returns, whatever the failure was.
static int expand_run(ReadRequest q, const uint32_t *slot = nullptr)      // slot: a _submit form's (the entry point has checked it)
{
    if (slot) { q.slot = *slot; q.submit = true; }
    ReadRun R(q);
    int r = R.begin();                                             // checks, sizes, the slot and its buffers
    if (r != RC_OK) return r;
    if ((r = R.host_walk()) == RC_OK &&                            // copy-in queued; the host indexes the frames' blocks
        (r = R.decode()) == RC_OK &&                               // the decoders, on the slot's two streams
        (r = R.route()) == RC_OK)                                  // the count and the kind's kernels behind it
        r = R.results();                                           // prefix and error word on their way; a submit is noted for its wait
    if (r == RC_OK && q.submit) return RC_OK;
    const hipError_t e = hipStreamSynchronize(R.s);
    if (r != RC_OK) return r;
    HIP_TRY(e);
    return R.finish();                                             // verdict, and a staged output's way back
}

// ---- the entry points: a _submit form differs from its synchronous twin in the slot (checked first), in insisting on an output, and in
// leaving the prefix to rc_expand_frames_wait - `slot` is nullptr for the synchronous form -----------------------------------------------------
struct EntryNames { const char *slot, *no_out; uint32_t max_depth; const char *depth; };
static int entries_run(ReadRequest q, const uint32_t *slot)
{
    static const EntryNames names[4] = {
        {"rc_expand_frames_submit: slot 0 or 1", "rc_expand_frames_submit: triplets must be device or page-locked host memory", 0, nullptr},
        {"rc_expand_frames_coo_submit: slot 0 or 1", "rc_expand_frames_coo_submit: the output must be device or page-locked host memory", 16,
         "rc_expand_frames_coo: values are uint16 (bit_depth <= 16)"},
        {"rc_expand_frames_coo32_submit: slot 0 or 1", "rc_expand_frames_coo32_submit: the output must be device or page-locked host memory", 32,
         "rc_expand_frames_coo32: values are uint32 (bit_depth <= 32)"},
        {"rc_expand_frames_l2_submit: slot 0 or 1", "rc_expand_frames_l2_submit: the output must be device or page-locked host memory", 0, nullptr}};
    static_assert(RK_TRIPLETS == 0 && RK_COO16 == 1 && RK_COO32 == 2 && RK_L2 == 3, "names[] is indexed by the kind");
    const EntryNames &nm = names[q.kind];
    if (slot && *slot >= RC_READ_SLOTS) return fail(RC_ERR_BAD_ARG, nm.slot);
    if (slot && !q.out) return fail(RC_ERR_BAD_ARG, nm.no_out);
    if (nm.max_depth && q.in.level == 1 && q.in.bit_depth > nm.max_depth) return fail(RC_ERR_BAD_ARG, nm.depth);
    return expand_run(q, slot);
}
RC_EXPORT int rc_expand_frames(uint32_t nx, uint32_t ny, uint32_t bit_depth, uint32_t level, uint32_t op_mode, uint32_t scheme,
                               const uint8_t *data, const uint32_t *sizes, uint32_t n, uint64_t *nnz_prefix, uint64_t *triplets, uint64_t cap)
{ return entries_run({.in = {nx, ny, bit_depth, level, op_mode, scheme, data, sizes, n}, .nnz_prefix = nnz_prefix, .kind = rc::RK_TRIPLETS, .out = triplets, .cap = cap},
                       nullptr); }
RC_EXPORT int rc_expand_frames_submit(uint32_t slot, uint32_t nx, uint32_t ny, uint32_t bit_depth, uint32_t level, uint32_t op_mode,
                                      uint32_t scheme, const uint8_t *data, const uint32_t *sizes, uint32_t n, uint64_t *triplets_dev, uint64_t cap)
{ return entries_run({.in = {nx, ny, bit_depth, level, op_mode, scheme, data, sizes, n}, .kind = rc::RK_TRIPLETS, .out = triplets_dev, .cap = cap}, &slot); }
RC_EXPORT int rc_expand_frames_coo(uint32_t nx, uint32_t ny, uint32_t bit_depth, uint32_t level, uint32_t op_mode, uint32_t scheme,
                                   const uint8_t *data, const uint32_t *sizes, uint32_t n, uint64_t *nnz_prefix, void *coo, uint64_t cap)
{ return entries_run({.in = {nx, ny, bit_depth, level, op_mode, scheme, data, sizes, n}, .nnz_prefix = nnz_prefix, .kind = rc::RK_COO16, .out = coo, .cap = cap}, nullptr); }
RC_EXPORT int rc_expand_frames_coo_submit(uint32_t slot, uint32_t nx, uint32_t ny, uint32_t bit_depth, uint32_t level, uint32_t op_mode,
                                          uint32_t scheme, const uint8_t *data, const uint32_t *sizes, uint32_t n, void *coo_dev, uint64_t cap)
{ return entries_run({.in = {nx, ny, bit_depth, level, op_mode, scheme, data, sizes, n}, .kind = rc::RK_COO16, .out = coo_dev, .cap = cap}, &slot); }
RC_EXPORT int rc_expand_frames_coo32(uint32_t nx, uint32_t ny, uint32_t bit_depth, uint32_t level, uint32_t op_mode, uint32_t scheme,
                                     const uint8_t *data, const uint32_t *sizes, uint32_t n, uint64_t *nnz_prefix, void *coo, uint64_t cap)
{ return entries_run({.in = {nx, ny, bit_depth, level, op_mode, scheme, data, sizes, n}, .nnz_prefix = nnz_prefix, .kind = rc::RK_COO32, .out = coo, .cap = cap}, nullptr); }
RC_EXPORT int rc_expand_frames_coo32_submit(uint32_t slot, uint32_t nx, uint32_t ny, uint32_t bit_depth, uint32_t level, uint32_t op_mode,
                                            uint32_t scheme, const uint8_t *data, const uint32_t *sizes, uint32_t n, void *coo_dev, uint64_t cap)
{ return entries_run({.in = {nx, ny, bit_depth, level, op_mode, scheme, data, sizes, n}, .kind = rc::RK_COO32, .out = coo_dev, .cap = cap}, &slot); }
RC_EXPORT int rc_expand_frames_l2(uint32_t nx, uint32_t ny, uint32_t bit_depth, uint32_t op_mode, uint32_t scheme, const uint8_t *data,
                                  const uint32_t *sizes, uint32_t n, uint64_t *nnz_prefix, void *rc, uint64_t cap, uint16_t *stats, uint64_t stats_cap)
{ return entries_run({.in = {nx, ny, bit_depth, 2, op_mode, scheme, data, sizes, n}, .nnz_prefix = nnz_prefix, .kind = rc::RK_L2, .out = rc, .cap = cap,
                        .stats = stats, .stats_cap = stats_cap}, nullptr); }
RC_EXPORT int rc_expand_frames_l2_submit(uint32_t slot, uint32_t nx, uint32_t ny, uint32_t bit_depth, uint32_t op_mode, uint32_t scheme,
                                         const uint8_t *data, const uint32_t *sizes, uint32_t n, void *rc_dev, uint64_t cap, uint16_t *stats_dev,
                                         uint64_t stats_cap)
{ return entries_run({.in = {nx, ny, bit_depth, 2, op_mode, scheme, data, sizes, n}, .kind = rc::RK_L2, .out = rc_dev, .cap = cap, .stats = stats_dev,
                        .stats_cap = stats_cap}, &slot); }

RC_EXPORT int rc_expand_frames_wait(uint32_t slot, uint64_t *nnz_prefix)
{
    if (slot >= RC_READ_SLOTS || !nnz_prefix) return fail(RC_ERR_BAD_ARG, "rc_expand_frames_wait: slot 0 or 1, nnz_prefix");
    UtilScope util_scope;
    int r = util_scope.enter();
    if (r != RC_OK) return r;
    ReadRes &u = g_util.rr[slot];
    if (!u.pending) return fail(RC_ERR_BAD_ARG, "rc_expand_frames_wait: nothing was submitted to this slot");
    u.pending = false;
    HIP_TRY(hipEventSynchronize(u.done));
    const rc::Verdict v = read_judge(u, rc::VR_WAIT, u.n, u.cap, nnz_prefix, {});
    return v.status == RC_OK && u.late_dst ? read_copy_back(u, u.n, u.cap, u.cell_bytes, u.late_dst) : v.status;
}

// ---- dense frame batches: a region of every frame as an array of cells (rc_dense.hip) -------------------------------------------------
// what both forms check before the device is asked for: from the arguments alone
static int dense_admit(uint32_t nx, uint32_t ny, uint32_t bit_depth, uint32_t level, uint32_t n, const DenseReq &q, const void *out, uint64_t out_cells)
{
    const rc::DenseRegion &g = q.region;
    if (!out || n == 0 || nx == 0 || ny == 0) return fail(RC_ERR_BAD_ARG, "rc_expand_frames_dense: NULL / zero argument");
    if (nx > 65535u || ny > 65535u) return fail(RC_ERR_BAD_ARG, "rc_expand_frames_dense: nx, ny in 1..65535");
    if (g.step_x == 0 || g.step_y == 0 || g.w == 0 || g.h == 0) return fail(RC_ERR_BAD_ARG, "rc_expand_frames_dense: w, h, step_x and step_y must be positive");
    if ((uint64_t)g.x0 + (uint64_t)(g.w - 1) * g.step_x >= nx || (uint64_t)g.y0 + (uint64_t)(g.h - 1) * g.step_y >= ny)
        return fail(RC_ERR_BAD_ARG, "rc_expand_frames_dense: the region leaves the frame");
    if (q.cell_bytes != 1 && q.cell_bytes != 2 && q.cell_bytes != 4) return fail(RC_ERR_BAD_ARG, "rc_expand_frames_dense: cell_bytes 1, 2 or 4");
    if (level == 1 && bit_depth > 32) return fail(RC_ERR_UNSUPPORTED, "rc_expand_frames_dense: bit_depth above 32 (the cells are uint32 at most)");
    if (level == 1 && bit_depth > 8 * q.cell_bytes) return fail(RC_ERR_BAD_ARG, "rc_expand_frames_dense: a cell of cell_bytes bytes does not hold bit_depth bits");
    if ((uintptr_t)out % q.cell_bytes) return fail(RC_ERR_BAD_ARG, "rc_expand_frames_dense: out must be aligned to its cells");
    if (out_cells < (uint64_t)n * g.w * g.h) return fail(RC_ERR_OUT_TOO_SMALL, "rc_expand_frames_dense: out holds fewer than n * w * h cells");
    return RC_OK;
}
static int dense_run(const uint32_t *slot, ReadRequest q)
{
    if (slot && *slot >= RC_READ_SLOTS) return fail(RC_ERR_BAD_ARG, "rc_expand_frames_dense_submit: slot 0 or 1");
    const int r = dense_admit(q.in.nx, q.in.ny, q.in.bit_depth, q.in.level, q.in.n, q.dense, q.out, q.cap);
    if (r != RC_OK) return r;
    q.table.row_cells = (uint64_t)q.dense.region.w * q.dense.region.h;
    return expand_run(q, slot);
}
RC_EXPORT int rc_expand_frames_dense(uint32_t nx, uint32_t ny, uint32_t bit_depth, uint32_t level, uint32_t op_mode, uint32_t scheme, const uint8_t *data,
                                     const uint32_t *sizes, uint32_t n, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, uint32_t step_x, uint32_t step_y,
                                     uint32_t cell_bytes, void *out, uint64_t out_cells, uint64_t *nnz_prefix)
{ return dense_run(nullptr, {.in = {nx, ny, bit_depth, level, op_mode, scheme, data, sizes, n}, .nnz_prefix = nnz_prefix, .kind = rc::RK_DENSE, .out = out,
                               .cap = out_cells, .dense = {{x0, y0, w, h, step_x, step_y}, cell_bytes}}); }
RC_EXPORT int rc_expand_frames_dense_submit(uint32_t slot, uint32_t nx, uint32_t ny, uint32_t bit_depth, uint32_t level, uint32_t op_mode, uint32_t scheme,
                                            const uint8_t *data, const uint32_t *sizes, uint32_t n, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
                                            uint32_t step_x, uint32_t step_y, uint32_t cell_bytes, void *out, uint64_t out_cells)
{ return dense_run(&slot, {.in = {nx, ny, bit_depth, level, op_mode, scheme, data, sizes, n}, .kind = rc::RK_DENSE, .out = out, .cap = out_cells,
                             .dense = {{x0, y0, w, h, step_x, step_y}, cell_bytes}}); }

// ---- electron counting: one event per connected component of a frame's set pixels (rc_count.hip) -------------------------------------
static int count_admit(uint32_t nx, uint32_t ny, uint32_t bit_depth, uint32_t level, uint32_t method)
{
    if (method > rc::CNT_MAX) return fail(RC_ERR_BAD_ARG, "rc_count_frames: method 0 (weighted average), 1 (unweighted average) or 2 (maximum)");
    if (nx > 65535u || ny > 65535u) return fail(RC_ERR_BAD_ARG, "rc_count_frames: nx, ny in 1..65535");
    if (level == 1 && bit_depth > 16) return fail(RC_ERR_UNSUPPORTED, "rc_count_frames: bit_depth above 16 (the sums are exact in 64 bits for 16-bit values)");
    return RC_OK;
}
static int count_run(const uint32_t *slot, ReadRequest q)
{
    if (slot && *slot >= RC_READ_SLOTS) return fail(RC_ERR_BAD_ARG, "rc_count_frames_submit: slot 0 or 1");
    if (slot && !q.out) return fail(RC_ERR_BAD_ARG, "rc_count_frames_submit: events must be device or page-locked host memory");
    const int r = count_admit(q.in.nx, q.in.ny, q.in.bit_depth, q.in.level, q.count.method);
    return r != RC_OK ? r : expand_run(q, slot);
}
RC_EXPORT int rc_count_frames(uint32_t nx, uint32_t ny, uint32_t bit_depth, uint32_t level, uint32_t op_mode, uint32_t scheme, const uint8_t *data,
                              const uint32_t *sizes, uint32_t n, uint32_t method, uint32_t area_threshold, uint64_t *nev_prefix, void *events, uint64_t cap)
{ return count_run(nullptr, {.in = {nx, ny, bit_depth, level, op_mode, scheme, data, sizes, n}, .nnz_prefix = nev_prefix, .kind = rc::RK_EVENTS, .out = events,
                               .cap = cap, .count = {method, area_threshold, 0}}); }
RC_EXPORT int rc_count_frames_submit(uint32_t slot, uint32_t nx, uint32_t ny, uint32_t bit_depth, uint32_t level, uint32_t op_mode, uint32_t scheme,
                                     const uint8_t *data, const uint32_t *sizes, uint32_t n, uint32_t method, uint32_t area_threshold, void *events_dev,
                                     uint64_t cap)
{ return count_run(&slot, {.in = {nx, ny, bit_depth, level, op_mode, scheme, data, sizes, n}, .kind = rc::RK_EVENTS, .out = events_dev, .cap = cap,
                             .count = {method, area_threshold, 0}}); }

// ---- summed views: an accumulator the caller owns, and expand_run's route into it ------------------------------------------------------
RC_EXPORT rc_sum *rc_sum_create(uint32_t nx, uint32_t ny, int *status)
{
    auto done = [&](int code) { if (status) *status = code; return (rc_sum *)nullptr; };
    if (nx == 0 || ny == 0 || nx > 65535u || ny > 65535u) return done(fail(RC_ERR_BAD_ARG, "rc_sum_create: nx, ny in 1..65535"));
    UtilScope util_scope;
    int r = util_scope.enter();
    if (r != RC_OK) return done(r);
    rc_sum *s = new (std::nothrow) rc_sum;
    if (!s) return done(fail(RC_ERR_WORKSPACE, "rc_sum_create: out of host memory"));
    s->device = g_util.device; s->nx = nx; s->ny = ny;
    const uint64_t bytes = (uint64_t)nx * ny * 4;
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&s->acc), bytes);
    if (e == hipSuccess) e = hipMemset(s->acc, 0, bytes);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&s->ev, hipEventDisableTiming);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        r = hip_fail(e, "rc_sum_create");
        if (s->stream) (void)hipStreamDestroy(s->stream);
        if (s->ev) (void)hipEventDestroy(s->ev);
        if (s->acc) (void)hipFree(s->acc);
        delete s;
        return done(r);
    }
    if (status) *status = RC_OK;
    return s;
}

RC_EXPORT int rc_sum_destroy(rc_sum *s)
{
    if (!s) return RC_OK;
    RC_ON_DEVICE(s->device);
    (void)hipEventSynchronize(s->ev);      // (an add that is still queued writes into acc)
    (void)hipStreamDestroy(s->stream);
    (void)hipEventDestroy(s->ev);
    (void)hipFree(s->acc);
    delete s;
    return RC_OK;
}

RC_EXPORT uint64_t rc_sum_bound(const rc_sum *s) { return s ? s->bound : 0; }

// what both add calls check before anything is queued; *grow: what the batch adds to the handle's bound
static int sum_admit(const rc_sum *s, uint32_t bit_depth, uint32_t level, uint32_t op_mode, const uint32_t *sizes, uint32_t n, uint64_t *grow)
{
    if (!s || !sizes || n == 0) return fail(RC_ERR_BAD_ARG, "rc_sum_add_frames: NULL / zero argument");
    if (level == 1 && bit_depth > 16) return fail(RC_ERR_UNSUPPORTED, "rc_sum_add_frames: bit_depth above 16 (the cells are uint32; 64-bit cells are not offered)");
    if (level == 1 && bit_depth == 0) return fail(RC_ERR_BAD_ARG, "bit_depth must be 1..64");
    // the frame shape is the handle's; stored streams (op_mode 0) show another one on their face - compressed ones when they decode (RC_ERR_CORRUPT)
    const uint64_t nb = ((uint64_t)s->nx * s->ny + 7) / 8;
    for (uint32_t f = 0; f < n && op_mode == 0; ++f)
        if (sizes[3 * f] != nb) return fail(RC_ERR_BAD_ARG, "rc_sum_add_frames: the frames' geometry differs from the handle's");
    *grow = (uint64_t)n * (level == 1 ? (1ull << bit_depth) - 1 : 1ull);
    if (s->bound + *grow > 0xFFFFFFFFull)
        return fail(RC_ERR_OUT_TOO_SMALL, "rc_sum_add_frames: a cell could pass 2^32 - 1 (rc_sum_fetch with reset first)");
    return RC_OK;
}
// expand_run runs on the caller's current device or RC_DEVICE; what a handle (a view, a per-frame table) owns lives on the device it was created on
static int handle_on_current_device(int device, const char *who)
{
    UtilScope util_scope;
    const int r = util_scope.enter();
    if (r != RC_OK) return r;
    return g_util.device == device ? RC_OK : fail(RC_ERR_BAD_ARG, (std::string(who) + ": the handle belongs to another device").c_str());
}

// the end of every add, plain or counted: the synchronous forms lend a prefix of their own to a caller without one; the bound grows with
// what was queued (a submit: a batch the device rejects later adds nothing, the bound stays an upper bound)
static int add_run(rc_sum *s, const uint32_t *slot, uint64_t grow, ReadRequest &q)
{
    std::vector<uint64_t> own(slot || q.nnz_prefix ? 0 : (size_t)q.in.n + 1);
    if (!own.empty()) q.nnz_prefix = own.data();
    q.sum = s;
    const int r = expand_run(q, slot);
    if (r == RC_OK) s->bound += grow;
    return r;
}
// shifts_msg: the form takes shifts, and this is what it says without them (q.in.nx, ny: the handle's, filled in here)
static int sum_add_run(rc_sum *s, const uint32_t *slot, const char *slot_msg, const char *shifts_msg, ReadRequest q)
{
    if (slot && *slot >= RC_READ_SLOTS) return fail(RC_ERR_BAD_ARG, slot_msg);
    if (shifts_msg && !q.shifts) return fail(RC_ERR_BAD_ARG, shifts_msg);
    uint64_t grow = 0;
    int r = sum_admit(s, q.in.bit_depth, q.in.level, q.in.op_mode, q.in.sizes, q.in.n, &grow);
    if (r == RC_OK) r = handle_on_current_device(s->device, "rc_sum_add_frames");
    if (r != RC_OK) return r;
    q.in.nx = s->nx; q.in.ny = s->ny;
    return add_run(s, slot, grow, q);
}
RC_EXPORT int rc_sum_add_frames(rc_sum *s, uint32_t bit_depth, uint32_t level, uint32_t op_mode, uint32_t scheme, const uint8_t *data,
                                const uint32_t *sizes, uint32_t n, uint64_t *nnz_prefix)
{ return sum_add_run(s, nullptr, nullptr, nullptr, {.in = {0, 0, bit_depth, level, op_mode, scheme, data, sizes, n}, .nnz_prefix = nnz_prefix, .kind = rc::RK_SUM}); }
RC_EXPORT int rc_sum_add_frames_submit(rc_sum *s, uint32_t slot, uint32_t bit_depth, uint32_t level, uint32_t op_mode, uint32_t scheme,
                                       const uint8_t *data, const uint32_t *sizes, uint32_t n)
{ return sum_add_run(s, &slot, "rc_sum_add_frames_submit: slot 0 or 1", nullptr, {.in = {0, 0, bit_depth, level, op_mode, scheme, data, sizes, n}, .kind = rc::RK_SUM}); }

// ---- aligned views: the same adds with frame f translated by (shifts[2 * f], shifts[2 * f + 1]) = (dy, dx) cells of the view ---------------
// Everything the unshifted calls check is checked as they check it, in their order; the shifts themselves cannot be wrong (any int32 pair
// is legal), only missing.  The bound grows as for the unshifted add: dropping only lowers a sum.
RC_EXPORT int rc_sum_add_frames_shifted(rc_sum *s, uint32_t bit_depth, uint32_t level, uint32_t op_mode, uint32_t scheme, const uint8_t *data,
                                        const uint32_t *sizes, uint32_t n, const int32_t *shifts, uint64_t *nnz_prefix)
{ return sum_add_run(s, nullptr, nullptr, "rc_sum_add_frames_shifted: shifts is NULL",
                       {.in = {0, 0, bit_depth, level, op_mode, scheme, data, sizes, n}, .nnz_prefix = nnz_prefix, .kind = rc::RK_SUM, .shifts = shifts}); }
RC_EXPORT int rc_sum_add_frames_shifted_submit(rc_sum *s, uint32_t slot, uint32_t bit_depth, uint32_t level, uint32_t op_mode, uint32_t scheme,
                                               const uint8_t *data, const uint32_t *sizes, uint32_t n, const int32_t *shifts)
{ return sum_add_run(s, &slot, "rc_sum_add_frames_shifted_submit: slot 0 or 1", "rc_sum_add_frames_shifted_submit: shifts is NULL",
                       {.in = {0, 0, bit_depth, level, op_mode, scheme, data, sizes, n}, .kind = rc::RK_SUM, .shifts = shifts}); }

RC_EXPORT int rc_sum_fetch(rc_sum *s, uint32_t *dst, int reset)
{
    if (!s || !dst) return fail(RC_ERR_BAD_ARG, "rc_sum_fetch: NULL argument");
    RC_ON_DEVICE(s->device);
    const uint64_t bytes = (uint64_t)s->nx * s->ny * 4;
    HIP_TRY(hipEventSynchronize(s->ev));
    HIP_TRY(hipMemcpyAsync(dst, s->acc, bytes, is_device_ptr(dst) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s->stream));
    if (reset) HIP_TRY(hipMemsetAsync(s->acc, 0, bytes, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    if (reset) s->bound = 0;
    return RC_OK;
}

// ---- counted views: one count per event, added to a view up to 16 times finer than the frame (rc_count.hip: k_cnt_place) -------------
// what both counted adds check before anything is queued - first what needs no device and no look at the handle, then the device, then
// the handle; *grow: what the batch adds to the handle's bound
static int counted_admit(const rc_sum *s, uint32_t nx, uint32_t ny, uint32_t upsample, uint32_t bit_depth, uint32_t level, const uint32_t *sizes,
                         uint32_t n, uint32_t method, uint64_t *grow)
{
    if (!s || !sizes || n == 0 || nx == 0 || ny == 0) return fail(RC_ERR_BAD_ARG, "rc_sum_add_counted: NULL / zero argument");
    if (upsample < 1 || upsample > 16) return fail(RC_ERR_BAD_ARG, "rc_sum_add_counted: upsample in 1..16");
    int r = count_admit(nx, ny, bit_depth, level, method);
    if (r != RC_OK) return r;
    if (level == 1 && bit_depth == 0) return fail(RC_ERR_BAD_ARG, "bit_depth must be 1..64");
    if ((r = handle_on_current_device(s->device, "rc_sum_add_counted")) != RC_OK) return r;
    if ((uint64_t)upsample * nx != s->nx || (uint64_t)upsample * ny != s->ny)
        return fail(RC_ERR_BAD_ARG, "rc_sum_add_counted: the handle's shape is not (upsample * nx, upsample * ny)");
    // a frame's events: an aligned 2 x 2 block of pixels belongs to at most one 8-connected component; at level 1 the value stream has room
    // for floor(8 * bytes / bit_depth) set pixels and k_expand_bases refuses a frame with more
    const uint64_t blocks = (uint64_t)((nx + 1) / 2) * ((ny + 1) / 2);
    *grow = 0;
    for (uint32_t f = 0; f < n; ++f) *grow += level == 1 ? std::min<uint64_t>(blocks, 8ull * sizes[3 * f + 2] / bit_depth) : blocks;
    if (s->bound + *grow > 0xFFFFFFFFull)
        return fail(RC_ERR_OUT_TOO_SMALL, "rc_sum_add_counted: a cell could pass 2^32 - 1 (rc_sum_fetch with reset first)");
    return RC_OK;
}
static int counted_run(rc_sum *s, const uint32_t *slot, const char *slot_msg, const char *shifts_msg, ReadRequest q)
{
    if (slot && *slot >= RC_READ_SLOTS) return fail(RC_ERR_BAD_ARG, slot_msg);
    if (shifts_msg && !q.shifts) return fail(RC_ERR_BAD_ARG, shifts_msg);
    uint64_t grow = 0;
    const int r = counted_admit(s, q.in.nx, q.in.ny, q.count.upsample, q.in.bit_depth, q.in.level, q.in.sizes, q.in.n, q.count.method, &grow);
    return r != RC_OK ? r : add_run(s, slot, grow, q);
}
RC_EXPORT int rc_sum_add_counted(rc_sum *s, uint32_t nx, uint32_t ny, uint32_t upsample, uint32_t bit_depth, uint32_t level, uint32_t op_mode, uint32_t scheme,
                                 const uint8_t *data, const uint32_t *sizes, uint32_t n, uint32_t method, uint32_t area_threshold, uint64_t *nev_prefix)
{ return counted_run(s, nullptr, nullptr, nullptr, {.in = {nx, ny, bit_depth, level, op_mode, scheme, data, sizes, n}, .nnz_prefix = nev_prefix,
                                                      .kind = rc::RK_COUNTED_SUM, .count = {method, area_threshold, upsample}}); }
RC_EXPORT int rc_sum_add_counted_submit(rc_sum *s, uint32_t slot, uint32_t nx, uint32_t ny, uint32_t upsample, uint32_t bit_depth, uint32_t level,
                                        uint32_t op_mode, uint32_t scheme, const uint8_t *data, const uint32_t *sizes, uint32_t n, uint32_t method,
                                        uint32_t area_threshold)
{ return counted_run(s, &slot, "rc_sum_add_counted_submit: slot 0 or 1", nullptr,
                       {.in = {nx, ny, bit_depth, level, op_mode, scheme, data, sizes, n}, .kind = rc::RK_COUNTED_SUM, .count = {method, area_threshold, upsample}}); }
// the counted adds with shifts in FINE cells (1 / upsample pixel): the event is placed as above and then translated
RC_EXPORT int rc_sum_add_counted_shifted(rc_sum *s, uint32_t nx, uint32_t ny, uint32_t upsample, uint32_t bit_depth, uint32_t level, uint32_t op_mode,
                                         uint32_t scheme, const uint8_t *data, const uint32_t *sizes, uint32_t n, uint32_t method, uint32_t area_threshold,
                                         const int32_t *shifts, uint64_t *nev_prefix)
{ return counted_run(s, nullptr, nullptr, "rc_sum_add_counted_shifted: shifts is NULL",
                       {.in = {nx, ny, bit_depth, level, op_mode, scheme, data, sizes, n}, .nnz_prefix = nev_prefix, .kind = rc::RK_COUNTED_SUM, .shifts = shifts,
                        .count = {method, area_threshold, upsample}}); }
RC_EXPORT int rc_sum_add_counted_shifted_submit(rc_sum *s, uint32_t slot, uint32_t nx, uint32_t ny, uint32_t upsample, uint32_t bit_depth, uint32_t level,
                                                uint32_t op_mode, uint32_t scheme, const uint8_t *data, const uint32_t *sizes, uint32_t n, uint32_t method,
                                                uint32_t area_threshold, const int32_t *shifts)
{ return counted_run(s, &slot, "rc_sum_add_counted_shifted_submit: slot 0 or 1", "rc_sum_add_counted_shifted_submit: shifts is NULL",
                       {.in = {nx, ny, bit_depth, level, op_mode, scheme, data, sizes, n}, .kind = rc::RK_COUNTED_SUM, .shifts = shifts,
                        .count = {method, area_threshold, upsample}}); }

// ---- per-frame tables: a batch of frames becomes int64[n][row_cells], one row per frame (rc_trace.hip, rc_corr.hip, rc_bins.hip) -----------
// What the three kinds share.  A handle owns one plane in device memory, read-only after create - batches on both slots and the synchronous
// call may use it at once - and knows the frames' shape, the kernels' parameter and the cells of a row.  A kind adds what its no-wrap rule needs:
//   traces        int32[ny * nx][kp], the weight planes interleaved (kp = k rounded up to a multiple of 4; the padding planes are zero);
//                 param = k, a row = the set pixels, the sum, its first moments and k weighted sums; every plane's maxabs
//   correlations  int32[ny + 2 R][nx + 2 R], the reference inside a border of zeros; param = R, a row = the (2 R + 1)^2 cells of the window;
//                 the reference's maxabs
//   bins          uint16[ny][nx], the label map - every label below n_bins or BINS_IGNORE: create has checked it, the kernel relies on it
//                 for nothing but the result; param = n_bins, a row = [counts n_bins][sums n_bins]; no rule (rc_bins.h: a cell stays below 2^48)
struct FrameTable {
    int device = -1;
    uint32_t nx = 0, ny = 0, param = 0;
    void *plane = nullptr;
    uint64_t row_cells = 0;
};
struct rc_trace : FrameTable { uint32_t bound[rc::TRACE_MAX_PLANES] = {}; };
struct rc_corr : FrameTable { uint32_t bound = 0; };
struct rc_bins : FrameTable {};
// what a kind's calls say: who = the synchronous entry point (a NULL handle is answered in its name too, so it is not the handle's to keep);
// row, wrap: the refusals of an output too small and of a batch that could wrap, behind `who`
struct TableKind { rc::ReadKind kind; const char *who, *row, *wrap; };
static const TableKind TRACE_KIND = {rc::RK_TRACE, "rc_trace_frames", ": out holds fewer than n * (4 + k) cells",
                                     ": a column could pass 2^63 - 1 (largest weight * largest value * set pixels a frame can hold)"};
static const TableKind CORR_KIND = {rc::RK_CORR, "rc_corr_frames", ": out holds fewer than n * (2 R + 1)^2 cells",
                                    ": a cell could pass 2^63 - 1 (largest |reference| * largest value * set pixels a frame can hold)"};
static const TableKind BINS_KIND = {rc::RK_BINS, "rc_bins_frames", ": out holds fewer than n * 2 * n_bins cells", nullptr};

// Create, for every kind: `check` judges the kind's own arguments before the device is asked for (nullptr, or the refusal's text); `fill`
// queues on `s` whatever brings the caller's data into t->plane and returns the first HIP error.  What it needs on the side it takes from
// `tmp`, which is given back here, behind the wait - a fill may return wherever it fails.  plane_bytes 0: a handle without a plane.
#define HIP_PASS(expr) do { const hipError_t e_ = (expr); if (e_ != hipSuccess) return e_; } while (0)
struct TableTemps {
    std::vector<void *> held;
    template <class P> hipError_t alloc(P **p, size_t bytes)
    {
        HIP_PASS(hipMalloc(reinterpret_cast<void **>(p), bytes));
        held.push_back(*p);
        return hipSuccess;
    }
};
template <class T, class Check, class Fill>
static T *table_create(const char *who, uint32_t nx, uint32_t ny, uint32_t param, uint64_t row_cells, uint64_t plane_bytes, int *status, Check check, Fill fill)
{
    auto done = [&](int code) { if (status) *status = code; return (T *)nullptr; };
    const std::string name(who);
    if (nx == 0 || ny == 0 || nx > 65535u || ny > 65535u) return done(fail(RC_ERR_BAD_ARG, (name + ": nx, ny in 1..65535").c_str()));
    if (const char *refusal = check()) return done(fail(RC_ERR_BAD_ARG, refusal));
    UtilScope util_scope;
    int r = util_scope.enter();
    if (r != RC_OK) return done(r);
    T *t = new (std::nothrow) T;
    if (!t) return done(fail(RC_ERR_WORKSPACE, (name + ": out of host memory").c_str()));
    t->device = g_util.device; t->nx = nx; t->ny = ny; t->param = param; t->row_cells = row_cells;
    if (plane_bytes) {
        TableTemps tmp;
        hipStream_t s = g_util.stream;
        hipError_t e = hipMalloc(&t->plane, plane_bytes);
        if (e == hipSuccess) e = fill(t, tmp, s);
        // (also after an error: copies and kernels queued before it may still read `tmp`'s memory and the caller's)
        const hipError_t e_sync = hipStreamSynchronize(s);
        if (e == hipSuccess) e = e_sync;
        for (void *p : tmp.held) (void)hipFree(p);
        if (e != hipSuccess) {
            r = hip_fail(e, who);
            if (t->plane) (void)hipFree(t->plane);
            delete t;
            return done(r);
        }
    }
    if (status) *status = RC_OK;
    return t;
}
template <class T>
static int table_destroy(T *t)
{
    if (!t) return RC_OK;
    RC_ON_DEVICE(t->device);
    // (a batch still queued on a slot reads the plane: both slots' streams and the synchronous call's are waited for)
    (void)hipDeviceSynchronize();
    if (t->plane) (void)hipFree(t->plane);
    delete t;
    return RC_OK;
}

// what both forms check before the device is asked for: from the arguments alone.  fits: the kind's no-wrap rule, asked last
template <class Fits>
static int table_admit(const TableKind &K, const FrameTable *t, const ReadFrames &in, const void *out, uint64_t out_cells, Fits fits)
{
    auto refuse = [&](int code, const char *what) { return fail(code, (std::string(K.who) + what).c_str()); };
    if (!t || !in.data || !in.sizes || !out || in.n == 0) return refuse(RC_ERR_BAD_ARG, ": NULL / zero argument");
    if (in.level < 1 || in.level > 3) return fail(RC_ERR_UNSUPPORTED, "rc_expand_frames: reduction level 1, 2 or 3");
    if (in.level == 1 && in.bit_depth == 0) return fail(RC_ERR_BAD_ARG, "bit_depth must be 1..64");
    if (in.level == 1 && in.bit_depth > 16) return refuse(RC_ERR_UNSUPPORTED, ": bit_depth above 16 (as for the summed views)");
    if ((uintptr_t)out % 8) return refuse(RC_ERR_BAD_ARG, ": out must be aligned to its int64 cells");
    if (out_cells < (uint64_t)in.n * t->row_cells) return refuse(RC_ERR_OUT_TOO_SMALL, K.row);
    // the frame shape is the handle's; stored streams (op_mode 0) show another one on their face - compressed ones when they decode (RC_ERR_CORRUPT)
    const uint64_t nb = ((uint64_t)t->nx * t->ny + 7) / 8;
    for (uint32_t f = 0; f < in.n && in.op_mode == 0; ++f)
        if (in.sizes[3 * f] != nb) return refuse(RC_ERR_BAD_ARG, ": the frames' geometry differs from the handle's");
    return fits() ? RC_OK : refuse(RC_ERR_OUT_TOO_SMALL, K.wrap);
}
template <class Fits>
static int table_run(const TableKind &K, FrameTable *t, const uint32_t *slot, ReadRequest q, Fits fits)      // (q.kind, q.in.nx, ny and q.table: filled in here)
{
    if (slot && *slot >= RC_READ_SLOTS) return fail(RC_ERR_BAD_ARG, (std::string(K.who) + "_submit: slot 0 or 1").c_str());
    int r = table_admit(K, t, q.in, q.out, q.cap, fits);
    if (r == RC_OK) r = handle_on_current_device(t->device, K.who);
    if (r != RC_OK) return r;
    q.kind = K.kind; q.in.nx = t->nx; q.in.ny = t->ny; q.table = {t->plane, t->param, t->row_cells};
    return expand_run(q, slot);
}

// ---- frame traces ---------------------------------------------------------------------------------------------------------------------------
RC_EXPORT rc_trace *rc_trace_create(uint32_t nx, uint32_t ny, uint32_t k, const int32_t *planes, int *status)
{
    using namespace rc;
    const uint64_t N = (uint64_t)nx * ny;
    const uint32_t kp = trace_padded_planes(k);
    auto check = [&]() -> const char * {
        if (k > TRACE_MAX_PLANES) return "rc_trace_create: at most 16 weight planes";
        return k && !planes ? "rc_trace_create: planes is NULL with k > 0" : nullptr;
    };
    auto fill = [&](rc_trace *t, TableTemps &tmp, hipStream_t s) -> hipError_t {
        int32_t *weights = static_cast<int32_t *>(t->plane);
        const bool on_device = is_device_ptr(planes);
        int32_t *stage = nullptr;          // one plane of a host caller's, on its way into the interleaved copy
        uint32_t *d_bound = nullptr;       // maxabs of a device caller's planes
        HIP_PASS(hipMemsetAsync(weights, 0, N * kp * 4, s));
        if (!on_device) HIP_PASS(tmp.alloc(&stage, N * 4));
        else {
            HIP_PASS(tmp.alloc(&d_bound, TRACE_MAX_PLANES * 4));
            HIP_PASS(hipMemsetAsync(d_bound, 0, TRACE_MAX_PLANES * 4, s));
        }
        for (uint32_t m = 0; m < k; ++m) {
            const int32_t *plane = planes + (uint64_t)m * N;
            if (on_device) launch_trace_maxabs(plane, N, d_bound + m, s);
            else {
                uint32_t a = 0;
                for (uint64_t p = 0; p < N; ++p) a = std::max(a, trace_abs(plane[p]));
                t->bound[m] = a;
                HIP_PASS(hipMemcpyAsync(stage, plane, N * 4, hipMemcpyHostToDevice, s));      // (`stage` is reused per plane: the stream orders copy and kernel)
                plane = stage;
            }
            launch_trace_interleave(plane, N, m, kp, weights, s);
            HIP_PASS(hipGetLastError());
        }
        return on_device ? hipMemcpyAsync(t->bound, d_bound, k * 4, hipMemcpyDeviceToHost, s) : hipSuccess;
    };
    return table_create<rc_trace>("rc_trace_create", nx, ny, k, TRACE_MOMENTS + k, N * kp * 4, status, check, fill);      // (k = 0: no plane)
}
RC_EXPORT int rc_trace_destroy(rc_trace *t) { return table_destroy(t); }
RC_EXPORT uint32_t rc_trace_columns(const rc_trace *t) { return t ? (uint32_t)t->row_cells : 0; }
RC_EXPORT uint32_t rc_trace_weight_bound(const rc_trace *t, uint32_t m) { return t && m < t->param ? t->bound[m] : 0; }
static int trace_run(rc_trace *t, const uint32_t *slot, const ReadRequest &q)
{
    return table_run(TRACE_KIND, t, slot, q,
                     [&] { return rc::trace_batch_fits(t->nx, t->ny, q.in.level, q.in.bit_depth, t->param, t->bound, q.in.sizes, q.in.n); });
}
RC_EXPORT int rc_trace_frames(rc_trace *t, uint32_t bit_depth, uint32_t level, uint32_t op_mode, uint32_t scheme, const uint8_t *data, const uint32_t *sizes,
                              uint32_t n, int64_t *out, uint64_t out_cells, uint64_t *nnz_prefix)
{ return trace_run(t, nullptr, {.in = {0, 0, bit_depth, level, op_mode, scheme, data, sizes, n}, .nnz_prefix = nnz_prefix, .out = out, .cap = out_cells}); }
RC_EXPORT int rc_trace_frames_submit(rc_trace *t, uint32_t slot, uint32_t bit_depth, uint32_t level, uint32_t op_mode, uint32_t scheme, const uint8_t *data,
                                     const uint32_t *sizes, uint32_t n, int64_t *out, uint64_t out_cells)
{ return trace_run(t, &slot, {.in = {0, 0, bit_depth, level, op_mode, scheme, data, sizes, n}, .out = out, .cap = out_cells}); }

// ---- correlation surfaces -------------------------------------------------------------------------------------------------------------------
RC_EXPORT rc_corr *rc_corr_create(uint32_t nx, uint32_t ny, uint32_t radius, const int32_t *reference, int *status)
{
    using namespace rc;
    auto check = [&]() -> const char * {
        if (radius > CORR_MAX_RADIUS) return "rc_corr_create: radius at most 16";
        return reference ? nullptr : "rc_corr_create: reference is NULL";
    };
    auto fill = [&](rc_corr *c, TableTemps &tmp, hipStream_t s) -> hipError_t {
        int32_t *padded = static_cast<int32_t *>(c->plane);
        const uint64_t N = (uint64_t)nx * ny;
        const uint32_t nxp = corr_padded_nx(nx, radius);
        const bool on_device = is_device_ptr(reference);
        uint32_t *d_bound = nullptr;       // maxabs of a device caller's reference
        HIP_PASS(hipMemsetAsync(padded, 0, corr_padded_cells(nx, ny, radius) * 4, s));
        if (on_device) {
            HIP_PASS(tmp.alloc(&d_bound, 4));
            HIP_PASS(hipMemsetAsync(d_bound, 0, 4, s));
            launch_trace_maxabs(reference, N, d_bound, s);
            HIP_PASS(hipGetLastError());
            HIP_PASS(hipMemcpyAsync(&c->bound, d_bound, 4, hipMemcpyDeviceToHost, s));
        } else
            for (uint64_t p = 0; p < N; ++p) c->bound = std::max(c->bound, trace_abs(reference[p]));
        // the image's rows into the middle of the border (row r of T starts at padded (r + R, R))
        return hipMemcpy2DAsync(padded + (uint64_t)radius * nxp + radius, (size_t)nxp * 4, reference, (size_t)nx * 4, (size_t)nx * 4, ny,
                                on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s);
    };
    return table_create<rc_corr>("rc_corr_create", nx, ny, radius, corr_cells(radius), corr_padded_cells(nx, ny, radius) * 4, status, check, fill);
}
RC_EXPORT int rc_corr_destroy(rc_corr *c) { return table_destroy(c); }
RC_EXPORT uint32_t rc_corr_side(const rc_corr *c) { return c ? rc::corr_side(c->param) : 0; }
RC_EXPORT uint32_t rc_corr_reference_bound(const rc_corr *c) { return c ? c->bound : 0; }
static int corr_run(rc_corr *c, const uint32_t *slot, const ReadRequest &q)
{
    return table_run(CORR_KIND, c, slot, q, [&] { return rc::corr_batch_fits(c->nx, c->ny, q.in.level, q.in.bit_depth, c->bound, q.in.sizes, q.in.n); });
}
RC_EXPORT int rc_corr_frames(rc_corr *c, uint32_t bit_depth, uint32_t level, uint32_t op_mode, uint32_t scheme, const uint8_t *data, const uint32_t *sizes,
                             uint32_t n, int64_t *out, uint64_t out_cells, uint64_t *nnz_prefix)
{ return corr_run(c, nullptr, {.in = {0, 0, bit_depth, level, op_mode, scheme, data, sizes, n}, .nnz_prefix = nnz_prefix, .out = out, .cap = out_cells}); }
RC_EXPORT int rc_corr_frames_submit(rc_corr *c, uint32_t slot, uint32_t bit_depth, uint32_t level, uint32_t op_mode, uint32_t scheme, const uint8_t *data,
                                    const uint32_t *sizes, uint32_t n, int64_t *out, uint64_t out_cells)
{ return corr_run(c, &slot, {.in = {0, 0, bit_depth, level, op_mode, scheme, data, sizes, n}, .out = out, .cap = out_cells}); }

// ---- binned frame traces --------------------------------------------------------------------------------------------------------------------
RC_EXPORT rc_bins *rc_bins_create(uint32_t nx, uint32_t ny, uint32_t n_bins, const uint16_t *labels, int *status)
{
    using namespace rc;
    static const char *const range = "rc_bins_create: a label at or above n_bins that is not 0xFFFF";
    const uint64_t N = (uint64_t)nx * ny;
    bool on_device = false;
    uint32_t top = 0;      // the largest label of a device caller's map: known behind create's wait
    auto check = [&]() -> const char * {
        if (n_bins == 0 || n_bins > BINS_MAX) return "rc_bins_create: n_bins in 1..4096";
        if (!labels) return "rc_bins_create: labels is NULL";
        // (without a GPU no pointer is a device pointer: host labels are judged before the device is asked for)
        on_device = is_device_ptr(labels);
        for (uint64_t p = 0; p < N && !on_device; ++p)
            if (labels[p] >= n_bins && labels[p] != BINS_IGNORE) return range;
        return nullptr;
    };
    auto fill = [&](rc_bins *b, TableTemps &tmp, hipStream_t s) -> hipError_t {
        uint32_t *d_top = nullptr;
        if (on_device) {
            HIP_PASS(tmp.alloc(&d_top, 4));
            HIP_PASS(hipMemsetAsync(d_top, 0, 4, s));
            launch_bins_label_max(labels, N, d_top, s);
            HIP_PASS(hipGetLastError());
            HIP_PASS(hipMemcpyAsync(&top, d_top, 4, hipMemcpyDeviceToHost, s));
        }
        return hipMemcpyAsync(b->plane, labels, N * 2, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s);
    };
    rc_bins *b = table_create<rc_bins>("rc_bins_create", nx, ny, n_bins, (uint64_t)BINS_PLANES * n_bins, N * 2, status, check, fill);
    if (b && top >= n_bins) {      // device labels are judged here: the handle goes the way every handle goes
        (void)table_destroy(b);
        b = nullptr;
        if (status) *status = fail(RC_ERR_BAD_ARG, range);
    }
    return b;
}
RC_EXPORT int rc_bins_destroy(rc_bins *b) { return table_destroy(b); }
RC_EXPORT uint32_t rc_bins_count(const rc_bins *b) { return b ? b->param : 0; }
static int bins_run(rc_bins *b, const uint32_t *slot, const ReadRequest &q) { return table_run(BINS_KIND, b, slot, q, [] { return true; }); }
RC_EXPORT int rc_bins_frames(rc_bins *b, uint32_t bit_depth, uint32_t level, uint32_t op_mode, uint32_t scheme, const uint8_t *data, const uint32_t *sizes,
                             uint32_t n, int64_t *out, uint64_t out_cells, uint64_t *nnz_prefix)
{ return bins_run(b, nullptr, {.in = {0, 0, bit_depth, level, op_mode, scheme, data, sizes, n}, .nnz_prefix = nnz_prefix, .out = out, .cap = out_cells}); }
RC_EXPORT int rc_bins_frames_submit(rc_bins *b, uint32_t slot, uint32_t bit_depth, uint32_t level, uint32_t op_mode, uint32_t scheme, const uint8_t *data,
                                    const uint32_t *sizes, uint32_t n, int64_t *out, uint64_t out_cells)
{ return bins_run(b, &slot, {.in = {0, 0, bit_depth, level, op_mode, scheme, data, sizes, n}, .out = out, .cap = out_cells}); }
