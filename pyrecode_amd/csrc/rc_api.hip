// rc_api.hip - the C ABI of librecode_hip.so (include/recode_hip.h): contexts, staging, entry points.
// No CPU implementation lives here: every compute entry point runs HIP kernels or returns RC_ERR_DEVICE.
#include "rc_host.h"
#include "rc_deflate_model.h"

thread_local std::string g_last_error;
WorkerPool *g_pool = new WorkerPool;
Util g_utils[RC_MAX_DEV];
thread_local Util *t_util = nullptr;


struct rc_ctx {
    int device = 0;
    hipStream_t own_stream = nullptr, stream = nullptr;
    uint32_t nx = 0, ny = 0, depth = 0, level = 0, op_mode = 0, scheme = 0, clevel = 0, max_batch = 0;
    uint32_t emit = rc::EMIT_RAW;
    // Per-batch scratch exists twice: batch i reduces into sets[i & 1] on `stream`; its scans / layout / assembly (small,
    // latency-bound kernels that leave most of the GPU idle) run on `pstream` and may overlap the next batch's reduce
    // kernel (rc_ctx_set_pipelined).  Geometry, threshold and fitted model are the same in both.
    rc::Scratch sets[2];
    int cur = 0;                          // set the NEXT batch uses
    int last = 0;                         // set of the most recent batch
    const rc::Scratch &geo() const { return sets[0]; }       // N, ntiles, nb, nb_stride, thr
    const rc::Scratch &recent() const { return sets[last]; } // the most recent batch's status word and binary maps
    // Every device and page-locked allocation of the ctx - scratch sets, pipe slots, staging - is on one of these lists (rc_host.h);
    // model_mem: the value stage's scratch of each set, which rc_ctx_set_source_bytes(ctx, 4) gives back.
    DevMem dmem, model_mem[2];
    PinMem hmem;
    hipStream_t pstream = nullptr;        // carries everything behind the reduce kernel
    hipStream_t pstream_b = nullptr;      // two chains (pipelined, level 2): the second stage of the batches on scratch set 1
    hipStream_t last_ps = nullptr;        // the stream the most recent batch's second stage went to
    bool two_chains = false;
    hipEvent_t ev_red[2] = {}, ev_post[2] = {}, ev_in[2] = {};
    bool post_pending[2] = {false, false};
    bool pipelined = false;
    bool thr_set = false;
    bool keep_bitmap = true;  // also store the raw binary maps when a device codec is active (rc_get_binary_map)
    uint32_t src_bytes = 2;   // bytes per source pixel: 2 (uint16 frames and dark), 1 (uint8) or 4 (uint32): rc_ctx_set_source_bytes
    uint32_t *thr32 = nullptr;   // uint32 sources: the threshold frame (geo().thr is the uint16 one)
    uint32_t last_n = 0;
    // staging for host callers
    DevBuf d_frames, d_out, d_dark;
    uint64_t *d_rec_off = nullptr;
    uint32_t *d_md = nullptr;
    void *d_ztab = nullptr;               // zstd FSE tables (EMIT_ZSTD)
    // the value stage (rc_launch.h): its format, set by rc_ctx_create (uint32 sources: none); values_on: the fitted table pays (else the stream stays stored)
    rc::ValueStage values = rc::VALUES_NONE;
    bool values_on = false;
    // tables fitted to a sample of the ctx's first batch (fit_value_model): modelled zstd (compression_level >= 1, every reduction level:
    // rc_zstd_model.h) and the DEFLATE value stage's (rc_deflate_model.h, with the sample's byte histogram)
    bool modelled = false, model_ready = false;
    rc::ZstdModel *d_model = nullptr, *h_model = nullptr;
    rc::ZstdSample *d_sample = nullptr, *h_sample = nullptr;
    rc::DeflateModel *d_dzm = nullptr, *h_dzm = nullptr;
    uint32_t *d_dzhist = nullptr, *h_dzhist = nullptr;
    uint32_t l2_sum = 0;                  // L2_statistics: 0/1 max, 2 sum
    rc::u32x2 *d_l2_node[2] = {};         // level 2: the labelling stage's nodes (rc_l2.hip) - one workspace per chain of second stages
    uint16_t *d_l2_base[2] = {};          // ... and its directory of rank bases
    rc::BatchStatus *h_status = nullptr;  // pinned: [0] most recent batch, [1] first failed batch since the last sync
    rc::BatchStatus *d_first_err = nullptr;
    uint32_t batch_seq = 0;               // batches enqueued since the last rc_ctx_sync
    // the previous batch's output buffers (two chains: a caller that hands consecutive batches the SAME buffers is serialised, see enqueue_batch)
    const uint8_t *prev_out = nullptr, *prev_rec = nullptr, *prev_md = nullptr;
    uint64_t prev_out_cap = 0;
    uint32_t prev_n = 0;
    hipEvent_t ev[5] = {};
    float stage_ms[5] = {};
    // optional per-enqueue stage events for the asynchronous path (rc_ctx_set_profiling)
    bool profiling = false;
    uint32_t prof_every = 1, prof_phase = 0;   // events around every prof_every-th batch (rc_ctx_set_profiling(ctx, k))
    bool profile_all = getenv("RC_PROFILE_ALL_STAGES") != nullptr;
    // host streaming form (rc_pipe_*): per slot device buffers, pinned metadata, events
    struct PipeSlot {
        uint8_t *d_in = nullptr;
        uint8_t *d_out = nullptr;
        uint64_t *d_rec = nullptr, *h_rec = nullptr;
        uint32_t *d_md = nullptr, *h_md = nullptr;
        rc::BatchStatus *h_stat = nullptr;
        hipEvent_t ev_h2d = nullptr, ev_done = nullptr, ev_fetch = nullptr, ev_val = nullptr;
        uint32_t *d_val = nullptr, *h_val = nullptr;   // validation frames: component counts of the ROI (0xFFFFFFFF: not a validation frame)
        bool has_val = false;
        uint32_t n = 0;
        bool zero_copy = false;
        enum State { FREE, SUBMITTED, RESULT_TAKEN, FETCHING } state = FREE;
    } pipe[RC_PIPE_SLOTS];
    hipStream_t copy_stream = nullptr, d2h_stream = nullptr;
    uint32_t val_gap = 0, val_x0 = 0, val_y0 = 0, val_w = 0, val_h = 0;   // rc_ctx_set_validation
    std::vector<hipEvent_t> prof_ev;   // 5 events per enqueued batch, in enqueue order
    size_t prof_used = 0;              // events consumed since the last rc_ctx_sync
    double prof_sum_ms[5] = {};
    uint64_t prof_batches = 0;
};

// ---- library ---------------------------------------------------------------------------------------------
RC_EXPORT int rc_abi_version(void) { return RC_ABI_VERSION; }

RC_EXPORT const char *rc_strerror(int status)
{
    switch (status) {
    case RC_OK: return "ok";
    case RC_ERR_BAD_ARG: return "bad argument";
    case RC_ERR_OUT_TOO_SMALL: return "output buffer too small";
    case RC_ERR_DEVICE: return "GPU / HIP error";
    case RC_ERR_UNSUPPORTED: return "not implemented on device";
    case RC_ERR_RECORD_TOO_LARGE: return "Buffer size smaller than compressed data size";
    case RC_ERR_CORRUPT: return "corrupt input stream";
    case RC_ERR_WORKSPACE: return "out of device memory for the ctx's workspace";
    default: return "unknown status";
    }
}
RC_EXPORT const char *rc_last_error(void) { return g_last_error.c_str(); }

RC_EXPORT int rc_device_count(int *count)
{
    if (!count) return fail(RC_ERR_BAD_ARG, "count is NULL");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        n = 0;
    }
    *count = n;
    return RC_OK;
}
RC_EXPORT int rc_scheme_on_device(uint32_t scheme)
{
    return (scheme == RC_SCHEME_LZ4 || scheme == RC_SCHEME_ZSTD || scheme == RC_SCHEME_BLOSC_LZ4 || scheme == RC_SCHEME_ZLIB_DEVICE) ? 1 : 0;
}

// ---- seam 1 --------------------------------------------------------------------------------------------------
static int alloc_set(rc_ctx *c, rc::Scratch &sc, DevMem &model_mem)
{
    using namespace rc;
    DevMem &m = c->dmem;
    const uint64_t B = c->max_batch, T = sc.ntiles;
    RC_ALLOC(m, sc.bitmap, B * sc.nb_stride + 64);  // + slack: k_gather reads whole 16-byte pieces
    RC_ALLOC(m, sc.tile_cnt, B * T * 4);
    RC_ALLOC(m, sc.tile_off, B * T * 4);
    RC_ALLOC(m, sc.tile_next, B * T * 4);
    RC_ALLOC(m, sc.frame_nnz, B * 4);
    RC_ALLOC(m, sc.frame_cbytes, B * 4);
    RC_ALLOC(m, sc.scan_part, B * ((T + 255) / 256) * 32);   // (a row of partials per scan segment: room for segments of 256 tiles, more rows than k_scan_seg's 4096-tile ones need)
    RC_ALLOC(m, sc.status, sizeof(BatchStatus));
    if (c->level != 3) RC_ALLOC(m, sc.pix_slots, B * T * TILE_PX * 2 + 64);
    if (c->emit != EMIT_RAW) {
        if (c->level == 1) {   // combined slots (rc_launch.h, Scratch::comb; profiles/r04_ab_combined_slots.log)
            sc.comb = c->emit == EMIT_ZSTD ? COMB_AT_BLK_SLOT : COMB_BEHIND_BLOCK;
            sc.blk_stride = 1536;                                  // 12 lines: the block image (<= 5) + 7 or more lines of residuals
        }
        RC_ALLOC(m, sc.blk_slots, B * T * (uint64_t)sc.blk_stride + 256);
        RC_ALLOC(m, sc.blk_size, B * T * 4);
        RC_ALLOC(m, sc.blk_off, B * T * 4);
        if (c->emit == EMIT_DEFLATE) {   // the zlib streams' Adler-32: per-tile partials of the map, per-frame sums (rc_deflate_block.h, k_gather)
            RC_ALLOC(m, sc.blk_aux, B * T * 4);
            RC_ALLOC(m, sc.zl_acc, B * 32);
            HIP_TRY(hipMemset(sc.zl_acc, 0, B * 32));
        }
    }
    if (c->values != VALUES_NONE) {   // the value stage's scratch (free_value_stage gives it back)
        const ValueGeom g = value_geom(c->values);
        sc.pixraw_stride = ((sc.N * 2 + 15) & ~15ull) + 32;
        sc.nchunk_max = (uint32_t)((sc.N * 2 + g.chunk - 1) / g.chunk) + 1;
        RC_ALLOC(model_mem, sc.pixraw, B * sc.pixraw_stride + 64);
        RC_ALLOC(model_mem, sc.pix_chunks, B * (uint64_t)sc.nchunk_max * g.slot + 64);
        if (c->values == VALUES_DEFLATE_HUFF) RC_ALLOC(model_mem, sc.chunk_aux, B * (uint64_t)(sc.nchunk_max + 1) * 8);
        RC_ALLOC(model_mem, sc.chunk_size, B * (uint64_t)sc.nchunk_max * 4);
        RC_ALLOC(model_mem, sc.chunk_off, B * (uint64_t)sc.nchunk_max * 4);
        RC_ALLOC(model_mem, sc.frame_pbytes, B * 4);
        HIP_TRY(hipMemset(sc.frame_pbytes, 0, B * 4));
    }
    HIP_TRY(hipMemset(sc.frame_nnz, 0, B * 4));
    HIP_TRY(hipMemset(sc.frame_cbytes, 0, B * 4));
    HIP_TRY(hipMemset(sc.status, 0, sizeof(BatchStatus)));
    return RC_OK;
}

// uint32 sources have no value stage: its scratch (alloc_set sized it for uint16 sources) goes back, every field of it is cleared
static void free_value_stage(rc_ctx *c)
{
    c->values = rc::VALUES_NONE;
    c->values_on = false;
    for (int k = 0; k < 2; ++k) {
        rc::Scratch &set = c->sets[k];
        c->model_mem[k].release_all();
        set.pixraw = nullptr; set.pix_chunks = nullptr; set.chunk_aux = nullptr; set.chunk_size = nullptr; set.chunk_off = nullptr;
        set.frame_pbytes = nullptr; set.pixraw_stride = 0; set.nchunk_max = 0;
    }
}

static int ctx_alloc(rc_ctx *c)
{
    using namespace rc;
    const uint64_t B = c->max_batch;
    RC_ON_DEVICE(c->device);
    HIP_TRY(hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking));
    // The second-stage stream: a plain one.  Measured and not adopted (same-box A/B):
    //  - a high-priority stream: no gain with LZ4 or zstd, 2 % slower at 11520x8184 (profiles/r05_exp32_second_stage_stream_priority_no_effect.log);
    //  - the second stage confined to the first n CUs (a CU-masked stream), so that its waves (80 VGPRs, latency bound) stop pushing out
    //    one of the three reduce waves on every SIMD: LZ4 123.7 k -> 126.2 k frames/s with n = 104, but zstd, whose second stage also
    //    carries the FSE kernel, 112 k -> 103 k; the reduce kernel on the remaining CUs besides: slower still (profiles/r04_ab_cu_partition.log).
    HIP_TRY(hipStreamCreateWithFlags(&c->pstream, hipStreamNonBlocking));
    {
        // (the second chain's stream: created at another priority so that it gets a hardware queue of its own - a plain third stream shared
        // the reduce stream's queue on the default four and cost every configuration 10 %, profiles/r05_exp23_two_chains_shared_queue.log)
        int lo = 0, hi = 0;
        HIP_TRY(hipDeviceGetStreamPriorityRange(&lo, &hi));
        HIP_TRY(hipStreamCreateWithPriority(&c->pstream_b, hipStreamNonBlocking, hi));
    }
    c->last_ps = c->pstream;
    c->stream = c->own_stream;
    DevMem &m = c->dmem;
    int r;
    RC_ALLOC(m, c->sets[0].thr, c->geo().N * 2);
    RC_ALLOC(m, c->d_first_err, sizeof(BatchStatus));
    HIP_TRY(hipMemset(c->d_first_err, 0, sizeof(BatchStatus)));
    c->sets[0].first_err = c->d_first_err;
    c->sets[1] = c->sets[0];  // geometry + the shared threshold
    for (int k = 0; k < 2; ++k)
        if ((r = alloc_set(c, c->sets[k], c->model_mem[k])) != RC_OK) return r;
    // Two chains (level 2): the second stage of a level-2 batch - directory, links, statistics, emit, then the level-1 stages - is a chain of
    // latency-bound kernels about as long as the reduce kernel itself; on ONE stream it paces the batches (step 0.70 ms against a reduce kernel
    // of 0.58).  The batches on scratch set 1 take a second stream and a second workspace (nodes + directory), so two consecutive
    // batches' chains overlap each other as well as the reduce kernels: +4 % at 1 % of the pixels set, +9 % on clustered events, nothing for
    // level 1 whose chain is a quarter of its reduce kernel (profiles/r05_exp24_two_chains.log).  Batches still COMPLETE in order.
    c->two_chains = false;   // (the second chain's workspace comes with the first rc_ctx_set_pipelined(ctx, 1): l2_second_chain)
    if (c->level == 2) {
        // level 2 (rc_l2.hip): a node {parent, accumulator} for every pixel of a batch (8 bytes each: 8.6 GB for 64 frames of 4096^2, of
        // which only the entries of set pixels with neighbours are ever touched), at rest - zero - between batches, and the directory of
        // rank bases (2 bytes per 64 pixels) - sized by the geometry, so no batch can exceed it.  One workspace per chain: a ctx that is
        // never pipelined has one chain and one workspace.
        const uint64_t ids = (uint64_t)c->geo().ntiles * rc::TILE_PX;
        RC_ALLOC(m, c->d_l2_node[0], B * ids * 8);
        HIP_TRY(hipMemset(c->d_l2_node[0], 0, B * ids * 8));
        RC_ALLOC(m, c->d_l2_base[0], B * (uint64_t)c->geo().ntiles * 64 * 2);   // (written by k_l2_dir before anything reads it)
        for (int i = 0; i < 2; ++i) {
            Scratch &set = c->sets[i];
            set.l2_node = c->d_l2_node[0]; set.l2_ids_per_frame = ids; set.l2_base = c->d_l2_base[0];
        }
    }
    if (c->emit == EMIT_ZSTD) {
        if ((r = zstd_encoder_tables(m, c->d_ztab)) != RC_OK) return r;
        // compression_level 0 = the fast encoder (raw literals, predefined tables, stored residuals); any other level = the
        // modelled one.  (The reference hands the level to libzstd, recode_writer.py:175-178; the device encoders have these two.)
        c->modelled = c->clevel != 0;
        if (c->modelled) {
            RC_ALLOC(m, c->d_model, sizeof(ZstdModel));
            RC_ALLOC(m, c->d_sample, sizeof(ZstdSample));
            RC_ALLOC(c->hmem, c->h_model, sizeof(ZstdModel));
            RC_ALLOC(c->hmem, c->h_sample, sizeof(ZstdSample));
        }
    }
    if (c->values == VALUES_DEFLATE_HUFF) {
        RC_ALLOC(m, c->d_dzm, sizeof(DeflateModel));
        RC_ALLOC(m, c->d_dzhist, 256 * 4);
        RC_ALLOC(c->hmem, c->h_dzm, sizeof(DeflateModel));
        RC_ALLOC(c->hmem, c->h_dzhist, 256 * 4);
    }
    RC_ALLOC(m, c->d_rec_off, (B + 1) * 8);
    RC_ALLOC(m, c->d_md, B * 3 * 4);
    RC_ALLOC(c->hmem, c->h_status, 2 * sizeof(BatchStatus));
    for (auto &e : c->ev) HIP_TRY(hipEventCreate(&e));
    for (auto &e : c->ev_red) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    for (auto &e : c->ev_post) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    for (auto &e : c->ev_in) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    return RC_OK;
}

RC_EXPORT rc_ctx *rc_ctx_create(uint32_t nx, uint32_t ny, uint32_t src_bit_depth, uint32_t reduction_level,
                                uint32_t op_mode, uint32_t scheme, uint32_t clevel, int device_id, uint32_t max_batch,
                                int *status)
{
    int dummy;
    if (!status) status = &dummy;
    *status = RC_OK;
    if (nx == 0 || ny == 0 || max_batch == 0 || max_batch > 65535u || op_mode > 1) {   // (a batch's frames are a launch's grid.y)
        *status = fail(RC_ERR_BAD_ARG, "nx, ny, max_batch must be > 0, max_batch <= 65535 and op_mode 0 or 1");
        return nullptr;
    }
    if ((uint64_t)nx * ny >= (1ull << 32)) {
        *status = fail(RC_ERR_BAD_ARG, "nx*ny must be < 2^32");
        return nullptr;
    }
    // A record may be as large as its raw frame (recode_writer.py:565-566), the format keeps every size of a record in a u32 metadata field
    // (structures.py:18-46) and k_gather places bytes at u32 offsets inside a record: a raw frame of 4 GiB or more cannot be represented
    // (uint16 sources: nx * ny < 2^31, e.g. 46 340^2; the reference's own C type holds nx, ny in 16 bits each, pyrecode.cpp:21-22, which
    // would allow 65 535^2).  rc_ctx_set_source_bytes checks again for the pixel size it is given.
    if ((uint64_t)nx * ny * 2 >= (1ull << 32)) {
        *status = fail(RC_ERR_UNSUPPORTED, "a raw frame of 4 GiB or more (nx*ny*bytes_per_pixel >= 2^32) does not fit the format's u32 size fields");
        return nullptr;
    }
    if (reduction_level < 1 || reduction_level > 3) {
        *status = fail(RC_ERR_UNSUPPORTED, "reduction_level 4 (centroiding) is not implemented on device");
        return nullptr;
    }
    if (reduction_level == 2 && nx > 65535u) {   // (the reference's C type holds nx in 16 bits, pyrecode.cpp:21-22; the labelling stage is tested up to there)
        *status = fail(RC_ERR_UNSUPPORTED, "reduction_level 2 needs nx <= 65535");
        return nullptr;
    }
    if (src_bit_depth < 1 || src_bit_depth > 32) {   // (<= 8: the reference's source dtype is uint8, > 16: uint32 - rc_ctx_set_source_bytes)
        *status = fail(RC_ERR_UNSUPPORTED, "source_bit_depth must be 1..32 (uint8 / uint16 / uint32 source frames)");
        return nullptr;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device_id < 0 || device_id >= ndev) {
        (void)hipGetLastError();
        *status = fail(RC_ERR_DEVICE, "no such HIP device (this library has no CPU path)");
        return nullptr;
    }
    rc_ctx *c = new (std::nothrow) rc_ctx();
    if (!c) {
        *status = fail(RC_ERR_DEVICE, "out of host memory");
        return nullptr;
    }
    c->device = device_id;
    c->nx = nx; c->ny = ny; c->depth = src_bit_depth; c->level = reduction_level; c->op_mode = op_mode;
    c->scheme = scheme; c->clevel = clevel; c->max_batch = max_batch;
    c->emit = (op_mode == 1 && rc_scheme_on_device(scheme)) ? scheme : rc::EMIT_RAW;
    c->values = rc::value_stage_of(c->emit, clevel, reduction_level);
    rc::Scratch &sc = c->sets[0];   // (ctx_alloc copies the geometry to the other set)
    sc.N = (uint64_t)nx * ny;
    sc.ntiles = (uint32_t)((sc.N + rc::TILE_PX - 1) / rc::TILE_PX);
    sc.nb = (sc.N + 7) / 8;
    sc.nb_stride = (uint64_t)sc.ntiles * rc::TILE_BM;
    sc.max_batch = max_batch;
    sc.guarded_loads = getenv("RC_REDUCE_GUARDED_LOADS") != nullptr;   // (tests; read once per ctx)
    int rcode = ctx_alloc(c);
    if (rcode != RC_OK) {
        *status = rcode;
        std::string keep = g_last_error;
        rc_ctx_destroy(c);
        g_last_error = keep;
        return nullptr;
    }
    return c;
}

RC_EXPORT int rc_ctx_destroy(rc_ctx *c)
{
    if (!c) return RC_OK;
    DeviceGuard dev_guard_;
    (void)dev_guard_.enter(c->device);
    for (hipStream_t st : {c->stream, c->pstream, c->pstream_b, c->own_stream, c->copy_stream, c->d2h_stream})
        if (st) (void)hipStreamSynchronize(st);
    c->dmem.release_all();
    for (DevMem &m : c->model_mem) m.release_all();
    c->hmem.release_all();
    for (auto &p : c->pipe)
        for (hipEvent_t e : {p.ev_h2d, p.ev_done, p.ev_fetch, p.ev_val})
            if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : {c->ev_red[0], c->ev_red[1], c->ev_post[0], c->ev_post[1], c->ev_in[0], c->ev_in[1]})
        if (e) (void)hipEventDestroy(e);
    for (auto &e : c->ev)
        if (e) (void)hipEventDestroy(e);
    for (auto &e : c->prof_ev) (void)hipEventDestroy(e);
    for (hipStream_t st : {c->copy_stream, c->d2h_stream, c->pstream, c->pstream_b, c->own_stream})
        if (st) (void)hipStreamDestroy(st);
    delete c;
    return RC_OK;
}

RC_EXPORT int rc_ctx_set_stream(rc_ctx *c, void *hip_stream)
{
    if (!c) return fail(RC_ERR_BAD_ARG, "ctx is NULL");
    c->stream = hip_stream ? reinterpret_cast<hipStream_t>(hip_stream) : c->own_stream;
    return RC_OK;
}

RC_EXPORT int rc_set_threshold(rc_ctx *c, const void *thr)
{
    if (!c || !thr) return fail(RC_ERR_BAD_ARG, "ctx / thr is NULL");
    if (c->depth > 16 && c->src_bytes != 4) return fail(RC_ERR_BAD_ARG, "src_bit_depth > 16 means uint32 sources: rc_ctx_set_source_bytes(ctx, 4) first");
    RC_ON_DEVICE(c->device);
    // (uint16 thresholds for uint16 AND uint8 sources - the device keeps them as uint16 -, uint32 ones for uint32 sources)
    HIP_TRY(hipMemcpyAsync(c->src_bytes == 4 ? (void *)c->thr32 : (void *)c->geo().thr, thr, c->geo().N * (c->src_bytes == 4 ? 4 : 2),
                           is_device_ptr(thr) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice,
                           c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->thr_set = true;
    return RC_OK;
}

RC_EXPORT int rc_set_dark(rc_ctx *c, const void *dark, int64_t epsilon)
{
    if (!c || !dark) return fail(RC_ERR_BAD_ARG, "ctx / dark is NULL");
    RC_ON_DEVICE(c->device);
    const void *src = dark;
    const uint64_t bytes = c->geo().N * c->src_bytes;
    if (!is_device_ptr(dark)) {
        int r = c->d_dark.ensure(c->dmem, bytes);
        if (r != RC_OK) return r;
        HIP_TRY(hipMemcpyAsync(c->d_dark.p, dark, bytes, hipMemcpyHostToDevice, c->stream));
        src = c->d_dark.p;
    }
    if (c->depth > 16 && c->src_bytes != 4) return fail(RC_ERR_BAD_ARG, "src_bit_depth > 16 means uint32 sources: rc_ctx_set_source_bytes(ctx, 4) first");
    if (c->src_bytes == 4) rc::launch_threshold32(static_cast<const uint32_t *>(src), epsilon, c->geo().N, c->thr32, c->stream);
    else rc::launch_threshold(src, epsilon, c->geo().N, c->geo().thr, c->stream, c->src_bytes);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->thr_set = true;
    return RC_OK;
}

// Source pixels of one byte (source_bit_depth <= 8: the reference's map_dtype gives uint8 frames and dark, misc.py:41-49).  Before
// rc_set_dark and the first batch; everything behind the frame loads is the same path (values, packing, codecs, records).
RC_EXPORT int rc_ctx_set_source_bytes(rc_ctx *c, uint32_t bytes_per_pixel)
{
    if (!c) return fail(RC_ERR_BAD_ARG, "ctx is NULL");
    if (bytes_per_pixel != 1 && bytes_per_pixel != 2 && bytes_per_pixel != 4) return fail(RC_ERR_BAD_ARG, "rc_ctx_set_source_bytes: 1 (uint8), 2 (uint16) or 4 (uint32)");
    if (bytes_per_pixel == 1 && c->depth > 8) return fail(RC_ERR_BAD_ARG, "rc_ctx_set_source_bytes: uint8 sources need src_bit_depth <= 8");
    if (bytes_per_pixel == 2 && c->depth > 16) return fail(RC_ERR_BAD_ARG, "rc_ctx_set_source_bytes: uint16 sources need src_bit_depth <= 16");
    if (c->batch_seq || c->thr_set) return fail(RC_ERR_BAD_ARG, "rc_ctx_set_source_bytes: call before rc_set_dark / rc_set_threshold and the first batch");
    if (c->geo().N * bytes_per_pixel >= (1ull << 32))
        return fail(RC_ERR_UNSUPPORTED, "rc_ctx_set_source_bytes: a raw frame of 4 GiB or more (nx*ny*bytes_per_pixel >= 2^32) does not fit the format's u32 size fields");
    if (bytes_per_pixel == 4) {
        // uint32 sources (source_bit_depth > 16, misc.py:41-49): rc_reduce32.hip.  Levels 1 and 3; the residual fields are depth bits wide, or
        // the values' four raw bytes when the depth is a multiple of 8 (`.tobytes()` of a uint32 array, recode_writer.py:463-464: 32 and 24
        // alike); zstd takes the fast encoder (the modelled one is fitted inside the uint16 kernel).
        if (c->depth <= 16) return fail(RC_ERR_BAD_ARG, "rc_ctx_set_source_bytes: uint32 sources are what source_bit_depth > 16 means (misc.py:41-49)");
        if (c->level == 2) return fail(RC_ERR_UNSUPPORTED, "rc_ctx_set_source_bytes: reduction level 2 is not implemented for uint32 sources");
        if (c->emit == rc::EMIT_DEFLATE) return fail(RC_ERR_UNSUPPORTED, "rc_ctx_set_source_bytes: the device DEFLATE encoder is not implemented for uint32 sources (use RC_SCHEME_ZLIB: the host's zlib)");
        RC_ON_DEVICE(c->device);
        // Everything that can fail happens first, into temporaries; the ctx changes only once all of it has succeeded (a failed
        // allocation leaves the uint16 ctx as it was).
        uint32_t *thr32 = nullptr;
        uint16_t *slots[2] = {nullptr, nullptr};
        bool ok = c->dmem.try_alloc(thr32, c->geo().N * 4) == hipSuccess;
        for (int k = 0; ok && k < 2 && c->level != 3; ++k)
            ok = c->dmem.try_alloc(slots[k], (uint64_t)c->max_batch * c->geo().ntiles * rc::TILE_PX * 4 + 64) == hipSuccess;
        if (!ok) {
            (void)hipGetLastError();
            c->dmem.free_one(thr32);
            for (uint16_t *&p : slots) c->dmem.free_one(p);
            return fail(RC_ERR_DEVICE, "rc_ctx_set_source_bytes: out of device memory for the uint32 threshold / residual slots");
        }
        if (c->depth % 8 == 0) c->depth = 32;
        c->modelled = false;
        free_value_stage(c);
        c->thr32 = thr32;
        for (int k = 0; k < 2; ++k) {
            rc::Scratch *set = &c->sets[k];
            set->pix_slot_bytes = rc::TILE_PX * 4;
            set->comb = rc::COMB_OFF;
            if (c->level != 3) {
                c->dmem.free_one(set->pix_slots);
                set->pix_slots = slots[k];
            }
        }
    }
    c->src_bytes = bytes_per_pixel;
    return RC_OK;
}
RC_EXPORT uint32_t rc_ctx_source_bytes(const rc_ctx *c) { return c ? c->src_bytes : 0; }

RC_EXPORT uint64_t rc_out_capacity(const rc_ctx *c, uint32_t n) { return c ? (uint64_t)n * c->geo().N * c->src_bytes : 0; }

RC_EXPORT uint32_t rc_md_fields(const rc_ctx *c)
{
    if (!c) return 0;
    const bool comp = c->emit != rc::EMIT_RAW;
    if (c->level != 3) return comp ? 3 : 1;
    return comp ? 1 : 0;
}

// Fit the ctx's tables to (up to two frames of) its first batch: synchronous, once per ctx and per rc_ctx_refit_model; every later frame is
// written under them.  The sample is reduced into the scratch set the batch is about to use and counted on the device, the host builds the model.
// Modelled zstd (every reduction level; the value stage's code at level 1 only): the plain encoder tokenizes the sample, k_zstd_sample turns the
// slots into histograms.  DEFLATE value stage: the sample's residual streams are laid out flat (PIX_MODE_FLAT), k_pd_hist counts their bytes.
static int fit_value_model(rc_ctx *c, const void *frames_dev, uint32_t n)
{
    using namespace rc;
    const bool dz = c->values == VALUES_DEFLATE_HUFF;
    hipStream_t s = c->stream;
    const Scratch &sc = c->sets[c->cur];
    const uint32_t ns = n < 2 ? n : 2;
    void *d_sample = dz ? (void *)c->d_dzhist : c->d_sample, *h_sample = dz ? (void *)c->h_dzhist : c->h_sample;
    void *d_model = dz ? (void *)c->d_dzm : c->d_model, *h_model = dz ? (void *)c->h_dzm : c->h_model;
    const size_t sample_bytes = dz ? 256 * 4 : sizeof(ZstdSample), model_bytes = dz ? sizeof(DeflateModel) : sizeof(ZstdModel);
    for (int k = 0; k < 2; ++k)
        if (c->post_pending[k]) HIP_TRY(hipStreamWaitEvent(s, c->ev_post[k], 0));
    HIP_TRY(hipMemsetAsync(d_sample, 0, sample_bytes, s));
    if (dz) {
        launch_reduce(sc, frames_dev, ns, 1u, CODEC_DEFLATE, true, c->depth, s, nullptr, c->src_bytes);
        launch_scans(sc, ns, true, true, s);
        RecordParams rp;
        rp.level = 1u; rp.emit = c->emit; rp.depth = c->depth; rp.first_frame_id = 0; rp.packed_slots = 1u;
        rp.frame_bytes = c->geo().N * c->src_bytes;
        rp.pix_mode = PIX_MODE_FLAT;
        launch_assemble(sc, rp, ns, nullptr, nullptr, c->batch_seq, s);   // (the flat pass touches neither the records nor their offsets)
        launch_pd_hist(sc, ns, c->depth, c->d_dzhist, s);
    } else {
        launch_reduce(sc, frames_dev, ns, c->level == 3 ? 3u : 1u, CODEC_ZSTD_FAST, true, c->depth, s, nullptr, c->src_bytes);   // (with the raw maps: the sample counts all their bytes)
        launch_zstd_sample(sc, ns, c->level == 1, c->depth, c->d_sample, s);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h_sample, d_sample, sample_bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (dz) {
        dm_build_model(c->h_dzhist, c->h_dzm);
        c->values_on = c->h_dzm->usable != 0;
    } else {
        // compression_level -> how much size the faster block form of the binary maps may cost (rc_zstd_model.h): the reference hands the
        // level to libzstd (recode_writer.py:175-178), where 1 is the fast end too.  Level 1: up to 5 % of the binary-map stream, level 2: 2 %,
        // from 3 on the smaller form always.
        zstd_model_from_sample(c->h_sample, c->h_model, c->clevel == 1 ? 50u : (c->clevel == 2 ? 20u : 0u));
        // (no value stage: reduction levels 2 and 3; a code that does not pay: the stream is stored, in 128 KiB Raw blocks)
        if (c->values == VALUES_NONE || !zm_code_pays(c->h_sample->pix, c->h_model->pix_code)) c->h_model->valid &= ~ZM_PIX_CODE;
        c->values_on = (c->h_model->valid & ZM_PIX_CODE) != 0;
    }
    HIP_TRY(hipMemcpyAsync(d_model, h_model, model_bytes, hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (Scratch &set : c->sets) {
        if (dz) { set.dz_model = c->d_dzm; continue; }
        const ZstdModel &M = *c->h_model;
        set.zm_model = c->d_model;
        set.zm_lit_code = c->d_model->lit_code;
        set.zm_valid = M.valid;
        set.zm_budget = zm_block_budget(M, BLK_SLOT);
        set.zm_seq_bits = (M.valid & ZM_SEQ_TABLES) ? M.seq.ll_log + M.seq.ml_log : 12u;
    }
    c->model_ready = true;
    return RC_OK;
}

// The block encoder fused into the reduce kernel for a ctx's record form.  uint32 sources (src_bytes 4, rc_reduce32.hip) have the fast zstd
// encoder only (the modelled one is fitted inside the uint16 kernel).
static uint32_t fused_codec(uint32_t emit, uint32_t clevel, bool modelled, uint32_t src_bytes)
{
    using namespace rc;
    switch (emit) {
    case EMIT_ZSTD: return modelled && src_bytes != 4 ? CODEC_ZSTD_MODELLED : CODEC_ZSTD_FAST;
    case EMIT_LZ4: return clevel != 0 ? CODEC_LZ4_EVENTS : CODEC_LZ4_RUNS;
    case EMIT_BLOSC: return CODEC_BLOSC;
    case EMIT_DEFLATE: return CODEC_DEFLATE;
    default: return CODEC_NONE;
    }
}

static int enqueue_batch(rc_ctx *c, const void *frames_dev, uint32_t n, uint32_t first_frame_id, uint8_t *out_dev,
                         uint64_t out_cap, uint64_t *rec_off_dev, uint32_t *md_dev, bool timed)
{
    using namespace rc;
    hipStream_t s = c->stream;
    if ((c->modelled || c->values == VALUES_DEFLATE_HUFF) && !c->model_ready) {
        int r = fit_value_model(c, frames_dev, n);
        if (r != RC_OK) return r;
    }
    RecordParams rp;
    rp.level = c->level == 3 ? 3u : 1u;  // level 2 records are framed exactly like level 1 (statistics in place of residuals)
    rp.emit = c->emit; rp.depth = c->depth; rp.first_frame_id = first_frame_id;
    rp.packed_slots = 1u;   // (level 2: k_l2_emit leaves its statistics as tile-local packed streams, like level-1 residuals)
    rp.frame_bytes = c->geo().N * c->src_bytes;   // a record may not exceed the raw frame (recode_writer.py:565-566)
    hipEvent_t *ev = nullptr;
    if (timed) ev = c->ev;
    else if (c->profiling && (c->prof_phase++ % c->prof_every) == 0) {
        if (c->prof_used + 5 > c->prof_ev.size()) {
            for (int i = 0; i < 5; ++i) {
                hipEvent_t e;
                HIP_TRY(hipEventCreate(&e));
                c->prof_ev.push_back(e);
            }
        }
        ev = c->prof_ev.data() + c->prof_used;
        c->prof_used += 5;
    }
    // Two streams, two scratch sets.  The reduce kernel runs on the ctx's stream `s` (behind whatever produced the frames
    // there); everything after it runs on `pstream`.  Default: `s` then waits for the batch's records, so stream order as
    // the caller sees it is the plain one.  Pipelined (rc_ctx_set_pipelined): `s` does not wait - the next batch's reduce
    // kernel overlaps this batch's scans / layout / assembly, and consumers order themselves with rc_ctx_wait_results.
    const int k = c->cur;
    c->cur ^= 1;
    c->last = k;
    const rc::Scratch &sc = c->sets[k];
    // (two chains: consecutive batches' second stages on two streams - they overlap each other as well as the reduce kernels)
    const bool two = c->pipelined && c->two_chains;
    hipStream_t ps = two && k == 1 ? c->pstream_b : c->pstream;
    c->last_ps = ps;
    // the batch two calls ago must have left this set.  (Round 5 tried to skip the wait when hipEventQuery says the event has completed -
    // it always has, in steady state: no gain in the step, 9 us more host time per call.)
    if (c->post_pending[k]) HIP_TRY(hipStreamWaitEvent(s, c->ev_post[k], 0));
    if (ev) HIP_TRY(hipEventRecord(ev[0], s));
    // every device codec's block encoder runs inside the reduce kernel (LZ4; blosc = bit-shuffle + LZ4; zstd: the
    // byte-parallel half - literals, sequence tokens - with the serial FSE half lane-per-block behind it)
    const bool fitted_seq = c->modelled && (c->h_model->valid & ZM_SEQ_TABLES);
    hipStream_t tail = nullptr;
    if (sc.N % TILE_PX) {   // a partial last tile: its small launch goes to the second-stage stream, behind "the frames are there"
        HIP_TRY(hipEventRecord(c->ev_in[k], s));
        HIP_TRY(hipStreamWaitEvent(ps, c->ev_in[k], 0));
        tail = ps;
    }
    const uint32_t codec = fused_codec(c->emit, c->clevel, c->modelled, c->src_bytes);
    const bool keep_maps = c->keep_bitmap || c->emit == EMIT_RAW;
    if (c->src_bytes == 4)   // uint32 sources (rc_reduce32.hip): reduce + pack with the codec's block encoder inside the kernel, as in the uint16 path
        launch_reduce32(sc, static_cast<const uint32_t *>(frames_dev), c->thr32, n, c->level, c->depth, s, codec, keep_maps);
    else
        launch_reduce(sc, frames_dev, n, c->level, codec, keep_maps, c->depth, s, tail, c->src_bytes);
    // every event costs a few microseconds of stream time: the asynchronous path records only the ones it needs
    // (start, end of the reduce kernel, end of the batch) unless RC_PROFILE_ALL_STAGES is set
    const bool all_ev = ev && (timed || c->profile_all);
    // (one event behind the reduce kernel: every packet on this stream is a few microseconds between two reduce kernels)
    hipEvent_t red = ev ? ev[1] : c->ev_red[k];
    HIP_TRY(hipEventRecord(red, s));
    HIP_TRY(hipStreamWaitEvent(ps, red, 0));
    if (c->level == 2) launch_l2(sc, n, c->nx, c->l2_sum, c->depth, ps);   // the tiles' raw values -> their components' statistics (rc_l2.hip)
    const bool lits_only = c->modelled && (c->h_model->valid & ZM_LITS_ONLY);   // dense maps: no block has sequences, nothing for the FSE chain to do
    if (c->emit == EMIT_ZSTD && !lits_only) launch_zstd_fse(sc, n, fitted_seq ? (const void *)&c->d_model->seq : c->d_ztab, fitted_seq, ps);
    if (all_ev) HIP_TRY(hipEventRecord(ev[2], ps));
    launch_scans(sc, n, c->level != 3, c->emit != EMIT_RAW, ps);
    if (all_ev) HIP_TRY(hipEventRecord(ev[3], ps));
    // the value stage (rc_launch.h), where the ctx's table pays: the residual stream is laid out flat, Huffman-coded in chunks and placed
    // behind the binary-map stream; its encoded size is part of the record layout
    if (c->values_on) {
        rp.pix_mode = PIX_MODE_FLAT;
        launch_assemble(sc, rp, n, out_dev, rec_off_dev, c->batch_seq, ps);
        launch_values_encode(c->values, sc, n, c->depth, ps);
        launch_values_scan(c->values, sc, n, c->depth, ps);
        rp.pix_mode = PIX_MODE_SKIP;
    }
    if (two && c->post_pending[k ^ 1]) {
        // Two chains run the second stages of batches i and i + 1 at the same time, which is why include/recode_hip.h asks a pipelined caller for
        // two sets of output buffers.  A caller that hands this batch a buffer the previous batch is still writing (rounds 1-4 tolerated that: one
        // second-stage stream serialised them) gets that order back instead of torn records: this batch's layout waits for the other chain.
        auto overlap = [](const uint8_t *a, uint64_t an, const uint8_t *b, uint64_t bn) { return a && b && a < b + bn && b < a + an; };
        const uint8_t *rec8 = reinterpret_cast<const uint8_t *>(rec_off_dev), *md8 = reinterpret_cast<const uint8_t *>(md_dev);
        if (overlap(out_dev, out_cap, c->prev_out, c->prev_out_cap) || overlap(rec8, (uint64_t)(n + 1) * 8, c->prev_rec, (uint64_t)(c->prev_n + 1) * 8) ||
            overlap(md8, (uint64_t)n * 12, c->prev_md, (uint64_t)c->prev_n * 12))
            HIP_TRY(hipStreamWaitEvent(ps, c->ev_post[k ^ 1], 0));
    }
    c->prev_out = out_dev; c->prev_out_cap = out_cap; c->prev_n = n;
    c->prev_rec = reinterpret_cast<const uint8_t *>(rec_off_dev); c->prev_md = reinterpret_cast<const uint8_t *>(md_dev);
    launch_layout(sc, rp, n, out_cap, rec_off_dev, md_dev, ps);
    launch_assemble(sc, rp, n, out_dev, rec_off_dev, c->batch_seq, ps);
    ++c->batch_seq;
    if (c->values_on) launch_values_gather(c->values, sc, n, c->depth, 16, out_dev, rec_off_dev, ps);
    if (ev) HIP_TRY(hipEventRecord(ev[4], ps));
    if (two && c->post_pending[k ^ 1]) HIP_TRY(hipStreamWaitEvent(ps, c->ev_post[k ^ 1], 0));   // batches still COMPLETE in order
    HIP_TRY(hipEventRecord(c->ev_post[k], ps));
    c->post_pending[k] = true;
    if (!c->pipelined) HIP_TRY(hipStreamWaitEvent(s, c->ev_post[k], 0));
    HIP_TRY(hipGetLastError());
    c->last_n = n;
    return RC_OK;
}

static int check_batch_args(rc_ctx *c, const void *frames, uint32_t n, const void *out, const void *rec, const void *md)
{
    if (!c || !frames || !out || !rec || !md) return fail(RC_ERR_BAD_ARG, "NULL argument");
    if (n == 0 || n > c->max_batch) return fail(RC_ERR_BAD_ARG, "n must be in 1..max_batch");
    if (!c->thr_set) return fail(RC_ERR_BAD_ARG, "threshold not set (rc_set_threshold / rc_set_dark)");
    return RC_OK;
}

RC_EXPORT int rc_reduce_compress_batch_async(rc_ctx *c, const void *frames_dev, uint32_t n, uint32_t first_frame_id,
                                             uint8_t *out_dev, uint64_t out_cap, uint64_t *rec_offsets_dev, uint32_t *md_dev)
{
    int r = check_batch_args(c, frames_dev, n, out_dev, rec_offsets_dev, md_dev);
    if (r != RC_OK) return r;
    RC_ON_DEVICE(c->device);
    return enqueue_batch(c, frames_dev, n, first_frame_id, out_dev, out_cap, rec_offsets_dev, md_dev, false);
}

// Level 2, first rc_ctx_set_pipelined(ctx, 1): the second chain's workspace (another 8 bytes per pixel and frame of the batch).  A GPU that
// cannot hold it keeps ONE chain - a few per cent slower (rc_api.hip, "two chains"), not an error.  The streams are drained when this runs.
static void l2_second_chain(rc_ctx *c)
{
    if (c->level != 2 || c->two_chains) return;
    const uint64_t B = c->max_batch, ids = (uint64_t)c->geo().ntiles * rc::TILE_PX;
    if (!c->d_l2_node[1]) {
        bool ok = c->dmem.try_alloc(c->d_l2_node[1], B * ids * 8) == hipSuccess && hipMemset(c->d_l2_node[1], 0, B * ids * 8) == hipSuccess &&
                  c->dmem.try_alloc(c->d_l2_base[1], B * (uint64_t)c->geo().ntiles * 64 * 2) == hipSuccess && hipDeviceSynchronize() == hipSuccess;
        if (!ok) {
            (void)hipGetLastError();
            c->dmem.free_one(c->d_l2_node[1]);
            c->dmem.free_one(c->d_l2_base[1]);
            return;
        }
    }
    c->sets[1].l2_node = c->d_l2_node[1];
    c->sets[1].l2_base = c->d_l2_base[1];
    c->two_chains = true;
}

RC_EXPORT int rc_ctx_set_pipelined(rc_ctx *c, int on)
{
    if (!c) return fail(RC_ERR_BAD_ARG, "ctx is NULL");
    RC_ON_DEVICE(c->device);
    HIP_TRY(hipStreamSynchronize(c->pstream));  // drain both: two chains on / off move set 1's second stage between the streams (l2_second_chain relies on it)
    HIP_TRY(hipStreamSynchronize(c->pstream_b));
    if (on) l2_second_chain(c);
    c->pipelined = on != 0;
    return RC_OK;
}
RC_EXPORT int rc_ctx_wait_results(rc_ctx *c, void *hip_stream)
{
    if (!c) return fail(RC_ERR_BAD_ARG, "ctx is NULL");
    RC_ON_DEVICE(c->device);
    if (c->post_pending[c->last])
        HIP_TRY(hipStreamWaitEvent(hip_stream ? reinterpret_cast<hipStream_t>(hip_stream) : c->stream, c->ev_post[c->last], 0));
    return RC_OK;
}

RC_EXPORT int rc_ctx_sync(rc_ctx *c)
{
    if (!c) return fail(RC_ERR_BAD_ARG, "ctx is NULL");
    RC_ON_DEVICE(c->device);
    HIP_TRY(hipStreamSynchronize(c->pstream_b));
    HIP_TRY(hipMemcpyAsync(&c->h_status[0], c->recent().status, sizeof(rc::BatchStatus), hipMemcpyDeviceToHost, c->pstream));
    HIP_TRY(hipMemcpyAsync(&c->h_status[1], c->d_first_err, sizeof(rc::BatchStatus), hipMemcpyDeviceToHost, c->pstream));
    HIP_TRY(hipMemsetAsync(c->d_first_err, 0, sizeof(rc::BatchStatus), c->pstream));
    HIP_TRY(hipStreamSynchronize(c->pstream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const uint32_t n_batches = c->batch_seq;
    c->batch_seq = 0;
    for (size_t b = 0; b + 5 <= c->prof_used; b += 5) {  // fold the finished batches' stage events into the sums
        float ms;
        if (!c->profile_all) {
            if (hipEventElapsedTime(&ms, c->prof_ev[b], c->prof_ev[b + 1]) == hipSuccess) c->prof_sum_ms[0] += ms;
        } else
        for (int i = 0; i < 4; ++i)
            if (hipEventElapsedTime(&ms, c->prof_ev[b + i], c->prof_ev[b + i + 1]) == hipSuccess) c->prof_sum_ms[i] += ms;
        if (hipEventElapsedTime(&ms, c->prof_ev[b], c->prof_ev[b + 4]) == hipSuccess) c->prof_sum_ms[4] += ms;
        ++c->prof_batches;
    }
    c->prof_used = 0;
    if (c->h_status[1].total != 0) c->h_status[1] = rc::first_err_decode(c->h_status[1].total);   // (k_gather leaves a key: rc_device.h)
    if (c->h_status[1].code != 0) {  // the first batch that failed since the last sync (not only the most recent one)
        char msg[160];
        if (n_batches > 1)
            snprintf(msg, sizeof msg, "%s (frame %u of batch %llu of the %u enqueued since the last sync)", rc_strerror(c->h_status[1].code),
                     c->h_status[1].frame, (unsigned long long)c->h_status[1].total, n_batches);
        else
            snprintf(msg, sizeof msg, "%s (frame %u of the batch)", rc_strerror(c->h_status[1].code), c->h_status[1].frame);
        return fail(c->h_status[1].code, msg);
    }
    return RC_OK;
}

RC_EXPORT int rc_reduce_compress_batch(rc_ctx *c, const void *frames, uint32_t n, uint32_t first_frame_id, uint8_t *out,
                                       uint64_t out_cap, uint64_t *rec_offsets, uint32_t *md)
{
    int r = check_batch_args(c, frames, n, out, rec_offsets, md);
    if (r != RC_OK) return r;
    RC_ON_DEVICE(c->device);
    const uint64_t frame_bytes = c->geo().N * c->src_bytes;
    const void *fdev = frames;
    if (!is_device_ptr(frames)) {
        r = c->d_frames.ensure(c->dmem, (uint64_t)n * frame_bytes);
        if (r != RC_OK) return r;
        HIP_TRY(hipMemcpyAsync(c->d_frames.p, frames, (uint64_t)n * frame_bytes, hipMemcpyHostToDevice, c->stream));
        fdev = c->d_frames.p;
    }
    uint8_t *odev = out;
    uint64_t cap = out_cap;
    const bool out_host = !is_device_ptr(out);
    if (out_host) {
        const uint64_t worst = (uint64_t)n * frame_bytes;
        cap = out_cap < worst ? out_cap : worst;
        r = c->d_out.ensure(c->dmem, cap);
        if (r != RC_OK) return r;
        odev = c->d_out.p;
    }
    r = enqueue_batch(c, fdev, n, first_frame_id, odev, cap, c->d_rec_off, c->d_md, true);
    if (r != RC_OK) return r;
    r = rc_ctx_sync(c);
    for (int i = 0; i < 4; ++i) (void)hipEventElapsedTime(&c->stage_ms[i], c->ev[i], c->ev[i + 1]);
    (void)hipEventElapsedTime(&c->stage_ms[4], c->ev[0], c->ev[4]);
    if (r != RC_OK) return r;
    int r2 = copy_out(rec_offsets, c->d_rec_off, (uint64_t)(n + 1) * 8, c->stream);
    if (r2 == RC_OK) r2 = copy_out(md, c->d_md, (uint64_t)n * 12, c->stream);
    if (r2 == RC_OK && out_host) r2 = copy_out(out, c->d_out.p, c->h_status->total, c->stream);
    if (r2 != RC_OK) return r2;
    HIP_TRY(hipStreamSynchronize(c->stream));
    return RC_OK;
}

// ---- seam 1, host streaming form ----------------------------------------------------------------------------------------
RC_EXPORT void *rc_host_alloc(uint64_t bytes)
{
    void *p = nullptr;
    if (hipHostMalloc(&p, bytes ? bytes : 16, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        fail(RC_ERR_DEVICE, "hipHostMalloc failed");
        return nullptr;
    }
    return p;
}
RC_EXPORT int rc_host_free(void *p)
{
    if (p) HIP_TRY(hipHostFree(p));
    return RC_OK;
}
RC_EXPORT int rc_host_register(void *p, uint64_t bytes)
{
    if (!p || !bytes) return fail(RC_ERR_BAD_ARG, "NULL / zero argument");
    HIP_TRY(hipHostRegister(p, bytes, hipHostRegisterDefault));
    return RC_OK;
}
RC_EXPORT int rc_host_unregister(void *p)
{
    if (p) HIP_TRY(hipHostUnregister(p));
    return RC_OK;
}

static int pipe_slot_init(rc_ctx *c, rc_ctx::PipeSlot &p)
{
    const uint64_t B = c->max_batch;
    if (!c->copy_stream) HIP_TRY(hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
    if (!c->d2h_stream) HIP_TRY(hipStreamCreateWithFlags(&c->d2h_stream, hipStreamNonBlocking));
    RC_ALLOC(c->dmem, p.d_in, B * c->geo().N * c->src_bytes + 64);
    RC_ALLOC(c->dmem, p.d_out, rc_out_capacity(c, (uint32_t)B) + 64);
    RC_ALLOC(c->dmem, p.d_rec, (B + 1) * 8);
    RC_ALLOC(c->dmem, p.d_md, B * 12);
    RC_ALLOC(c->hmem, p.h_rec, (B + 1) * 8);
    RC_ALLOC(c->hmem, p.h_md, B * 12);
    RC_ALLOC(c->hmem, p.h_stat, sizeof(rc::BatchStatus));
    HIP_TRY(hipEventCreateWithFlags(&p.ev_h2d, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&p.ev_done, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&p.ev_fetch, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&p.ev_val, hipEventDisableTiming));
    RC_ALLOC(c->dmem, p.d_val, B * 4 + 64);
    RC_ALLOC(c->hmem, p.h_val, B * 4 + 64);
    return RC_OK;
}

RC_EXPORT int rc_ctx_set_validation(rc_ctx *c, uint32_t gap, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h)
{
    if (!c) return fail(RC_ERR_BAD_ARG, "ctx is NULL");
    if (gap && (w == 0 || h == 0 || w > 128 || h > 128 || (uint64_t)x0 + w > c->nx || (uint64_t)y0 + h > c->ny))
        return fail(RC_ERR_BAD_ARG, "rc_ctx_set_validation: the region must lie inside the frame and hold at most 128 x 128 pixels");
    c->val_gap = gap; c->val_x0 = x0; c->val_y0 = y0; c->val_w = w; c->val_h = h;
    return RC_OK;
}

RC_EXPORT int rc_pipe_validation(rc_ctx *c, uint32_t slot, uint32_t *counts)
{
    if (!c || slot >= RC_PIPE_SLOTS || !counts) return fail(RC_ERR_BAD_ARG, "NULL argument / slot out of range");
    rc_ctx::PipeSlot &p = c->pipe[slot];
    if (p.state != p.SUBMITTED && p.state != p.RESULT_TAKEN) return fail(RC_ERR_BAD_ARG, "nothing submitted on this slot");
    if (!p.has_val) { for (uint32_t i = 0; i < p.n; ++i) counts[i] = 0xFFFFFFFFu; return RC_OK; }
    HIP_TRY(hipEventSynchronize(p.ev_val));
    memcpy(counts, p.h_val, (uint64_t)p.n * 4);
    return RC_OK;
}

RC_EXPORT int rc_pipe_submit(rc_ctx *c, uint32_t slot, const void *frames_host, uint32_t n, uint32_t first_frame_id)
{
    if (!c || !frames_host || slot >= RC_PIPE_SLOTS) return fail(RC_ERR_BAD_ARG, "NULL argument / slot out of range");
    if (n == 0 || n > c->max_batch) return fail(RC_ERR_BAD_ARG, "n must be in 1..max_batch");
    if (!c->thr_set) return fail(RC_ERR_BAD_ARG, "threshold not set (rc_set_threshold / rc_set_dark)");
    RC_ON_DEVICE(c->device);
    rc_ctx::PipeSlot &p = c->pipe[slot];
    if (p.state != p.FREE) return fail(RC_ERR_BAD_ARG, "slot is still in use (result / fetch_wait not called)");
    if (!p.d_in) {
        int r = pipe_slot_init(c, p);
        if (r != RC_OK) return r;
    }
    if (!c->pipelined) {   // the streaming form always lets consecutive batches overlap
        HIP_TRY(hipStreamSynchronize(c->pstream));   // drain both: two chains on / off move set 1's second stage between the streams (l2_second_chain relies on it)
        HIP_TRY(hipStreamSynchronize(c->pstream_b));
        l2_second_chain(c);
        c->pipelined = true;
    }
    // Page-locked (or registered) frames are read by the reduce kernel IN PLACE, over the link: every frame byte is needed
    // exactly once, by wide nontemporal loads, so a copy into device memory first would only add a pass (and the copy
    // engines moved 26-31 GB/s where the kernel's own reads move what the link gives).
    const void *fdev = nullptr;
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, frames_host) == hipSuccess) {
        if (a.type == hipMemoryTypeHost && a.devicePointer) fdev = a.devicePointer;
    } else (void)hipGetLastError();
    p.zero_copy = fdev != nullptr;
    if (!fdev) {
        HIP_TRY(hipMemcpyAsync(p.d_in, frames_host, (uint64_t)n * c->geo().N * c->src_bytes, hipMemcpyHostToDevice, c->copy_stream));
        HIP_TRY(hipEventRecord(p.ev_h2d, c->copy_stream));
        HIP_TRY(hipStreamWaitEvent(c->stream, p.ev_h2d, 0));
        fdev = p.d_in;
    }
    int r = enqueue_batch(c, fdev, n, first_frame_id, p.d_out, rc_out_capacity(c, c->max_batch), p.d_rec, p.d_md, false);
    if (r != RC_OK) return r;
    p.has_val = c->val_gap != 0;
    if (p.has_val) {   // validation frames of this batch: the dose-rate count, from the frames the reduce kernel has just read
        rc::launch_roi_components(fdev, c->src_bytes == 4 ? (const void *)c->thr32 : (const void *)c->geo().thr, c->geo().N, c->nx, n, first_frame_id, c->val_gap, c->val_x0, c->val_y0, c->val_w, c->val_h, p.d_val, c->stream, c->src_bytes);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(p.h_val, p.d_val, (uint64_t)n * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipEventRecord(p.ev_val, c->stream));
    }
    if (p.zero_copy) HIP_TRY(hipEventRecord(p.ev_h2d, c->stream));   // "input consumed" = the reduce kernel (and the count) have run
    hipStream_t ps = c->last_ps;   // carries the batch's assembly: the metadata follows it
    HIP_TRY(hipMemcpyAsync(p.h_rec, p.d_rec, (uint64_t)(n + 1) * 8, hipMemcpyDeviceToHost, ps));
    HIP_TRY(hipMemcpyAsync(p.h_md, p.d_md, (uint64_t)n * 12, hipMemcpyDeviceToHost, ps));
    HIP_TRY(hipMemcpyAsync(p.h_stat, c->recent().status, sizeof(rc::BatchStatus), hipMemcpyDeviceToHost, ps));
    HIP_TRY(hipEventRecord(p.ev_done, ps));
    p.n = n;
    p.state = p.SUBMITTED;
    return RC_OK;
}

RC_EXPORT int rc_pipe_input_done(rc_ctx *c, uint32_t slot)
{
    if (!c || slot >= RC_PIPE_SLOTS) return fail(RC_ERR_BAD_ARG, "NULL argument / slot out of range");
    if (c->pipe[slot].state == rc_ctx::PipeSlot::FREE) return RC_OK;
    HIP_TRY(hipEventSynchronize(c->pipe[slot].ev_h2d));
    return RC_OK;
}

RC_EXPORT int rc_pipe_result(rc_ctx *c, uint32_t slot, uint64_t *rec_offsets, uint32_t *md, uint64_t *total)
{
    if (!c || slot >= RC_PIPE_SLOTS || !rec_offsets || !md || !total) return fail(RC_ERR_BAD_ARG, "NULL argument / slot out of range");
    rc_ctx::PipeSlot &p = c->pipe[slot];
    if (p.state != p.SUBMITTED) return fail(RC_ERR_BAD_ARG, "nothing submitted on this slot");
    HIP_TRY(hipEventSynchronize(p.ev_done));
    p.state = p.RESULT_TAKEN;
    if (p.h_stat->code != 0) {
        char msg[128];
        snprintf(msg, sizeof msg, "%s (frame %u of the batch)", rc_strerror(p.h_stat->code), p.h_stat->frame);
        p.state = p.FREE;
        return fail(p.h_stat->code, msg);
    }
    memcpy(rec_offsets, p.h_rec, (uint64_t)(p.n + 1) * 8);
    memcpy(md, p.h_md, (uint64_t)p.n * 12);
    *total = p.h_stat->total;
    return RC_OK;
}

RC_EXPORT int rc_pipe_fetch(rc_ctx *c, uint32_t slot, uint8_t *dst_host, uint64_t bytes)
{
    if (!c || slot >= RC_PIPE_SLOTS || (!dst_host && bytes)) return fail(RC_ERR_BAD_ARG, "NULL argument / slot out of range");
    rc_ctx::PipeSlot &p = c->pipe[slot];
    if (p.state != p.RESULT_TAKEN) return fail(RC_ERR_BAD_ARG, "rc_pipe_result has not been called for this slot");
    if (bytes > p.h_stat->total) return fail(RC_ERR_BAD_ARG, "more bytes than the batch's records hold");
    RC_ON_DEVICE(c->device);
    if (bytes) HIP_TRY(hipMemcpyAsync(dst_host, p.d_out, bytes, hipMemcpyDeviceToHost, c->d2h_stream));
    HIP_TRY(hipEventRecord(p.ev_fetch, c->d2h_stream));
    p.state = p.FETCHING;
    return RC_OK;
}

RC_EXPORT int rc_pipe_fetch_wait(rc_ctx *c, uint32_t slot)
{
    if (!c || slot >= RC_PIPE_SLOTS) return fail(RC_ERR_BAD_ARG, "NULL argument / slot out of range");
    rc_ctx::PipeSlot &p = c->pipe[slot];
    if (p.state == p.RESULT_TAKEN) { p.state = p.FREE; return RC_OK; }   // nothing fetched: the slot is simply released
    if (p.state != p.FETCHING) return fail(RC_ERR_BAD_ARG, "rc_pipe_fetch has not been called for this slot");
    HIP_TRY(hipEventSynchronize(p.ev_fetch));
    p.state = p.FREE;
    return RC_OK;
}

RC_EXPORT int rc_ctx_refit_model(rc_ctx *c)
{
    if (!c) return fail(RC_ERR_BAD_ARG, "ctx is NULL");
    c->model_ready = false;
    return RC_OK;
}

RC_EXPORT int rc_get_binary_map(rc_ctx *c, uint32_t i, uint8_t *bitmap_out)
{
    if (!c || !bitmap_out) return fail(RC_ERR_BAD_ARG, "NULL argument");
    if (i >= c->last_n) return fail(RC_ERR_BAD_ARG, "frame index outside the most recent batch");
    if (!c->keep_bitmap && c->emit != rc::EMIT_RAW && c->level != 2) return fail(RC_ERR_BAD_ARG, "binary maps are not kept (rc_ctx_keep_binary_maps(ctx, 0))");
    RC_ON_DEVICE(c->device);
    int r = copy_out(bitmap_out, c->recent().bitmap + (uint64_t)i * c->geo().nb_stride, c->geo().nb, c->stream);
    if (r != RC_OK) return r;
    HIP_TRY(hipStreamSynchronize(c->stream));
    return RC_OK;
}

RC_EXPORT int rc_ctx_set_profiling(rc_ctx *c, int on)
{
    if (!c) return fail(RC_ERR_BAD_ARG, "ctx is NULL");
    c->profiling = on != 0;
    c->prof_every = on > 1 ? (uint32_t)on : 1u;
    c->prof_phase = 0;
    for (double &v : c->prof_sum_ms) v = 0;
    c->prof_batches = 0;
    return RC_OK;
}
RC_EXPORT int rc_ctx_get_profile(rc_ctx *c, double sum_ms[5], uint64_t *batches)
{
    if (!c || !sum_ms || !batches) return fail(RC_ERR_BAD_ARG, "NULL argument");
    memcpy(sum_ms, c->prof_sum_ms, sizeof c->prof_sum_ms);
    *batches = c->prof_batches;
    return RC_OK;
}

RC_EXPORT int rc_ctx_set_l2_statistics(rc_ctx *c, uint32_t l2_statistics)
{
    if (!c || l2_statistics > 2) return fail(RC_ERR_BAD_ARG, "l2_statistics must be 0, 1 (max) or 2 (sum)");
    c->l2_sum = l2_statistics == 2 ? 1u : 0u;
    return RC_OK;
}

RC_EXPORT int rc_ctx_keep_binary_maps(rc_ctx *c, int on)
{
    if (!c) return fail(RC_ERR_BAD_ARG, "ctx is NULL");
    c->keep_bitmap = on != 0;
    return RC_OK;
}

RC_EXPORT int rc_get_stage_ms(rc_ctx *c, float ms[5])
{
    if (!c || !ms) return fail(RC_ERR_BAD_ARG, "NULL argument");
    memcpy(ms, c->stage_ms, sizeof c->stage_ms);
    return RC_OK;
}

// ---- seam 3 ------------------------------------------------------------------------------------------------------
RC_EXPORT int64_t rc_unpack_frame_sparse(uint32_t nx, uint32_t ny, uint32_t bit_depth, const uint8_t *bitmap,
                                         const uint8_t *pixvals, uint64_t pixvals_bytes, uint64_t *out,
                                         uint64_t out_cap_triplets, uint32_t reduction_level)
{
    if (!bitmap || nx == 0 || ny == 0 || (!out && out_cap_triplets)) return fail(RC_ERR_BAD_ARG, "NULL / zero argument");
    if (reduction_level == 1 && (bit_depth == 0 || bit_depth > 64)) return fail(RC_ERR_BAD_ARG, "bit_depth must be 1..64");
    if (reduction_level == 1 && !pixvals && pixvals_bytes) return fail(RC_ERR_BAD_ARG, "pixvals is NULL");
    UtilScope util_scope;
    int r = util_scope.enter();
    if (r != RC_OK) return r;
    Util &u = g_util;
    const uint64_t N = (uint64_t)nx * ny, nb = (N + 7) / 8, nb8 = (nb + 7) / 8;
    const uint32_t nblk = (uint32_t)((nb8 + rc::WG - 1) / rc::WG);
    const uint8_t *d_bm = nullptr, *d_px = nullptr;
    r = stage_in(bitmap, nb, u.a, d_bm, nb8 * 8 - nb + 8);
    if (r != RC_OK) return r;
    if (reduction_level == 1 && pixvals_bytes) {
        r = stage_in(pixvals, pixvals_bytes, u.b, d_px);
        if (r != RC_OK) return r;
    }
    r = u.w.ensure(u.dmem, (uint64_t)nblk * 8 + 16);
    if (r != RC_OK) return r;
    uint32_t *blk_cnt = u.w.as<uint32_t>(), *blk_off = blk_cnt + nblk;
    uint64_t *nnz_dev = reinterpret_cast<uint64_t *>(blk_cnt + 2 * (uint64_t)nblk);
    // pass 1: count, so the output can be bounds-checked (and sized) before anything is written
    rc::launch_expand_count(d_bm, nb8, N, blk_cnt, blk_off, nnz_dev, u.stream);
    HIP_TRY(hipMemcpyAsync(u.h_scalar, nnz_dev, 8, hipMemcpyDeviceToHost, u.stream));
    HIP_TRY(hipStreamSynchronize(u.stream));
    const uint64_t nnz = *u.h_scalar;
    if (!out) return (int64_t)nnz;  // counting call
    if (nnz > out_cap_triplets) return fail(RC_ERR_OUT_TOO_SMALL, "out holds fewer triplets than the bitmap has set bits");
    if (reduction_level == 1 && (nnz * bit_depth + 7) / 8 > pixvals_bytes)
        return fail(RC_ERR_CORRUPT, "pixvals shorter than popcount(bitmap) * bit_depth bits");
    if (nnz == 0) return 0;
    StagedOut so;
    if ((r = so.begin(out, nnz * 24)) != RC_OK) return r;
    rc::launch_expand_emit(d_bm, nb8, N, nx, blk_off, d_px, pixvals_bytes, bit_depth, reduction_level, nnz, so.as<uint64_t>(), u.stream);
    HIP_TRY(hipGetLastError());
    if ((r = so.finish(out, nnz * 24)) != RC_OK) return r;
    return (int64_t)nnz;
}

RC_EXPORT int rc_bit_pack(const uint16_t *pixvals, uint64_t n, uint32_t bit_depth, uint8_t *out, uint64_t out_n)
{
    if (!out || (!pixvals && n)) return fail(RC_ERR_BAD_ARG, "NULL argument");
    if (bit_depth == 0 || bit_depth > 32) return fail(RC_ERR_BAD_ARG, "bit_depth must be 1..32");
    if (out_n != (n * bit_depth + 7) / 8) return fail(RC_ERR_BAD_ARG, "out_n must be ceil(n*bit_depth/8)");
    if (out_n == 0) return RC_OK;
    UtilScope util_scope;
    int r = util_scope.enter();
    if (r != RC_OK) return r;
    Util &u = g_util;
    const uint16_t *d_in = nullptr;
    r = stage_in(pixvals, n * 2, u.a, d_in);
    if (r != RC_OK) return r;
    StagedOut so;
    if ((r = so.begin(out, out_n)) != RC_OK) return r;
    rc::launch_bit_pack(d_in, n, bit_depth, so.as<uint8_t>(), out_n, u.stream);
    HIP_TRY(hipGetLastError());
    return so.finish(out, out_n);
}

RC_EXPORT int rc_bit_unpack(const uint8_t *packed, uint64_t packed_bytes, uint64_t n, uint32_t bit_depth, uint64_t *out)
{
    if (!out || (!packed && packed_bytes)) return fail(RC_ERR_BAD_ARG, "NULL argument");
    if (bit_depth == 0 || bit_depth > 64) return fail(RC_ERR_BAD_ARG, "bit_depth must be 1..64");
    if ((n * bit_depth + 7) / 8 > packed_bytes) return fail(RC_ERR_CORRUPT, "packed shorter than n * bit_depth bits");
    if (n == 0) return RC_OK;
    UtilScope util_scope;
    int r = util_scope.enter();
    if (r != RC_OK) return r;
    Util &u = g_util;
    const uint8_t *d_in = nullptr;
    r = stage_in(packed, packed_bytes, u.a, d_in);
    if (r != RC_OK) return r;
    StagedOut so;
    if ((r = so.begin(out, n * 8)) != RC_OK) return r;
    rc::launch_bit_unpack(d_in, packed_bytes, n, bit_depth, so.as<uint64_t>(), u.stream);
    HIP_TRY(hipGetLastError());
    return so.finish(out, n * 8);
}

// ---- synthetic stacks -------------------------------------------------------------------------------------------
RC_EXPORT int rc_synth_dark(int device_id, uint32_t seed, uint64_t n_pixels, uint16_t *dark_dev)
{
    if (!dark_dev) return fail(RC_ERR_BAD_ARG, "NULL argument");
    RC_ON_DEVICE(device_id);
    rc::launch_synth_dark(seed, n_pixels, dark_dev, nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    return RC_OK;
}
RC_EXPORT int rc_synth_frames_clustered(int device_id, uint32_t seed, uint32_t first_frame, uint32_t n_frames, uint32_t nx, uint32_t ny,
                                        uint32_t seed_ppm, const uint16_t *dark_dev, uint16_t *frames_dev)
{
    if (!dark_dev || !frames_dev || n_frames == 0 || nx == 0 || ny == 0) return fail(RC_ERR_BAD_ARG, "NULL / zero argument");
    if ((uint64_t)nx * ny > 0xFFFFFFFFull) return fail(RC_ERR_BAD_ARG, "rc_synth_frames_clustered: nx * ny must fit 32 bits");
    RC_ON_DEVICE(device_id);
    rc::launch_synth_frames_clustered(seed, first_frame, n_frames, nx, ny, seed_ppm, dark_dev, frames_dev, nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    return RC_OK;
}
RC_EXPORT int rc_synth_frames(int device_id, uint32_t seed, uint32_t first_frame, uint32_t n_frames, uint64_t n_pixels,
                              uint32_t sparsity_ppm, const uint16_t *dark_dev, uint16_t *frames_dev)
{
    if (!dark_dev || !frames_dev || n_frames == 0) return fail(RC_ERR_BAD_ARG, "NULL / zero argument");
    RC_ON_DEVICE(device_id);
    rc::launch_synth_frames(seed, first_frame, n_frames, n_pixels, sparsity_ppm, dark_dev, frames_dev, nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    return RC_OK;
}
