// rc_count.hip - electron counting on the decoded streams of a batch (rc_count_frames, gfx950): every 8-connected component of a frame's
// set pixels becomes one event at its centroid.  Runs inside the batched reader behind launch_expand_batch_count, in the place of the emit
// and sum kernels, and reads what they read.
//
//   pyrecode/utils/converters.py:59-123   l1_to_l4_converter (scipy.ndimage.label per frame :88, then a helper per frame :90)
//   pyrecode/utils/converters.py:167-259  _get_centroids_2d_nb_w, _nb_u, _nb_m (per-label sums in float32; np.round at :92)
//
// A set pixel's id is frame_base[f] + its rank inside its frame: ids ascend in raster order over the whole batch, and the smaller id of
// two joined trees stays the root, so a component's root is its first pixel and the roots in id order are scipy's label order.  A frame
// owns the id range [frame_base[f], frame_base[f + 1]): no link can leave it.  Workspace per id: a uint32 parent (0 = root, else
// parent id + 1 - zero is the resting state, set by one memset per batch), a uint32 area and 2, 3 or 5 uint64 sums (rc_count.h: CntSums).
//
//   k_cnt_dir    rank of every 64-pixel word's first set pixel in its frame (blk_off + a workgroup scan): turns a position into an id
//   k_cnt_link   every set pixel joins its earlier neighbours W, N - or NW, NE where N is clear - by union-find
//   k_cnt_acc    every set pixel adds its terms to its root's sums; a lane joins the consecutive pixels of its word that share a root,
//                the wave joins the lanes that share one, before a 64-bit no-return atomic is issued
//   k_cnt_roots  roots that pass area_threshold, counted per (frame, block); rc_expand.hip's two scans turn the counts into offsets
//   k_cnt_emit   the events, in id order, with their divisions (rc_count.h: cnt_finish)
//   k_cnt_place  counted views (rc_sum_add_counted), in the place of k_cnt_roots, the scans and k_cnt_emit: one count per kept component
//                added to its cell of the caller's view, on a grid up to 16 times finer (rc_count.h: cnt_finish_fine)
//
// Every kernel is one lane per 64-pixel word, grid (blocks of WG words, frames), and starts with the same gate: nothing happens once *err
// is set (a decoder, a short value stream, too many events for the caller's buffer).  Loops: a word's set bits are consumed one per
// iteration; a find walks to strictly smaller ids; a union retries only behind a compare-and-swap that lost to another link of the same
// root, and goes on from that root's new, smaller parent (rc_l2.hip: uf_find_t / uf_union rest on the same two facts).
#include "rc_count.h"

#include "rc_expand.h"

namespace rc {
namespace {

struct CntArgs {
    const uint8_t *bm;
    uint64_t bm_stride, nb8, N;
    uint32_t nx, nblk, n;
    const uint32_t *blk_off;
    const uint64_t *frame_base;
    const uint8_t *pv;
    uint64_t pv_stride;
    const uint32_t *pv_bytes;
    uint32_t d, level, thr;
    uint64_t id_cap;
    uint32_t *dir, *parent, *area;
    unsigned long long *acc;       // sum j of id x at acc[j * id_cap + x]
    uint32_t *ev_cnt;
    const uint32_t *ev_off;
    const uint64_t *ev_base;
    uint64_t cap;
    void *events;
    uint32_t *view;                // counted views: the caller's cells, a grid `up` times finer than the frame (NULL: events)
    uint64_t view_cells;
    uint32_t up;
    const int32_t *shifts;         // aligned views: frame f's (dy, dx) in cells of the view at [2 * f], [2 * f + 1] (NULL: none)
    int *err;
};

// (workgroup-uniform) the ids the kernels are about to index the workspace with all lie below id_cap: the host sized it from what the
// streams can hold, k_expand_bases has checked the streams against the count
__device__ __forceinline__ bool cnt_gate(const CntArgs &A) { return *A.err == 0 && A.frame_base[A.n] <= A.id_cap; }

__device__ __forceinline__ uint32_t cnt_find(uint32_t *__restrict__ parent, uint32_t x)
{
    uint32_t p = __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    while (p != 0) {                       // p - 1 < x: the walk descends
        const uint32_t gp = __hip_atomic_load(parent + (p - 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (gp != 0) __hip_atomic_store(parent + x, gp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // path halving: still an ancestor, still smaller
        x = p - 1;
        p = gp;
    }
    return x;
}
__device__ __attribute__((noinline)) void cnt_union(uint32_t *__restrict__ parent, uint32_t a, uint32_t b)
{
    for (;;) {
        a = cnt_find(parent, a);
        b = cnt_find(parent, b);
        if (a == b) return;
        if (a > b) { const uint32_t t = a; a = b; b = t; }
        const uint32_t old = atomicCAS(parent + b, 0u, a + 1u);    // on a root only
        if (old == 0) return;
        b = old - 1;                                               // b was hung meanwhile, under something smaller than b: go on from there
    }
}

// the frame as a kernel's lane sees it
struct CntFrame {
    const uint8_t *bm;
    const uint32_t *dir;
    uint32_t base;       // frame_base[f]
    uint64_t nb8, N;
    __device__ __forceinline__ uint64_t word(uint32_t wi) const { return expand_word(bm, nb8, N, wi); }
    __device__ __forceinline__ bool set(uint32_t q) const { return (word(q >> 6) >> (q & 63u)) & 1ull; }
    // rank in the frame of the set pixel at q
    __device__ __forceinline__ uint32_t rank(uint32_t q) const { return dir[q >> 6] + (uint32_t)__builtin_popcountll(word(q >> 6) & ((1ull << (q & 63u)) - 1ull)); }
};
__device__ __forceinline__ CntFrame cnt_frame(const CntArgs &A, uint32_t f)
{
    return CntFrame{A.bm + f * A.bm_stride, A.dir + (uint64_t)f * A.nblk * WG, (uint32_t)A.frame_base[f], A.nb8, A.N};
}

// Walks the set pixels of the lane's word in raster order: position p in the frame, row, column and rank (one division per word, the
// pixels behind the first step the column - as k_expand_emit_b).
struct CntWalk {
    uint64_t bits;
    uint32_t p0, row, col, prev, r;
    __device__ __forceinline__ CntWalk(uint64_t w, uint64_t i, uint32_t nx, uint32_t rank0) : bits(w), p0((uint32_t)(i * 64)), row(0), col(0), prev(0), r(rank0)
    {
        if (bits) { row = p0 / nx; col = p0 - row * nx; }
    }
    __device__ __forceinline__ bool next(uint32_t nx, uint32_t &p, uint32_t &rank)
    {
        if (!bits) return false;
        const uint32_t b = (uint32_t)__builtin_ctzll(bits);
        bits &= bits - 1;
        col += b - prev;
        prev = b;
        while (col >= nx) { col -= nx; ++row; }      // (at most 64 / nx + 1 rows per word in total)
        p = p0 + b;
        rank = r++;
        return true;
    }
};

__global__ __launch_bounds__(WG) void k_cnt_dir(CntArgs A)
{
    __shared__ uint32_t sm[WAVES + 1];
    if (*A.err) return;
    if (A.frame_base[A.n] > A.id_cap) {       // (cannot happen: see cnt_gate; if it does the batch is refused, not indexed)
        if (threadIdx.x == 0) atomicOr(A.err, 1);
        return;
    }
    const uint32_t f = blockIdx.y;
    const uint64_t i = (uint64_t)blockIdx.x * WG + threadIdx.x;
    uint32_t tot;
    const uint32_t local = block_excl_scan((uint32_t)__builtin_popcountll(expand_word(A.bm + f * A.bm_stride, A.nb8, A.N, i)), sm, &tot);
    A.dir[(uint64_t)f * A.nblk * WG + i] = A.blk_off[(uint64_t)f * A.nblk + blockIdx.x] + local;
}

// W's upper neighbours are NW and N, N's side neighbours are NW and NE: with W and N linked, NW and NE hang on them through their own
// links.  So: W if set; N if set; otherwise NE if set, and NW if set and W is clear.  The first column has no W / NW, the last no NE, the
// first row of a frame no upper neighbour at all - tested on row and column, never on p alone.
__global__ __launch_bounds__(WG) void k_cnt_link(CntArgs A)
{
    if (!cnt_gate(A)) return;
    const uint32_t f = blockIdx.y;
    const uint64_t i = (uint64_t)blockIdx.x * WG + threadIdx.x;
    const CntFrame F = cnt_frame(A, f);
    const uint64_t w = expand_word(F.bm, A.nb8, A.N, i);
    if (!w) return;
    const uint32_t nx = A.nx;
    CntWalk it(w, i, nx, F.dir[i]);
    uint32_t p, rank;
    while (it.next(nx, p, rank)) {
        const uint32_t self = F.base + rank;
        const bool has_w = it.col > 0, has_up = it.row > 0, has_e = it.col + 1 < nx;
        const bool W = has_w && F.set(p - 1);
        const bool Nn = has_up && F.set(p - nx);
        if (W) cnt_union(A.parent, self, self - 1);              // (ranks are consecutive along a row)
        if (Nn) cnt_union(A.parent, self, F.base + F.rank(p - nx));
        else if (has_up) {
            if (!W && has_w && F.set(p - nx - 1)) cnt_union(A.parent, self, F.base + F.rank(p - nx - 1));
            if (has_e && F.set(p - nx + 1)) cnt_union(A.parent, self, F.base + F.rank(p - nx + 1));
        }
    }
}

__device__ __forceinline__ unsigned long long cnt_wave_sum(unsigned long long v)
{
#pragma unroll
    for (int d = 32; d; d >>= 1) v += __shfl_xor(v, d);
    return v;
}
__device__ __forceinline__ unsigned long long cnt_wave_max(unsigned long long v)
{
#pragma unroll
    for (int d = 32; d; d >>= 1) { const unsigned long long o = __shfl_xor(v, d); v = o > v ? o : v; }
    return v;
}

// a lane's pending terms for one root
template <uint32_t M>
struct CntPend {
    uint32_t root = 0, area = 0;
    unsigned long long a = 0, b = 0, w = 0, za = 0, zb = 0;
    __device__ __forceinline__ void add(uint32_t v, uint32_t row, uint32_t col, uint32_t p)
    {
        ++area;
        w += v;
        if (M == CNT_WEIGHTED) {
            a += (unsigned long long)v * row;
            b += (unsigned long long)v * col;
            if (v == 0) { za += row; zb += col; }
        } else if (M == CNT_UNWEIGHTED) { a += row; b += col; }
        else { const unsigned long long k = cnt_max_key(v, p); a = k > a ? k : a; }
    }
    __device__ __forceinline__ void flush(const CntArgs &A)
    {
        if (!area) return;
        unsigned long long *s = A.acc + root;
        (void)atomicAdd(A.area + root, area);
        if (M == CNT_MAX) (void)atomicMax(s, a);
        else {
            if (a) (void)atomicAdd(s, a);
            if (b) (void)atomicAdd(s + A.id_cap, b);
        }
        if (w) (void)atomicAdd(s + (M == CNT_MAX ? 1 : 2) * A.id_cap, w);
        if (M == CNT_WEIGHTED && za) (void)atomicAdd(s + 3 * A.id_cap, za);
        if (M == CNT_WEIGHTED && zb) (void)atomicAdd(s + 4 * A.id_cap, zb);
        area = 0; a = b = w = za = zb = 0;
    }
};

constexpr uint32_t CNT_JOIN_MIN = 8;      // lanes on one root from which the wave adds them up first (6 shuffle steps per sum against one atomic per lane)

template <uint32_t M>
__global__ __launch_bounds__(WG) void k_cnt_acc(CntArgs A)
{
    if (!cnt_gate(A)) return;
    const uint32_t f = blockIdx.y;
    const uint64_t i = (uint64_t)blockIdx.x * WG + threadIdx.x;
    const CntFrame F = cnt_frame(A, f);
    const uint64_t w = expand_word(F.bm, A.nb8, A.N, i);
    const uint32_t nx = A.nx;
    const uint8_t *pix = A.pv + f * A.pv_stride;
    const uint64_t pix_bytes = A.level == 1 ? A.pv_bytes[f] : 0;
    const uint32_t dmask = A.level == 1 ? (1u << A.d) - 1u : 0u;       // (level 1: 1 <= d <= 16)
    CntPend<M> P;
    CntWalk it(w, i, nx, w ? F.dir[i] : 0u);
    uint32_t p, rank;
    while (it.next(nx, p, rank)) {
        const uint32_t root = cnt_find(A.parent, F.base + rank);
        const uint32_t v = A.level == 1 ? expand_field16(pix, pix_bytes, rank, A.d, dmask) : 1u;
        if (root != P.root) { P.flush(A); P.root = root; }
        P.add(v, it.row, it.col, p);
    }
    // every lane of the wave is here, each with at most one root's terms left
    const uint32_t lane = (uint32_t)lane_id();
    bool pending = P.area != 0;
    for (uint64_t rem = __builtin_amdgcn_ballot_w64(pending); rem;) {
        const uint32_t leader = (uint32_t)__builtin_ctzll(rem);
        const uint32_t r = (uint32_t)__shfl((int)P.root, (int)leader);
        const bool in = pending && P.root == r;
        const uint64_t same = __builtin_amdgcn_ballot_w64(in);
        if (__builtin_popcountll(same) >= CNT_JOIN_MIN) {         // (uniform)
            const unsigned long long area = cnt_wave_sum(in ? P.area : 0u), ws = cnt_wave_sum(in ? P.w : 0ull);
            const unsigned long long a = M == CNT_MAX ? cnt_wave_max(in ? P.a : 0ull) : cnt_wave_sum(in ? P.a : 0ull);
            const unsigned long long b = M == CNT_MAX ? 0ull : cnt_wave_sum(in ? P.b : 0ull);
            const unsigned long long za = M == CNT_WEIGHTED ? cnt_wave_sum(in ? P.za : 0ull) : 0ull;
            const unsigned long long zb = M == CNT_WEIGHTED ? cnt_wave_sum(in ? P.zb : 0ull) : 0ull;
            if (lane == leader) { P.area = (uint32_t)area; P.w = ws; P.a = a; P.b = b; P.za = za; P.zb = zb; }
            else if (in) { pending = false; P.area = 0; }
        }
        rem &= ~same;
    }
    if (pending) P.flush(A);
}

// bit b set: the word's pixel b is a root whose component passes the threshold
__device__ __forceinline__ uint64_t cnt_keep_mask(const CntArgs &A, const CntFrame &F, uint64_t w, uint64_t i)
{
    uint64_t keep = 0;
    if (!w) return 0;
    uint32_t id = F.base + F.dir[i];
    for (uint64_t bits = w; bits; bits &= bits - 1, ++id)
        if (A.parent[id] == 0 && A.area[id] > A.thr) keep |= bits & (0 - bits);
    return keep;
}

__global__ __launch_bounds__(WG) void k_cnt_roots(CntArgs A)
{
    __shared__ uint32_t sm[WAVES + 1];
    if (!cnt_gate(A)) return;
    const uint32_t f = blockIdx.y;
    const uint64_t i = (uint64_t)blockIdx.x * WG + threadIdx.x;
    const CntFrame F = cnt_frame(A, f);
    const uint64_t keep = cnt_keep_mask(A, F, expand_word(F.bm, A.nb8, A.N, i), i);
    uint32_t tot;
    (void)block_excl_scan((uint32_t)__builtin_popcountll(keep), sm, &tot);
    if (threadIdx.x == 0) A.ev_cnt[(uint64_t)f * A.nblk + blockIdx.x] = tot;
}

// the sums of root `id` as k_cnt_acc<M> left them
template <uint32_t M>
__device__ __forceinline__ CntSums cnt_sums(const CntArgs &A, uint32_t id)
{
    const unsigned long long *s = A.acc + id;
    CntSums S;
    S.area = A.area[id];
    S.a = s[0];
    S.b = M == CNT_MAX ? 0 : s[A.id_cap];
    S.w = s[(M == CNT_MAX ? 1 : 2) * A.id_cap];
    S.za = M == CNT_WEIGHTED ? s[3 * A.id_cap] : 0;
    S.zb = M == CNT_WEIGHTED ? s[4 * A.id_cap] : 0;
    return S;
}

// events = uint64 weight[cap] | int32 rows[cap] | int32 cols[cap] | uint32 area[cap]
template <uint32_t M>
__global__ __launch_bounds__(WG) void k_cnt_emit(CntArgs A)
{
    __shared__ uint32_t sm[WAVES + 1];
    if (!cnt_gate(A)) return;           // (also: k_expand_bases found more events than cap)
    const uint32_t f = blockIdx.y;
    const uint64_t i = (uint64_t)blockIdx.x * WG + threadIdx.x;
    const CntFrame F = cnt_frame(A, f);
    const uint64_t w = expand_word(F.bm, A.nb8, A.N, i);
    uint64_t keep = cnt_keep_mask(A, F, w, i);
    uint32_t tot;
    const uint32_t local = block_excl_scan((uint32_t)__builtin_popcountll(keep), sm, &tot);
    if (!keep) return;
    uint64_t e = A.ev_base[f] + A.ev_off[(uint64_t)f * A.nblk + blockIdx.x] + local;
    uint64_t *o_w = static_cast<uint64_t *>(A.events);
    int32_t *o_row = reinterpret_cast<int32_t *>(o_w + A.cap), *o_col = o_row + A.cap;
    uint32_t *o_area = reinterpret_cast<uint32_t *>(o_col + A.cap);
    const uint32_t id0 = F.base + F.dir[i];
    for (; keep; keep &= keep - 1, ++e) {
        if (e >= A.cap) break;
        const uint32_t b = (uint32_t)__builtin_ctzll(keep);
        const uint32_t id = id0 + (uint32_t)__builtin_popcountll(w & ((1ull << b) - 1ull));
        const CntSums S = cnt_sums<M>(A, id);
        int32_t row, col;
        cnt_finish(M, S, A.nx, &row, &col);
        o_w[e] = S.w;
        o_row[e] = row;
        o_col[e] = col;
        o_area[e] = S.area;
    }
}

// Counted views: k_cnt_roots and k_cnt_emit in one pass, and no event.  Every kept root of the lane's word is finished on the finer grid
// (cnt_finish_fine) and counted into its cell with one 32-bit no-return atomic - the cells belong to the caller's handle, other batches
// and earlier calls have added to them, and several components of a frame may share one (a ring around a dot).  The block's number of
// events goes to ev_cnt for the frames' event prefix.  A centroid lies inside its frame, so a cell inside the view (cnt_place); an
// index that did not would be dropped, not written.  With shifts (rc_sum_add_counted_shifted) the cell is translated by the frame's (dy, dx)
// fine cells, in 64 bits - any int32 pair is legal -, and a count that leaves the view is dropped; the block's number of events is not.
template <uint32_t M>
__global__ __launch_bounds__(WG) void k_cnt_place(CntArgs A)
{
    __shared__ uint32_t sm[WAVES + 1];
    if (!cnt_gate(A)) return;
    const uint32_t f = blockIdx.y;
    const uint64_t i = (uint64_t)blockIdx.x * WG + threadIdx.x;
    const CntFrame F = cnt_frame(A, f);
    const uint64_t w = expand_word(F.bm, A.nb8, A.N, i);
    uint64_t keep = cnt_keep_mask(A, F, w, i);
    uint32_t tot;
    (void)block_excl_scan((uint32_t)__builtin_popcountll(keep), sm, &tot);
    if (threadIdx.x == 0) A.ev_cnt[(uint64_t)f * A.nblk + blockIdx.x] = tot;
    if (!keep) return;
    const uint32_t id0 = F.base + F.dir[i];
    const uint64_t fnx = (uint64_t)A.up * A.nx;
    for (; keep; keep &= keep - 1) {
        const uint32_t b = (uint32_t)__builtin_ctzll(keep);
        const uint32_t id = id0 + (uint32_t)__builtin_popcountll(w & ((1ull << b) - 1ull));
        uint32_t frow, fcol;
        cnt_finish_fine(M, cnt_sums<M>(A, id), A.nx, A.up, &frow, &fcol);
        if (A.shifts) {
            const int64_t row = (int64_t)frow + A.shifts[2 * f], col = (int64_t)fcol + A.shifts[2 * f + 1];
            if (row >= 0 && col >= 0 && col < (int64_t)fnx && row < (int64_t)(A.view_cells / fnx)) (void)atomicAdd(A.view + (uint64_t)row * fnx + (uint64_t)col, 1u);
            continue;
        }
        const uint64_t cell = frow * fnx + fcol;
        if (fcol < fnx && cell < A.view_cells) (void)atomicAdd(A.view + cell, 1u);
    }
}

// workspace: uint64 ev_nnz[n] | ev_base[n + 1] | sums[words * id_cap] | uint32 parent[id_cap] | area[id_cap] | ev_cnt[n * nblk] |
// ev_off[n * nblk] | dir[n * nblk * WG]; sums .. ev_cnt rest at zero before the kernels run
struct CntLayout {
    uint64_t o_sums, o_parent, o_area, o_evcnt, o_evoff, o_dir, bytes;
};
CntLayout cnt_layout(uint64_t nb8, uint32_t n, uint64_t id_cap, uint32_t method)
{
    const uint64_t nblk = (nb8 + WG - 1) / WG;
    CntLayout L;
    L.o_sums = (2 * (uint64_t)n + 1) * 8;
    L.o_parent = L.o_sums + cnt_acc_words(method) * id_cap * 8;
    L.o_area = L.o_parent + id_cap * 4;
    L.o_evcnt = L.o_area + id_cap * 4;
    L.o_evoff = L.o_evcnt + n * nblk * 4;
    L.o_dir = L.o_evoff + n * nblk * 4;
    L.bytes = L.o_dir + n * nblk * WG * 4;
    return L;
}

template <uint32_t M>
void cnt_launch(const CntArgs &A, uint64_t nb8, uint64_t *ev_nnz, uint64_t *ev_base, uint32_t *ev_off, hipEvent_t order, hipStream_t s)
{
    const dim3 grid(A.nblk, A.n), wg(WG);
    hipLaunchKernelGGL(k_cnt_dir, grid, wg, 0, s, A);
    hipLaunchKernelGGL(k_cnt_link, grid, wg, 0, s, A);
    hipLaunchKernelGGL(k_cnt_acc<M>, grid, wg, 0, s, A);
    if (A.view) {
        (void)hipStreamWaitEvent(s, order, 0);
        hipLaunchKernelGGL(k_cnt_place<M>, grid, wg, 0, s, A);
        (void)hipEventRecord(order, s);
        launch_expand_batch_scan(A.ev_cnt, ev_off, nb8, A.n, ev_nnz, ev_base, ~0ull, A.err, s);
        return;
    }
    hipLaunchKernelGGL(k_cnt_roots, grid, wg, 0, s, A);
    launch_expand_batch_scan(A.ev_cnt, ev_off, nb8, A.n, ev_nnz, ev_base, A.events ? A.cap : ~0ull, A.err, s);
    if (A.events) hipLaunchKernelGGL(k_cnt_emit<M>, grid, wg, 0, s, A);
}

}  // namespace

uint64_t cnt_workspace_bytes(uint64_t nb8, uint32_t n, uint64_t id_cap, uint32_t method) { return cnt_layout(nb8, n, id_cap, method).bytes; }
uint64_t *cnt_ev_base(uint8_t *workspace, uint32_t n) { return reinterpret_cast<uint64_t *>(workspace) + n; }

namespace {
void cnt_run(const uint8_t *bm, uint64_t bm_stride, uint64_t nb8, uint64_t N, uint32_t nx, uint32_t n, const uint32_t *blk_off,
             const uint64_t *frame_base, const uint8_t *pv, uint64_t pv_stride, const uint32_t *pv_bytes, uint32_t d, uint32_t level, uint32_t method,
             uint32_t area_threshold, uint8_t *workspace, uint64_t id_cap, void *events, uint64_t cap, uint32_t *view, uint64_t view_cells,
             uint32_t upsample, const int32_t *shifts, hipEvent_t order, int *err, hipStream_t s)
{
    const CntLayout L = cnt_layout(nb8, n, id_cap, method);
    uint64_t *ev_nnz = reinterpret_cast<uint64_t *>(workspace), *ev_base = cnt_ev_base(workspace, n);
    uint32_t *ev_off = reinterpret_cast<uint32_t *>(workspace + L.o_evoff);
    CntArgs A;
    A.bm = bm; A.bm_stride = bm_stride; A.nb8 = nb8; A.N = N;
    A.nx = nx; A.nblk = (uint32_t)((nb8 + WG - 1) / WG); A.n = n;
    A.blk_off = blk_off; A.frame_base = frame_base;
    A.pv = pv; A.pv_stride = pv_stride; A.pv_bytes = pv_bytes;
    A.d = d; A.level = level; A.thr = area_threshold;
    A.id_cap = id_cap;
    A.dir = reinterpret_cast<uint32_t *>(workspace + L.o_dir);
    A.parent = reinterpret_cast<uint32_t *>(workspace + L.o_parent);
    A.area = reinterpret_cast<uint32_t *>(workspace + L.o_area);
    A.acc = reinterpret_cast<unsigned long long *>(workspace + L.o_sums);
    A.ev_cnt = reinterpret_cast<uint32_t *>(workspace + L.o_evcnt);
    A.ev_off = ev_off; A.ev_base = ev_base;
    A.cap = cap; A.events = events;
    A.view = view; A.view_cells = view_cells; A.up = upsample;
    A.shifts = shifts;
    A.err = err;
    (void)hipMemsetAsync(workspace + L.o_sums, 0, L.o_evoff - L.o_sums, s);
    if (method == CNT_WEIGHTED) cnt_launch<CNT_WEIGHTED>(A, nb8, ev_nnz, ev_base, ev_off, order, s);
    else if (method == CNT_UNWEIGHTED) cnt_launch<CNT_UNWEIGHTED>(A, nb8, ev_nnz, ev_base, ev_off, order, s);
    else cnt_launch<CNT_MAX>(A, nb8, ev_nnz, ev_base, ev_off, order, s);
}
}  // namespace

void launch_count_events(const uint8_t *bm, uint64_t bm_stride, uint64_t nb8, uint64_t N, uint32_t nx, uint32_t n, const uint32_t *blk_off,
                         const uint64_t *frame_base, const uint8_t *pv, uint64_t pv_stride, const uint32_t *pv_bytes, uint32_t d, uint32_t level,
                         uint32_t method, uint32_t area_threshold, uint8_t *workspace, uint64_t id_cap, void *events, uint64_t cap, int *err,
                         hipStream_t s)
{
    cnt_run(bm, bm_stride, nb8, N, nx, n, blk_off, frame_base, pv, pv_stride, pv_bytes, d, level, method, area_threshold, workspace, id_cap, events, cap,
            nullptr, 0, 1, nullptr, nullptr, err, s);
}

void launch_count_place(const uint8_t *bm, uint64_t bm_stride, uint64_t nb8, uint64_t N, uint32_t nx, uint32_t n, const uint32_t *blk_off,
                        const uint64_t *frame_base, const uint8_t *pv, uint64_t pv_stride, const uint32_t *pv_bytes, uint32_t d, uint32_t level,
                        uint32_t method, uint32_t area_threshold, uint8_t *workspace, uint64_t id_cap, uint32_t *view, uint64_t view_cells,
                        uint32_t upsample, hipEvent_t order, int *err, hipStream_t s, const int32_t *shifts)
{
    cnt_run(bm, bm_stride, nb8, N, nx, n, blk_off, frame_base, pv, pv_stride, pv_bytes, d, level, method, area_threshold, workspace, id_cap, nullptr, 0,
            view, view_cells, upsample, shifts, order, err, s);
}

}  // namespace rc
