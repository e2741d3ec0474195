// rc_inflate.hip - batched device inflate for the zlib streams of this library's device DEFLATE encoder (compression_scheme 0 written
// by a ctx with RC_SCHEME_ZLIB_DEVICE), behind rc_expand_frames(op_mode 1, scheme RC_SCHEME_ZLIB_DEVICE).  Replaces the stock inflate of
// the reference's reader (pyrecode/recode_reader.py:379-471: zlib.decompress of both streams, frame by frame) for n frames at once.
//
//   k_inf_candidates   a workgroup per stream: every byte position that may start a unit, compacted in position order
//   k_inf_map_sizes    a lane per candidate of a map stream: decode WITHOUT output -> its end -> the candidate that sits there (chain link)
//   k_inf_val<false>   a wavefront per candidate of a value stream: the same (a coded chunk: table in LDS, bits staged in LDS, one lane decodes)
//   k_inf_chain        a workgroup per stream: follow the links from the candidate at offset 2 (links staged in LDS) -> the units' candidates
//   k_inf_map_place    a lane per unit: decode again, into LDS, and the workgroup writes its 64 tiles to the decoded-streams buffer
//   k_inf_val<true>    a wavefront per unit: decode again (stored chunks: a copy), through an LDS stage, to the decoded-streams buffer
// The second decode goes straight to where rc_expand.hip's kernels expect mode-0 data (rc_reader.hip: bitmaps at f * bm_stride, value
// streams behind them); there are no per-candidate output slots.  Any violation of the streams' structure raises bit 8 of *err - "not
// this encoder's stream, use the stock decoder" - and the kernels behind it, the expand kernels among them, then write nothing.
// The decoding core and its safety contract: rc_inflate.h.
#include "rc_inflate.h"
#include "rc_launch.h"

#include <cstdio>
#include <cstdlib>

namespace rc {

constexpr int INF_ERR = 8;

__device__ __forceinline__ InfGlobalLoad inf_loader(const uint8_t *data, const InfStream &S)
{
    const uint32_t off = (uint32_t)(S.src & 3u);
    return InfGlobalLoad{reinterpret_cast<const uint32_t *>(data + (S.src - off)), (S.csize + off + 3u) >> 2};
}
// the bit position of byte p of the stream / the stream's trailer, as InfBits counts
__device__ __forceinline__ uint32_t inf_bit(const InfStream &S, uint32_t p) { return 8u * (p + (uint32_t)(S.src & 3u)); }

// index of the candidate at byte `end` of the stream (its sorted positions: pos[0 .. n)), INF_TERM for the trailer, INF_NONE otherwise
__device__ __forceinline__ uint32_t inf_link(const uint32_t *__restrict__ pos, uint32_t n, uint32_t end, uint32_t csize)
{
    if (end == csize - 4u) return INF_TERM;
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (pos[mid] < end) lo = mid + 1; else hi = mid;
    }
    return lo < n && pos[lo] == end ? lo : INF_NONE;
}

__global__ __launch_bounds__(WG) void k_inf_candidates(const uint8_t *__restrict__ data, const InfStream *__restrict__ streams,
                                                         uint32_t *__restrict__ cand_pos, uint32_t *__restrict__ ncand, int *__restrict__ err)
{
    __shared__ uint32_t sm[WAVES + 1];
    const InfStream S = streams[blockIdx.x];
    const uint8_t *p0 = data + S.src;
    auto at = [&](uint32_t q) { return (uint32_t)p0[q]; };
    uint32_t carry = 0;
    constexpr uint32_t PER = 16;                                     // positions per lane and pass: 4 KiB of the stream between two scans
    for (uint32_t base = 0; base < S.csize; base += PER * WG) {      // (workgroup-uniform)
        const uint32_t p = base + PER * threadIdx.x;
        uint32_t m = 0;
#pragma unroll
        for (uint32_t j = 0; j < PER; ++j)
            if (inf_is_candidate(at, p + j, S.csize, S.unit)) m |= 1u << j;
        uint32_t tot;
        uint32_t at_out = carry + block_excl_scan((uint32_t)__builtin_popcount(m), sm, &tot);
        for (; m; m &= m - 1, ++at_out)
            if (at_out < S.cap) cand_pos[S.cand0 + at_out] = p + (uint32_t)__builtin_ctz(m);
        carry += tot;
    }
    if (threadIdx.x == 0) {
        ncand[blockIdx.x] = min(carry, S.cap);
        if (carry > S.cap) atomicOr(err, INF_ERR);
    }
}

struct InfNoOut {
    __device__ __forceinline__ void put(uint32_t, uint32_t) {}
    __device__ __forceinline__ uint32_t get(uint32_t) { return 0; }
};

__global__ __launch_bounds__(WG) void k_inf_map_sizes(const uint8_t *__restrict__ data, const InfStream *__restrict__ streams,
                                                        const uint32_t *__restrict__ cand_pos, const uint32_t *__restrict__ ncand,
                                                        uint32_t *__restrict__ link)
{
    const InfStream S = streams[blockIdx.y];
    const uint32_t nc = ncand[blockIdx.y], c = blockIdx.x * WG + threadIdx.x;
    if (c >= nc) return;
    const uint32_t p = cand_pos[S.cand0 + c];
    InfBits<InfGlobalLoad> bits(inf_loader(data, S));
    uint32_t pos = inf_bit(S, p), regen = 0, bfinal = 0;
    InfNoOut none;
    const bool ok = p < S.csize && inf_map_unit<false>(bits, pos, inf_bit(S, S.csize - 4u), none, regen, bfinal);
    link[S.cand0 + c] = ok ? inf_link(cand_pos + S.cand0, nc, (pos >> 3) - (uint32_t)(S.src & 3u), S.csize) : INF_NONE;
}

// One workgroup per stream.  Unit k of the stream is the k-th candidate on the chain from candidate 0 (offset 2); the chain must have
// exactly S.units links and end at the trailer.  Links point forward, so the walk passes the table once: a window of it in LDS at a time.
constexpr uint32_t INF_CHAIN_WIN = 8192;
__global__ __launch_bounds__(WG) void k_inf_chain(const InfStream *__restrict__ streams, const uint32_t *__restrict__ ncand,
                                                    const uint32_t *__restrict__ link, uint32_t *__restrict__ unit_cand, int *__restrict__ err)
{
    __shared__ uint32_t win[INF_CHAIN_WIN];
    __shared__ uint32_t s_c, s_k, s_state;     // state: 0 walking, 1 done, 2 refused
    const InfStream S = streams[blockIdx.x];
    const uint32_t nc = ncand[blockIdx.x];
    if (threadIdx.x == 0) { s_c = 0; s_k = 0; s_state = nc ? 0u : 2u; }
    __syncthreads();
    while (s_state == 0) {                     // (every pass takes at least one link: at most nc passes)
        const uint32_t w0 = s_c, wn = min(INF_CHAIN_WIN, nc - w0);
        for (uint32_t i = threadIdx.x; i < wn; i += WG) win[i] = link[S.cand0 + w0 + i];
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t c = w0, k = s_k, state = 0;
            while (c - w0 < wn) {
                if (k >= S.units) { state = 2; break; }
                unit_cand[S.unit0 + k++] = c;
                const uint32_t nx = win[c - w0];
                if (nx == INF_TERM) { state = k == S.units ? 1u : 2u; break; }
                if (nx <= c || nx >= nc) { state = 2; break; }     // (INF_NONE among them)
                c = nx;
            }
            s_c = c; s_k = k; s_state = state;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0 && s_state == 2) atomicOr(err, INF_ERR);
}

// ---- place: the map's units -----------------------------------------------------------------------------------------------------
// 64 lanes, a unit each; lane u's dword w lives at LDS word w * 65 + u: lanes of one decode step and lanes of one output row both
// fall into different banks.
constexpr uint32_t INF_TILE_WORDS = INF_MAP_UNIT / 4;
struct InfLdsOut {
    uint32_t *lds;      // + lane
    uint32_t acc, cnt;
    __device__ __forceinline__ void put(uint32_t, uint32_t byte)      // (in order: the position is cnt)
    {
        acc |= byte << (8u * (cnt & 3u));
        if ((cnt & 3u) == 3u) { lds[(cnt >> 2) * 65u] = acc; acc = 0; }
        ++cnt;
    }
    __device__ __forceinline__ uint32_t get(uint32_t i)               // i < cnt <= INF_MAP_UNIT (checked by inf_map_unit)
    {
        const uint32_t wv = (i >> 2) == (cnt >> 2) ? acc : lds[(i >> 2) * 65u];
        return (wv >> (8u * (i & 3u))) & 0xFFu;
    }
};
__global__ __launch_bounds__(64) void k_inf_map_place(const uint8_t *__restrict__ data, const InfStream *__restrict__ streams,
                                                        const uint32_t *__restrict__ cand_pos, const uint32_t *__restrict__ ncand,
                                                        const uint32_t *__restrict__ unit_cand, uint8_t *__restrict__ out, int *__restrict__ err)
{
    __shared__ uint32_t tile[INF_TILE_WORDS * 65];
    if (*err) return;        // (workgroup-uniform: every kernel that raises it has finished)
    const InfStream S = streams[blockIdx.y];
    const uint32_t k0 = blockIdx.x * 64u, k = k0 + threadIdx.x;
    for (uint32_t i = threadIdx.x; i < INF_TILE_WORDS * 65; i += 64) tile[i] = 0;
    __syncthreads();
    if (k < S.units) {
        const uint32_t c = unit_cand[S.unit0 + k], want = min(INF_MAP_UNIT, S.size - min(S.size, k * INF_MAP_UNIT));
        bool ok = c < ncand[blockIdx.y];
        if (ok) {
            const uint32_t p = cand_pos[S.cand0 + c];
            InfBits<InfGlobalLoad> bits(inf_loader(data, S));
            InfLdsOut o{tile + threadIdx.x, 0u, 0u};
            uint32_t pos = inf_bit(S, p), regen = 0, bfinal = 0;
            ok = p < S.csize && inf_map_unit<true>(bits, pos, inf_bit(S, S.csize - 4u), o, regen, bfinal) && regen == want &&
                 bfinal == (k + 1 == S.units ? 1u : 0u);
            if (o.cnt & 3u) o.lds[(o.cnt >> 2) * 65u] = o.acc;
        }
        if (!ok) atomicOr(err, INF_ERR);
    }
    __syncthreads();
    uint32_t *dst = reinterpret_cast<uint32_t *>(out + S.dst);
    for (uint32_t j = threadIdx.x; j < 64u * INF_TILE_WORDS; j += 64) {
        const uint32_t u = j / INF_TILE_WORDS, w = j % INF_TILE_WORDS, kk = k0 + u;
        if (kk >= S.units) break;
        const uint32_t have = min(INF_MAP_UNIT, S.size - min(S.size, kk * INF_MAP_UNIT));
        if (4u * w < have) dst[(uint64_t)kk * INF_TILE_WORDS + w] = tile[w * 65u + u];
    }
}

// ---- the value stream's candidates / units: a wavefront each -----------------------------------------------------------------------
constexpr uint32_t INF_WIN_WORDS = 1024, INF_WIN_MARGIN = 4, INF_STAGE = 4096;
struct InfLdsLoad {
    const uint32_t *win;
    uint32_t w0;
    __device__ __forceinline__ uint32_t operator()(uint32_t w) const { return w - w0 < INF_WIN_WORDS + INF_WIN_MARGIN ? win[w - w0] : 0u; }
};
template <bool PLACE>
__global__ __launch_bounds__(64) void k_inf_val(const uint8_t *__restrict__ data, const InfStream *__restrict__ streams,
                                                  const uint32_t *__restrict__ cand_pos, const uint32_t *__restrict__ ncand,
                                                  uint32_t *__restrict__ link, const uint32_t *__restrict__ unit_cand, uint8_t *__restrict__ out,
                                                  int *__restrict__ err)
{
    __shared__ InfDyn D;
    __shared__ uint32_t win[INF_WIN_WORDS + INF_WIN_MARGIN];
    __shared__ uint32_t stage[PLACE ? INF_STAGE / 4 : 1];
    __shared__ uint32_t s_state, s_pos, s_n, s_bf;
    if (PLACE && *err) return;
    const InfStream S = streams[blockIdx.y];
    const uint32_t nc = ncand[blockIdx.y], lane = threadIdx.x;
    uint32_t c = blockIdx.x, want = INF_VAL_UNIT, last = 0;
    if (PLACE) {
        if (blockIdx.x >= S.units) return;
        c = unit_cand[S.unit0 + blockIdx.x];
        want = min(INF_VAL_UNIT, S.size - min(S.size, blockIdx.x * INF_VAL_UNIT));
        last = blockIdx.x + 1 == S.units ? 1u : 0u;
    }
    if (c >= nc) {
        if (PLACE && lane == 0) atomicOr(err, INF_ERR);
        return;
    }
    const uint32_t p = cand_pos[S.cand0 + c], lim = inf_bit(S, S.csize - 4u), off = (uint32_t)(S.src & 3u);
    const InfGlobalLoad gl = inf_loader(data, S);
    InfBits<InfGlobalLoad> gbits(gl);
    uint32_t pos = inf_bit(S, p), regen = 0, bfinal = 0;
    uint8_t *dst = out + S.dst + (uint64_t)blockIdx.x * INF_VAL_UNIT;       // (PLACE only)
    bool ok = p < S.csize - 4u;
    const uint32_t btype = ok ? (gbits.peek(pos) >> 1) & 3u : 3u;           // (wave-uniform, like everything up to the decode loop)
    if (btype == 0u) {
        ok = inf_stored_header(gbits, pos, lim, INF_VAL_UNIT, regen, bfinal);
        if (PLACE && ok && regen == want) {
            // the bytes start at stream byte pos / 8: dwords of the destination from the two aligned dwords under them
            const uint32_t b0 = pos >> 3, sh = b0 & 3u;
            uint32_t *d32 = reinterpret_cast<uint32_t *>(dst);
            for (uint32_t i = lane; 4u * i < regen; i += 64) {
                const uint32_t lo = gl((b0 >> 2) + i), hi = sh ? gl((b0 >> 2) + i + 1) : 0u;
                uint32_t v = __builtin_amdgcn_alignbyte(hi, lo, sh);
                if (4u * i + 4u > regen) v &= (1u << (8u * (regen - 4u * i))) - 1u;
                d32[i] = v;
            }
        }
        pos += 8u * regen;
    } else if (btype == 2u) {
        uint32_t w0 = pos >> 5, flushed = 0;
        for (uint32_t i = lane; i < INF_WIN_WORDS + INF_WIN_MARGIN; i += 64) win[i] = gl(w0 + i);
        __syncthreads();
        if (lane == 0) {
            InfBits<InfLdsLoad> lb(InfLdsLoad{win, w0});
            uint32_t q = pos, bf = 0;
            // (a header of the subset ends far inside the first window; one that would not is refused by the bound on its bits)
            const bool h = inf_dyn_header(lb, q, min(lim, pos + INF_DYN_HEADER_BITS), D, bf);
            s_state = h ? (uint32_t)INF_MORE : (uint32_t)INF_FAIL; s_pos = q; s_n = 0; s_bf = bf;
        }
        __syncthreads();
        bfinal = s_bf;
        uint32_t state = s_state;
        pos = s_pos;
        __syncthreads();
        while (state == INF_MORE) {            // (every pass consumes bits or flushes the stage: bounded by the stream's bits + want / INF_STAGE)
            if ((pos >> 5) != w0) {
                w0 = pos >> 5;
                for (uint32_t i = lane; i < INF_WIN_WORDS + INF_WIN_MARGIN; i += 64) win[i] = gl(w0 + i);
                __syncthreads();
            }
            if (lane == 0) {
                InfBits<InfLdsLoad> lb(InfLdsLoad{win, w0});
                uint32_t q = pos, n = s_n;
                uint8_t *st8 = reinterpret_cast<uint8_t *>(stage);
                const int r = inf_literals(lb, q, 32u * (w0 + INF_WIN_WORDS), lim, D, n, PLACE ? flushed + INF_STAGE : want + 1u, want,
                                           [&](uint32_t at, uint32_t byte) { if (PLACE) st8[at - flushed] = (uint8_t)byte; });
                s_state = (uint32_t)r; s_pos = q; s_n = n;
            }
            __syncthreads();
            state = s_state; pos = s_pos;
            const uint32_t n = s_n;
            if (PLACE && state != INF_FAIL && (n - flushed == INF_STAGE || state == INF_DONE)) {
                const uint32_t m = n - flushed;                 // <= INF_STAGE, and flushed + m <= want
                uint32_t *d32 = reinterpret_cast<uint32_t *>(dst + flushed);
                for (uint32_t i = lane; 4u * i < m; i += 64) {
                    uint32_t v = stage[i];
                    if (4u * i + 4u > m) v &= (1u << (8u * (m - 4u * i))) - 1u;
                    d32[i] = v;
                }
                flushed = n;
            }
            __syncthreads();
            regen = n;
        }
        ok = state == INF_DONE && inf_close(gbits, pos, lim, bfinal);
    } else
        ok = false;
    if (PLACE) {
        if (lane == 0 && !(ok && regen == want && bfinal == last)) atomicOr(err, INF_ERR);
    } else if (lane == 0)
        link[S.cand0 + c] = ok ? inf_link(cand_pos + S.cand0, nc, (pos >> 3) - off, S.csize) : INF_NONE;
}

void launch_inflate(const uint8_t *data, const InfStream *streams, uint32_t n_map, uint32_t n_val, uint32_t map_cap_max, uint32_t map_units_max,
                    uint32_t val_cap_max, uint32_t val_units_max, uint32_t *cand_pos, uint32_t *ncand, uint32_t *link, uint32_t *unit_cand,
                    uint8_t *out, int *err, hipStream_t s)
{
    const uint32_t ns = n_map + n_val;
    // RC_READ_TIMING (development): every kernel between two events, the stream waited for and the times printed - the call is then no longer asynchronous
    static const bool timing = getenv("RC_READ_TIMING") != nullptr;
    hipEvent_t ev[7] = {};
    int nev = 0;
    auto mark = [&] {
        if (timing && hipEventCreate(&ev[nev]) == hipSuccess) { (void)hipEventRecord(ev[nev], s); ++nev; }
    };
    mark();
    hipLaunchKernelGGL(k_inf_candidates, dim3(ns), dim3(WG), 0, s, data, streams, cand_pos, ncand, err);
    mark();
    hipLaunchKernelGGL(k_inf_map_sizes, dim3((map_cap_max + WG - 1) / WG, n_map), dim3(WG), 0, s, data, streams, cand_pos, ncand, link);
    mark();
    if (n_val)
        hipLaunchKernelGGL(k_inf_val<false>, dim3(val_cap_max, n_val), dim3(64), 0, s, data, streams + n_map, cand_pos, ncand + n_map, link, nullptr,
                           nullptr, err);
    mark();
    hipLaunchKernelGGL(k_inf_chain, dim3(ns), dim3(WG), 0, s, streams, ncand, link, unit_cand, err);
    mark();
    hipLaunchKernelGGL(k_inf_map_place, dim3((map_units_max + 63) / 64, n_map), dim3(64), 0, s, data, streams, cand_pos, ncand, unit_cand, out, err);
    mark();
    if (n_val)
        hipLaunchKernelGGL(k_inf_val<true>, dim3(val_units_max, n_val), dim3(64), 0, s, data, streams + n_map, cand_pos, ncand + n_map, nullptr,
                           unit_cand, out, err);
    mark();
    if (nev == 7 && hipEventSynchronize(ev[6]) == hipSuccess) {
        float ms[6] = {};
        for (int i = 0; i < 6; ++i) (void)hipEventElapsedTime(&ms[i], ev[i], ev[i + 1]);
        fprintf(stderr, "rc_inflate: streams %u, candidates %.3f ms, map sizes %.3f, value sizes %.3f, chain %.3f, map place %.3f, value place %.3f\n", ns, ms[0],
                ms[1], ms[2], ms[3], ms[4], ms[5]);
    }
    for (int i = 0; i < nev; ++i) (void)hipEventDestroy(ev[i]);
}

}  // namespace rc
