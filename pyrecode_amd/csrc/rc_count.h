// rc_count.h - electron counting (rc_count.hip): what turns one connected component's integer sums into its event - or into its cell of a
// counted view on a finer grid -, host and device, and the launchers of the kernels.  The arithmetic compiles as plain C++
// (tests/native/count_centroid_check.cpp and count_place_check.cpp run it under the sanitizers).
//
// Reference: pyrecode/utils/converters.py - l1_to_l4_converter (:59-123) and its helpers _get_centroids_2d_nb_w (:167-197, weighted average),
// _get_centroids_2d_nb_u (:200-226, unweighted) and _get_centroids_2d_nb_m (:229-259, maximum).  The reference accumulates in float32 and
// rounds with np.round (:92); here the sums are exact integers and the quotient is rounded from quotient and remainder.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RC_COUNT_HD __host__ __device__ inline
#else
#define RC_COUNT_HD inline
#endif

namespace rc {

constexpr uint32_t CNT_WEIGHTED = 0, CNT_UNWEIGHTED = 1, CNT_MAX = 2;   // `method` of rc_count_frames

// S / w (w > 0) rounded to the nearest integer, ties to the even one - np.round of the exact rational.  The remainder is compared with
// what is left of the divisor (r against w - r), so no intermediate can pass 64 bits whatever S and w are.
RC_COUNT_HD uint64_t cnt_rhe(uint64_t S, uint64_t w)
{
    const uint64_t q = S / w, r = S - q * w, rest = w - r;   // r < w: rest >= 1
    if (r > rest) return q + 1;
    if (r < rest) return q;
    return q + (q & 1u);
}

// The same centroid S / w on a grid s times finer (1 <= s <= 16): pixel centres lie at integers, fine cell k has its centre at
// (k - (s - 1) / 2) / s, and the result is the cell whose centre is nearest - the exact rational u = (2 s S + (s - 1) w) / (2 w) rounded
// to the nearest integer, ties to the even one.  s = 1 is cnt_rhe.  Domain: w < 2^48 (values of 16 bits, areas below 2^32) and
// S <= 65535 w (the centroid lies inside a frame); there every intermediate stays below 2^64 without a 128-bit type: with S = q w + r,
// u = s q + (2 s r + (s - 1) w) / (2 w), whose numerator is below 2^5 2^48 + 2^4 2^48.  The parity of the TOTAL decides a tie.
RC_COUNT_HD uint64_t cnt_place(uint64_t S, uint64_t w, uint32_t s)
{
    const uint64_t q = S / w, r = S - q * w;
    const uint64_t num = 2 * (uint64_t)s * r + (uint64_t)(s - 1) * w, den = 2 * w;      // num < 3 s w < 2^54
    const uint64_t qq = num / den, rem = num - qq * den, rest = den - rem;              // rem < den: rest >= 1
    const uint64_t t = (uint64_t)s * q + qq;
    if (rem > rest) return t + 1;
    if (rem < rest) return t;
    return t + (t & 1u);
}

// A component's sums.  a, b by method: weighted = sum of v * row, v * col; unweighted = sum of row, col; maximum = a is the largest key
// (cnt_max_key) of its pixels, b unused.  w = sum of v, area = pixels.  za, zb (weighted only) = sum of row, col over the pixels whose v
// is 0: a component of weight 0 consists of nothing else, so they are its unweighted sums.
struct CntSums {
    uint64_t a, b, w, za, zb;
    uint32_t area;
};

// maximum: larger v wins, among equal v the earlier pixel (p = row * nx + col < 2^32 - 1, so a key is never 0 and 0 means "none yet")
RC_COUNT_HD uint64_t cnt_max_key(uint32_t v, uint32_t p) { return ((uint64_t)v << 32) | (uint64_t)(0xFFFFFFFFu - p); }

// the event's pixel.  area >= 1.
RC_COUNT_HD void cnt_finish(uint32_t method, const CntSums &s, uint32_t nx, int32_t *row, int32_t *col)
{
    if (method == CNT_MAX) {
        const uint32_t p = 0xFFFFFFFFu - (uint32_t)s.a;
        *row = (int32_t)(p / nx);
        *col = (int32_t)(p % nx);
    } else if (method == CNT_WEIGHTED && s.w != 0) {
        *row = (int32_t)cnt_rhe(s.a, s.w);
        *col = (int32_t)cnt_rhe(s.b, s.w);
    } else {   // unweighted, or weighted with nothing to weigh by
        *row = (int32_t)cnt_rhe(method == CNT_WEIGHTED ? s.za : s.a, s.area);
        *col = (int32_t)cnt_rhe(method == CNT_WEIGHTED ? s.zb : s.b, s.area);
    }
}

// the event's cell on the grid s times finer (counted views): cnt_finish with cnt_place in the place of cnt_rhe; the maximum's pixel
// is placed by its centre
RC_COUNT_HD void cnt_finish_fine(uint32_t method, const CntSums &s, uint32_t nx, uint32_t up, uint32_t *frow, uint32_t *fcol)
{
    if (method == CNT_MAX) {
        const uint32_t p = 0xFFFFFFFFu - (uint32_t)s.a;
        *frow = (uint32_t)cnt_place(p / nx, 1, up);
        *fcol = (uint32_t)cnt_place(p % nx, 1, up);
    } else if (method == CNT_WEIGHTED && s.w != 0) {
        *frow = (uint32_t)cnt_place(s.a, s.w, up);
        *fcol = (uint32_t)cnt_place(s.b, s.w, up);
    } else {   // unweighted, or weighted with nothing to weigh by
        *frow = (uint32_t)cnt_place(method == CNT_WEIGHTED ? s.za : s.a, s.area, up);
        *fcol = (uint32_t)cnt_place(method == CNT_WEIGHTED ? s.zb : s.b, s.area, up);
    }
}

}  // namespace rc

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
namespace rc {
// 64-bit accumulators per set pixel by method (CntSums: a, b, w, za, zb | a, b, w | a, w), next to a uint32 parent and a uint32 area
constexpr uint32_t cnt_acc_words(uint32_t method) { return method == CNT_WEIGHTED ? 5u : method == CNT_UNWEIGHTED ? 3u : 2u; }
// bytes of workspace for n frames whose set pixels number at most id_cap (ids: frame_base[f] + rank; id_cap < 2^32 - 1)
uint64_t cnt_workspace_bytes(uint64_t nb8, uint32_t n, uint64_t id_cap, uint32_t method);
// where the frames' event prefix (n + 1 entries) lies in the workspace once the kernels have run
uint64_t *cnt_ev_base(uint8_t *workspace, uint32_t n);
// Behind launch_expand_batch_count on the same stream (blk_off, frame_base, *err as the gate): labels the n frames' set pixels, reduces
// every component and writes the events that pass area_threshold as uint64 weight[cap] | int32 rows[cap] | int32 cols[cap] |
// uint32 area[cap] (events == NULL: counts only).  More events than cap raise bit 1 of *err and nothing is written.
void launch_count_events(const uint8_t *bm, uint64_t bm_stride, uint64_t nb8, uint64_t N, uint32_t nx, uint32_t n, const uint32_t *blk_off,
                         const uint64_t *frame_base, const uint8_t *pv, uint64_t pv_stride, const uint32_t *pv_bytes, uint32_t d, uint32_t level,
                         uint32_t method, uint32_t area_threshold, uint8_t *workspace, uint64_t id_cap, void *events, uint64_t cap, int *err,
                         hipStream_t s);
// Counted views (rc_sum_add_counted): the same labelling and sums, and in the place of the event arrays one count per kept component
// added to view[frow * (upsample * nx) + fcol] (cnt_finish_fine; view_cells = (upsample * nx) * (upsample * ny) uint32 cells, zero
// or more counts in them already).  No event is written anywhere; the frames' event prefix lies at cnt_ev_base as above.  order: the
// adding kernel waits for this event and records it again (the handle's adds, whichever stream they come from, are one sequence).
// shifts (device memory, int32[2 * n], NULL: none): frame f's counts land (shifts[2 * f], shifts[2 * f + 1]) = (dy, dx) cells of the view away,
// those that leave it are dropped (rc_sum_add_counted_shifted).
void launch_count_place(const uint8_t *bm, uint64_t bm_stride, uint64_t nb8, uint64_t N, uint32_t nx, uint32_t n, const uint32_t *blk_off,
                        const uint64_t *frame_base, const uint8_t *pv, uint64_t pv_stride, const uint32_t *pv_bytes, uint32_t d, uint32_t level,
                        uint32_t method, uint32_t area_threshold, uint8_t *workspace, uint64_t id_cap, uint32_t *view, uint64_t view_cells,
                        uint32_t upsample, hipEvent_t order, int *err, hipStream_t s, const int32_t *shifts = nullptr);
}  // namespace rc
#endif
