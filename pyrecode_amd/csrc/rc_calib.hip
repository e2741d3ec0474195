// rc_calib.hip - calibration on the device: what turns a flat-field acquisition into threshold frames.
//
// Reference: pyrecode/utils/calibration.py
//   _median_std_nb (:48-57)        np.median / np.std of every pixel over nFrames frames        -> k_calib_cols<CALIB_STATS>
//   _get_fit_params (:64-71)       np.histogram(frame - median, bins=100) over the last frames  -> k_calib_hist (edges from the host)
//   _get_pixel_thresh_2 (:26-45)   mean of the (k+1)-th and k-th largest value above the median -> k_calib_cols<CALIB_TOP>
// The input is a uint16 stack [n][N] in C order: a pixel's column is strided by a whole frame, so a one-wave workgroup takes a tile of 64
// consecutive pixels - one 128-byte line per frame -, stages [frame][pixel] in LDS (one read of the stack from HBM) and gives every lane
// one column; the per-column logic (rc_calib.h: 16-step bitwise bisection for the ranks, exact-integer moments) then runs over LDS.  A
// column of more than CALIB_LDS_MAX_FRAMES values does not fit: the same logic runs over global memory (about 17 reads of the column).
#include <limits.h>

#include <algorithm>

#include "rc_calib.h"
#include "rc_launch.h"

namespace rc {

constexpr int CALIB_STATS = 0, CALIB_TOP = 1;
constexpr uint32_t CALIB_TILE = 64;                    // pixels per workgroup: 128 bytes of every frame

struct LdsCol {
    const uint16_t *s;                                 // &tile[0][lane]
    __device__ __forceinline__ uint32_t operator()(uint32_t i) const { return s[i * CALIB_TILE]; }
};
struct GlobalCol {
    const uint16_t *g;                                 // &stack[0][pixel]
    uint64_t N;
    __device__ __forceinline__ uint32_t operator()(uint32_t i) const { return g[(uint64_t)i * N]; }
};

struct CalibArgs {
    const uint16_t *stack;
    uint32_t n;
    uint64_t N;
    uint32_t n_stats;            // CALIB_STATS: frames (the last ones) whose `frame - median` range is taken
    float *median;               // CALIB_STATS: out; CALIB_TOP: in
    float *sdev;                 // CALIB_STATS: out (np.std)
    int32_t *range2;             // CALIB_STATS: {min, max} of 2 * frame - 2 * median (atomic; the host presets INT_MAX, INT_MIN)
    uint32_t k;                  // CALIB_TOP: expected_n_events
    float *acc;                  // CALIB_TOP: out
    unsigned long long *n_undefined;   // CALIB_TOP: pixels with fewer than k + 1 values above their median (atomic; preset 0)
};

__device__ __forceinline__ int wave_min_i32(int v)
{
#pragma unroll
    for (int d = 32; d; d >>= 1) v = min(v, __shfl_xor(v, d));
    return v;
}
__device__ __forceinline__ int wave_max_i32(int v)
{
#pragma unroll
    for (int d = 32; d; d >>= 1) v = max(v, __shfl_xor(v, d));
    return v;
}

// one pixel's column -> its outputs; every lane of the wave calls this (have = false: a lane behind the last pixel)
template <int MODE, class Col>
__device__ __forceinline__ void calib_column(const CalibArgs &a, const Col &col, uint64_t p, bool have)
{
    if (MODE == CALIB_STATS) {
        int lo = INT_MAX, hi = INT_MIN;
        if (have) {
            const uint32_t m2 = calib_median2(col, a.n);
            a.median[p] = 0.5f * (float)m2;
            a.sdev[p] = calib_std(col, a.n);
            for (uint32_t f = a.n - a.n_stats; f < a.n; ++f) {
                const int v = 2 * (int)col(f) - (int)m2;
                lo = min(lo, v);
                hi = max(hi, v);
            }
        }
        lo = wave_min_i32(lo);
        hi = wave_max_i32(hi);
        if (lane_id() == 0 && lo <= hi) {
            atomicMin(a.range2, lo);
            atomicMax(a.range2 + 1, hi);
        }
    } else {
        bool undefined = false;
        if (have) {
            float t = 65535.0f;      // the source dtype's maximum: a pixel without a defined threshold never fires
            undefined = !calib_top_pair(col, a.n, a.median[p], a.k, t);
            a.acc[p] = t;
        }
        const uint64_t u = __builtin_amdgcn_ballot_w64(undefined);
        if (lane_id() == 0 && u) atomicAdd(a.n_undefined, (unsigned long long)__builtin_popcountll(u));
    }
}

// grid: one-wave workgroups over tiles of 64 pixels; dynamic LDS: n * 128 bytes.  vec: 16-byte loads - eight lanes fetch one frame's line,
// eight frames per instruction - when every frame of the stack starts at a 16-byte boundary; otherwise a 2-byte load per lane and frame.
template <int MODE>
__global__ __launch_bounds__(64) void k_calib_cols(CalibArgs a, int vec)
{
    extern __shared__ __attribute__((aligned(16))) uint16_t s_tile[];   // [n][64]
    const uint32_t lane = (uint32_t)lane_id();
    const uint64_t p0 = (uint64_t)blockIdx.x * CALIB_TILE;
    if (vec) {
        const uint32_t sub = lane & 7u, fr = lane >> 3;
        const uint64_t px = p0 + 8u * sub;                            // (N is a multiple of 8 here: a group of 8 pixels is inside the frame or behind it)
        constexpr int U = 4;
        for (uint32_t f0 = 0; f0 < a.n; f0 += 8u * U) {
            u32x4 v[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const uint32_t f = f0 + 8u * u + fr;
                v[u] = u32x4{0u, 0u, 0u, 0u};
                if (f < a.n && px < a.N) v[u] = *reinterpret_cast<const u32x4 *>(a.stack + (uint64_t)f * a.N + px);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const uint32_t f = f0 + 8u * u + fr;
                if (f < a.n) *reinterpret_cast<u32x4 *>(s_tile + f * CALIB_TILE + 8u * sub) = v[u];
            }
        }
    } else {
        const uint64_t p = p0 + lane;
        for (uint32_t f = 0; f < a.n; ++f) s_tile[f * CALIB_TILE + lane] = p < a.N ? a.stack[(uint64_t)f * a.N + p] : (uint16_t)0;
    }
    __syncthreads();
    calib_column<MODE>(a, LdsCol{s_tile + lane}, p0 + lane, p0 + lane < a.N);
}

// the same per-column logic over global memory, a lane per pixel: columns too long for LDS
template <int MODE>
__global__ __launch_bounds__(256) void k_calib_cols_global(CalibArgs a)
{
    const uint64_t p = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const bool have = p < a.N;
    calib_column<MODE>(a, GlobalCol{a.stack + (have ? p : 0), a.N}, p, have);
}

template <int MODE>
static void launch_calib_cols(const CalibArgs &a, hipStream_t s)
{
    if (a.n <= CALIB_LDS_MAX_FRAMES) {
        const int vec = (a.N % 8u == 0 && (reinterpret_cast<uintptr_t>(a.stack) & 15u) == 0) ? 1 : 0;
        const uint32_t grid = (uint32_t)((a.N + CALIB_TILE - 1) / CALIB_TILE);
        hipLaunchKernelGGL(k_calib_cols<MODE>, dim3(grid), dim3(64), (size_t)a.n * CALIB_TILE * 2u, s, a, vec);
    } else {
        hipLaunchKernelGGL(k_calib_cols_global<MODE>, dim3((uint32_t)((a.N + 255u) / 256u)), dim3(256), 0, s, a);
    }
}

void launch_calib_stats(const uint16_t *stack, uint32_t n, uint64_t N, uint32_t n_stats, float *median, float *sdev, int32_t *range2, hipStream_t s)
{
    CalibArgs a{};
    a.stack = stack; a.n = n; a.N = N; a.n_stats = n_stats; a.median = median; a.sdev = sdev; a.range2 = range2;
    launch_calib_cols<CALIB_STATS>(a, s);
}

void launch_calib_top(const uint16_t *stack, uint32_t n, uint64_t N, const float *median, uint32_t k, float *acc, uint64_t *n_undefined, hipStream_t s)
{
    CalibArgs a{};
    a.stack = stack; a.n = n; a.N = N; a.median = const_cast<float *>(median); a.k = k; a.acc = acc;
    a.n_undefined = reinterpret_cast<unsigned long long *>(n_undefined);
    launch_calib_cols<CALIB_TOP>(a, s);
}

// ---- histogram of frame - median ----------------------------------------------------------------------------------------------
// np.histogram's definition: value x = double(d) - double(m) belongs to the bin with edges[i] <= x < edges[i + 1], the last bin closed on
// the right; the n_bins + 1 edges come from the host (np.histogram_bin_edges).  Nearly every value falls into two or three bins - the
// noise peak is narrow, rare events stretch the range -, so a wave first joins its equal bins: one LDS add per DISTINCT bin of the 64
// lanes, into the wave's own histogram - always by lane 0 (every lane knows the bin and its count: both are wave-uniform), so all updates
// of a wave's histogram are one thread's loads and stores in program order and need no atomics.  One global add per bin and workgroup at the end.
constexpr int HIST_T = 256;
__global__ __launch_bounds__(HIST_T) void k_calib_hist(const uint16_t *__restrict__ frames, uint32_t n_stats, uint64_t N, const float *__restrict__ median,
                                                       const double *__restrict__ edges, uint32_t nb, unsigned long long *__restrict__ counts)
{
    extern __shared__ __attribute__((aligned(16))) double s_edges[];   // [nb + 1], then uint32 [HIST_T / 64][nb]
    uint32_t *s_hist = reinterpret_cast<uint32_t *>(s_edges + nb + 1);
    for (uint32_t i = threadIdx.x; i <= nb; i += HIST_T) s_edges[i] = edges[i];
    for (uint32_t i = threadIdx.x; i < (HIST_T / 64) * nb; i += HIST_T) s_hist[i] = 0;
    __syncthreads();
    uint32_t *h = s_hist + (threadIdx.x >> 6) * nb;
    const uint32_t lane = (uint32_t)lane_id();
    const double e_first = s_edges[0], e_last = s_edges[nb];
    for (uint64_t base = (uint64_t)blockIdx.x * HIST_T; base < N; base += (uint64_t)gridDim.x * HIST_T) {
        const uint64_t p = base + threadIdx.x;
        const bool have = p < N;
        const double m = have ? (double)median[p] : 0.0;
        for (uint32_t f = 0; f < n_stats; ++f) {
            int bin = -1;
            if (have) {
                const double x = (double)frames[(uint64_t)f * N + p] - m;
                if (x >= e_first && x <= e_last) {
                    uint32_t lo = 0, hi = nb;               // edges[lo] <= x, and x < edges[hi] or hi == nb
                    while (hi - lo > 1) {
                        const uint32_t mid = (lo + hi) >> 1;
                        if (s_edges[mid] <= x) lo = mid;
                        else hi = mid;
                    }
                    bin = (int)lo;
                }
            }
            for (uint64_t rem = __builtin_amdgcn_ballot_w64(bin >= 0); rem;) {
                const uint32_t leader = (uint32_t)__builtin_ctzll(rem);
                const int b = __shfl(bin, (int)leader);
                const uint64_t same = __builtin_amdgcn_ballot_w64(bin == b);
                if (lane == 0) h[b] += (uint32_t)__builtin_popcountll(same);
                rem &= ~same;
            }
        }
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < nb; i += HIST_T) {
        unsigned long long c = 0;
        for (uint32_t w = 0; w < HIST_T / 64; ++w) c += s_hist[w * nb + i];
        if (c) atomicAdd(counts + i, c);
    }
}

void launch_calib_hist(const uint16_t *frames, uint32_t n_stats, uint64_t N, const float *median, const double *edges, uint32_t n_bins,
                       uint64_t *counts, hipStream_t s)
{
    // a wave's counters are 32 bits wide: enough workgroups that none sees 2^31 values
    const uint64_t blocks = (N + HIST_T - 1) / HIST_T;
    const uint64_t need = (N * (uint64_t)n_stats >> 31) + 1;
    const uint32_t grid = (uint32_t)std::min<uint64_t>(blocks, std::max<uint64_t>(4096, need));
    const size_t lds = (size_t)(n_bins + 1) * 8u + (size_t)(HIST_T / 64) * n_bins * 4u;
    hipLaunchKernelGGL(k_calib_hist, dim3(grid), dim3(HIST_T), lds, s, frames, n_stats, N, median, edges, n_bins,
                       reinterpret_cast<unsigned long long *>(counts));
}

}  // namespace rc
