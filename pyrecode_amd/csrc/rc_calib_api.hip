// rc_calib_api.hip - the stateless calibration seam (include/recode_hip.h): rc_calib_stats / rc_calib_histogram / rc_calib_top_thresholds
// on the caller's current GPU (utility context, rc_host.h).  Replaces the per-pixel loops of pyrecode/utils/calibration.py
// (_median_std_nb :48-57, the histogram of _get_fit_params :64-71, _get_pixel_thresh_2 :26-45); the fit itself stays on the host
// (pyrecode_amd/utils/calibration.py).  Sizes are checked before any device is touched.
#include <limits.h>

#include "rc_calib.h"
#include "rc_host.h"

namespace {
// Where the kernels write results the caller wants at host or device addresses: a device destination is written in place, host
// destinations share the utility context's staging buffer g_util.o and are copied back by finish().
struct CalibOuts {
    struct Item { void *dst; uint64_t bytes, off; bool host; };
    std::vector<Item> items;
    uint64_t staged = 0;
    size_t add(void *dst, uint64_t bytes)
    {
        const bool host = !is_device_ptr(dst);
        items.push_back(Item{dst, bytes, staged, host});
        if (host) staged += (bytes + 15) & ~15ull;
        return items.size() - 1;
    }
    int reserve() { return staged ? g_util.o.ensure(g_util.dmem, staged) : RC_OK; }
    template <class T> T *dev(size_t i) const { return items[i].host ? reinterpret_cast<T *>(g_util.o.p + items[i].off) : static_cast<T *>(items[i].dst); }
    int finish()
    {
        HIP_TRY(hipGetLastError());
        for (const Item &it : items)
            if (it.host) HIP_TRY(hipMemcpyAsync(it.dst, g_util.o.p + it.off, it.bytes, hipMemcpyDeviceToHost, g_util.stream));
        HIP_TRY(hipStreamSynchronize(g_util.stream));
        return RC_OK;
    }
};

int calib_sizes(const char *who, uint32_t n, uint64_t n_pixels)
{
    if (n == 0 || n > rc::CALIB_MAX_FRAMES) return fail(RC_ERR_BAD_ARG, (std::string(who) + ": 1 .. 65535 frames").c_str());
    if (n_pixels == 0 || n_pixels > (1ull << 36)) return fail(RC_ERR_BAD_ARG, (std::string(who) + ": 1 .. 2^36 pixels per frame").c_str());
    return RC_OK;
}
}  // namespace

RC_EXPORT uint32_t rc_calib_lds_max_frames(void) { return rc::CALIB_LDS_MAX_FRAMES; }

RC_EXPORT int rc_calib_stats(const uint16_t *stack, uint32_t n, uint64_t n_pixels, uint32_t n_stats, float *median, float *std_out, int32_t *range2)
{
    using namespace rc;
    if (!stack || !median || !std_out || !range2) return fail(RC_ERR_BAD_ARG, "NULL argument");
    int r = calib_sizes("rc_calib_stats", n, n_pixels);
    if (r != RC_OK) return r;
    if (n_stats > n) return fail(RC_ERR_BAD_ARG, "rc_calib_stats: n_stats exceeds the number of frames");
    UtilScope util_scope;
    if ((r = util_scope.enter()) != RC_OK) return r;
    Util &u = g_util;
    const uint16_t *d_stack = nullptr;
    if ((r = stage_in(stack, (uint64_t)n * n_pixels * 2u, u.a, d_stack)) != RC_OK) return r;
    CalibOuts outs;
    const size_t o_med = outs.add(median, n_pixels * 4u), o_std = outs.add(std_out, n_pixels * 4u), o_rng = outs.add(range2, 8);
    if ((r = outs.reserve()) != RC_OK) return r;
    int32_t *h_rng = reinterpret_cast<int32_t *>(u.h_scalar);
    h_rng[0] = INT_MAX;
    h_rng[1] = INT_MIN;
    HIP_TRY(hipMemcpyAsync(outs.dev<int32_t>(o_rng), h_rng, 8, hipMemcpyHostToDevice, u.stream));
    launch_calib_stats(d_stack, n, n_pixels, n_stats, outs.dev<float>(o_med), outs.dev<float>(o_std), outs.dev<int32_t>(o_rng), u.stream);
    return outs.finish();
}

RC_EXPORT int rc_calib_histogram(const uint16_t *frames, uint32_t n_stats, uint64_t n_pixels, const float *median, const double *edges,
                                 uint32_t n_bins, uint64_t *counts)
{
    using namespace rc;
    if (!frames || !median || !edges || !counts) return fail(RC_ERR_BAD_ARG, "NULL argument");
    int r = calib_sizes("rc_calib_histogram", n_stats, n_pixels);
    if (r != RC_OK) return r;
    if (n_bins == 0 || n_bins > 1024) return fail(RC_ERR_BAD_ARG, "rc_calib_histogram: 1 .. 1024 bins");
    UtilScope util_scope;
    if ((r = util_scope.enter()) != RC_OK) return r;
    Util &u = g_util;
    const uint16_t *d_frames = nullptr;
    const float *d_median = nullptr;
    const double *d_edges = nullptr;
    if ((r = stage_in(frames, (uint64_t)n_stats * n_pixels * 2u, u.a, d_frames)) != RC_OK || (r = stage_in(median, n_pixels * 4u, u.b, d_median)) != RC_OK ||
        (r = stage_in(edges, (uint64_t)(n_bins + 1) * 8u, u.w, d_edges)) != RC_OK)
        return r;
    CalibOuts outs;
    const size_t o_cnt = outs.add(counts, (uint64_t)n_bins * 8u);
    if ((r = outs.reserve()) != RC_OK) return r;
    HIP_TRY(hipMemsetAsync(outs.dev<uint64_t>(o_cnt), 0, (uint64_t)n_bins * 8u, u.stream));
    launch_calib_hist(d_frames, n_stats, n_pixels, d_median, d_edges, n_bins, outs.dev<uint64_t>(o_cnt), u.stream);
    return outs.finish();
}

RC_EXPORT int rc_calib_top_thresholds(const uint16_t *stack, uint32_t n, uint64_t n_pixels, const float *median, uint32_t k, float *acc,
                                      uint64_t *n_undefined)
{
    using namespace rc;
    if (!stack || !median || !acc || !n_undefined) return fail(RC_ERR_BAD_ARG, "NULL argument");
    int r = calib_sizes("rc_calib_top_thresholds", n, n_pixels);
    if (r != RC_OK) return r;
    if (k == 0) return fail(RC_ERR_BAD_ARG, "rc_calib_top_thresholds: k (expected_n_events) must be at least 1");
    UtilScope util_scope;
    if ((r = util_scope.enter()) != RC_OK) return r;
    Util &u = g_util;
    const uint16_t *d_stack = nullptr;
    const float *d_median = nullptr;
    if ((r = stage_in(stack, (uint64_t)n * n_pixels * 2u, u.a, d_stack)) != RC_OK || (r = stage_in(median, n_pixels * 4u, u.b, d_median)) != RC_OK) return r;
    CalibOuts outs;
    const size_t o_acc = outs.add(acc, n_pixels * 4u), o_und = outs.add(n_undefined, 8);
    if ((r = outs.reserve()) != RC_OK) return r;
    HIP_TRY(hipMemsetAsync(outs.dev<uint64_t>(o_und), 0, 8, u.stream));
    launch_calib_top(d_stack, n, n_pixels, d_median, k, outs.dev<float>(o_acc), outs.dev<uint64_t>(o_und), u.stream);
    return outs.finish();
}
