"""Calibration: a flat-field acquisition -> the threshold ("dark reference") frames every other layer starts from.

Interface = the reference's pyrecode/utils/calibration.py: `make_calibration_frames` (:87-138) with its signature, prints and file
names; `calibrate` is the same computation on an array that is already in memory, returning everything as a dict.

Where the work runs
  device  per-pixel median and standard deviation over all frames, the range of `frame - median` (rc_calib_stats: _median_std_nb :48-57),
          the 100-bin histogram of `frame - median` over the last n_stats_frames frames (rc_calib_histogram: np.histogram of
          _get_fit_params :71), the event counts per threshold (a reduction-level-2 ctx in reduce-only mode: its record carries the
          binary map and one statistic per 8-connected component - _count_events :19-23), the "accurate" thresholds
          (rc_calib_top_thresholds: _get_pixel_thresh_2 :26-45)
  host    the bin edges (np.histogram_bin_edges of the range - numpy's own widening of an empty range included), the Gaussian fit
          (scipy.optimize.curve_fit, the rest of _get_fit_params :72-84), `floor(median + sigma * i)` (:115) and the files
There is no CPU path for the device half: without a GPU the calls raise.

Departures from the reference, on purpose
  * frames are read with this package's em_reader (MRC / SEQ), not pims (absent here)
  * curve_fit does not fix the sign of sigma: the model depends on sigma^2 only, and the fit can end on the negative root (the reference
    then writes thresholds BELOW the median).  The value is used as it comes, like the reference does, and a warning is issued
  * a pixel with fewer than expected_n_events + 1 values above its median has no accurate threshold: the reference casts
    np.finfo(float32).min to the target integer type there, which is undefined.  Such pixels get the type's maximum (they never fire) and
    are counted in `n_undefined_pixels`
"""
import ctypes as C
import os
import warnings
from datetime import datetime
from pathlib import Path

import numpy as np

N_BINS = 100                      # _get_fit_params: np.histogram(..., bins=100)
_POP8 = np.array([bin(i).count("1") for i in range(256)], np.uint8)


def _gaussian(x, a, x0, sigma):
    return a * np.exp(-(x - x0) ** 2 / (2 * sigma ** 2))


def fit_sigma(hist, edges):
    """The host half of _get_fit_params (:72-84): (fit_std, p0, popt) of the Gaussian fitted to the normalised histogram."""
    from scipy.optimize import curve_fit
    h = np.asarray(hist).astype(np.int64)
    c = [(edges[i] + edges[i + 1]) / 2 for i in range(len(edges) - 1)]
    hn = h / np.sum(h)
    mean = np.average(c, weights=hn)
    sigma = np.sqrt(np.average((c - mean) ** 2, weights=hn))
    p0 = [np.max(hn), mean, sigma]
    popt, _ = curve_fit(_gaussian, c, hn, p0=p0)
    return popt[2], p0, popt


def threshold_frame(median, fit_std, i, dtype):
    """:115 - `fit_std` stays the numpy float64 scalar curve_fit returned, so the sum is taken in float64 as in the reference"""
    return np.floor(median + fit_std * i).astype(dtype)


def _resolve_device(torch, tensor_device=None):
    """The ONE GPU all of a calibration runs on: RC_DEVICE when set (the stateless entry points obey it), else the tensor's device, else
    the caller's current device.  A device tensor on another GPU than RC_DEVICE names is refused."""
    env = os.environ.get("RC_DEVICE")
    dev = int(env) if env else None
    if tensor_device is not None:
        if dev is not None and dev != tensor_device:
            raise ValueError("the tensor lives on GPU %d, RC_DEVICE names GPU %d" % (tensor_device, dev))
        return tensor_device
    if dev is not None:
        return dev
    return torch.cuda.current_device() if torch is not None else 0


class _Stack:
    """The frames as the library sees them: an address (device memory when torch can put them there, else the caller's host array,
    which the library then stages per call), the geometry, the one GPU everything runs on, and what must stay alive meanwhile.
    The library reads device memory on streams of its own (include/recode_hip.h, "ordering of device pointers"): whatever torch still
    has queued for the frames - the caller's kernels that produce them, the copy `contiguous()` may launch, an upload - is waited for
    here, before the first call."""

    def __init__(self, data):
        self.torch = None
        if isinstance(data, np.ndarray):
            if data.dtype != np.uint16:
                raise NotImplementedError("calibration takes uint16 frames, not %s" % data.dtype)
            if data.ndim != 3:
                raise ValueError("data must be [n, ny, nx]")
            self.host = np.ascontiguousarray(data)
            self.n, self.ny, self.nx = self.host.shape
            self.keep, self.address = self.host, self.host.ctypes.data
            try:
                import torch
                if torch.cuda.is_available():
                    self.torch = torch
            except ImportError:
                pass
            self.device = _resolve_device(self.torch)
            if self.torch is not None:
                with warnings.catch_warnings():      # (a read-only array - a memory-mapped file - is only read from here)
                    warnings.simplefilter("ignore", UserWarning)
                    self.keep = self.torch.from_numpy(self.host.view(np.int16)).to("cuda:%d" % self.device)
                self.address = self.keep.data_ptr()
        else:
            import torch
            if not isinstance(data, torch.Tensor):
                raise TypeError("data must be a numpy array or a torch tensor")
            if data.dtype != torch.uint16:
                raise NotImplementedError("calibration takes uint16 frames, not %s" % data.dtype)
            if data.dim() != 3:
                raise ValueError("data must be [n, ny, nx]")
            if not data.is_cuda:
                raise ValueError("a torch tensor must live on the device (pass host data as a numpy array)")
            self.torch = torch
            self.device = _resolve_device(torch, data.device.index)
            self.keep = data.contiguous()
            self.n, self.ny, self.nx = (int(v) for v in self.keep.shape)
            self.address, self.host = self.keep.data_ptr(), None
        self.n_pixels = self.ny * self.nx
        self.synchronize()

    def synchronize(self):
        if self.torch is not None:
            self.torch.cuda.synchronize(self.device)

    def frame_address(self, f):
        return self.address + 2 * self.n_pixels * f

    def on_device(self):
        import contextlib
        return self.torch.cuda.device(self.device) if self.torch is not None else contextlib.nullcontext()

    def device_copy(self, a):
        """address of a float32 array for the next call: a device copy when torch is there (no upload per call), else the array itself"""
        if self.torch is None:
            return a, a.ctypes.data
        t = self.torch.from_numpy(a).to("cuda:%d" % self.device)
        self.synchronize()
        return t, t.data_ptr()


def _count_events(hip, st, first, n_frames, thresholds):
    """_count_events (:19-23) for every threshold frame and every frame of [first, first + n_frames): (components, set pixels) as two
    int64 arrays [len(thresholds)][n_frames].  The labelling is the writer's own reduction level 2 (rc_l2.hip) in reduce-only mode:
    record = u32 frame id | u32 bytes of statistics | binary map | one 16-bit statistic per 8-connected component."""
    lib = hip.lib()
    batch = min(n_frames, 8)
    ctx = hip.ReduceContext(st.nx, st.ny, 16, reduction_level=2, op_mode=0, scheme=0, clevel=0, device_id=st.device, max_batch=batch)
    try:
        out = np.empty(ctx.out_capacity(batch), np.uint8)
        rec = np.zeros(batch + 1, np.uint64)
        md = np.zeros((batch, 3), np.uint32)
        events = np.zeros((len(thresholds), n_frames), np.int64)
        pixels = np.zeros((len(thresholds), n_frames), np.int64)
        for i, t in enumerate(thresholds):
            ctx.set_threshold(t)
            for f0 in range(0, n_frames, batch):
                nb = min(batch, n_frames - f0)
                hip.check(lib.rc_reduce_compress_batch(ctx.handle, st.frame_address(first + f0), nb, f0, hip.ptr(out), out.size, hip.ptr(rec),
                                                       hip.ptr(md)), "rc_reduce_compress_batch")
                for z in range(nb):
                    r = out[int(rec[z]):int(rec[z + 1])]
                    n_packed = int(r[4:8].view("<u4")[0])
                    events[i, f0 + z] = n_packed // 2
                    pixels[i, f0 + z] = int(_POP8[r[8:8 + ctx.bitmap_bytes]].sum(dtype=np.int64))
        return events, pixels
    finally:
        ctx.close()


def calibrate(data, n_stats_frames, n_sigmas, use_acc=False, sigma_acc=-1, *, verbose=False, _start=None):
    """data: [n, ny, nx] uint16 numpy array, or a torch.uint16 tensor on the device (other dtypes: NotImplementedError).

    Returns a dict: median, std (float32 [ny, nx]), hist (int64[100]), edges (float64[101]), fit_std (the fitted sigma, sign as
    curve_fit left it), thresholds (list of n_sigmas frames of the data's dtype), avg_n_events, avg_p_foreground_pixels, dose_rate
    (lists, one entry per sigma); with use_acc and 0 <= sigma_acc < n_sigmas also expected_n_events and - when that is at least 2 -
    acc_threshold (float32 [ny, nx]; cast it to the target dtype as the thresholds are) and n_undefined_pixels.
    verbose: the reference's prints."""
    from .. import _lib as hip
    start = _start or datetime.now()
    st = _Stack(data)
    n, n_pixels = st.n, st.n_pixels
    n_stats_frames = int(n_stats_frames)
    if not 1 <= n_stats_frames <= n:
        raise ValueError("n_stats_frames must be 1 .. %d (the number of frames)" % n)
    lib = hip.lib()
    dtype = np.uint16
    with st.on_device():
        # ---- median, std, range of frame - median (device) ----------------------------------------------------------------------------
        median = np.empty((st.ny, st.nx), np.float32)
        std = np.empty((st.ny, st.nx), np.float32)
        range2 = np.zeros(2, np.int32)
        hip.check(lib.rc_calib_stats(st.address, n, n_pixels, n_stats_frames, hip.ptr(median), hip.ptr(std), hip.ptr(range2)), "rc_calib_stats")
        med_keep, med_address = st.device_copy(median)
        # ---- histogram (edges: host, counts: device) and fit (host) ----------------------------------------------------------------------
        edges = np.histogram_bin_edges(np.array([range2[0] / 2.0, range2[1] / 2.0]), bins=N_BINS)
        counts = np.zeros(N_BINS, np.uint64)
        hip.check(lib.rc_calib_histogram(st.frame_address(n - n_stats_frames), n_stats_frames, n_pixels, med_address, hip.ptr(edges), N_BINS,
                                         hip.ptr(counts)), "rc_calib_histogram")
        hist = counts.astype(np.int64)
        fit_std, p0, popt = fit_sigma(hist, edges)
        if fit_std < 0:
            warnings.warn("calibration: the Gaussian fit ended on a negative sigma (%g); it is used as it is, as the reference does - thresholds "
                          "for sigma >= 1 lie BELOW the median" % fit_std, RuntimeWarning, stacklevel=2)
        if verbose:
            print("\n Fit Result \n Init params=", p0, "\n Optimal params=", popt)
            print('\nAvg. std.dev. per pixel:', np.average(std))
            print('Global intensity std. dev.:', fit_std)
            print("Calibration time:", datetime.now() - start, "\n")
        # ---- thresholds (host) and their event counts (device) ---------------------------------------------------------------------------
        thresholds = [threshold_frame(median, fit_std, i, dtype) for i in range(n_sigmas)]
        events, pixels = _count_events(hip, st, n - n_stats_frames, n_stats_frames, thresholds)
        res = {"median": median, "std": std, "fit_std": fit_std, "hist": hist, "edges": edges, "thresholds": thresholds,
               "avg_n_events": [], "avg_p_foreground_pixels": [], "dose_rate": []}
        for i in range(n_sigmas):
            n_events = 0
            p_foreground_pixels = 0
            for f in range(n_stats_frames):                 # (the reference's own order of additions, :117-124)
                n_events += int(events[i, f])
                p_foreground_pixels += (int(pixels[i, f]) / n_pixels)
            avg_n_events = n_events / n_stats_frames
            avg_p_foreground_pixels = p_foreground_pixels / n_stats_frames
            res["avg_n_events"].append(avg_n_events)
            res["avg_p_foreground_pixels"].append(avg_p_foreground_pixels)
            res["dose_rate"].append(avg_n_events / n_pixels)
            if verbose:
                print("Avg. prop. foreground pixels for sigma=" + str(i) + " is: " + str(avg_p_foreground_pixels))
                print("Avg. electron count for sigma=" + str(i) + " is: " + str(avg_n_events))
                print("Avg. dose rate for sigma=" + str(i) + " is: " + str(avg_n_events / n_pixels))
                print("")
            if use_acc and i == sigma_acc:
                expected_n_events = int(np.ceil(n * (avg_n_events / n_pixels)))
                res["expected_n_events"] = expected_n_events
                if verbose:
                    print(expected_n_events)
                if expected_n_events < 2:
                    print("Unable to compute accurate thresholds: too few events in dataset")
                else:
                    # ---- accurate thresholds (device) ---------------------------------------------------------------------------
                    acc = np.empty((st.ny, st.nx), np.float32)
                    undefined = C.c_uint64(0)
                    hip.check(lib.rc_calib_top_thresholds(st.address, n, n_pixels, med_address, expected_n_events, hip.ptr(acc),
                                                          C.addressof(undefined)), "rc_calib_top_thresholds")
                    res["acc_threshold"] = acc
                    res["n_undefined_pixels"] = int(undefined.value)
                    if verbose:
                        print(acc)
        del med_keep
    return res


def _file_type(path):
    from ..misc import rc_cfg as rc
    ext = os.path.splitext(str(path))[1].lower()
    if ext in (".mrc", ".mrcs"):
        return rc.FILE_TYPE_MRC
    if ext == ".seq":
        return rc.FILE_TYPE_SEQ
    raise ValueError("calibration reads MRC (.mrc, .mrcs) and SEQ (.seq) files, not %r" % ext)


def make_calibration_frames(filepath, dtype, nFrames, n_stats_frames, n_sigmas, savepath='', filename_prefix='',
                            use_acc=False, sigma_acc=-1):
    """Reference :87-138, with the same prints and the same file names: `<prefix>__dark_ref_<i>.bin` (the prefix gets a '_' appended
    when it does not end in one, and the name part starts with another) and `<prefix>__dark_ref_<i>A.bin` for the accurate frame, each
    written with `.astype(dtype).tofile`.  Returns the dict of `calibrate`."""
    from ..em_reader import emfile
    _filepath = str(Path(filepath))
    if not filename_prefix.endswith('_'):
        filename_prefix += '_'
    start = datetime.now()
    with emfile(_filepath, _file_type(_filepath)) as fp:
        d = np.ascontiguousarray(fp[0:nFrames]).astype(dtype, copy=False)
    res = calibrate(d, n_stats_frames, n_sigmas, use_acc=use_acc, sigma_acc=sigma_acc, verbose=True, _start=start)
    for i, t in enumerate(res["thresholds"]):
        t.astype(dtype).tofile(os.path.join(savepath, filename_prefix + "_dark_ref_" + str(i) + ".bin"))
        if use_acc and i == sigma_acc and "acc_threshold" in res:
            res["acc_threshold"].astype(dtype).tofile(os.path.join(savepath, filename_prefix + "_dark_ref_" + str(i) + "A.bin"))
    return res

