"""ctypes binding of librecode_hip.so (C ABI: include/recode_hip.h).

The library is hand-written HIP for gfx950 and has no CPU path; this module fails loudly when the shared object
is missing or when a compute call finds no GPU.  Nothing here imports the oracle.
"""
import ctypes as C
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RC_LIB_PATH") or os.path.join(_HERE, "librecode_hip.so")   # (RC_LIB_PATH: A/B runs of two builds, tools/ab_libs.py)

RC_OK = 0
RC_ERR_BAD_ARG = -1
RC_ERR_OUT_TOO_SMALL = -2
RC_ERR_DEVICE = -3
RC_ERR_UNSUPPORTED = -4
RC_ERR_RECORD_TOO_LARGE = -5
RC_ERR_CORRUPT = -6
RC_ERR_WORKSPACE = -7
RC_SCHEME_ZLIB_DEVICE = 0x100   # compression_scheme 0 records from the device's own DEFLATE encoder (include/recode_hip.h)

# every symbol include/recode_hip.h declares: (restype, argtypes)
_u8p, _u16p, _u32p, _u64p = C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p  # raw addresses: host or device
_i32p = C.c_void_p
SIGNATURES = {
    "rc_abi_version": (C.c_int, []),
    "rc_strerror": (C.c_char_p, [C.c_int]),
    "rc_last_error": (C.c_char_p, []),
    "rc_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "rc_scheme_on_device": (C.c_int, [C.c_uint32]),
    "rc_ctx_create": (C.c_void_p, [C.c_uint32] * 7 + [C.c_int, C.c_uint32, C.POINTER(C.c_int)]),
    "rc_ctx_destroy": (C.c_int, [C.c_void_p]),
    "rc_ctx_set_stream": (C.c_int, [C.c_void_p, C.c_void_p]),
    "rc_ctx_set_source_bytes": (C.c_int, [C.c_void_p, C.c_uint32]),
    "rc_ctx_source_bytes": (C.c_uint32, [C.c_void_p]),
    "rc_set_dark": (C.c_int, [C.c_void_p, _u16p, C.c_int64]),
    "rc_set_threshold": (C.c_int, [C.c_void_p, _u16p]),
    "rc_out_capacity": (C.c_uint64, [C.c_void_p, C.c_uint32]),
    "rc_md_fields": (C.c_uint32, [C.c_void_p]),
    "rc_reduce_compress_batch": (C.c_int, [C.c_void_p, _u16p, C.c_uint32, C.c_uint32, _u8p, C.c_uint64, _u64p, _u32p]),
    "rc_reduce_compress_batch_async": (C.c_int, [C.c_void_p, _u16p, C.c_uint32, C.c_uint32, _u8p, C.c_uint64, _u64p, _u32p]),
    "rc_ctx_sync": (C.c_int, [C.c_void_p]),
    "rc_ctx_set_pipelined": (C.c_int, [C.c_void_p, C.c_int]),
    "rc_ctx_wait_results": (C.c_int, [C.c_void_p, C.c_void_p]),
    "rc_ctx_refit_model": (C.c_int, [C.c_void_p]),
    "rc_get_binary_map": (C.c_int, [C.c_void_p, C.c_uint32, _u8p]),
    "rc_ctx_keep_binary_maps": (C.c_int, [C.c_void_p, C.c_int]),
    "rc_ctx_set_l2_statistics": (C.c_int, [C.c_void_p, C.c_uint32]),
    "rc_get_stage_ms": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "rc_ctx_set_profiling": (C.c_int, [C.c_void_p, C.c_int]),
    "rc_ctx_get_profile": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]),
    "rc_host_alloc": (C.c_void_p, [C.c_uint64]),
    "rc_host_free": (C.c_int, [C.c_void_p]),
    "rc_host_register": (C.c_int, [C.c_void_p, C.c_uint64]),
    "rc_host_unregister": (C.c_int, [C.c_void_p]),
    "rc_pipe_submit": (C.c_int, [C.c_void_p, C.c_uint32, _u16p, C.c_uint32, C.c_uint32]),
    "rc_pipe_input_done": (C.c_int, [C.c_void_p, C.c_uint32]),
    "rc_pipe_result": (C.c_int, [C.c_void_p, C.c_uint32, _u64p, _u32p, C.POINTER(C.c_uint64)]),
    "rc_pipe_fetch": (C.c_int, [C.c_void_p, C.c_uint32, _u8p, C.c_uint64]),
    "rc_pipe_fetch_wait": (C.c_int, [C.c_void_p, C.c_uint32]),
    "rc_ctx_set_validation": (C.c_int, [C.c_void_p] + [C.c_uint32] * 5),
    "rc_pipe_validation": (C.c_int, [C.c_void_p, C.c_uint32, _u32p]),
    "rc_compress": (C.c_int, [C.c_uint32, C.c_uint32, _u8p, C.c_uint64, _u8p, C.c_uint64, C.POINTER(C.c_uint64)]),
    "rc_decompress": (C.c_int, [C.c_uint32, _u8p, C.c_uint64, _u8p, C.c_uint64, C.POINTER(C.c_uint64)]),
    "rc_compress_bound": (C.c_uint64, [C.c_uint32, C.c_uint64]),
    "rc_unpack_frame_sparse": (C.c_int64, [C.c_uint32, C.c_uint32, C.c_uint32, _u8p, _u8p, C.c_uint64, _u64p, C.c_uint64, C.c_uint32]),
    "rc_expand_frames": (C.c_int, [C.c_uint32] * 6 + [_u8p, _u32p, C.c_uint32, _u64p, _u64p, C.c_uint64]),
    "rc_expand_frames_submit": (C.c_int, [C.c_uint32] * 7 + [_u8p, _u32p, C.c_uint32, _u64p, C.c_uint64]),
    "rc_expand_frames_wait": (C.c_int, [C.c_uint32, _u64p]),
    "rc_expand_frames_coo": (C.c_int, [C.c_uint32] * 6 + [_u8p, _u32p, C.c_uint32, _u64p, C.c_void_p, C.c_uint64]),
    "rc_expand_frames_coo_submit": (C.c_int, [C.c_uint32] * 7 + [_u8p, _u32p, C.c_uint32, C.c_void_p, C.c_uint64]),
    "rc_expand_frames_coo32": (C.c_int, [C.c_uint32] * 6 + [_u8p, _u32p, C.c_uint32, _u64p, C.c_void_p, C.c_uint64]),
    "rc_expand_frames_coo32_submit": (C.c_int, [C.c_uint32] * 7 + [_u8p, _u32p, C.c_uint32, C.c_void_p, C.c_uint64]),
    "rc_expand_frames_l2": (C.c_int, [C.c_uint32] * 5 + [_u8p, _u32p, C.c_uint32, _u64p, C.c_void_p, C.c_uint64, _u16p, C.c_uint64]),
    "rc_expand_frames_l2_submit": (C.c_int, [C.c_uint32] * 6 + [_u8p, _u32p, C.c_uint32, C.c_void_p, C.c_uint64, _u16p, C.c_uint64]),
    "rc_expand_frames_dense": (C.c_int, [C.c_uint32] * 6 + [_u8p, _u32p] + [C.c_uint32] * 8 + [C.c_void_p, C.c_uint64, _u64p]),
    "rc_expand_frames_dense_submit": (C.c_int, [C.c_uint32] * 7 + [_u8p, _u32p] + [C.c_uint32] * 8 + [C.c_void_p, C.c_uint64]),
    "rc_sum_create": (C.c_void_p, [C.c_uint32, C.c_uint32, C.POINTER(C.c_int)]),
    "rc_sum_destroy": (C.c_int, [C.c_void_p]),
    "rc_count_frames": (C.c_int, [C.c_uint32] * 6 + [_u8p, _u32p] + [C.c_uint32] * 3 + [_u64p, C.c_void_p, C.c_uint64]),
    "rc_count_frames_submit": (C.c_int, [C.c_uint32] * 7 + [_u8p, _u32p] + [C.c_uint32] * 3 + [C.c_void_p, C.c_uint64]),
    "rc_sum_add_frames": (C.c_int, [C.c_void_p] + [C.c_uint32] * 4 + [_u8p, _u32p, C.c_uint32, _u64p]),
    "rc_sum_add_frames_submit": (C.c_int, [C.c_void_p] + [C.c_uint32] * 5 + [_u8p, _u32p, C.c_uint32]),
    "rc_sum_add_counted": (C.c_int, [C.c_void_p] + [C.c_uint32] * 7 + [_u8p, _u32p] + [C.c_uint32] * 3 + [_u64p]),
    "rc_sum_add_counted_submit": (C.c_int, [C.c_void_p] + [C.c_uint32] * 8 + [_u8p, _u32p] + [C.c_uint32] * 3),
    "rc_sum_add_frames_shifted": (C.c_int, [C.c_void_p] + [C.c_uint32] * 4 + [_u8p, _u32p, C.c_uint32, _i32p, _u64p]),
    "rc_sum_add_frames_shifted_submit": (C.c_int, [C.c_void_p] + [C.c_uint32] * 5 + [_u8p, _u32p, C.c_uint32, _i32p]),
    "rc_sum_add_counted_shifted": (C.c_int, [C.c_void_p] + [C.c_uint32] * 7 + [_u8p, _u32p] + [C.c_uint32] * 3 + [_i32p, _u64p]),
    "rc_sum_add_counted_shifted_submit": (C.c_int, [C.c_void_p] + [C.c_uint32] * 8 + [_u8p, _u32p] + [C.c_uint32] * 3 + [_i32p]),
    "rc_sum_fetch": (C.c_int, [C.c_void_p, _u32p, C.c_int]),
    "rc_sum_bound": (C.c_uint64, [C.c_void_p]),
    "rc_trace_columns": (C.c_uint32, [C.c_void_p]),
    "rc_trace_weight_bound": (C.c_uint32, [C.c_void_p, C.c_uint32]),
    "rc_corr_side": (C.c_uint32, [C.c_void_p]),
    "rc_corr_reference_bound": (C.c_uint32, [C.c_void_p]),
    "rc_bins_count": (C.c_uint32, [C.c_void_p]),
    "rc_host_decoder_available": (C.c_int, [C.c_uint32]),
    "rc_host_decode_streams": (C.c_int, [C.c_uint32, _u8p, _u8p, _u64p, C.c_uint32, C.c_uint32]),
    "rc_split_triplets": (C.c_int, [_u64p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]),
    "rc_bit_pack": (C.c_int, [_u16p, C.c_uint64, C.c_uint32, _u8p, C.c_uint64]),
    "rc_bit_unpack": (C.c_int, [_u8p, C.c_uint64, C.c_uint64, C.c_uint32, _u64p]),
    "rc_calib_stats": (C.c_int, [_u16p, C.c_uint32, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rc_calib_lds_max_frames": (C.c_uint32, []),
    "rc_calib_histogram": (C.c_int, [_u16p, C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32, _u64p]),
    "rc_calib_top_thresholds": (C.c_int, [_u16p, C.c_uint32, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p, _u64p]),
    "rc_synth_dark": (C.c_int, [C.c_int, C.c_uint32, C.c_uint64, _u16p]),
    "rc_synth_frames": (C.c_int, [C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32, _u16p, _u16p]),
    "rc_synth_frames_clustered": (C.c_int, [C.c_int] + [C.c_uint32] * 6 + [_u16p, _u16p]),
}
for _p in ("rc_trace", "rc_corr", "rc_bins"):      # the per-frame tables: the same four entry points per kind
    SIGNATURES.update({
        _p + "_create": (C.c_void_p, [C.c_uint32] * 3 + [C.c_void_p, C.POINTER(C.c_int)]),
        _p + "_destroy": (C.c_int, [C.c_void_p]),
        _p + "_frames": (C.c_int, [C.c_void_p] + [C.c_uint32] * 4 + [_u8p, _u32p, C.c_uint32, C.c_void_p, C.c_uint64, _u64p]),
        _p + "_frames_submit": (C.c_int, [C.c_void_p] + [C.c_uint32] * 5 + [_u8p, _u32p, C.c_uint32, C.c_void_p, C.c_uint64]),
    })

_lib = None


class RecodeHipError(RuntimeError):
    pass


def lib():
    """Load librecode_hip.so (once).  If torch is going to be used in this process it must be imported first: both link
    the HIP runtime by SONAME and exactly one copy may be live ("one HIP runtime per process")."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RecodeHipError(
                "librecode_hip.so is not built (%s). Run `python -c 'import __graft_entry__ as g; g.build()'` or "
                "`make -C pyrecode_amd/csrc`. There is no CPU fallback." % LIB_PATH)
        if "torch" not in sys.modules:
            try:  # keep a single HIP runtime in the process: let torch (if installed) load its own first
                import torch  # noqa: F401
            except Exception:
                pass
        L = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)  # AttributeError here == header / library mismatch
            fn.restype, fn.argtypes = res, args
        if L.rc_abi_version() != 3:
            raise RecodeHipError("librecode_hip.so ABI version mismatch")
        _lib = L
    return _lib


def last_error():
    return (lib().rc_last_error() or b"").decode()


def check(status, what=""):
    """Map an rc_status to the exception type the reference raises at the same point."""
    if status >= 0:
        return status
    msg = "%s%s: %s" % (what + ": " if what else "", lib().rc_strerror(status).decode(), last_error())
    if status == RC_ERR_UNSUPPORTED:
        raise NotImplementedError(msg)
    if status in (RC_ERR_BAD_ARG, RC_ERR_RECORD_TOO_LARGE, RC_ERR_OUT_TOO_SMALL, RC_ERR_CORRUPT):
        raise ValueError(msg)
    if status == RC_ERR_WORKSPACE:
        raise MemoryError(msg)
    raise RecodeHipError(msg)


def device_count():
    n = C.c_int(0)
    check(lib().rc_device_count(C.byref(n)))
    return n.value


def ptr(a):
    """Address of a numpy array's data, or an int address (e.g. torch.Tensor.data_ptr()) passed through."""
    if isinstance(a, np.ndarray):
        if not a.flags["C_CONTIGUOUS"]:
            raise ValueError("array must be C-contiguous")
        return a.ctypes.data
    if a is None:
        return None
    return int(a)


def shift_rows(shifts, n=None, what="shifts"):
    """Per-frame shifts as the aligned adds take them: an integer array-like of shape (n, 2), (dy, dx) per frame -> C-contiguous int32[n, 2].
    A float (or any non-integer) dtype, another shape and a value outside int32 are ValueError: nothing is rounded or wrapped silently."""
    a = np.asarray(shifts)
    if a.dtype.kind not in "iu":
        raise ValueError("%s: an integer array of (dy, dx) rows, not dtype %s (round the shifts yourself)" % (what, a.dtype))
    if a.ndim != 2 or a.shape[1] != 2 or (n is not None and a.shape[0] != int(n)):
        raise ValueError("%s: shape %s, wanted (%s, 2)" % (what, a.shape, "n" if n is None else int(n)))
    if a.size and (int(a.min()) < -(1 << 31) or int(a.max()) > (1 << 31) - 1):
        raise ValueError("%s: a value outside int32" % what)
    return np.ascontiguousarray(a, dtype=np.int32)


PIPE_SLOTS = 3


class PinnedBuffer:
    """Page-locked host memory (rc_host_alloc) seen as a numpy uint8 array: the staging the streaming form copies from / to
    without the HIP runtime's intermediate copy."""

    def __init__(self, nbytes):
        self.nbytes = int(nbytes)
        self._p = lib().rc_host_alloc(self.nbytes)
        if not self._p:
            raise RecodeHipError("rc_host_alloc(%d): %s" % (self.nbytes, last_error()))
        self.array = np.ctypeslib.as_array((C.c_uint8 * max(self.nbytes, 1)).from_address(self._p))[:self.nbytes]

    def close(self):
        p, self._p = getattr(self, "_p", None), None
        if p and _lib is not None:
            self.array = None
            _lib.rc_host_free(p)

    __del__ = close


class FrameSum:
    """A summed view on the device: rc_sum_create .. rc_sum_destroy (include/recode_hip.h) - one uint32 cell per pixel that batches of
    stored frames are added into, whichever reader they come from.  `geom` is the tuple the batched readers pass to rc_expand_frames:
    (nx, ny, bit_depth, reduction_level, op_mode, scheme); its nx, ny must be the handle's.  One thread uses a handle at a time."""

    LIMIT = 0xFFFFFFFF        # what a cell holds: an add that could pass it is refused (RC_ERR_OUT_TOO_SMALL -> ValueError)

    def __init__(self, nx, ny):
        st = C.c_int(0)
        self.nx, self.ny = int(nx), int(ny)
        self._h = lib().rc_sum_create(self.nx, self.ny, C.byref(st))
        if not self._h:
            check(st.value, "rc_sum_create")

    @property
    def handle(self):
        return self._h

    def _codec(self, geom):
        if (int(geom[0]), int(geom[1])) != (self.nx, self.ny):
            raise ValueError("FrameSum: frames of %d x %d added to a view of %d x %d" % (geom[0], geom[1], self.nx, self.ny))
        return tuple(int(v) for v in geom[2:6])

    @staticmethod
    def grows_by(geom, n):
        """what a batch of n frames adds to bound()"""
        return int(n) * (((1 << int(geom[2])) - 1) if int(geom[3]) == 1 else 1)

    def add_status(self, geom, data, sizes, n, prefix=None):
        """rc_sum_add_frames, status returned (the readers fall back on RC_ERR_UNSUPPORTED / RC_ERR_CORRUPT)"""
        return lib().rc_sum_add_frames(self._h, *self._codec(geom), ptr(data), ptr(sizes), n, ptr(prefix))

    def add(self, geom, data, sizes, n):
        """Add n stored frames (data: their blobs back to back, sizes uint32[n][3] - as rc_expand_frames takes them); returns the
        frames' set-pixel prefix uint64[n + 1].  A rejected batch raises and adds nothing."""
        prefix = np.zeros(n + 1, np.uint64)
        check(self.add_status(geom, data, sizes, n, prefix), "rc_sum_add_frames")
        return prefix

    def submit_status(self, slot, geom, data, sizes, n):
        return lib().rc_sum_add_frames_submit(self._h, slot, *self._codec(geom), ptr(data), ptr(sizes), n)

    def submit(self, slot, geom, data, sizes, n):
        """Queue the batch on slot 0 or 1 (data stays valid until rc_expand_frames_wait(slot) has returned, which gives the verdict)."""
        check(self.submit_status(slot, geom, data, sizes, n), "rc_sum_add_frames_submit")

    # ---- aligned views (rc_sum_add_frames_shifted): frame f lands shifts[f] = (dy, dx) cells away, what leaves the view is dropped -----------
    def add_shifted_status(self, geom, data, sizes, n, shifts, prefix=None):
        """rc_sum_add_frames_shifted, status returned; shifts: int32[n, 2] (shift_rows)"""
        return lib().rc_sum_add_frames_shifted(self._h, *self._codec(geom), ptr(data), ptr(sizes), n, ptr(shift_rows(shifts, n)), ptr(prefix))

    def add_shifted(self, geom, data, sizes, n, shifts):
        """add() with frame f translated by shifts[f] = (dy, dx) whole pixels; the prefix counts the frames' set pixels, placed or not"""
        prefix = np.zeros(n + 1, np.uint64)
        check(self.add_shifted_status(geom, data, sizes, n, shifts, prefix), "rc_sum_add_frames_shifted")
        return prefix

    def submit_shifted_status(self, slot, geom, data, sizes, n, shifts):
        """rc_sum_add_frames_shifted_submit (the library copies the shifts before it returns)"""
        return lib().rc_sum_add_frames_shifted_submit(self._h, slot, *self._codec(geom), ptr(data), ptr(sizes), n, ptr(shift_rows(shifts, n)))

    def submit_shifted(self, slot, geom, data, sizes, n, shifts):
        check(self.submit_shifted_status(slot, geom, data, sizes, n, shifts), "rc_sum_add_frames_shifted_submit")

    def add_counted_shifted_status(self, geom, data, sizes, n, shifts, method=0, area_threshold=0, upsample=1, prefix=None):
        """rc_sum_add_counted_shifted, status returned; shifts in FINE cells (1 / upsample pixel)"""
        return lib().rc_sum_add_counted_shifted(self._h, *self._codec_counted(geom, upsample), ptr(data), ptr(sizes), n, int(method), int(area_threshold),
                                                ptr(shift_rows(shifts, n)), ptr(prefix))

    def add_counted_shifted(self, geom, data, sizes, n, shifts, method=0, area_threshold=0, upsample=1):
        """add_counted() with frame f's counts translated by shifts[f] = (dy, dx) fine cells; the prefix counts the kept events, placed or not"""
        prefix = np.zeros(n + 1, np.uint64)
        check(self.add_counted_shifted_status(geom, data, sizes, n, shifts, method, area_threshold, upsample, prefix), "rc_sum_add_counted_shifted")
        return prefix

    def submit_counted_shifted_status(self, slot, geom, data, sizes, n, shifts, method=0, area_threshold=0, upsample=1):
        """rc_sum_add_counted_shifted_submit on slot 0 or 1"""
        nx, ny, s, *codec = self._codec_counted(geom, upsample)
        return lib().rc_sum_add_counted_shifted_submit(self._h, slot, nx, ny, s, *codec, ptr(data), ptr(sizes), n, int(method), int(area_threshold),
                                                       ptr(shift_rows(shifts, n)))

    # ---- counted views (rc_sum_add_counted): one count per event of the frames, on a grid `upsample` times finer than theirs --------------
    def _codec_counted(self, geom, upsample):
        s = int(upsample)
        if (s * int(geom[0]), s * int(geom[1])) != (self.nx, self.ny):
            raise ValueError("FrameSum: frames of %d x %d counted at upsample %d into a view of %d x %d" % (geom[0], geom[1], s, self.nx, self.ny))
        return (int(geom[0]), int(geom[1]), s) + tuple(int(v) for v in geom[2:6])

    @staticmethod
    def grows_by_counted(geom, sizes, n):
        """what a counted batch of n frames adds to bound(): per frame the components it can hold - an aligned 2 x 2 block of pixels belongs
        to at most one - and, at level 1, no more than the set pixels its value stream has room for"""
        nx, ny, d, level = (int(v) for v in geom[:4])
        blocks = ((nx + 1) // 2) * ((ny + 1) // 2)
        if level != 1:
            return int(n) * blocks
        return sum(min(blocks, 8 * int(b) // d) for b in np.asarray(sizes).reshape(-1, 3)[:int(n), 2])

    def add_counted_status(self, geom, data, sizes, n, method=0, area_threshold=0, upsample=1, prefix=None):
        """rc_sum_add_counted, status returned; method: the code (reader_batched.count_method)"""
        return lib().rc_sum_add_counted(self._h, *self._codec_counted(geom, upsample), ptr(data), ptr(sizes), n, int(method), int(area_threshold), ptr(prefix))

    def add_counted(self, geom, data, sizes, n, method=0, area_threshold=0, upsample=1):
        """Count n stored frames' events (rc_count_frames' components, method and area_threshold) into the view, which is `upsample` times
        finer than the frames: a FrameSum(upsample * nx, upsample * ny).  Returns the frames' EVENT prefix uint64[n + 1].  A rejected batch
        raises and adds nothing."""
        prefix = np.zeros(n + 1, np.uint64)
        check(self.add_counted_status(geom, data, sizes, n, method, area_threshold, upsample, prefix), "rc_sum_add_counted")
        return prefix

    def submit_counted_status(self, slot, geom, data, sizes, n, method=0, area_threshold=0, upsample=1):
        """rc_sum_add_counted_submit on slot 0 or 1; rc_expand_frames_wait(slot) gives the verdict and the event prefix"""
        nx, ny, s, *codec = self._codec_counted(geom, upsample)
        return lib().rc_sum_add_counted_submit(self._h, slot, nx, ny, s, *codec, ptr(data), ptr(sizes), n, int(method), int(area_threshold))

    def fetch(self, reset=False, out=None):
        """uint32[ny, nx]: the cells, after every queued add; reset=True zeroes them and the bound"""
        if out is None:
            out = np.empty((self.ny, self.nx), np.uint32)
        elif not isinstance(out, np.ndarray) or out.dtype != np.uint32 or out.size != self.ny * self.nx or not out.flags["C_CONTIGUOUS"]:
            raise ValueError("FrameSum.fetch: out must be a C-contiguous uint32 array of ny * nx = %d cells" % (self.ny * self.nx))
        check(lib().rc_sum_fetch(self._h, ptr(out), 1 if reset else 0), "rc_sum_fetch")
        return out

    def fetch_view(self, reset=False):
        """fetch() into page-locked memory of this handle's (one copy over the link, no staging through the runtime's bounce buffers:
        a 4096 x 4096 view is 67 MB): a VIEW, valid until the next fetch_view() or close()"""
        if getattr(self, "_pin", None) is None:
            self._pin = PinnedBuffer(4 * self.nx * self.ny)
        return self.fetch(reset, self._pin.array.view(np.uint32).reshape(self.ny, self.nx))

    def bound(self):
        """the largest value a cell can hold so far - an UPPER bound: a batch that was queued (submit) and that the device then refused
        added nothing, but has been counted"""
        return int(lib().rc_sum_bound(self._h))

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h and _lib is not None:
            _lib.rc_sum_destroy(h)
        pin, self._pin = getattr(self, "_pin", None), None
        if pin is not None:
            pin.close()

    __del__ = close


def library_device():
    """The device the library's handle-making and batch calls run on: RC_DEVICE when it is set, otherwise torch's current device."""
    import torch
    return int(os.environ["RC_DEVICE"]) if os.environ.get("RC_DEVICE") else torch.cuda.current_device()


def on_library_device(tensor, who, what):
    """ValueError for a GPU tensor that does not live on library_device(): a handle copies it there on streams of its own"""
    if tensor.device.index != library_device():
        raise ValueError("%s: %s on %s, the handle is made on cuda:%d (the current device, or RC_DEVICE)" % (who, what, tensor.device, library_device()))


def int32_planes(weights, nx, ny, max_planes, who, what="weights"):
    """(the planes as C-contiguous int32[k, ny, nx] - numpy, or torch on the GPU -, k): what FrameTrace takes as weights and FrameCorrelation
    as its reference (max_planes 1).  `who` and `what` word the ValueError of anything else."""
    if weights is None:
        return None, 0
    on_gpu = hasattr(weights, "data_ptr") and not isinstance(weights, np.ndarray)
    if on_gpu and not weights.is_cuda:
        weights, on_gpu = weights.numpy(), False
    if not on_gpu and not isinstance(weights, np.ndarray):
        raise ValueError("%s: %s must be a numpy array or a torch tensor" % (who, what))
    shape = tuple(int(v) for v in weights.shape)
    if len(shape) == 2:
        shape = (1,) + shape
    if len(shape) != 3 or shape[1:] != (ny, nx) or not 1 <= shape[0] <= max_planes:
        raise ValueError("%s: %s of shape %s - (ny, nx) or (k, ny, nx) with ny, nx = %d, %d and 1 <= k <= %d"
                         % (who, what, tuple(weights.shape), ny, nx, max_planes))
    lo, hi = -(1 << 31), (1 << 31) - 1
    if on_gpu:
        import torch
        if weights.dtype.is_floating_point or weights.dtype.is_complex or weights.dtype == torch.bool:
            raise ValueError("%s: %s of dtype %s (an integer dtype that fits int32)" % (who, what, weights.dtype))
        # The library runs on the caller's current device (RC_DEVICE overrides it) and on streams of its own: the tensor must live on that
        # device, and everything queued on it - the kernels that produced the weights, the int32 copy below - must have finished before
        # the handle's create call reads it (the library's streams are not ordered behind torch's).
        on_library_device(weights, who, what)
        if weights.dtype not in (torch.int8, torch.int16, torch.int32, torch.uint8) and weights.numel():
            # (unsigned 32- and 64-bit values are judged through the signed view of the same width: what does not fit int32 is negative
            # there, or above 2^31 - 1; torch reduces signed dtypes only)
            signed = {getattr(torch, "uint16", None): torch.int32, getattr(torch, "uint32", None): torch.int32, getattr(torch, "uint64", None): torch.int64}
            seen = weights if weights.dtype not in signed else weights.to(torch.int32) if weights.element_size() == 2 else weights.view(signed[weights.dtype])
            floor = lo if weights.dtype not in signed else 0
            if not (floor <= int(seen.min()) and int(seen.max()) <= hi):
                raise ValueError("%s: %s do not fit int32" % (who, what))
        planes = weights.reshape(shape).to(torch.int32).contiguous()
        torch.cuda.synchronize(weights.device)
        return planes, shape[0]
    if weights.dtype.kind not in "iu":
        raise ValueError("%s: %s of dtype %s (an integer dtype that fits int32)" % (who, what, weights.dtype))
    if weights.size and not (lo <= int(weights.min()) and int(weights.max()) <= hi):
        raise ValueError("%s: %s do not fit int32" % (who, what))
    return np.ascontiguousarray(weights.reshape(shape), dtype=np.int32), shape[0]


class _FrameTable:
    """What FrameTrace, FrameCorrelation and FrameBins share: a handle (rc_<kind>_create .. rc_<kind>_destroy, include/recode_hip.h) that
    keeps one read-only plane on the device and turns a batch of stored frames into an int64 table, one row of out_shape(1) per frame.  A
    subclass names its entry points' prefix and the verb of the geometry refusal, converts its input and calls _create, and says out_shape(n)."""

    _prefix = None      # "rc_trace", "rc_corr", "rc_bins"
    _verb = None        # "frames of .. <verb> with a handle of .."

    def __init__(self, nx, ny):
        self.nx, self.ny = int(nx), int(ny)
        self._h = None

    def _create(self, param, plane):
        """rc_<kind>_create(nx, ny, param, plane): `plane` (numpy, a torch tensor, or None) is kept alive until the call has copied it"""
        st = C.c_int(0)
        addr = None if plane is None else plane.data_ptr() if hasattr(plane, "data_ptr") else ptr(plane)
        self._h = getattr(lib(), self._prefix + "_create")(self.nx, self.ny, param, addr, C.byref(st))
        if not self._h:
            check(st.value, self._prefix + "_create")

    @property
    def handle(self):
        return self._h

    def _codec(self, geom):
        if (int(geom[0]), int(geom[1])) != (self.nx, self.ny):
            raise ValueError("%s: frames of %d x %d %s with a handle of %d x %d" % (type(self).__name__, geom[0], geom[1], self._verb, self.nx, self.ny))
        return tuple(int(v) for v in geom[2:6])

    def frames_status(self, geom, data, sizes, n, out, out_cells, prefix=None):
        """rc_<kind>_frames, status returned (the readers fall back on RC_ERR_UNSUPPORTED / RC_ERR_CORRUPT); out: an array or an address"""
        return getattr(lib(), self._prefix + "_frames")(self._h, *self._codec(geom), ptr(data), ptr(sizes), n, ptr(out), out_cells, ptr(prefix))

    def frames(self, geom, data, sizes, n):
        """The table of n stored frames (data: their blobs back to back, sizes uint32[n][3] - as rc_expand_frames takes them):
        (int64 of out_shape(n) - the class says what a row holds -, the frames' set-pixel prefix uint64[n + 1]).  A rejected batch raises."""
        out, prefix = np.empty(self.out_shape(n), np.int64), np.zeros(n + 1, np.uint64)
        check(self.frames_status(geom, data, sizes, n, out, out.size, prefix), self._prefix + "_frames")
        return out, prefix

    def submit_status(self, slot, geom, data, sizes, n, out, out_cells):
        """rc_<kind>_frames_submit on slot 0 or 1 (out: device or page-locked memory; data stays valid until rc_expand_frames_wait(slot) has
        returned, which gives the verdict and the prefix)"""
        return getattr(lib(), self._prefix + "_frames_submit")(self._h, slot, *self._codec(geom), ptr(data), ptr(sizes), n, ptr(out), out_cells)

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h and _lib is not None:
            getattr(_lib, self._prefix + "_destroy")(h)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    __del__ = close


class FrameTrace(_FrameTable):
    """Frame traces on the device: rc_trace_create .. rc_trace_destroy (include/recode_hip.h) - per frame of a batch of stored frames the
    number of set pixels, the sum of their values, the sums weighted by row and by column, and the sums under k weight planes the handle
    keeps a copy of: int64[n, 4 + k], exact.  weights: None (the four moments alone), or a numpy array / a torch tensor on the GPU of shape
    (ny, nx) or (k, ny, nx), k <= 16, of an integer dtype whose values fit int32; anything else raises ValueError.  A tensor must be on the device the library runs on - the
    current device, or RC_DEVICE -; its device is synchronised before the handle copies it, so a tensor that kernels of the caller are still
    writing is read when they are done.  `geom` is the tuple the
    batched readers pass to rc_expand_frames: (nx, ny, bit_depth, reduction_level, op_mode, scheme); its nx, ny must be the handle's.  One
    thread uses a handle at a time; the weights are read-only, so batches on both slots may share it."""

    MAX_PLANES = 16
    _prefix, _verb = "rc_trace", "traced"

    def __init__(self, nx, ny, weights=None):
        super().__init__(nx, ny)
        planes, self.k = int32_planes(weights, self.nx, self.ny, self.MAX_PLANES, "FrameTrace")
        self._create(self.k, planes)

    @property
    def columns(self):
        return 4 + self.k

    def out_shape(self, n):
        return (n, self.columns)

    def weight_bounds(self):
        """max |W_m| of every plane, as the handle holds them for the no-wrap rule (INT32_MIN counts as 2^31)"""
        return [int(lib().rc_trace_weight_bound(self._h, m)) for m in range(self.k)]


class FrameCorrelation(_FrameTable):
    """Correlation surfaces on the device: rc_corr_create .. rc_corr_destroy (include/recode_hip.h) - per frame of a batch of stored frames
    the overlap of its set pixels with a reference image at every offset of a window, int64[n, S, S] with S = 2 * radius + 1, exact:
    out[f, dy + R, dx + R] = sum v * reference[row + dy, col + dx] (0 outside the image).  reference: a numpy array / a torch tensor on the
    GPU of shape (ny, nx) of an integer dtype whose values fit int32 (what FrameTrace takes as one plane, with its rules for a tensor's
    device), or a FrameSum of that shape, whose cells are fetched on the device - refused (ValueError) when its bound() exceeds 2^31 - 1.
    radius: 0..16.  The handle keeps its own zero-bordered copy; batches on both slots and several readers may share it.  `geom` as for
    FrameTrace."""

    MAX_RADIUS = 16
    _prefix, _verb = "rc_corr", "correlated"

    def __init__(self, nx, ny, reference, radius=8):
        super().__init__(nx, ny)
        self.radius = int(radius)
        if not 0 <= self.radius <= self.MAX_RADIUS:
            raise ValueError("FrameCorrelation: radius %d (0 .. %d)" % (self.radius, self.MAX_RADIUS))
        plane = self._from_sum(reference) if isinstance(reference, FrameSum) else int32_planes(reference, self.nx, self.ny, 1, "FrameCorrelation", "reference")[0]
        self._create(self.radius, plane)

    def _from_sum(self, fs):
        """a FrameSum's cells as an int32 tensor on its device: rc_sum_fetch with a device destination, no trip over the link.  The cells
        are uint32; up to 2^31 - 1 they are the same bits as int32, and the handle's bound says whether any can be larger"""
        if (fs.nx, fs.ny) != (self.nx, self.ny):
            raise ValueError("FrameCorrelation: a FrameSum of %d x %d as the reference of frames of %d x %d" % (fs.nx, fs.ny, self.nx, self.ny))
        if fs.bound() > (1 << 31) - 1:
            raise ValueError("FrameCorrelation: the FrameSum's cells may exceed 2^31 - 1 (bound %d): they do not fit int32" % fs.bound())
        import torch
        cells = torch.empty((self.ny, self.nx), dtype=torch.int32, device="cuda:%d" % library_device())
        check(lib().rc_sum_fetch(fs._h, cells.data_ptr(), 0), "rc_sum_fetch")      # (returns with the copy done)
        return cells

    @property
    def side(self):
        return 2 * self.radius + 1

    def out_shape(self, n):
        return (n, self.side, self.side)

    def reference_bound(self):
        """max |reference| as the handle holds it for the no-wrap rule (INT32_MIN counts as 2^31)"""
        return int(lib().rc_corr_reference_bound(self._h))


class FrameBins(_FrameTable):
    """Binned frame traces on the device: rc_bins_create .. rc_bins_destroy (include/recode_hip.h) - per frame of a batch of stored frames
    and per bin of a label map the number of set pixels and the sum of their values, int64[n, 2, B] ([:, 0] the counts, [:, 1] the sums),
    exact.  labels: a numpy array / a torch
    tensor on the GPU of shape (ny, nx) of any integer dtype whose values fit uint16 (a tensor by FrameTrace's rules for its device), each
    cell a bin 0 .. B - 1 or 0xFFFF ("in no bin").  n_bins: B, 1 .. 4096; None: max(label != 0xFFFF) + 1 (1 when every pixel is ignored).
    The handle keeps its own copy; batches on both slots and several readers may share it.  `geom` as for FrameTrace."""

    MAX_BINS = 4096
    IGNORE = 0xFFFF
    _prefix, _verb = "rc_bins", "binned"

    def __init__(self, nx, ny, labels, n_bins=None):
        super().__init__(nx, ny)
        plane, top = self._uint16_labels(labels)
        self.n_bins = top + 1 if n_bins is None else int(n_bins)
        if not 1 <= self.n_bins <= self.MAX_BINS:
            raise ValueError("FrameBins: n_bins %d (1 .. %d)" % (self.n_bins, self.MAX_BINS))
        if top >= self.n_bins:
            raise ValueError("FrameBins: a label of %d with n_bins %d (bins are 0 .. n_bins - 1, 0xFFFF is 'in no bin')" % (top, self.n_bins))
        self._create(self.n_bins, plane)

    def _uint16_labels(self, labels):
        """(the labels as C-contiguous uint16[ny, nx] - numpy, or torch on the GPU as int16 of the same bits -, the largest label that is
        not 0xFFFF - 0 when there is none)"""
        on_gpu = hasattr(labels, "data_ptr") and not isinstance(labels, np.ndarray)
        if on_gpu and not labels.is_cuda:
            labels, on_gpu = labels.numpy(), False
        if not on_gpu and not isinstance(labels, np.ndarray):
            raise ValueError("FrameBins: labels must be a numpy array or a torch tensor")
        if tuple(int(v) for v in labels.shape) != (self.ny, self.nx):
            raise ValueError("FrameBins: labels of shape %s - (ny, nx) = (%d, %d)" % (tuple(labels.shape), self.ny, self.nx))
        if on_gpu:
            import torch
            if labels.dtype.is_floating_point or labels.dtype.is_complex or labels.dtype == torch.bool:
                raise ValueError("FrameBins: labels of dtype %s (an integer dtype whose values fit uint16)" % labels.dtype)
            on_library_device(labels, "FrameBins", "labels")      # (and the ordering before rc_bins_create reads it: as for FrameTrace's weights)
            unsigned = {getattr(torch, "uint16", None): torch.int32, getattr(torch, "uint32", None): torch.int64, getattr(torch, "uint64", None): torch.int64}
            # (torch reduces signed dtypes: uint16 and uint32 widen, uint64 is judged through its signed view - too large is negative there)
            wide = labels.view(torch.int64) if labels.dtype == getattr(torch, "uint64", None) else labels.to(unsigned.get(labels.dtype, labels.dtype))
            if wide.numel() and not (0 <= int(wide.min()) and int(wide.max()) <= 0xFFFF):
                raise ValueError("FrameBins: labels do not fit uint16")
            kept = wide[wide != self.IGNORE]
            top = int(kept.max()) if kept.numel() else 0
            plane = wide.to(torch.int32).to(torch.int16).contiguous() if wide.dtype != torch.int16 else wide.contiguous()   # (the low 16 bits)
            torch.cuda.synchronize(labels.device)
            return plane, top
        if labels.dtype.kind not in "iu":
            raise ValueError("FrameBins: labels of dtype %s (an integer dtype whose values fit uint16)" % labels.dtype)
        if labels.size and not (0 <= int(labels.min()) and int(labels.max()) <= 0xFFFF):
            raise ValueError("FrameBins: labels do not fit uint16")
        kept = labels[labels != self.IGNORE]
        return np.ascontiguousarray(labels, dtype=np.uint16), (int(kept.max()) if kept.size else 0)

    def out_shape(self, n):
        return (n, 2, self.n_bins)


class ReduceContext:
    """One writer's device state: rc_ctx_create .. rc_ctx_destroy.  Mirrors what ReCoDeWriter.start() sets up
    (reference recode_writer.py:212-230) plus the threshold frame of __init__ (:126-137)."""

    def __init__(self, nx, ny, src_bit_depth, reduction_level=1, op_mode=1, scheme=2, clevel=1, device_id=0, max_batch=16, src_dtype=np.uint16,
                 device_zlib=False):
        """src_dtype: numpy dtype of the frames and the dark frame - uint16, or uint8 (source_bit_depth <= 8: rc_ctx_set_source_bytes)
        device_zlib: compression_scheme 0 encoded by the device's DEFLATE encoder (valid zlib streams, not stock zlib's bytes).  clevel 0 / 1:
        the binary map is coded, the packed values are stored blocks; clevel >= 2 (reduction level 1): the packed values are Huffman-coded
        too - a literals-only dynamic block per 32 KiB chunk that pays, under one table fitted to the ctx's first batch (refit_model()
        fits it again); a record never grows over its clevel-1 form"""
        if device_zlib and scheme == 0 and op_mode == 1:
            scheme = RC_SCHEME_ZLIB_DEVICE
        st = C.c_int(0)
        self.src_dtype = np.dtype(src_dtype)
        if self.src_dtype not in (np.dtype(np.uint16), np.dtype(np.uint8), np.dtype(np.uint32)):
            raise NotImplementedError("source dtype %s: the device path takes unsigned integer frames (uint8, uint16, uint32)" % self.src_dtype)
        self._h = lib().rc_ctx_create(nx, ny, src_bit_depth, reduction_level, op_mode, scheme, clevel, device_id, max_batch,
                                      C.byref(st))
        if not self._h:
            check(st.value, "rc_ctx_create")
        self.nx, self.ny, self.depth, self.level = nx, ny, src_bit_depth, reduction_level
        self.op_mode, self.scheme, self.max_batch, self.device_id = op_mode, scheme, max_batch, device_id
        self.n_pixels = nx * ny
        self.bitmap_bytes = (self.n_pixels + 7) // 8
        self.on_device_codec = bool(op_mode == 1 and lib().rc_scheme_on_device(scheme))
        if self.src_dtype.itemsize != 2:
            st = lib().rc_ctx_set_source_bytes(self._h, self.src_dtype.itemsize)
            if st != RC_OK:
                self.close()
                check(st, "rc_ctx_set_source_bytes")

    @property
    def handle(self):
        return self._h

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h and _lib is not None:  # _lib is None during interpreter shutdown
            _lib.rc_ctx_destroy(h)

    __del__ = close

    def set_stream(self, hip_stream):
        check(lib().rc_ctx_set_stream(self._h, hip_stream), "rc_ctx_set_stream")

    def set_dark(self, dark, epsilon=0):
        dark = np.ascontiguousarray(dark, dtype=self.src_dtype) if isinstance(dark, np.ndarray) else dark
        check(lib().rc_set_dark(self._h, ptr(dark), int(epsilon)), "rc_set_dark")

    def set_threshold(self, thr):
        if isinstance(thr, np.ndarray):   # uint16 thresholds for uint8 and uint16 sources, uint32 ones for uint32 sources (include/recode_hip.h)
            thr = np.ascontiguousarray(thr, dtype=np.uint32 if self.src_dtype.itemsize == 4 else np.uint16)
        check(lib().rc_set_threshold(self._h, ptr(thr)), "rc_set_threshold")

    def out_capacity(self, n):
        return lib().rc_out_capacity(self._h, n)

    def reduce_compress_batch(self, frames, first_frame_id=0, out=None):
        """frames: uint16[n, ny, nx] (numpy; uint8 for a ctx of uint8 sources).  Returns (out u8 array, rec_offsets u64[n+1], md u32[n,3])."""
        frames = np.ascontiguousarray(frames, dtype=self.src_dtype)
        n = frames.shape[0]
        if out is None:
            out = np.empty(self.out_capacity(n), np.uint8)
        rec = np.zeros(n + 1, np.uint64)
        md = np.zeros((n, 3), np.uint32)
        check(lib().rc_reduce_compress_batch(self._h, ptr(frames), n, first_frame_id, ptr(out), out.size, ptr(rec), ptr(md)),
              "rc_reduce_compress_batch")
        return out, rec, md

    def enqueue(self, frames_dev, n, first_frame_id, out_dev, out_cap, rec_dev, md_dev):
        check(lib().rc_reduce_compress_batch_async(self._h, ptr(frames_dev), n, first_frame_id, ptr(out_dev), out_cap,
                                                   ptr(rec_dev), ptr(md_dev)), "rc_reduce_compress_batch_async")

    def sync(self):
        check(lib().rc_ctx_sync(self._h), "rc_ctx_sync")

    def set_pipelined(self, on=True):
        """Let the next batch's reduce kernel overlap this batch's scans / layout / assembly (include/recode_hip.h)."""
        check(lib().rc_ctx_set_pipelined(self._h, 1 if on else 0), "rc_ctx_set_pipelined")

    def wait_results(self, stream_handle=None):
        """Order `stream_handle` (None: the ctx's stream) behind the most recent batch's records."""
        check(lib().rc_ctx_wait_results(self._h, C.c_void_p(stream_handle) if stream_handle else None), "rc_ctx_wait_results")

    # ---- host streaming form (include/recode_hip.h, rc_pipe_*) ---------------------------------------------------------
    def pipe_submit(self, slot, frames_host, n, first_frame_id):
        check(lib().rc_pipe_submit(self._h, slot, ptr(frames_host), n, first_frame_id), "rc_pipe_submit")

    def pipe_input_done(self, slot):
        check(lib().rc_pipe_input_done(self._h, slot), "rc_pipe_input_done")

    def pipe_result(self, slot, n):
        """Wait for the slot's batch: (rec_offsets u64[n+1], md u32[n,3], total record bytes)."""
        rec = np.zeros(n + 1, np.uint64)
        md = np.zeros((n, 3), np.uint32)
        total = C.c_uint64(0)
        check(lib().rc_pipe_result(self._h, slot, ptr(rec), ptr(md), C.byref(total)), "rc_pipe_result")
        return rec, md, total.value

    def pipe_fetch(self, slot, dst_host, nbytes):
        check(lib().rc_pipe_fetch(self._h, slot, ptr(dst_host), nbytes), "rc_pipe_fetch")

    def pipe_fetch_wait(self, slot):
        check(lib().rc_pipe_fetch_wait(self._h, slot), "rc_pipe_fetch_wait")

    def set_validation(self, gap, x0=0, y0=0, w=0, h=0):
        """Validation frames on the streaming path: count the ROI's connected components on the device (include/recode_hip.h)."""
        check(lib().rc_ctx_set_validation(self._h, int(gap), int(x0), int(y0), int(w), int(h)), "rc_ctx_set_validation")

    def pipe_validation(self, slot, n):
        """uint32[n]: component count of the ROI per frame of the slot's batch, 0xFFFFFFFF where the frame is no validation frame."""
        counts = np.zeros(n, np.uint32)
        check(lib().rc_pipe_validation(self._h, slot, ptr(counts)), "rc_pipe_validation")
        return counts

    def refit_model(self):
        """zstd, modelled encoder: fit the entropy tables again to the next batch (include/recode_hip.h)."""
        check(lib().rc_ctx_refit_model(self._h), "rc_ctx_refit_model")

    def binary_map(self, i):
        out = np.empty(self.bitmap_bytes, np.uint8)
        check(lib().rc_get_binary_map(self._h, i, ptr(out)), "rc_get_binary_map")
        return out

    def set_l2_statistics(self, code):
        check(lib().rc_ctx_set_l2_statistics(self._h, int(code)), "rc_ctx_set_l2_statistics")

    def keep_binary_maps(self, on=True):
        check(lib().rc_ctx_keep_binary_maps(self._h, 1 if on else 0))

    def set_profiling(self, on=True, every=1):
        """Stage events on the asynchronous path; every = k > 1: around every k-th batch only."""
        check(lib().rc_ctx_set_profiling(self._h, (max(int(every), 1) if on else 0)))

    def profile(self):
        """(sum_ms[5], batches) accumulated by the asynchronous path since set_profiling()."""
        s, n = (C.c_double * 5)(), C.c_uint64(0)
        check(lib().rc_ctx_get_profile(self._h, s, C.byref(n)))
        return list(s), n.value

    def stage_ms(self):
        ms = (C.c_float * 5)()
        check(lib().rc_get_stage_ms(self._h, ms))
        return list(ms)
