"""The batched side of ReCoDeReader (no counterpart in the reference, which reads frame by frame): many frames per device call
(rc_expand_frames & co.), the streaming iterators, part files indexed for batched access, the host-decoded path for streams only a
stock decoder takes, and the read-ahead that serves the reference's own frame-at-a-time calls out of batches.  ReCoDeReader
(recode_reader.py) inherits BatchedAccess; the methods here use its file handle, header, metadata table and COO helpers.
"""
import os
from contextlib import contextmanager
from types import SimpleNamespace

import numpy as np

from . import recode_compressors as compressors
from . import _lib
from .misc import effective_cpus


def _pinned(buf, nbytes):
    """a _lib.PinnedBuffer of at least `nbytes`: `buf` itself when it is large enough, else a new one with a quarter to spare (`buf` is
    closed first).  A caller that needs slack behind its data asks for it in `nbytes`."""
    if buf is None or buf.nbytes < nbytes:
        if buf is not None:
            buf.close()
        buf = _lib.PinnedBuffer(max(int(nbytes * 1.25), 1 << 20))
    return buf


def _l1_cap(sizes, d):
    """level 1: a frame's packed stream holds one d-bit field per set pixel, so its size bounds the batch's entries without a counting call"""
    return max(int((sizes[:, 2].astype(np.uint64) * 8 // d).sum()), 1)


def _slot_taken(st):
    """the library's two streaming slots are per process and device: this status of a submit call says that ANOTHER iterator (another
    reader's) holds the slot.  The batch then goes through the synchronous call, which has resources of its own."""
    return st == _lib.RC_ERR_BAD_ARG and 'submitted batch' in _lib.last_error()


def _stock_decoded(h):
    """whether the stock decoders on the thread pool take the streams of this file (then one device call expands the stored pieces): the
    route of host-only schemes (zlib / bz2 / lzma) and of zstd / LZ4 streams the device decoders refused"""
    return int(h['reduction_level']) in (1, 3) and int(h['rc_operation_mode']) == 1 and int(h['compression_scheme']) in (0, 1, 2, 4, 5)


def _route(h, foreign, device_blosc, device_zlib, family):
    """Which way a file's batches go, decided in this one place: ('device', the scheme code they are offered to the device decoders under),
    ('host-decode', None) - stock decoders on the thread pool, then one device call on the stored pieces - or ('per-frame', None).
    foreign: the device decoders refused this file's streams once (ReCoDeReader._foreign_file).  family: what the ladder's kinds name
    (_Kind.family, asked by _offer with the kind's switches) - 'triplets' (_Entries: get_frames_triplets, iter_frames_triplets, the
    read-ahead), 'l2' (_L2: get_frames_l2, iter_frames_l2) or 'sum' (every other kind: the summed and counted views, the events, dense
    batches, traces).  The entry points of 'triplets' and 'l2' ask it once more beforehand: a 'per-frame' file does not enter the ladder,
    and a 'host-decode' file streams through _iter_host_decoded.  The families differ, and each difference is tested behaviour: 'triplets' offers blosc-LZ4 and zlib only behind its switches (device_blosc,
    device_zlib); 'sum' has no such history to keep and offers both by default - zlib as RC_SCHEME_ZLIB_DEVICE, which refuses every zlib
    stream but this library's own; 'l2' needs fields of 8 to 16 bits and has no host-decoded route."""
    level, mode, scheme = int(h['reduction_level']), int(h['rc_operation_mode']), int(h['compression_scheme'])
    zlib = level in (1, 3) and mode == 1 and scheme == 0 and not foreign
    if family == 'l2':
        taken, schemes, zlib = 8 <= int(h['target_bit_depth']) <= 16, (1, 2, 8), False
    elif family == 'sum':
        taken, schemes = True, (1, 2, 8)
    else:
        taken, schemes, zlib = level in (1, 3), (1, 2, 8) if device_blosc else (1, 2), zlib and bool(device_zlib)
    if taken and (mode == 0 or (scheme in schemes and not foreign)):
        return 'device', scheme
    if taken and zlib:
        return 'device', _lib.RC_SCHEME_ZLIB_DEVICE
    if family != 'l2' and _stock_decoded(h):
        return 'host-decode', None
    return 'per-frame', None


COUNT_METHODS = {'weighted_average': 0, 'unweighted_average': 1, 'max': 2}


def count_method(method):
    """rc_count_frames' code of a method name of the reference's l1_to_l4_converter"""
    if method not in COUNT_METHODS:
        raise ValueError("method must be one of 'weighted_average', 'unweighted_average', 'max'")
    return COUNT_METHODS[method]


def plan_sub_volume(key, shape):
    """What numpy's stack[key] selects, per axis, for a key of slices and integers (one per axis of `shape`), restated for a reader that
    walks forwards: a list of (start, count, step, flip, drop) - the `count` indices start, start + step, ... with step > 0, ascending;
    flip: numpy delivers them in the opposite order (a negative step); drop: the axis was indexed with an integer and is not in the
    result.  stack[key] == take(those indices)[::-1 where flip] with the dropped axes indexed at 0.  None bounds, negative indices and
    bounds beyond the axis follow numpy (slice.indices); an integer out of range raises IndexError."""
    import operator
    if not isinstance(key, tuple) or len(key) != len(shape):
        raise IndexError('one slice or integer per axis')
    plan = []
    for k, size in zip(key, shape):
        size = int(size)
        if isinstance(k, slice):
            r = range(*k.indices(size))
            if len(r) == 0:
                plan.append((0, 0, 1, False, False))
            elif r.step > 0:
                plan.append((r.start, len(r), r.step, False, False))
            else:
                plan.append((r[-1], len(r), -r.step, True, False))
        else:
            i = operator.index(k)
            if not -size <= i < size:
                raise IndexError('index %d is out of bounds for an axis of size %d' % (i, size))
            plan.append((i % size, 1, 1, False, True))
    return plan


def centre_of_mass(traces):
    """(row, col) as float64 arrays from a dict of get_frame_traces / iter_frame_traces: sum_row / sum and sum_col / sum per frame - the
    intensity centre of mass in pixel coordinates -, NaN for a frame whose sum is 0"""
    s = np.asarray(traces['sum'], np.float64)
    safe = np.where(s != 0, s, 1.0)
    row = np.where(s != 0, np.asarray(traces['sum_row'], np.float64) / safe, np.nan)
    col = np.where(s != 0, np.asarray(traces['sum_col'], np.float64) / safe, np.nan)
    return row, col


def estimate_shifts(corr, group=1):
    """Per-frame shifts from the surfaces of get_frame_correlations / iter_frame_correlations: corr is int64[n, S, S] (or the dict that holds
    it as 'corr'), S = 2 R + 1.  The surfaces of each run of `group` consecutive frames are summed first (correlation is linear: a fraction's
    surface is the sum of its frames'; the last group may be shorter) - ValueError when group * max|corr| could pass 2^63 - 1.  Per group
    the peak is the largest cell, ties broken by the smallest dy^2 + dx^2, then the smallest dy, then the smallest dx - an all-zero surface
    gives (0, 0).  Returns a dict of arrays with one entry per FRAME, every frame of a group carrying its group's: 'shifts' int32[n, 2] -
    (dy, dx), as sum_frames(shifts=...) takes them -, 'peak' int64[n], 'on_border' bool[n] - |dy| == R or |dx| == R: the drift may exceed
    the window -, 'valid' bool[n] - peak > 0 -, and 'refined' float64[n, 2]: the shift plus, per axis, the vertex of the parabola through
    the peak and its two neighbours, computed as a Fraction of Python integers and converted once (offset 0 on the border or where the
    denominator is 0).  For counted views multiply `refined` by upsample and round."""
    from fractions import Fraction
    c = np.asarray(corr['corr'] if isinstance(corr, dict) else corr)
    if c.ndim != 3 or c.shape[1] != c.shape[2] or c.shape[1] % 2 != 1 or c.dtype.kind not in 'iu':
        raise ValueError('estimate_shifts: corr of shape %s, dtype %s - wanted integer [n, S, S] with S odd' % (c.shape, c.dtype))
    group = int(group)
    if group < 1:
        raise ValueError('estimate_shifts: group must be at least 1')
    n, S = c.shape[0], c.shape[1]
    R = S // 2
    c = c.astype(np.int64, copy=False)
    if n and group * max(abs(int(c.min())), abs(int(c.max()))) > (1 << 63) - 1:
        raise ValueError('estimate_shifts: the sum of %d surfaces could pass 2^63 - 1' % group)
    out = {'shifts': np.zeros((n, 2), np.int32), 'peak': np.zeros(n, np.int64), 'on_border': np.zeros(n, bool), 'valid': np.zeros(n, bool),
           'refined': np.zeros((n, 2), np.float64)}
    d = np.arange(-R, R + 1)
    # the tie-break as one key per cell, smallest first: dy^2 + dx^2, then dy, then dx
    key = ((d[:, None] ** 2 + d[None, :] ** 2) * S + (d[:, None] + R)) * S + (d[None, :] + R)
    for a in range(0, n, group):
        g = c[a:a + group].sum(axis=0, dtype=np.int64)
        peak = int(g.max())
        at = int(np.argmin(np.where(g == peak, key, key.max() + 1)))
        iy, ix = divmod(at, S)
        dy, dx = iy - R, ix - R
        border = abs(dy) == R or abs(dx) == R
        fine = [Fraction(dy), Fraction(dx)]
        if not border:
            for axis, (lo, hi) in enumerate(((g[iy - 1, ix], g[iy + 1, ix]), (g[iy, ix - 1], g[iy, ix + 1]))):
                lo, hi = int(lo), int(hi)
                den = 2 * (lo - 2 * peak + hi)
                if den != 0:
                    fine[axis] += Fraction(lo - hi, den)
        rows = slice(a, a + group)
        out['shifts'][rows] = (dy, dx)
        out['peak'][rows] = peak
        out['on_border'][rows] = border
        out['valid'][rows] = peak > 0
        out['refined'][rows] = (float(fine[0]), float(fine[1]))
    return out


def radial_labels(ny, nx, cy, cx, bin_width=1, n_bins=None):
    """The label map of a radial (azimuthal) profile for get_frame_bins / _lib.FrameBins: uint16[ny, nx], pixel (r, c) in bin
    isqrt((2 r - 2 cy)^2 + (2 c - 2 cx)^2) // (2 * bin_width) - floor(distance from (cy, cx) / bin_width) in exact integers.  cy, cx: integers
    or odd halves (2 cy and 2 cx must be integers: a centre on a pixel or between two); bin_width: a positive integer.  n_bins: the bins
    kept, 1 .. 4096 - a pixel beyond the last one gets 0xFFFF ("in no bin"); None: every bin the frame reaches (ValueError above 4096)."""
    ny, nx, w = int(ny), int(nx), int(bin_width)
    cy2, cx2 = 2 * cy, 2 * cx
    if cy2 != int(cy2) or cx2 != int(cx2):
        raise ValueError('radial_labels: cy and cx must be integers or odd halves')
    if ny < 1 or nx < 1 or w < 1 or w != bin_width:
        raise ValueError('radial_labels: ny, nx and bin_width must be positive integers')
    cy2, cx2 = int(cy2), int(cx2)
    dy, dx = 2 * np.arange(ny, dtype=np.int64) - cy2, 2 * np.arange(nx, dtype=np.int64) - cx2
    if max(abs(int(dy[0])), abs(int(dy[-1]))) >= 1 << 30 or max(abs(int(dx[0])), abs(int(dx[-1]))) >= 1 << 30:
        raise ValueError('radial_labels: the centre is too far from the frame')
    sq = dy[:, None] ** 2 + dx[None, :] ** 2                       # below 2^61
    root = np.floor(np.sqrt(sq.astype(np.float64))).astype(np.int64)
    root -= root * root > sq                                        # (the float square root is off by one at most: put right in integers)
    root += (root + 1) * (root + 1) <= sq
    bins = root // (2 * w)
    top = int(bins.max()) + 1
    if n_bins is None:
        n_bins = top
        if n_bins > 4096:
            raise ValueError('radial_labels: the frame reaches %d bins (4096 at most: a larger bin_width, or n_bins)' % n_bins)
    n_bins = int(n_bins)
    if not 1 <= n_bins <= 4096:
        raise ValueError('radial_labels: n_bins %d (1 .. 4096)' % n_bins)
    return np.where(bins < n_bins, bins, 0xFFFF).astype(np.uint16)


def bin_areas(labels, n_bins):
    """int64[n_bins]: the pixels of every bin of a label map (0xFFFF and anything at or above n_bins: in no bin) - the denominator of a mean
    profile, sum / (count of frames * area) or count / area"""
    labels = np.asarray(labels)
    if labels.dtype.kind not in 'iu':
        raise ValueError('bin_areas: labels of dtype %s (an integer dtype)' % labels.dtype)
    n_bins = int(n_bins)
    flat = labels.reshape(-1).astype(np.int64)
    return np.bincount(flat[(flat >= 0) & (flat < n_bins)], minlength=n_bins).astype(np.int64)


def _event_views(buf, cap, total):
    """(rows int32, cols int32, area uint32, weight uint64): the first `total` events of rc_count_frames' output of capacity `cap`"""
    return (buf[8 * cap:12 * cap].view(np.int32)[:total], buf[12 * cap:16 * cap].view(np.int32)[:total],
            buf[16 * cap:20 * cap].view(np.uint32)[:total], buf[:8 * cap].view(np.uint64)[:total])


def count_frames_now(geom, data, sizes, k, method, area_threshold):
    """One synchronous rc_count_frames for k frames, their streams back to back in `data` and offered under geom = (nx, ny, bit depth,
    level, op_mode, scheme): (status, event prefix, (rows, cols, area, weight) - None unless the status is RC_OK).  Events <= set
    pixels: level 1 bounds them from the sizes; levels 2 and 3 need the counting call first."""
    L = _lib.lib()
    prefix = np.zeros(k + 1, np.uint64)
    args = tuple(geom) + (_lib.ptr(data), _lib.ptr(sizes), k, method, area_threshold)
    if geom[3] == 1:
        cap = _l1_cap(sizes, geom[2])
    else:
        st = L.rc_count_frames(*args, _lib.ptr(prefix), None, 0)
        if st != _lib.RC_OK:
            return st, prefix, None
        cap = max(int(prefix[k]), 1)
    buf = np.empty(20 * cap, np.uint8)
    st = L.rc_count_frames(*args, _lib.ptr(prefix), _lib.ptr(buf), cap)
    return st, prefix, _event_views(buf, cap, int(prefix[k])) if st == _lib.RC_OK else None


def _area_threshold(area_threshold):
    thr = int(area_threshold)
    if not 0 <= thr < 1 << 32:
        raise ValueError('area_threshold must fit 32 bits')
    return thr


class _Kind:
    """What the ladder (BatchedAccess._offer / _settle) is told about the kind of result a batch becomes; one small subclass per kind.
    geom is a batch's tuple for rc_expand_frames - (nx, ny, bit depth, level, op_mode, scheme) -, and every rung of the ladder makes the
    same call under another one: the file's own, the stored pieces' (.., 0, scheme) of a host-decoded batch, _stored_pieces_per_frame's.
    What a kind keeps between the calls for a job is in job.payload, next to the ladder's own fields."""
    what = None                           # the library call, as _lib.check's messages name it (queued: what + '_submit')
    verdict = 'rc_expand_frames_wait'     # ... and as they name a streamed batch's verdict
    family, switches = 'sum', ()          # what _route is asked with: the route family, and (device_blosc, device_zlib) where it has them
    retry = ()                            # verdicts of a queued batch that send it through the synchronous call once before it is judged

    @staticmethod
    def queues(level):
        """whether batches of this level go through the two slots (False: the synchronous call, which counts first)"""
        return True

    def room(self, job, geom, sizes, k):
        """prepares the job's output for a batch of k frames under geom: called once before every rung's call(s)"""

    def call(self, job, geom, data, sizes, k, slot=None):
        """the device call, status returned: queued on `slot`, or (None) synchronous"""
        raise NotImplementedError

    def per_frame(self, reader, job):
        """the bottom rung: the frame-at-a-time reader's frames restated as stored ones, through the same call"""
        geom, data, sizes = reader._stored_pieces_per_frame(job.first, job.count, job.frames)
        self.room(job, geom, sizes, job.count)
        _lib.check(self.call(job, geom, data, sizes, job.count), self.what)

    def item(self, job):
        """what the stream yields for a finished job (None: nothing)"""


class _PlainAdder(_Kind):
    """A batch's frames added into a _lib.FrameSum, their values (rc_sum_add_frames / _submit): the job's payload names the handle (fs),
    its window and whether it is the window's last job.  fold(fs, grow), where set, is called before an add that grows fs's bound by
    `grow` - the host-decoded and per-frame adds included, so a batch that was queued and then refused grows the bound twice.
    shifts: None, or (dy, dx) rows for frames z0 .. z0 + n - 1 of the call, checked against n (_lib.shift_rows) (rc_sum_add_frames_shifted / _submit): every rung of the ladder -
    the device decoders, the host-decoded batch, the per-frame restatement - then makes the shifted call, with the rows of the job's frames."""
    what = 'rc_sum_add_frames'
    fold = None

    def __init__(self, z0=0, shifts=None, n=None):
        self.z0, self.shifts = int(z0), None if shifts is None else _lib.shift_rows(shifts, n)
        if shifts is not None:
            self.what += '_shifted'

    @staticmethod
    def view_shape(nx, ny):
        return nx, ny

    @staticmethod
    def grows_by(geom, sizes, n):
        return _lib.FrameSum.grows_by(geom, n)

    def room(self, job, geom, sizes, k):
        if self.fold is not None:
            self.fold(job.payload.fs, self.grows_by(geom, sizes, k))

    def rows(self, job):
        a = job.first - self.z0
        return self.shifts[a:a + job.count]

    def call(self, job, geom, data, sizes, k, slot=None):
        fs = job.payload.fs
        if self.shifts is None:
            return fs.add_status(geom, data, sizes, k) if slot is None else fs.submit_status(slot, geom, data, sizes, k)
        rows = self.rows(job)
        return fs.add_shifted_status(geom, data, sizes, k, rows) if slot is None else fs.submit_shifted_status(slot, geom, data, sizes, k, rows)

    def item(self, job):
        return job.payload.window if job.payload.last else None


class _CountedAdder(_PlainAdder):
    """The counted add (rc_sum_add_counted / _submit): one count per event of the frames, the view `upsample` times finer than they are.
    Levels 2 and 3 wait for their set-pixel count inside the call: they go through the synchronous one, like the events themselves.
    shifts: as _PlainAdder's, in fine cells (rc_sum_add_counted_shifted / _submit)."""
    what = 'rc_sum_add_counted'

    def __init__(self, method, area_threshold, upsample, z0=0, shifts=None, n=None):
        self.code, self.thr, self.s = count_method(method), _area_threshold(area_threshold), int(upsample)
        if not 1 <= self.s <= 16:
            raise ValueError('upsample must be in 1..16')
        super().__init__(z0, shifts, n)

    @staticmethod
    def queues(level):
        return level == 1

    def view_shape(self, nx, ny):
        return self.s * nx, self.s * ny

    @staticmethod
    def grows_by(geom, sizes, n):
        return _lib.FrameSum.grows_by_counted(geom, sizes, n)

    def call(self, job, geom, data, sizes, k, slot=None):
        fs, how = job.payload.fs, (self.code, self.thr, self.s)
        if self.shifts is None:
            return fs.add_counted_status(geom, data, sizes, k, *how) if slot is None else fs.submit_counted_status(slot, geom, data, sizes, k, *how)
        rows = self.rows(job)
        if slot is None:
            return fs.add_counted_shifted_status(geom, data, sizes, k, rows, *how)
        return fs.submit_counted_shifted_status(slot, geom, data, sizes, k, rows, *how)


class _Events(_Kind):
    """A batch's events (rc_count_frames / _submit): level 1 bounds them from the sizes and is queued, its output the slot's; levels 2 and
    3 have no bound short of their pixels and go through the synchronous call, which counts first (count_frames_now)."""
    what = verdict = 'rc_count_frames'

    def __init__(self, method, area_threshold, outs):
        self.code, self.thr, self.outs = count_method(method), _area_threshold(area_threshold), outs

    @staticmethod
    def queues(level):
        return level == 1

    def call(self, job, geom, data, sizes, k, slot=None):
        p = job.payload
        p.result = None
        if slot is None:
            st, p.prefix, p.result = count_frames_now(geom, data, sizes, k, self.code, self.thr)
            return st
        p.cap = _l1_cap(sizes, geom[2])
        self.outs[2 + slot] = _pinned(self.outs[2 + slot], 20 * p.cap)
        return _lib.lib().rc_count_frames_submit(slot, *geom, _lib.ptr(data), _lib.ptr(sizes), k, self.code, self.thr, self.outs[2 + slot]._p, p.cap)

    def item(self, job):
        p = job.payload
        if p.result is None:          # (the queued call delivered: copies of the slot's output)
            p.result = tuple(a.copy() for a in _event_views(self.outs[2 + job.slot].array, p.cap, int(p.prefix[job.count])))
        return (job.first, p.prefix) + p.result


class _Dense(_Kind):
    """A region of a batch's frames as cells of dt (rc_expand_frames_dense / _submit), written to the slot's page-locked output (outs:
    the reader's stream buffers) - sized before every rung, because the fall-backs write there too - or to `dst`, an address in host or
    device memory, which the synchronous form is given."""
    what = 'rc_expand_frames_dense'

    def __init__(self, region, dt, outs=None, dst=None):
        self.region, self.dt, self.outs, self.dst = tuple(region), dt, outs, dst

    def _cells(self, k):
        return k * self.region[2] * self.region[3]

    def room(self, job, geom, sizes, k):
        if self.outs is not None:
            self.outs[2 + job.slot] = _pinned(self.outs[2 + job.slot], self._cells(k) * self.dt.itemsize)

    def call(self, job, geom, data, sizes, k, slot=None):
        L = _lib.lib()
        dst = self.dst if self.outs is None else self.outs[2 + job.slot]._p
        args = tuple(geom) + (_lib.ptr(data), _lib.ptr(sizes), k) + self.region + (self.dt.itemsize, dst, self._cells(k))
        return L.rc_expand_frames_dense(*args, None) if slot is None else L.rc_expand_frames_dense_submit(slot, *args)

    def item(self, job):
        if self.outs is None:         # (the caller's own memory has been written)
            return None
        k, (w, h) = job.count, self.region[2:4]
        return job.payload.index, self.outs[2 + job.slot].array[:self._cells(k) * self.dt.itemsize].view(self.dt).reshape(k, h, w)


class _Tables(_Kind):
    """A batch's per-frame table (rc_trace_frames, rc_corr_frames or rc_bins_frames / _submit on `handle`, the _lib.FrameTrace,
    FrameCorrelation or FrameBins): int64 of handle.out_shape(k) in the slot's page-locked output, handed out as as_dict(first, k, cells)
    makes it - as_dict(first, k, cells, prefix) with `with_prefix`, for a dict that holds the frames' set pixels.  The synchronous call's
    set-pixel prefix is kept where a waited-for verdict's is (job.payload.prefix): whichever call answered last says how many pixels the
    frames have."""

    def __init__(self, handle, outs, as_dict, with_prefix=False):
        self.handle, self.outs, self.as_dict, self.with_prefix = handle, outs, as_dict, with_prefix
        self.what = handle._prefix + '_frames'

    def _cells(self, k):
        return int(np.prod(self.handle.out_shape(k)))

    def room(self, job, geom, sizes, k):
        self.outs[2 + job.slot] = _pinned(self.outs[2 + job.slot], 8 * self._cells(k))

    def call(self, job, geom, data, sizes, k, slot=None):
        out = (self.outs[2 + job.slot]._p, self._cells(k))
        if slot is not None:
            return self.handle.submit_status(slot, geom, data, sizes, k, *out)
        job.payload.prefix = np.zeros(k + 1, np.uint64)
        return self.handle.frames_status(geom, data, sizes, k, *out, job.payload.prefix)

    def item(self, job):
        k = job.count
        cells = self.outs[2 + job.slot].array[:8 * self._cells(k)].view(np.int64).reshape(self.handle.out_shape(k))
        return job.first, self.as_dict(job.first, k, cells, *((job.payload.prefix,) if self.with_prefix else ()))


def _device_path(dev):
    """last_batch_path of a batch the device decoders took under scheme `dev`"""
    return 'device-inflate' if dev == _lib.RC_SCHEME_ZLIB_DEVICE else 'device'


class _Job:
    """One batch of a streaming pipeline: frames first .. first + count - 1 - or the `count` frames that `frames` lists, ascending -, the
    device slot (0 or 1) it goes through, whether it is queued there (submitted and not yet waited for), and what its family keeps
    between start and finish."""
    __slots__ = ('first', 'count', 'slot', 'queued', 'payload', 'frames')

    def __init__(self, first, count, payload=None, frames=None):
        self.first, self.count, self.slot, self.queued, self.payload, self.frames = first, count, 0, False, payload, frames


def _jobs(z0, n, batch):
    return [_Job(a, min(batch, z0 + n - a)) for a in range(z0, z0 + n, batch)]


def _wait(job):
    """the verdict on a queued job: (status, nnz prefix uint64[count + 1])"""
    prefix = np.zeros(job.count + 1, np.uint64)
    st = _lib.lib().rc_expand_frames_wait(job.slot, _lib.ptr(prefix))
    job.queued = False
    return st, prefix


def _drain(job):
    """a consumer that stops early leaves a job queued: wait for it before its buffers go away (the verdict is of no interest)"""
    if job is not None and job.queued:
        _wait(job)


class _BatchBuffers:
    """What a reader's batched access allocates on first use and keeps until the reader is closed: page-locked buffers, host blobs, the
    mapped file and the thread pools.  close() waits for the pools and frees everything."""

    def __init__(self):
        self.pin_blob = None                  # page-locked image of a batch's file bytes (the synchronous calls)
        self.stream = [None] * 4              # [blob 0, blob 1, output 0, output 1] of the streaming iterators' two slots
        self.l2 = [None, None]                # page-locked statistics of iter_frames_l2's two slots
        self.pin_pieces = [None] * 3          # stored-pieces images of host-decoded batches: two for the iterator, one for the synchronous call
        self.host_blobs = [None, None]        # file bytes for the host decoders where the file cannot be mapped
        self.file_map = None                  # the file, mapped, for the host decoders
        self.pools = {}

    def pool(self, name, workers):
        """the thread pool `name`: 'read' (a few threads for page-cache reads), 'decode' (stock decoders of the Python level) or 'coord'
        (the thread that decodes one batch ahead, _iter_host_decoded)"""
        if name not in self.pools:
            from concurrent.futures import ThreadPoolExecutor
            self.pools[name] = ThreadPoolExecutor(max_workers=workers)
        return self.pools[name]

    def mapped(self, fp):
        if self.file_map is None:
            import mmap
            try:
                self.file_map = mmap.mmap(fp.fileno(), 0, access=mmap.ACCESS_READ)
            except (OSError, ValueError):
                pass                              # (not mappable: positional reads into a buffer instead)
        return self.file_map

    def close(self):
        for p in self.pools.values():
            p.shutdown(wait=True)
        for b in [self.pin_blob] + self.stream + self.l2 + self.pin_pieces:
            if b is not None:
                b.close()
        if self.file_map is not None:
            try:
                self.file_map.close()
            except BufferError:                # (a caller still holds a view of a batch: the map goes with it)
                pass
        self.__init__()


class _BatchOut:
    """Where a batch's expanded entries go and how they are laid out: the reference's uint64 (row, col, value) rows (24 bytes a set
    pixel; rc_expand_frames), or the three arrays of the COO matrix its reader wraps them into - int32 rows | int32 columns | values,
    each `cap` entries long.  value_bytes is the width of a value: 2 (uint16, 10 bytes an entry; rc_expand_frames_coo) or 4 (uint32, 12
    bytes; rc_expand_frames_coo32 - level-1 files of more than 16 bits, see for_file).  holder: None (an array of its own per call) or a
    list whose element `at` is a _lib.PinnedBuffer / None (page-locked, reused, grown when too small: results are views, valid until its
    next use)."""

    def __init__(self, coo=False, holder=None, value_bytes=2, at=0):
        if value_bytes not in (2, 4):
            raise ValueError('COO values are uint16 or uint32')
        self.coo, self.holder, self.at, self.value_bytes = bool(coo), holder, at, int(value_bytes)
        self.esz = 8 + self.value_bytes if coo else 24
        self.buf, self.cap = None, 0

    @classmethod
    def for_file(cls, header, coo=False, holder=None, at=0):
        """the layout for a file: its COO values are uint32 when it is a level-1 file whose fields are wider than 16 bits (what the
        reference's reader returns for it: recode_reader.py:464-471, misc.py:41-52), uint16 otherwise"""
        wide = int(header['reduction_level']) == 1 and int(header['target_bit_depth']) > 16
        return cls(coo, holder, 4 if wide else 2, at)

    def room(self, cap):
        nbytes = cap * self.esz
        if self.holder is None:
            self.buf = np.empty(nbytes, np.uint8)
        else:
            self.holder[self.at] = _pinned(self.holder[self.at], nbytes)
            self.buf = self.holder[self.at].array[:nbytes]
        self.cap = cap
        return self

    def ptr(self):
        return _lib.ptr(self.buf)

    def fn(self, L, submit=False):
        name = 'rc_expand_frames' + (('_coo32' if self.value_bytes == 4 else '_coo') if self.coo else '') + ('_submit' if submit else '')
        return getattr(L, name)

    def result(self, total):
        return self.views(self.buf, self.cap, total, self.coo, self.value_bytes)

    @staticmethod
    def views(buf, cap, total, coo, value_bytes=2):
        """the first `total` entries of a buffer of capacity `cap` in the layout (coo, value_bytes)"""
        if not coo:
            return buf[:total * 24].view(np.uint64).reshape(total, 3)
        vt = np.uint32 if value_bytes == 4 else np.uint16
        return (buf[:4 * cap].view(np.int32)[:total], buf[4 * cap:8 * cap].view(np.int32)[:total],
                buf[8 * cap:(8 + value_bytes) * cap].view(vt)[:total])

    @staticmethod
    def from_triplets(trip, coo, value_bytes=2):
        """the frame-at-a-time path's triplets in the layout asked for"""
        if not coo:
            return trip
        return (trip[:, 0].astype(np.int32), trip[:, 1].astype(np.int32), trip[:, 2].astype(np.uint32 if value_bytes == 4 else np.uint16))


class _Entries(_Kind):
    """A batch's set pixels as triplet rows or as the COO arrays (rc_expand_frames, _coo, _coo32 / _submit: the layout is
    _BatchOut.for_file's).  Level 1 bounds them from the sizes and is queued; level 3 needs the counting call, which the synchronous form
    has.  out: the caller's holder of the synchronous form (get_frames_triplets' `out`); slots: the reader's stream buffers, whose outputs
    the queued level takes - that batch's item is a VIEW of the slot's page-locked output, valid until the generator is advanced; any
    other batch's arrays are the call's own.  The bottom rung builds the entries on the host from the frame-at-a-time reader's frames."""
    what, family = 'rc_expand_frames', 'triplets'

    def __init__(self, header, coo=False, out=None, device_blosc=False, device_zlib=False, slots=None):
        self.header, self.coo, self.out, self.slots = header, coo, out, slots
        self.switches = (device_blosc, device_zlib)

    @staticmethod
    def queues(level):
        return level == 1

    def room(self, job, geom, sizes, k):
        holder, at = (self.out, 0) if self.slots is None or geom[3] != 1 else (self.slots, 2 + job.slot)
        job.payload.dst = _BatchOut.for_file(self.header, self.coo, holder, at)
        if geom[3] == 1:
            job.payload.dst.room(_l1_cap(sizes, geom[2]))

    def call(self, job, geom, data, sizes, k, slot=None):
        p, L = job.payload, _lib.lib()
        dst, src, p.result = p.dst, tuple(geom) + (_lib.ptr(data), _lib.ptr(sizes), k), None
        if slot is not None:
            return dst.fn(L, submit=True)(slot, *src, dst.ptr(), dst.cap)
        p.prefix = np.zeros(k + 1, np.uint64)
        if geom[3] != 1:
            st = L.rc_expand_frames(*src, _lib.ptr(p.prefix), None, 0)
            if st != _lib.RC_OK:
                return st
            dst.room(max(int(p.prefix[k]), 1))
        return dst.fn(L)(*src, _lib.ptr(p.prefix), dst.ptr(), dst.cap)

    def per_frame(self, reader, job):
        p, parts, reader.last_batch_path = job.payload, [], 'per-frame'
        p.prefix = np.zeros(job.count + 1, np.uint64)
        for i, m in enumerate(reader._frames_one_by_one(job.first, job.count, job.frames)):
            m = m[0] if isinstance(m, tuple) else m
            t = np.stack([m.row.astype(np.uint64), m.col.astype(np.uint64), m.data.astype(np.uint64)], axis=1) if m is not None and m.nnz \
                else np.zeros((0, 3), np.uint64)
            parts.append(t)
            p.prefix[i + 1] = p.prefix[i] + t.shape[0]
        trip = np.concatenate(parts) if parts else np.zeros((0, 3), np.uint64)
        p.result = _BatchOut.from_triplets(trip, self.coo, _BatchOut.for_file(self.header, self.coo).value_bytes)

    def item(self, job):
        p = job.payload
        return job.first, p.prefix, p.result if p.result is not None else p.dst.result(int(p.prefix[job.count]))


class _L2(_Kind):
    """A level-2 batch's set pixels and summary statistics (rc_expand_frames_l2 / _submit; dtype: the file's, as get_frame returns the
    statistics).  A batch's set pixels cannot be bounded from the metadata: the synchronous call counts first; a stream's first queued
    batch is counted as well, and every later one is given the room the densest batch delivered so far needed per frame (`densest`) plus
    a quarter - one that still does not fit (retry) raises the estimate from its verdict's prefix and goes through the synchronous call.
    outs, stats: the reader's stream buffers and statistics buffers, which the queued form writes; the items are copies of their own."""
    what, family = 'rc_expand_frames_l2', 'l2'
    retry = (_lib.RC_ERR_OUT_TOO_SMALL,)

    def __init__(self, dtype, outs=None, stats=None):
        self.dtype, self.outs, self.stats, self.densest = dtype, outs, stats, None

    def room(self, job, geom, sizes, k):
        job.payload.sp = np.zeros(k + 1, np.int64)        # the statistics prefix: one field of the file's bit depth per component
        np.cumsum(sizes[:, 2].astype(np.int64) * 8 // geom[2], out=job.payload.sp[1:])

    def call(self, job, geom, data, sizes, k, slot=None):
        p, L = job.payload, _lib.lib()
        shape, codec, src, ns, p.result = geom[:3], geom[4:], (_lib.ptr(data), _lib.ptr(sizes), k), int(p.sp[k]), None
        if slot is None and p.prefix is not None:         # (a queued batch that did not fit: its verdict's prefix says what it needs)
            self.densest = max(self.densest or 0, int(p.prefix[k]) / k)
        if slot is None or self.densest is None:
            prefix = np.zeros(k + 1, np.uint64)
            st = L.rc_expand_frames(*shape, 2, *codec, *src, _lib.ptr(prefix), None, 0)      # the counting call sizes rows / columns
            if st != _lib.RC_OK:
                return st
            p.cap = max(int(prefix[k]), 1)
        else:
            p.cap = int(self.densest * k * 1.25) + 1024
        if slot is not None:
            self.outs[2 + slot] = _pinned(self.outs[2 + slot], 8 * p.cap)
            self.stats[slot] = _pinned(self.stats[slot], 2 * max(ns, 1))
            return L.rc_expand_frames_l2_submit(slot, *shape, *codec, *src, self.outs[2 + slot]._p, p.cap, self.stats[slot]._p, ns)
        rc, stats = np.empty(2 * p.cap, np.int32), np.empty(max(ns, 1), np.uint16)
        st = L.rc_expand_frames_l2(*shape, *codec, *src, _lib.ptr(prefix), _lib.ptr(rc), p.cap, _lib.ptr(stats), ns)
        tot, p.prefix = int(prefix[k]), prefix
        if st == _lib.RC_OK:
            p.result = rc[:tot], rc[p.cap:p.cap + tot], stats[:ns].astype(self.dtype, copy=False)
        return st

    def per_frame(self, reader, job):
        p, n, reader.last_batch_path = job.payload, job.count, 'per-frame'
        rows, cols, stats = [], [], []
        p.prefix, p.sp = np.zeros(n + 1, np.uint64), np.zeros(n + 1, np.int64)
        for i, (m, st) in enumerate(reader._frames_one_by_one(job.first, n, job.frames)):
            if m is not None and m.nnz:
                rows.append(m.row.astype(np.int32))
                cols.append(m.col.astype(np.int32))
            if st is not None:
                stats.append(np.asarray(st, self.dtype))
            p.prefix[i + 1] = p.prefix[i] + (m.nnz if m is not None else 0)
            p.sp[i + 1] = p.sp[i] + (len(st) if st is not None else 0)
        cat = lambda parts, dt: np.concatenate(parts) if parts else np.zeros(0, dt)
        p.result = cat(rows, np.int32), cat(cols, np.int32), cat(stats, self.dtype)

    def item(self, job):
        p, k = job.payload, job.count
        if p.result is None:          # (the queued call delivered: copies of the slot's outputs)
            tot, ns = int(p.prefix[k]), int(p.sp[k])
            self.densest = max(self.densest or 0, tot / k)
            rc = self.outs[2 + job.slot].array[:8 * p.cap].view(np.int32)
            p.result = rc[:tot].copy(), rc[p.cap:p.cap + tot].copy(), self.stats[job.slot].array[:2 * ns].view(np.uint16).astype(self.dtype)
        return (job.first, p.prefix) + p.result[:2] + (p.sp,) + p.result[2:]


class BatchedAccess:
    """Mixin of ReCoDeReader: see the module docstring.  State it uses is declared in ReCoDeReader.__init__; its buffers and pools are
    ReCoDeReader._bufs (a _BatchBuffers)."""

    def _load_part_index(self):
        """Intermediate (part) files carry no metadata table: every record is `u32 frame_id | metadata row | data` (reference
        recode_writer.py:559-574).  One walk over the record headers gives the batched readers what the seek table gives them for a
        merged file: per record the metadata row, the data's size and position - and the frame id, in `part_frame_ids`.  A record cut
        short at the end of the file (a writer that was interrupted) ends the index."""
        h = self._header
        level, mode = h['reduction_level'], h['rc_operation_mode']
        fields = self._md_fields()
        hdr = 4 + self._sz_frame_metadata
        std = sum(int(f['bytes']) for f in fields)
        fd = self._fp.fileno()
        pos, ids, mds, sizes, offs = self._frame_data_start_position, [], [], [], []
        while pos + hdr <= self._file_size:
            raw = os.pread(fd, hdr, pos)
            if len(raw) < hdr:
                break
            d, at = {}, 4
            for f in fields:
                d[f['name']] = np.frombuffer(raw, dtype=f['dtype'], count=1, offset=at)[0]
                at += int(f['bytes'])
            size = int(self._structures.get_frame_data_size(level, mode, d))
            if pos + hdr + size > self._file_size:
                break
            ids.append(int(np.frombuffer(raw, np.uint32, 1)[0]))
            mds.append(d)
            sizes.append(size)
            offs.append(pos + hdr - self._frame_data_start_position)
            pos += hdr + size
        assert std <= self._sz_frame_metadata
        self._frame_metadata = mds
        self.part_frame_ids = np.array(ids, np.uint32)
        self._seek_table = np.zeros((len(ids), 2), np.uint64)
        self._seek_table[:, 0] = sizes
        self._seek_table[:, 1] = offs            # (relative to the first record, like a merged file's - but NOT contiguous)

    def _batch_frames(self):
        """number of frames the batched readers can address: nz of a merged file, the records of a part file (indexed on first use)"""
        if self._is_intermediate:
            if self._frame_metadata is None:
                self._load_part_index()
            return len(self._frame_metadata)
        return int(self._header['nz'])

    def _read_batch_into(self, blob, z0, n, move_fp=True):
        """the data of frames z0 .. z0+n-1 -> blob, back to back (what rc_expand_frames takes): one contiguous range of a merged file;
        a part file's records have their headers in between, so frame by frame"""
        lo = self._frame_data_start_position + int(self._seek_table[z0, 1])
        if not self._is_intermediate:
            return self._read_into(blob, lo, move_fp)
        some, total = self._piecewise(blob, range(z0, z0 + n), 'file shorter than its records say')
        nthr = 4 if total >= (8 << 20) and n >= 4 else 1      # (as _read_into: a read from the page cache is a memcpy)
        if nthr == 1:
            return some(0, n)
        cuts = [n * t // nthr for t in range(nthr + 1)]
        list(self._bufs.pool('read', 4).map(lambda t: some(cuts[t], cuts[t + 1]), range(nthr)))

    def _piecewise(self, blob, frames, short):
        """(some, bytes in all): some(lo, hi) reads the data of frames[lo:hi] to their places in `blob`, where the frames that `frames`
        lists lie back to back - one positional read per frame, and more where one comes back short; `short`: what to say of a file
        that ends before a frame does"""
        fd, table, start = self._fp.fileno(), self._seek_table, self._frame_data_start_position
        ats = np.concatenate([[0], np.cumsum(table[list(frames), 0].astype(np.int64))])

        def some(lo, hi):
            for i in range(lo, hi):
                at, end = int(ats[i]), int(ats[i + 1])
                pos = start + int(table[int(frames[i]), 1]) - at
                while at < end:
                    k = os.preadv(fd, [memoryview(blob[at:end])], pos + at)
                    if k <= 0:
                        raise ValueError(short)
                    at += k
        return some, int(ats[-1])

    def _frame_range(self, z0, n, batch=None):
        """the number of frames a batched call covers (n, or None: from z0 to the end), checked against the file.  The synchronous calls
        (batch None) take at least one frame; the iterators take none as well, and a positive batch size"""
        nz = self._batch_frames()
        n = nz - z0 if n is None else n
        if z0 < 0 or z0 + n > nz or (n <= 0 if batch is None else (n < 0 or batch <= 0)):
            raise ValueError('Requested frame index is greater than number of frames in dataset')
        return n

    def _route_for(self, family, device_blosc=False, device_zlib=False):
        return _route(self._header, self._foreign_file, device_blosc, device_zlib, family)

    def _batch_sizes(self, a, k, frames=None):
        """(sizes uint32[k][3] as rc_expand_frames & co. take them, bytes of the k frames' data) of frames a .. a+k-1 - or of the k frames
        whose indices `frames` lists"""
        level = int(self._header['reduction_level'])
        sizes = np.zeros((k, 3), np.uint32)
        ids = range(a, a + k) if frames is None else [int(z) for z in frames]
        for j, z in enumerate(ids):
            md = self._frame_metadata[z]
            sz_map, sz_val = self._stream_sizes(md)
            sizes[j, 0] = sz_map
            if level == 1:
                sizes[j, 1], sizes[j, 2] = sz_val, int(md['bytes_in_packed_pixvals'])
            elif level == 2:
                sizes[j, 1], sizes[j, 2] = sz_val, int(md['bytes_in_packed_summary_stats'])     # (the summed views' device call steps over them)
        return sizes, int(self._seek_table[list(ids), 0].sum())

    def _frames_one_by_one(self, z0, n, frames=None):
        """_get_frame_sparse's result for each of frames z0 .. z0+n-1 (or of those `frames` lists, ascending): the frame-at-a-time path
        under the batched calls (the stock decoder is the judge, and names the frame that is to blame).  Afterwards a part file's
        position - get_next_frame's cursor - is where it was, and a merged file's frame counter is behind the batch."""
        keep = self._fp.tell()
        ids = range(z0, z0 + n) if frames is None else [int(z) for z in frames]
        for z in ids:
            self._fp.seek(self._frame_data_start_position + int(self._seek_table[z, 1]), 0)
            yield self._get_frame_sparse(self._frame_metadata[z])
        if self._is_intermediate:
            self._fp.seek(keep, 0)
        else:
            self._note_batch_end(ids[-1] + 1 if len(ids) else z0)

    def _two_slots(self, jobs, start, finish, stop=None):
        """The driver of the streaming pipelines: two jobs in flight over the list `jobs` (_Job), job j on slot j & 1 of the whole sequence.
        start(job) reads the job's bytes and queues it on the device (job.queued says whether it did); finish(job) waits for it and returns
        the item to yield (None: nothing to yield for this job).  start(j + 1) runs before finish(j): while the device works on one batch
        the next one is read and copied in.  stop(job), asked before the job behind `job` is started, ends the sequence with `job` waited
        for and not finished (the caller goes on from job.first by other means).  However the generator ends - a consumer that stops
        early, an exception -, a job still queued is waited for before its buffers can go away."""
        def begin(j):
            jobs[j].slot, jobs[j].queued = j & 1, False
            start(jobs[j])
            return jobs[j]
        queued = None        # the job started last and not finished
        try:
            queued = begin(0) if jobs else None
            for j in range(len(jobs)):
                job = queued
                if stop is not None and stop(job):
                    return
                queued = begin(j + 1) if j + 1 < len(jobs) else None
                res = finish(job)
                self._note_batch_end(job.first + job.count)
                if res is not None:
                    yield res
        finally:
            if queued is not None:
                try:
                    _drain(queued)
                except Exception:         # (a generator finalised while the interpreter shuts down)
                    pass

    @contextmanager
    def _takes_over_from_readahead(self):
        """What every streaming generator a caller drives is wrapped in.  The read-ahead under get_frame / get_next_frame keeps an iterator
        of its own alive on the same page-locked blobs and slots, with one batch queued on the device: it is ended first (its queued batch
        waited for, the window it serves forgotten), and it stays off while the generator lives (_user_iters)."""
        self._ra = None
        self._close_ra_iter()
        self._user_iters += 1
        try:
            yield
        finally:
            self._user_iters -= 1

    # ---- the ladder: a batch is offered to the device decoders and falls back rung by rung ----------------------------------------------
    def _batch_geom(self, mode, scheme):
        h = self._header
        return int(h['nx']), int(h['ny']), int(h['target_bit_depth']), int(h['reduction_level']), mode, scheme

    def _offer(self, kind, job, sync=False):
        """The ladder's first half, _two_slots' start: the job's file bytes are read into page-locked memory - the slot's blob, or (sync)
        the synchronous calls' - and, where the route of the kind's family names a device scheme, offered to the device decoders as `kind`
        (a _Kind) calls them: queued on the job's slot, or through the synchronous call when the kind does not queue this level, when
        another reader holds the slot, or in the synchronous form.  Of a queued call only RC_OK (job.queued), RC_ERR_UNSUPPORTED and
        RC_ERR_CORRUPT pass; the synchronous call's status is _settle's to judge.  The job's payload keeps sizes, blob, dev (the scheme
        offered under, None: not offered), status and prefix (a waited-for verdict's)."""
        if job.payload is None:
            job.payload = SimpleNamespace()
        p, k, bufs = job.payload, job.count, self._bufs
        p.sizes, nbytes = self._batch_sizes(job.first, k, job.frames)
        if sync:
            bufs.pin_blob = _pinned(bufs.pin_blob, nbytes + 64)
            p.blob = bufs.pin_blob.array[:nbytes]
        else:
            bufs.stream[job.slot] = _pinned(bufs.stream[job.slot], nbytes + 64)
            p.blob = bufs.stream[job.slot].array[:nbytes]
        if job.frames is None:
            self._read_batch_into(p.blob, job.first, k)
        else:
            self._read_frames_into(p.blob, job.frames)
        p.dev, p.status, p.prefix = self._route_for(kind.family, *kind.switches)[1], None, None
        if p.dev is None:
            return
        geom = self._batch_geom(int(self._header['rc_operation_mode']), p.dev)
        call = (job, geom, p.blob, p.sizes, k)
        kind.room(job, geom, p.sizes, k)
        if not sync and kind.queues(geom[3]):
            p.status = kind.call(*call, job.slot)
            if not _slot_taken(p.status):
                if p.status not in (_lib.RC_OK, _lib.RC_ERR_UNSUPPORTED, _lib.RC_ERR_CORRUPT):
                    _lib.check(p.status, kind.what + '_submit')
                job.queued = p.status == _lib.RC_OK
                return
        # a level that waits for its count inside the call, or another reader's iterator holds the slot: the synchronous call has
        # resources of its own
        p.status = kind.call(*call)

    def _settle(self, kind, job, sync=False):
        """The ladder's second half, _two_slots' finish: waits for a queued job's verdict (one the kind lists in `retry` sends the batch
        through the synchronous call once, and that call's status is judged), and takes the batch down the rungs the device decoders
        left - the stock decoders on the thread pool and the same call on the stored pieces, then the frame-at-a-time reader
        (kind.per_frame).  Sets last_batch_path; marks the file foreign when a batch that was offered came out of the stock decoders
        instead.  Returns kind.item(job)."""
        p, k = job.payload, job.count
        st, offered = p.status, p.dev is not None
        if job.queued:
            st, p.prefix = _wait(job)
            if st in kind.retry:
                st = kind.call(job, self._batch_geom(int(self._header['rc_operation_mode']), p.dev), p.blob, p.sizes, k)
        if offered and st == _lib.RC_OK:
            self.last_batch_path = _device_path(p.dev)
        elif offered and st not in (_lib.RC_ERR_UNSUPPORTED, _lib.RC_ERR_CORRUPT):
            _lib.check(st, kind.what if sync else kind.verdict)
        else:
            # refused by the device decoders (a stock encoder's streams, or damage: the stock decoder is the judge), or never theirs
            got = self._host_decode_batch(p.blob, p.sizes, k, 2) if _stock_decoded(self._header) else None
            if got is not None:
                (data, sizes), geom = got, self._batch_geom(0, int(self._header['compression_scheme']))
                kind.room(job, geom, sizes, k)
                _lib.check(kind.call(job, geom, data, sizes, k), kind.what)
            else:
                kind.per_frame(self, job)
            self.last_batch_path = 'host-decode + device-expand' if got is not None else 'per-frame'
            if offered and got is not None:
                self._foreign_file = True        # not offered to the device decoders again
        return kind.item(job)

    def _rungs(self, kind, jobs, stop=None):
        """the streaming form: `jobs` through _offer / _settle on the two slots, the items of `kind` yielded (stop: see _two_slots)"""
        return self._two_slots(jobs, lambda job: self._offer(kind, job), lambda job: self._settle(kind, job), stop)

    def _ladder(self, kind, jobs, stop=None):
        """_rungs as a generator of a caller's own: the read-ahead hands over first"""
        with self._takes_over_from_readahead():
            yield from self._rungs(kind, jobs, stop)

    def _now(self, kind, job):
        """the synchronous form: one job down the ladder on the synchronous calls' blob, nothing queued; kind.item(job)"""
        self._offer(kind, job, sync=True)
        item = self._settle(kind, job, sync=True)
        self._note_batch_end(job.first + job.count)
        return item

    def _straight_per_frame(self, kind, jobs):
        """A file whose route is 'per-frame' does not enter the ladder: its batches are answered straight from kind.per_frame, nothing is
        read into page-locked memory (the frame-at-a-time reader reads the file itself)."""
        for job in jobs:
            job.payload = SimpleNamespace()
            kind.per_frame(self, job)
            yield kind.item(job)

    _RA_FRAMES = 32          # frames fetched ahead once the calls turn out to be sequential
    _RA_BYTES = 512 << 20    # ... as long as their triplets fit into this much page-locked memory
    _RA_PIPELINED = True     # the batch behind the current one is prepared meanwhile (False: one synchronous batched call per window)

    def _readahead_frame(self, z):
        """The frame-at-a-time calls of the reference (get_frame in a loop, get_next_frame) served out of the batched reader: after
        three calls in sequence the frames from z on are fetched a batch at a time (get_frames_triplets into a page-locked buffer
        of this reader's), and the following calls only wrap their rows as COO.  Returns the COO matrix, or None for "take the
        frame-at-a-time path" (not sequential, level 2, an empty frame - whose conventions that path knows -, or a batch the batched
        reader could not deliver: the per-frame path then names the frame that is to blame).  The iterator stays alive between
        calls (the batch behind the current one is prepared meanwhile); one that finds a device slot taken by another reader's sends that
        batch through the synchronous call, so any number of readers in a process may do this side by side."""
        if self._ra_off or int(self._header['reduction_level']) not in (1, 3):
            return None
        if int(self._header['reduction_level']) == 1 and int(self._header['target_bit_depth']) > 32:
            return None        # (the read-ahead's batches come as the COO arrays, whose values are uint32 at most)
        if self._user_iters:
            # a caller's own iter_frames_* on THIS reader is alive: it owns the reader's page-locked batch buffers (the read-ahead's
            # iterator would write the next batch into what that one's arrays view) - these calls go frame by frame meanwhile
            return None
        ra = self._ra
        fetch = False
        if ra is not None and not (ra[0] <= z < ra[0] + ra[1]):
            fetch = z == ra[0] + ra[1]                   # the batch behind the one just used up
            ra = self._ra = None
            if not fetch:
                self._close_ra_iter()
        if ra is None and not fetch:
            last = self._ra_last
            self._ra_streak = self._ra_streak + 1 if last is not None and z == last + 1 else 0
            fetch = self._ra_streak >= 2
        self._ra_last = z
        if ra is None:
            if not fetch:
                return None
            nz = self._batch_frames()
            if nz - z < 2:
                return None
            k, d, level = self._RA_FRAMES, int(self._header['target_bit_depth']), int(self._header['reduction_level'])
            # batches sized by what they expand to (10 or 12 bytes per set pixel): the value stream's length says how many there are; a
            # bitmap-only file does not - one set pixel in ten is assumed
            if level == 1:
                per = max(int(self._frame_metadata[z]['bytes_in_packed_pixvals']) * 8 // d * _BatchOut.for_file(self._header, True).esz, 1)
            else:
                per = max(int(self._header['nx']) * int(self._header['ny']), 1)
            k = min(max(2, min(k, self._RA_BYTES // per)), nz - z)
            if self._ra_buf is None:
                self._ra_buf = [None]
            keep = (self._current_frame_index, self._fp.tell())
            try:
                if self._route_for('triplets')[0] == 'host-decode' or self._RA_PIPELINED:
                    # The streaming iterator, kept alive between calls: while the caller works through this batch the next one is on its
                    # way - decoded by the helper thread (streams only a stock decoder takes), or read, walked and queued on the device
                    # (this library's own streams; the iterator of another reader that finds the slot taken goes through the
                    # synchronous call for that batch, so readers side by side still all get their frames).
                    if self._ra_iter is None or self._ra_iter_at != z:
                        self._close_ra_iter()
                        self._ra_iter = self._iter_frames_impl(z, nz - z, batch=k, coo=True)
                    try:
                        a, prefix, arrays = next(self._ra_iter)
                    except StopIteration:
                        self._close_ra_iter()
                        return None
                    k = len(prefix) - 1
                    self._ra_iter_at = z + k
                else:
                    prefix, arrays = self.get_frames_triplets(z, k, out=self._ra_buf, coo=True)
            except Exception:
                self._close_ra_iter()
                self._ra_off = True
                return None
            finally:
                self._current_frame_index = keep[0]
                self._fp.seek(keep[1], 0)
            if self.last_batch_path == 'per-frame':      # nothing batched about this file: frame by frame it is
                self._ra_off = True
                return None
            ra = self._ra = (z, k, prefix, arrays)
        a, _, prefix, (rows, cols, vals) = ra
        lo, hi = int(prefix[z - a]), int(prefix[z - a + 1])
        if hi == lo:
            return None
        self.readahead_frames_served = self.readahead_frames_served + 1
        # the batch came as the COO arrays themselves (rc_expand_frames_coo / _coo32): the frame's matrix takes its own copies of its slices
        return self._coo_from_arrays(vals[lo:hi].astype(self._numpy_dtype), rows[lo:hi].copy(), cols[lo:hi].copy())

    def _close_ra_iter(self):
        it, self._ra_iter, self._ra_iter_at = self._ra_iter, None, -1
        if it is not None:
            it.close()

    def _drop_readahead(self):
        self._ra = None
        self._close_ra_iter()
        buf = self._ra_buf
        if buf is not None and buf[0] is not None:
            buf[0].close()
        self._ra_buf = None

    # ---- batched access (device-resident decode + expand; no counterpart in the reference, which reads frame by frame) ------
    def get_frames_triplets(self, z0, n, out=None, coo=False, device_blosc=False, device_zlib=False):
        """Frames z0 .. z0+n-1 of a merged file - or records z0 .. z0+n-1 of a part file, whose frame ids are part_frame_ids[z] - in ONE
        device call (rc_expand_frames): both streams of every frame are
        decompressed and expanded on the GPU without a host round trip in between.  Returns (nnz_prefix uint64[n+1],
        triplets uint64[total, 3]) - frame i's (row, col, value) rows are triplets[nnz_prefix[i]:nnz_prefix[i+1]], in the
        reference's row-major order (pyrecode.cpp:95-119).  Falls back to the per-frame path (stock decoder on the host) for
        streams outside the device decoders' subset, for level 2 and for host-only schemes.
        out: None (the triplets come in an array of their own), or a one-element list holding a _lib.PinnedBuffer or None - the
        triplets are then written into that page-locked buffer (grown when too small) and the returned array is a view of it,
        valid until the next call with the same holder.
        coo=True: instead of the triplet rows, (rows int32[total], columns int32[total], values[total]) - the arrays of the COO
        matrices the frame-at-a-time calls return, 10 instead of 24 bytes per set pixel over the link (rc_expand_frames_coo: values
        uint16), or 12 for a level-1 file of more than 16 bits (rc_expand_frames_coo32: values uint32).
        device_blosc=True: a blosc-LZ4 file (compression_scheme 8) at level 1 or 3 goes through the device call as well (the batched
        blosc decoder of rc_expand_frames).  A switch, and off by default, because the path such files take through this call is part of
        its tested behaviour: they read frame by frame, and callers - the read-ahead among them - see 'per-frame' in last_batch_path.
        device_zlib=True: a zlib file (compression_scheme 0) at level 1 or 3 is offered to the batched device inflate (rc_expand_frames with
        RC_SCHEME_ZLIB_DEVICE), which reads the streams of this library's device DEFLATE encoder and refuses every other zlib stream; a
        refused file takes the host-decoded path (the ladder's next rung), as it does without the switch, and is not offered again.  last_batch_path is
        'device-inflate' for a batch the device decoded.  Off by default: the host-decoded path of such files is tested behaviour."""
        n = self._frame_range(z0, n)
        kind, job = _Entries(self._header, coo, out, device_blosc, device_zlib), _Job(z0, n)
        if self._route_for(kind.family, *kind.switches)[0] == 'per-frame':
            return next(self._straight_per_frame(kind, [job]))[1:]
        return self._now(kind, job)[1:]

    def _note_batch_end(self, z):
        if not self._is_intermediate:        # (a part file's sequential cursor is its file position, which the batched readers leave alone)
            self._current_frame_index = z

    def _host_decode_batch(self, blob, sizes, n, slot):
        """The 2 n streams of a batch (file bytes in `blob`, stream sizes in `sizes`) through the stock decoder of the file's scheme on the
        thread pool, each straight into its place of a stored-pieces image in page-locked memory (sizes are known beforehand: the
        binary map's nb bytes, the value stream's bytes_in_packed_pixvals); ONE device call then expands the image (op_mode 0).
        Streams a FOREIGN encoder wrote (the reference's own files: lz4.frame with linked 64 KiB blocks, libzstd with 4-stream literals and
        real offsets) are serial chains of some 10^5 dependent steps per frame - the stock decoder on a CPU core walks one in about a
        millisecond, a GPU lane needs ~1 us per step ("Foreign streams") -, so they are decoded by the SAME library calls the
        reference makes (recode_compressors.py:46-49), all of the batch at once (the libraries release the GIL).  Returns (pieces, sizes of a mode-0 batch), or None when
        there is no stock decoder for the scheme or it rejected a stream.  `slot` picks one of three images: two for the streaming
        iterator (a batch is decoded while the device still copies the previous one in), one for the synchronous call."""
        h = self._header
        level, scheme = int(h['reduction_level']), int(h['compression_scheme'])
        nb = self._structures.binary_image_sz_bytes
        dec = compressors.host_stream_decoder(scheme)
        if dec is None:
            return None
        spans, off, dst = [], 0, 0
        sizes0 = np.zeros((n, 3), np.uint32)
        for i in range(n):
            spans.append((off, int(sizes[i, 0]), dst, nb))
            off += int(sizes[i, 0])
            dst += nb
            sizes0[i, 0] = nb
            if level == 1:
                npk = int(sizes[i, 2])
                spans.append((off, int(sizes[i, 1]), dst, npk))
                off += int(sizes[i, 1])
                dst += npk
                sizes0[i, 1] = sizes0[i, 2] = npk
        images = self._bufs.pin_pieces
        images[slot] = _pinned(images[slot], dst + 64)
        pieces = images[slot].array[:dst]
        # zstd / LZ4 / zlib: the library's own worker threads make the stock library's calls (rc_host_decode_streams) - no
        # interpreter in the loop; the other schemes, or a host without those shared libraries: the Python-level decoders on a pool
        L = _lib.lib()
        if scheme in (0, 1, 2) and L.rc_host_decoder_available(scheme):
            table = np.array([(a, b, c, e) for a, b, c, e in spans], np.uint64).reshape(-1, 4)
            src = np.frombuffer(memoryview(blob), np.uint8)
            st = L.rc_host_decode_streams(scheme, _lib.ptr(src), _lib.ptr(pieces), _lib.ptr(table), table.shape[0], 0)
            if st == _lib.RC_OK:
                return pieces, sizes0
            if st != _lib.RC_ERR_UNSUPPORTED:
                return None                              # a stream the stock decoder rejects: the per-frame path names it
        view = memoryview(blob)

        def one(sp):
            src_off, src_n, at, want = sp
            if want:
                dec(view[src_off:src_off + src_n], want, pieces[at:at + want])
        try:
            spans.sort(key=lambda sp: -sp[1])            # longest streams first: the pool's tail is then a short one
            list(self._bufs.pool('decode', min(16, effective_cpus()[0])).map(one, spans))
        except Exception:
            return None
        return pieces, sizes0

    def _iter_host_decoded(self, z0, n, batch, coo=False):
        """iter_frames_triplets for files whose streams only a stock decoder takes (foreign encoders, zlib / bz2 / lzma): batch i + 1 is
        read and decoded on the host's thread pool while the device expands batch i (rc_expand_frames_submit / _wait, op_mode 0, on the
        page-locked stored-pieces image) and the consumer works on its triplets."""
        geom0 = self._batch_geom(0, int(self._header['compression_scheme']))
        kind = _Entries(self._header, coo, slots=self._bufs.stream)
        jobs = _jobs(z0, n, batch)
        bufs = self._bufs
        coord = bufs.pool('coord', 1)
        file_map = bufs.mapped(self._fp) if not self._is_intermediate else None

        def prepare(i):
            """read and decode job i on the helper thread: its payload is _host_decode_batch's result"""
            job = jobs[i]
            job.slot = i & 1
            sizes, total = self._batch_sizes(job.first, job.count)
            if file_map is not None:
                lo = self._frame_data_start_position + int(self._seek_table[job.first, 1])
                blob = np.frombuffer(file_map, np.uint8, total, lo)             # the decoders read the page cache itself
            else:
                if bufs.host_blobs[job.slot] is None or bufs.host_blobs[job.slot].size < total:
                    bufs.host_blobs[job.slot] = np.empty(int(total * 1.25) + 64, np.uint8)
                blob = bufs.host_blobs[job.slot][:total]
                self._read_batch_into(blob, job.first, job.count, move_fp=False)
            job.payload = self._host_decode_batch(blob, sizes, job.count, job.slot)
            return job

        fut = coord.submit(prepare, 0) if jobs else None
        job = None
        try:
            for i in range(len(jobs)):
                job = fut.result()
                fut = None
                if job.payload is None:
                    # the stock decoder rejected a stream: the synchronous call goes frame by frame and names it (nothing decodes ahead
                    # meanwhile: that call reads the same file and may use the same pools)
                    res = self.get_frames_triplets(job.first, job.count, coo=coo)
                fut = coord.submit(prepare, i + 1) if i + 1 < len(jobs) else None
                if job.payload is not None:
                    (pieces, sizes0), job.payload = job.payload, SimpleNamespace()
                    call = (job, geom0, pieces, sizes0, job.count)
                    kind.room(job, geom0, sizes0, job.count)
                    st = kind.call(*call, job.slot) if kind.queues(geom0[3]) else None
                    if st is None or _slot_taken(st):
                        # level 3 needs a counting call to size its output, and the synchronous form does both; at level 1 another
                        # iterator of this process holds the slot, and the synchronous call has resources of its own
                        _lib.check(kind.call(*call), kind.what)
                    else:
                        _lib.check(st, kind.what + '_submit')
                        job.queued = True
                        st, job.payload.prefix = _wait(job)
                        _lib.check(st, kind.verdict)
                    res = kind.item(job)[1:]
                    self.last_batch_path = 'host-decode + device-expand'
                self._note_batch_end(job.first + job.count)
                yield (job.first,) + res
        finally:
            if fut is not None:
                try:
                    fut.result()          # the decode that runs ahead writes into buffers close() frees
                except Exception:
                    pass
            try:
                _drain(job)
            except Exception:             # (a generator finalised while the interpreter shuts down)
                pass

    def iter_frames_triplets(self, z0=0, n=None, batch=64, coo=False, device_blosc=False, device_zlib=False):
        """The caller's own streaming iterator (documented at _iter_frames_impl; device_blosc, device_zlib: as in get_frames_triplets):
        the read-ahead's, which runs _iter_frames_impl too, is ended first and stays off while this generator lives."""
        with self._takes_over_from_readahead():
            yield from self._iter_frames_impl(z0, n, batch, coo, device_blosc, device_zlib)

    def _iter_frames_impl(self, z0=0, n=None, batch=64, coo=False, device_blosc=False, device_zlib=False):
        """Streams frames z0 .. z0+n-1 of a merged file (records z0 .. of a part file: the reference's own read test sums a part file's
        frames one get_next_frame at a time, tests/recode_v1_read_test.py:9-21) through the batched device reader, two batches in flight
        (rc_expand_frames_submit / _wait): while the device decodes one batch, the next one is read from the file, its block headers
        are walked and its bytes copied in.  Yields (first frame index, nnz_prefix uint64[k+1], triplets uint64[total, 3]) per batch
        of k <= `batch` frames; `triplets` is a VIEW of page-locked memory the device wrote directly - valid until the generator is
        advanced (copy it to keep it).  The batches go down the ladder as entries (_Entries; a level-3 batch through the synchronous call,
        which counts first); a file whose streams only a stock decoder takes - known beforehand, or found out when a batch comes out of
        the stock decoders - goes through _iter_host_decoded (from that batch on), level 2 and what else is left frame by frame.  coo=True: the third item is (rows int32, columns int32, values) instead of the triplet rows -
        10 instead of 24 bytes per set pixel over the link (rc_expand_frames_coo_submit: values uint16), 12 for a level-1 file of more than
        16 bits (rc_expand_frames_coo32_submit: values uint32)."""
        n = self._frame_range(z0, n, batch)
        kind, jobs = _Entries(self._header, coo, None, device_blosc, device_zlib, self._bufs.stream), _jobs(z0, n, batch)
        route = self._route_for(kind.family, *kind.switches)[0]
        if route == 'host-decode':
            yield from self._iter_host_decoded(z0, n, batch, coo)  # stock decoders on the pool, one batch ahead of the device
            return
        if route == 'per-frame':
            yield from self._straight_per_frame(kind, jobs)
            return
        resume = []

        def stop(job):
            """a batch turned out to be a foreign encoder's: the rest of the file, from `job` on, goes through the host-decoded pipeline"""
            if self._foreign_file:
                resume.append(job.first)
            return self._foreign_file
        yield from self._rungs(kind, jobs, stop)         # (not _ladder: the read-ahead's own iterator must not take over from itself)
        if resume:
            yield from self._iter_host_decoded(resume[0], z0 + n - resume[0], batch, coo)

    # ---- level 2 in batches: set pixels and summary statistics (rc_expand_frames_l2) ------------------------------------------
    def _l2_kind(self, what):
        """the _L2 kind of this file, which must be a level-2 file, and whether its batches enter the ladder (else: frame by frame)"""
        if int(self._header['reduction_level']) != 2:
            raise ValueError('%s reads reduction level 2 files' % what)
        return _L2(self._numpy_dtype, self._bufs.stream, self._bufs.l2), self._route_for('l2')[0] == 'device'

    def get_frames_l2(self, z0, n):
        """Frames z0 .. z0+n-1 of a LEVEL-2 file (records of a part file, indexed like get_frames_triplets') in one device call
        (rc_expand_frames_l2): both streams of every frame decoded on the GPU, the binary maps expanded and the statistics unpacked there.
        Returns (nnz_prefix uint64[n+1], rows int32[total], columns int32[total], stats_prefix int64[n+1], stats): frame i's set pixels
        are rows / columns[nnz_prefix[i]:nnz_prefix[i+1]] in row-major order (every value is 1), its summary statistics - one per
        connected component, in label order, in the file's dtype as get_frame returns them - stats[stats_prefix[i]:stats_prefix[i+1]].
        Falls back to the frame-at-a-time path (last_batch_path says which) for fields narrower than 8 bits, host-only schemes and
        streams the device decoders refuse."""
        kind, laddered = self._l2_kind('get_frames_l2')
        job = _Job(z0, self._frame_range(z0, n))
        return (self._now(kind, job) if laddered else next(self._straight_per_frame(kind, [job])))[1:]

    def iter_frames_l2(self, z0=0, n=None, batch=64):
        """Streams a level-2 file through rc_expand_frames_l2_submit / rc_expand_frames_wait, two batches in flight like
        iter_frames_triplets: yields (first frame index, nnz_prefix, rows, columns, stats_prefix, stats) per batch of up to `batch` frames
        (get_frames_l2's items).  rows / columns / stats are copies of their own.  A level-2 batch's set pixels cannot be bounded from
        the metadata, so the first batch is counted on the device and every later one is given the room the densest batch so far
        needed per frame plus a quarter; a batch that still does not fit goes through the synchronous call, which counts first, and one
        the device path does not take goes frame by frame (_L2)."""
        kind, laddered = self._l2_kind('iter_frames_l2')
        jobs = _jobs(z0, self._frame_range(z0, n, batch), batch)
        if laddered:
            yield from self._ladder(kind, jobs)
            return
        with self._takes_over_from_readahead():
            yield from self._straight_per_frame(kind, jobs)

    # ---- summed views (rc_sum_*): frames added up on the device, nothing per set pixel over the link --------------------------------
    def _stored_pieces_per_frame(self, a, k, frames=None):
        """frames a .. a+k-1 (or those `frames` lists) through the frame-at-a-time reader (_get_frame_sparse: the stock decoder is the judge,
        and names the frame that is to blame), restated as stored frames - the binary map, and at level 1 the values packed again at the file's own bit depth:
        (geometry of a mode-0 batch, its bytes, its sizes).  A dense mask, a sort and a pack per frame on the host: the slow route's price."""
        h = self._header
        nx, ny, level, d = int(h['nx']), int(h['ny']), int(h['reduction_level']), int(h['target_bit_depth'])
        nb = (nx * ny + 7) // 8
        sizes, parts = np.zeros((k, 3), np.uint32), []
        shifts = np.arange(d, dtype=np.uint32)
        for i, m in enumerate(self._frames_one_by_one(a, k, frames)):
            m = m[0] if isinstance(m, tuple) else m
            dense, vals = np.zeros(ny * nx, bool), np.zeros(0, np.uint32)
            if m is not None and m.nnz:
                idx = m.row.astype(np.int64) * nx + m.col
                dense[idx] = True
                vals = m.data[np.argsort(idx, kind='stable')].astype(np.uint32)
            parts.append(np.packbits(dense, bitorder='little'))
            sizes[i, 0] = nb
            if level == 1:
                # d-bit fields, LSB first, zero-padded to a byte (recode_writer.py:637-652)
                packed = np.packbits(((vals[:, None] >> shifts) & 1).astype(np.uint8).reshape(-1), bitorder='little')
                parts.append(packed)
                sizes[i, 1] = sizes[i, 2] = packed.size
        return (nx, ny, d, 1 if level == 1 else 3, 0, 0), np.ascontiguousarray(np.concatenate(parts)), sizes

    def _sum_stream(self, windows, batch, adder):
        """The engine of sum_frames and iter_frame_sums: windows = [(first frame, frames > 0, FrameSum)], one after the other; their batches
        go down the ladder (_ladder: rc_sum_add_frames_submit / rc_expand_frames_wait on the two slots) as ONE sequence, so the next batch -
        the next window's first one, into its own handle, included - is read from the file and queued before this one is waited for.
        Yields a window's index once every batch of it has been added.  Every device call is made on the caller's thread.  adder: what is
        added - the frames' values (_PlainAdder) or their events (_CountedAdder).  Routes and fall-backs: see sum_frames."""
        jobs = [_Job(b, min(batch, a + k - b), SimpleNamespace(fs=fs, window=w, last=b + batch >= a + k))
                for w, (a, k, fs) in enumerate(windows) for b in range(a, a + k, batch)]
        return self._ladder(adder, jobs)

    def sum_frames(self, z0=0, n=None, batch=64, into=None, shifts=None):
        """The sum of frames z0 .. z0+n-1 of a merged file (records of a part file) as uint64[ny, nx] - what the reference's viewer and its
        own read test build one get_next_frame at a time (utils/viewer.py:65-68, tests/recode_v1_read_test.py:9-21) -, added up ON THE
        DEVICE (rc_sum_add_frames_submit / rc_expand_frames_wait, two batches in flight: the next batch's bytes are read from the file while
        the device decodes and adds the previous one); 4 bytes per pixel cross the link at the end instead of 10 per set pixel per frame.
        Level 1: the sum of the pixels' values; levels 2 and 3: the number of frames in which a pixel is set.  The device's cells are uint32:
        before a batch could take one past 2^32 - 1 the view is fetched, folded into the uint64 result and reset.
        into: a _lib.FrameSum of this file's shape - the frames are added into it (with those of other readers), nothing is fetched, and the
        number of frames added is returned; a sum that could pass 2^32 - 1 raises ValueError, with the batches before it added.  The
        handle's bound() is an UPPER bound: a batch the device queued and then refused (the first one or two batches of a stock encoder's
        file, which are then decoded on the host and added again) has grown it twice, so a caller's handle can be refused up to two
        batches' share early.
        Routes, per batch (last_batch_path): the device decoders ("device", "device-inflate"); for streams they refuse and for host-only
        schemes the stock decoders on the thread pool, then one add of the stored pieces ("host-decode + device-expand"); what is left
        goes through the frame-at-a-time reader ("per-frame").  Files of more than 16 bits are not taken (NotImplementedError).
        shifts: None, or an integer array-like of shape (n, 2) - (dy, dx) whole pixels for frames z0 .. z0 + n - 1: what frame f adds to
        pixel (r, c) it then adds to (r + dy_f, c + dx_f), and what leaves the view is dropped (rc_sum_add_frames_shifted, on every route).
        A float dtype, another shape or a value outside int32 is a ValueError."""
        n = self._frame_range(z0, n, batch)
        self._check_levels_and_bits(*self._SUMS)
        return self._sum_into(z0, n, batch, into, _PlainAdder(z0, shifts, n))

    def _sum_into(self, z0, n, batch, into, adder):
        """sum_frames and sum_frames_counted behind their argument checks"""
        vx, vy = adder.view_shape(int(self._header['nx']), int(self._header['ny']))
        fs = into if into is not None else _lib.FrameSum(vx, vy)
        total = None if into is not None else np.zeros((vy, vx), np.uint64)

        def fold(view, grow):
            """this call's own view is folded before `grow` could overflow it (rc_sum_fetch waits for every queued add itself)"""
            if view.bound() + grow > view.LIMIT:
                np.add(total, view.fetch_view(reset=True), out=total)
        adder.fold = fold if total is not None else None
        try:
            if n:
                for _ in self._sum_stream([(z0, n, fs)], batch, adder):
                    pass
            if total is None:
                return n
            np.add(total, fs.fetch_view(), out=total)
            return total
        finally:
            if into is None:
                fs.close()

    # (what the summed views, the counting and the traces do not take, as _check_levels_and_bits words it: who refuses, and why 16 bits)
    _SUMS = ('sum_frames', 'the cells of a summed view are uint32')
    _COUNTS = ('counting', 'the sums are exact in 64 bits for 16-bit values')
    _TRACES = ('frame traces', 'the sums are exact in 64 bits for 16-bit values')
    _CORR = ('correlation surfaces', 'the sums are exact in 64 bits for 16-bit values')
    _BINS = ('binned frame traces', 'the sums are exact in 64 bits for 16-bit values')

    def _check_levels_and_bits(self, who, why):
        """levels 1 to 3, and at level 1 fields of 16 bits at most: NotImplementedError otherwise"""
        level, d = int(self._header['reduction_level']), int(self._header['target_bit_depth'])
        if level not in (1, 2, 3):
            raise NotImplementedError('%s: reduction level %d' % (who, level))
        if level == 1 and d > 16:
            raise NotImplementedError('%s: files of more than 16 bits (target_bit_depth %d): %s' % (who, d, why))

    def iter_frame_sums(self, frames_per_view, z0=0, n=None, batch=64, shifts=None):
        """Views of `frames_per_view` consecutive frames each (the last one of what is left): yields (first index, count, uint32[ny, nx]) -
        a loop over sum_frames' engine with two device views that alternate: all windows' batches form one sequence on the two slots, so
        the next window's first batch is read and queued - into the other view - before this window's image is fetched.  One thread does
        it all.  The image is a VIEW of page-locked memory the device copied into, valid until the generator is advanced (copy it to keep
        it), like the batches of iter_frames_triplets.  A window whose sum could pass 2^32 - 1 raises ValueError.
        shifts: as for sum_frames, one (dy, dx) row per frame of z0 .. z0 + n - 1 - the aligned views of a drifting series."""
        if frames_per_view <= 0 or batch <= 0:
            raise ValueError('frames_per_view and batch must be positive')
        n = self._frame_range(z0, n, batch)
        self._check_levels_and_bits(*self._SUMS)
        yield from self._iter_sums(frames_per_view, z0, n, batch, _PlainAdder(z0, shifts, n))

    def _iter_sums(self, frames_per_view, z0, n, batch, adder):
        """iter_frame_sums and iter_frame_sums_counted behind their argument checks"""
        vx, vy = adder.view_shape(int(self._header['nx']), int(self._header['ny']))
        views = [_lib.FrameSum(vx, vy), _lib.FrameSum(vx, vy)]
        windows = [(a, min(frames_per_view, z0 + n - a), views[i & 1]) for i, a in enumerate(range(z0, z0 + n, frames_per_view))]
        stream = self._sum_stream(windows, batch, adder)
        try:
            for w in stream:
                a, k, view = windows[w]
                yield a, k, view.fetch_view(reset=True)
        finally:
            stream.close()
            for v in views:
                v.close()

    # ---- electron counting (rc_count_frames): one event per connected component, labelled and reduced on the device -------------------
    def _count_stream(self, z0, n, batch, area_threshold, method):
        """The engine of get_frames_counted and iter_frames_counted: the batches go down the ladder as events (_Events:
        rc_count_frames_submit / rc_expand_frames_wait on the two slots), so the next batch is read from the file and queued before this
        one is waited for.  Routes and fall-backs are the summed views' (sum_frames)."""
        yield from self._ladder(_Events(method, area_threshold, self._bufs.stream), _jobs(z0, n, batch))

    def get_frames_counted(self, z0, n, area_threshold=0, method='weighted_average'):
        """Electron counting of frames z0 .. z0+n-1 of a merged file (records of a part file) in ONE device call (rc_count_frames): what the
        reference's l1_to_l4_converter does frame by frame on the host (utils/converters.py:59-123) - every 8-connected puddle of set pixels
        becomes one event.  Returns (nev_prefix uint64[n+1], rows int32, cols int32, area uint32, weight uint64): frame i's events are
        [nev_prefix[i], nev_prefix[i+1]) of the four arrays, ordered as scipy.ndimage.label numbers their components; area = the
        component's pixels, weight = the sum of their values (levels 2 and 3: every value is 1); an event is kept iff area > area_threshold.
        method: 'weighted_average' (the intensity-weighted centroid, a component of weight 0 placed as by 'unweighted_average'),
        'unweighted_average' or 'max' (the brightest pixel, the first in raster order among equals).  Centroids are the exact rational
        rounded half to even - no floating point.  Unlike the reference: it accumulates in float32; it hands (col, row) to coo_matrix as
        (row, col), here rows are rows; it sends every method name to the weighted helper, here each does what its helper was written
        for.  Only the events cross the link (20 bytes each).  Routes and last_batch_path as for sum_frames; files of more than 16 bits are
        not taken (NotImplementedError)."""
        n = self._frame_range(z0, n)
        self._check_levels_and_bits(*self._COUNTS)
        stream = self._count_stream(z0, n, n, area_threshold, method)      # (one batch of n frames)
        try:
            return next(stream)[1:]
        finally:
            stream.close()

    def iter_frames_counted(self, z0=0, n=None, batch=64, area_threshold=0, method='weighted_average'):
        """get_frames_counted for a whole file, streamed: yields (first frame index, nev_prefix, rows, cols, area, weight) per batch of up to
        `batch` frames, two batches in flight (rc_count_frames_submit / rc_expand_frames_wait).  The arrays are copies of their own."""
        n = self._frame_range(z0, n, batch)
        self._check_levels_and_bits(*self._COUNTS)
        count_method(method)
        yield from self._count_stream(z0, n, batch, area_threshold, method)

    # ---- counted views (rc_sum_add_counted): the events of a range of frames summed on the device, on a grid up to 16 times finer ---------
    def sum_frames_counted(self, z0=0, n=None, batch=64, area_threshold=0, method='weighted_average', upsample=1, into=None, shifts=None):
        """The counted image of frames z0 .. z0+n-1 as uint64[upsample * ny, upsample * nx]: every event of get_frames_counted (same
        components, method and area_threshold) is ONE count, added on the device to the cell of a grid `upsample` (1..16) times finer
        than the sensor's whose centre lies nearest to the event's exact centroid (ties to the even cell index; pixel centres at
        integers, fine cell k at (k - (upsample - 1) / 2) / upsample).  upsample = 1 is np.add.at of get_frames_counted's (rows, cols).
        What a caller of the reference's l1_to_l4_converter does with its result on the host (utils/converters.py:59-123, then the
        viewer's np.add, utils/viewer.py:65-68) - no event crosses the link, 4 bytes per cell do at the end.  The view costs
        4 * upsample^2 * nx * ny bytes on the device and as much page-locked memory on the host (1 GiB for 4096 x 4096 at 4).
        into: a _lib.FrameSum(upsample * nx, upsample * ny) - the counts are added into it and the number of frames is returned.
        Engine, routes, fall-backs, last_batch_path and the fold before a cell could overflow: sum_frames.  Levels 2 and 3 (every value 1)
        go through the synchronous call.  Files of more than 16 bits are not taken (NotImplementedError).
        shifts: as for sum_frames, in FINE cells (1 / upsample pixel): the event is placed on the fine grid and then translated, so an
        integer shift is a drift correction at 1 / upsample-pixel resolution (rc_sum_add_counted_shifted)."""
        n = self._frame_range(z0, n, batch)
        self._check_levels_and_bits(*self._SUMS)
        self._check_levels_and_bits(*self._COUNTS)
        return self._sum_into(z0, n, batch, into, _CountedAdder(method, area_threshold, upsample, z0, shifts, n))

    def iter_frame_sums_counted(self, frames_per_view, z0=0, n=None, batch=64, area_threshold=0, method='weighted_average', upsample=1, shifts=None):
        """iter_frame_sums with sum_frames_counted's images: yields (first index, count, uint32[upsample * ny, upsample * nx]) per window of
        `frames_per_view` frames - a VIEW of page-locked memory, valid until the generator is advanced.  shifts: as for sum_frames_counted."""
        if frames_per_view <= 0 or batch <= 0:
            raise ValueError('frames_per_view and batch must be positive')
        n = self._frame_range(z0, n, batch)
        self._check_levels_and_bits(*self._SUMS)
        self._check_levels_and_bits(*self._COUNTS)
        yield from self._iter_sums(frames_per_view, z0, n, batch, _CountedAdder(method, area_threshold, upsample, z0, shifts, n))

    # ---- dense frame batches (rc_expand_frames_dense): a region of every frame as an array, written on the device --------------------------
    _DENSE_BYTES = 256 << 20      # the dense output of a batch the streaming calls size themselves (8 frames of 4096 x 4096 uint16)

    def _dense_check_file(self):
        """the cell type of this file's dense frames: its numpy dtype, which must be an unsigned integer of 1, 2 or 4 bytes"""
        h = self._header
        level, d = int(h['reduction_level']), int(h['target_bit_depth'])
        dt = np.dtype(self._numpy_dtype)
        if level not in (1, 2, 3):
            raise NotImplementedError('dense frames: reduction level %d' % level)
        if dt.kind != 'u' or dt.itemsize not in (1, 2, 4):
            raise NotImplementedError('dense frames: target dtype %s (the cells are unsigned integers of 1, 2 or 4 bytes)' % dt)
        if level == 1 and (d > 32 or d > 8 * dt.itemsize):
            raise NotImplementedError('dense frames: files of more than 32 bits, or of more bits than their dtype holds (target_bit_depth %d, %s)' % (d, dt))
        return dt

    def _dense_region(self, roi):
        """roi = None (the whole frame) or (slice_y, slice_x) -> (x0, y0, w, h, step_x, step_y) as rc_expand_frames_dense takes it; the
        slices follow numpy's rules, and must select something, walking forwards"""
        ny, nx = int(self._header['ny']), int(self._header['nx'])
        if roi is None:
            return 0, 0, nx, ny, 1, 1
        if not (isinstance(roi, tuple) and len(roi) == 2 and all(isinstance(s, slice) for s in roi)):
            raise ValueError('roi must be (slice_y, slice_x)')
        (y0, h, sy, fy, _), (x0, w, sx, fx, _) = plan_sub_volume(roi, (ny, nx))
        if fy or fx or h == 0 or w == 0:
            raise ValueError('roi: an empty selection or a negative step (get_sub_volume takes those)')
        return x0, y0, w, h, sx, sy

    def _dense_batch(self, region, dt):
        """the frames of the largest batch whose dense output stays within _DENSE_BYTES - and at least one"""
        return max(1, self._DENSE_BYTES // (region[2] * region[3] * dt.itemsize))

    def _read_frames_into(self, blob, frames):
        """the data of the frames `frames` lists (ascending) -> blob, back to back: a run of consecutive frames as _read_batch_into reads it,
        anything else gathered piece by piece, the way _read_batch_into does for part files"""
        k, a = len(frames), int(frames[0])
        if int(frames[-1]) - a + 1 == k:
            return self._read_batch_into(blob, a, k)
        self._piecewise(blob, frames, 'file shorter than its seek table says')[0](0, k)
        if not self._is_intermediate:         # (where reading a run leaves a merged file: behind the last frame read)
            self._fp.seek(self._frame_data_start_position + int(self._seek_table[int(frames[-1])].sum()), 0)

    def _dense_stream(self, groups, region, dt):
        """The engine of iter_frames_dense and get_sub_volume: groups = [frame indices, ascending] - one batch each - down the ladder as
        dense cells (_Dense: rc_expand_frames_dense_submit / rc_expand_frames_wait on the two slots), so the next batch is read from the
        file and queued before this one is waited for.  Yields (index of the group, array[k, h, w]): a VIEW of the slot's page-locked
        output, valid until the generator advances.  Routes and fall-backs are the summed views' (sum_frames)."""
        # (a job's first frame is chosen so that first + count is behind its last frame: where _two_slots leaves a merged file's counter)
        jobs = [_Job(int(g[-1]) + 1 - len(g), len(g), SimpleNamespace(index=i), g) for i, g in enumerate(groups)]
        return self._ladder(_Dense(region, dt, self._bufs.stream), jobs)

    def get_frames_dense(self, z0, n, roi=None, out=None):
        """Frames z0 .. z0+n-1 of a merged file (records of a part file) as an array[n, h, w] of the file's dtype in ONE device call
        (rc_expand_frames_dense): what np.stack of get_frame(z)['data'].toarray() gives - a memset and a scatter per frame on the host
        (utils/viewer.py:65-68) - written by the device, zeros included; nothing per set pixel crosses the link.
        roi: None (whole frames) or (slice_y, slice_x), numpy's rules, positive steps: only that region is written and copied.
        out: None (an array of its own), a C-contiguous numpy array of shape (n, h, w) and the file's dtype, or an object with data_ptr(),
        shape, element_size() and is_contiguous() - a torch tensor on the GPU -, which the device writes in place; `out` is returned.
        For WHOLE frames wanted in host memory the link carries 2 bytes per pixel here against 10 per set pixel on the COO route
        (get_frames_coo): below one set pixel in five that route moves less - this one saves the host's memset and scatter
        (DESIGN.md 7f has the rates measured side by side).
        Routes (last_batch_path) and fall-backs as for sum_frames.  A dtype that is not an unsigned integer of 1, 2 or 4 bytes, and files
        of more than 32 bits, are not taken (NotImplementedError)."""
        dt = self._dense_check_file()
        n = self._frame_range(z0, n)
        region = self._dense_region(roi)
        shape = (n, region[3], region[2])
        if out is None:
            out = np.empty(shape, dt)
        if isinstance(out, np.ndarray):
            if out.dtype != dt or out.shape != shape or not out.flags['C_CONTIGUOUS']:
                raise ValueError('get_frames_dense: out must be a C-contiguous %s array of shape %s' % (dt, shape))
            dst = _lib.ptr(out)
        else:
            if tuple(out.shape) != shape or out.element_size() != dt.itemsize or not out.is_contiguous():
                raise ValueError('get_frames_dense: out must be contiguous, of shape %s and %d bytes an element' % (shape, dt.itemsize))
            dst = int(out.data_ptr())
        kind, job = _Dense(region, dt, dst=dst), _Job(z0, n)
        self._now(kind, job)        # (the ladder in its synchronous form: nothing is queued, `out` is written in place)
        return out

    def iter_frames_dense(self, z0=0, n=None, batch=None, roi=None):
        """get_frames_dense for a whole file, streamed: yields (first frame index, array[k, h, w]) per batch of up to `batch` frames, two
        batches in flight (rc_expand_frames_dense_submit / rc_expand_frames_wait).  The array is a VIEW of page-locked memory, valid until
        the generator is advanced (copy it to keep it), like the batches of iter_frames_triplets.  batch=None: the largest batch whose dense
        output is at most 256 MiB, and at least one frame - 8 frames of 4096 x 4096 uint16."""
        dt = self._dense_check_file()
        region = self._dense_region(roi)
        batch = self._dense_batch(region, dt) if batch is None else batch
        n = self._frame_range(z0, n, batch)
        groups = [np.arange(a, min(a + batch, z0 + n)) for a in range(z0, z0 + n, batch)]
        for i, arr in self._dense_stream(groups, region, dt):
            yield int(groups[i][0]), arr

    def get_sub_volume(self, slice_z, slice_y, slice_x):
        """What numpy's stack[slice_z, slice_y, slice_x] returns - values, shape and dtype -, stack[z] being the toarray() of frame z's COO
        matrix as get_frame returns it (records of a part file: record z): the method the reference's source readers implement
        (em_reader.py:111-116) and its ReCoDeReader leaves a stub (recode_reader.py:185-186).  Slices and integers, None bounds, negative
        indices and negative steps follow numpy's rules (plan_sub_volume); as in the reference's readers a slice_z.stop beyond nz raises
        IndexError.  Only the selected frames are read - a z step other than 1 gathers their blobs piece by piece -, only the selected
        region of each is written by the device (rc_expand_frames_dense) and copied; batches are sized as in iter_frames_dense."""
        dt = self._dense_check_file()
        shape = (self._batch_frames(), int(self._header['ny']), int(self._header['nx']))
        if isinstance(slice_z, slice) and slice_z.stop is not None and slice_z.stop > shape[0]:
            raise IndexError('slice_z.stop (%d) is beyond the number of frames (%d)' % (slice_z.stop, shape[0]))
        (z0, cz, sz, fz, dz), (y0, cy, sy, fy, dy), (x0, cx, sx, fx, dx) = plan_sub_volume((slice_z, slice_y, slice_x), shape)
        vol = np.empty((cz, cy, cx), dt)
        if vol.size:
            region = (x0, y0, cx, cy, sx, sy)
            frames = z0 + sz * np.arange(cz)
            batch = self._dense_batch(region, dt)
            groups = [frames[a:a + batch] for a in range(0, cz, batch)]
            for i, arr in self._dense_stream(groups, region, dt):
                vol[i * batch:i * batch + arr.shape[0]] = arr
        vol = vol[::-1 if fz else 1, ::-1 if fy else 1, ::-1 if fx else 1]
        return vol[0 if dz else slice(None), 0 if dy else slice(None), 0 if dx else slice(None)]

    # ---- per-frame tables: frame traces (rc_trace_frames), correlation surfaces (rc_corr_frames), binned traces (rc_bins_frames) - a few
    # exact integers per frame, reduced on the device.  One engine; a kind is its limits, its handle and the dict it makes of a batch's cells
    def _frame_ids(self, first, k):
        """the indices of frames first .. first + k - 1, a part file's frame ids"""
        return self.part_frame_ids[first:first + k].astype(np.int64) if self._is_intermediate else np.arange(first, first + k, dtype=np.int64)

    def _table_handle(self, arg, cls, make, what):
        """(the handle to use, whether this call made it): a caller's `cls` as it is - its shape must be the file's -, else make(nx, ny)"""
        nx, ny = int(self._header['nx']), int(self._header['ny'])
        if isinstance(arg, cls):
            if (arg.nx, arg.ny) != (nx, ny):
                raise ValueError('%s: a %s of %d x %d for frames of %d x %d' % (what, cls.__name__, arg.nx, arg.ny, nx, ny))
            return arg, False
        return make(nx, ny), True

    def _table_stream(self, z0, n, batch, limits, arg, cls, make, as_dict, with_prefix=False):
        """The engine of the six methods below, a generator: the file's levels and bits are judged, then the handle (_table_handle), and the
        batches go down the ladder as _Tables (rc_<kind>_frames_submit / rc_expand_frames_wait on the two slots), so the next batch is read
        from the file and queued before this one is waited for; 8 bytes per cell of a frame's row cross the link.  Yields (first frame,
        dict).  Routes and fall-backs are the summed views' (sum_frames).  The stream is always closed, the handle if this call made it."""
        self._check_levels_and_bits(*limits)
        handle, own = self._table_handle(arg, cls, make, limits[0])
        stream = self._ladder(_Tables(handle, self._bufs.stream, as_dict, with_prefix), _jobs(z0, n, batch))
        try:
            yield from stream
        finally:
            stream.close()
            if own:
                handle.close()

    @staticmethod
    def _only_batch(stream):
        """the dict of a _table_stream of one batch"""
        try:
            return next(stream)[1]
        finally:
            stream.close()

    def _trace_dict(self, first, k, cells):
        """a batch's int64[k, 4 + planes] as the dict get_frame_traces returns (copies of their own)"""
        return {'count': cells[:, 0].copy(), 'sum': cells[:, 1].copy(), 'sum_row': cells[:, 2].copy(), 'sum_col': cells[:, 3].copy(),
                'weighted': cells[:, 4:].copy(), 'frame_ids': self._frame_ids(first, k)}

    def _trace_stream(self, z0, n, batch, weights):
        return self._table_stream(z0, n, batch, self._TRACES, weights, _lib.FrameTrace, lambda nx, ny: _lib.FrameTrace(nx, ny, weights), self._trace_dict)

    def get_frame_traces(self, z0, n, weights=None):
        """Per frame of z0 .. z0+n-1 of a merged file (records of a part file) a few exact integers, reduced ON THE DEVICE in one call
        (rc_trace_frames): what the reference prints as a dose rate per frame (utils/converters.py:108-111) and what a caller otherwise
        computes from every frame's COO matrix on the host.  Returns a dict of int64 arrays: 'count' [n] - the set pixels -, 'sum' [n] - the
        sum of their values (levels 2 and 3: every value is 1) -, 'sum_row' and 'sum_col' [n] - the sums of value * row and value * column
        (centre_of_mass turns them into coordinates) -, 'weighted' [n, k] - the sums of value * weights[m][row][col] -, and 'frame_ids' [n]
        - the frames' indices, a part file's frame ids.
        weights: None, an integer array or GPU tensor of shape (ny, nx) or (k, ny, nx), k <= 16, whose values fit int32 - masks of a virtual
        detector, an ROI -, or a _lib.FrameTrace the caller made, so that the part files of a run share one copy of the weights.  A batch
        in which a column could pass 2^63 - 1 raises ValueError.  Routes (last_batch_path) and fall-backs as for sum_frames; files of more
        than 16 bits are not taken (NotImplementedError)."""
        n = self._frame_range(z0, n)
        return self._only_batch(self._trace_stream(z0, n, n, weights))

    def iter_frame_traces(self, z0=0, n=None, batch=64, weights=None):
        """get_frame_traces for a whole file, streamed: yields (first frame index, dict) per batch of up to `batch` frames, two batches in
        flight (rc_trace_frames_submit / rc_expand_frames_wait).  The arrays are copies of their own."""
        n = self._frame_range(z0, n, batch)
        yield from self._trace_stream(z0, n, batch, weights)

    def _corr_dict(self, first, k, cells, prefix):
        """a batch's int64[k, S, S] and set-pixel prefix as the dict get_frame_correlations returns (copies of their own)"""
        return {'corr': cells.copy(), 'count': np.diff(np.asarray(prefix[:k + 1]).astype(np.int64)), 'frame_ids': self._frame_ids(first, k)}

    def _corr_stream(self, z0, n, batch, reference, radius):
        def make(nx, ny):
            if reference is None:
                raise ValueError('correlation surfaces: a reference is needed - an integer (ny, nx) array or GPU tensor, a FrameSum, or a FrameCorrelation')
            return _lib.FrameCorrelation(nx, ny, reference, radius)
        return self._table_stream(z0, n, batch, self._CORR, reference, _lib.FrameCorrelation, make, self._corr_dict, with_prefix=True)

    def get_frame_correlations(self, z0, n, reference=None, radius=8):
        """Per frame of z0 .. z0+n-1 of a merged file (records of a part file) its correlation surface with `reference`, summed ON THE
        DEVICE in one call (rc_corr_frames): 'corr' int64[n, S, S], S = 2 * radius + 1, corr[f, dy + R, dx + R] = the sum over the frame's set
        pixels (row, col) of value * reference[row + dy, col + dx] (0 outside the image; levels 2 and 3: every value is 1) - the overlap
        with the reference of the frame translated by (dy, dx), so estimate_shifts' argmax is what sum_frames(shifts=...) takes.  Also
        'count' int64[n] - the frames' set pixels - and 'frame_ids' int64[n].
        reference: an integer array or GPU tensor of shape (ny, nx) whose values fit int32, a _lib.FrameSum of that shape (a summed view:
        its cells stay on the device), or a _lib.FrameCorrelation the caller made - `radius` (0..16) is then the handle's -, so that
        the part files of a run share one copy.  A batch in which a cell could pass 2^63 - 1 raises ValueError.  Routes
        (last_batch_path) and fall-backs as for sum_frames; files of more than 16 bits are not taken (NotImplementedError)."""
        n = self._frame_range(z0, n)
        return self._only_batch(self._corr_stream(z0, n, n, reference, radius))

    def iter_frame_correlations(self, z0=0, n=None, batch=64, reference=None, radius=8):
        """get_frame_correlations for a whole file, streamed: yields (first frame index, dict) per batch of up to `batch` frames, two
        batches in flight (rc_corr_frames_submit / rc_expand_frames_wait).  The arrays are copies of their own."""
        n = self._frame_range(z0, n, batch)
        yield from self._corr_stream(z0, n, batch, reference, radius)

    def _bins_dict(self, first, k, cells):
        """a batch's int64[k, 2, B] as the dict get_frame_bins returns (copies of their own)"""
        return {'count': cells[:, 0].copy(), 'sum': cells[:, 1].copy(), 'frame_ids': self._frame_ids(first, k)}

    def _bins_stream(self, z0, n, batch, labels, n_bins):
        def make(nx, ny):
            if labels is None:
                raise ValueError('binned frame traces: labels are needed - an integer (ny, nx) array or GPU tensor, or a FrameBins')
            return _lib.FrameBins(nx, ny, labels, n_bins)
        return self._table_stream(z0, n, batch, self._BINS, labels, _lib.FrameBins, make, self._bins_dict)

    def get_frame_bins(self, z0, n, labels=None, n_bins=None):
        """Per frame of z0 .. z0+n-1 of a merged file (records of a part file) and per bin of the label map the number of set pixels and the
        sum of their values, reduced ON THE DEVICE in one call (rc_bins_frames): 'count' int64[n, B], 'sum' int64[n, B] (levels 2 and 3:
        every value is 1, so 'sum' equals 'count') and 'frame_ids' int64[n].  labels: an integer array or GPU tensor of shape (ny, nx), each
        cell a bin 0 .. B - 1 or 0xFFFF ("in no bin") - radial_labels makes a radial profile's -, with n_bins = B (1 .. 4096; None: the
        largest label + 1); or a _lib.FrameBins the caller made - n_bins is then the handle's -, so that the part files of a run share one
        copy.  bin_areas(labels, B) is the denominator of a mean profile.  Routes (last_batch_path) and fall-backs as for sum_frames; files of
        more than 16 bits are not taken (NotImplementedError)."""
        n = self._frame_range(z0, n)
        return self._only_batch(self._bins_stream(z0, n, n, labels, n_bins))

    def iter_frame_bins(self, z0=0, n=None, batch=64, labels=None, n_bins=None):
        """get_frame_bins for a whole file, streamed: yields (first frame index, dict) per batch of up to `batch` frames, two batches in
        flight (rc_bins_frames_submit / rc_expand_frames_wait).  The arrays are copies of their own."""
        n = self._frame_range(z0, n, batch)
        yield from self._bins_stream(z0, n, batch, labels, n_bins)

    def get_frames_coo(self, z0, n, out=None):
        """get_frames_triplets in the COO layout: (nnz_prefix, (rows int32, columns int32, values uint16 - uint32 for a level-1 file of
        more than 16 bits))"""
        return self.get_frames_triplets(z0, n, out=out, coo=True)

    def iter_frames_coo(self, z0=0, n=None, batch=64):
        """iter_frames_triplets in the COO layout: yields (first frame, nnz_prefix, (rows int32, columns int32, values uint16 - uint32
        for a level-1 file of more than 16 bits))"""
        return self.iter_frames_triplets(z0, n, batch, coo=True)

    def get_frames(self, z0, n):
        """{frame index: {'metadata', 'data': COO}} for n consecutive frames, decoded in one device call."""
        level, d = int(self._header['reduction_level']), int(self._header['target_bit_depth'])
        coo_ok = level == 3 or (level == 1 and d <= 32)          # (the COO arrays' values are uint32 at most)
        prefix, got = self.get_frames_triplets(z0, n, coo=coo_ok)
        out = {}
        for i in range(n):
            lo, hi = int(prefix[i]), int(prefix[i + 1])
            if coo_ok:      # the batch came as the matrices' own arrays: a frame's matrix takes copies of its slices
                coo = self._coo_from_arrays(got[2][lo:hi].astype(self._numpy_dtype), got[0][lo:hi].copy(), got[1][lo:hi].copy())
            else:
                coo = self._make_coo_frame(hi - lo, got[lo:hi])
            key = int(self.part_frame_ids[z0 + i]) if self._is_intermediate else z0 + i      # (what get_next_frame keys a part file's frames by)
            out[key] = {'metadata': self._frame_metadata[z0 + i], 'data': coo}
        return out
