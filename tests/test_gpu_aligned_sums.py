"""-m gpu: aligned views - per-frame shifts applied while the device sums frames.  The gather kernel (k_sum_shift) and the translated
placement of k_cnt_place through the C ABI on stored streams built with numpy (tests/test_gpu_frame_sums.py's builders and frame kinds,
tests/centroid_model.py's for the counted form), zero shifts against the unshifted call, shifted and unshifted adds into one handle on
both slots, the submit / wait form with a rejected batch in the middle, ReCoDeReader's `shifts=` on every rung of the ladder, and
ReCoDeViewer with a shift table by frame id.  The expectation is the exact model (tests/aligned_sum_model.py); every comparison is `==`."""
import os
import shutil

import numpy as np
import pytest

import aligned_sum_model as am
import centroid_model as cm
import counted_view_model as cv
import test_gpu_counted_views as cviews
import test_gpu_frame_sums as fsum
from conftest import GOLDEN, load_npz

pytestmark = pytest.mark.gpu
FILES = os.path.join(GOLDEN, "files")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT32_MIN, INT32_MAX = am.INT32_MIN, am.INT32_MAX


@pytest.fixture(scope="module")
def hip():
    from pyrecode_amd import _lib
    if _lib.device_count() == 0:
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    return _lib


def _pair(t, nx):
    """a (dy, dx) whose linear offset dy * nx + dx is t, dx the smallest in magnitude"""
    dy = int(round(t / nx))
    return dy, t - dy * nx


def _shift_list(ny, nx):
    """the shifts the frames of a kernel test draw from in turn"""
    out = [(0, 0), (0, 1), (0, -1), (1, 0), (-1, 0), (0, 63), (0, 64), (0, 65)]
    out += [_pair(sign * (edge + k), nx) for edge in (64, 16384) for sign in (1, -1) for k in (-1, 0, 1)]       # the funnel's word and block boundaries
    out += [(ny - 1, nx - 1), (-(ny - 1), -(nx - 1))]                                                           # one corner survives
    out += [(ny, 0), (0, nx), (-ny - 5, 3), (INT32_MAX, INT32_MIN)]                                             # nothing survives
    return out


def test_the_shift_list_covers_what_it_is_meant_to():
    got = _shift_list(192, 256)
    for want in ((64, 0), (64, 1), (64, -1), (-64, 0), (0, 64), (0, -64), (191, 255), (-191, -255), (192, 0), (0, 256)):
        assert want in got
    assert all(dy * 130 + dx == t for t in (63, 64, 65, -16385, 16383) for dy, dx in [_pair(t, 130)])
    assert len(got) == 26


class _Sum(fsum._Sum):
    """fsum._Sum with the shifted calls, as a C program would make them"""

    def add_shifted(self, d, level, blob, sizes, n, shifts, prefix=None):
        shifts = np.ascontiguousarray(shifts, np.int32)
        return self.L.rc_sum_add_frames_shifted(self.h, d, level, 0, 0, self.hip.ptr(blob), self.hip.ptr(sizes), n, self.hip.ptr(shifts), self.hip.ptr(prefix))

    def submit_shifted(self, slot, d, level, blob, sizes, n, shifts):
        shifts = np.ascontiguousarray(shifts, np.int32)
        st = self.L.rc_sum_add_frames_shifted_submit(self.h, slot, d, level, 0, 0, self.hip.ptr(blob), self.hip.ptr(sizes), n, self.hip.ptr(shifts))
        shifts[:] = 0x5A5A5A5A           # (the library has copied them: the submitter may reuse the array)
        return st


# ---- 1. the kernel, through the C ABI ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level,d", fsum.KINDS)
@pytest.mark.parametrize("ny,nx", fsum.SHAPES)
def test_shifted_sum_kernel_on_stored_streams(hip, ny, nx, level, d):
    """rc_sum_add_frames_shifted, op_mode 0.  The batches of test_sum_kernel_on_stored_streams - n = 1 (each frame kind alone), n = 3 (one frame
    group) and n = 11 (three groups: 4 + 4 + 3) - and one more of 11 that starts with the all-set frame, all into one view, every frame with
    the next shift of _shift_list (the start of the walk depends on the kind, so each shift meets several frame kinds over the
    parameters): the view, every batch's set-pixel prefix - the unshifted counts - and the bound, which grows as unshifted."""
    rng = np.random.default_rng(1000 * ny + 10 * d + level)
    shifts_all = _shift_list(ny, nx)
    at = 7 * fsum.KINDS.index((level, d))
    view = _Sum(hip, nx, ny)
    want = np.zeros((ny, nx), np.uint64)
    batches = [(1, k) for k in range(5)] + [(3, 0), (3, 3), (11, 0), (11, 2)]
    grown = 0
    for n, first in batches:
        vals = fsum._frames(rng, n, ny, nx, d, level, first)
        shifts = [shifts_all[(at + k) % len(shifts_all)] for k in range(n)]
        at += n
        blob, sizes, _ = fsum._stored_batch(vals, d, level, rng)
        prefix = np.zeros(n + 1, np.uint64)
        assert view.add_shifted(d, level, blob, sizes, n, shifts, prefix) == hip.RC_OK, hip.last_error()
        assert np.array_equal(prefix[1:], np.cumsum((vals != 0).reshape(n, -1).sum(1)).astype(np.uint64))
        want += am.shifted_sum(vals, shifts)
        grown += n * ((1 << d) - 1 if level == 1 else 1)
        assert view.bound() == grown
    got = view.fetch()
    view.close()
    assert sum(n for n, _ in batches) >= len(shifts_all) and int(want.max()) <= grown and want.any()
    assert np.array_equal(got.astype(np.uint64), want), "%d cells differ, first at %s" % (int((got != want).sum()), np.argwhere(got != want)[:4].tolist())


@pytest.mark.parametrize("shift", [(0, 1), (0, -1), (1, 0), (-1, 0), (0, 63), (0, 64), (0, 65), (64, 0), (64, 1), (64, -1), (-64, 0), (-63, -255), (191, 255)])
def test_an_all_set_frame_shows_the_column_mask_as_an_exact_rectangle(hip, shift):
    """(192, 256), every pixel set, 16 bits, pixel p holding p % 65535 + 1 - neighbours differ -, one frame, one shift: the view is the source
    rectangle moved, zeros around it, and every value is its source pixel's (a rank off by one would show)"""
    ny, nx, d = 192, 256, 16
    vals = (np.arange(ny * nx, dtype=np.uint32) % 65535 + 1).reshape(1, ny, nx)
    blob, sizes, _ = fsum._stored_batch(vals, d, 1, np.random.default_rng(0))
    view = _Sum(hip, nx, ny)
    assert view.add_shifted(d, 1, blob, sizes, 1, [shift]) == hip.RC_OK, hip.last_error()
    got = view.fetch()
    view.close()
    want = am.shifted_sum(vals, [shift])
    dy, dx = shift
    assert int((want != 0).sum()) == (ny - abs(dy)) * (nx - abs(dx))
    assert np.array_equal(got.astype(np.uint64), want)


def test_zero_shifts_are_the_unshifted_call(hip):
    ny, nx, d, n = 127, 130, 12, 7
    rng = np.random.default_rng(3)
    for level in (1, 3):
        vals = fsum._frames(rng, n, ny, nx, d, level)
        blob, sizes, _ = fsum._stored_batch(vals, d, level, rng)
        a, b = _Sum(hip, nx, ny), _Sum(hip, nx, ny)
        pa, pb = np.zeros(n + 1, np.uint64), np.zeros(n + 1, np.uint64)
        assert a.add(d, level, blob, sizes, n, pa) == hip.RC_OK and b.add_shifted(d, level, blob, sizes, n, np.zeros((n, 2), np.int32), pb) == hip.RC_OK
        va, vb = a.fetch(), b.fetch()
        assert a.bound() == b.bound() and np.array_equal(pa, pb)
        a.close()
        b.close()
        assert va.any() and np.array_equal(va, vb)


def test_shifted_and_unshifted_adds_share_a_handle_on_both_slots(hip):
    ny, nx, d, n = 127, 130, 12, 5
    rng = np.random.default_rng(4)
    view = _Sum(hip, nx, ny)
    L = view.L
    want = np.zeros((ny, nx), np.uint64)
    queued = []
    for i, shifted in enumerate((True, False, False, True)):          # slots 0, 1, 0, 1: each slot takes one of either kind
        vals = fsum._frames(rng, n, ny, nx, d, 1, first=i)
        blob, sizes, _ = fsum._stored_batch(vals, d, 1, rng)
        shifts = [(i + 1, -2 * k) for k in range(n)]
        if i >= 2:
            assert L.rc_expand_frames_wait(i & 1, hip.ptr(np.zeros(n + 1, np.uint64))) == hip.RC_OK
        if shifted:
            assert view.submit_shifted(i & 1, d, 1, blob, sizes, n, shifts) == hip.RC_OK, hip.last_error()
            want += am.shifted_sum(vals, shifts)
        else:
            assert view.submit(i & 1, d, 1, blob, sizes, n) == hip.RC_OK, hip.last_error()
            want += vals.sum(0, dtype=np.uint64)
        queued.append((blob, sizes))                                  # (the bytes stay valid until the wait)
    got = view.fetch()
    for slot in (0, 1):
        assert L.rc_expand_frames_wait(slot, hip.ptr(np.zeros(n + 1, np.uint64))) == hip.RC_OK
    vals = fsum._frames(rng, 2, ny, nx, d, 1)
    blob, sizes, _ = fsum._stored_batch(vals, d, 1, rng)
    assert view.add(d, 1, blob, sizes, 2) == hip.RC_OK and view.add_shifted(d, 1, blob, sizes, 2, [(3, 3), (-3, -3)]) == hip.RC_OK
    assert np.array_equal(got.astype(np.uint64), want)
    assert np.array_equal(view.fetch().astype(np.uint64), want + vals.sum(0, dtype=np.uint64) + am.shifted_sum(vals, [(3, 3), (-3, -3)]))
    assert view.bound() == (4 * n + 4) * 4095
    view.close()


def test_submit_wait_with_a_rejected_batch_in_the_middle(hip):
    """Six shifted batches alternating between the slots.  Batch 3 declares one frame's value stream one byte short of what its set pixels
    need: rc_expand_frames_wait answers RC_ERR_CORRUPT, the batch adds nothing, the batches around it land; the counts are valid either way."""
    ny, nx, d, n = 127, 130, 12, 5
    rng = np.random.default_rng(9)
    view = _Sum(hip, nx, ny)
    L = view.L
    want = np.zeros((ny, nx), np.uint64)
    batches = []
    for i in range(6):
        vals = fsum._frames(rng, n, ny, nx, d, 1, first=i)
        shifts = [(k - 2, 3 * i - 7) for k in range(n)]
        blob, sizes, where = fsum._stored_batch(vals, d, 1, rng)
        if i == 3:
            z = next(z for z in range(n) if where[z][1] > 8)
            at, size = where[z]
            blob = np.ascontiguousarray(np.concatenate([blob[:at + size - 1], blob[at + size:]]))
            sizes[z, 1] = sizes[z, 2] = size - 1
        else:
            want += am.shifted_sum(vals, shifts)
        batches.append((vals, blob, sizes, shifts))
    verdicts = []

    def wait(i):
        prefix = np.zeros(n + 1, np.uint64)
        verdicts.append(L.rc_expand_frames_wait(i & 1, hip.ptr(prefix)))
        assert np.array_equal(prefix[1:], np.cumsum((batches[i][0] != 0).reshape(n, -1).sum(1)).astype(np.uint64))
    for i in range(6):
        if i >= 2:
            wait(i - 2)
        assert view.submit_shifted(i & 1, d, 1, batches[i][1], batches[i][2], n, batches[i][3]) == hip.RC_OK, hip.last_error()
    assert view.submit_shifted(0, d, 1, batches[0][1], batches[0][2], n, batches[0][3]) == hip.RC_ERR_BAD_ARG and "submitted batch" in hip.last_error()
    got = view.fetch()
    wait(4)
    wait(5)
    assert verdicts == [hip.RC_OK] * 3 + [hip.RC_ERR_CORRUPT] + [hip.RC_OK] * 2
    assert np.array_equal(got.astype(np.uint64), want)
    assert view.bound() == 6 * n * 4095
    view.close()


def test_refusals_are_the_unshifted_calls(hip):
    """with a real handle: another geometry, 20-bit values, a slot above 1 and NULL shifts - no cell and no bound changes"""
    ny, nx, d = 127, 130, 12
    rng = np.random.default_rng(5)
    view = _Sum(hip, nx, ny)
    L, p = view.L, hip.ptr
    vals = fsum._frames(rng, 3, ny, nx, d, 1)
    blob, sizes, _ = fsum._stored_batch(vals, d, 1, rng)
    other, osz, _ = fsum._stored_batch(fsum._frames(rng, 2, 3, 21, d, 1), d, 1, rng)
    z = np.zeros((3, 2), np.int32)
    assert view.add_shifted(d, 1, other, osz, 2, z[:2]) == hip.RC_ERR_BAD_ARG and "geometry" in hip.last_error()
    assert view.add_shifted(20, 1, blob, sizes, 3, z) == hip.RC_ERR_UNSUPPORTED and view.submit_shifted(0, 20, 1, blob, sizes, 3, z) == hip.RC_ERR_UNSUPPORTED
    assert view.submit_shifted(2, d, 1, blob, sizes, 3, z) == hip.RC_ERR_BAD_ARG
    assert L.rc_sum_add_frames_shifted(view.h, d, 1, 0, 0, p(blob), p(sizes), 3, None, None) == hip.RC_ERR_BAD_ARG
    assert L.rc_sum_add_frames_shifted_submit(view.h, 0, d, 1, 0, 0, p(blob), p(sizes), 3, None) == hip.RC_ERR_BAD_ARG
    assert L.rc_expand_frames_wait(0, p(np.zeros(4, np.uint64))) == hip.RC_ERR_BAD_ARG          # (nothing was queued)
    assert view.bound() == 0 and not view.fetch().any()
    fs = hip.FrameSum(2 * nx, 2 * ny)
    frames = [cm.bernoulli_frame(ny, nx, d, 0.03, z) for z in range(3)]
    data, csz = cm.stored_batch(frames, 1, d)
    for cnx, cny, s in ((nx, ny, 1), (nx, ny, 3), (ny, nx, 2)):          # a handle of the wrong shape
        assert L.rc_sum_add_counted_shifted(fs.handle, cnx, cny, s, d, 1, 0, 0, p(data), p(csz), 3, 0, 0, p(z), None) == hip.RC_ERR_BAD_ARG and "shape" in hip.last_error()
        assert L.rc_sum_add_counted_shifted_submit(fs.handle, 0, cnx, cny, s, d, 1, 0, 0, p(data), p(csz), 3, 0, 0, p(z)) == hip.RC_ERR_BAD_ARG
    assert fs.add_counted_shifted_status((nx, ny, 17, 1, 0, 0), data, csz, 3, z, 0, 0, 2) == hip.RC_ERR_UNSUPPORTED
    assert fs.bound() == 0 and not fs.fetch().any()
    fs.close()
    view.close()


# ---- 2. the counted form -----------------------------------------------------------------------------------------------------------------
def _fine_shifts(s, ny, nx):
    """shifts in fine cells: +-1, +-upsample, a mixed one, out of the view in each direction, the int32 extremes"""
    return [(0, 0), (1, -1), (-1, 1), (s, -s), (-s, s), (2 * s + 1, -3), (s * ny, 0), (-s * ny, 0), (0, s * nx), (0, -s * nx), (INT32_MIN, INT32_MAX),
            (INT32_MAX, INT32_MIN)]


@pytest.mark.parametrize("s", [1, 2, 3, 16])
@pytest.mark.parametrize("shape", [(3, 21), (127, 130)])
def test_counted_shifted_on_stored_streams(hip, shape, s):
    """rc_sum_add_counted_shifted on centroid_model's frames - 4 % Bernoulli with stored zeros, one all-set frame -, level 1 at 12 bits with
    every method and level 3 with the weighted one: the view against the translated model, the event prefix unchanged by the shifts, the
    bound's growth the unshifted rule"""
    ny, nx = shape
    shifts = _fine_shifts(s, ny, nx)
    n = len(shifts)
    frames = [cm.bernoulli_frame(ny, nx, 12, 0.04, 300 + k, zero_fraction=0.1) for k in range(n)]
    frames[5] = (np.ones(shape, bool), np.full(shape, 4095, np.uint16))
    fs = hip.FrameSum(s * nx, s * ny)
    try:
        for level, methods in ((1, (0, 1, 2)), (3, (0,))):
            g = (nx, ny, 12, level, 0, 0)
            data, sizes = cm.stored_batch(frames, level, 12)
            for method in methods:
                comps = cv.components(cviews._model_frames(frames, level), cm.METHODS[method], 0)
                want = am.shifted_view_of(comps, shape, s, shifts)
                prefix = fs.add_counted_shifted(g, data, sizes, n, shifts, method, 0, s)
                assert np.array_equal(prefix, np.concatenate([[0], np.cumsum([len(c) for c in comps])]).astype(np.uint64))
                assert fs.bound() == hip.FrameSum.grows_by_counted(g, sizes, n)
                got = fs.fetch(reset=True)
                assert 0 < int(want.sum()) < int(prefix[n]) and np.array_equal(got, want), (level, method, int((got != want).sum()))
        zero = fs.add_counted_shifted((nx, ny, 12, 1, 0, 0), *cm.stored_batch(frames, 1, 12), n, np.zeros((n, 2), np.int64), 0, 0, s)
        same = fs.fetch(reset=True)
        assert np.array_equal(zero, fs.add_counted((nx, ny, 12, 1, 0, 0), *cm.stored_batch(frames, 1, 12), n, 0, 0, s))
        assert np.array_equal(same, fs.fetch(reset=True))                 # all-zero shifts: the unshifted call, cell for cell
    finally:
        fs.close()


def test_two_events_translated_onto_one_cell_both_count(hip):
    """a ring around a dot: two components with one centroid, at (3, 4) of a 7 x 9 frame.  Translated by (-3 s, -4 s) fine cells both land in
    the view's first cell; one fine cell further both are gone.  Submitted on both slots into one handle."""
    shape, s = (7, 9), 4
    b = np.zeros(shape, bool)
    b[1:6, 2:7] = True
    b[2:5, 3:6] = False
    b[3, 4] = True
    frames = [(b, b.astype(np.uint16))] * 3
    data, sizes = cm.stored_batch(frames, 3, 8)
    g = (9, 7, 8, 3, 0, 0)
    at = cv.place(3, 1, s), cv.place(4, 1, s)
    shifts = [(-at[0], -at[1]), (-at[0] - 1, -at[1]), (0, 0)]
    want = am.shifted_counted_view(frames, shifts, s=s)
    assert int(want[0, 0]) == 2 and int(want[at]) == 2 and int(want.sum()) == 4
    fs = hip.FrameSum(s * 9, s * 7)
    try:
        assert fs.add_counted_shifted(g, data, sizes, 3, shifts, 0, 0, s).tolist() == [0, 2, 4, 6]
        assert np.array_equal(fs.fetch(reset=True), want)
        L = hip.lib()
        g1 = (9, 7, 8, 1, 0, 0)
        data1, sizes1 = cm.stored_batch(frames, 1, 8)                     # (level 1 queues; levels 2 and 3 count first, synchronously)
        for slot in (0, 1):
            hip.check(fs.submit_counted_shifted_status(slot, g1, data1, sizes1, 3, shifts, 0, 0, s), "submit")
        for slot in (0, 1):
            prefix = np.zeros(4, np.uint64)
            assert L.rc_expand_frames_wait(slot, hip.ptr(prefix)) == hip.RC_OK and prefix.tolist() == [0, 2, 4, 6]
        assert np.array_equal(fs.fetch(), 2 * want)
    finally:
        fs.close()


# ---- 3. the reader: every rung of the ladder applies the shifts -----------------------------------------------------------------------------
def _drift(n, seed, lim=6):
    rng = np.random.default_rng(seed)
    out = np.clip(np.cumsum(rng.integers(-2, 3, (n, 2)), 0), -lim, lim).astype(np.int64)
    out[n // 2] = (200, -1)                  # one frame out of the view altogether
    return out


def _paths(rd):
    """the routes the reader's batches take from here on (the frame-at-a-time reader notes its own reads too, before a route is named)"""
    seen = set()
    keep = rd._note_batch_end
    rd._note_batch_end = lambda z: (seen.add(rd.last_batch_path) if rd.last_batch_path is not None else None, keep(z))[1]
    return seen


def _check_reader(rd, vals, path):
    """sum_frames(shifts=) and iter_frame_sums(shifts=) - windows of 5 in batches of 3: the windows straddle batch boundaries - against the model
    from the frames' values, on the route `path` and no other"""
    n = vals.shape[0]
    shifts = _drift(n, n)
    seen = _paths(rd)
    got = rd.sum_frames(batch=3, shifts=shifts)
    assert seen == {path} and got.dtype == np.uint64 and np.array_equal(got, am.shifted_sum(vals, shifts))
    assert not np.array_equal(got, vals.sum(0, dtype=np.uint64))          # (a rung that ignored the shifts would give this)
    assert np.array_equal(rd.sum_frames(2, n - 3, batch=2, shifts=shifts[2:n - 1].tolist()), am.shifted_sum(vals[2:n - 1], shifts[2:n - 1]))
    windows = [(a, k, img.copy()) for a, k, img in rd.iter_frame_sums(5, batch=3, shifts=shifts.astype(np.int16))]
    assert [(a, k) for a, k, _ in windows] == [(a, min(5, n - a)) for a in range(0, n, 5)] and seen == {path}
    for a, k, img in windows:
        assert img.dtype == np.uint32 and np.array_equal(img, am.shifted_sum(vals[a:a + k], shifts[a:a + k]))
    assert np.array_equal(rd.sum_frames(batch=3), vals.sum(0, dtype=np.uint64))                  # None: today's path, untouched


@pytest.fixture(scope="module")
def stack():
    """20 frames of 127 x 130, 12 bits, 3 % set; frame 7 is empty (test_gpu_frame_sums.py's)"""
    rng = np.random.default_rng(21)
    ny, nx, nz = 127, 130, 20
    dark = rng.integers(80, 121, (ny, nx)).astype(np.uint16)
    frames = np.where(rng.random((nz, ny, nx)) < 0.03, dark + rng.integers(1, 3900, (nz, ny, nx)), dark // 2).astype(np.uint16)
    frames[7] = 0
    return dark, frames


def test_reader_on_the_device_rung(hip, stack, tmp_path):
    dark, frames = stack
    rd = fsum._open(fsum._write(tmp_path, dark, frames, 1, 2))
    try:
        _check_reader(rd, np.where(frames > dark, frames.astype(np.int64) - dark, 0).astype(np.uint32), "device")
    finally:
        rd.close()


def test_reader_on_the_host_decode_rung(hip):
    g = load_npz("g3_l1z12.npz")
    rd = fsum._open(os.path.join(FILES, "g3_l1z12.rc1"))
    try:
        _check_reader(rd, g["decoded"].astype(np.uint32), "host-decode + device-expand")
    finally:
        rd.close()


def test_reader_on_the_per_frame_rung(hip, stack, tmp_path):
    dark, frames = stack
    rd = fsum._open(fsum._write(tmp_path, dark, frames, 2, 0, l2_statistics=2))
    try:
        _check_reader(rd, (frames > dark).astype(np.uint32), "per-frame")
    finally:
        rd.close()


def test_reader_counted_with_shifts_on_the_device_rung(hip, stack, tmp_path):
    dark, frames = stack
    rd = fsum._open(fsum._write(tmp_path, dark, frames, 1, 2))
    try:
        n, shape = frames.shape[0], frames.shape[1:]
        model = cviews._frames_of(rd, 0, n)
        comps = cv.components(model, "weighted_average", 0)
        shifts = _drift(n, 77)
        seen = _paths(rd)
        windows = [(a, k, img.copy()) for a, k, img in rd.iter_frame_sums_counted(6, batch=4, upsample=2, shifts=shifts)]
        assert [(a, k) for a, k, _ in windows] == [(0, 6), (6, 6), (12, 6), (18, 2)] and seen == {"device"}
        for a, k, img in windows:
            want = am.shifted_view_of(comps[a:a + k], shape, 2, shifts[a:a + k])
            assert img.dtype == np.uint32 and want.any() and np.array_equal(img, want)
        got = rd.sum_frames_counted(3, 9, batch=4, upsample=2, method="max", area_threshold=1, shifts=shifts[3:12])
        assert np.array_equal(got, am.shifted_counted_view(model[3:12], shifts[3:12], "max", 1, 2))
        assert np.array_equal(rd.sum_frames_counted(upsample=2), cv.view_of(comps, shape, 2))
    finally:
        rd.close()


# ---- 4. the viewer ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("counting", [None, dict(upsample=2)])
def test_viewer_with_a_shift_table_by_frame_id(hip, tmp_path, capsys, counting):
    """G7's two parts (ids with gaps), fractionation 5: every frame is translated by the row of its ID; an id beyond the table is a
    ValueError at the window that needs it, and the window stays the next one"""
    from pyrecode_amd.utils.viewer import ReCoDeViewer
    g = load_npz("g7_stream.npz")
    thr = fsum._thr(g)
    for node in range(2):
        shutil.copy(os.path.join(FILES, "g7_stream.rc1_part%03d" % node), str(tmp_path))
    nz, ny, nx = g["frames"].shape
    vals = np.where(g["frames"] > thr, g["frames"].astype(np.int64) - thr, 0).astype(np.uint32)
    table = _drift(nz, 5, lim=4)
    table[3] = (-2, 3)
    s = 2 if counting else 1
    v = ReCoDeViewer(str(tmp_path), "g7_stream.rc1", 2, 5, counting=counting, shifts=table)
    short = ReCoDeViewer(str(tmp_path), "g7_stream.rc1", 2, 5, counting=counting, shifts=table[:12])
    try:
        assert v.get_shape() == (s * ny, s * nx)
        for start, count in ((0, 5), (5, 5), (10, 5), (15, 1)):
            view = v.get_next_view()
            assert view["start"] == start and view["n_Frames"] == count
            ids = np.arange(start, start + count)
            if counting:
                want = am.shifted_counted_view([(vals[i] != 0, vals[i]) for i in ids], table[ids], s=2)
            else:
                want = am.shifted_sum(vals[ids], table[ids])
            assert want.any() and np.array_equal(view["view"], want.astype(np.float64))
        assert v.get_next_view() is None
        assert short.get_next_view()["start"] == 0 and short.get_next_view()["start"] == 5
        for _ in range(2):
            with pytest.raises(ValueError, match="frame id"):
                short.get_next_view()
    finally:
        v.close()
        short.close()


# ---- 5. the kernel's footprint -----------------------------------------------------------------------------------------------------------
def test_shift_kernel_footprint():
    """k_sum_shift's descriptor in the built library, read the way test_gpu_frame_sums.py::test_sum_kernel_footprint reads its sibling's (no GPU
    needed, but the file's other tests do): exactly one symbol, no scratch, and between 1 and 81 920 B of static LDS - two workgroups share a
    CU's 160 KiB."""
    import re
    import struct
    import subprocess
    import tempfile
    lib = os.path.join(REPO, "pyrecode_amd", "librecode_hip.so")
    llvm = "/opt/rocm/lib/llvm/bin"
    tools = [os.path.join(llvm, t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")]
    if not os.path.exists(lib):
        pytest.fail("pyrecode_amd/librecode_hip.so is not built")
    if not all(os.path.exists(t) for t in tools):
        pytest.skip("ROCm LLVM tools not present")
    found = {}
    with tempfile.TemporaryDirectory() as d:
        fat = os.path.join(d, "fat.bin")
        subprocess.run([tools[0], "-O", "binary", "--only-section=.hip_fatbin", lib, fat], check=True)
        data = open(fat, "rb").read()
        starts = [m.start() for m in re.finditer(re.escape(b"__CLANG_OFFLOAD_BUNDLE__"), data)]
        for i, (a, b) in enumerate(zip(starts, starts[1:] + [len(data)])):
            bun, elf = os.path.join(d, "b%d.bin" % i), os.path.join(d, "b%d.elf" % i)
            open(bun, "wb").write(data[a:b])
            subprocess.run([tools[1], "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=" + bun, "--output=" + elf],
                           check=True, stderr=subprocess.DEVNULL)
            image = open(elf, "rb").read()
            sec = subprocess.run([tools[2], "-S", "-W", elf], check=True, capture_output=True, text=True).stdout
            m = re.search(r"\]\s+\.rodata\s+PROGBITS\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)", sec)
            if not m:
                continue
            ro_addr, ro_off = int(m.group(1), 16), int(m.group(2), 16)
            for line in subprocess.run([tools[2], "-s", "-W", elf], check=True, capture_output=True, text=True).stdout.splitlines():
                f = line.split()
                if len(f) >= 8 and f[-1].endswith(".kd") and f[3] == "OBJECT" and "k_sum_shift" in f[-1]:
                    off = int(f[1], 16) - ro_addr + ro_off
                    found[f[-1]] = struct.unpack_from("<II", image, off)       # group_segment_fixed_size, private_segment_fixed_size
    assert len(found) == 1, "k_sum_shift: %d symbols in the library" % len(found)
    lds, scratch = list(found.values())[0]
    assert scratch == 0 and 1 <= lds <= 81920, "k_sum_shift: %d B of LDS, %d B of scratch per lane" % (lds, scratch)
