"""-m gpu: summed views.  The accumulation kernel (k_expand_sum_b) through the C ABI on stored streams built with numpy, the accumulator's
bookkeeping (bound, reset, refusals), the submit / wait form with a rejected batch in the middle, ReCoDeReader.sum_frames / iter_frame_sums on
golden files and on files this library writes, and ReCoDeViewer over part files whose ids have gaps.  Expected values are plain numpy: at
level 1 the sum over frames of where(frame > thr, frame - thr, 0), at levels 2 and 3 the count of frame > thr; equality is exact."""
import ctypes as C
import os
import shutil

import numpy as np
import pytest

from conftest import GOLDEN, load_npz

pytestmark = pytest.mark.gpu
FILES = os.path.join(GOLDEN, "files")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCK_PIXELS = 256 * 64       # pixels one workgroup of the expand kernels owns (rc_device.h: WG words of 64 bitmap bits)


@pytest.fixture(scope="module")
def hip():
    from pyrecode_amd import _lib
    if _lib.device_count() == 0:
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    return _lib


# ---- stored (op_mode 0) frames from numpy ------------------------------------------------------------------------------------------------
def _pack_fields(vals, d):
    """d-bit LSB-first fields, zero-padded to a byte (recode_writer.py:637-652)"""
    bits = ((np.asarray(vals, np.uint32)[:, None] >> np.arange(d, dtype=np.uint32)) & 1).astype(np.uint8).reshape(-1)
    return np.packbits(bits, bitorder="little")


def _stored_batch(values, d, level, rng):
    """values uint32[n][ny][nx] (0 = not set) -> (blob, sizes uint32[n][3], per-frame (start of the value stream in blob, its bytes))"""
    n = values.shape[0]
    parts, sizes, at, where = [], np.zeros((n, 3), np.uint32), 0, []
    for z in range(n):
        flat = values[z].reshape(-1)
        bm = np.packbits(flat != 0, bitorder="little")
        parts.append(bm)
        at += bm.size
        sizes[z, 0] = bm.size
        if level == 1:
            pv = _pack_fields(flat[flat != 0], d)
        elif level == 2:
            pv = rng.integers(0, 256, 3 + z, dtype=np.uint8)      # the statistics stream: bytes the sum steps over
        else:
            pv = np.zeros(0, np.uint8)
        parts.append(pv)
        where.append((at, pv.size))
        at += pv.size
        sizes[z, 1] = sizes[z, 2] = pv.size
    return np.ascontiguousarray(np.concatenate(parts)), sizes, where


def _frames(rng, n, ny, nx, d, level, first=0):
    """the frame kinds of a batch in turn, starting with kind `first`: 1 % random | empty | every pixel at 2^d - 1 | only the last pixel | 1 %
    random; pixel (ny // 2, nx // 2) is set in every frame but the empty one.  At levels 2 / 3 a set pixel's value is 1."""
    top = (1 << d) - 1 if level == 1 else 1
    out = np.zeros((n, ny, nx), np.uint32)
    for z in range(n):
        kind = (first + z) % 5
        if kind in (0, 4):
            out[z] = np.where(rng.random((ny, nx)) < 0.01, rng.integers(1, top + 1, (ny, nx)), 0)
        elif kind == 2:
            out[z] = top
        elif kind == 3:
            out[z, -1, -1] = top
        if kind != 1:
            out[z, ny // 2, nx // 2] = max(1, top - z)
    return out


class _Sum:
    """rc_sum_create .. rc_sum_destroy, called as a C program would"""

    def __init__(self, hip, nx, ny):
        self.hip, self.L, self.nx, self.ny = hip, hip.lib(), nx, ny
        st = C.c_int(0)
        self.h = self.L.rc_sum_create(nx, ny, C.byref(st))
        assert self.h and st.value == hip.RC_OK, hip.last_error()

    def add(self, d, level, blob, sizes, n, prefix=None, mode=0, scheme=0):
        return self.L.rc_sum_add_frames(self.h, d, level, mode, scheme, self.hip.ptr(blob), self.hip.ptr(sizes), n, self.hip.ptr(prefix))

    def submit(self, slot, d, level, blob, sizes, n):
        return self.L.rc_sum_add_frames_submit(self.h, slot, d, level, 0, 0, self.hip.ptr(blob), self.hip.ptr(sizes), n)

    def fetch(self, reset=False):
        out = np.full((self.ny, self.nx), 0xA5A5A5A5, np.uint32)
        assert self.L.rc_sum_fetch(self.h, self.hip.ptr(out), int(reset)) == self.hip.RC_OK, self.hip.last_error()
        return out

    def bound(self):
        return int(self.L.rc_sum_bound(self.h))

    def close(self):
        assert self.L.rc_sum_destroy(self.h) == self.hip.RC_OK


SHAPES = [(1, 1), (3, 21), (127, 130), (192, 256)]       # one pixel | N = 63 < a word | a block + 126 pixels, N % 64 = 62, N % 8 = 6 | three blocks
KINDS = [(1, 9), (1, 12), (1, 16), (3, 0), (2, 12)]      # (level, bit depth)


@pytest.mark.parametrize("level,d", KINDS)
@pytest.mark.parametrize("ny,nx", SHAPES)
def test_sum_kernel_on_stored_streams(hip, ny, nx, level, d):
    """rc_sum_add_frames, op_mode 0.  n = 1 (each frame kind as a batch of its own), n = 3 (one frame group: the kernel's loop sums three
    frames in LDS before its flush) and n = 11 (the launch splits a batch of more than 4 frames into groups - 4 + 4 + 3 -, whose flushes meet in
    the cells), all into one view: the sum of everything added, and every batch's set-pixel prefix."""
    assert (ny * nx - 1) // BLOCK_PIXELS + 1 == {1: 1, 63: 1, 16510: 2, 49152: 3}[ny * nx]
    rng = np.random.default_rng(1000 * ny + 10 * d + level)
    view = _Sum(hip, nx, ny)
    want = np.zeros((ny, nx), np.uint64)
    batches = [(1, k) for k in range(5)] + [(3, 0), (3, 3), (11, 0)]
    grown = 0
    for n, first in batches:
        vals = _frames(rng, n, ny, nx, d, level, first)
        blob, sizes, _ = _stored_batch(vals, d, level, rng)
        prefix = np.zeros(n + 1, np.uint64)
        assert view.add(d, level, blob, sizes, n, prefix) == hip.RC_OK, hip.last_error()
        assert np.array_equal(prefix[1:], np.cumsum((vals != 0).reshape(n, -1).sum(1)).astype(np.uint64))
        want += vals.sum(0, dtype=np.uint64)
        grown += n * ((1 << d) - 1 if level == 1 else 1)
        assert view.bound() == grown
    got = view.fetch()
    assert int(want.max()) <= grown and int(want[ny // 2, nx // 2]) > 0
    assert np.array_equal(got.astype(np.uint64), want)
    view.close()


def test_accumulation_reset_and_geometry(hip):
    """Two adds and a fetch are the sum; a fetch leaves the cells as they are, one with reset leaves zeros and a bound of 0; stored frames of
    another shape are RC_ERR_BAD_ARG, 20-bit values RC_ERR_UNSUPPORTED - and neither changes a cell or the bound."""
    ny, nx, d = 127, 130, 12
    rng = np.random.default_rng(5)
    view = _Sum(hip, nx, ny)
    a, b = _frames(rng, 3, ny, nx, d, 1), _frames(rng, 2, ny, nx, d, 1, first=2)
    for vals in (a, b):
        blob, sizes, _ = _stored_batch(vals, d, 1, rng)
        assert view.add(d, 1, blob, sizes, vals.shape[0]) == hip.RC_OK, hip.last_error()      # (nnz_prefix may be NULL)
    want = (a.sum(0, dtype=np.uint64) + b.sum(0, dtype=np.uint64)).astype(np.uint32)
    assert np.array_equal(view.fetch(), want) and np.array_equal(view.fetch(), want)
    assert view.bound() == 5 * 4095
    other, osz, _ = _stored_batch(_frames(rng, 2, 3, 21, d, 1), d, 1, rng)
    assert view.add(d, 1, other, osz, 2) == hip.RC_ERR_BAD_ARG and "geometry" in hip.last_error()
    blob, sizes, _ = _stored_batch(a, d, 1, rng)
    assert view.add(20, 1, blob, sizes, 3) == hip.RC_ERR_UNSUPPORTED and "16" in hip.last_error()
    assert view.submit(0, 20, 1, blob, sizes, 3) == hip.RC_ERR_UNSUPPORTED
    assert view.bound() == 5 * 4095 and np.array_equal(view.fetch(reset=True), want)
    assert view.bound() == 0 and not view.fetch().any()
    assert view.add(d, 1, blob, sizes, 3) == hip.RC_OK
    assert np.array_equal(view.fetch().astype(np.uint64), a.sum(0, dtype=np.uint64))
    view.close()
    fs = hip.FrameSum(nx, ny)
    for bad in (np.zeros((ny, nx), np.uint16), np.zeros(ny * nx - 1, np.uint32), np.zeros((ny, 2 * nx), np.uint32)[:, ::2]):
        with pytest.raises(ValueError, match="uint32"):
            fs.fetch(out=bad)
    fs.close()
    with pytest.raises(ValueError, match="view of"):
        fs = hip.FrameSum(nx, ny)
        try:
            fs.add((21, 3, d, 1, 0, 0), other, osz, 2)
        finally:
            fs.close()


def test_no_silent_wrap(hip):
    """One pixel, 16 bits: 65 535 frames of 65 535 are accepted - the bound is 65 535^2 = 4 294 836 225, and so is the cell.  Three more frames
    could pass 2^32 - 1: RC_ERR_OUT_TOO_SMALL before anything is queued, cell and bound unchanged."""
    n = 65535
    vals = np.full((n, 1, 1), 65535, np.uint32)
    blob = np.tile(np.array([1, 0xFF, 0xFF], np.uint8), n)
    sizes = np.tile(np.array([1, 2, 2], np.uint32), (n, 1))
    view = _Sum(hip, 1, 1)
    assert view.add(16, 1, blob, sizes, n) == hip.RC_OK, hip.last_error()
    assert view.bound() == 4294836225 == int(vals.sum(dtype=np.uint64))
    assert int(view.fetch()[0, 0]) == 4294836225
    assert view.add(16, 1, blob[:9], sizes[:3], 3) == hip.RC_ERR_OUT_TOO_SMALL
    assert view.submit(1, 16, 1, blob[:9], sizes[:3], 3) == hip.RC_ERR_OUT_TOO_SMALL
    assert view.L.rc_expand_frames_wait(1, hip.ptr(np.zeros(4, np.uint64))) == hip.RC_ERR_BAD_ARG      # (nothing was queued)
    assert view.bound() == 4294836225 and int(view.fetch()[0, 0]) == 4294836225
    view.close()


def test_submit_wait_with_a_rejected_batch_in_the_middle(hip):
    """Six batches, alternating between the two slots, into one view.  Batch 3 declares one frame's value stream two bytes shorter than its
    set pixels need - the refusal k_expand_bases makes on the device -: rc_expand_frames_wait answers RC_ERR_CORRUPT for it and it adds
    nothing; the cells are the sum of the other five."""
    ny, nx, d, n = 127, 130, 12, 5
    rng = np.random.default_rng(9)
    view = _Sum(hip, nx, ny)
    L = view.L
    want = np.zeros((ny, nx), np.uint64)
    batches = []
    for i in range(6):
        vals = _frames(rng, n, ny, nx, d, 1, first=i)
        blob, sizes, where = _stored_batch(vals, d, 1, rng)
        if i == 3:
            z = next(z for z in range(n) if where[z][1] > 8)
            at, size = where[z]
            blob = np.ascontiguousarray(np.concatenate([blob[:at + size - 2], blob[at + size:]]))
            sizes[z, 1] = sizes[z, 2] = size - 2
        else:
            want += vals.sum(0, dtype=np.uint64)
        batches.append((vals, blob, sizes))
    verdicts = []

    def wait(i):
        vals = batches[i][0]
        prefix = np.zeros(n + 1, np.uint64)
        verdicts.append(L.rc_expand_frames_wait(i & 1, hip.ptr(prefix)))
        assert np.array_equal(prefix[1:], np.cumsum((vals != 0).reshape(n, -1).sum(1)).astype(np.uint64))     # (the counts are valid either way)
    for i in range(6):
        if i >= 2:
            wait(i - 2)
        assert view.submit(i & 1, d, 1, batches[i][1], batches[i][2], n) == hip.RC_OK, hip.last_error()
    assert view.submit(0, d, 1, batches[0][1], batches[0][2], n) == hip.RC_ERR_BAD_ARG and "submitted batch" in hip.last_error()
    got = view.fetch()              # waits for the two adds that are still queued
    wait(4)
    wait(5)
    assert verdicts == [hip.RC_OK] * 3 + [hip.RC_ERR_CORRUPT] + [hip.RC_OK] * 2
    assert np.array_equal(got.astype(np.uint64), want)
    assert view.bound() == 6 * n * 4095         # (an upper bound: the rejected batch was counted when it was queued)
    view.close()


# ---- the reader ------------------------------------------------------------------------------------------------------------------------
def _open(path, part=False):
    from pyrecode_amd.recode_reader import ReCoDeReader
    rd = ReCoDeReader(path, is_intermediate=part)
    rd.open(print_header=False)
    return rd


def _thr(g):
    cfg = dict(zip(g["cfg_keys"].tolist(), (int(v) for v in g["cfg_vals"])))
    return (g["dark"] + g["dark"].dtype.type(cfg["calibration_threshold_epsilon"])).astype(g["dark"].dtype)


def _l1_sum(frames, thr):
    return np.where(frames > thr, frames.astype(np.int64) - thr, 0).sum(0).astype(np.uint64)


def test_sum_frames_on_golden_files(hip):
    g = load_npz("g3_l1z12.npz")
    want = g["decoded"].sum(0, dtype=np.uint64)
    assert np.array_equal(want, _l1_sum(g["frames"], _thr(g))) and int(want.max()) == 11004
    rd = _open(os.path.join(FILES, "g3_l1z12.rc1"))
    got = rd.sum_frames()
    assert got.dtype == np.uint64 and got.shape == want.shape and np.array_equal(got, want)
    assert rd.last_batch_path == "host-decode + device-expand"          # stock zlib: refused by the device inflate, decoded on the host, added on the device
    assert np.array_equal(rd.sum_frames(2, 5, batch=2), g["decoded"][2:7].sum(0, dtype=np.uint64))
    views = [(a, k, img.copy()) for a, k, img in rd.iter_frame_sums(5)]
    assert [(a, k) for a, k, _ in views] == [(0, 5), (5, 3)]
    for a, k, img in views:                  # (copies: the generator's images are views of one page-locked buffer)
        assert img.dtype == np.uint32 and np.array_equal(img, g["decoded"][a:a + k].sum(0, dtype=np.uint64))
    assert rd.sum_frames(0, 0).sum() == 0
    with pytest.raises(ValueError):
        rd.sum_frames(0, 9)
    rd.close()
    g = load_npz("g3_l3z.npz")
    rd = _open(os.path.join(FILES, "g3_l3z.rc3"))
    assert np.array_equal(rd.sum_frames(batch=3), (g["frames"] > _thr(g)).sum(0).astype(np.uint64))
    rd.close()
    g = load_npz("g10_u8d8.npz")
    rd = _open(os.path.join(FILES, "g10_u8d8.rc1"))
    assert np.array_equal(rd.sum_frames(), g["decoded"].sum(0, dtype=np.uint64)) and g["decoded"].any()
    rd.close()
    rd = _open(os.path.join(FILES, "g11_u32d20.rc1"))
    with pytest.raises(NotImplementedError, match="16 bits"):
        rd.sum_frames()
    rd.close()


def test_sum_frames_on_part_files_whose_ids_have_gaps(hip):
    g = load_npz("g7_stream.npz")
    thr = _thr(g)
    for node in range(2):
        ids = g["ids_part%d" % node]
        rd = _open(os.path.join(FILES, "g7_stream.rc1_part%03d" % node), part=True)
        assert np.array_equal(rd.sum_frames(batch=4), _l1_sum(g["frames"][ids], thr))
        assert rd.part_frame_ids.tolist() == ids.tolist()
        assert np.array_equal(rd.sum_frames(2, 3), _l1_sum(g["frames"][ids[2:5]], thr))
        rd.close()


def _write(tmp, dark, frames, level, scheme, device_zlib=False, **extra):
    from pyrecode_amd.params import InputParams
    from pyrecode_amd.recode_reader import merge_parts
    from pyrecode_amd.recode_writer import ReCoDeWriter
    g = load_npz("g3_l1z12.npz")
    nz, ny, nx = frames.shape
    cfg = dict(zip(g["cfg_keys"].tolist(), (int(v) for v in g["cfg_vals"])))
    cfg.update(num_rows=ny, num_cols=nx, num_frames=nz, num_threads=2, compression_scheme=scheme, reduction_level=level,
               calibration_threshold_epsilon=0, **extra)
    (tmp / "params.txt").write_text("".join("%s = %d\n" % kv for kv in cfg.items()))
    for node in range(2):
        ip = InputParams()
        ip.load(str(tmp / "params.txt"))
        w = ReCoDeWriter("s", dark_data=dark, output_directory=str(tmp), input_params=ip, mode="batch", validation_frame_gap=-1, node_id=node,
                         batch_size=4, device_zlib=device_zlib)
        w.start()
        w.run(frames)
        w.close()
    merge_parts(str(tmp), "s.rc%d" % level, 2)
    return str(tmp / ("s.rc%d" % level))


@pytest.fixture(scope="module")
def stack():
    """20 frames of 127 x 130 (two blocks, the second one short), 12 bits, 3 % set; frame 7 is empty"""
    rng = np.random.default_rng(21)
    ny, nx, nz = 127, 130, 20
    dark = rng.integers(80, 121, (ny, nx)).astype(np.uint16)
    frames = np.where(rng.random((nz, ny, nx)) < 0.03, dark + rng.integers(1, 3900, (nz, ny, nx)), dark // 2).astype(np.uint16)
    frames[7] = 0
    return dark, frames


@pytest.mark.parametrize("level,scheme,dz,path", [(1, 2, False, "device"), (1, 1, False, "device"), (1, 8, False, "device"),
                                                  (1, 0, True, "device-inflate"), (3, 2, False, "device")])
def test_sum_frames_on_this_librarys_files(hip, stack, tmp_path, level, scheme, dz, path):
    """LZ4, zstd, blosc-LZ4 and the device's own zlib streams at level 1, LZ4 at level 3: every batch - 8, 8 and a ragged 4 - is decoded and
    added on the device; a caller's handle receives the same frames."""
    dark, frames = stack
    want = _l1_sum(frames, dark) if level == 1 else (frames > dark).sum(0).astype(np.uint64)
    rd = _open(_write(tmp_path, dark, frames, level, scheme, dz))
    paths = set()
    keep = rd._note_batch_end
    rd._note_batch_end = lambda z: (paths.add(rd.last_batch_path), keep(z))[1]
    got = rd.sum_frames(batch=8)
    assert paths == {path} and np.array_equal(got, want)
    fs = hip.FrameSum(130, 127)
    assert rd.sum_frames(3, 9, batch=4, into=fs) == 9 and rd.sum_frames(12, 1, into=fs) == 1
    part = (_l1_sum(frames[3:13], dark) if level == 1 else (frames[3:13] > dark).sum(0)).astype(np.uint32)
    assert fs.bound() == 10 * (4095 if level == 1 else 1) and np.array_equal(fs.fetch(reset=True), part)
    fs.close()
    rd.close()


@pytest.mark.parametrize("scheme,path", [(2, "device"), (0, "per-frame")])
def test_sum_frames_at_level_2_and_on_the_frame_at_a_time_route(hip, stack, tmp_path, scheme, path):
    """Level 2 counts set pixels like level 3, the statistics stream stepped over: an LZ4 file on the device; a zlib file - level 2 has no
    host-decoded batches - frame by frame, restated as stored frames and added like any batch, so a caller's handle receives them too."""
    dark, frames = stack
    want = (frames > dark).sum(0).astype(np.uint64)
    rd = _open(_write(tmp_path, dark, frames, 2, scheme, l2_statistics=2))
    assert np.array_equal(rd.sum_frames(batch=8), want) and rd.last_batch_path == path
    fs = hip.FrameSum(130, 127)
    assert rd.sum_frames(5, 7, batch=3, into=fs) == 7
    assert np.array_equal(fs.fetch(), (frames[5:12] > dark).sum(0).astype(np.uint32))
    fs.close()
    rd.close()


def test_sum_frames_on_host_only_schemes(hip):
    """bz2 (the reference's file): the stock decoder on the thread pool, then one add of the stored pieces; a level-1 file that has to go frame
    by frame keeps its values (the restated frames carry them at the file's own depth, so the bound grows as for any batch)"""
    g = load_npz("g9_l1bz2.npz")
    want = _l1_sum(g["frames"], _thr(g))
    rd = _open(os.path.join(FILES, "g9_l1bz2.rc1_part000"), part=True)
    n = rd._batch_frames()
    rd.close()
    rd = _open(os.path.join(FILES, "g9_l1bz2.rc1_part001"), part=True)
    n += rd._batch_frames()
    got = rd.sum_frames()
    assert rd.last_batch_path == "host-decode + device-expand"
    rd._host_decode_batch = lambda *a: None                   # (as when no stock decoder takes the batch)
    assert np.array_equal(rd.sum_frames(), got) and rd.last_batch_path == "per-frame"
    rd.close()
    rd = _open(os.path.join(FILES, "g9_l1bz2.rc1_part000"), part=True)
    got = got + rd.sum_frames()
    rd.close()
    assert n == g["frames"].shape[0] and got.any() and np.array_equal(got, want)


def test_sum_frames_folds_before_a_cell_could_wrap(hip, stack, tmp_path, monkeypatch):
    """sum_frames keeps its own view below FrameSum.LIMIT: with the limit lowered to what two batches of 8 twelve-bit frames can reach, the
    third batch makes it fetch, fold into the uint64 result and reset first - the sum is the same; a caller's handle is not folded: the add
    that could pass the cells' real limit is refused (test_no_silent_wrap), here the lowered one is simply passed."""
    dark, frames = stack
    rd = _open(_write(tmp_path, dark, frames, 1, 2))
    resets = []
    fetch = hip.FrameSum.fetch_view
    monkeypatch.setattr(hip.FrameSum, "LIMIT", 16 * 4095)
    monkeypatch.setattr(hip.FrameSum, "fetch_view", lambda self, reset=False: (resets.append(reset), fetch(self, reset))[1])
    assert np.array_equal(rd.sum_frames(batch=8), _l1_sum(frames, dark))
    assert resets == [True, False]
    fs = hip.FrameSum(130, 127)
    assert rd.sum_frames(batch=8, into=fs) == 20 and fs.bound() == 20 * 4095
    assert np.array_equal(fs.fetch(), _l1_sum(frames, dark).astype(np.uint32))
    fs.close()
    rd.close()


def test_iter_frame_sums_alternates_two_views_on_the_callers_thread(hip, stack, tmp_path, monkeypatch):
    """Windows of 6 frames in batches of 4 over 20 frames: 6, 6, 6 and 2 frames, every window two batches but the last, the batches of all
    windows one sequence on the two slots and the windows alternating between two device views - each image is its window's sum, also when
    the consumer is slow to come back or stops early.  Every device call is made on the thread that drives the generator (a helper thread
    would run on its own current device, not the caller's)."""
    import threading
    dark, frames = stack
    rd = _open(_write(tmp_path, dark, frames, 1, 1))
    threads, submits = set(), []
    submit = hip.FrameSum.submit_status
    monkeypatch.setattr(hip.FrameSum, "submit_status",
                        lambda self, slot, *a: (threads.add(threading.get_ident()), submits.append((id(self), slot)), submit(self, slot, *a))[2])
    seen = []
    for a, k, img in rd.iter_frame_sums(6, batch=4):
        assert img.dtype == np.uint32 and np.array_equal(img, _l1_sum(frames[a:a + k], dark))
        seen.append((a, k))
    assert seen == [(0, 6), (6, 6), (12, 6), (18, 2)] and rd.last_batch_path == "device"
    assert threads == {threading.get_ident()}
    assert [slot for _, slot in submits] == [0, 1, 0, 1, 0, 1, 0] and len({v for v, _ in submits}) == 2
    assert [v for v, _ in submits] == [submits[0][0]] * 2 + [submits[2][0]] * 2 + [submits[0][0]] * 2 + [submits[2][0]]
    it = rd.iter_frame_sums(5, 3, 12, batch=2)
    a, k, img = next(it)
    assert (a, k) == (3, 5) and np.array_equal(img, _l1_sum(frames[3:8], dark))
    it.close()                                   # (a batch of the next window is queued: waited for, both views freed)
    assert np.array_equal(rd.sum_frames(3, 12), _l1_sum(frames[3:15], dark))
    rd.close()


def test_viewer_over_part_files(hip, tmp_path, capsys):
    """ReCoDeViewer on copies of G7's part files, fractionation 5: views of 5, 5, 5 and 1 frames - the warning once -, each the float64 sum of
    its frames by id, over both parts; then None."""
    from pyrecode_amd.utils.viewer import ReCoDeViewer
    g = load_npz("g7_stream.npz")
    thr = _thr(g)
    for node in range(2):
        shutil.copy(os.path.join(FILES, "g7_stream.rc1_part%03d" % node), str(tmp_path))
    v = ReCoDeViewer(str(tmp_path), "g7_stream.rc1", 2, 5)
    assert v.get_shape() == g["frames"].shape[1:]
    capsys.readouterr()
    for start, count in ((0, 5), (5, 5), (10, 5), (15, 1)):
        view = v.get_next_view()
        assert view["start"] == start and view["n_Frames"] == count
        assert view["view"].dtype == np.float64
        assert np.array_equal(view["view"], _l1_sum(g["frames"][start:start + count], thr).astype(np.float64))
    assert v.get_next_view() is None
    out = capsys.readouterr().out
    assert out.count("Warning: read fewer frames (1) than requested (5).") == 1 and out.count("Warning") == 1
    v.close()


def test_sum_kernel_footprint():
    """k_expand_sum_b's descriptor in the built library (read the way tests/test_kernel_footprint.py reads the others'; no GPU needed, but the
    file's other tests do): no scratch, and at most 81 920 B of static LDS - two workgroups share a CU's 160 KiB."""
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
                if len(f) >= 8 and f[-1].endswith(".kd") and f[3] == "OBJECT" and "k_expand_sum_b" in f[-1]:
                    off = int(f[1], 16) - ro_addr + ro_off
                    found[f[-1]] = struct.unpack_from("<II", image, off)       # group_segment_fixed_size, private_segment_fixed_size
    assert len(found) == 1, "k_expand_sum_b is not in the library"
    lds, scratch = list(found.values())[0]
    assert scratch == 0 and 0 < lds <= 81920, "k_expand_sum_b: %d B of LDS, %d B of scratch per lane" % (lds, scratch)
