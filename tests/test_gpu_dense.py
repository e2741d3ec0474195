"""-m gpu: dense frame batches.  The kernel (k_expand_dense_b) through the C ABI on stored streams built with numpy - every cell of the output
against the numpy model (tests/dense_model.py), the bytes around the output untouched -, refusals that must write nothing, the submit / wait
form with a refused batch between two good ones, and ReCoDeReader.get_frames_dense / iter_frames_dense / get_sub_volume on golden files and on
files this library writes, against np.stack of get_frame(z)'s toarray() indexed by numpy.  Every comparison is == on integers."""
import os
import struct

import numpy as np
import pytest

from conftest import GOLDEN, load_npz
from dense_model import dense_model
from test_gpu_frame_sums import _frames, _open, _stored_batch, _write      # the frame kinds, stored batches and written files of the summed views' tests

pytestmark = pytest.mark.gpu
FILES = os.path.join(GOLDEN, "files")
BLOCK_PIXELS = 256 * 64       # pixels one workgroup of the expand kernels owns
GUARD = 64                    # cells in front of and behind an output that must keep their fill
FILL = 0xA5


@pytest.fixture(scope="module")
def hip():
    import torch  # noqa: F401 - before the library: one HIP runtime per process
    from pyrecode_amd import _lib
    if _lib.device_count() == 0:
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    return _lib


class _Out:
    """`cells` cells of dtype dt, GUARD + skew cells behind the start of a 64-byte aligned buffer filled with 0xA5 that extends GUARD cells
    past them: where == 'host' (pageable), 'pinned' or 'device' (a torch tensor)"""

    def __init__(self, hip, cells, dt, where, skew=0):
        self.dt, self.cells, self.where, self.lo = np.dtype(dt), cells, where, GUARD + skew
        nbytes = (self.lo + cells + GUARD) * self.dt.itemsize
        if where == "device":
            import torch
            self.t = torch.full((nbytes,), FILL, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            base = self.t.data_ptr()
        else:
            if where == "pinned":
                self.pin = hip.PinnedBuffer(nbytes + 64)
                raw = self.pin.array
            else:
                raw = np.empty(nbytes + 64, np.uint8)
            off = (-raw.ctypes.data) % 64
            self.a = raw[off:off + nbytes]
            self.a[:] = FILL
            base = self.a.ctypes.data
        assert base % 64 == 0
        self.ptr = base + self.lo * self.dt.itemsize

    def check(self, want):
        """the cells are `want` (None: still the fill) and the guards have their fill"""
        got = (self.t.cpu().numpy() if self.where == "device" else self.a).view(self.dt)
        fill = np.frombuffer(bytes([FILL]) * self.dt.itemsize, self.dt)[0]
        body = got[self.lo:self.lo + self.cells]
        assert (got[:self.lo] == fill).all() and (got[self.lo + self.cells:] == fill).all(), "a cell outside the output was written"
        if want is None:
            assert (body == fill).all(), "a refused batch wrote to the output"
        else:
            assert body.dtype == want.dtype and np.array_equal(body, want.reshape(-1))

    def close(self):
        if self.where == "pinned":
            self.a = None
            self.pin.close()


def _dense(hip, geom, blob, sizes, n, region, out, prefix=None, slot=None, cells=None):
    args = tuple(geom) + (hip.ptr(blob), hip.ptr(sizes), n) + tuple(region) + (out.dt.itemsize, out.ptr, out.cells if cells is None else cells)
    L = hip.lib()
    return L.rc_expand_frames_dense(*args, hip.ptr(prefix)) if slot is None else L.rc_expand_frames_dense_submit(slot, *args)


def _regions(ny, nx):
    """full frame | the four corner pixels | first and last column | one row inside the second block only | rows that straddle the first
    block boundary | steps (2, 3) and (5, 1) | a step larger than the region"""
    full = (0, 0, nx, ny, 1, 1)
    out = [full, (0, 0, 1, 1, 1, 1), (nx - 1, 0, 1, 1, 1, 1), (0, ny - 1, 1, 1, 1, 1), (nx - 1, ny - 1, 1, 1, 1, 1),
           (0, 0, 1, ny, 1, 1), (nx - 1, 0, 1, ny, 1, 1),
           (0, 0, (nx + 1) // 2, (ny + 2) // 3, 2, 3), (0, 0, (nx + 4) // 5, ny, 5, 1), (nx // 3, ny // 2, 1, 1, nx + 7, ny + 7)]
    if ny * nx > BLOCK_PIXELS:
        r = BLOCK_PIXELS // nx                     # the row the first block ends in
        inside = [y for y in range(ny) if y * nx >= BLOCK_PIXELS and (y + 1) * nx <= min(2 * BLOCK_PIXELS, ny * nx)]
        if inside:
            out.append((0, inside[0], nx, 1, 1, 1))
            out.append((1, inside[0], max(nx - 2, 1), 1, 1, 1))
        lo, hi = max(r - 1, 0), min(r + 1, ny - 1)
        out.append((0, lo, nx, hi - lo + 1, 1, 1))                       # whole rows: the linear flush, from a block's middle
        out.append((nx // 4, lo, max(nx - nx // 4 - 1, 1), hi - lo + 1, 1, 1))    # a window across the boundary: the mapped flush
        out.append((BLOCK_PIXELS % nx if ny == 2 else 0, 0, 1, ny, 1, 1))
    return out


SHAPES = [(1, 1), (3, 21), (127, 130), (192, 256), (2, 20000)]
KINDS = [(1, 5, 1), (1, 8, 1), (1, 9, 2), (1, 12, 2), (1, 16, 2), (1, 17, 4), (1, 24, 4), (1, 32, 4), (3, 0, 1), (3, 0, 2), (2, 12, 2)]      # (level, d, cell bytes)


@pytest.mark.parametrize("level,d,cell", KINDS)
@pytest.mark.parametrize("ny,nx", SHAPES)
def test_dense_kernel_on_stored_streams(hip, ny, nx, level, d, cell):
    """rc_expand_frames_dense, op_mode 0: batches of n = 1 (each frame kind alone), 3 and 11, every region of _regions, into host and into
    device memory, and the full frame and the two stepped regions once more with the output one cell off a 64-byte boundary.  The output
    sits between guard cells; it and they are prefilled with 0xA5."""
    assert (ny * nx - 1) // BLOCK_PIXELS + 1 == {1: 1, 63: 1, 16510: 2, 49152: 3, 40000: 3}[ny * nx]
    dt = np.dtype("u%d" % cell)
    rng = np.random.default_rng(1000 * ny + 10 * d + level + cell)
    geom = (nx, ny, d, level, 0, 0)
    regions = _regions(ny, nx)
    for n, first in [(1, k) for k in range(5)] + [(3, 1), (11, 0)]:
        vals = _frames(rng, n, ny, nx, d, level, first)
        blob, sizes, _ = _stored_batch(vals, d, level, rng)
        full, counts = dense_model(blob, sizes, ny, nx, d, level, regions[0], dt)
        assert np.array_equal(full, vals.astype(dt)) and np.array_equal(counts[1:], np.cumsum((vals != 0).reshape(n, -1).sum(1)).astype(np.uint64))
        for i, region in enumerate(regions if n != 1 or first == 0 else regions[:1] + regions[7:9]):
            x0, y0, w, h, sx, sy = region
            want = np.ascontiguousarray(full[:, y0:y0 + (h - 1) * sy + 1:sy, x0:x0 + (w - 1) * sx + 1:sx])
            assert want.shape == (n, h, w)
            for where, skew in [("host", 0), ("device", 0)] + ([("device", 1), ("host", 1)] if i in (0, 7, 8) else []):
                out = _Out(hip, n * w * h, dt, where, skew)
                prefix = np.zeros(n + 1, np.uint64)
                assert _dense(hip, geom, blob, sizes, n, region, out, prefix) == hip.RC_OK, hip.last_error()
                out.check(want)
                assert np.array_equal(prefix, counts)


def _short_stream(vals, d, rng):
    """a stored level-1 batch whose frame `z` declares a value stream one field shorter than its set pixels need"""
    blob, sizes, where = _stored_batch(vals, d, 1, rng)
    z = next(z for z in range(vals.shape[0]) if where[z][1] > 8)
    at, size = where[z]
    keep = (((vals[z] != 0).sum() - 1) * d + 7) // 8
    assert keep < size
    blob = np.ascontiguousarray(np.concatenate([blob[:at + keep], blob[at + size:]]))
    sizes = sizes.copy()
    sizes[z, 1] = sizes[z, 2] = keep
    return blob, sizes


def _lz4_batch(hip, ny, nx, d, n, rng):
    """n level-1 frames through this library's own writer (LZ4): (geom, blob, sizes, per-frame offset of the binary map's stream, values)"""
    dark = rng.integers(80, 121, (ny, nx)).astype(np.uint16)
    frames = np.where(rng.random((n, ny, nx)) < 0.03, dark + rng.integers(1, 2000, (n, ny, nx)), dark // 2).astype(np.uint16)
    ctx = hip.ReduceContext(nx, ny, d, 1, 1, 2, 1, 0, max_batch=n)
    ctx.set_dark(dark, 0)
    rec_bytes, rec, _ = ctx.reduce_compress_batch(frames)
    ctx.close()
    parts, sizes, starts, at = [], np.zeros((n, 3), np.uint32), [], 0
    for z in range(n):
        r = rec_bytes[int(rec[z]):int(rec[z + 1])]
        _, cb, cp, npk = struct.unpack_from("<IIII", r.tobytes(), 0)
        assert r.size == 16 + cb + cp
        parts.append(r[16:])
        sizes[z] = (cb, cp, npk)
        starts.append(at)
        at += cb + cp
    want = np.where(frames > dark, frames - dark, 0).astype(np.uint16)
    return (nx, ny, d, 1, 1, 2), np.ascontiguousarray(np.concatenate(parts)), sizes, starts, want


@pytest.mark.parametrize("where", ["host", "pinned", "device"])
def test_refusals_write_nothing(hip, where):
    """A level-1 frame whose value stream is one field short: RC_ERR_CORRUPT, from the device (k_expand_bases).  An LZ4 frame of this
    library's writer whose first block header was damaged (one byte flipped: the block now claims to be 4 MiB longer): RC_ERR_CORRUPT or
    RC_ERR_UNSUPPORTED.  Neither writes a cell - in the synchronous form and through submit / wait (page-locked and device outputs)."""
    ny, nx, d, n = 127, 130, 12, 3
    rng = np.random.default_rng(77)
    vals = _frames(rng, n, ny, nx, d, 1)
    short_blob, short_sizes = _short_stream(vals, d, rng)
    geom, blob, sizes, starts, want = _lz4_batch(hip, ny, nx, d, n, rng)
    bad = blob.copy()
    flg = int(blob[starts[1] + 4])    # magic 4 | FLG BD [content size 8] [dictionary id 4] HC | block size 4: its third byte
    bad[starts[1] + 7 + (8 if flg & 8 else 0) + (4 if flg & 1 else 0) + 2] ^= 0x40
    region = (0, 0, nx, ny, 1, 1)
    L = hip.lib()
    for slot in [None] + ([0] if where != "host" else []):
        for g, b, s, allowed in (((nx, ny, d, 1, 0, 0), short_blob, short_sizes, (hip.RC_ERR_CORRUPT,)),
                                 (geom, bad, sizes, (hip.RC_ERR_CORRUPT, hip.RC_ERR_UNSUPPORTED))):
            out = _Out(hip, n * ny * nx, np.uint16, where)
            prefix = np.zeros(n + 1, np.uint64)
            st = _dense(hip, g, b, s, n, region, out, prefix, slot)
            if slot is not None and st == hip.RC_OK:
                st = L.rc_expand_frames_wait(slot, hip.ptr(prefix))
            assert st in allowed, (st, hip.last_error())
            out.check(None)
            out.close()
    # ... and the undamaged batch is what the writer was given
    out = _Out(hip, n * ny * nx, np.uint16, where)
    assert _dense(hip, geom, blob, sizes, n, region, out) == hip.RC_OK, hip.last_error()
    out.check(want)
    out.close()


@pytest.mark.parametrize("where", ["pinned", "device"])
def test_submit_wait_with_a_refused_batch_between_two_good_ones(hip, where):
    """Two slots in flight: good (slot 0), one field short (slot 1), good (slot 0 again, once its first batch has been waited for).  The
    verdicts are OK, RC_ERR_CORRUPT, OK; the refused batch's output keeps its fill, the prefixes are the set pixels either way.  A pageable
    host output is refused by _submit with nothing left pending."""
    ny, nx, d, n = 127, 130, 12, 4
    rng = np.random.default_rng(31)
    L = hip.lib()
    geom, region = (nx, ny, d, 1, 0, 0), (3, 2, 40, 60, 3, 2)
    batches = []
    for i in range(3):
        vals = _frames(rng, n, ny, nx, d, 1, first=i)
        blob, sizes = _short_stream(vals, d, rng) if i == 1 else _stored_batch(vals, d, 1, rng)[:2]
        want = np.ascontiguousarray(vals[:, 2:2 + 59 * 2 + 1:2, 3:3 + 39 * 3 + 1:3]).astype(np.uint16)
        batches.append((vals, blob, sizes, want, _Out(hip, n * 40 * 60, np.uint16, where)))

    def submit(i, slot):
        assert _dense(hip, geom, batches[i][1], batches[i][2], n, region, batches[i][4], slot=slot) == hip.RC_OK, hip.last_error()

    def wait(i, slot, verdict):
        prefix = np.zeros(n + 1, np.uint64)
        assert L.rc_expand_frames_wait(slot, hip.ptr(prefix)) == verdict, hip.last_error()
        assert np.array_equal(prefix[1:], np.cumsum((batches[i][0] != 0).reshape(n, -1).sum(1)).astype(np.uint64))
        batches[i][4].check(batches[i][3] if verdict == hip.RC_OK else None)
    submit(0, 0)
    submit(1, 1)
    assert _dense(hip, geom, batches[2][1], batches[2][2], n, region, batches[2][4], slot=0) == hip.RC_ERR_BAD_ARG and "submitted batch" in hip.last_error()
    wait(0, 0, hip.RC_OK)
    submit(2, 0)
    wait(1, 1, hip.RC_ERR_CORRUPT)
    wait(2, 0, hip.RC_OK)
    pageable = _Out(hip, n * 40 * 60, np.uint16, "host")
    assert _dense(hip, geom, batches[0][1], batches[0][2], n, region, pageable, slot=1) == hip.RC_ERR_BAD_ARG and "page-locked" in hip.last_error()
    assert L.rc_expand_frames_wait(1, hip.ptr(np.zeros(n + 1, np.uint64))) == hip.RC_ERR_BAD_ARG       # (nothing was queued)
    pageable.check(None)
    for b in batches:
        b[4].close()


# ---- the reader ------------------------------------------------------------------------------------------------------------------------
KEYS = [(slice(None), slice(None), slice(None)), (slice(2, None), slice(None, 4), slice(-3, None)), (slice(None, None, 2), slice(2, 100, 3), slice(None, -1, 2)),
        (slice(None, None, -1), slice(None, None, -2), slice(-3, None, -1)), (slice(-3, 4, None), slice(0, None, 1), slice(2, 4, 3)),
        (0, slice(None), slice(None)), (-1, 3, slice(None, None, -2)), (slice(None), -1, 0), (3, 0, -1), (slice(0, 4, 3), slice(None), 3),
        (slice(2, 2), slice(None), slice(None)), (slice(None, None, -2), slice(-3, None, 3), slice(2, None, 2)), (slice(1, 4), slice(4, 0, -1), slice(None))]


def _stack_of(path, part=False):
    """np.stack of the frames' toarray(), through the frame-at-a-time calls of a reader of its own"""
    rd = _open(path, part)
    out = []
    for z in range(rd._batch_frames() if part else int(rd._header["nz"])):
        d = rd.get_next_frame() if part else rd.get_frame(z)
        out.append(list(d.values())[0]["data"].toarray())
    rd.close()
    return np.stack(out)


def _check_reader(rd, stack, paths):
    """get_sub_volume on KEYS, get_frames_dense with and without a region and into the caller's arrays, iter_frames_dense in ragged batches;
    paths: what last_batch_path may say"""
    seen = set()
    keep = rd._note_batch_end
    rd._note_batch_end = lambda z: (seen.add(rd.last_batch_path), keep(z))[1]
    for key in KEYS:
        got, want = rd.get_sub_volume(*key), stack[key]
        assert got.dtype == want.dtype == np.dtype(rd._numpy_dtype) and got.shape == want.shape and np.array_equal(got, want), key
    nz = stack.shape[0]
    got = rd.get_frames_dense(1, nz - 1)
    assert got.dtype == stack.dtype and np.array_equal(got, stack[1:])
    roi = (slice(3, None, 2), slice(-7, -1))
    mine = np.full(stack[:2][(slice(None),) + roi].shape, 0xA5, stack.dtype)
    assert rd.get_frames_dense(0, 2, roi=roi, out=mine) is mine and np.array_equal(mine, stack[:2][(slice(None),) + roi])
    import torch
    tens = torch.full((stack.size * stack.dtype.itemsize,), 0xA5, dtype=torch.uint8, device="cuda")
    tens = tens.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[stack.dtype.itemsize]).view(stack.shape)
    assert rd.get_frames_dense(0, nz, out=tens) is tens
    assert np.array_equal(tens.cpu().numpy().view(stack.dtype), stack)
    for bad in (np.zeros(stack.shape, np.float32), np.zeros((nz + 1,) + stack.shape[1:], stack.dtype), np.zeros(stack.shape[::-1], stack.dtype).T):
        with pytest.raises(ValueError):
            rd.get_frames_dense(0, nz, out=bad)
    with pytest.raises(ValueError):
        rd.get_frames_dense(0, 1, roi=(slice(None, None, -1), slice(None)))
    got = [(a, arr.copy()) for a, arr in rd.iter_frames_dense(1, batch=3, roi=roi)]
    assert [a for a, _ in got] == list(range(1, nz, 3))
    assert np.array_equal(np.concatenate([arr for _, arr in got]), stack[1:][(slice(None),) + roi])
    with pytest.raises(IndexError):
        rd.get_sub_volume(slice(0, nz + 1), slice(None), slice(None))
    with pytest.raises(IndexError):
        rd.get_sub_volume(nz, slice(None), slice(None))
    assert seen <= set(paths) and seen, seen
    rd._note_batch_end = keep


@pytest.mark.parametrize("name", ["g3_l1z12.rc1", "g3_l3z.rc3", "g10_u8d8.rc1", "g11_u32d20.rc1", "g11_u32d32.rc1"])
def test_reader_on_golden_files(hip, name):
    """merged files of the reference's zlib streams (levels 1 and 3; uint8, uint16 and uint32 values): refused by the device inflate, decoded
    by the stock decoder on the thread pool, expanded on the device"""
    stack = _stack_of(os.path.join(FILES, name))
    assert stack.any() and stack.dtype == {"g3_l1z12.rc1": np.uint16, "g3_l3z.rc3": np.uint16, "g10_u8d8.rc1": np.uint8}.get(name, np.uint32)
    rd = _open(os.path.join(FILES, name))
    _check_reader(rd, stack, {"host-decode + device-expand"})
    assert rd.last_batch_path == "host-decode + device-expand"
    if name == "g3_l1z12.rc1":
        rd._host_decode_batch = lambda *a: None                   # (as when no stock decoder takes the batch)
        assert np.array_equal(rd.get_sub_volume(slice(None, None, 3), slice(None), slice(2, None)), stack[::3, :, 2:]) and rd.last_batch_path == "per-frame"
        assert np.array_equal(rd.get_frames_dense(2, 3), stack[2:5]) and rd.last_batch_path == "per-frame"
    rd.close()


def test_reader_on_part_files(hip):
    """the records of a part file, addressed by their position (their frame ids have gaps): part_frame_ids says which frames they are"""
    g = load_npz("g7_stream.npz")
    for node in range(2):
        path = os.path.join(FILES, "g7_stream.rc1_part%03d" % node)
        stack = _stack_of(path, part=True)
        assert stack.shape[0] == len(g["ids_part%d" % node]) and stack.any()
        rd = _open(path, part=True)
        _check_reader(rd, stack, {"host-decode + device-expand"})
        assert rd.part_frame_ids.tolist() == g["ids_part%d" % node].tolist()
        rd.close()


@pytest.fixture(scope="module")
def stack20():
    """20 frames of 127 x 130 (two blocks, the second one short), 12 bits, 3 % set; frame 7 is empty"""
    rng = np.random.default_rng(22)
    ny, nx, nz = 127, 130, 20
    dark = rng.integers(80, 121, (ny, nx)).astype(np.uint16)
    frames = np.where(rng.random((nz, ny, nx)) < 0.03, dark + rng.integers(1, 3900, (nz, ny, nx)), dark // 2).astype(np.uint16)
    frames[7] = 0
    return dark, frames


@pytest.mark.parametrize("level,scheme,dz,path", [(1, 2, False, "device"), (1, 1, False, "device"), (1, 8, False, "device"),
                                                  (1, 0, True, "device-inflate"), (3, 2, False, "device"), (2, 2, False, "device")])
def test_reader_on_this_librarys_files(hip, stack20, tmp_path, monkeypatch, level, scheme, dz, path):
    """LZ4, zstd, blosc-LZ4 and the device's own zlib streams at level 1, LZ4 at levels 3 and 2: every batch is decoded and written on the
    device.  With the budget of a batch lowered to one frame's cells - and below -, batch=None still means one frame a batch."""
    dark, frames = stack20
    want = np.where(frames > dark, frames - dark if level == 1 else 1, 0).astype(np.uint16)
    extra = dict(l2_statistics=2) if level == 2 else {}
    file = _write(tmp_path, dark, frames, level, scheme, dz, **extra)
    if level != 2:
        assert np.array_equal(_stack_of(file), want)
    rd = _open(file)
    _check_reader(rd, want, {path})
    for budget in (127 * 130 * 2, 1000):
        monkeypatch.setattr(rd, "_DENSE_BYTES", budget)
        got = [(a, arr.copy()) for a, arr in rd.iter_frames_dense(15)]
        assert [a for a, _ in got] == [15, 16, 17, 18, 19] and all(arr.shape == (1, 127, 130) for _, arr in got)
        assert np.array_equal(np.concatenate([arr for _, arr in got]), want[15:])
        assert np.array_equal(rd.get_sub_volume(slice(None, None, -7), slice(None), slice(None, None, 4)), want[::-7, :, ::4])
    monkeypatch.setattr(rd, "_DENSE_BYTES", 5 * 127 * 130 * 2 + 100)
    assert [(a, arr.shape[0]) for a, arr in rd.iter_frames_dense()] == [(0, 5), (5, 5), (10, 5), (15, 5)]
    assert rd.last_batch_path == path
    rd.close()


def test_sub_volume_between_frame_at_a_time_calls(hip, stack20, tmp_path):
    """get_frame in a loop - the read-ahead serves it from the fourth call on -, then get_sub_volume, then get_next_frame: the sub-volume ends
    the read-ahead's window and leaves the frame counter behind its last frame, as sum_frames does; get_next_frame goes on from there and
    the read-ahead comes back after three calls in sequence."""
    dark, frames = stack20
    want = np.where(frames > dark, frames - dark, 0).astype(np.uint16)
    rd = _open(_write(tmp_path, dark, frames, 1, 2))
    for z in range(6):
        assert np.array_equal(rd.get_frame(z)[z]["data"].toarray(), want[z])
    served = rd.readahead_frames_served
    assert served >= 3 and rd._ra is not None
    assert np.array_equal(rd.get_sub_volume(slice(2, 9, 3), slice(5, 100), slice(None, None, -1)), want[2:9:3, 5:100, ::-1])
    state = (rd._current_frame_index, rd._ra, rd._ra_iter, rd.readahead_frames_served)
    assert state == (9, None, None, served)
    rd.sum_frames(2, 7)
    assert (rd._current_frame_index, rd._ra, rd._ra_iter, rd.readahead_frames_served) == state
    rd.get_sub_volume(slice(2, 9, 3), 0, 0)
    for z in range(9, 15):
        d = rd.get_next_frame()
        assert list(d) == [z] and np.array_equal(d[z]["data"].toarray(), want[z])
    assert rd.readahead_frames_served > served and rd._current_frame_index == 15
    rd.close()
