"""-m gpu: correlation surfaces.  The kernels of rc_corr.hip through the C ABI on stored streams built with numpy - every cell of the output
against the exact model (tests/corr_model.py), the cells around the output untouched -, references from host memory, device memory and a
FrameSum, the no-wrap refusal, the submit / wait form with a refused batch in the middle, ReCoDeReader.get_frame_correlations /
iter_frame_correlations on golden files (one per route) and on part files, planted drift end to end - written with ReCoDeWriter,
estimated, and summed back onto the pattern -, and the kernel's footprint.  Every comparison is == on integers."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN, load_npz
from corr_model import corr_model, corr_of_frames, reference_bound
from test_corr_cpu import check_frame_call_arguments
from test_gpu_traces import KINDS, SHAPES, _decoded_l1, _frames, _open, _Out, _planes, _stored_batch, _thr, _write   # noqa: F401 - the traces' helpers

pytestmark = pytest.mark.gpu
FILES = os.path.join(GOLDEN, "files")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCK_PIXELS = 256 * 64       # pixels one block of the expand kernels holds
STAGE = 2048                  # set pixels a workgroup of k_expand_corr_b collects before its waves walk them (rc_corr.hip: CORR_STAGE)
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1
RADII = [0, 1, 3, 8, 16]


@pytest.fixture(scope="module")
def hip():
    import torch  # noqa: F401 - before the library: one HIP runtime per process
    from pyrecode_amd import _lib
    if _lib.device_count() == 0:
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    return _lib


class _Corr:
    """rc_corr_create .. rc_corr_destroy, called as a C program would; reference: int32[ny][nx] in host memory - or, with device=True,
    copied to the GPU first"""

    def __init__(self, hip, nx, ny, radius, reference, device=False):
        self.hip, self.L, self.S = hip, hip.lib(), 2 * radius + 1
        reference = np.ascontiguousarray(reference, np.int32)
        addr = hip.ptr(reference)
        if device:
            import torch
            self.t = torch.from_numpy(reference).cuda()
            torch.cuda.synchronize()
            addr = self.t.data_ptr()
        st = C.c_int(0)
        self.h = self.L.rc_corr_create(nx, ny, radius, addr, C.byref(st))
        assert self.h and st.value == hip.RC_OK, hip.last_error()
        assert self.L.rc_corr_side(self.h) == self.S

    def bound(self):
        return int(self.L.rc_corr_reference_bound(self.h))

    def frames(self, d, level, blob, sizes, n, out, prefix=None, slot=None, cells=None):
        args = (d, level, 0, 0, self.hip.ptr(blob), self.hip.ptr(sizes), n, out.ptr, out.cells if cells is None else cells)
        if slot is None:
            return self.L.rc_corr_frames(self.h, *args, self.hip.ptr(prefix))
        return self.L.rc_corr_frames_submit(self.h, slot, *args)

    def close(self):
        assert self.L.rc_corr_destroy(self.h) == self.hip.RC_OK


def _wild(rng, ny, nx):
    """a reference over the whole int32 range, negatives, INT32_MIN and INT32_MAX among its values"""
    return _planes(rng, ny, nx, 1)[0]


@pytest.mark.parametrize("R", RADII)
@pytest.mark.parametrize("level,d", KINDS + [(1, 1)])
@pytest.mark.parametrize("ny,nx", SHAPES)
def test_corr_kernel_on_stored_streams(hip, ny, nx, level, d, R):
    """rc_corr_frames, op_mode 0, one batch of the five frame kinds - random, empty, every pixel at 2^d - 1 (16384 set pixels a block: the
    stage is filled eight times over), only the last pixel, random - into host memory with a handle made from a host reference and into
    device memory with a handle made from a device reference.  The output sits between guard cells; it and they are prefilled with 0xA5:
    every cell is written, none beside them.  (1, 1) and (3, 21): the window is larger than the frame; (3, 21): nx < 64; (127, 130) and
    up: more than one block; (2, 20000): rows longer than a block."""
    rng = np.random.default_rng(1000 * ny + 100 * R + 10 * d + level)
    T = _wild(rng, ny, nx)
    handles = {"host": _Corr(hip, nx, ny, R, T), "device": _Corr(hip, nx, ny, R, T, device=True)}
    assert handles["host"].bound() == handles["device"].bound() == reference_bound(T)
    n, S = 5, 2 * R + 1
    vals = _frames(rng, n, ny, nx, d, level)
    blob, sizes, _ = _stored_batch(vals, d, level, rng)
    want, counts = corr_model(blob, sizes, ny, nx, d, level, T, R)
    assert want.shape == (n, S, S) and not want[1].any() and counts[5] - counts[4] > 0
    assert np.array_equal(want[:, R, R], (vals.astype(np.int64) * T).reshape(n, -1).sum(1))      # (the centre cell: 49152 * 65535 * 2^31 < 2^63)
    for where, cr in handles.items():
        out = _Out(hip, n * S * S, np.int64, where)
        prefix = np.zeros(n + 1, np.uint64)
        assert cr.frames(d, level, blob, sizes, n, out, prefix) == hip.RC_OK, hip.last_error()
        out.check(want.reshape(-1))
        assert np.array_equal(prefix, counts)
    for cr in handles.values():
        cr.close()


def test_a_workgroup_keeps_its_sums_across_blocks(hip):
    """2048 frames of 2 x 20000 (three blocks): the launch aims for 4096 workgroups, so a workgroup walks TWO blocks of its frame - blocks
    0 and 1, the stage carried from one to the next - and a second one block 2 (tests/test_corr_cpu.py: "w 625 2048 3" -> 2 2; the launch
    is padded to 8 chunks a frame, six of which have nothing to do).  Most frames hold one pixel; frame 0 and the last one are 10 % set (1600 set pixels a block: the second block finds no room behind the first
    and the stage is walked in between), frame 1 is full, frame 2 holds 1 % in block 0 and every pixel from block 1 on (a block that
    overflows the stage arrives with the stage in use), frame 3 is empty."""
    ny, nx, d, n, R = 2, 20000, 12, 2048, 3
    rng = np.random.default_rng(41)
    T = _wild(rng, ny, nx)
    vals = np.zeros((n, ny * nx), np.uint32)
    vals[np.arange(n), rng.integers(0, ny * nx, n)] = rng.integers(1, 1 << d, n)
    for f in (0, n - 1):
        vals[f] = np.where(rng.random(ny * nx) < 0.1, rng.integers(1, 1 << d, ny * nx), 0)
    vals[1] = (1 << d) - 1
    vals[2] = np.where(rng.random(ny * nx) < 0.01, rng.integers(1, 1 << d, ny * nx), 0)
    vals[2, BLOCK_PIXELS:] = 77
    vals[3] = 0
    per_block = [(vals[0, a:a + BLOCK_PIXELS] != 0).sum() for a in (0, BLOCK_PIXELS)]
    assert min(per_block) > STAGE // 2 and max(per_block) < STAGE and 0 < (vals[2, :BLOCK_PIXELS] != 0).sum() < STAGE
    blob, sizes, _ = _stored_batch(vals.reshape(n, ny, nx), d, 1, rng)
    want, counts = corr_model(blob, sizes, ny, nx, d, 1, T, R)
    cr = _Corr(hip, nx, ny, R, T)
    out = _Out(hip, n * 49, np.int64, "device")
    prefix = np.zeros(n + 1, np.uint64)
    assert cr.frames(d, 1, blob, sizes, n, out, prefix) == hip.RC_OK, hip.last_error()
    out.check(want.reshape(-1))
    assert np.array_equal(prefix, counts) and not want[3].any() and want[4].any()
    cr.close()


def test_references_from_host_device_and_a_frame_sum(hip):
    """the same reference from host and from device memory through the FrameCorrelation wrapper (numpy of a narrower dtype, a torch tensor
    of a wider one): the same bound, the same surfaces; a FrameSum as the reference gives the surfaces of its fetched cells, and is refused
    once a cell of it could pass 2^31 - 1"""
    import torch
    ny, nx, d, R = 127, 130, 12, 3
    rng = np.random.default_rng(3)
    vals = _frames(rng, 5, ny, nx, d, 1)
    blob, sizes, _ = _stored_batch(vals, d, 1, rng)
    geom = (nx, ny, d, 1, 0, 0)
    T = _wild(rng, ny, nx)
    want, counts = corr_model(blob, sizes, ny, nx, d, 1, T, R)
    with hip.FrameCorrelation(nx, ny, T, R) as a, hip.FrameCorrelation(nx, ny, torch.from_numpy(T.astype(np.int64)).cuda(), R) as b:
        assert a.reference_bound() == b.reference_bound() == reference_bound(T) == 1 << 31 and a.side == b.side == 7 and a.radius == 3
        for fc in (a, b):
            got, prefix = fc.frames(geom, blob, sizes, 5)
            assert got.dtype == np.int64 and got.shape == (5, 7, 7) and np.array_equal(got, want) and np.array_equal(prefix, counts)
        out = np.zeros((5, 7, 7), np.int64)
        assert a.frames_status(geom, blob, sizes, 5, out, out.size) == hip.RC_OK and np.array_equal(out, want)      # (nnz_prefix may be NULL)
    small = rng.integers(-(1 << 15), 1 << 15, (ny, nx)).astype(np.int16)
    with hip.FrameCorrelation(nx, ny, small) as a:
        assert a.radius == 8 and a.side == 17 and np.array_equal(a.frames(geom, blob, sizes, 5)[0], corr_model(blob, sizes, ny, nx, d, 1, small, 8)[0])
    with pytest.raises(ValueError, match="correlated with a handle"):
        with hip.FrameCorrelation(21, 3, np.ones((3, 21), np.int32)) as fc:
            fc.frames(geom, blob, sizes, 5)
    # a summed view as the reference: its cells never leave the device
    fs = hip.FrameSum(nx, ny)
    fs.add(geom, blob, sizes, 5)
    fs.add(geom, blob, sizes, 5)
    cells = fs.fetch()
    assert np.array_equal(cells, 2 * vals.sum(0, dtype=np.uint64)) and fs.bound() == 10 * 4095
    with hip.FrameCorrelation(nx, ny, fs, R) as fc:
        assert fc.reference_bound() == int(cells.max())
        assert np.array_equal(fc.frames(geom, blob, sizes, 5)[0], corr_model(blob, sizes, ny, nx, d, 1, cells, R)[0])
    assert np.array_equal(fs.fetch(), cells)                  # (the view is as it was)
    with pytest.raises(ValueError, match="FrameSum of"):
        hip.FrameCorrelation(nx + 1, ny, fs, R)
    fs.close()
    one = hip.FrameSum(1, 1)
    empty, esizes = np.zeros(4096, np.uint8), np.tile(np.array([[1, 0, 0]], np.uint32), (4096, 1))
    for i in range(9):                                         # 9 * 4096 * 65535 > 2^31 - 1 > 8 * 4096 * 65535
        if i == 8:
            hip.FrameCorrelation(1, 1, one, 0).close()
        one.add((1, 1, 16, 1, 0, 0), empty, esizes, 4096)
    assert one.bound() == 9 * 4096 * 65535 > INT32_MAX > 8 * 4096 * 65535
    with pytest.raises(ValueError, match="2\\^31 - 1"):
        hip.FrameCorrelation(1, 1, one, 0)
    one.close()


def test_frame_call_arguments_are_checked_before_anything_is_queued(hip):
    check_frame_call_arguments(hip)


def test_no_silent_wrap(hip):
    """3 x 65535, 16 bits, a reference of INT32_MAX.  A frame with 10 set pixels of 65535 is accepted and exact (its value stream has room for
    10 fields: 10 * 65535 * (2^31 - 1) is far below 2^63); a frame with every pixel set is RC_ERR_OUT_TOO_SMALL before anything is queued, in
    both forms, and out keeps its fill (tests/test_corr_cpu.py's "b" cases: the two lie on either side of the bound)."""
    ny, nx, d, R = 3, 65535, 16, 1
    rng = np.random.default_rng(11)
    T = np.full((ny, nx), INT32_MAX, np.int32)
    cr = _Corr(hip, nx, ny, R, T)
    assert cr.bound() == INT32_MAX
    vals = np.zeros((1, ny, nx), np.uint32)
    vals.reshape(-1)[np.append(rng.choice(ny * nx - 1, 9, replace=False), ny * nx - 1)] = 65535      # (the last pixel among them)
    blob, sizes, _ = _stored_batch(vals, d, 1, rng)
    assert sizes[0, 2] == 20
    want, counts = corr_model(blob, sizes, ny, nx, d, 1, T, R)
    assert want[0, 1, 1] == 655350 * INT32_MAX and counts[1] == 10
    for where in ("host", "device"):
        out = _Out(hip, 9, np.int64, where)
        prefix = np.zeros(2, np.uint64)
        assert cr.frames(d, 1, blob, sizes, 1, out, prefix) == hip.RC_OK, hip.last_error()
        out.check(want.reshape(-1))
        assert np.array_equal(prefix, counts)
    full, fsizes, _ = _stored_batch(np.full((1, ny, nx), 65535, np.uint32), d, 1, rng)
    assert fsizes[0, 2] == 2 * 196605
    for where in ("host", "device"):
        out = _Out(hip, 9, np.int64, where)
        assert cr.frames(d, 1, full, fsizes, 1, out, np.zeros(2, np.uint64)) == hip.RC_ERR_OUT_TOO_SMALL and "2^63" in hip.last_error()
        assert cr.frames(d, 1, full, fsizes, 1, out, slot=1) == hip.RC_ERR_OUT_TOO_SMALL
        out.check(None)
    assert cr.L.rc_expand_frames_wait(1, hip.ptr(np.zeros(4, np.uint64))) == hip.RC_ERR_BAD_ARG      # (nothing was queued)
    cr.close()


def test_submit_wait_with_a_rejected_batch_in_the_middle(hip):
    """Six batches alternating between the two slots on ONE handle, into page-locked (even batches) and device (odd batches) outputs.  Batch 3
    declares one frame's value stream two bytes shorter than its set pixels need - the refusal k_expand_bases makes on the device -:
    rc_expand_frames_wait answers RC_ERR_CORRUPT for it and its out keeps its fill; the other five are exact.  A busy slot is RC_ERR_BAD_ARG."""
    ny, nx, d, n, R = 127, 130, 12, 5, 3
    rng = np.random.default_rng(9)
    T = _wild(rng, ny, nx)
    cr = _Corr(hip, nx, ny, R, T, device=True)
    L = cr.L
    batches = []
    for i in range(6):
        vals = _frames(rng, n, ny, nx, d, 1, first=i)
        blob, sizes, where = _stored_batch(vals, d, 1, rng)
        want, counts = corr_model(blob, sizes, ny, nx, d, 1, T, R)
        want = want.reshape(-1)
        if i == 3:
            z = next(z for z in range(n) if where[z][1] > 8)
            at, size = where[z]
            blob = np.ascontiguousarray(np.concatenate([blob[:at + size - 2], blob[at + size:]]))
            sizes[z, 1] = sizes[z, 2] = size - 2
            want = None
        pin = hip.PinnedBuffer(blob.size + 64)          # (a submitted batch's bytes stay where they are until the wait)
        pin.array[:blob.size] = blob
        batches.append((pin, sizes, want, counts, _Out(hip, n * 49, np.int64, "device" if i & 1 else "pinned")))
    verdicts = []

    def wait(i):
        prefix = np.zeros(n + 1, np.uint64)
        verdicts.append(L.rc_expand_frames_wait(i & 1, hip.ptr(prefix)))
        assert np.array_equal(prefix, batches[i][3])          # (the counts are valid either way)
        batches[i][4].check(batches[i][2])
    for i in range(6):
        if i >= 2:
            wait(i - 2)
        pin, sizes, _, _, out = batches[i]
        assert cr.frames(d, 1, pin.array, sizes, n, out, slot=i & 1) == hip.RC_OK, hip.last_error()
    assert cr.frames(d, 1, batches[0][0].array, batches[0][1], n, batches[0][4], slot=0) == hip.RC_ERR_BAD_ARG and "submitted batch" in hip.last_error()
    pageable = np.zeros(n * 49, np.int64)
    wait(4)
    wait(5)
    assert verdicts == [hip.RC_OK] * 3 + [hip.RC_ERR_CORRUPT] + [hip.RC_OK] * 2
    args = (d, 1, 0, 0, hip.ptr(batches[0][0].array), hip.ptr(batches[0][1]), n, hip.ptr(pageable), pageable.size)
    assert L.rc_corr_frames_submit(cr.h, 0, *args) == hip.RC_ERR_BAD_ARG and "page-locked" in hip.last_error() and "rc_corr_frames_submit" in hip.last_error()
    assert L.rc_expand_frames_wait(0, hip.ptr(np.zeros(n + 1, np.uint64))) == hip.RC_ERR_BAD_ARG and not pageable.any()
    cr.close()
    for pin, _, _, _, out in batches:
        out.close()
        pin.close()


# ---- the reader ------------------------------------------------------------------------------------------------------------------------
def _same(got, decoded, T, R, ids):
    assert sorted(got) == ["corr", "count", "frame_ids"]
    S = 2 * R + 1
    want = corr_of_frames(decoded, T, R)
    assert got["corr"].dtype == np.int64 and got["corr"].shape == (len(decoded), S, S) and np.array_equal(got["corr"], want)
    assert got["count"].dtype == np.int64 and np.array_equal(got["count"], (np.asarray(decoded) != 0).reshape(len(decoded), -1).sum(1))
    assert got["frame_ids"].dtype == np.int64 and got["frame_ids"].tolist() == [int(i) for i in ids]
    return want


def _reference(rng, ny, nx):
    return rng.integers(-1000, 1001, (ny, nx)).astype(np.int32)


def test_correlations_on_a_golden_file_per_route(hip):
    rng = np.random.default_rng(5)
    # stored streams (op_mode 0): the device takes them as they are
    g = load_npz("g3_l1ro16.npz")
    dec = g["decoded"].astype(np.int64)
    nz, ny, nx = dec.shape
    T = _reference(rng, ny, nx)
    rd = _open(os.path.join(FILES, "g3_l1ro16.rc1"))
    assert _same(rd.get_frame_correlations(0, nz, T, radius=2), dec, T, 2, range(nz)).any() and rd.last_batch_path == "device"
    rd.close()
    # stock zlib: refused by the device inflate, decoded on the host, correlated on the device
    g = load_npz("g3_l1z12.npz")
    dec = g["decoded"].astype(np.int64)
    nz, ny, nx = dec.shape
    T = _reference(rng, ny, nx)
    rd = _open(os.path.join(FILES, "g3_l1z12.rc1"))
    assert _same(rd.get_frame_correlations(0, nz, T), dec, T, 8, range(nz)).any() and rd.last_batch_path == "host-decode + device-expand"
    _same(rd.get_frame_correlations(2, 5, T, radius=1), dec[2:7], T, 1, range(2, 7))
    seen = [(z, t) for z, t in rd.iter_frame_correlations(batch=3, reference=T, radius=3)]
    assert [z for z, _ in seen] == list(range(0, nz, 3)) and rd.last_batch_path == "host-decode + device-expand"
    for z, t in seen:
        _same(t, dec[z:z + 3], T, 3, range(z, min(z + 3, nz)))
    assert list(rd.iter_frame_correlations(0, 0, reference=T)) == []
    with pytest.raises(ValueError):
        rd.get_frame_correlations(0, nz + 1, T)
    with pytest.raises(ValueError):
        rd.get_frame_correlations(0, 2)                                        # (no reference)
    with pytest.raises(ValueError):
        rd.get_frame_correlations(0, 2, np.ones((ny, nx + 1), np.int32))
    with pytest.raises(ValueError):
        rd.get_frame_correlations(0, 2, T, radius=17)
    rd.close()
    # level 3: every value is 1
    g = load_npz("g3_l3z.npz")
    dec = (g["frames"] > _thr(g)).astype(np.int64)
    T = _reference(rng, dec.shape[1], dec.shape[2])
    rd = _open(os.path.join(FILES, "g3_l3z.rc3"))
    _same(rd.get_frame_correlations(0, dec.shape[0], T, radius=4), dec, T, 4, range(dec.shape[0]))
    rd.close()
    # bz2 without a stock decoder for the batch: frame by frame, restated as stored frames
    g = load_npz("g9_l1bz2.npz")
    dec = _decoded_l1(g)
    T = _reference(rng, dec.shape[1], dec.shape[2])
    rd = _open(os.path.join(FILES, "g9_l1bz2.rc1_part000"), part=True)
    n, ids = rd._batch_frames(), rd.part_frame_ids
    rd._host_decode_batch = lambda *a: None
    _same(rd.get_frame_correlations(0, n, T, radius=2), dec[ids], T, 2, ids)
    assert rd.last_batch_path == "per-frame"
    got = list(rd.iter_frame_correlations(batch=2, reference=T, radius=2))
    assert rd.last_batch_path == "per-frame" and [z for z, _ in got] == list(range(0, n, 2))
    for z, t in got:
        _same(t, dec[ids[z:z + 2]], T, 2, ids[z:z + 2])
    rd.close()
    rd = _open(os.path.join(FILES, "g11_u32d20.rc1"))
    with pytest.raises(NotImplementedError, match="16 bits"):
        rd.get_frame_correlations(0, 1, np.ones((int(rd._header["ny"]), int(rd._header["nx"])), np.int32))
    rd.close()


def test_correlations_on_part_files_with_one_shared_handle(hip):
    """G7's part files, whose ids have gaps: 'frame_ids' are the frames' ids, and the two readers share one FrameCorrelation - one copy of
    the reference on the device - which stays usable after both are closed"""
    g = load_npz("g7_stream.npz")
    dec = _decoded_l1(g)
    rng = np.random.default_rng(7)
    T = _reference(rng, dec.shape[1], dec.shape[2])
    fc = hip.FrameCorrelation(dec.shape[2], dec.shape[1], T, 5)
    for node in range(2):
        ids = g["ids_part%d" % node]
        rd = _open(os.path.join(FILES, "g7_stream.rc1_part%03d" % node), part=True)
        _same(rd.get_frame_correlations(0, len(ids), fc), dec[ids], T, 5, ids)
        _same(rd.get_frame_correlations(2, 3, fc, radius=1), dec[ids[2:5]], T, 5, ids[2:5])          # (the handle's radius holds)
        at = 0
        for z, t in rd.iter_frame_correlations(batch=4, reference=fc):
            assert z == at
            _same(t, dec[ids[z:z + 4]], T, 5, ids[z:z + 4])
            at += 4
        assert at >= len(ids)
        rd.close()
    assert fc.reference_bound() == reference_bound(T)
    fc.close()
    rd = _open(os.path.join(FILES, "g7_stream.rc1_part000"), part=True)
    with pytest.raises(ValueError, match="FrameCorrelation of"):
        with hip.FrameCorrelation(8, 4, np.ones((4, 8), np.int32)) as other:
            rd.get_frame_correlations(0, 1, other)
    rd.close()


def test_planted_drift_end_to_end(hip, tmp_path):
    """127 x 130, 12 bits, R = 3: a sparse pattern with a margin of R clear at every edge, frame f the pattern rolled by a known s_f - the
    corners of the window among them -, written with ReCoDeWriter (LZ4: decoded on the device), correlated with the pattern
    (get_frame_correlations), estimated (estimate_shifts: exactly -s_f) and summed with those shifts (sum_frames(shifts=...)): every cell
    equals the sum of the unshifted pattern frames, n times the pattern.  Then the recipe as a user runs it, the reference a summed view of
    the first fraction, which never leaves the device."""
    from pyrecode_amd.reader_batched import estimate_shifts
    ny, nx, R, nz = 127, 130, 3, 12
    rng = np.random.default_rng(17)
    pattern = np.zeros((ny, nx), np.int64)
    pattern[R:ny - R, R:nx - R] = np.where(rng.random((ny - 2 * R, nx - 2 * R)) < 0.01, rng.integers(1, 3900, (ny - 2 * R, nx - 2 * R)), 0)
    drifts = [(0, 0), (0, 0), (R, R), (-R, -R), (R, -R), (-R, R), (1, -2), (0, 3)] + [tuple(int(v) for v in rng.integers(-R, R + 1, 2)) for _ in range(nz - 8)]
    dark = rng.integers(80, 121, (ny, nx)).astype(np.uint16)
    moved = np.stack([np.roll(pattern, s, (0, 1)) for s in drifts])
    frames = np.where(moved > 0, dark + moved, dark // 2).astype(np.uint16)
    rd = _open(_write(tmp_path, dark, frames, 1, 2))
    got = rd.get_frame_correlations(0, nz, pattern, radius=R)
    assert rd.last_batch_path == "device" and np.array_equal(got["corr"], corr_of_frames(moved, pattern, R))
    assert got["count"].tolist() == [int((pattern != 0).sum())] * nz
    est = estimate_shifts(got)
    assert est["shifts"].tolist() == [[-s[0], -s[1]] for s in drifts] and est["valid"].all()
    assert est["peak"].tolist() == [int((pattern * pattern).sum())] * nz
    summed = rd.sum_frames(shifts=est["shifts"])
    assert np.array_equal(summed, (nz * pattern).astype(np.uint64)) and not np.array_equal(rd.sum_frames(), summed)
    # the three library calls of the recipe: a first fraction as the reference, the surfaces per fraction of two frames, the aligned sum
    fs = hip.FrameSum(nx, ny)
    assert rd.sum_frames(0, 2, into=fs) == 2
    est = estimate_shifts(rd.get_frame_correlations(0, nz, fs, radius=R))
    assert est["shifts"].tolist() == [[-s[0], -s[1]] for s in drifts]             # (T = twice the pattern: the same peaks)
    assert np.array_equal(rd.sum_frames(shifts=est["shifts"]), summed)
    fs.close()
    rd.close()


def test_corr_kernel_footprint():
    """k_expand_corr_b's descriptors in the built library (read the way test_gpu_traces.py::test_trace_kernel_footprint reads its kernel's;
    no GPU needed, but the file's other tests do): five instantiations - 1, 2, 5, 9 and 18 accumulators a lane -, no scratch, and at most
    32 768 B of static LDS: the five workgroups a CU holds at the largest instantiation's registers (4 waves per SIMD and one to spare)
    share its 160 KiB.  Sizes from the descriptor only."""
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
                if len(f) >= 8 and f[-1].endswith(".kd") and f[3] == "OBJECT" and "k_expand_corr_b" in f[-1]:
                    off = int(f[1], 16) - ro_addr + ro_off
                    found[f[-1]] = struct.unpack_from("<II", image, off)       # group_segment_fixed_size, private_segment_fixed_size
    assert len(found) == 5, "k_expand_corr_b (1, 2, 5, 9 and 18 accumulators a lane) is not in the library"
    for name, (lds, scratch) in found.items():
        assert scratch == 0 and 0 < lds <= 32768, "%s: %d B of LDS, %d B of scratch per lane" % (name, lds, scratch)
