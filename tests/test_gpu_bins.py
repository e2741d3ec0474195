"""-m gpu: binned frame traces.  The kernels of rc_bins.hip through the C ABI on stored streams built with numpy - every cell of the output
against the exact model (tests/bins_model.py), the cells around the output untouched -, label maps from host and device memory, the label
patterns (one bin, every pixel its own bin, random, radial), a batch in which a workgroup walks more than one block, the identity against
rc_trace_frames on the device, the submit / wait form with a refused batch in the middle, ReCoDeReader.get_frame_bins / iter_frame_bins on
golden files (one per route) and on part files, and the kernel's footprint.  Every comparison is == on integers."""
import ctypes as C
import os

import numpy as np
import pytest

import bins_model as bm
from bins_model import IGNORE, bins_model, bins_of_frames, one_hot_planes
from conftest import GOLDEN, load_npz
from test_bins_cpu import check_frame_call_arguments
from test_gpu_traces import _decoded_l1, _frames, _open, _Out, _stored_batch, _thr, _Trace

pytestmark = pytest.mark.gpu
FILES = os.path.join(GOLDEN, "files")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCK_PIXELS = 256 * 64       # pixels one block of the expand kernels holds
SHAPES = [(1, 1), (3, 21), (127, 130), (192, 256), (2, 20000), (64, 64)]
BINS = [1, 2, 17, 256, 4096]
KINDS = [(1, 1), (1, 12), (1, 16), (2, 12), (3, 0)]      # (level, bit depth); frame kind 2 of a batch is full: at d = 16 every value is 65535


@pytest.fixture(scope="module")
def hip():
    import torch  # noqa: F401 - before the library: one HIP runtime per process
    from pyrecode_amd import _lib
    if _lib.device_count() == 0:
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    return _lib


class _Bins:
    """rc_bins_create .. rc_bins_destroy, called as a C program would; labels: uint16[ny][nx] in host memory - or, with device=True, copied
    to the GPU first"""

    def __init__(self, hip, nx, ny, B, labels, device=False):
        self.hip, self.L, self.B = hip, hip.lib(), B
        labels = np.ascontiguousarray(labels, np.uint16)
        addr = hip.ptr(labels)
        if device:
            import torch
            self.t = torch.from_numpy(labels.view(np.int16)).cuda()
            torch.cuda.synchronize()
            addr = self.t.data_ptr()
        st = C.c_int(0)
        self.h = self.L.rc_bins_create(nx, ny, B, addr, C.byref(st))
        assert self.h and st.value == hip.RC_OK, hip.last_error()
        assert self.L.rc_bins_count(self.h) == B

    def frames(self, d, level, blob, sizes, n, out, prefix=None, slot=None, cells=None):
        args = (d, level, 0, 0, self.hip.ptr(blob), self.hip.ptr(sizes), n, out.ptr, out.cells if cells is None else cells)
        if slot is None:
            return self.L.rc_bins_frames(self.h, *args, self.hip.ptr(prefix))
        return self.L.rc_bins_frames_submit(self.h, slot, *args)

    def close(self):
        assert self.L.rc_bins_destroy(self.h) == self.hip.RC_OK


def _random_labels(rng, ny, nx, B, ignore):
    """every pixel in a random bin - a fifth of them in none with `ignore` -, the last bin and (B > 1) bin 0 among them"""
    lab = rng.integers(0, B, (ny, nx)).astype(np.uint16)
    if ignore:
        lab[rng.random((ny, nx)) < 0.2] = IGNORE
    lab[ny // 2, nx // 2] = B - 1              # (the pixel every non-empty frame of _frames sets)
    lab[-1, -1] = 0 if not ignore else lab[-1, -1]
    return lab


def _run(hip, handles, d, level, blob, sizes, n, want, counts):
    """host handle into host memory, device handle into device memory: every cell, the guards, the prefix"""
    for where, hb in handles.items():
        out = _Out(hip, n * 2 * hb.B, np.int64, where)
        prefix = np.zeros(n + 1, np.uint64)
        assert hb.frames(d, level, blob, sizes, n, out, prefix) == hip.RC_OK, hip.last_error()
        out.check(want.reshape(-1))
        assert np.array_equal(prefix, counts)


@pytest.mark.parametrize("B", BINS)
@pytest.mark.parametrize("level,d", KINDS)
@pytest.mark.parametrize("ny,nx", SHAPES)
def test_bins_kernel_on_stored_streams(hip, ny, nx, level, d, B):
    """rc_bins_frames, op_mode 0, one batch of the five frame kinds - random, empty, every pixel at 2^d - 1 (a full frame), only the last
    pixel, random - under random labels with and without the ignore label, into host memory with a handle made from host labels and into
    device memory with a handle made from device labels.  The output sits between guard cells; it and they are prefilled with 0xA5: every
    cell is written, none beside them.  (1, 1) and (3, 21): fewer pixels than a word; (127, 130) and up: more than one block; (2, 20000):
    rows longer than a block.  B = 1, 2, 17, 256: the smallest histogram tier; 4096: the largest (more bins than most frames have pixels)."""
    rng = np.random.default_rng(1000 * ny + 100 * level + 10 * d + B)
    n = 5
    vals = _frames(rng, n, ny, nx, d, level)
    blob, sizes, _ = _stored_batch(vals, d, level, rng)
    for ignore in (False, True):
        lab = _random_labels(rng, ny, nx, B, ignore)
        handles = {"host": _Bins(hip, nx, ny, B, lab), "device": _Bins(hip, nx, ny, B, lab, device=True)}
        want, counts = bins_model(blob, sizes, ny, nx, d, level, lab, B)
        assert want.shape == (n, 2, B) and not want[1].any() and counts[5] - counts[4] > 0
        kept = (lab != IGNORE)[None]
        assert np.array_equal(want[:, 0].sum(1), ((vals != 0) & kept).reshape(n, -1).sum(1))
        assert np.array_equal(want[:, 1].sum(1), (vals.astype(np.int64) * kept).reshape(n, -1).sum(1))
        assert want[2, 0].sum() == kept.sum()                                                    # (the full frame: a bin's count is its area)
        if level != 1:
            assert np.array_equal(want[:, 0], want[:, 1])
        _run(hip, handles, d, level, blob, sizes, n, want, counts)
        for hb in handles.values():
            hb.close()


@pytest.mark.parametrize("level,d", [(1, 12), (1, 16), (3, 0)])
@pytest.mark.parametrize("ny,nx", [(3, 21), (127, 130), (192, 256), (2, 20000), (64, 64)])
def test_label_patterns(hip, ny, nx, level, d):
    """every pixel in ONE bin - the only bin, and bin 5 of 17 (all of a wave's adds go to one LDS address) -; every pixel in no bin; every pixel its
    OWN bin (64 x 64 with B = 4096; elsewhere pixel p in bin p % 4096: no two neighbours share one); runs of one bin that end inside a
    word (bins of 5 consecutive pixels); a radial map about the frame's middle and one about a corner, cut off before the frame's edge"""
    from pyrecode_amd.reader_batched import bin_areas, radial_labels
    rng = np.random.default_rng(ny + d)
    n = 5
    vals = _frames(rng, n, ny, nx, d, level)
    vals[4] = np.where(rng.random((ny, nx)) < 0.3, vals[2], 0)        # (denser than 1 %: words with several set pixels)
    blob, sizes, _ = _stored_batch(vals, d, level, rng)
    p = np.arange(ny * nx).reshape(ny, nx)
    mid = radial_labels(ny, nx, ny // 2, nx // 2 + (0.5 if nx % 2 == 0 else 0), 1, n_bins=4096)      # ((2, 20000) reaches past bin 4095: cut off there)
    corner = radial_labels(ny, nx, -0.5, -0.5, 2, n_bins=max(1, min(ny, nx) // 4))
    maps = [(np.zeros((ny, nx), np.uint16), 1), (np.full((ny, nx), 5, np.uint16), 17), (np.full((ny, nx), IGNORE, np.uint16), 2),
            ((p % 4096).astype(np.uint16), 4096), ((p // 5 % 300).astype(np.uint16), 300),
            (mid, int(mid[mid != IGNORE].max()) + 1), (corner, max(1, min(ny, nx) // 4))]
    if (ny, nx) == (64, 64):
        assert np.unique(maps[3][0]).size == 4096
    assert (corner == IGNORE).any() and ((mid == IGNORE).any() == (nx == 20000))
    for lab, B in maps:
        want, counts = bins_model(blob, sizes, ny, nx, d, level, lab, B)
        assert np.array_equal(want, bins_of_frames(vals, lab, B)) and np.array_equal(want[2, 0], bin_areas(lab, B))
        handles = {"host": _Bins(hip, nx, ny, B, lab), "device": _Bins(hip, nx, ny, B, lab, device=True)}
        _run(hip, handles, d, level, blob, sizes, n, want, counts)
        for hb in handles.values():
            hb.close()


@pytest.mark.parametrize("B", [17, 4096])
def test_a_workgroup_keeps_its_histogram_across_blocks(hip, B):
    """2048 frames of 192 x 256 (three blocks) in one batch.  B = 17: the launch aims for 4096 workgroups, so a workgroup walks blocks 0 and
    1 of its frame with the histogram carried from one to the next, and a second one the short last chunk, block 2 (tests/test_bins_cpu.py:
    "w 768 2048 17" -> 2 2).  B = 4096: 512 workgroups are aimed for and one workgroup walks all three blocks ("w 768 2048 4096" -> 3 1).
    Most frames hold one pixel; frame 0 and the last one are 10 % set, frame 1 is full, frame 2 holds 1 % in block 0 and every pixel from
    block 1 on, frame 3 is empty.  Bins 0 .. 2 are horizontal bands that follow the blocks, so a bin's total needs every block's share."""
    ny, nx, d, n = 192, 256, 12, 2048
    assert bm.chunks(3, n, B) == ((2, 2) if B == 17 else (3, 1))
    rng = np.random.default_rng(41 + B)
    lab = _random_labels(rng, ny, nx, B, True)
    lab[::7] = (np.arange(ny)[::7, None] * nx // BLOCK_PIXELS % B).astype(np.uint16)      # (rows of bin 0, 1, 2: the block they lie in)
    vals = np.zeros((n, ny * nx), np.uint32)
    vals[np.arange(n), rng.integers(0, ny * nx, n)] = rng.integers(1, 1 << d, n)
    for f in (0, n - 1):
        vals[f] = np.where(rng.random(ny * nx) < 0.1, rng.integers(1, 1 << d, ny * nx), 0)
    vals[1] = (1 << d) - 1
    vals[2] = np.where(rng.random(ny * nx) < 0.01, rng.integers(1, 1 << d, ny * nx), 0)
    vals[2, BLOCK_PIXELS:] = 77
    vals[3] = 0
    blob, sizes, _ = _stored_batch(vals.reshape(n, ny, nx), d, 1, rng)
    want, counts = bins_model(blob, sizes, ny, nx, d, 1, lab, B)
    hb = _Bins(hip, nx, ny, B, lab)
    out = _Out(hip, n * 2 * B, np.int64, "device")
    prefix = np.zeros(n + 1, np.uint64)
    assert hb.frames(d, 1, blob, sizes, n, out, prefix) == hip.RC_OK, hip.last_error()
    out.check(want.reshape(-1))
    assert np.array_equal(prefix, counts) and not want[3].any() and want[4].any()
    if B == 17:
        assert all(want[1, 0, b] > nx for b in range(3))
    hb.close()


def test_the_identity_against_the_traces_on_the_device(hip):
    """B = 16 on the batches of the kernel test, 127 x 130 at 12 and 16 bits and at level 3: plane 1 equals rc_trace_frames' 16 weighted
    columns under the one-hot planes labels == b, both computed by the device; summed over the bins, plane 0 plus the ignored set pixels is
    the traces' count and plane 1 plus their values the traces' sum (the ignored ones read off a second trace handle, whose one plane is
    labels == 0xFFFF)"""
    ny, nx, n, B = 127, 130, 5, 16
    rng = np.random.default_rng(16)
    lab = _random_labels(rng, ny, nx, B, True)
    hb = _Bins(hip, nx, ny, B, lab, device=True)
    hot, gone = _Trace(hip, nx, ny, one_hot_planes(lab, B)), _Trace(hip, nx, ny, (lab == IGNORE).astype(np.int32)[None], device=True)
    for level, d in ((1, 12), (1, 16), (3, 0)):
        vals = _frames(rng, n, ny, nx, d, level)
        blob, sizes, _ = _stored_batch(vals, d, level, rng)
        got, t_hot, t_gone = np.zeros((n, 2, B), np.int64), np.zeros((n, 20), np.int64), np.zeros((n, 5), np.int64)
        outs = []
        for h, dst in ((hb, got), (hot, t_hot), (gone, t_gone)):
            out = _Out(hip, dst.size, np.int64, "host")
            assert h.frames(d, level, blob, sizes, n, out, np.zeros(n + 1, np.uint64)) == hip.RC_OK, hip.last_error()
            outs.append(out.a.view(np.int64)[out.lo:out.lo + out.cells].reshape(dst.shape).copy())
        got, t_hot, t_gone = outs
        assert np.array_equal(got[:, 1], t_hot[:, 4:]) and got[:, 1].any()
        assert np.array_equal(got[:, 1].sum(1) + t_gone[:, 4], t_hot[:, 1]) and t_gone[:, 4].any()
        if level == 3:
            assert np.array_equal(got[:, 0], t_hot[:, 4:]) and np.array_equal(got[:, 0].sum(1) + t_gone[:, 4], t_hot[:, 0])
        assert np.array_equal(got, bins_model(blob, sizes, ny, nx, d, level, lab, B)[0])
    for h in (hb, hot, gone):
        h.close()


def test_labels_from_host_and_device_through_the_wrapper(hip):
    """the same labels as numpy of a wider dtype and as a torch tensor on the GPU: the same n_bins - the largest label + 1 -, the same
    result; nnz_prefix optional; a device label at or above n_bins is refused by the small kernel; another geometry is a ValueError"""
    import torch
    ny, nx, d, B = 127, 130, 12, 300
    rng = np.random.default_rng(3)
    vals = _frames(rng, 5, ny, nx, d, 1)
    blob, sizes, _ = _stored_batch(vals, d, 1, rng)
    geom = (nx, ny, d, 1, 0, 0)
    lab = _random_labels(rng, ny, nx, B, True)
    want, counts = bins_model(blob, sizes, ny, nx, d, 1, lab, B)
    with hip.FrameBins(nx, ny, lab.astype(np.int64)) as a, hip.FrameBins(nx, ny, torch.from_numpy(lab.astype(np.int32)).cuda()) as b:
        assert a.n_bins == b.n_bins == B
        for fb in (a, b):
            got, prefix = fb.frames(geom, blob, sizes, 5)
            assert got.dtype == np.int64 and got.shape == (5, 2, B) and np.array_equal(got, want) and np.array_equal(prefix, counts)
        out = np.zeros((5, 2, B), np.int64)
        assert a.frames_status(geom, blob, sizes, 5, out, out.size) == hip.RC_OK and np.array_equal(out, want)      # (nnz_prefix may be NULL)
    with hip.FrameBins(nx, ny, lab, n_bins=B + 50) as fb:                   # (more bins than labels: the rest stay zero)
        got = fb.frames(geom, blob, sizes, 5)[0]
        assert np.array_equal(got[:, :, :B], want) and not got[:, :, B:].any()
    with pytest.raises(ValueError, match="binned with a handle"):
        with hip.FrameBins(21, 3, np.zeros((3, 21), np.uint16)) as fb:
            fb.frames(geom, blob, sizes, 5)
    with pytest.raises(ValueError, match="n_bins"):
        hip.FrameBins(nx, ny, torch.from_numpy(lab.astype(np.int32)).cuda(), n_bins=B - 1)
    dev = torch.from_numpy(lab.view(np.int16)).cuda()
    torch.cuda.synchronize()
    st = C.c_int(0)
    assert hip.lib().rc_bins_create(nx, ny, B - 1, dev.data_ptr(), C.byref(st)) is None and st.value == hip.RC_ERR_BAD_ARG and "0xFFFF" in hip.last_error()
    h = hip.lib().rc_bins_create(nx, ny, B, dev.data_ptr(), C.byref(st))
    assert h and st.value == hip.RC_OK and hip.lib().rc_bins_destroy(h) == hip.RC_OK


def test_frame_call_arguments_are_checked_before_anything_is_queued(hip):
    check_frame_call_arguments(hip)


def test_submit_wait_with_a_rejected_batch_in_the_middle(hip):
    """Six batches alternating between the two slots on ONE handle, into page-locked (even batches) and device (odd batches) outputs.  Batch 3
    declares one frame's value stream two bytes shorter than its set pixels need - the refusal k_expand_bases makes on the device -:
    rc_expand_frames_wait answers RC_ERR_CORRUPT for it and its out keeps its fill; the other five are exact.  A busy slot is RC_ERR_BAD_ARG."""
    ny, nx, d, n, B = 127, 130, 12, 5, 300
    rng = np.random.default_rng(9)
    lab = _random_labels(rng, ny, nx, B, True)
    hb = _Bins(hip, nx, ny, B, lab, device=True)
    L = hb.L
    batches = []
    for i in range(6):
        vals = _frames(rng, n, ny, nx, d, 1, first=i)
        blob, sizes, where = _stored_batch(vals, d, 1, rng)
        want, counts = bins_model(blob, sizes, ny, nx, d, 1, lab, B)
        want = want.reshape(-1)
        if i == 3:
            z = next(z for z in range(n) if where[z][1] > 8)
            at, size = where[z]
            blob = np.ascontiguousarray(np.concatenate([blob[:at + size - 2], blob[at + size:]]))
            sizes[z, 1] = sizes[z, 2] = size - 2
            want = None
        pin = hip.PinnedBuffer(blob.size + 64)          # (a submitted batch's bytes stay where they are until the wait)
        pin.array[:blob.size] = blob
        batches.append((pin, sizes, want, counts, _Out(hip, n * 2 * B, np.int64, "device" if i & 1 else "pinned")))
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
        assert hb.frames(d, 1, pin.array, sizes, n, out, slot=i & 1) == hip.RC_OK, hip.last_error()
    assert hb.frames(d, 1, batches[0][0].array, batches[0][1], n, batches[0][4], slot=0) == hip.RC_ERR_BAD_ARG and "submitted batch" in hip.last_error()
    pageable = np.zeros(n * 2 * B, np.int64)
    wait(4)
    wait(5)
    assert verdicts == [hip.RC_OK] * 3 + [hip.RC_ERR_CORRUPT] + [hip.RC_OK] * 2
    args = (d, 1, 0, 0, hip.ptr(batches[0][0].array), hip.ptr(batches[0][1]), n, hip.ptr(pageable), pageable.size)
    assert L.rc_bins_frames_submit(hb.h, 0, *args) == hip.RC_ERR_BAD_ARG and "page-locked" in hip.last_error() and "rc_bins_frames_submit" in hip.last_error()
    assert L.rc_expand_frames_wait(0, hip.ptr(np.zeros(n + 1, np.uint64))) == hip.RC_ERR_BAD_ARG and not pageable.any()
    hb.close()
    for pin, _, _, _, out in batches:
        out.close()
        pin.close()


# ---- the reader ------------------------------------------------------------------------------------------------------------------------
def _same(got, decoded, lab, B, ids):
    assert sorted(got) == ["count", "frame_ids", "sum"]
    want = bins_of_frames(decoded, lab, B)
    for key, plane in (("count", 0), ("sum", 1)):
        assert got[key].dtype == np.int64 and got[key].shape == (len(decoded), B) and np.array_equal(got[key], want[:, plane]), key
    assert got["frame_ids"].dtype == np.int64 and got["frame_ids"].tolist() == [int(i) for i in ids]
    return want


def _file_labels(rng, ny, nx, B=40):
    lab = rng.integers(0, B, (ny, nx)).astype(np.uint16)
    lab[rng.random((ny, nx)) < 0.1] = IGNORE
    lab[0, 0] = B - 1
    return lab


def test_bins_on_a_golden_file_per_route(hip):
    from pyrecode_amd.reader_batched import radial_labels
    rng = np.random.default_rng(5)
    # stored streams (op_mode 0): the device takes them as they are
    g = load_npz("g3_l1ro16.npz")
    dec = g["decoded"].astype(np.int64)
    nz, ny, nx = dec.shape
    lab = _file_labels(rng, ny, nx)
    rd = _open(os.path.join(FILES, "g3_l1ro16.rc1"))
    assert _same(rd.get_frame_bins(0, nz, lab), dec, lab, 40, range(nz)).any() and rd.last_batch_path == "device"
    rd.close()
    # stock zlib: refused by the device inflate, decoded on the host, binned on the device
    g = load_npz("g3_l1z12.npz")
    dec = g["decoded"].astype(np.int64)
    nz, ny, nx = dec.shape
    lab = _file_labels(rng, ny, nx)
    rd = _open(os.path.join(FILES, "g3_l1z12.rc1"))
    assert _same(rd.get_frame_bins(0, nz, lab), dec, lab, 40, range(nz)).any() and rd.last_batch_path == "host-decode + device-expand"
    _same(rd.get_frame_bins(2, 5, lab, n_bins=64), dec[2:7], lab, 64, range(2, 7))
    seen = [(z, t) for z, t in rd.iter_frame_bins(batch=3, labels=lab)]
    assert [z for z, _ in seen] == list(range(0, nz, 3)) and rd.last_batch_path == "host-decode + device-expand"
    for z, t in seen:
        _same(t, dec[z:z + 3], lab, 40, range(z, min(z + 3, nz)))
    # a radial profile about a half centre, as a user asks for it
    rad = radial_labels(ny, nx, (ny - 1) / 2, (nx - 1) / 2)
    B = int(rad.max()) + 1
    want = _same(rd.get_frame_bins(0, nz, rad), dec, rad, B, range(nz))
    assert np.array_equal(want, bins_of_frames(dec, bm.radial_model(ny, nx, ny - 1, nx - 1, 1, 4096), B)) and want[:, 0].sum() == (dec != 0).sum()
    assert list(rd.iter_frame_bins(0, 0, labels=lab)) == []
    with pytest.raises(ValueError):
        rd.get_frame_bins(0, nz + 1, lab)
    with pytest.raises(ValueError):
        rd.get_frame_bins(0, 2)                                                 # (no labels)
    with pytest.raises(ValueError):
        rd.get_frame_bins(0, 2, np.zeros((ny, nx + 1), np.uint16))
    with pytest.raises(ValueError):
        rd.get_frame_bins(0, 2, lab, n_bins=39)
    rd.close()
    # level 3: every value is 1
    g = load_npz("g3_l3z.npz")
    dec = (g["frames"] > _thr(g)).astype(np.int64)
    lab = _file_labels(rng, dec.shape[1], dec.shape[2])
    rd = _open(os.path.join(FILES, "g3_l3z.rc3"))
    got = rd.get_frame_bins(0, dec.shape[0], lab)
    _same(got, dec, lab, 40, range(dec.shape[0]))
    assert np.array_equal(got["count"], got["sum"]) and got["count"].any()
    rd.close()
    # bz2 without a stock decoder for the batch: frame by frame, restated as stored frames
    g = load_npz("g9_l1bz2.npz")
    dec = _decoded_l1(g)
    lab = _file_labels(rng, dec.shape[1], dec.shape[2])
    rd = _open(os.path.join(FILES, "g9_l1bz2.rc1_part000"), part=True)
    n, ids = rd._batch_frames(), rd.part_frame_ids
    rd._host_decode_batch = lambda *a: None
    _same(rd.get_frame_bins(0, n, lab), dec[ids], lab, 40, ids)
    assert rd.last_batch_path == "per-frame"
    got = list(rd.iter_frame_bins(batch=2, labels=lab))
    assert rd.last_batch_path == "per-frame" and [z for z, _ in got] == list(range(0, n, 2))
    for z, t in got:
        _same(t, dec[ids[z:z + 2]], lab, 40, ids[z:z + 2])
    rd.close()
    rd = _open(os.path.join(FILES, "g11_u32d20.rc1"))
    with pytest.raises(NotImplementedError, match="16 bits"):
        rd.get_frame_bins(0, 1, np.zeros((int(rd._header["ny"]), int(rd._header["nx"])), np.uint16))
    rd.close()


def test_bins_on_part_files_with_one_shared_handle(hip):
    """G7's part files, whose ids have gaps: 'frame_ids' are the frames' ids, and the two readers share one FrameBins - one copy of the
    labels on the device - which stays usable after both are closed"""
    g = load_npz("g7_stream.npz")
    dec = _decoded_l1(g)
    rng = np.random.default_rng(7)
    lab = _file_labels(rng, dec.shape[1], dec.shape[2])
    fb = hip.FrameBins(dec.shape[2], dec.shape[1], lab, n_bins=48)
    for node in range(2):
        ids = g["ids_part%d" % node]
        rd = _open(os.path.join(FILES, "g7_stream.rc1_part%03d" % node), part=True)
        _same(rd.get_frame_bins(0, len(ids), fb), dec[ids], lab, 48, ids)
        _same(rd.get_frame_bins(2, 3, fb, n_bins=7), dec[ids[2:5]], lab, 48, ids[2:5])          # (the handle's n_bins holds)
        at = 0
        for z, t in rd.iter_frame_bins(batch=4, labels=fb):
            assert z == at
            _same(t, dec[ids[z:z + 4]], lab, 48, ids[z:z + 4])
            at += 4
        assert at >= len(ids)
        rd.close()
    assert fb.n_bins == 48 == hip.lib().rc_bins_count(fb.handle)
    fb.close()
    rd = _open(os.path.join(FILES, "g7_stream.rc1_part000"), part=True)
    with pytest.raises(ValueError, match="FrameBins of"):
        with hip.FrameBins(8, 4, np.zeros((4, 8), np.uint16)) as other:
            rd.get_frame_bins(0, 1, other)
    rd.close()


def test_bins_kernel_footprint():
    """k_expand_bins_b's descriptors in the built library (read the way test_gpu_corr.py::test_corr_kernel_footprint reads its kernel's; no
    GPU needed, but the file's other tests do): six instantiations - the tiers of 256, 1024 and 4096 bins, each with sums (level 1) and
    without -, no scratch, and the static LDS rc_bins.h states: a count per bin of the tier and, with sums, a sum - 12 or 4 bytes a bin,
    48 KiB at 4096 bins - plus at most the scan's 20 bytes rounded up to 32.  Sizes from the descriptor only."""
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
                if len(f) >= 8 and f[-1].endswith(".kd") and f[3] == "OBJECT" and "k_expand_bins_b" in f[-1]:
                    off = int(f[1], 16) - ro_addr + ro_off
                    found[f[-1]] = struct.unpack_from("<II", image, off)       # group_segment_fixed_size, private_segment_fixed_size
    seen = set()
    for name, (lds, scratch) in found.items():
        m = re.search(r"k_expand_bins_bILj(\d+)ELb([01])E", name)              # (the template arguments: the tier, whether sums are kept)
        assert m, name
        tier, sums = int(m.group(1)), m.group(2) == "1"
        seen.add((tier, sums))
        floor = bm.lds_bytes(tier, 1 if sums else 3)
        assert bm.tier(tier) == tier and scratch == 0 and floor <= lds <= floor + 32, "%s: %d B of LDS, %d B of scratch per lane" % (name, lds, scratch)
    assert seen == {(t, s) for t in (256, 1024, 4096) for s in (False, True)}, "k_expand_bins_b (256, 1024, 4096 bins; with and without sums) is not in the library"
    assert bm.lds_bytes(4096, 1) == 48 * 1024
