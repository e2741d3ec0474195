"""-m gpu: frame traces.  The kernels of rc_trace.hip through the C ABI on stored streams built with numpy - every cell of the output against the
exact model (tests/trace_model.py), the cells around the output untouched -, the no-wrap refusal, the submit / wait form with a refused batch
in the middle, ReCoDeReader.get_frame_traces / iter_frame_traces on golden files and on files this library writes, against the decoded frames
reduced with numpy, and the kernel's footprint.  Every comparison is == on integers."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN, load_npz
from test_gpu_dense import _Out                                                   # an output between guard cells, prefilled with 0xA5
from test_gpu_frame_sums import _frames, _open, _stored_batch, _thr, _write, stack   # noqa: F401 - the frame kinds, stored batches, written files and the stack fixture of the summed views' tests
from test_trace_cpu import check_frame_call_arguments
from trace_model import trace_model, weight_bounds

pytestmark = pytest.mark.gpu
FILES = os.path.join(GOLDEN, "files")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCK_PIXELS = 256 * 64       # pixels one workgroup of the expand kernels owns
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1


@pytest.fixture(scope="module")
def hip():
    import torch  # noqa: F401 - before the library: one HIP runtime per process
    from pyrecode_amd import _lib
    if _lib.device_count() == 0:
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    return _lib


class _Trace:
    """rc_trace_create .. rc_trace_destroy, called as a C program would; planes: None, or int32[k][ny][nx] in host memory - or, with
    device=True, copied to the GPU first"""

    def __init__(self, hip, nx, ny, planes=None, device=False):
        self.hip, self.L = hip, hip.lib()
        self.k = 0 if planes is None else planes.shape[0]
        addr = None
        if planes is not None:
            planes = np.ascontiguousarray(planes, np.int32)
            addr = hip.ptr(planes)
            if device:
                import torch
                self.t = torch.from_numpy(planes).cuda()
                torch.cuda.synchronize()
                addr = self.t.data_ptr()
        st = C.c_int(0)
        self.h = self.L.rc_trace_create(nx, ny, self.k, addr, C.byref(st))
        assert self.h and st.value == hip.RC_OK, hip.last_error()
        assert self.L.rc_trace_columns(self.h) == 4 + self.k

    def bounds(self):
        return [int(self.L.rc_trace_weight_bound(self.h, m)) for m in range(self.k)]

    def frames(self, d, level, blob, sizes, n, out, prefix=None, slot=None, cells=None):
        args = (d, level, 0, 0, self.hip.ptr(blob), self.hip.ptr(sizes), n, out.ptr, out.cells if cells is None else cells)
        if slot is None:
            return self.L.rc_trace_frames(self.h, *args, self.hip.ptr(prefix))
        return self.L.rc_trace_frames_submit(self.h, slot, *args)

    def close(self):
        assert self.L.rc_trace_destroy(self.h) == self.hip.RC_OK


def _planes(rng, ny, nx, k):
    """k = 1: random full-range int32 with INT32_MIN and INT32_MAX in it.  k = 3: ones | the row index | the column index.  k = 16: those
    three, a 0/1 mask of one rectangle that straddles the first block boundary (the middle of a frame that has none), the full-range plane,
    zeros, and ten more random planes of 1 .. 31 bits, signed"""
    if k == 0:
        return None
    wild = rng.integers(INT32_MIN, INT32_MAX + 1, (ny, nx), dtype=np.int64).astype(np.int32)
    wild.reshape(-1)[rng.integers(0, ny * nx)] = INT32_MIN
    if ny * nx > 1:
        wild.reshape(-1)[(int(np.argmin(wild)) + 1) % (ny * nx)] = INT32_MAX
    if k == 1:
        return wild[None]
    rows, cols = np.indices((ny, nx)).astype(np.int32)
    basic = [np.ones((ny, nx), np.int32), rows, cols]
    if k == 3:
        return np.stack(basic)
    r = BLOCK_PIXELS // nx                                  # the row the first block ends in
    mask = np.zeros((ny, nx), np.int32)
    if ny * nx <= BLOCK_PIXELS:
        mask[ny // 4:3 * ny // 4 + 1, nx // 4:3 * nx // 4 + 1] = 1
    elif nx > BLOCK_PIXELS:
        mask[:, BLOCK_PIXELS - 400:BLOCK_PIXELS + 600] = 1
    else:
        mask[max(r - 1, 0):min(r + 1, ny - 1) + 1, nx // 4:3 * nx // 4 + 1] = 1
        assert mask.reshape(-1)[:BLOCK_PIXELS].any() and mask.reshape(-1)[BLOCK_PIXELS:].any()
    more = [rng.integers(-(1 << b), 1 << b, (ny, nx), dtype=np.int64).astype(np.int32) for b in (1, 2, 4, 7, 8, 12, 15, 16, 24, 31)]
    out = np.stack(basic + [mask, wild, np.zeros((ny, nx), np.int32)] + more)
    assert out.shape[0] == 16 == k
    return out


SHAPES = [(1, 1), (3, 21), (127, 130), (192, 256), (2, 20000)]
KINDS = [(1, 5), (1, 9), (1, 12), (1, 16), (3, 0), (2, 12)]      # (level, bit depth)


@pytest.mark.parametrize("k", [0, 1, 3, 16])
@pytest.mark.parametrize("level,d", KINDS)
@pytest.mark.parametrize("ny,nx", SHAPES)
def test_trace_kernel_on_stored_streams(hip, ny, nx, level, d, k):
    """rc_trace_frames, op_mode 0: batches of n = 1 (each frame kind alone: random, empty, every pixel at 2^d - 1, only the last pixel, random),
    3 (one frame group) and 11 (groups of 4 + 4 + 3), into host memory with a handle made from host planes and into device memory with a
    handle made from device planes.  The output sits between guard cells; it and they are prefilled with 0xA5: every cell is written, none
    beside them.  (2, 20000): rows longer than a block, so a word's pixels change row in the middle of a block."""
    assert (ny * nx - 1) // BLOCK_PIXELS + 1 == {1: 1, 63: 1, 16510: 2, 49152: 3, 40000: 3}[ny * nx]
    rng = np.random.default_rng(1000 * ny + 100 * k + 10 * d + level)
    planes = _planes(rng, ny, nx, k)
    handles = {"host": _Trace(hip, nx, ny, planes), "device": _Trace(hip, nx, ny, planes, device=True)}
    if k:
        assert handles["host"].bounds() == handles["device"].bounds() == weight_bounds(planes)
    for n, first in [(1, f) for f in range(5)] + [(3, 1), (11, 0)]:
        vals = _frames(rng, n, ny, nx, d, level, first)
        blob, sizes, _ = _stored_batch(vals, d, level, rng)
        want, counts = trace_model(blob, sizes, ny, nx, d, level, planes)
        v = vals.astype(np.int64)
        assert np.array_equal(want[:, 0], (vals != 0).reshape(n, -1).sum(1)) and np.array_equal(want[:, 1], v.reshape(n, -1).sum(1))
        assert np.array_equal(want[:, 2], (v * np.arange(ny)[None, :, None]).reshape(n, -1).sum(1))
        assert np.array_equal(want[:, 3], (v * np.arange(nx)[None, None, :]).reshape(n, -1).sum(1))
        if k >= 3:      # the planes of ones, of the row index and of the column index repeat columns 1, 2 and 3
            assert np.array_equal(want[:, 4:7], want[:, 1:4])
        if k == 16:
            assert not want[:, 9].any()                                     # the plane of zeros
        for where, tr in handles.items():
            out = _Out(hip, n * (4 + k), np.int64, where)
            prefix = np.zeros(n + 1, np.uint64)
            assert tr.frames(d, level, blob, sizes, n, out, prefix) == hip.RC_OK, hip.last_error()
            out.check(want)
            assert np.array_equal(prefix, counts)
    for tr in handles.values():
        tr.close()


def test_handles_from_host_and_device_planes_behave_alike(hip):
    """the same planes from host and from device memory, through the FrameTrace wrapper (numpy of a narrower dtype, a torch tensor on the GPU):
    the same bounds - numpy's -, the same traces, (ny, nx) accepted as one plane, nnz_prefix optional"""
    import torch
    ny, nx, d = 127, 130, 12
    rng = np.random.default_rng(3)
    planes = _planes(rng, ny, nx, 16)
    vals = _frames(rng, 5, ny, nx, d, 1)
    blob, sizes, _ = _stored_batch(vals, d, 1, rng)
    want, counts = trace_model(blob, sizes, ny, nx, d, 1, planes)
    geom = (nx, ny, d, 1, 0, 0)
    with hip.FrameTrace(nx, ny, planes) as a, hip.FrameTrace(nx, ny, torch.from_numpy(planes).cuda()) as b:
        assert a.weight_bounds() == b.weight_bounds() == weight_bounds(planes) == [int(np.abs(p.astype(np.int64)).max()) for p in planes]
        assert a.weight_bounds()[4] == 1 << 31 and a.columns == b.columns == 20
        for ft in (a, b):
            got, prefix = ft.frames(geom, blob, sizes, 5)
            assert got.dtype == np.int64 and np.array_equal(got, want) and np.array_equal(prefix, counts)
        out = np.zeros((5, 20), np.int64)
        assert a.frames_status(geom, blob, sizes, 5, out, out.size) == hip.RC_OK and np.array_equal(out, want)      # (nnz_prefix may be NULL)
    small = planes[12].astype(np.int16)            # 15 bits, signed
    with hip.FrameTrace(nx, ny, small) as a, hip.FrameTrace(nx, ny, torch.from_numpy(small.astype(np.int64)).cuda()) as b:
        assert a.k == b.k == 1 and a.weight_bounds() == b.weight_bounds() == weight_bounds(small[None])
        assert np.array_equal(a.frames(geom, blob, sizes, 5)[0], b.frames(geom, blob, sizes, 5)[0])
        assert np.array_equal(a.frames(geom, blob, sizes, 5)[0][:, 4], want[:, 4 + 12])
    with pytest.raises(ValueError, match="traced with a handle"):
        with hip.FrameTrace(21, 3) as ft:
            ft.frames(geom, blob, sizes, 5)


def test_handle_from_a_tensor_that_kernels_are_still_writing(hip):
    """The library reads device planes on a stream of its own, which is not ordered behind torch's: FrameTrace waits for the tensor's device
    before rc_trace_create copies it.  The weights here are the end of a chain of 300 elementwise passes over 32 Mi int64 values (about a
    hundred milliseconds of queued kernels) and the handle is made straight from them, with nothing in between: its bounds and its traces are those
    of the finished tensor.  GPU tensors whose values do not fit int32 raise ValueError, whatever their dtype."""
    import torch
    ny, nx, d, k = 127, 130, 12, 16
    rng = np.random.default_rng(13)
    vals = _frames(rng, 3, ny, nx, d, 1, first=2)          # every pixel set | only the last one | random: none is empty
    blob, sizes, _ = _stored_batch(vals, d, 1, rng)
    hip.FrameTrace(nx, ny, np.ones((k, ny, nx), np.int32)).close()      # (the library's first-use allocations are behind us: nothing in the create path waits by accident)
    big = torch.arange(1 << 25, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    for i in range(300):
        big = (big * 1103515245 + 12345 + i) % 2147483629
    weights = (big[:k * ny * nx].reshape(k, ny, nx) - (1 << 30)).to(torch.int32)      # (int32 as it is: no range check of FrameTrace's reads it first)
    ft = hip.FrameTrace(nx, ny, weights)                                 # (no synchronisation of the caller's)
    planes = weights.cpu().numpy().astype(np.int64)
    assert int(np.abs(planes).max()) > 1 << 29 and len(np.unique(planes[:, 0, 0])) == k
    want, counts = trace_model(blob, sizes, ny, nx, d, 1, planes)
    assert ft.weight_bounds() == weight_bounds(planes)
    got, prefix = ft.frames((nx, ny, d, 1, 0, 0), blob, sizes, 3)
    assert np.array_equal(got, want) and np.array_equal(prefix, counts) and want[:, 4:].all()
    ft.close()
    too_big = [torch.full((ny, nx), 1 << 31, dtype=torch.int64, device="cuda"), torch.full((ny, nx), -(1 << 31) - 1, dtype=torch.int64, device="cuda")]
    if hasattr(torch, "uint32"):
        too_big.append(torch.full((ny, nx), INT32_MIN, dtype=torch.int32, device="cuda").view(torch.uint32))      # the bits of 2^31 as uint32
    for w in too_big:
        with pytest.raises(ValueError, match="fit int32"):
            hip.FrameTrace(nx, ny, w)
    if hasattr(torch, "uint32"):
        with hip.FrameTrace(nx, ny, torch.full((ny, nx), 7, dtype=torch.int32, device="cuda").view(torch.uint32)) as ft:
            assert ft.weight_bounds() == [7]


def test_frame_call_arguments_are_checked_before_anything_is_queued(hip):
    check_frame_call_arguments(hip)


def test_no_silent_wrap(hip):
    """3 x 65535, 16 bits, one plane of INT32_MAX.  A frame with 10 set pixels of 65535 is accepted and exact (its value stream has room for
    10 fields: 10 * 65535 * (2^31 - 1) is far below 2^63); a frame with every pixel set is RC_ERR_OUT_TOO_SMALL before anything is queued, in
    both forms, and out keeps its fill (tests/test_trace_cpu.py checks that the two lie on either side of the bound)."""
    ny, nx, d = 3, 65535, 16
    rng = np.random.default_rng(11)
    planes = np.full((1, ny, nx), INT32_MAX, np.int32)
    tr = _Trace(hip, nx, ny, planes)
    assert tr.bounds() == [INT32_MAX]
    vals = np.zeros((1, ny, nx), np.uint32)
    vals.reshape(-1)[np.append(rng.choice(ny * nx - 1, 9, replace=False), ny * nx - 1)] = 65535      # (the last pixel among them)
    blob, sizes, _ = _stored_batch(vals, d, 1, rng)
    assert sizes[0, 2] == 20
    want, counts = trace_model(blob, sizes, ny, nx, d, 1, planes)
    assert want[0, 0] == 10 and want[0, 1] == 655350 and want[0, 4] == 655350 * INT32_MAX
    for where in ("host", "device"):
        out = _Out(hip, 5, np.int64, where)
        prefix = np.zeros(2, np.uint64)
        assert tr.frames(d, 1, blob, sizes, 1, out, prefix) == hip.RC_OK, hip.last_error()
        out.check(want)
        assert np.array_equal(prefix, counts)
    full, fsizes, _ = _stored_batch(np.full((1, ny, nx), 65535, np.uint32), d, 1, rng)
    assert fsizes[0, 2] == 2 * 196605
    for where in ("host", "device"):
        out = _Out(hip, 5, np.int64, where)
        assert tr.frames(d, 1, full, fsizes, 1, out, np.zeros(2, np.uint64)) == hip.RC_ERR_OUT_TOO_SMALL and "2^63" in hip.last_error()
        assert tr.frames(d, 1, full, fsizes, 1, out, slot=1) == hip.RC_ERR_OUT_TOO_SMALL
        out.check(None)
    assert tr.L.rc_expand_frames_wait(1, hip.ptr(np.zeros(4, np.uint64))) == hip.RC_ERR_BAD_ARG      # (nothing was queued)
    tr.close()


def test_submit_wait_with_a_rejected_batch_in_the_middle(hip):
    """Six batches alternating between the two slots on ONE handle, into page-locked (even batches) and device (odd batches) outputs.  Batch 3
    declares one frame's value stream two bytes shorter than its set pixels need - the refusal k_expand_bases makes on the device -:
    rc_expand_frames_wait answers RC_ERR_CORRUPT for it and its out keeps its fill; the other five are exact.  A busy slot is RC_ERR_BAD_ARG."""
    ny, nx, d, n, k = 127, 130, 12, 5, 3
    rng = np.random.default_rng(9)
    planes = _planes(rng, ny, nx, 16)[3:6]          # the mask, the full-range plane, zeros
    tr = _Trace(hip, nx, ny, planes, device=True)
    L = tr.L
    batches = []
    for i in range(6):
        vals = _frames(rng, n, ny, nx, d, 1, first=i)
        blob, sizes, where = _stored_batch(vals, d, 1, rng)
        want, counts = trace_model(blob, sizes, ny, nx, d, 1, planes)
        if i == 3:
            z = next(z for z in range(n) if where[z][1] > 8)
            at, size = where[z]
            blob = np.ascontiguousarray(np.concatenate([blob[:at + size - 2], blob[at + size:]]))
            sizes[z, 1] = sizes[z, 2] = size - 2
            want = None
        pin = hip.PinnedBuffer(blob.size + 64)          # (a submitted batch's bytes stay where they are until the wait)
        pin.array[:blob.size] = blob
        batches.append((pin, sizes, want, counts, _Out(hip, n * (4 + k), np.int64, "device" if i & 1 else "pinned")))
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
        assert tr.frames(d, 1, pin.array, sizes, n, out, slot=i & 1) == hip.RC_OK, hip.last_error()
    assert tr.frames(d, 1, batches[0][0].array, batches[0][1], n, batches[0][4], slot=0) == hip.RC_ERR_BAD_ARG and "submitted batch" in hip.last_error()
    pageable = np.zeros(n * (4 + k), np.int64)
    wait(4)
    wait(5)
    assert verdicts == [hip.RC_OK] * 3 + [hip.RC_ERR_CORRUPT] + [hip.RC_OK] * 2
    args = (d, 1, 0, 0, hip.ptr(batches[0][0].array), hip.ptr(batches[0][1]), n, hip.ptr(pageable), pageable.size)
    assert L.rc_trace_frames_submit(tr.h, 0, *args) == hip.RC_ERR_BAD_ARG and "page-locked" in hip.last_error()      # (pageable memory is not taken)
    assert L.rc_expand_frames_wait(0, hip.ptr(np.zeros(n + 1, np.uint64))) == hip.RC_ERR_BAD_ARG and not pageable.any()
    tr.close()
    for pin, _, _, _, out in batches:
        out.close()
        pin.close()


# ---- the reader ------------------------------------------------------------------------------------------------------------------------
def _reduce(decoded, planes=None):
    """what get_frame_traces returns for these dense frames (0 = not set), with numpy: values of 16 bits at most, a few thousand pixels,
    planes of 20 bits at most - every sum is exact in int64"""
    v = np.asarray(decoded).astype(np.int64)
    n, ny, nx = v.shape
    planes = np.zeros((0, ny, nx), np.int64) if planes is None else np.asarray(planes).reshape(-1, ny, nx).astype(np.int64)
    assert int(np.abs(planes).max(initial=0)) < 1 << 20 and int(v.max(initial=0)) < 1 << 16 and ny * nx < 1 << 20
    return {"count": (v != 0).reshape(n, -1).sum(1), "sum": v.reshape(n, -1).sum(1),
            "sum_row": (v * np.arange(ny)[None, :, None]).reshape(n, -1).sum(1), "sum_col": (v * np.arange(nx)[None, None, :]).reshape(n, -1).sum(1),
            "weighted": np.einsum("fyx,myx->fm", v, planes)}


def _same(got, want, ids):
    assert sorted(got) == ["count", "frame_ids", "sum", "sum_col", "sum_row", "weighted"]
    for key in ("count", "sum", "sum_row", "sum_col", "weighted"):
        assert got[key].dtype == np.int64 and got[key].shape == want[key].shape and np.array_equal(got[key], want[key]), key
    assert got["frame_ids"].tolist() == [int(i) for i in ids]


def _cut(want, a, b):
    return {key: val[a:b] for key, val in want.items()}


def _masks(rng, ny, nx, k=2):
    """a 0/1 mask of the frame's middle and a plane of small signed weights (and k - 2 more of those)"""
    mask = np.zeros((ny, nx), np.int32)
    mask[ny // 4:3 * ny // 4, nx // 4:3 * nx // 4] = 1
    return np.stack([mask] + [rng.integers(-1000, 1001, (ny, nx)).astype(np.int32) for _ in range(k - 1)])


def test_traces_on_golden_files(hip):
    from pyrecode_amd.reader_batched import centre_of_mass
    rng = np.random.default_rng(5)
    g = load_npz("g3_l1z12.npz")
    dec = g["decoded"]
    nz, ny, nx = dec.shape
    planes = _masks(rng, ny, nx, 3)
    want = _reduce(dec, planes)
    assert want["count"].any() and want["weighted"].any()
    rd = _open(os.path.join(FILES, "g3_l1z12.rc1"))
    _same(rd.get_frame_traces(0, nz, planes), want, range(nz))
    assert rd.last_batch_path == "host-decode + device-expand"          # stock zlib: refused by the device inflate, decoded on the host, reduced on the device
    _same(rd.get_frame_traces(2, 5), _cut(_reduce(dec), 2, 7), range(2, 7))
    _same(rd.get_frame_traces(1, 3, planes[1]), _cut(_reduce(dec, planes[1]), 1, 4), range(1, 4))          # (one plane as (ny, nx))
    seen = [(z, t) for z, t in rd.iter_frame_traces(batch=3, weights=planes)]
    assert [z for z, _ in seen] == list(range(0, nz, 3))
    for z, t in seen:
        _same(t, _cut(want, z, z + 3), range(z, min(z + 3, nz)))
    row, col = centre_of_mass(rd.get_frame_traces(0, nz))
    assert want["sum"].all() and np.array_equal(row, want["sum_row"] / want["sum"]) and np.array_equal(col, want["sum_col"] / want["sum"])
    assert list(rd.iter_frame_traces(0, 0)) == []
    with pytest.raises(ValueError):
        rd.get_frame_traces(0, nz + 1)
    with pytest.raises(ValueError):
        rd.get_frame_traces(0, 2, np.ones((ny, nx + 1), np.int32))
    with pytest.raises(ValueError):
        rd.get_frame_traces(0, 2, np.ones((ny, nx), np.float32))
    rd.close()
    g = load_npz("g3_l3z.npz")
    dec = (g["frames"] > _thr(g)).astype(np.int64)
    rd = _open(os.path.join(FILES, "g3_l3z.rc3"))
    planes = _masks(rng, dec.shape[1], dec.shape[2])
    got = rd.get_frame_traces(0, dec.shape[0], planes)
    _same(got, _reduce(dec, planes), range(dec.shape[0]))
    assert np.array_equal(got["count"], got["sum"]) and got["count"].any()
    rd.close()
    rd = _open(os.path.join(FILES, "g11_u32d20.rc1"))
    with pytest.raises(NotImplementedError, match="16 bits"):
        rd.get_frame_traces(0, 1)
    with pytest.raises(NotImplementedError, match="16 bits"):
        next(rd.iter_frame_traces())
    rd.close()


def _decoded_l1(g):
    thr = _thr(g)
    return np.where(g["frames"] > thr, g["frames"].astype(np.int64) - thr, 0)


def test_traces_on_part_files_with_one_shared_handle(hip):
    """G7's part files, whose ids have gaps: 'frame_ids' are the frames' ids, and the two readers share one FrameTrace - one copy of the
    weights on the device - which stays usable after both are closed"""
    g = load_npz("g7_stream.npz")
    dec = _decoded_l1(g)
    rng = np.random.default_rng(7)
    planes = _masks(rng, dec.shape[1], dec.shape[2], 4)
    ft = hip.FrameTrace(dec.shape[2], dec.shape[1], planes)
    for node in range(2):
        ids = g["ids_part%d" % node]
        want = _reduce(dec[ids], planes)
        rd = _open(os.path.join(FILES, "g7_stream.rc1_part%03d" % node), part=True)
        _same(rd.get_frame_traces(0, len(ids), ft), want, ids)
        _same(rd.get_frame_traces(2, 3, ft), _cut(want, 2, 5), ids[2:5])
        at = 0
        for z, t in rd.iter_frame_traces(batch=4, weights=ft):
            assert z == at
            _same(t, _cut(want, z, z + 4), ids[z:z + 4])
            at += 4
        assert at >= len(ids) and rd.part_frame_ids.tolist() == ids.tolist()
        rd.close()
    assert ft.weight_bounds() == weight_bounds(planes)
    ft.close()
    rd = _open(os.path.join(FILES, "g7_stream.rc1_part000"), part=True)
    with pytest.raises(ValueError, match="FrameTrace of"):
        with hip.FrameTrace(8, 4) as other:
            rd.get_frame_traces(0, 1, other)
    rd.close()


def test_traces_on_host_only_schemes(hip):
    """bz2 (the reference's file): the stock decoder on the thread pool, then one device call on the stored pieces; without a stock decoder
    for the batch, frame by frame, restated as stored frames"""
    g = load_npz("g9_l1bz2.npz")
    dec = _decoded_l1(g)
    rng = np.random.default_rng(8)
    planes = _masks(rng, dec.shape[1], dec.shape[2])
    seen = []
    for node in range(2):
        rd = _open(os.path.join(FILES, "g9_l1bz2.rc1_part%03d" % node), part=True)
        n = rd._batch_frames()
        ids = rd.part_frame_ids
        want = _reduce(dec[ids], planes)
        _same(rd.get_frame_traces(0, n, planes), want, ids)
        assert rd.last_batch_path == "host-decode + device-expand"
        rd._host_decode_batch = lambda *a: None                   # (as when no stock decoder takes the batch)
        _same(rd.get_frame_traces(0, n, planes), want, ids)
        assert rd.last_batch_path == "per-frame"
        got = list(rd.iter_frame_traces(batch=2, weights=planes))
        assert rd.last_batch_path == "per-frame" and [z for z, _ in got] == list(range(0, n, 2))
        for z, t in got:
            _same(t, _cut(want, z, z + 2), ids[z:z + 2])
        seen += ids.tolist()
        rd.close()
    assert sorted(seen) == list(range(dec.shape[0])) and dec.any()


@pytest.mark.parametrize("level,scheme,dz,path", [(1, 2, False, "device"), (1, 1, False, "device"), (1, 8, False, "device"),
                                                  (1, 0, True, "device-inflate"), (2, 2, False, "device"), (3, 2, False, "device")])
def test_traces_on_this_librarys_files(hip, stack, tmp_path, level, scheme, dz, path):
    """LZ4, zstd, blosc-LZ4 and the device's own zlib streams at level 1, LZ4 at levels 2 and 3: every batch - 8, 8 and a ragged 4 - is decoded
    and reduced on the device; frame 7 is empty: a row of zeros.  A generator that is stopped early leaves the slots reusable."""
    dark, frames = stack
    dec = np.where(frames > dark, frames.astype(np.int64) - dark, 0) if level == 1 else (frames > dark).astype(np.int64)
    rng = np.random.default_rng(level + scheme)
    planes = _masks(rng, 127, 130, 5)
    want = _reduce(dec, planes)
    extra = dict(l2_statistics=2) if level == 2 else {}
    rd = _open(_write(tmp_path, dark, frames, level, scheme, dz, **extra))
    paths = set()
    keep = rd._note_batch_end
    rd._note_batch_end = lambda z: (paths.add(rd.last_batch_path), keep(z))[1]
    got = list(rd.iter_frame_traces(batch=8, weights=planes))
    assert paths == {path} and [(z, len(t["count"])) for z, t in got] == [(0, 8), (8, 8), (16, 4)]
    for z, t in got:
        _same(t, _cut(want, z, z + 8), range(z, min(z + 8, 20)))
    assert not any(got[0][1][key][7].any() for key in ("count", "sum", "sum_row", "sum_col", "weighted")) and got[0][1]["count"][6] > 0
    _same(rd.get_frame_traces(0, 20, planes), want, range(20))
    assert rd.last_batch_path == path
    it = rd.iter_frame_traces(3, 12, batch=2)
    z, t = next(it)
    assert z == 3
    _same(t, _cut(_reduce(dec), 3, 5), range(3, 5))
    it.close()                                   # (the next batch is queued: waited for, the handle freed)
    _same(rd.get_frame_traces(3, 12, planes[0]), _cut(_reduce(dec, planes[0]), 3, 15), range(3, 15))
    assert [z for z, _ in rd.iter_frame_traces(batch=8)] == [0, 8, 16]
    rd.close()


def test_two_readers_share_the_slots_on_the_sum_familys_ladder(hip, tmp_path, monkeypatch):
    """The two streaming slots belong to the process: two readers of one small LZ4 file (6 frames of 48 x 64, 12 bits, level 1) advanced in
    turn - dense batches of two frames on one, traces on the other - find each other's batches on the slots, and the batch that finds its
    slot taken goes through the synchronous call of the same ladder: every batch equals a third reader's get_frames_dense /
    get_frame_traces, and every one was decoded on the device.  Then two sum_frames into ONE handle while an iterator of the first reader
    still holds a slot: twice a single reader's sum.  Six frames in batches of two is the smallest run in which both slots are held
    when the other reader arrives."""
    from pyrecode_amd import reader_batched as rb
    rng = np.random.default_rng(33)
    ny, nx, nz = 48, 64, 6
    dark = rng.integers(80, 121, (ny, nx)).astype(np.uint16)
    frames = np.where(rng.random((nz, ny, nx)) < 0.05, dark + rng.integers(1, 3900, (nz, ny, nx)), dark // 2).astype(np.uint16)
    path = _write(tmp_path, dark, frames, 1, 2)
    a, b, ref = _open(path), _open(path), _open(path)
    planes = _masks(rng, ny, nx)
    taken, asked = [], rb._slot_taken
    monkeypatch.setattr(rb, "_slot_taken", lambda st: (taken.append(asked(st)), taken[-1])[1])      # (a count of the submits that found a slot held)
    dense_it, trace_it = a.iter_frames_dense(batch=2), b.iter_frame_traces(batch=2, weights=planes)
    dense, traces = [], []
    for _ in range(3):
        z, arr = next(dense_it)
        dense.append((z, arr.copy()))
        assert a.last_batch_path == "device"
        traces.append(next(trace_it))
        assert b.last_batch_path == "device"
    assert next(dense_it, None) is None and next(trace_it, None) is None and [z for z, _ in dense] == [z for z, _ in traces] == [0, 2, 4]
    assert any(taken), "no batch found its slot taken: the synchronous rung was not walked"
    for (z, arr), (_, t) in zip(dense, traces):
        want = ref.get_frames_dense(z, 2)
        assert ref.last_batch_path == "device" and arr.dtype == want.dtype and np.array_equal(arr, want) and want.any()
        _same(t, ref.get_frame_traces(z, 2, planes), range(z, z + 2))
    # the summed views: both readers add into one handle while a dense iterator of a third still holds slot 1
    want = ref.sum_frames(batch=2)
    del taken[:]
    held = ref.iter_frames_dense(batch=2)
    next(held)
    fs = hip.FrameSum(nx, ny)
    for rd in (a, b):
        assert rd.sum_frames(batch=2, into=fs) == nz and rd.last_batch_path == "device"
    held.close()
    assert any(taken) and np.array_equal(fs.fetch().astype(np.uint64), 2 * want) and want.any()
    fs.close()
    for rd in (a, b, ref):
        rd.close()


def test_trace_kernel_footprint():
    """k_expand_trace_b's descriptors in the built library (read the way test_gpu_frame_sums.py::test_sum_kernel_footprint reads its kernel's;
    no GPU needed, but the file's other tests do): both instantiations - with and without weights -, no scratch, and at most 81 920 B of static
    LDS - two workgroups share a CU's 160 KiB.  Sizes from the descriptor only."""
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
                if len(f) >= 8 and f[-1].endswith(".kd") and f[3] == "OBJECT" and "k_expand_trace_b" in f[-1]:
                    off = int(f[1], 16) - ro_addr + ro_off
                    found[f[-1]] = struct.unpack_from("<II", image, off)       # group_segment_fixed_size, private_segment_fixed_size
    assert len(found) == 2, "k_expand_trace_b (with and without weights) is not in the library"
    for name, (lds, scratch) in found.items():
        assert scratch == 0 and 0 < lds <= 81920, "%s: %d B of LDS, %d B of scratch per lane" % (name, lds, scratch)
