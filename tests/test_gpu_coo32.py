"""-m gpu: the COO output with uint32 values (rc_expand_frames_coo32 / _coo32_submit) against the triplet rows of the same batch, and the
public reader on files of more than 16 bits: such files come back as int32 rows | int32 columns | uint32 values from the device on every
batched route, and the frame-at-a-time calls are served from batches like a uint16 file's."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, load_npz, synth_frames

pytestmark = pytest.mark.gpu
FILES = os.path.join(GOLDEN, "files")
WG_PIXELS = 256 * 64          # pixels one workgroup of the expand kernels covers (rc_device.h: WG words of 64 bitmap bits)
EMIT_STAGE = 1024             # entries a workgroup stages in LDS; one with more writes directly (rc_expand.hip)


@pytest.fixture(scope="module")
def hip():
    from pyrecode_amd import _lib
    if _lib.device_count() == 0:
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    return _lib


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    oracle.lib()
    return oracle


def _synth_u32(seed, n, ny, nx, sparsity, d):
    """uint32 thresholds and frames whose residuals span all d bits: the first pixel of frame 0 carries 2^d - 1 (0xFFFFFFFF at d = 32)
    over a threshold of 0, the events' amplitudes are uniform up to 2^d - 1001; frame 2 is empty."""
    rng = np.random.default_rng(seed)
    top = (1 << d) - 1
    thr = rng.integers(0, 1000, (ny, nx)).astype(np.uint32)
    thr.flat[0] = 0
    frames = np.empty((n, ny, nx), np.uint32)
    for z in range(n):
        mask = rng.random((ny, nx)) < sparsity
        amp = rng.integers(1, top - 999, (ny, nx), dtype=np.int64)
        frames[z] = np.where(mask, thr + amp, thr // 2).astype(np.uint32)
    frames[0].flat[0] = top
    frames[2] = 0
    return thr, frames


def _batch(hip, frames, thr, d, level, mode, scheme, src_dtype):
    """the frames through the device writer -> (blob of the frames' data back to back, sizes uint32[n][3]) as rc_expand_frames takes them"""
    n, ny, nx = frames.shape
    ctx = hip.ReduceContext(nx, ny, d, level, mode, scheme, 1, 0, max_batch=n, src_dtype=src_dtype)
    ctx.set_threshold(thr)
    out, rec, md = ctx.reduce_compress_batch(frames, 0)
    ctx.close()
    nb = (ny * nx + 7) // 8
    sizes = np.zeros((n, 3), np.uint32)
    blobs = []
    for z in range(n):
        r = out[int(rec[z]):int(rec[z + 1])]
        if level == 1 and mode == 1:
            sizes[z] = md[z, :3]
            blobs.append(r[16:])
        elif level == 1:
            sizes[z] = (nb, md[z, 0], md[z, 0])
            blobs.append(r[8:])
        else:
            sizes[z, 0] = md[z, 0]
            blobs.append(r[8:])
    return np.ascontiguousarray(np.concatenate(blobs)), sizes


CODECS = [(0, 0), (1, 2), (1, 1)]      # (op_mode, scheme): reduce-only, LZ4, zstd
CASES = [(d, mode, scheme, 1) for d in (17, 20, 24, 31, 32) for mode, scheme in CODECS] + [(20, 1, 2, 3)]


@pytest.mark.parametrize("sparsity", [0.04, 0.12])
@pytest.mark.parametrize("d,mode,scheme,level", CASES)
def test_expand_frames_coo32_layout_equals_the_triplets(hip, orc, d, mode, scheme, level, sparsity):
    """rc_expand_frames_coo32 / _coo32_submit: the batch as int32 rows | int32 columns | uint32 values - entry for entry the triplet rows of
    rc_expand_frames (themselves the oracle's per frame), into pageable host memory, device memory and page-locked memory (the streaming
    form), with spare capacity, with none, and refused when one short.  70 x 300 frames are two workgroups each; at 4 % both stage their
    entries in LDS, at 12 % the first one holds more than EMIT_STAGE and writes directly.  Values with bit d-1 set (and 0xFFFFFFFF at
    d = 32) rule out a 16-bit or signed truncation."""
    import torch
    ny, nx, n = 70, 300, 5
    thr, frames = _synth_u32(41 + d, n, ny, nx, sparsity, d)
    binary = frames > thr
    first_wg = [int(binary[z].reshape(-1)[:WG_PIXELS].sum()) for z in range(n) if z != 2]
    assert all(c > EMIT_STAGE for c in first_wg) if sparsity > 0.1 else all(0 < c <= EMIT_STAGE for c in first_wg)
    blob, sizes = _batch(hip, frames, thr, d, level, mode, scheme, np.uint32)
    L = hip.lib()
    nnz = int(binary.sum())
    geom = (nx, ny, d, level, mode, scheme)
    want_prefix, want = np.zeros(n + 1, np.uint64), np.zeros((nnz, 3), np.uint64)
    hip.check(L.rc_expand_frames(*geom, hip.ptr(blob), hip.ptr(sizes), n, hip.ptr(want_prefix), hip.ptr(want), nnz))
    assert int(want_prefix[n]) == nnz and int(want_prefix[3]) == int(want_prefix[2])
    for z in range(n):                                                   # the reference of this test against the oracle's expand
        bitmap = orc.pack_binary_frame(binary[z])
        packed = orc.bit_pack32((frames[z][binary[z]] - thr[binary[z]]).astype(np.uint32), d) if level == 1 else None
        assert np.array_equal(want[int(want_prefix[z]):int(want_prefix[z + 1])], orc.unpack_frame_sparse(nx, ny, d, bitmap, packed, level)), z
    if level == 1:
        assert int(want[0, 2]) & ((1 << d) - 1) == (1 << d) - 1 and bool(((want[:, 2] >> np.uint64(d - 1)) & np.uint64(1)).any())
        assert d != 32 or bool((want[:, 2] == 0xFFFFFFFF).any())
        assert bool((want[:, 2] > 0xFFFF).any())
    else:
        assert bool((want[:, 2] == 1).all())

    def check(buf, cap, prefix):
        assert np.array_equal(prefix, want_prefix)
        rows, cols, vals = buf[:4 * cap].view(np.int32)[:nnz], buf[4 * cap:8 * cap].view(np.int32)[:nnz], buf[8 * cap:12 * cap].view(np.uint32)[:nnz]
        assert np.array_equal(rows, want[:, 0].astype(np.int32)) and np.array_equal(cols, want[:, 1].astype(np.int32))
        assert np.array_equal(vals.astype(np.uint64), want[:, 2])
    for cap in (nnz, nnz + 37):
        prefix = np.zeros(n + 1, np.uint64)
        host = np.full(12 * cap + 16, 0xA5, np.uint8)                    # pageable host memory, guard bytes behind
        hip.check(L.rc_expand_frames_coo32(*geom, hip.ptr(blob), hip.ptr(sizes), n, hip.ptr(prefix), hip.ptr(host), cap))
        check(host, cap, prefix)
        assert (host[12 * cap:] == 0xA5).all()
        dev = torch.full((12 * cap + 16,), 0x5A, dtype=torch.uint8, device="cuda")
        prefix[:] = 0
        hip.check(L.rc_expand_frames_coo32(*geom, hip.ptr(blob), hip.ptr(sizes), n, hip.ptr(prefix), dev.data_ptr(), cap))
        got = dev.cpu().numpy()
        check(got, cap, prefix)
        assert (got[12 * cap:] == 0x5A).all()
        pin = hip.PinnedBuffer(12 * cap + 16)
        pin.array[:] = 0x77
        hip.check(L.rc_expand_frames_coo32_submit(1, *geom, hip.ptr(blob), hip.ptr(sizes), n, pin._p, cap))
        prefix[:] = 0
        hip.check(L.rc_expand_frames_wait(1, hip.ptr(prefix)))
        check(pin.array, cap, prefix)
        assert (pin.array[12 * cap:] == 0x77).all()
        pin.close()
    prefix = np.zeros(n + 1, np.uint64)
    small = np.zeros(12 * nnz, np.uint8)
    assert L.rc_expand_frames_coo32(*geom, hip.ptr(blob), hip.ptr(sizes), n, hip.ptr(prefix), hip.ptr(small), nnz - 1) == hip.RC_ERR_OUT_TOO_SMALL
    assert np.array_equal(prefix, want_prefix)


def test_expand_frames_coo32_argument_limits(hip):
    """Values are uint32: bit_depth 33 is RC_ERR_BAD_ARG for both new calls (nothing left pending); rc_expand_frames_coo still refuses a
    20-bit file, synchronous and submitted."""
    ny, nx, n, d = 70, 300, 5, 20
    thr, frames = _synth_u32(7, n, ny, nx, 0.04, d)
    blob, sizes = _batch(hip, frames, thr, d, 1, 0, 0, np.uint32)
    L = hip.lib()
    cap = int((frames > thr).sum())
    prefix = np.zeros(n + 1, np.uint64)
    out = np.zeros(12 * cap, np.uint8)
    pin = hip.PinnedBuffer(12 * cap)
    src = (hip.ptr(blob), hip.ptr(sizes), n)
    assert L.rc_expand_frames_coo32(nx, ny, 33, 1, 0, 0, *src, hip.ptr(prefix), hip.ptr(out), cap) == hip.RC_ERR_BAD_ARG
    assert L.rc_expand_frames_coo32_submit(0, nx, ny, 33, 1, 0, 0, *src, pin._p, cap) == hip.RC_ERR_BAD_ARG
    assert L.rc_expand_frames_wait(0, hip.ptr(prefix)) == hip.RC_ERR_BAD_ARG                       # (nothing was submitted)
    assert L.rc_expand_frames_coo(nx, ny, d, 1, 0, 0, *src, hip.ptr(prefix), hip.ptr(out), cap) == hip.RC_ERR_BAD_ARG
    assert L.rc_expand_frames_coo_submit(0, nx, ny, d, 1, 0, 0, *src, pin._p, cap) == hip.RC_ERR_BAD_ARG
    hip.check(L.rc_expand_frames_coo32(nx, ny, d, 1, 0, 0, *src, hip.ptr(prefix), hip.ptr(out), cap))
    assert int(prefix[n]) == cap
    pin.close()


@pytest.mark.parametrize("mode,scheme", CODECS)
def test_expand_frames_coo32_widens_a_narrow_file(hip, orc, mode, scheme):
    """A 12-bit blob from uint16 sources through rc_expand_frames_coo32: rows, columns and prefix of rc_expand_frames_coo, its uint16 values as uint32."""
    ny, nx, n, d = 70, 300, 5, 12
    dark, frames = synth_frames(43, n, ny, nx, 0.04, d)
    frames[2] = 0
    thr = orc.threshold(dark, 0)
    blob, sizes = _batch(hip, frames, thr, d, 1, mode, scheme, np.uint16)
    L = hip.lib()
    nnz = int((frames > thr).sum())
    geom = (nx, ny, d, 1, mode, scheme)
    p16, p32 = np.zeros(n + 1, np.uint64), np.zeros(n + 1, np.uint64)
    b16, b32 = np.zeros(10 * nnz, np.uint8), np.zeros(12 * nnz, np.uint8)
    hip.check(L.rc_expand_frames_coo(*geom, hip.ptr(blob), hip.ptr(sizes), n, hip.ptr(p16), hip.ptr(b16), nnz))
    hip.check(L.rc_expand_frames_coo32(*geom, hip.ptr(blob), hip.ptr(sizes), n, hip.ptr(p32), hip.ptr(b32), nnz))
    assert int(p16[n]) == nnz and np.array_equal(p16, p32)
    assert np.array_equal(b16[:8 * nnz], b32[:8 * nnz])
    v16, v32 = b16[8 * nnz:].view(np.uint16), b32[8 * nnz:].view(np.uint32)
    assert bool(v16.any()) and np.array_equal(v16.astype(np.uint32), v32)


# ---- the public reader on files of more than 16 bits -------------------------------------------------------------------------------------
def _scatter(shape, batches):
    """(first frame, prefix, (rows, cols, vals)) batches -> dense uint64 frames; the values' dtype must be uint32"""
    img = np.zeros(shape, np.uint64)
    for a, pre, (rows, cols, vals) in batches:
        assert rows.dtype == np.int32 and cols.dtype == np.int32 and vals.dtype == np.uint32
        for i in range(len(pre) - 1):
            lo, hi = int(pre[i]), int(pre[i + 1])
            img[a + i, rows[lo:hi], cols[lo:hi]] = vals[lo:hi]
    return img


@pytest.mark.parametrize("tag", ["u32d17", "u32d20", "u32d24", "u32d32"])
def test_reader_returns_uint32_coo_for_the_references_wide_files(tag):
    """G11's merged files (zlib: the host-decoded route, one device expand per batch): get_frames_coo gives uint32 values that scatter to what
    the reference's reader returned, and a get_frame loop gives the same frames as uint32 matrices - served by the read-ahead from the
    third call on.  The streak rule (_readahead_frame): a call counts once the two before it were its predecessors, so calls 0 and 1 go
    frame by frame, call 2 fetches the batch of frames 2 .. nz-1 (nz - 2 >= 2 in every fixture) and every non-empty frame from there on
    is served: readahead_frames_served == nz - 2 (no fixture has an empty frame)."""
    from pyrecode_amd.recode_reader import ReCoDeReader
    g = load_npz("g11_%s.npz" % tag)
    want = g["decoded"]
    nz = want.shape[0]
    rd = ReCoDeReader(os.path.join(FILES, "g11_%s.rc1" % tag))
    rd.open(print_header=False)
    pre, arrays = rd.get_frames_coo(0, nz)
    assert rd.last_batch_path == "host-decode + device-expand"
    assert np.array_equal(_scatter(want.shape, [(0, pre, arrays)]), want)
    rd.close()
    rd = ReCoDeReader(os.path.join(FILES, "g11_%s.rc1" % tag))
    rd.open(print_header=False)
    for z in range(nz):
        m = rd.get_frame(z)[z]["data"]
        assert m.dtype == np.uint32 and m.data.dtype == np.uint32
        assert np.array_equal(np.asarray(m.todense()).astype(np.uint64), want[z]), "frame %d" % z
    assert nz >= 4 and bool((want.reshape(nz, -1) != 0).any(axis=1).all())
    assert rd.readahead_frames_served == nz - 2
    rd.close()


@pytest.mark.parametrize("scheme", [2, 1])
def test_reader_streams_uint32_coo_from_device_codec_files(scheme, tmp_path):
    """uint32 frames (20 bits) written with LZ4 / zstd on the device, two nodes, merged: iter_frames_coo and get_frames deliver uint32 COO
    arrays / matrices of where(frame > dark, frame - dark, 0) through the batched device path."""
    from pyrecode_amd.params import InputParams
    from pyrecode_amd.recode_reader import ReCoDeReader, merge_parts
    from pyrecode_amd.recode_writer import ReCoDeWriter
    g = load_npz("g11_u32d20.npz")
    rng = np.random.default_rng(5)
    ny, nx, nz = 96, 200, 7
    dark = rng.integers(1000, 70000, (ny, nx)).astype(np.uint32)
    frames = np.where(rng.random((nz, ny, nx)) < 0.05, dark + rng.integers(1, 900000, (nz, ny, nx)), dark // 2).astype(np.uint32)
    want = np.where(frames > dark, frames - dark, 0).astype(np.uint32)
    assert bool((want > 0xFFFF).any())
    cfg = dict(zip(g["cfg_keys"].tolist(), (int(v) for v in g["cfg_vals"])))
    cfg.update(num_rows=ny, num_cols=nx, num_frames=nz, num_threads=2, compression_scheme=scheme, calibration_threshold_epsilon=0)
    (tmp_path / "params.txt").write_text("".join("%s = %d\n" % kv for kv in cfg.items()))
    for node in range(2):
        ip = InputParams()
        ip.load(str(tmp_path / "params.txt"))
        w = ReCoDeWriter("u32", dark_data=dark, output_directory=str(tmp_path), input_params=ip, mode="batch", validation_frame_gap=-1,
                         node_id=node, batch_size=3)
        w.start()
        w.run(frames)
        w.close()
    merge_parts(str(tmp_path), "u32.rc1", 2)
    rd = ReCoDeReader(str(tmp_path / "u32.rc1"))
    rd.open(print_header=False)
    batches, paths = [], set()
    for a, pre, (rows, cols, vals) in rd.iter_frames_coo(batch=3):
        paths.add(rd.last_batch_path)
        batches.append((a, pre.copy(), (rows.copy(), cols.copy(), vals.copy())))     # (views of page-locked memory, valid until the next step)
    assert [b[0] for b in batches] == [0, 3, 6] and paths == {"device"}
    assert np.array_equal(_scatter(want.shape, batches), want)
    got = rd.get_frames(0, nz)
    assert rd.last_batch_path == "device" and sorted(got) == list(range(nz))
    for z in range(nz):
        m = got[z]["data"]
        assert m.dtype == np.uint32 and m.data.dtype == np.uint32 and np.array_equal(np.asarray(m.todense()), want[z])
    rd.close()
