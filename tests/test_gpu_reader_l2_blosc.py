"""The batched device reader on blosc-LZ4 streams (compression_scheme 8) and on reduction level 2: rc_expand_frames & co. with scheme 8 and
with level 2, rc_expand_frames_l2 / _l2_submit, and the reader methods on top (get_frames_l2, iter_frames_l2, device_blosc=True).
Expectations come from the oracle (binarize_l1 / pack_binary_frame), from scipy.ndimage.label with the 3 x 3 structure (the rule
test_gpu_parity._l2_expected states) and, at file level, from the frame-at-a-time path (get_frame with the read-ahead off)."""
import struct

import numpy as np
import pytest

from conftest import load_npz, synth_frames
from test_gpu_api import _write_parts
from test_gpu_parity import _l2_expected

pytestmark = pytest.mark.gpu


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


def _records(hip, frames, thr, d, level, mode, scheme, stat=None):
    """the frames through a ReduceContext -> (blob of the frames' data back to back, sizes uint32[n][3], the records)"""
    n, ny, nx = frames.shape
    ctx = hip.ReduceContext(nx, ny, d, level, mode, scheme, 1, 0, max_batch=n)
    ctx.set_threshold(thr)
    if stat is not None:
        ctx.set_l2_statistics(stat)
    out, rec, md = ctx.reduce_compress_batch(frames, 0)
    ctx.close()
    nb = (ny * nx + 7) // 8
    sizes, blobs = np.zeros((n, 3), np.uint32), []
    for z in range(n):
        r = out[int(rec[z]):int(rec[z + 1])]
        if mode == 1 and level in (1, 2):
            sizes[z] = md[z, :3]
            blobs.append(r[16:])
        elif mode == 1:
            sizes[z, 0] = md[z, 0]
            blobs.append(r[8:])
        else:
            sizes[z] = (nb, md[z, 0], md[z, 0])
            blobs.append(r[8:])
        assert blobs[-1].size == int(sizes[z, 0]) + (int(sizes[z, 1]) if level != 3 else 0)
    return np.ascontiguousarray(np.concatenate(blobs)), sizes, blobs


def _expected_l1(orc, frames, thr, level):
    """row-major (rows, columns, values) of every frame and their prefix, from the oracle"""
    rows, cols, vals, prefix = [], [], [], [0]
    for f in frames:
        binary, pix = orc.binarize_l1(f, thr)
        binary = np.asarray(binary).reshape(f.shape).astype(bool)
        r, c = np.nonzero(binary)
        rows.append(r.astype(np.int64))
        cols.append(c.astype(np.int64))
        vals.append(np.asarray(pix, np.int64) if level == 1 else np.ones(r.size, np.int64))
        prefix.append(prefix[-1] + r.size)
    return np.concatenate(rows), np.concatenate(cols), np.concatenate(vals), np.array(prefix, np.uint64)


def _blosc_batches(ny, nx, d, level, seed):
    """two batches of three frames: [0.1 % sparse, empty, 5 % sparse] and [uniformly random at ~50 % (blocks that do not compress), 5 % sparse,
    all set at level 3 / 0.1 % sparse at level 1]"""
    dark, a = synth_frames(seed, 3, ny, nx, 0.001, d)
    _, five = synth_frames(seed + 1, 2, ny, nx, 0.05, d)
    rng = np.random.default_rng(seed + 2)
    a[1] = 0
    a[2] = five[0]
    b = a.copy()
    b[0] = np.where(rng.random((ny, nx)) < 0.5, dark + 7, 0).astype(np.uint16)
    b[1] = five[1]
    if level == 3:
        b[2] = (dark + 9).astype(np.uint16)
    else:
        b[2] = a[0]
    return dark, a, b


@pytest.mark.parametrize("level,d", [(1, 12), (1, 16), (3, 12), (3, 16)])
@pytest.mark.parametrize("ny,nx", [(16, 16), (50, 70), (72, 136), (64, 512)])   # map bytes: 32 (nothing shuffled), 438 (one partial tile, tail
def test_expand_frames_decodes_blosc_records(hip, orc, ny, nx, level, d):     # not a multiple of 8), 1224 (2 tiles + 25 elements), 4096 (8 tiles)
    """Records ReduceContext(scheme 8) wrote, through rc_expand_frames and rc_expand_frames_coo, and once through _submit / _wait with a
    batch on each slot: rows, columns and values equal the oracle's row-major list."""
    L = hip.lib()
    dark, fa, fb = _blosc_batches(ny, nx, d, level, 300 + ny + d)
    thr = orc.threshold(dark, 0)
    geom = (nx, ny, d, level, 1, 8)
    jobs = []
    for frames in (fa, fb):
        blob, sizes, blobs = _records(hip, frames, thr, d, level, 1, 8)
        jobs.append((blob, sizes, _expected_l1(orc, frames, thr, level)))
        if frames is fb and ny * nx // 8 >= 512:      # the random frame's tiles do not compress: stored blocks (csize == 512) are among the inputs
            chunk = blobs[0].tobytes()
            nblocks = -(-(ny * nx // 8) // 512)
            bstarts = struct.unpack_from("<%di" % nblocks, chunk, 16)
            assert any(struct.unpack_from("<i", chunk, s)[0] == 512 for s in bstarts)
    n = 3
    for blob, sizes, (rows, cols, vals, want_prefix) in jobs:
        nnz = int(want_prefix[n])
        prefix = np.zeros(n + 1, np.uint64)
        hip.check(L.rc_expand_frames(*geom, hip.ptr(blob), hip.ptr(sizes), n, hip.ptr(prefix), None, 0))      # the counting call
        assert np.array_equal(prefix, want_prefix)
        cap = nnz + 5
        trip = np.full((cap, 3), 0xA5A5, np.uint64)
        prefix[:] = 0
        hip.check(L.rc_expand_frames(*geom, hip.ptr(blob), hip.ptr(sizes), n, hip.ptr(prefix), hip.ptr(trip), cap))
        assert np.array_equal(prefix, want_prefix)
        assert np.array_equal(trip[:nnz, 0], rows.astype(np.uint64)) and np.array_equal(trip[:nnz, 1], cols.astype(np.uint64))
        assert np.array_equal(trip[:nnz, 2], vals.astype(np.uint64))
        assert (trip[nnz:] == 0xA5A5).all()
        coo = np.full(10 * cap + 16, 0xA5, np.uint8)
        prefix[:] = 0
        hip.check(L.rc_expand_frames_coo(*geom, hip.ptr(blob), hip.ptr(sizes), n, hip.ptr(prefix), hip.ptr(coo), cap))
        assert np.array_equal(prefix, want_prefix)
        assert np.array_equal(coo[:4 * cap].view(np.int32)[:nnz], rows.astype(np.int32))
        assert np.array_equal(coo[4 * cap:8 * cap].view(np.int32)[:nnz], cols.astype(np.int32))
        assert np.array_equal(coo[8 * cap:10 * cap].view(np.uint16)[:nnz], vals.astype(np.uint16))
        assert (coo[10 * cap:] == 0xA5).all()
    # both slots in flight: batch a on slot 0 (triplets), batch b on slot 1 (COO), page-locked outputs
    pins = []
    for slot, (blob, sizes, (rows, cols, vals, want_prefix)) in enumerate(jobs):
        cap = max(int(want_prefix[n]), 1)
        src = hip.PinnedBuffer(blob.size)
        src.array[:] = blob
        dst = hip.PinnedBuffer((10 if slot else 24) * cap + 16)
        dst.array[:] = 0x77
        fn = L.rc_expand_frames_coo_submit if slot else L.rc_expand_frames_submit
        hip.check(fn(slot, *geom, hip.ptr(src.array), hip.ptr(sizes), n, dst._p, cap))
        pins.append((src, dst, cap))
    for slot, (blob, sizes, (rows, cols, vals, want_prefix)) in enumerate(jobs):
        src, dst, cap = pins[slot]
        nnz = int(want_prefix[n])
        prefix = np.zeros(n + 1, np.uint64)
        hip.check(L.rc_expand_frames_wait(slot, hip.ptr(prefix)))
        assert np.array_equal(prefix, want_prefix)
        if slot:
            assert np.array_equal(dst.array[:4 * cap].view(np.int32)[:nnz], rows.astype(np.int32))
            assert np.array_equal(dst.array[4 * cap:8 * cap].view(np.int32)[:nnz], cols.astype(np.int32))
            assert np.array_equal(dst.array[8 * cap:10 * cap].view(np.uint16)[:nnz], vals.astype(np.uint16))
            assert (dst.array[10 * cap:] == 0x77).all()
        else:
            got = dst.array[:24 * cap].view(np.uint64).reshape(cap, 3)[:nnz]
            assert np.array_equal(got[:, 0], rows.astype(np.uint64)) and np.array_equal(got[:, 1], cols.astype(np.uint64))
            assert np.array_equal(got[:, 2], vals.astype(np.uint64))
            assert (dst.array[24 * cap:] == 0x77).all()
        src.close()
        dst.close()


def _l2_frames(ny, nx, d, seed):
    """three frames: clustered events (components that cross tile and row boundaries), an empty frame, and one frame that is a single
    component whose sum wraps modulo 2^d"""
    dark, frames = synth_frames(seed, 3, ny, nx, 0.02, d)
    rng = np.random.default_rng(seed + 1)
    seeds = frames[0] > dark
    grown = seeds.copy()
    grown[:, 1:] |= seeds[:, :-1] & (rng.random((ny, nx - 1)) < 0.7)        # to the right: across 64-pixel words and tile ends
    grown[1:, :] |= seeds[:-1, :] & (rng.random((ny - 1, nx)) < 0.7)        # below: across rows
    grown[1:, 1:] |= seeds[:-1, :-1] & (rng.random((ny - 1, nx - 1)) < 0.5)  # diagonal: 8-connectivity
    amp = rng.integers(2, 1 << (d - 2), (ny, nx))
    frames[0] = np.where(grown, dark + amp, 0).astype(np.uint16)
    frames[1] = 0
    frames[2] = (dark + 40).astype(np.uint16)
    return dark, frames


@pytest.mark.parametrize("stat", [1, 2])                                      # max, sum
@pytest.mark.parametrize("mode,scheme", [(0, 0), (1, 2), (1, 1), (1, 8)])
@pytest.mark.parametrize("ny,nx,d", [(72, 136, 12), (50, 70, 8)])
def test_expand_frames_l2_gives_pixels_and_statistics(hip, orc, ny, nx, d, mode, scheme, stat):
    """Level-2 records through rc_expand_frames_l2 (rows, columns, statistics against scipy's labelling), through rc_expand_frames with
    reduction_level 2 (the same pixels with value 1; its counting call), through _l2_submit / _wait; depths outside 8..16 and a statistics
    buffer one entry short are refused, the latter with a valid prefix."""
    L = hip.lib()
    n = 3
    dark, frames = _l2_frames(ny, nx, d, 50 + ny + stat)
    thr = orc.threshold(dark, 1)
    rows, cols, stats, want_prefix, sp = [], [], [], [0], [0]
    for f in frames:
        binary, vals = _l2_expected(f, thr, stat, d)
        r, c = np.nonzero(binary)
        rows.append(r.astype(np.int32))
        cols.append(c.astype(np.int32))
        stats.append(vals.astype(np.uint16))
        want_prefix.append(want_prefix[-1] + r.size)
        sp.append(sp[-1] + vals.size)
    rows, cols, stats = np.concatenate(rows), np.concatenate(cols), np.concatenate(stats)
    want_prefix = np.array(want_prefix, np.uint64)
    nnz, ns = int(want_prefix[n]), sp[n]
    assert sp[2] == sp[1] and sp[3] == sp[2] + 1 and nnz > ny * nx          # an empty frame, then ONE component
    if stat == 2:
        assert int(frames[2].astype(np.int64).sum()) >= 1 << d             # ... whose sum wraps
    blob, sizes, _ = _records(hip, frames, thr, d, 2, mode, scheme, stat)
    assert [int(8 * s // d) for s in sizes[:, 2]] == [sp[i + 1] - sp[i] for i in range(n)]
    src = (mode, scheme, hip.ptr(blob), hip.ptr(sizes), n)
    prefix = np.zeros(n + 1, np.uint64)
    hip.check(L.rc_expand_frames(nx, ny, d, 2, *src, hip.ptr(prefix), None, 0))
    assert np.array_equal(prefix, want_prefix)
    trip = np.zeros((nnz, 3), np.uint64)
    prefix[:] = 0
    hip.check(L.rc_expand_frames(nx, ny, d, 2, *src, hip.ptr(prefix), hip.ptr(trip), nnz))
    assert np.array_equal(prefix, want_prefix)
    assert np.array_equal(trip[:, 0], rows.astype(np.uint64)) and np.array_equal(trip[:, 1], cols.astype(np.uint64)) and (trip[:, 2] == 1).all()
    cap = nnz + 3
    rc = np.full(2 * cap + 4, -7, np.int32)
    st = np.full(ns + 4, 0xBEEF, np.uint16)
    prefix[:] = 0
    hip.check(L.rc_expand_frames_l2(nx, ny, d, *src, hip.ptr(prefix), hip.ptr(rc), cap, hip.ptr(st), ns))
    assert np.array_equal(prefix, want_prefix)
    assert np.array_equal(rc[:nnz], rows) and np.array_equal(rc[cap:cap + nnz], cols)
    assert (rc[nnz:cap] == -7).all() and (rc[cap + nnz:] == -7).all()
    assert np.array_equal(st[:ns], stats) and (st[ns:] == 0xBEEF).all()
    # the streaming form, page-locked outputs
    pin_in, pin_rc, pin_st = hip.PinnedBuffer(blob.size), hip.PinnedBuffer(8 * cap + 16), hip.PinnedBuffer(2 * ns + 16)
    pin_in.array[:] = blob
    pin_rc.array[:] = 0x77
    pin_st.array[:] = 0x77
    hip.check(L.rc_expand_frames_l2_submit(1, nx, ny, d, mode, scheme, hip.ptr(pin_in.array), hip.ptr(sizes), n, pin_rc._p, cap, pin_st._p, ns))
    prefix[:] = 0
    hip.check(L.rc_expand_frames_wait(1, hip.ptr(prefix)))
    assert np.array_equal(prefix, want_prefix)
    got = pin_rc.array[:8 * cap].view(np.int32)
    assert np.array_equal(got[:nnz], rows) and np.array_equal(got[cap:cap + nnz], cols)
    assert np.array_equal(pin_st.array[:2 * ns].view(np.uint16), stats)
    assert (pin_rc.array[8 * cap:] == 0x77).all() and (pin_st.array[2 * ns:] == 0x77).all()
    assert L.rc_expand_frames_l2_submit(1, nx, ny, d, mode, scheme, hip.ptr(pin_in.array), hip.ptr(sizes), n, pin_rc._p, cap, pin_st._p, ns - 1) \
        == hip.RC_ERR_OUT_TOO_SMALL
    for b in (pin_in, pin_rc, pin_st):
        b.close()
    # refusals
    for bad in (6, 24):
        assert L.rc_expand_frames_l2(nx, ny, bad, *src, hip.ptr(prefix), hip.ptr(rc), cap, hip.ptr(st), ns) == hip.RC_ERR_UNSUPPORTED
    rc[:] = -7
    st[:] = 0xBEEF
    prefix[:] = 0
    assert L.rc_expand_frames_l2(nx, ny, d, *src, hip.ptr(prefix), hip.ptr(rc), cap, hip.ptr(st), ns - 1) == hip.RC_ERR_OUT_TOO_SMALL
    assert np.array_equal(prefix, want_prefix)
    assert (rc == -7).all() and (st == 0xBEEF).all()
    prefix[:] = 0
    assert L.rc_expand_frames_l2(nx, ny, d, *src, hip.ptr(prefix), hip.ptr(rc), nnz - 1, hip.ptr(st), ns) == hip.RC_ERR_OUT_TOO_SMALL
    assert np.array_equal(prefix, want_prefix)


def test_expand_frames_refuses_malformed_blosc_chunks(hip, orc):
    """One 72 x 136 blosc record, damaged five ways the host walk must catch (and once in a way only the decoding wave sees): the call
    returns its status, writes nothing, and a good batch on the same slot goes through afterwards."""
    L = hip.lib()
    ny, nx, d = 72, 136, 12
    dark, frames = synth_frames(9, 1, ny, nx, 0.05, d)
    thr = orc.threshold(dark, 0)
    blob, sizes, _ = _records(hip, frames, thr, d, 1, 1, 8)
    rows, cols, vals, want_prefix = _expected_l1(orc, frames, thr, 1)
    nnz = int(want_prefix[1])
    geom = (nx, ny, d, 1, 1, 8)
    nblocks = -(-(ny * nx // 8) // 512)
    bstarts = struct.unpack_from("<%di" % nblocks, blob.tobytes(), 16)

    def damaged(what):
        b, s = blob.copy(), sizes.copy()
        if what == "typesize":
            b[3] = 4
        elif what == "split":
            b[2] &= 0xEF
        elif what == "bstart":
            b[16 + 4:16 + 8] = np.frombuffer(struct.pack("<i", int(sizes[0, 0]) + 100), np.uint8)
        elif what == "short":
            s[0, 0] -= 3
        elif what == "csize":
            b[bstarts[0]:bstarts[0] + 4] = np.frombuffer(struct.pack("<i", 600), np.uint8)
        elif what == "block":       # the first block one byte shorter than its LZ4 stream: it no longer decodes to 512 bytes
            c = struct.unpack_from("<i", blob.tobytes(), bstarts[0])[0]
            assert 1 < c < 512
            b[bstarts[0]:bstarts[0] + 4] = np.frombuffer(struct.pack("<i", c - 1), np.uint8)
        return b, s
    cases = [("typesize", hip.RC_ERR_UNSUPPORTED), ("split", hip.RC_ERR_UNSUPPORTED), ("bstart", hip.RC_ERR_CORRUPT), ("short", hip.RC_ERR_CORRUPT),
             ("csize", hip.RC_ERR_CORRUPT), ("block", hip.RC_ERR_CORRUPT)]
    pin_in, pin_out = hip.PinnedBuffer(blob.size), hip.PinnedBuffer(10 * nnz + 16)
    for what, status in cases:
        b, s = damaged(what)
        prefix = np.zeros(2, np.uint64)
        out = np.full(10 * nnz + 16, 0xA5, np.uint8)
        assert L.rc_expand_frames_coo(*geom, hip.ptr(b), hip.ptr(s), 1, hip.ptr(prefix), hip.ptr(out), nnz) == status, what
        assert (out == 0xA5).all(), what
        pin_in.array[:] = b
        pin_out.array[:] = 0x77
        st = L.rc_expand_frames_coo_submit(0, *geom, hip.ptr(pin_in.array), hip.ptr(s), 1, pin_out._p, nnz)
        if what == "block":         # seen on the device: reported by the wait
            hip.check(st)
            st = L.rc_expand_frames_wait(0, hip.ptr(prefix))
        assert st == status, what
        assert (pin_out.array[10 * nnz:] == 0x77).all(), what
        # a good batch on the same slot
        pin_in.array[:] = blob
        hip.check(L.rc_expand_frames_coo_submit(0, *geom, hip.ptr(pin_in.array), hip.ptr(sizes), 1, pin_out._p, nnz))
        hip.check(L.rc_expand_frames_wait(0, hip.ptr(prefix)))
        assert np.array_equal(prefix, want_prefix)
        assert np.array_equal(pin_out.array[:4 * nnz].view(np.int32), rows.astype(np.int32))
        assert np.array_equal(pin_out.array[4 * nnz:8 * nnz].view(np.int32), cols.astype(np.int32))
        assert np.array_equal(pin_out.array[8 * nnz:10 * nnz].view(np.uint16), vals.astype(np.uint16))
    pin_in.close()
    pin_out.close()


def _write_file(tmp_path, base, level, scheme, **extra):
    from pyrecode_amd.recode_reader import merge_parts
    ny, nx, d, nz = 72, 136, 12, 7
    dark, frames = synth_frames(31, nz, ny, nx, 0.05, d)
    frames[nz - 1] = 0
    g = load_npz("g3_l1z12.npz")
    over = dict(num_rows=ny, num_cols=nx, num_frames=nz, num_threads=2, compression_scheme=scheme, reduction_level=level,
                calibration_threshold_epsilon=0, **extra)
    _write_parts(tmp_path, base, dark, frames, 2, g, batch_size=3, **over)
    merge_parts(str(tmp_path), "%s.rc%d" % (base, level), 2)
    return nz


def _l2_reference(rd, nz):
    """(rows, columns, statistics) of every frame from the frame-at-a-time path"""
    rd._ra_off = True
    want = []
    for z in range(nz):
        fr = rd.get_frame(z)[z]
        m, st = fr["data"], fr.get("summary_stats")
        want.append((m.row.astype(np.int32), m.col.astype(np.int32), np.asarray(st) if st is not None else np.zeros(0, np.uint16)))
    return want


def _check_l2_batch(want, a, prefix, rows, cols, sp, stats, dtype):
    assert rows.dtype == np.int32 and cols.dtype == np.int32 and stats.dtype == dtype
    for i in range(len(prefix) - 1):
        lo, hi, s0, s1 = int(prefix[i]), int(prefix[i + 1]), int(sp[i]), int(sp[i + 1])
        r, c, st = want[a + i]
        assert np.array_equal(rows[lo:hi], r) and np.array_equal(cols[lo:hi], c), "frame %d" % (a + i)
        assert np.array_equal(stats[s0:s1], st), "frame %d" % (a + i)


def test_get_frames_l2_and_iter_frames_l2_equal_get_frame(tmp_path, orc):
    """A level-2 blosc file (BASELINE configuration 4's codec), merged and as a part file: get_frames_l2 and iter_frames_l2 deliver
    get_frame's (pixels, statistics) frame by frame, on the device."""
    from pyrecode_amd.recode_reader import ReCoDeReader
    nz = _write_file(tmp_path, "l2", 2, 8, l2_statistics=2)
    rd = ReCoDeReader(str(tmp_path / "l2.rc2"))
    rd.open(print_header=False)
    want = _l2_reference(rd, nz)
    assert sum(w[0].size for w in want) > 0 and sum(w[2].size for w in want) > 0 and want[nz - 1][0].size == 0
    got = rd.get_frames_l2(0, nz)
    assert rd.last_batch_path == 'device'
    _check_l2_batch(want, 0, *got, rd._numpy_dtype)
    seen = 0
    for item in rd.iter_frames_l2(batch=3):
        assert rd.last_batch_path == 'device'
        _check_l2_batch(want, item[0], *item[1:], rd._numpy_dtype)
        seen += len(item[1]) - 1
    assert seen == nz
    got = rd.get_frames_l2(2, 3)
    _check_l2_batch(want, 2, *got, rd._numpy_dtype)
    rd.close()
    part = ReCoDeReader(str(tmp_path / "l2.rc2_part001"), is_intermediate=True)
    part.open(print_header=False)
    k = part._batch_frames()
    ids = [int(i) for i in part.part_frame_ids]
    assert 0 < k < nz
    by_id = [want[i] for i in ids]
    got = part.get_frames_l2(0, k)
    assert part.last_batch_path == 'device'
    _check_l2_batch(by_id, 0, *got, part._numpy_dtype)
    seen = 0
    for item in part.iter_frames_l2(batch=2):
        assert part.last_batch_path == 'device'
        _check_l2_batch(by_id, item[0], *item[1:], part._numpy_dtype)
        seen += len(item[1]) - 1
    assert seen == k
    part.close()


def test_get_frames_l2_falls_back_for_host_only_schemes(tmp_path, orc):
    """a level-2 zlib file: no device decoder - get_frames_l2 / iter_frames_l2 answer through the frame-at-a-time path"""
    from pyrecode_amd.recode_reader import ReCoDeReader
    nz = _write_file(tmp_path, "l2z", 2, 0, l2_statistics=1)
    rd = ReCoDeReader(str(tmp_path / "l2z.rc2"))
    rd.open(print_header=False)
    want = _l2_reference(rd, nz)
    got = rd.get_frames_l2(0, nz)
    assert rd.last_batch_path == 'per-frame'
    _check_l2_batch(want, 0, *got, rd._numpy_dtype)
    for item in rd.iter_frames_l2(batch=4):
        _check_l2_batch(want, item[0], *item[1:], rd._numpy_dtype)
    rd.close()


def test_device_blosc_switch_routes_level1_blosc_files_through_the_device(tmp_path, orc):
    """get_frames_triplets / iter_frames_triplets(device_blosc=True) on a level-1 blosc file: the default call's result, from the device;
    the default call keeps its frame-at-a-time path."""
    from pyrecode_amd.recode_reader import ReCoDeReader
    nz = _write_file(tmp_path, "b1", 1, 8)
    rd = ReCoDeReader(str(tmp_path / "b1.rc1"))
    rd.open(print_header=False)
    rd._ra_off = True
    for coo in (False, True):
        want_prefix, want = rd.get_frames_triplets(0, nz, coo=coo)
        assert rd.last_batch_path == 'per-frame'
        assert int(want_prefix[nz]) > 0
        prefix, got = rd.get_frames_triplets(0, nz, coo=coo, device_blosc=True)
        assert rd.last_batch_path == 'device'
        pieces = [(0, prefix, got)] + list(rd.iter_frames_triplets(batch=3, coo=coo, device_blosc=True))
        assert rd.last_batch_path == 'device'
        for a, pre, body in pieces:
            lo, hi = int(want_prefix[a]), int(want_prefix[a + len(pre) - 1])
            assert np.array_equal(pre.astype(np.int64) + lo, want_prefix[a:a + len(pre)].astype(np.int64))
            if coo:
                for x, y in zip(body, want):
                    assert x.dtype == y.dtype and np.array_equal(x, y[lo:hi])
            else:
                assert body.dtype == np.uint64 and np.array_equal(body, want[lo:hi])
        list(rd.iter_frames_triplets(batch=3, coo=coo))
        assert rd.last_batch_path == 'per-frame'
    rd.close()


def _write_sparse_then_dense(tmp_path, base, seed):
    """a level-2 blosc-LZ4 file of 7 frames of 72 x 136: frames 0..2 hold 4 set pixels each, frames 3..5 about 5 %, frame 6 about 15 %"""
    from pyrecode_amd.recode_reader import merge_parts
    ny, nx, d, nz = 72, 136, 12, 7
    dark, frames = synth_frames(seed, nz, ny, nx, 0.05, d)
    rng = np.random.default_rng(seed + 1)
    for z in range(3):
        frames[z] = dark // 2
        at = rng.choice(ny * nx, 4, replace=False)
        frames[z].reshape(-1)[at] = dark.reshape(-1)[at] + 500
    frames[6] = np.where(rng.random((ny, nx)) < 0.15, dark + rng.integers(1, 2000, (ny, nx)), dark // 2).astype(np.uint16)
    sub = tmp_path / base
    sub.mkdir()
    over = dict(num_rows=ny, num_cols=nx, num_frames=nz, num_threads=1, compression_scheme=8, reduction_level=2,
                calibration_threshold_epsilon=0, l2_statistics=2)
    _write_parts(sub, base, dark, frames, 1, load_npz("g3_l1z12.npz"), batch_size=3, **over)
    merge_parts(str(sub), base + ".rc2", 1)
    return str(sub / (base + ".rc2")), nz


def test_iter_frames_l2_retries_a_batch_its_estimate_was_too_small_for(hip, tmp_path, monkeypatch):
    """iter_frames_l2 sizes a batch from the densest batch DELIVERED so far.  Frames 0..2 hold 4 set pixels each, frames 3..5 about 5 % of
    72 x 136 and frame 6 about 15 %.  In batches of three, batch j + 1 is queued before batch j is waited for: the first two batches are
    both counted on the device, and the third - frame 6 alone, queued when only the first batch has been delivered - is given
    1 * 4 * 1.25 + 1024 = 1029 entries and needs about 1470.  Its verdict is RC_ERR_OUT_TOO_SMALL and it goes through the synchronous
    call; every item still equals get_frame's pixels and statistics, and every batch was decoded on the device."""
    from pyrecode_amd import reader_batched as rb
    from pyrecode_amd.recode_reader import ReCoDeReader
    path, nz = _write_sparse_then_dense(tmp_path, "grow", 57)
    rd = ReCoDeReader(path)
    rd.open(print_header=False)
    want = _l2_reference(rd, nz)
    assert all(0 < w[0].size <= 4 for w in want[:3]) and all(400 < w[0].size < 600 for w in want[3:6]) and want[6][0].size > 1 * 4 * 1.25 + 1024
    verdicts, wait = [], rb._wait
    monkeypatch.setattr(rb, "_wait", lambda job: (verdicts.append(wait(job)), verdicts[-1])[1])
    firsts = []
    for item in rd.iter_frames_l2(batch=3):
        assert rd.last_batch_path == 'device'
        _check_l2_batch(want, item[0], *item[1:], rd._numpy_dtype)
        firsts.append((item[0], len(item[1]) - 1))
    assert firsts == [(0, 3), (3, 3), (6, 1)]
    assert [st for st, _ in verdicts] == [hip.RC_OK, hip.RC_OK, hip.RC_ERR_OUT_TOO_SMALL]
    rd.close()


def test_two_level2_iterators_side_by_side(hip, tmp_path, monkeypatch):
    """test_gpu_api.py::test_two_streaming_iterators_side_by_side for level 2: two readers of two level-2 files advanced in turn both
    deliver every frame, and a submit did find its slot held by the other reader's batch - that batch went through the synchronous call."""
    from pyrecode_amd import reader_batched as rb
    from pyrecode_amd.recode_reader import ReCoDeReader
    sets = []
    for base, seed in (("one", 61), ("two", 67)):
        path, nz = _write_sparse_then_dense(tmp_path, base, seed)
        rd = ReCoDeReader(path)
        rd.open(print_header=False)
        sets.append((rd, _l2_reference(rd, nz)))
    taken, asked = [], rb._slot_taken
    monkeypatch.setattr(rb, "_slot_taken", lambda st: (taken.append(asked(st)), taken[-1])[1])      # (a count of the submits that found a slot held)
    its = [rd.iter_frames_l2(batch=2) for rd, _ in sets]
    seen, alive = [0, 0], [True, True]
    while any(alive):
        for j in (0, 1):
            item = next(its[j], None) if alive[j] else None
            if item is None:
                alive[j] = False
                continue
            rd, want = sets[j]
            assert rd.last_batch_path == 'device'
            _check_l2_batch(want, item[0], *item[1:], rd._numpy_dtype)
            seen[j] += len(item[1]) - 1
    assert seen == [nz, nz] and any(taken), "no batch found its slot taken: the synchronous call was not exercised"
    for rd, _ in sets:
        rd.close()
