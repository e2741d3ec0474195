"""-m gpu: the batched device inflate (rc_inflate.hip) - rc_expand_frames & co. with op_mode 1 and scheme RC_SCHEME_ZLIB_DEVICE, and the
readers' device_zlib=True on top.
  - the catalogue of tests/inflate_chain_model.py (every case of the candidate / chain scheme, judged on the CPU by test_inflate_chain_cpu.py)
    against the same frames expanded with op_mode 0 from their uncompressed pieces, and against the pixels numpy reads off the bitmap;
  - streams the reader must refuse: status, untouched output, and a good call behind them;
  - files: ReCoDeWriter(device_zlib=True) -> ReCoDeReader(device_zlib=True) against the frame-at-a-time path; a stock-zlib file falls back."""
import os
import zlib

import numpy as np
import pytest

import inflate_chain_model as icm

pytestmark = pytest.mark.gpu

ZDEV = 0x100
HERE = os.path.dirname(os.path.abspath(__file__))
FRAMES = icm.catalogue()
REFUSED = icm.refused_catalogue(FRAMES)


@pytest.fixture(scope="module")
def hip():
    from pyrecode_amd import _lib
    if _lib.device_count() == 0:
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    assert _lib.RC_SCHEME_ZLIB_DEVICE == ZDEV
    return _lib


def _batch(frames, level, compressed):
    """(blob, sizes) of a batch as rc_expand_frames takes it: the frames' streams (mode 1) or their uncompressed pieces (mode 0)"""
    sizes, parts = np.zeros((len(frames), 3), np.uint32), []
    for i, f in enumerate(frames):
        m, v = (f["map_stream"], f["val_stream"]) if compressed else (f["bitmap"], f["values"])
        parts.append(m)
        sizes[i, 0] = len(m)
        if level == 1:
            parts.append(v)
            sizes[i, 1], sizes[i, 2] = len(v), len(f["values"])
    return np.frombuffer(b"".join(parts), np.uint8).copy(), sizes


def _expand(hip, geom, blob, sizes, fn="rc_expand_frames", fill=0xA5):
    """-> (status, prefix, output array, cap); the output is filled with `fill` first"""
    L, n = hip.lib(), sizes.shape[0]
    nx, ny, d, level = geom[:4]
    cap = int(sizes[:, 2].astype(np.uint64).sum()) * 8 // d + 3 if level == 1 else nx * ny * n + 3
    out = np.full((24 if fn == "rc_expand_frames" else 10) * cap + 16, fill, np.uint8)
    prefix = np.zeros(n + 1, np.uint64)
    st = getattr(L, fn)(*geom, hip.ptr(blob), hip.ptr(sizes), n, hip.ptr(prefix), hip.ptr(out), cap)
    return st, prefix, out, cap


def _pixels(f):
    bits = np.unpackbits(np.frombuffer(f["bitmap"], np.uint8), bitorder="little")[:f["nx"] * f["ny"]]
    k = np.nonzero(bits)[0]
    return k // f["nx"], k % f["nx"]


def _groups():
    """batches of catalogue frames of one geometry; a geometry with one frame has it twice (streams at other offsets and alignments)"""
    by = {}
    for f in FRAMES:
        by.setdefault((f["nx"], f["ny"], f["d"]), []).append(f)
    return [fs + fs[:1] for fs in by.values()]


@pytest.mark.parametrize("level", [1, 3])
@pytest.mark.parametrize("frames", _groups(), ids=lambda fs: "+".join(f["name"] for f in fs[:-1]))
def test_catalogue_through_expand_frames(hip, frames, level):
    nx, ny, d = frames[0]["nx"], frames[0]["ny"], frames[0]["d"]
    n = len(frames)
    blob0, sizes0 = _batch(frames, level, False)
    blob1, sizes1 = _batch(frames, level, True)
    for fn in ("rc_expand_frames", "rc_expand_frames_coo"):
        st0, want_prefix, want, cap = _expand(hip, (nx, ny, d, level, 0, 0), blob0, sizes0, fn)
        hip.check(st0)
        st, prefix, got, _ = _expand(hip, (nx, ny, d, level, 1, ZDEV), blob1, sizes1, fn)
        hip.check(st)
        assert np.array_equal(prefix, want_prefix)
        assert np.array_equal(got, want)                     # entries and the untouched rest alike
        nnz = int(prefix[n])
        rows = np.concatenate([_pixels(f)[0] for f in frames])
        cols = np.concatenate([_pixels(f)[1] for f in frames])
        assert nnz == rows.size
        if fn == "rc_expand_frames":
            t = got[:24 * cap].view(np.uint64).reshape(cap, 3)[:nnz]
            assert np.array_equal(t[:, 0], rows.astype(np.uint64)) and np.array_equal(t[:, 1], cols.astype(np.uint64))
        else:
            assert np.array_equal(got[:4 * cap].view(np.int32)[:nnz], rows) and np.array_equal(got[4 * cap:8 * cap].view(np.int32)[:nnz], cols)
    # the counting call
    L = hip.lib()
    prefix = np.zeros(n + 1, np.uint64)
    hip.check(L.rc_expand_frames(nx, ny, d, level, 1, ZDEV, hip.ptr(blob1), hip.ptr(sizes1), n, hip.ptr(prefix), None, 0))
    assert np.array_equal(prefix, want_prefix)


def test_submit_wait_on_both_slots(hip):
    """two catalogue batches in flight, one per slot, triplets and COO into page-locked memory"""
    L = hip.lib()
    jobs = []
    for slot, frames in enumerate([g for g in _groups() if g[0]["d"] <= 16][:2]):
        f0 = frames[0]
        geom = (f0["nx"], f0["ny"], f0["d"], 1)
        fn = "rc_expand_frames_coo" if slot else "rc_expand_frames"
        st, want_prefix, want, cap = _expand(hip, geom + (0, 0), *_batch(frames, 1, False), fn)
        hip.check(st)
        blob, sizes = _batch(frames, 1, True)
        src = hip.PinnedBuffer(blob.size + 64)
        src.array[:blob.size] = blob
        dst = hip.PinnedBuffer(want.size)
        dst.array[:] = 0xA5
        hip.check(getattr(L, fn + "_submit")(slot, *geom, 1, ZDEV, hip.ptr(src.array), hip.ptr(sizes), len(frames), dst._p, cap))
        jobs.append((src, dst, want_prefix, want, len(frames)))
    for slot, (src, dst, want_prefix, want, n) in enumerate(jobs):
        prefix = np.zeros(n + 1, np.uint64)
        hip.check(L.rc_expand_frames_wait(slot, hip.ptr(prefix)))
        assert np.array_equal(prefix, want_prefix) and np.array_equal(dst.array[:want.size], want)
        src.close()
        dst.close()


@pytest.mark.parametrize("frame", REFUSED, ids=lambda f: f["name"])
def test_refused_streams_leave_the_output_alone(hip, frame):
    good = next(f for f in FRAMES if f["name"] == "short_last_tile")
    for fn in ("rc_expand_frames", "rc_expand_frames_coo"):
        geom = (frame["nx"], frame["ny"], frame["d"], 1, 1, ZDEV)
        blob, sizes = _batch([frame, frame], 1, True)
        st, prefix, out, _ = _expand(hip, geom, blob, sizes, fn, fill=0x5C)
        assert st in (hip.RC_ERR_UNSUPPORTED, hip.RC_ERR_CORRUPT), st
        assert (out == 0x5C).all()
        ggeom = (good["nx"], good["ny"], good["d"], 1)
        st0, want_prefix, want, _ = _expand(hip, ggeom + (0, 0), *_batch([good], 1, False), fn)
        st1, prefix, got, _ = _expand(hip, ggeom + (1, ZDEV), *_batch([good], 1, True), fn)
        assert (st0, st1) == (0, 0) and np.array_equal(prefix, want_prefix) and np.array_equal(got, want)


def test_refused_batch_on_a_streaming_slot(hip):
    """a batch with a stock-zlib stream is refused - by the host's look at the header at submit, or by the device and then at _wait -,
    the page-locked output untouched, and the slot takes a good batch next"""
    L = hip.lib()
    good = next(f for f in FRAMES if f["name"] == "short_last_tile")
    bad = dict(good, map_stream=zlib.compress(good["bitmap"], 1))
    geom = (good["nx"], good["ny"], good["d"], 1)
    st, want_prefix, want, cap = _expand(hip, geom + (0, 0), *_batch([good, good], 1, False))
    hip.check(st)
    dst = hip.PinnedBuffer(want.size)
    for frames, ok in (([good, bad], False), ([good, good], True)):
        blob, sizes = _batch(frames, 1, True)
        src = hip.PinnedBuffer(blob.size + 64)
        src.array[:blob.size] = blob
        dst.array[:] = 0xA5
        prefix = np.zeros(3, np.uint64)
        st = L.rc_expand_frames_submit(0, *geom, 1, ZDEV, hip.ptr(src.array), hip.ptr(sizes), 2, dst._p, cap)
        if st == 0:
            st = L.rc_expand_frames_wait(0, hip.ptr(prefix))
        if ok:
            hip.check(st)
            assert np.array_equal(prefix, want_prefix) and np.array_equal(dst.array[:want.size], want)
        else:
            assert st == hip.RC_ERR_UNSUPPORTED and (dst.array[:want.size] == 0xA5).all()
        src.close()
    dst.close()


def test_other_entry_points_keep_their_answers(hip):
    """scheme 0 stays unsupported, and so does level 2 with the device scheme"""
    L = hip.lib()
    f = next(f for f in FRAMES if f["name"] == "one_tile")
    blob, sizes = _batch([f], 1, True)
    assert _expand(hip, (f["nx"], f["ny"], f["d"], 1, 1, 0), blob, sizes)[0] == hip.RC_ERR_UNSUPPORTED
    assert _expand(hip, (f["nx"], f["ny"], f["d"], 2, 1, ZDEV), blob, sizes)[0] == hip.RC_ERR_UNSUPPORTED
    prefix, rc, stats = np.zeros(2, np.uint64), np.zeros(8 * 4096, np.uint8), np.zeros(4096, np.uint16)
    st = L.rc_expand_frames_l2(f["nx"], f["ny"], f["d"], 1, ZDEV, hip.ptr(blob), hip.ptr(sizes), 1, hip.ptr(prefix), hip.ptr(rc), 4096, hip.ptr(stats), 4096)
    assert st == hip.RC_ERR_UNSUPPORTED


# ---- records of the device encoder itself ------------------------------------------------------------------------------------------
def _device_records(hip, frames, thr, d, level, clevel):
    n, ny, nx = frames.shape
    ctx = hip.ReduceContext(nx, ny, d, level, 1, 0, clevel, 0, max_batch=n, device_zlib=True)
    ctx.set_threshold(thr)
    out, rec, md = ctx.reduce_compress_batch(frames, 0)
    ctx.close()
    sizes, blobs = np.zeros((n, 3), np.uint32), []
    for z in range(n):
        r = out[int(rec[z]):int(rec[z + 1])]
        if level == 1:
            sizes[z] = md[z, :3]
            blobs.append(r[16:])
        else:
            sizes[z, 0] = md[z, 0]
            blobs.append(r[8:])
    return blobs, sizes


def test_large_frames_long_chains(hip):
    """4096 x 4096 at 1 %, 4 frames: 4096 tiles per map (the chain passes every one), a dozen value chunks, coded at compression_level 6"""
    L = hip.lib()
    ny = nx = 4096
    d, n = 12, 4
    rng = np.random.default_rng(7)
    frames = np.zeros((n, ny * nx), np.uint16)
    for z in range(n):
        at = np.unique(rng.integers(0, ny * nx, ny * nx // 100))
        frames[z, at] = rng.choice(np.array([1, 2, 3, 4, 5, 9, 300], np.uint16), at.size, p=[.4, .25, .15, .1, .05, .03, .02])
    frames = frames.reshape(n, ny, nx)
    thr = np.zeros((ny, nx), np.uint16)
    blobs, sizes = _device_records(hip, frames, thr, d, 1, 6)
    pieces, sizes0 = [], np.zeros((n, 3), np.uint32)
    coded = 0
    for z in range(n):
        cb, cp = int(sizes[z, 0]), int(sizes[z, 1])
        m, v = zlib.decompress(blobs[z][:cb].tobytes()), zlib.decompress(blobs[z][cb:cb + cp].tobytes())
        coded += (blobs[z][cb + 2] & 6) == 4
        pieces += [m, v]
        sizes0[z] = (len(m), len(v), len(v))
        assert len(v) == sizes[z, 2] and len(m) == ny * nx // 8
    assert coded == n
    blob1 = np.ascontiguousarray(np.concatenate(blobs))
    blob0 = np.frombuffer(b"".join(pieces), np.uint8).copy()
    st0, want_prefix, want, cap = _expand(hip, (nx, ny, d, 1, 0, 0), blob0, sizes0, "rc_expand_frames_coo")
    st1, prefix, got, _ = _expand(hip, (nx, ny, d, 1, 1, ZDEV), blob1, sizes, "rc_expand_frames_coo")
    assert (st0, st1) == (0, 0)
    assert np.array_equal(prefix, want_prefix) and int(prefix[n]) > n * (ny * nx // 101)
    assert np.array_equal(got, want)


# ---- files -----------------------------------------------------------------------------------------------------------------------
def _write_file(tmp, data, dark, depth, level, clevel, nodes=3):
    from pyrecode_amd.params import InputParams
    from pyrecode_amd.recode_writer import ReCoDeWriter
    from pyrecode_amd.recode_reader import merge_parts
    nz, ny, nx = data.shape
    text = open(os.path.join(HERE, "golden", "files", "recode_params_minimal_read_write_test.txt")).read()
    for a, b in (("compression_level = 1", "compression_level = %d" % clevel), ("reduction_level = 1", "reduction_level = %d" % level),
                 ("source_bit_depth = 12", "source_bit_depth = %d" % depth), ("target_bit_depth = 12", "target_bit_depth = %d" % depth)):
        assert a in text
        text = text.replace(a, b)
    params = tmp / "params.txt"
    params.write_text(text)
    for node in range(nodes):
        ip = InputParams()
        ip.load(str(params))
        ip.nx, ip.ny, ip.nz = nx, ny, nz
        ip.source_data_type = ip.target_data_type = 0
        w = ReCoDeWriter("t", dark_data=dark, output_directory=str(tmp), input_params=ip, node_id=node, device_zlib=True)
        w.start()
        assert not w._host_compress
        w.run(data)
        w.close()
    name = "t.rc%d" % level
    merge_parts(str(tmp), name, nodes)
    return str(tmp / name)


def _events(rng, nz, ny, nx, p, depth, amp=None):
    top = (1 << depth) - 1
    vals = rng.integers(1, top + 1, (nz, ny, nx)) if amp is None else rng.choice(np.asarray(amp), (nz, ny, nx))
    return np.where(rng.random((nz, ny, nx)) < p, vals, 0).astype(np.uint16)


def _check_file(path, nz, batch=None, level=1):
    """get_frames_triplets and iter_frames_triplets with device_zlib=True against get_frame, frame by frame"""
    from pyrecode_amd.recode_reader import ReCoDeReader
    rd = ReCoDeReader(path)
    rd.open(print_header=False)
    assert rd.get_header().as_dict()["compression_scheme"] == 0
    want = []
    for z in range(nz):
        m = rd.get_frame(z)[z]["data"].tocoo()
        order = np.lexsort((m.col, m.row))
        want.append((m.row[order].astype(np.int64), m.col[order].astype(np.int64), m.data[order].astype(np.int64)))
    prefix, (rows, cols, vals) = rd.get_frames_triplets(0, nz, coo=True, device_zlib=True)
    assert rd.last_batch_path == "device-inflate"
    for z in range(nz):
        lo, hi = int(prefix[z]), int(prefix[z + 1])
        assert np.array_equal(rows[lo:hi], want[z][0]) and np.array_equal(cols[lo:hi], want[z][1]) and np.array_equal(vals[lo:hi].astype(np.int64), want[z][2])
    prefix, trip = rd.get_frames_triplets(1 if nz > 1 else 0, 1, device_zlib=True)
    z = 1 if nz > 1 else 0
    assert rd.last_batch_path == "device-inflate" and np.array_equal(trip[:, 2].astype(np.int64), want[z][2])
    seen = 0
    for a, pre, (rows, cols, vals) in rd.iter_frames_triplets(0, nz, batch=batch or nz, coo=True, device_zlib=True):
        assert rd.last_batch_path == "device-inflate" and a == seen
        for j in range(len(pre) - 1):
            lo, hi = int(pre[j]), int(pre[j + 1])
            w = want[a + j]
            assert np.array_equal(rows[lo:hi], w[0]) and np.array_equal(cols[lo:hi], w[1]) and np.array_equal(vals[lo:hi].astype(np.int64), w[2])
        seen += len(pre) - 1
    assert seen == nz and not rd._foreign_file
    # the default is what it was
    rd.get_frames_triplets(0, nz)
    assert rd.last_batch_path == "host-decode + device-expand"
    rd.close()


@pytest.mark.parametrize("ny,nx", [(64, 64), (64, 65), (24, 40)])
def test_small_files_round_trip(hip, tmp_path, ny, nx):
    """one tile, two tiles with a short last one, less than a tile.  (The 3 x 5 frame of the catalogue goes through rc_expand_frames above; as a
    FILE it does not exist: two zlib streams and a record header exceed the 30 bytes of the raw frame, and the writer refuses such a record
    as the reference does - 24 x 40 is a frame under one tile that it writes.)"""
    rng = np.random.default_rng(ny * nx)
    data = _events(rng, 3, ny, nx, 0.05, 12)
    assert data.reshape(3, -1).any(axis=1).all()
    _check_file(_write_file(tmp_path, data, np.zeros((ny, nx), np.uint16), 12, 1, 1), 3)


@pytest.mark.parametrize("depth", [16, 12])
@pytest.mark.parametrize("clevel", [1, 6])
def test_files_with_stored_and_coded_values(hip, tmp_path, depth, clevel):
    """512 x 512 at 14.5 %: ~ 76 KB (d = 16) / 57 KB (d = 12) of values per frame - stored chunks at compression_level 1, at level 6 coded ones,
    two or three per frame"""
    rng = np.random.default_rng(depth + clevel)
    data = _events(rng, 3, 512, 512, 0.145, depth, amp=[1, 1, 1, 2, 2, 3, 5, 8, 200])
    path = _write_file(tmp_path, data, np.zeros((512, 512), np.uint16), depth, 1, clevel)
    from pyrecode_amd.recode_reader import ReCoDeReader
    rd = ReCoDeReader(path)
    rd.open(print_header=False)
    md = rd._frame_metadata[0]
    rd._fp.seek(rd._frame_data_start_position + int(rd._seek_table[0, 1]) + int(md["bytes_in_compressed_binary_map"]), 0)
    first = rd._fp.read(3)
    rd.close()
    assert first[:2] == b"\x78\x01" and (first[2] & 6) == (4 if clevel == 6 else 0)
    assert int(md["bytes_in_packed_pixvals"]) > 32768
    _check_file(path, 3)


def test_level_3_file_and_all_set_region(hip, tmp_path):
    """reduction level 3 (bitmap only), with a block of rows all set: tiles that do not shrink are stored blocks"""
    rng = np.random.default_rng(3)
    data = _events(rng, 3, 512, 512, 0.02, 12)
    data[1, 100:300, :] = 7
    path = _write_file(tmp_path, data, np.zeros((512, 512), np.uint16), 12, 3, 1)
    _check_file(path, 3, level=3)


def test_all_set_region_level_1(hip, tmp_path):
    rng = np.random.default_rng(4)
    data = _events(rng, 3, 512, 512, 0.02, 12)
    data[2, 64:192, :] = 9
    data[0, :, :] = 3
    _check_file(_write_file(tmp_path, data, np.zeros((512, 512), np.uint16), 12, 1, 6), 3)


def test_ragged_last_batch_pipelined(hip, tmp_path):
    rng = np.random.default_rng(13)
    data = _events(rng, 13, 128, 192, 0.03, 12)
    _check_file(_write_file(tmp_path, data, np.zeros((128, 192), np.uint16), 12, 1, 6), 13, batch=4)


def test_stock_zlib_file_falls_back(hip):
    """the reference's own zlib file: refused once, read through the host-decoded path, the same frames as without the switch"""
    from pyrecode_amd.recode_reader import ReCoDeReader
    path = os.path.join(HERE, "golden", "files", "g3_l1z12.rc1")
    rd = ReCoDeReader(path)
    rd.open(print_header=False)
    nz = rd._batch_frames()
    want_prefix, want = rd.get_frames_triplets(0, nz)
    assert rd.last_batch_path == "host-decode + device-expand" and not rd._foreign_file
    want = want.copy()
    prefix, trip = rd.get_frames_triplets(0, nz, device_zlib=True)
    assert rd.last_batch_path == "host-decode + device-expand" and rd._foreign_file
    assert np.array_equal(prefix, want_prefix) and np.array_equal(trip, want)
    prefix, trip = rd.get_frames_triplets(0, nz, device_zlib=True)          # not offered again
    assert rd.last_batch_path == "host-decode + device-expand" and rd._foreign_file and np.array_equal(trip, want)
    rd.close()
    rd = ReCoDeReader(path)
    rd.open(print_header=False)
    seen = 0
    for a, pre, tr in rd.iter_frames_triplets(0, nz, batch=2, device_zlib=True):
        lo, hi = int(want_prefix[a]), int(want_prefix[a + len(pre) - 1])
        assert rd.last_batch_path == "host-decode + device-expand"
        assert np.array_equal(tr, want[lo:hi])
        seen += len(pre) - 1
    assert seen == nz and rd._foreign_file
    rd.close()
