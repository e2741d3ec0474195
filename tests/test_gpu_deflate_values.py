"""-m gpu: the device DEFLATE encoder at compression_level >= 2 (rc_pix_deflate.hip) through the C ABI.  Both streams of every record must be
zlib streams STDLIB zlib expands to the oracle's bytes, the metadata row must match their lengths, the map stream must equal
deflate_block_model.bitmap_stream and the value stream must equal the serial model (tests/deflate_values_model.py::encode_values) under the
table the stream itself carries - or the stored stream where no chunk is coded."""
import struct
import zlib

import numpy as np
import pytest

import deflate_block_model as model
import deflate_values_model as vmodel
from conftest import synth_frames

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


def _check_record(orc, r, frame, thr, d, fid, md_row=None, table=None):
    """-> (cp, length of the stored form, the table the value stream carries or None)"""
    bitmap = orc.pack_binary_frame(frame > thr).tobytes()
    got_fid, cb, cp, npk = struct.unpack_from("<IIII", r, 0)
    assert got_fid == fid and len(r) == 16 + cb + cp
    if md_row is not None:
        assert (cb, cp, npk) == tuple(int(v) for v in md_row)
    _, pix = orc.binarize_l1(frame, thr)
    packed = orc.bit_pack(pix, d).tobytes()
    assert npk == len(packed)
    assert zlib.decompress(r[16:16 + cb]) == bitmap           # (zlib.decompress also checks the Adler-32 and that nothing trails the stream)
    assert zlib.decompress(r[16 + cb:]) == packed
    assert r[16:16 + cb] == model.bitmap_stream(bitmap), "binary-map stream differs from the serial model"
    stream = r[16 + cb:]
    t = vmodel.parse_table(stream)
    if table is not None and t is not None:
        assert t == table, "two frames of one ctx carry different tables"
    want = vmodel.encode_values(packed, t) if t is not None else model.stored_stream(packed)
    assert stream == want, "residual stream differs from the serial model"
    return cp, len(model.stored_stream(packed)), t


def _records(out, rec, n):
    return [out[int(rec[z]):int(rec[z + 1])].tobytes() for z in range(n)]


@pytest.mark.parametrize("d", [16, 12, 11, 8, 3, 1])
def test_depths_and_chunk_borders(hip, orc, d):
    """The residual stream spans several 32 KiB chunks at bit phases of every kind; at d = 16 chunks are coded (inner and final ones) and the
    stream is smaller than the stored form - which is what compression_level 1 still writes."""
    ny, nx = 512, 700
    dark, frames = synth_frames(900 + d, 2, ny, nx, 0.22, 12)
    thr = orc.threshold(dark, 0)
    ctx = hip.ReduceContext(nx, ny, d, 1, 1, 0, 2, 0, max_batch=2, device_zlib=True)
    ctx.set_dark(dark, 0)
    out, rec, md = ctx.reduce_compress_batch(frames, first_frame_id=0)
    table = None
    for z, r in enumerate(_records(out, rec, 2)):
        cp, stored, t = _check_record(orc, r, frames[z], thr, d, z, md[z], table)
        table = table or t
        assert cp <= stored
        if d == 16:
            assert t is not None and cp < stored
    ctx.close()


def test_edge_frames(hip, orc):
    ny, nx = 200, 333
    dark, frames = synth_frames(77, 3, ny, nx, 0.02, 12)
    frames[0] = 0                        # nothing set: the residual stream is one empty stored block
    frames[1] = 4000                     # everything set
    thr = orc.threshold(dark, 0)
    ctx = hip.ReduceContext(nx, ny, 12, 1, 1, 0, 2, 0, max_batch=3, device_zlib=True)
    ctx.set_dark(dark, 0)
    out, rec, md = ctx.reduce_compress_batch(frames, first_frame_id=50)
    for z, r in enumerate(_records(out, rec, 3)):
        _check_record(orc, r, frames[z], thr, 12, 50 + z, md[z])
    ctx.close()


def test_data_unlike_the_table_and_refit(hip, orc):
    """A second batch of constant 0xFFFF residuals under a table fitted to ordinary ones (every symbol has a code), then once more after
    refit_model()."""
    ny, nx, d = 256, 512, 16
    rng = np.random.default_rng(5)
    dark = np.zeros((ny, nx), np.uint16)                     # threshold 0: a set pixel's residual is its value
    thr = orc.threshold(dark, 0)
    frames = np.where(rng.random((2, ny, nx)) < 0.3, rng.integers(1, 2048, (2, ny, nx)), 0).astype(np.uint16)
    const = np.where(rng.random((2, ny, nx)) < 0.3, 0xFFFF, 0).astype(np.uint16)
    ctx = hip.ReduceContext(nx, ny, d, 1, 1, 0, 2, 0, max_batch=2, device_zlib=True)
    ctx.set_dark(dark, 0)
    out, rec, md = ctx.reduce_compress_batch(frames, first_frame_id=0)
    t0 = None
    for z, r in enumerate(_records(out, rec, 2)):
        t0 = _check_record(orc, r, frames[z], thr, d, z, md[z], t0)[2]
    assert t0 is not None
    out, rec, md = ctx.reduce_compress_batch(const, first_frame_id=2)
    for z, r in enumerate(_records(out, rec, 2)):
        t = _check_record(orc, r, const[z], thr, d, 2 + z, md[z])[2]
        assert t is None or t == t0
    ctx.refit_model()
    out, rec, md = ctx.reduce_compress_batch(const, first_frame_id=4)
    for z, r in enumerate(_records(out, rec, 2)):
        cp, stored, t = _check_record(orc, r, const[z], thr, d, 4 + z, md[z])
        assert t is not None and t != t0 and cp < stored // 4
    ctx.close()


def test_more_than_4096_tiles_take_the_segmented_scans(hip, orc):
    """4097 tiles: the tile scans are k_scan_seg / k_scan_fix, which must leave a DEFLATE ctx's block-size words as they are (no zstd model).
    Three chunks (two inner, one final); two calls on one ctx - the second starts with the table fitted."""
    ny, nx, d = 4097, 4096, 16
    rng = np.random.default_rng(41)
    dark = np.zeros((ny, nx), np.uint16)
    thr = orc.threshold(dark, 0)
    flat = np.zeros(ny * nx, np.uint16)
    flat[rng.integers(0, ny * nx, 33600)] = rng.integers(1, 2048, 33600)      # 0.2 % of the pixels
    ctx = hip.ReduceContext(nx, ny, d, 1, 1, 0, 2, 0, max_batch=1, device_zlib=True)
    ctx.set_dark(dark, 0)
    table = None
    for call, frame in enumerate((flat.reshape(ny, nx), flat[::-1].reshape(ny, nx).copy())):
        out, rec, md = ctx.reduce_compress_batch(frame[None], first_frame_id=call)
        assert 2 << 15 < int(md[0][2]) <= 3 << 15
        cp, stored, t = _check_record(orc, _records(out, rec, 1)[0], frame, thr, d, call, md[0], table)
        assert t is not None and cp < stored
        table = t
    ctx.close()


def test_uint8_sources(hip, orc):
    ny, nx = 130, 260
    rng = np.random.default_rng(3)
    dark = rng.integers(8, 12, (ny, nx)).astype(np.uint8)
    frames = np.where(rng.random((3, ny, nx)) < 0.5, rng.integers(20, 60, (3, ny, nx)), rng.integers(0, 8, (3, ny, nx))).astype(np.uint8)
    thr = dark.astype(np.uint16)
    ctx = hip.ReduceContext(nx, ny, 8, 1, 1, 0, 2, 0, max_batch=3, src_dtype=np.uint8, device_zlib=True)
    ctx.set_dark(dark, 0)
    out, rec, md = ctx.reduce_compress_batch(frames, first_frame_id=0)
    coded = 0
    for z, r in enumerate(_records(out, rec, 3)):
        coded += _check_record(orc, r, frames[z].astype(np.uint16), thr, 8, z, md[z])[2] is not None
    assert coded == 3
    ctx.close()


def test_level_1_next_to_level_2_and_the_other_reduction_levels(hip, orc):
    """compression_level 1 still stores the values; reduction levels 2 and 3 write at compression_level 2 what they write at 1."""
    ny, nx, d = 256, 512, 16
    dark, frames = synth_frames(21, 2, ny, nx, 0.2, 12)
    thr = orc.threshold(dark, 0)
    recs = {}
    for clevel in (1, 2):
        ctx = hip.ReduceContext(nx, ny, d, 1, 1, 0, clevel, 0, max_batch=2, device_zlib=True)
        ctx.set_dark(dark, 0)
        out, rec, md = ctx.reduce_compress_batch(frames, first_frame_id=0)
        recs[clevel] = _records(out, rec, 2)
        ctx.close()
    for z in range(2):
        cb, cp = struct.unpack_from("<II", recs[1][z], 4)
        _, pix = orc.binarize_l1(frames[z], thr)
        assert recs[1][z][16 + cb:] == model.stored_stream(orc.bit_pack(pix, d).tobytes())
        cp2, stored, t = _check_record(orc, recs[2][z], frames[z], thr, d, z)
        assert t is not None and cp2 < cp == stored
    for level in (2, 3):
        got = {}
        for clevel in (1, 2):
            ctx = hip.ReduceContext(nx, ny, 12, level, 1, 0, clevel, 0, max_batch=2, device_zlib=True)
            ctx.set_dark(dark, 0)
            out, rec, md = ctx.reduce_compress_batch(frames, first_frame_id=0)
            got[clevel] = out[:int(rec[2])].tobytes()
            ctx.close()
        assert got[1] == got[2]


def test_async_pipelined_batches(hip, orc):
    import torch
    ny, nx, B, d = 256, 1024, 6, 16
    dark, frames = synth_frames(12, 3 * B, ny, nx, 0.1, 14)
    thr = orc.threshold(dark, 0)
    ctx = hip.ReduceContext(nx, ny, d, 1, 1, 0, 2, 0, max_batch=B, device_zlib=True)
    ctx.set_dark(dark, 0)
    ctx.keep_binary_maps(False)
    ctx.set_pipelined(True)
    fd = torch.from_numpy(frames.view(np.int16)).cuda()
    cap = int(ctx.out_capacity(B))
    outs = [torch.empty(cap, dtype=torch.uint8, device="cuda") for _ in range(2)]       # two output sets, used in turn
    recs = [torch.empty(B + 1, dtype=torch.int64, device="cuda") for _ in range(2)]
    mds = [torch.empty((B, 3), dtype=torch.int32, device="cuda") for _ in range(2)]
    got = []
    for i in range(3):
        if i == 2:        # set 0 is handed out again: take its first batch's results
            ctx.sync()
            got.append((recs[0].cpu().numpy(), outs[0].cpu().numpy(), mds[0].cpu().numpy()))
        ctx.enqueue(fd[i * B:(i + 1) * B].data_ptr(), B, i * B, outs[i & 1].data_ptr(), cap, recs[i & 1].data_ptr(), mds[i & 1].data_ptr())
    ctx.sync()
    got.append((recs[1].cpu().numpy(), outs[1].cpu().numpy(), mds[1].cpu().numpy()))
    got.append((recs[0].cpu().numpy(), outs[0].cpu().numpy(), mds[0].cpu().numpy()))
    table = None
    for i, (rec, out, md) in enumerate(got):
        for z, r in enumerate(_records(out, rec, B)):
            t = _check_record(orc, r, frames[i * B + z], thr, d, i * B + z, md[z], table)[2]
            table = table or t
    assert table is not None
    ctx.close()


def test_writer_at_compression_level_6_writes_smaller_files_the_reader_reads(hip, orc, tmp_path):
    """ReCoDeWriter(device_zlib=True) on the reference's test configuration with compression_level = 6: part files merge, the reader returns
    the frames, and the file is smaller than the same run at compression_level 1."""
    import os
    from pyrecode_amd.params import InputParams
    from pyrecode_amd.recode_writer import ReCoDeWriter
    from pyrecode_amd.recode_reader import ReCoDeReader, merge_parts
    here = os.path.dirname(os.path.abspath(__file__))
    rng = np.random.default_rng(0)
    data = np.clip(rng.integers(0, 4096, (9, 512, 512)).astype(np.int32) - 3500, 0, None).astype(np.uint16)
    dark = np.zeros((512, 512), np.uint16)
    sizes = {}
    for clevel in (6, 1):
        d = tmp_path / ("cl%d" % clevel)
        d.mkdir()
        # (compression_level is read-only on InputParams, as in the reference: the level comes from a copy of the config file)
        text = open(os.path.join(here, "golden", "files", "recode_params_minimal_read_write_test.txt")).read()
        assert "compression_level = 1" in text
        params = d / "params.txt"
        params.write_text(text.replace("compression_level = 1", "compression_level = %d" % clevel))
        for node in range(3):
            ip = InputParams()
            ip.load(str(params))
            assert ip.compression_level == clevel
            ip.nx, ip.ny, ip.nz = 512, 512, 9
            ip.source_data_type = ip.target_data_type = 0
            w = ReCoDeWriter("t", dark_data=dark, output_directory=str(d), input_params=ip, node_id=node, device_zlib=True)
            w.start()
            assert not w._host_compress
            w.run(data)
            w.close()
        merge_parts(str(d), "t.rc1", 3)
        rd = ReCoDeReader(str(d / "t.rc1"))
        rd.open(print_header=False)
        assert rd.get_header().as_dict()["compression_scheme"] == 0
        for z in range(9):
            assert np.array_equal(np.asarray(rd.get_frame(z)[z]["data"].todense()), data[z])
        rd.close()
        sizes[clevel] = os.path.getsize(str(d / "t.rc1"))
    assert sizes[6] < sizes[1], sizes
