"""CPU: the host-side mirror of the reference interface (header, structures, params, reader parsing, merge_parts) against
files written by the reference itself, and the C-ABI library's symbol table.  No compute entry point is called."""
import os
import re
import shutil
import struct

import numpy as np
import pytest

from conftest import GOLDEN, REPO, load_npz

FILES = os.path.join(GOLDEN, "files")
CASES = [("l1z12", 1, 3), ("l1z16", 1, 2), ("l1ro16", 1, 2), ("l3z", 3, 2)]


def test_library_exports_every_declared_symbol():
    from pyrecode_amd import _lib
    hdr = open(os.path.join(REPO, "include", "recode_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(rc_[a-z0-9_]+)\s*\(", hdr))
    assert declared and declared == set(_lib.SIGNATURES), declared ^ set(_lib.SIGNATURES)
    L = _lib.lib()  # resolves every symbol; raises AttributeError on a mismatch
    assert L.rc_abi_version() == 3
    assert L.rc_scheme_on_device(2) == 1 and L.rc_scheme_on_device(0) == 0
    assert L.rc_strerror(-5).decode() == "Buffer size smaller than compressed data size"


def test_ctx_arguments_are_checked_before_any_device_is_touched():
    """rc_ctx_create refuses what no launch could take - with or without a GPU: zero sizes, a batch beyond a launch's grid.y, depths beyond 32."""
    from pyrecode_amd import _lib
    for kw, pat in ((dict(max_batch=0), "max_batch"), (dict(max_batch=65536), "65535"), (dict(nx=0), "nx"), (dict(depth=33), "source_bit_depth")):
        a = dict(nx=64, ny=64, depth=12, max_batch=4)
        a.update(kw)
        with pytest.raises((_lib.RecodeHipError, ValueError, NotImplementedError), match=pat):
            _lib.ReduceContext(a["nx"], a["ny"], a["depth"], max_batch=a["max_batch"])


def test_no_gpu_means_loud_failure_not_fallback():
    from pyrecode_amd import _lib
    if _lib.device_count() > 0:
        pytest.skip("a GPU is visible")
    with pytest.raises(_lib.RecodeHipError, match="no CPU path"):
        _lib.ReduceContext(64, 64, 12)
    out = np.zeros(8, np.uint8)
    vals = np.arange(4, dtype=np.uint16)
    with pytest.raises(_lib.RecodeHipError):
        _lib.check(_lib.lib().rc_bit_pack(vals.ctypes.data, 4, 12, out.ctypes.data, 6))
    # every other stateless compute entry point: RC_ERR_DEVICE, nothing computed on the host
    import ctypes as C
    L = _lib.lib()
    n = C.c_uint64(0)
    src = np.zeros(64, np.uint8)
    big = np.zeros(4096, np.uint8)
    u64 = np.zeros(64, np.uint64)
    sizes = np.array([[8, 8, 8]], np.uint32)
    for scheme in (1, 2, 8):
        assert L.rc_compress(scheme, 1, src.ctypes.data, src.size, big.ctypes.data, big.size, C.byref(n)) == _lib.RC_ERR_DEVICE
        assert L.rc_decompress(scheme, src.ctypes.data, src.size, big.ctypes.data, big.size, C.byref(n)) == _lib.RC_ERR_DEVICE
    assert L.rc_bit_unpack(src.ctypes.data, 6, 4, 12, u64.ctypes.data) == _lib.RC_ERR_DEVICE
    assert L.rc_unpack_frame_sparse(8, 8, 12, src.ctypes.data, src.ctypes.data, 6, u64.ctypes.data, 16, 1) == _lib.RC_ERR_DEVICE
    assert L.rc_expand_frames(8, 8, 12, 1, 0, 0, src.ctypes.data, sizes.ctypes.data, 1, u64.ctypes.data, u64.ctypes.data + 64, 4) == _lib.RC_ERR_DEVICE
    assert L.rc_expand_frames_submit(0, 8, 8, 12, 1, 0, 0, src.ctypes.data, sizes.ctypes.data, 1, u64.ctypes.data, 4) == _lib.RC_ERR_DEVICE


def test_product_never_imports_the_oracle():
    pkg = os.path.join(REPO, "pyrecode_amd")
    for root, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h")):
                text = open(os.path.join(root, f)).read()
                assert "import oracle" not in text and "from oracle" not in text and "librecode_oracle" not in text, f


@pytest.mark.parametrize("tag,level,nodes", CASES)
def test_header_roundtrip_and_offsets(tag, level, nodes):
    from pyrecode_amd.recode_header import ReCoDeHeader
    path = os.path.join(FILES, "g3_%s.rc%d_part000" % (tag, level))
    raw = open(path, "rb").read(512)
    h = ReCoDeHeader()
    h.load(path)
    assert h.recode_header_length == 512 and h.to_bytes() == raw
    d = h.as_dict()
    # SURVEY §8f-N3 offsets
    assert struct.unpack_from("<Q", raw, 0)[0] == 158966344846346 == d["uid"]
    assert (raw[8], raw[9], raw[10], raw[11], raw[12], raw[13]) == (0, 2, 1, level, d["rc_operation_mode"], 1)
    assert struct.unpack_from("<III", raw, 15) == (d["nx"], d["ny"], d["nz"])
    assert h.get_field_position_in_bytes("nz") == 23 and h.get_field_position_in_bytes("source_file_name") == 37
    assert h.get_field_position_in_bytes("source_bit_depth") == 258 and raw[258] == d["source_bit_depth"]
    assert d["source_file_name"] == ("g3_" + tag).ljust(100)
    assert h.get_frame_data_offset(True, 12) == 512 and h.get_frame_data_offset(False, 12) == 512 + 12 * d["nz"]


@pytest.mark.parametrize("tag,level,nodes", CASES)
def test_header_create_matches_reference_bytes(tag, level, nodes, tmp_path):
    from pyrecode_amd.params import InitParams, InputParams
    from pyrecode_amd.recode_header import ReCoDeHeader
    g = load_npz("g3_%s.npz" % tag)
    cfg = tmp_path / "p.txt"
    cfg.write_text("".join("%s = %d\n" % (k, int(v)) for k, v in zip(g["cfg_keys"].tolist(), g["cfg_vals"])))
    ip = InputParams()
    ip.load(str(cfg))
    assert ip.validate()
    init = InitParams("batch", str(tmp_path), image_filename="g3_" + tag)
    h = ReCoDeHeader()
    h.create(init, ip, True)
    h.set("source_header_length", 0)
    assert h.validate()
    # the part header's nz is rewritten at close() with the frames that node wrote
    ref = open(os.path.join(FILES, "g3_%s.rc%d_part000" % (tag, level)), "rb").read(512)
    h.update("nz", struct.unpack_from("<I", ref, 23)[0])
    assert h.to_bytes() == ref


def test_params_file_of_the_reference_test_loads():
    from pyrecode_amd.params import InputParams
    ip = InputParams()
    ip.load(os.path.join(FILES, "recode_params_minimal_read_write_test.txt"))
    ip.source_data_type = 0
    ip.target_data_type = 0
    assert ip.validate()
    assert (ip.nx, ip.ny, ip.nz, ip.num_threads) == (512, 512, 9, 3)
    assert (ip.reduction_level, ip.rc_operation_mode, ip.compression_scheme, ip.compression_level) == (1, 1, 0, 1)
    assert ip.source_bit_depth == 12 and ip.source_numpy_dtype is np.uint16
    bad = InputParams()
    with pytest.raises(AssertionError, match="Unknown parameter"):
        bad._param_map.pop("num_rows")
        bad.load(os.path.join(FILES, "recode_params_minimal_read_write_test.txt"))


def test_structures_match_reference_layout():
    from pyrecode_amd.structures import ReCoDeStructures
    s = ReCoDeStructures({"nx": 53, "ny": 37})
    assert s.binary_image_sz_bytes == 246
    assert [f["name"] for f in s.standard_frame_metadata_structure_for(1, 1)] == [
        "bytes_in_compressed_binary_map", "bytes_in_compressed_pixvals", "bytes_in_packed_pixvals"]
    assert s.get_standard_frame_metadata_size(1, 1) == 12 and s.get_standard_frame_metadata_size(1, 0) == 4
    assert s.get_standard_frame_metadata_size(3, 1) == 4 and s.get_standard_frame_metadata_size(3, 0) == 0
    md = {"bytes_in_compressed_binary_map": 10, "bytes_in_compressed_pixvals": 20, "bytes_in_packed_pixvals": 99}
    assert s.get_frame_data_size(1, 1, md) == 30
    assert s.get_frame_data_size(1, 0, {"bytes_in_packed_pixvals": 7}) == 246 + 7
    assert s.get_frame_data_size(3, 0, {}) == 246 and s.get_frame_data_size(4, 1, md) == 10


@pytest.mark.parametrize("tag,level,nodes", CASES)
def test_merge_parts_reproduces_reference_merged_file(tag, level, nodes, tmp_path):
    from pyrecode_amd.recode_reader import merge_parts
    base = "g3_%s.rc%d" % (tag, level)
    for i in range(nodes):
        shutil.copy(os.path.join(FILES, "%s_part%03d" % (base, i)), tmp_path)
    merge_parts(str(tmp_path), base, nodes)
    assert (tmp_path / base).read_bytes() == open(os.path.join(FILES, base), "rb").read()


@pytest.mark.parametrize("tag,level,nodes", CASES)
def test_reader_raw_access_and_seek_table(tag, level, nodes):
    from pyrecode_amd.recode_reader import ReCoDeReader
    g = load_npz("g3_%s.npz" % tag)
    nz = g["frames"].shape[0]
    base = os.path.join(FILES, "g3_%s.rc%d" % (tag, level))
    rd = ReCoDeReader(base, is_intermediate=False)
    rd.open(print_header=False)
    assert rd.get_shape() == (nz, g["frames"].shape[1], g["frames"].shape[2])
    merged = open(base, "rb").read()
    start = 512 + nz * rd.sz_frame_metadata
    pieces = []
    for z in range(nz):
        f = rd.get_next_frame_raw()
        (fid, body), = f.items()
        assert fid == z
        blob = b"".join(body["data"].values())
        assert merged[start + int(rd._seek_table[z, 1]):start + int(rd._seek_table[z, 1]) + len(blob)] == blob
        pieces.append(blob)
    assert b"".join(pieces) == merged[start:]
    rd.close()
    # intermediate file: frame ids follow the contiguous-block rule; EOF -> None
    part = ReCoDeReader(base + "_part001", is_intermediate=True)
    part.open(print_header=False)
    ids = []
    while True:
        f = part.get_next_frame_raw(read_data=False)
        if f is None:
            break
        ids.append(int(list(f.keys())[0]))
    per = -(-nz // nodes)
    assert ids == list(range(per, min(2 * per, nz)))
    with pytest.raises(ValueError):
        part.get_frame(0)
    part.close()
    # the batched readers' index of a part file (one walk over the record headers): same ids, metadata rows and data positions as the
    # sequential walk; a file cut in the middle of its last record indexes the whole records only; the sequential cursor is left alone
    for node in range(nodes):
        path = base + "_part%03d" % node
        part = ReCoDeReader(path, is_intermediate=True)
        part.open(print_header=False)
        seq = []
        while True:
            f = part.get_next_frame_raw(read_data=False)
            if f is None:
                break
            (fid, body), = f.items()
            seq.append((int(fid), {k: int(v) for k, v in body["metadata"].items()}, part.get_file_position()))
        part.close()
        part = ReCoDeReader(path, is_intermediate=True)
        part.open(print_header=False)
        first = part.get_next_frame_raw(read_data=False)
        here = part.get_file_position()
        assert part._batch_frames() == len(seq) and part.get_file_position() == here
        assert part.part_frame_ids.tolist() == [q[0] for q in seq]
        for z, (fid, md, end) in enumerate(seq):
            assert {k: int(v) for k, v in part._frame_metadata[z].items()} == md
            assert part._frame_data_start_position + int(part._seek_table[z, 1]) + int(part._seek_table[z, 0]) == end
        part.close()
    whole = open(base + "_part000", "rb").read()
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        cut = os.path.join(tmp, "cut.rc%d_part000" % level)
        with open(cut, "wb") as f:
            f.write(whole[:-3])
        part = ReCoDeReader(cut, is_intermediate=True)
        part.open(print_header=False)
        full = ReCoDeReader(base + "_part000", is_intermediate=True)
        full.open(print_header=False)
        assert part._batch_frames() == full._batch_frames() - 1
        part.close()
        full.close()


def test_writer_constructor_validation(tmp_path):
    from pyrecode_amd.params import InputParams
    from pyrecode_amd.recode_writer import ReCoDeWriter
    g = load_npz("g3_l1z12.npz")
    cfg = tmp_path / "p.txt"
    cfg.write_text("".join("%s = %d\n" % (k, int(v)) for k, v in zip(g["cfg_keys"].tolist(), g["cfg_vals"])))

    def params(**over):
        ip = InputParams()
        ip.load(str(cfg))
        for k, v in over.items():
            ip._param_map[k] = v
        return ip
    with pytest.raises(RuntimeError, match="different shapes"):
        ReCoDeWriter("x", dark_data=np.zeros((3, 3), np.uint16), output_directory=str(tmp_path), input_params=params())
    with pytest.raises(ValueError, match="Invalid input params"):
        ReCoDeWriter("x", dark_data=g["dark"], output_directory=str(tmp_path), input_params=params(reduction_level=7))
    with pytest.raises(ValueError, match="Invalid initialization parameters"):
        ReCoDeWriter("x", dark_data=g["dark"], output_directory="", input_params=params())
    with pytest.raises(NotImplementedError):
        ReCoDeWriter("x", dark_data=g["dark"], output_directory=str(tmp_path), input_params=params(reduction_level=4))
    w = ReCoDeWriter("x", dark_data=g["dark"], output_directory=str(tmp_path), input_params=params())
    assert w._header["nx"] == 56 and w._header["is_intermediate"] is True


def test_compressor_seam_host_schemes_and_errors():
    from pyrecode_amd import recode_compressors as rcmp
    data = bytes(range(256)) * 8
    for scheme in (0, 4, 5):
        c = rcmp.compress(scheme, 1, data, None)
        assert rcmp.de_compress(scheme, c, None) == data
    import zlib
    assert rcmp.compress(0, 1, data, None) == zlib.compress(data, 1)
    with pytest.raises(NotImplementedError):
        rcmp.compress(12, 1, data, None)
    with pytest.raises(NotImplementedError):
        rcmp.de_compress(99, data, None)
    assert rcmp.import_checks({"compression_scheme": 0}) and rcmp.import_checks({"compression_scheme": 2})


def test_merge_interleaves_stream_mode_parts_by_frame_id(tmp_path):
    """Fixture G7: part files the reference's writer produced in mode='stream' (chunks of 5, 4, 1, 6 frames on 2 nodes: ids
    [0,1,2,5,6,9,10,11,12] and [3,4,7,8,13,14,15]).  merge_parts is a real k-way merge by frame id - the reference's own keeps the POPPED
    id as a part's next key and would emit 0,1,2,5,...: frame z of the merged file is the record with id z."""
    from pyrecode_amd.recode_reader import ReCoDeReader, merge_parts
    g = load_npz("g7_stream.npz")
    by_id = {}
    for node in range(2):
        fn = "g7_stream.rc1_part%03d" % node
        shutil.copy(os.path.join(FILES, fn), tmp_path / fn)
        part = ReCoDeReader(str(tmp_path / fn), is_intermediate=True)
        part.open(print_header=False)
        ids = []
        while True:
            f = part.get_next_frame_raw()
            if f is None:
                break
            (fid, body), = f.items()
            ids.append(int(fid))
            by_id[int(fid)] = ({k: int(v) for k, v in body["metadata"].items()}, b"".join(body["data"].values()))
        assert ids == g["ids_part%d" % node].tolist()
        part.close()
    merge_parts(str(tmp_path), "g7_stream.rc1", 2)
    rd = ReCoDeReader(str(tmp_path / "g7_stream.rc1"), is_intermediate=False)
    rd.open(print_header=False)
    nz = g["frames"].shape[0]
    assert rd.get_shape()[0] == nz == len(by_id)
    for z in range(nz):
        (fid, body), = rd.get_next_frame_raw().items()
        assert fid == z
        assert {k: int(v) for k, v in body["metadata"].items()} == by_id[z][0]
        assert b"".join(body["data"].values()) == by_id[z][1], "frame %d" % z
    rd.close()


@pytest.mark.parametrize("host_decoded", [False, True])
def test_readahead_state_machine_without_a_gpu(monkeypatch, host_decoded):
    """ReCoDeReader._readahead_frame (the frame-at-a-time calls served from batches fetched ahead) with the batched call stubbed at
    get_frames_triplets: it starts with the third call in sequence, moves from batch to batch, drops its window on a jump, leaves empty
    frames and the frame counter / file position to the frame-at-a-time path, and turns itself off when a batch fails."""
    from pyrecode_amd.recode_reader import ReCoDeReader, _BatchOut
    g = load_npz("g3_l1z12.npz")
    frames, dark = g["frames"], g["dark"]
    want = np.where(frames > dark, frames - dark, 0).astype(np.uint16)
    nz = frames.shape[0]
    rd = ReCoDeReader(os.path.join(FILES, "g3_l1z12.rc1"), is_intermediate=False)
    rd.open(print_header=False)
    rd._RA_FRAMES = 3
    calls = []

    def fake(z0, n, out=None, coo=False):
        assert coo and out is rd._ra_buf
        calls.append((z0, n))
        rows, cols, vals, prefix = [], [], [], np.zeros(n + 1, np.uint64)
        for i in range(n):
            r, c = np.nonzero(want[z0 + i]) if z0 + i != 5 else (np.zeros(0, np.int64), np.zeros(0, np.int64))   # frame 5 pretends to be empty
            rows.append(r.astype(np.int32)); cols.append(c.astype(np.int32)); vals.append(want[z0 + i][r, c])
            prefix[i + 1] = prefix[i] + r.size
        rd.last_batch_path = "device"
        rd._current_frame_index = 99                     # (what a batched call leaves behind: the caller must not see it)
        rd._fp.seek(7, 0)
        return prefix, (np.concatenate(rows), np.concatenate(cols), np.concatenate(vals))
    def fake_iter(z0, n, batch, coo=False):              # the host-decoded pipeline (zlib files, stock-encoder files), batch by batch
        assert coo
        for a in range(z0, z0 + n, batch):
            k = min(batch, z0 + n - a)
            yield (a,) + fake(a, k, out=rd._ra_buf, coo=True)
    monkeypatch.setattr(rd, "get_frames_triplets", fake)
    monkeypatch.setattr(rd, "_iter_frames_impl", fake_iter)          # (what the read-ahead drives: the public iterator's body)
    if not host_decoded:
        rd._header["compression_scheme"] = 1             # (a file of this library's own zstd streams ...
        rd._RA_PIPELINED = False                         #  ... through the other form: one synchronous batched call per window)
    rd._current_frame_index = 3
    rd._fp.seek(123, 0)
    assert rd._readahead_frame(0) is None and rd._readahead_frame(1) is None and calls == []
    m = rd._readahead_frame(2)
    assert calls == [(2, 3)] and np.array_equal(np.asarray(m.todense()), want[2]) and m.dtype == np.uint16
    assert rd._current_frame_index == 3 and rd._fp.tell() == 123               # put back
    assert np.array_equal(np.asarray(rd._readahead_frame(3).todense()), want[3]) and calls == [(2, 3)]
    assert np.array_equal(np.asarray(rd._readahead_frame(4).todense()), want[4]) and calls == [(2, 3)]
    assert rd._readahead_frame(5) is None and calls == [(2, 3), (5, 3)]          # the next batch; the empty frame is not served
    assert np.array_equal(np.asarray(rd._readahead_frame(6).todense()), want[6]) and rd.readahead_frames_served == 4
    assert rd._readahead_frame(1) is None and rd._ra is None                     # a jump back: window dropped, streak restarts
    assert rd._readahead_frame(2) is None
    assert np.array_equal(np.asarray(rd._readahead_frame(3).todense()), want[3]) and calls[-1] == (3, 3)
    assert rd._readahead_frame(7) is None and rd._ra is None and calls[-1] == (3, 3)     # a jump ahead, past the window's end: dropped as well
    assert rd._readahead_frame(6) is None                                          # (backwards again)

    def failing(z0, n, out=None, coo=False):
        raise ValueError("a damaged stream")
    def failing_iter(z0, n, batch, coo=False):
        raise ValueError("a damaged stream")
        yield
    monkeypatch.setattr(rd, "get_frames_triplets", failing)
    monkeypatch.setattr(rd, "_iter_frames_impl", failing_iter)
    rd._ra, rd._ra_last, rd._ra_streak = None, 0, 1
    assert rd._readahead_frame(1) is None and rd._ra_off is True
    assert rd._readahead_frame(2) is None
    rd.close()
    # the layout helper: triplet rows / the three COO arrays inside one buffer of `cap` entries
    buf = np.arange(10 * 7, dtype=np.uint8)
    r, c, v = _BatchOut.views(buf, 7, 5, True)
    assert r.dtype == np.int32 and r.size == 5 and r.ctypes.data == buf.ctypes.data
    assert c.ctypes.data == buf.ctypes.data + 4 * 7 and v.dtype == np.uint16 and v.ctypes.data == buf.ctypes.data + 8 * 7 and v.size == 5
    t = _BatchOut.views(np.zeros(24 * 7, np.uint8), 7, 5, False)
    assert t.shape == (5, 3) and t.dtype == np.uint64
    tr = np.array([[1, 2, 3], [4, 5, 70000]], np.uint64)
    rr, cc, vv = _BatchOut.from_triplets(tr, True)
    assert rr.tolist() == [1, 4] and cc.tolist() == [2, 5] and vv.dtype == np.uint16 and _BatchOut.from_triplets(tr, False) is tr


def test_batched_access_on_an_empty_part_file(tmp_path):
    """a part file that holds its header and nothing else (a writer whose block of the stack was empty): no frames, no batches, None"""
    from pyrecode_amd.recode_reader import ReCoDeReader
    src = open(os.path.join(FILES, "g3_l1z12.rc1_part000"), "rb").read()
    p = tmp_path / "empty.rc1_part000"
    p.write_bytes(src[:512])
    rd = ReCoDeReader(str(p), is_intermediate=True)
    rd.open(print_header=False)
    assert rd._batch_frames() == 0 and rd.part_frame_ids.size == 0
    assert list(rd.iter_frames_triplets(batch=4)) == [] and list(rd.iter_frames_coo(batch=4)) == []
    assert rd.get_next_frame() is None
    with pytest.raises(ValueError):
        rd.get_frames_triplets(0, 1)
    rd.close()


def test_frames_of_4_gib_and_more_are_refused_before_any_gpu_work():
    """A record may be as large as its raw frame and every size in a record is a u32 (structures.py:18-46): nx * ny * bytes_per_pixel >= 2^32 cannot
    be represented.  rc_ctx_create says so (RC_ERR_UNSUPPORTED -> NotImplementedError) instead of wrapping - argument checks come before the
    device is looked for, so this runs without a GPU."""
    import ctypes as C
    from pyrecode_amd import _lib
    L = _lib.lib()
    st = C.c_int(0)
    for nx, ny in ((50000, 50000), (65535, 32769), (46341, 46341)):          # uint16: 2 * nx * ny >= 2^32
        assert not L.rc_ctx_create(nx, ny, 16, 1, 1, 2, 1, 0, 4, C.byref(st))
        assert st.value == _lib.RC_ERR_UNSUPPORTED, (nx, ny, st.value)
        assert b"4 GiB" in L.rc_last_error()
    with pytest.raises(NotImplementedError):
        _lib.ReduceContext(50000, 50000, 16, 1, 1, 2, 1, 0, max_batch=1)
    assert not L.rc_ctx_create(70000, 70000, 16, 1, 1, 2, 1, 0, 4, C.byref(st)) and st.value == _lib.RC_ERR_BAD_ARG   # nx * ny itself >= 2^32
    if _lib.device_count() > 0:   # (the refusals above hold everywhere; the last line needs a host without a device)
        pytest.skip("a device is present: a 46340 x 46340 ctx would allocate ~45 GB there instead of failing with RC_ERR_DEVICE")
    assert not L.rc_ctx_create(46340, 46340, 16, 1, 1, 2, 1, 0, 4, C.byref(st)) and st.value == _lib.RC_ERR_DEVICE    # representable: only the GPU is missing here


def test_out_of_memory_has_a_status_and_an_exception_of_its_own():
    from pyrecode_amd import _lib
    assert _lib.lib().rc_strerror(_lib.RC_ERR_WORKSPACE) == b"out of device memory for the ctx's workspace"
    import pyrecode_amd._lib as m
    orig = m.last_error
    m.last_error = lambda: "hipMalloc"
    try:
        with pytest.raises(MemoryError):
            _lib.check(_lib.RC_ERR_WORKSPACE, "rc_ctx_create")
    finally:
        m.last_error = orig


def _recording_driver(monkeypatch, njobs, finish_raises_at=None, stop_at=None):
    """BatchedAccess._two_slots over njobs jobs of 3 frames each with recording fakes: (the generator, its jobs, the log)"""
    from pyrecode_amd import reader_batched as rb
    log = []

    class Bare(rb.BatchedAccess):
        def _note_batch_end(self, z):
            log.append(("note", z))
    jobs = rb._jobs(10, 3 * njobs, 3)

    def start(job):
        log.append(("start", jobs.index(job), job.slot))
        job.queued = True

    def finish(job):
        log.append(("finish", jobs.index(job)))
        job.queued = False
        if jobs.index(job) == finish_raises_at:
            raise ValueError("finish %d" % jobs.index(job))
        return "item %d" % jobs.index(job)
    monkeypatch.setattr(rb, "_drain", lambda job: log.append(("drain", jobs.index(job))))
    stop = None if stop_at is None else (lambda job: (log.append(("stop?", jobs.index(job))), jobs.index(job) == stop_at)[1])
    return Bare()._two_slots(jobs, start, finish, stop), jobs, log


def test_two_slot_driver_order_slots_and_drain(monkeypatch):
    """The driver of the streaming pipelines (BatchedAccess._two_slots): start(j + 1) runs before finish(j), job j goes through slot j & 1,
    the frame counter is noted after finish and before the item is handed out, and however the generator ends a job that is still queued
    is drained - once."""
    gen, jobs, log = _recording_driver(monkeypatch, 0)
    assert list(gen) == [] and log == []
    gen, jobs, log = _recording_driver(monkeypatch, 1)
    assert list(gen) == ["item 0"] and log == [("start", 0, 0), ("finish", 0), ("note", 13)]
    gen, jobs, log = _recording_driver(monkeypatch, 3)
    assert [(j.first, j.count) for j in jobs] == [(10, 3), (13, 3), (16, 3)]
    assert next(gen) == "item 0"
    assert log == [("start", 0, 0), ("start", 1, 1), ("finish", 0), ("note", 13)]              # noted before the item is handed out
    assert list(gen) == ["item 1", "item 2"]
    assert [e for e in log if e[0] in ("start", "finish")] == [("start", 0, 0), ("start", 1, 1), ("finish", 0), ("start", 2, 0), ("finish", 1),
                                                               ("finish", 2)]
    assert [j.slot for j in jobs] == [0, 1, 0] and not any(e[0] == "drain" for e in log)
    # closed after the first item: job 1 is queued and is drained, once
    gen, jobs, log = _recording_driver(monkeypatch, 3)
    assert next(gen) == "item 0"
    gen.close()
    assert [e for e in log if e[0] == "drain"] == [("drain", 1)] and ("start", 2, 0) not in log
    # finish raises: the job queued behind it is still drained, and the exception reaches the caller
    gen, jobs, log = _recording_driver(monkeypatch, 3, finish_raises_at=0)
    with pytest.raises(ValueError, match="finish 0"):
        next(gen)
    assert log == [("start", 0, 0), ("start", 1, 1), ("finish", 0), ("drain", 1)]
    # the stop hook, asked before the next job is started: the queued job is drained, not finished, and the driver ends
    gen, jobs, log = _recording_driver(monkeypatch, 3, stop_at=1)
    assert list(gen) == ["item 0"]
    assert log == [("start", 0, 0), ("stop?", 0), ("start", 1, 1), ("finish", 0), ("note", 13), ("stop?", 1), ("drain", 1)]


def test_drain_waits_only_for_a_queued_job(monkeypatch):
    """the drain routine proper: a job that is not queued (never submitted, or already waited for) costs no device call"""
    from pyrecode_amd import reader_batched as rb
    waited = []
    monkeypatch.setattr(rb, "_wait", lambda job: waited.append(job.first))
    job = rb._Job(4, 2)
    rb._drain(None)
    rb._drain(job)
    assert waited == []
    job.queued = True
    rb._drain(job)
    assert waited == [4]


def _recording_ladder(monkeypatch, dev, queued=0, wait=0, sync=0, queues=True, stock=True, host_decodes=True, slot_taken=False):
    """The ladder of the 'sum' route family (BatchedAccess._offer / _settle) with a recording fake kind and a reader of fakes, over three
    jobs of two frames: (the reader, the kind, the jobs, the log).  dev: the scheme the route offers under (None: never offered); queued,
    wait, sync: the statuses the queued call, the verdict and the synchronous call under the FILE's geometry answer (the stored pieces'
    calls, op_mode 0, always succeed); slot_taken: the queued call answers as when another reader holds the slot.  The file: 8 x 4,
    12 bits, level 1, op_mode 1, scheme 2 - so (1, dev) marks a call on the file's bytes, (0, 2) one on host-decoded pieces and (0, 0)
    one on _stored_pieces_per_frame's."""
    from types import SimpleNamespace
    from pyrecode_amd import _lib, reader_batched as rb
    log = []
    pieces, sizes0 = np.zeros(4, np.uint8), np.zeros((2, 3), np.uint32)

    class Bare(rb.BatchedAccess):
        _header = dict(nx=8, ny=4, target_bit_depth=12, reduction_level=1, rc_operation_mode=1, compression_scheme=2)
        _foreign_file, last_batch_path, _ra, _user_iters = False, None, None, 0

        def __init__(self):
            self._bufs = SimpleNamespace(stream=[None] * 4, pin_blob=None)

        def _close_ra_iter(self):
            pass

        def _note_batch_end(self, z):
            pass

        def _route_for(self, family, device_blosc=False, device_zlib=False):
            assert family == 'sum'
            return ('device', dev) if dev is not None else ('host-decode' if stock else 'per-frame', None)

        def _batch_sizes(self, a, k, frames=None):
            return np.zeros((k, 3), np.uint32), 16

        def _read_batch_into(self, blob, z0, n, move_fp=True):
            log.append(("read", (z0 - 10) // 2, blob.size))

        def _host_decode_batch(self, blob, sizes, n, slot):
            log.append(("host-decode", slot))
            return (pieces, sizes0) if host_decodes else None

        def _stored_pieces_per_frame(self, a, k, frames=None):
            log.append(("frame by frame", a, k))
            return (8, 4, 12, 1, 0, 0), pieces, sizes0
    jobs = rb._jobs(10, 6, 2)

    class Kind(rb._Kind):
        what = "fake_call"
        args = {}

        def queues(self, level):
            return queues

        def room(self, job, geom, sizes, k):
            log.append(("room", jobs.index(job)) + tuple(geom[4:]))

        def call(self, job, geom, data, sizes, k, slot=None):
            log.append(("call", jobs.index(job), "sync" if slot is None else "slot %d" % slot) + tuple(geom[4:]))
            self.args.setdefault(jobs.index(job), []).append((geom, data.ctypes.data, sizes.ctypes.data, k))
            assert tuple(geom[:4]) == (8, 4, 12, 1) and k == job.count == 2
            return 0 if geom[4] == 0 else sync if slot is None else _lib.RC_ERR_BAD_ARG if slot_taken else queued

        def item(self, job):
            return "item %d" % jobs.index(job)

    def wait_(job):
        log.append(("wait", jobs.index(job)))
        job.queued = False
        return wait, np.zeros(job.count + 1, np.uint64)
    monkeypatch.setattr(rb, "_pinned", lambda buf, nbytes: buf if buf is not None else SimpleNamespace(array=np.zeros(nbytes, np.uint8)))
    monkeypatch.setattr(rb, "_wait", wait_)
    monkeypatch.setattr(rb, "_stock_decoded", lambda h: stock)
    monkeypatch.setattr(_lib, "last_error", lambda: "slot 0 holds a submitted batch" if slot_taken else "")
    return Bare(), Kind(), jobs, log


def test_the_ladder_of_the_sum_family_rung_by_rung(monkeypatch):
    """One ladder for every kind of result of the 'sum' route family: which calls the kind receives - queued or synchronous, under which
    geometry's (op_mode, scheme) -, last_batch_path and _foreign_file for every rung, in the streaming form (_ladder on _two_slots) and in
    the synchronous one (what get_frames_dense uses)."""
    from pyrecode_amd import _lib
    UNS, BAD, DEVICE = _lib.RC_ERR_UNSUPPORTED, _lib.RC_ERR_CORRUPT, _lib.RC_ERR_DEVICE
    items = ["item 0", "item 1", "item 2"]

    def calls(log, j=None):
        return [e for e in log if e[0] in ("call", "host-decode", "frame by frame") and (j is None or e[1] == j or e[0] != "call")]
    # queued, and the wait says OK: 'device'; the file bytes are read, then the output is sized, then the batch is offered, and job j + 1
    # is offered before job j is waited for
    r, kind, jobs, log = _recording_ladder(monkeypatch, dev=2)
    assert list(r._ladder(kind, jobs)) == items and (r.last_batch_path, r._foreign_file, r._user_iters) == ("device", False, 0)
    start = lambda j: [("read", j, 16), ("room", j, 1, 2), ("call", j, "slot %d" % (j & 1), 1, 2)]
    assert log == start(0) + start(1) + [("wait", 0)] + start(2) + [("wait", 1), ("wait", 2)] and not any(j.queued for j in jobs)
    r, kind, jobs, log = _recording_ladder(monkeypatch, dev=_lib.RC_SCHEME_ZLIB_DEVICE)
    assert list(r._ladder(kind, jobs)) == items and (r.last_batch_path, r._foreign_file) == ("device-inflate", False)
    # queued, the wait says UNSUPPORTED, the host decode delivers: the same call on the stored pieces, and the file is marked
    r, kind, jobs, log = _recording_ladder(monkeypatch, dev=2, wait=UNS)
    gen = r._ladder(kind, jobs)
    assert next(gen) == "item 0" and r._user_iters == 1
    assert (r.last_batch_path, r._foreign_file) == ("host-decode + device-expand", True)
    assert [e for e in log if e[1:2] == (0,) or e[0] == "host-decode"] == [
        ("read", 0, 16), ("room", 0, 1, 2), ("call", 0, "slot 0", 1, 2), ("wait", 0), ("host-decode", 2), ("room", 0, 0, 2), ("call", 0, "sync", 0, 2)]
    assert list(gen) == items[1:] and r._user_iters == 0 and not any(e[0] == "frame by frame" for e in log)
    # the submit says CORRUPT, no stock decoder for the file: frame by frame, nothing waited for, the file is not marked
    r, kind, jobs, log = _recording_ladder(monkeypatch, dev=2, queued=BAD, stock=False)
    assert list(r._ladder(kind, jobs)) == items and (r.last_batch_path, r._foreign_file) == ("per-frame", False)
    assert [e for e in log if e[1:2] == (1,) or e[0] == "frame by frame" and e[1] == 12] == [
        ("read", 1, 16), ("room", 1, 1, 2), ("call", 1, "slot 1", 1, 2), ("frame by frame", 12, 2), ("room", 1, 0, 0), ("call", 1, "sync", 0, 0)]
    assert not any(e[0] in ("wait", "host-decode") for e in log) and not any(j.queued for j in jobs)
    # ... and a stock decoder that gives up leads to the same rung
    r, kind, jobs, log = _recording_ladder(monkeypatch, dev=2, wait=BAD, host_decodes=False)
    assert list(r._ladder(kind, jobs)) == items and (r.last_batch_path, r._foreign_file) == ("per-frame", False)
    assert calls(log, 2)[-3:] == [("host-decode", 2), ("frame by frame", 14, 2), ("call", 2, "sync", 0, 0)]
    # never offered, the host decode delivers: no call under the file's geometry, the file is not marked
    r, kind, jobs, log = _recording_ladder(monkeypatch, dev=None)
    assert list(r._ladder(kind, jobs)) == items and (r.last_batch_path, r._foreign_file) == ("host-decode + device-expand", False)
    assert [e for e in log if e[0] != "read"] == [e for j in range(3) for e in (("host-decode", 2), ("room", j, 0, 2), ("call", j, "sync", 0, 2))]
    # another reader holds the slot: one queued attempt, then the synchronous call with the same arguments, whose status is the verdict
    r, kind, jobs, log = _recording_ladder(monkeypatch, dev=2, slot_taken=True)
    assert list(r._ladder(kind, jobs)) == items and (r.last_batch_path, r._foreign_file) == ("device", False)
    assert [e for e in log if e[0] != "read"] == [e for j in range(3) for e in (("room", j, 1, 2), ("call", j, "slot %d" % (j & 1), 1, 2), ("call", j, "sync", 1, 2))]
    assert all(len(a) == 2 and a[0] == a[1] for a in kind.args.values()) and not any(j.queued for j in jobs)
    r, kind, jobs, log = _recording_ladder(monkeypatch, dev=2, slot_taken=True, sync=UNS)
    assert list(r._ladder(kind, jobs)) == items and (r.last_batch_path, r._foreign_file) == ("host-decode + device-expand", True)
    # a kind that does not queue this level: no queued attempt at all
    r, kind, jobs, log = _recording_ladder(monkeypatch, dev=2, queues=False)
    assert list(r._ladder(kind, jobs)) == items and r.last_batch_path == "device"
    assert [e for e in log if e[0] == "call"] == [("call", j, "sync", 1, 2) for j in range(3)] and not any(e[0] == "wait" for e in log)
    # a status outside OK / UNSUPPORTED / CORRUPT - of the submit, of the verdict, of the synchronous offer - raises, and no decoder is asked
    for kw in (dict(queued=DEVICE), dict(wait=DEVICE), dict(sync=DEVICE, queues=False), dict(sync=DEVICE, slot_taken=True)):
        r, kind, jobs, log = _recording_ladder(monkeypatch, dev=2, **kw)
        with pytest.raises(_lib.RecodeHipError, match="fake_call_submit" if "queued" in kw else "rc_expand_frames_wait"):
            list(r._ladder(kind, jobs))
        assert r.last_batch_path is None and not r._foreign_file and r._user_iters == 0, kw
        assert not any(e[0] in ("host-decode", "frame by frame") for e in log) and not any(j.queued for j in jobs), kw
    # the synchronous form walks the same rungs, on the synchronous calls' blob and with no queued attempt
    for kw, path, foreign, want in (
            (dict(dev=2), "device", False, [("call", 0, "sync", 1, 2)]),
            (dict(dev=_lib.RC_SCHEME_ZLIB_DEVICE), "device-inflate", False, [("call", 0, "sync", 1, _lib.RC_SCHEME_ZLIB_DEVICE)]),
            (dict(dev=2, sync=UNS), "host-decode + device-expand", True, [("call", 0, "sync", 1, 2), ("host-decode", 2), ("call", 0, "sync", 0, 2)]),
            (dict(dev=2, sync=BAD, stock=False), "per-frame", False, [("call", 0, "sync", 1, 2), ("frame by frame", 10, 2), ("call", 0, "sync", 0, 0)]),
            (dict(dev=None), "host-decode + device-expand", False, [("host-decode", 2), ("call", 0, "sync", 0, 2)]),
            (dict(dev=None, stock=False), "per-frame", False, [("frame by frame", 10, 2), ("call", 0, "sync", 0, 0)])):
        r, kind, jobs, log = _recording_ladder(monkeypatch, **kw)
        r._offer(kind, jobs[0], sync=True)
        assert r._settle(kind, jobs[0], sync=True) == "item 0" and (r.last_batch_path, r._foreign_file) == (path, foreign), kw
        assert calls(log) == want and r._bufs.pin_blob is not None and r._bufs.stream == [None] * 4 and not jobs[0].queued, kw
    r, kind, jobs, log = _recording_ladder(monkeypatch, dev=2, sync=DEVICE)
    r._offer(kind, jobs[0], sync=True)
    with pytest.raises(_lib.RecodeHipError, match="fake_call: "):
        r._settle(kind, jobs[0], sync=True)
    assert calls(log) == [("call", 0, "sync", 1, 2)] and r.last_batch_path is None


def test_the_ladder_of_a_kind_with_a_family_a_bottom_rung_and_a_retry_of_its_own(monkeypatch):
    """What the triplets and level-2 kinds add to the ladder, on the recording fakes of the test above (three jobs of two frames, no
    device): the route is asked with the kind's family and switches; a per_frame override is the bottom rung instead of
    _stored_pieces_per_frame; a queued batch whose verdict the kind lists in `retry` goes through the synchronous call once, and that
    call's status is what is judged; `stop` ends the stream once a settled job has marked the file foreign."""
    from pyrecode_amd import _lib, reader_batched as rb
    UNS, BAD, SMALL = _lib.RC_ERR_UNSUPPORTED, _lib.RC_ERR_CORRUPT, _lib.RC_ERR_OUT_TOO_SMALL
    items = ["item 0", "item 1", "item 2"]

    def ladder(family=None, switches=None, per_frame=False, retry=None, asked=None, **kw):
        r, kind, jobs, log = _recording_ladder(monkeypatch, **kw)
        if family is not None:
            kind.family, kind.switches = family, switches
            route = type(r)._route_for
            monkeypatch.setattr(type(r), "_route_for", lambda self, fam, *sw: (asked.append((fam,) + sw), route(self, 'sum'))[1])
        if per_frame:
            kind.per_frame = lambda reader, job: log.append(("per_frame", reader is r, jobs.index(job)))
        if retry is not None:
            kind.retry = retry
        return r, kind, jobs, log
    # family and switches: _route_for receives exactly those, once per job
    asked = []
    r, kind, jobs, log = ladder('triplets', (True, False), asked=asked, dev=2)
    assert list(r._ladder(kind, jobs)) == items and asked == [('triplets', True, False)] * 3 and r.last_batch_path == "device"
    # a per_frame override is called at the bottom rung, _stored_pieces_per_frame is not, and the path is 'per-frame'
    for kw in (dict(dev=2, queued=BAD, stock=False), dict(dev=2, wait=UNS, host_decodes=False), dict(dev=None, stock=False)):
        r, kind, jobs, log = ladder(per_frame=True, **kw)
        assert list(r._ladder(kind, jobs)) == items and (r.last_batch_path, r._foreign_file) == ("per-frame", False), kw
        assert [e for e in log if e[0] == "per_frame"] == [("per_frame", True, j) for j in range(3)], kw
        assert not any(e[0] == "frame by frame" or e[0] == "call" and e[3:] == (0, 0) for e in log), kw
    r, kind, jobs, log = ladder(per_frame=True, dev=2, sync=BAD, stock=False)
    r._offer(kind, jobs[0], sync=True)
    assert r._settle(kind, jobs[0], sync=True) == "item 0" and r.last_batch_path == "per-frame"
    assert [e for e in log if e[0] in ("call", "per_frame", "frame by frame")] == [("call", 0, "sync", 1, 2), ("per_frame", True, 0)]
    # retry: the wait's verdict is listed - exactly one synchronous call follows, with the queued call's arguments, and its status is judged
    r, kind, jobs, log = ladder(retry=(SMALL,), dev=2, wait=SMALL)
    assert list(r._ladder(kind, jobs)) == items and (r.last_batch_path, r._foreign_file) == ("device", False)
    assert [e for e in log if e[1:2] == (1,)] == [("read", 1, 16), ("room", 1, 1, 2), ("call", 1, "slot 1", 1, 2), ("wait", 1), ("call", 1, "sync", 1, 2)]
    assert all(len(a) == 2 and a[0] == a[1] for a in kind.args.values()) and not any(e[0] in ("host-decode", "frame by frame") for e in log)
    r, kind, jobs, log = ladder(retry=(SMALL,), dev=2, wait=SMALL, sync=UNS)            # (the synchronous call's refusal goes down the rungs)
    assert list(r._ladder(kind, jobs)) == items and (r.last_batch_path, r._foreign_file) == ("host-decode + device-expand", True)
    assert [e for e in log if e[0] == "call" and e[1] == 0] == [("call", 0, "slot 0", 1, 2), ("call", 0, "sync", 1, 2), ("call", 0, "sync", 0, 2)]
    r, kind, jobs, log = ladder(retry=(SMALL,), dev=2, wait=SMALL, sync=SMALL)          # (once: the same status from the synchronous call raises)
    with pytest.raises(ValueError, match="rc_expand_frames_wait"):
        list(r._ladder(kind, jobs))
    assert [e for e in log if e[0] == "call" and e[1] == 0] == [("call", 0, "slot 0", 1, 2), ("call", 0, "sync", 1, 2)]
    assert r.last_batch_path is None and not any(j.queued for j in jobs)
    r, kind, jobs, log = ladder(dev=2, wait=SMALL)                                      # (a kind that lists nothing: the verdict raises as it is)
    with pytest.raises(ValueError, match="rc_expand_frames_wait"):
        list(r._ladder(kind, jobs))
    assert not any(e[:3] == ("call", 0, "sync") for e in log)
    # stop: job 0 comes out of the stock decoders and marks the file; job 1, queued meanwhile, is waited for and not delivered
    r, kind, jobs, log = ladder(dev=2, wait=UNS)
    stopped = []
    gen = r._ladder(kind, jobs, stop=lambda job: (stopped.append((jobs.index(job), r._foreign_file)), r._foreign_file)[1])
    assert list(gen) == ["item 0"] and stopped == [(0, False), (1, True)] and r._foreign_file
    assert [e for e in log if e[0] == "wait"] == [("wait", 0), ("wait", 1)] and not any(j.queued for j in jobs)
    assert not any(e[0] in ("read", "room", "call") and e[1] == 2 for e in log) and [e for e in log if e[0] == "call" and e[1] == 1] == [("call", 1, "slot 1", 1, 2)]


# (family, reduction level, operation mode, _foreign_file, then one string per (device_blosc, device_zlib) = (F, F), (F, T), (T, F), (T, T)
# with one letter per compression scheme 0, 1, 2, 4, 5, 8): D = 'device' under the file's scheme, Z = 'device' under RC_SCHEME_ZLIB_DEVICE,
# H = 'host-decode', P = 'per-frame'
ROUTE_TABLE = [
    ('triplets', 1, 0, False, 'DDDDDD', 'DDDDDD', 'DDDDDD', 'DDDDDD'),
    ('triplets', 1, 0, True , 'DDDDDD', 'DDDDDD', 'DDDDDD', 'DDDDDD'),
    ('triplets', 1, 1, False, 'HDDHHP', 'ZDDHHP', 'HDDHHD', 'ZDDHHD'),
    ('triplets', 1, 1, True , 'HHHHHP', 'HHHHHP', 'HHHHHP', 'HHHHHP'),
    ('triplets', 2, 0, False, 'PPPPPP', 'PPPPPP', 'PPPPPP', 'PPPPPP'),
    ('triplets', 2, 0, True , 'PPPPPP', 'PPPPPP', 'PPPPPP', 'PPPPPP'),
    ('triplets', 2, 1, False, 'PPPPPP', 'PPPPPP', 'PPPPPP', 'PPPPPP'),
    ('triplets', 2, 1, True , 'PPPPPP', 'PPPPPP', 'PPPPPP', 'PPPPPP'),
    ('triplets', 3, 0, False, 'DDDDDD', 'DDDDDD', 'DDDDDD', 'DDDDDD'),
    ('triplets', 3, 0, True , 'DDDDDD', 'DDDDDD', 'DDDDDD', 'DDDDDD'),
    ('triplets', 3, 1, False, 'HDDHHP', 'ZDDHHP', 'HDDHHD', 'ZDDHHD'),
    ('triplets', 3, 1, True , 'HHHHHP', 'HHHHHP', 'HHHHHP', 'HHHHHP'),
    ('l2'      , 1, 0, False, 'DDDDDD', 'DDDDDD', 'DDDDDD', 'DDDDDD'),
    ('l2'      , 1, 0, True , 'DDDDDD', 'DDDDDD', 'DDDDDD', 'DDDDDD'),
    ('l2'      , 1, 1, False, 'PDDPPD', 'PDDPPD', 'PDDPPD', 'PDDPPD'),
    ('l2'      , 1, 1, True , 'PPPPPP', 'PPPPPP', 'PPPPPP', 'PPPPPP'),
    ('l2'      , 2, 0, False, 'DDDDDD', 'DDDDDD', 'DDDDDD', 'DDDDDD'),
    ('l2'      , 2, 0, True , 'DDDDDD', 'DDDDDD', 'DDDDDD', 'DDDDDD'),
    ('l2'      , 2, 1, False, 'PDDPPD', 'PDDPPD', 'PDDPPD', 'PDDPPD'),
    ('l2'      , 2, 1, True , 'PPPPPP', 'PPPPPP', 'PPPPPP', 'PPPPPP'),
    ('l2'      , 3, 0, False, 'DDDDDD', 'DDDDDD', 'DDDDDD', 'DDDDDD'),
    ('l2'      , 3, 0, True , 'DDDDDD', 'DDDDDD', 'DDDDDD', 'DDDDDD'),
    ('l2'      , 3, 1, False, 'PDDPPD', 'PDDPPD', 'PDDPPD', 'PDDPPD'),
    ('l2'      , 3, 1, True , 'PPPPPP', 'PPPPPP', 'PPPPPP', 'PPPPPP'),
    ('sum'     , 1, 0, False, 'DDDDDD', 'DDDDDD', 'DDDDDD', 'DDDDDD'),
    ('sum'     , 1, 0, True , 'DDDDDD', 'DDDDDD', 'DDDDDD', 'DDDDDD'),
    ('sum'     , 1, 1, False, 'ZDDHHD', 'ZDDHHD', 'ZDDHHD', 'ZDDHHD'),
    ('sum'     , 1, 1, True , 'HHHHHP', 'HHHHHP', 'HHHHHP', 'HHHHHP'),
    ('sum'     , 2, 0, False, 'DDDDDD', 'DDDDDD', 'DDDDDD', 'DDDDDD'),
    ('sum'     , 2, 0, True , 'DDDDDD', 'DDDDDD', 'DDDDDD', 'DDDDDD'),
    ('sum'     , 2, 1, False, 'PDDPPD', 'PDDPPD', 'PDDPPD', 'PDDPPD'),
    ('sum'     , 2, 1, True , 'PPPPPP', 'PPPPPP', 'PPPPPP', 'PPPPPP'),
    ('sum'     , 3, 0, False, 'DDDDDD', 'DDDDDD', 'DDDDDD', 'DDDDDD'),
    ('sum'     , 3, 0, True , 'DDDDDD', 'DDDDDD', 'DDDDDD', 'DDDDDD'),
    ('sum'     , 3, 1, False, 'ZDDHHD', 'ZDDHHD', 'ZDDHHD', 'ZDDHHD'),
    ('sum'     , 3, 1, True , 'HHHHHP', 'HHHHHP', 'HHHHHP', 'HHHHHP'),
]


@pytest.mark.parametrize("row", ROUTE_TABLE, ids=lambda r: "%s-L%d-m%d-%s" % (r[0].strip(), r[1], r[2], "foreign" if r[3] else "own"))
def test_route_table(row):
    """reader_batched._route against the table above.  The table was filled once by evaluating, for every combination, the expressions
    the readers carried before there was one route function (zdev / fast / host_only of get_frames_triplets, which the two conditions of
    the streaming iterator agreed with; _l2_on_device; _sum_device_scheme and the host-decode condition of the summed views' finish) - it
    records that behaviour, it is not derived from _route.  Fields of 12 bits throughout; the level-2 family's limits of 8 and 16 bits
    are checked at the end.  One cell differs from what the old iterator did and cannot occur: blosc-LZ4 with device_blosc on a
    file marked foreign was queued by the iterator and then handed on at once; no reader marks a blosc file foreign, and the frames came
    out frame by frame either way ('P', what get_frames_triplets did)."""
    from pyrecode_amd import _lib
    from pyrecode_amd.reader_batched import _route
    family, level, mode, foreign = row[0].strip(), row[1], row[2], row[3]
    names = {'D': 'device', 'Z': 'device', 'H': 'host-decode', 'P': 'per-frame'}
    for cells, (blosc, zl) in zip(row[4:], ((False, False), (False, True), (True, False), (True, True))):
        for letter, scheme in zip(cells, (0, 1, 2, 4, 5, 8)):
            h = {'reduction_level': level, 'rc_operation_mode': mode, 'compression_scheme': scheme, 'target_bit_depth': 12}
            code = {'D': scheme, 'Z': _lib.RC_SCHEME_ZLIB_DEVICE}.get(letter)
            assert _route(h, foreign, blosc, zl, family) == (names[letter], code), (scheme, blosc, zl)
            if family == 'l2':
                for d, ok in ((7, False), (8, True), (16, True), (17, False)):
                    want = (names[letter], code) if ok else ('per-frame', None)
                    assert _route(dict(h, target_bit_depth=d), foreign, blosc, zl, family) == want, (scheme, d)


def test_pinned_buffer_growth_rule(monkeypatch):
    """reader_batched._pinned, the one place page-locked buffers are made: a quarter more than asked for and 1 MiB at least; a buffer that
    is large enough is reused; a smaller one is closed before its successor is made"""
    from pyrecode_amd import _lib
    from pyrecode_amd.reader_batched import _pinned, _BatchOut
    log = []

    class Stub:
        def __init__(self, nbytes):
            self.nbytes = nbytes
            self.array = np.zeros(nbytes, np.uint8)
            log.append(("new", nbytes))

        def close(self):
            log.append(("close", self.nbytes))
    monkeypatch.setattr(_lib, "PinnedBuffer", Stub)
    a = _pinned(None, 100)
    assert a.nbytes == 1 << 20 and log == [("new", 1 << 20)]
    assert _pinned(a, 1 << 20) is a and _pinned(a, 5) is a and len(log) == 1                    # large enough: reused
    b = _pinned(a, (1 << 20) + 1)
    assert b is not a and b.nbytes == int(((1 << 20) + 1) * 1.25) and log[1:] == [("close", 1 << 20), ("new", b.nbytes)]   # old one closed first
    c = _pinned(b, 4 << 20)
    assert c.nbytes == 5 << 20 and log[3:] == [("close", b.nbytes), ("new", 5 << 20)]
    # _BatchOut.room goes through it: element `at` of its holder
    holder = [None, c]
    out = _BatchOut(coo=True, holder=holder, at=1).room(1000)
    assert holder[1] is c and out.buf.size == 10000 and len(log) == 5
    out.room(1 << 20)
    assert holder[1] is not c and holder[1].nbytes == int(10 * (1 << 20) * 1.25) and log[5] == ("close", 5 << 20) and holder[0] is None
