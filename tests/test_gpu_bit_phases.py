"""-m gpu: residuals that use every bit of d, and tile chains that complete a shared stream byte in every way k_gather can
(tests/bitphase_cases.py), against the oracle - every level-1 emit, the batched reader, level 2 and two full-size configurations.
The streams are judged like in tests/test_gpu_parity.py / tests/test_gpu_deflate.py: stock liblz4, stock libzstd, stdlib zlib plus the
serial DEFLATE model, the blosc1 decoder from the spec."""
import struct
import zlib

import numpy as np
import pytest

import bitphase_cases as bc
import deflate_block_model as model
from test_gpu_parity import SHAPES, _check_lz4, _l2_expected, _zstd_system_decode

pytestmark = pytest.mark.gpu

DT = {"uint8": np.uint8, "uint16": np.uint16, "uint32": np.uint32}
# (op_mode, scheme, clevel, device zlib)
EMITS = {"raw": (0, 0, 1, False), "lz4c0": (1, 2, 0, False), "lz4c1": (1, 2, 1, False), "zstdc0": (1, 1, 0, False),
         "zstdc1": (1, 1, 1, False), "blosc": (1, 8, 1, False), "zlib": (1, 0, 1, True)}


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


def _torch_dtype(torch, dtype):
    return {1: torch.uint8, 2: torch.int16, 4: torch.int32}[np.dtype(dtype).itemsize]


def _signed(a):
    a = np.ascontiguousarray(a)
    return a if a.dtype == np.uint8 else a.view({2: np.int16, 4: np.int32}[a.dtype.itemsize])


def _pack(orc, vals, d, dtype):
    if np.dtype(dtype) == np.uint32:
        return orc.bit_pack32(np.asarray(vals, np.uint32), d).tobytes()
    return orc.bit_pack(np.asarray(vals, np.uint16), d).tobytes()


def _run(hip, torch, frames_d, B, nx, ny, d, dtype, emit, dark=None, thr=None, eps=0, level=1, stat=None, pipelined=False):
    """One batch through the device-resident path; returns (records bytes, rec offsets, md)."""
    op_mode, scheme, clevel, dz = EMITS[emit]
    ctx = hip.ReduceContext(nx, ny, d, level, op_mode, scheme, clevel, 0, max_batch=B, src_dtype=dtype, device_zlib=dz)
    try:
        if dark is not None:
            ctx.set_dark(dark, eps)
        else:
            ctx.set_threshold(thr)
        if stat is not None:
            ctx.set_l2_statistics(stat)
        if pipelined:
            ctx.set_pipelined(True)
        cap = int(ctx.out_capacity(B))
        out = torch.empty(cap, dtype=torch.uint8, device="cuda")
        rec = torch.zeros(B + 1, dtype=torch.int64, device="cuda")
        md = torch.zeros((B, 3), dtype=torch.int32, device="cuda")
        ctx.enqueue(frames_d.data_ptr(), B, 0, out.data_ptr(), cap, rec.data_ptr(), md.data_ptr())
        ctx.sync()
        rec_h, md_h = rec.cpu().numpy(), md.cpu().numpy().view(np.uint32)
        return out[:int(rec_h[-1])].cpu().numpy().tobytes(), rec_h, md_h
    finally:
        ctx.close()


def _judge(orc, emit, r, fid, bitmap, packed, md_row, tag, model_bitmap=True):
    """One level-1 record against the oracle's bitmap and packed stream."""
    if emit == "raw":
        assert r == struct.pack("<II", fid, len(packed)) + bitmap + packed, tag
        assert int(md_row[0]) == len(packed), tag
        return
    got_fid, cb, cp, npk = struct.unpack_from("<IIII", r, 0)
    assert (got_fid, npk) == (fid, len(packed)) and (cb, cp, npk) == tuple(int(v) for v in md_row) and len(r) == 16 + cb + cp, tag
    sb, sp = r[16:16 + cb], r[16 + cb:]
    if emit.startswith("lz4"):
        _check_lz4(orc, sb, bitmap)
        _check_lz4(orc, sp, packed)
    elif emit.startswith("zstd"):
        assert _zstd_system_decode(sb) == bitmap, tag + ": binary map"
        assert _zstd_system_decode(sp) == packed, tag + ": values"
    elif emit == "blosc":
        assert orc.blosc1_decode(sb) == bitmap, tag + ": binary map"
        assert orc.blosc1_decode(sp) == packed, tag + ": values"
    else:
        assert zlib.decompress(sb) == bitmap, tag + ": binary map"
        assert zlib.decompress(sp) == packed, tag + ": values"
        assert sp == model.stored_stream(packed), tag + ": value stream differs from the serial model"
        if model_bitmap:
            assert sb == model.bitmap_stream(bitmap), tag + ": binary-map stream differs from the serial model"


def _split_for_reader(out, rec, md, emit, n, nb):
    sizes = np.zeros((n, 3), np.uint32)
    parts = []
    for z in range(n):
        r = np.frombuffer(out, np.uint8)[int(rec[z]):int(rec[z + 1])]
        if emit == "raw":
            sizes[z] = (nb, md[z, 0], md[z, 0])
            parts.append(r[8:])
        else:
            sizes[z] = md[z, :3]
            parts.append(r[16:])
    return np.ascontiguousarray(np.concatenate(parts)), sizes


# ---- the tile-chain matrix ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,d,tpi", bc.chain_matrix(), ids=lambda v: str(v))
def test_tile_chains_every_emit(hip, orc, dt, d, tpi):
    import torch
    dtype = DT[dt]
    B, nt = bc.TPI_GEOMETRY[tpi]
    assert bc.gather_tpi(B, nt) == tpi
    cs = bc.tile_chain_frames(d, nt, dtype, B=B, tpi=tpi, seed=tpi)
    N, nx, ny, nb = cs["N"], cs["nx"], cs["ny"], (cs["N"] + 7) // 8
    dark = cs["dark"]
    # the frames on the device: the threshold everywhere (not set), dark + value at the events
    frames_d = torch.from_numpy(_signed(dark)).cuda().repeat(B, 1)
    gidx = np.concatenate([z * N + p for z, p in enumerate(cs["idx"])])
    gval = np.concatenate([(dark[p].astype(np.uint64) + v).astype(dtype) for p, v in zip(cs["idx"], cs["vals"])])
    frames_d.view(-1)[torch.from_numpy(gidx).cuda()] = torch.from_numpy(_signed(gval)).cuda()
    # the oracle's streams, once per frame set
    want = []
    for z in range(B):
        bm = np.zeros(N, bool)
        bm[cs["idx"][z]] = True
        want.append((np.packbits(bm, bitorder="little").tobytes(), _pack(orc, cs["vals"][z], d, dtype)))
    if tpi == 8:   # small sets: the records the oracle makes of the frames themselves
        host = bc.chain_host_frames(cs)
        thr = dark.reshape(ny, nx)
        for z in range(B):
            l1 = orc.l1_record32 if dtype == np.uint32 else orc.l1_record
            assert l1(host[z], thr, d, z, mode=0)[0] == struct.pack("<II", z, len(want[z][1])) + want[z][0] + want[z][1]
    emits = [e for e in EMITS if not (e == "zlib" and dtype == np.uint32)]   # (device zlib refuses uint32 sources: tested elsewhere)
    if tpi == 64:
        emits = ["raw", "lz4c1", "zstdc1"] + (["zlib"] if dtype != np.uint32 else [])
    for emit in emits:
        out, rec, md = _run(hip, torch, frames_d, B, nx, ny, d, dtype, emit, dark=dark)
        for z in range(B):
            _judge(orc, emit, out[int(rec[z]):int(rec[z + 1])], z, want[z][0], want[z][1], md[z], "%s d %d tpi %d %s frame %d" % (dt, d, tpi, emit, z),
                   model_bitmap=tpi == 8)
        if tpi != 8 or emit not in ("raw", "zstdc1", "lz4c1"):
            continue
        # ... and back through the batched reader: triplets (every dtype), COO (d <= 16)
        blob, sizes = _split_for_reader(out, rec, md, emit, B, nb)
        scheme = EMITS[emit][1]
        mode = EMITS[emit][0]
        trip_want = np.concatenate([orc.unpack_frame_sparse(nx, ny, d, np.frombuffer(w[0], np.uint8), np.frombuffer(w[1], np.uint8))
                                    for w in want])
        nnz = trip_want.shape[0]
        prefix = np.zeros(B + 1, np.uint64)
        got = np.zeros((nnz, 3), np.uint64)
        L = hip.lib()
        hip.check(L.rc_expand_frames(nx, ny, d, 1, mode, scheme, hip.ptr(blob), hip.ptr(sizes), B, hip.ptr(prefix), hip.ptr(got), nnz),
                  "rc_expand_frames %s d %d %s" % (dt, d, emit))
        assert int(prefix[B]) == nnz
        assert np.array_equal(got, trip_want), "reader: %s d %d %s" % (dt, d, emit)
        if d <= 16:
            coo = np.zeros(10 * nnz + 16, np.uint8)
            prefix[:] = 0
            hip.check(L.rc_expand_frames_coo(nx, ny, d, 1, mode, scheme, hip.ptr(blob), hip.ptr(sizes), B, hip.ptr(prefix), hip.ptr(coo), nnz))
            assert np.array_equal(coo[:4 * nnz].view(np.int32), trip_want[:, 0].astype(np.int32))
            assert np.array_equal(coo[4 * nnz:8 * nnz].view(np.int32), trip_want[:, 1].astype(np.int32))
            assert np.array_equal(coo[8 * nnz:10 * nnz].view(np.uint16), trip_want[:, 2].astype(np.uint16)), "COO: %s d %d %s" % (dt, d, emit)


@pytest.mark.parametrize("emit", ["lz4c1", "zlib"])
def test_tile_chains_through_the_pipelined_enqueue_path(hip, orc, emit):
    """One depth through the pipelined form (two scratch sets, the next batch's reduce kernel next to this batch's assembly)."""
    import torch
    d, tpi = 5, 16
    B, nt = bc.TPI_GEOMETRY[tpi]
    cs = bc.tile_chain_frames(d, nt, np.uint16, B=B, tpi=tpi, seed=99)
    N, nx, ny = cs["N"], cs["nx"], cs["ny"]
    frames_d = torch.from_numpy(_signed(cs["dark"])).cuda().repeat(B, 1)
    gidx = np.concatenate([z * N + p for z, p in enumerate(cs["idx"])])
    gval = np.concatenate([(cs["dark"][p].astype(np.uint64) + v).astype(np.uint16) for p, v in zip(cs["idx"], cs["vals"])])
    frames_d.view(-1)[torch.from_numpy(gidx).cuda()] = torch.from_numpy(_signed(gval)).cuda()
    out, rec, md = _run(hip, torch, frames_d, B, nx, ny, d, np.uint16, emit, dark=cs["dark"], pipelined=True)
    for z in range(B):
        bm = np.zeros(N, bool)
        bm[cs["idx"][z]] = True
        _judge(orc, emit, out[int(rec[z]):int(rec[z + 1])], z, np.packbits(bm, bitorder="little").tobytes(), _pack(orc, cs["vals"][z], d, np.uint16),
               md[z], "pipelined %s frame %d" % (emit, z), model_bitmap=False)


# ---- full-range residuals on the SHAPES list ------------------------------------------------------------------------------------------
FULL_SHAPES = [(ny, nx, s, 9 + i % 8, 1 + i % 6, i % 3 == 2) for i, (ny, nx, s, _, _) in enumerate(SHAPES)]   # ny, nx, s, d, eps, overflow


@pytest.mark.parametrize("emit", list(EMITS))
@pytest.mark.parametrize("ny,nx,s,d,eps,overflow", FULL_SHAPES)
def test_full_range_residuals_every_emit(hip, orc, ny, nx, s, d, eps, overflow, emit):
    import torch
    dark, frames = bc.full_range_frames(300 + ny + d, 3, ny, nx, s, d, np.uint16, eps, overflow)
    thr = orc.threshold(dark, eps)
    assert (dark.astype(np.int64) + eps > 65535).any()   # wrapped thresholds are part of the data
    frames_d = torch.from_numpy(_signed(frames.reshape(3, -1))).cuda()
    out, rec, md = _run(hip, torch, frames_d, 3, nx, ny, d, np.uint16, emit, dark=dark, eps=eps)
    for z in range(3):
        binary, pix = orc.binarize_l1(frames[z], thr)
        bitmap, packed = orc.pack_binary_frame(binary).tobytes(), orc.bit_pack(pix, d).tobytes()
        _judge(orc, emit, out[int(rec[z]):int(rec[z + 1])], z, bitmap, packed, md[z], "%dx%d d %d %s frame %d" % (ny, nx, d, emit, z))


@pytest.mark.parametrize("stat", [0, 1, 2])
@pytest.mark.parametrize("d", [9, 13, 15, 16])
def test_l2_full_range_values_wrap_mod_2_to_the_d(hip, orc, d, stat):
    """Level 2 on large components of full-range values: maxima above 2^d - 1 and sums far beyond it, stored modulo 2^d."""
    import torch
    ny, nx = 150, 260
    dark, frames = bc.full_range_frames(700 + d + stat, 3, ny, nx, 0.5, d, np.uint16, 2, overflow=True)
    frames[1, :, ::3] = np.maximum(frames[1, :, ::3], (dark[:, ::3].astype(np.int64) + 3).clip(0, 65535).astype(np.uint16))   # long snakes
    thr = orc.threshold(dark, 2)
    frames_d = torch.from_numpy(_signed(frames.reshape(3, -1))).cuda()
    for emit in ("raw", "lz4c1"):
        out, rec, md = _run(hip, torch, frames_d, 3, nx, ny, d, np.uint16, emit, dark=dark, eps=2, level=2, stat=stat)
        for z in range(3):
            binary, vals = _l2_expected(frames[z], thr, stat, d)
            if stat == 2:
                assert z > 0 or (vals.size and int(np.asarray(frames[z][binary], np.int64).sum()) >= 1 << d)
            bitmap, packed = orc.pack_binary_frame(binary).tobytes(), orc.bit_pack(vals, d).tobytes()
            _judge(orc, emit, out[int(rec[z]):int(rec[z + 1])], z, bitmap, packed, md[z], "L2 d %d stat %d %s frame %d" % (d, stat, emit, z))
