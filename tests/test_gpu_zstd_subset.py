"""-m gpu: the device zstd decoder (rc_zstd_dec.h walks, rc_zstd_dec.hip decodes one block per lane) on every frame form its subset
admits, written by the from-the-RFC writer of tests/zstd_frame_writer.py - not by this library's encoders, which take one fixed
choice at every point of the format.  The reference answer is the plaintext the writer was given (that the stock libzstd decodes
every one of these frames to it is established without a GPU in tests/test_zstd_frame_writer_cpu.py).  Every case is an ordinary
in-bounds decode; damaged streams are the business of the mutation tests in test_gpu_parity.py."""
import ctypes as C

import numpy as np
import pytest

import zstd_frame_writer as W
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


@pytest.fixture(scope="module")
def frames():
    return list(W.corpus())


def _decompress(hip, frame, cap, guard=64):
    src = np.frombuffer(frame, np.uint8)
    out = np.full(cap + guard, 0xA5, np.uint8)
    n = C.c_uint64(0)
    st = hip.lib().rc_decompress(1, hip.ptr(src), src.size, hip.ptr(out), cap, C.byref(n))
    assert (out[cap:] == 0xA5).all(), "bytes behind the capacity were written"
    return st, int(n.value), out[:cap]


def test_rc_decompress_gives_the_plaintext_for_every_in_subset_frame(hip, frames):
    """host memory in, host memory out, the destination exactly as long as the plaintext: RC_OK and the plaintext, for every frame of
    the corpus - none RC_ERR_UNSUPPORTED, none RC_ERR_CORRUPT"""
    wrong = []
    for name, data, frame, _ in frames:
        st, n, out = _decompress(hip, frame, len(data))
        if st != hip.RC_OK or n != len(data):
            wrong.append((name, st, n, len(data), hip.last_error()))
        elif out.tobytes() != data:
            got = np.frombuffer(data, np.uint8) != out
            wrong.append((name, "other bytes", int(got.sum()), int(np.flatnonzero(got)[0])))
    assert not wrong, (len(wrong), wrong[:8])


def test_rc_decompress_size_query_and_short_destination(hip, frames):
    """dst NULL with capacity 0 asks for the size: RC_ERR_OUT_TOO_SMALL and an upper bound of the decoded size (the frame is not decoded
    for it unless the bound is within 1024 bytes: only a last block with sequences may be counted with up to 511 bytes too many).  A
    destination one byte short is within those 1024 bytes, so the frame is decoded: refused with the EXACT size, nothing written behind it."""
    L = hip.lib()
    for name, data, frame, _ in frames[::3]:
        src = np.frombuffer(frame, np.uint8)
        n = C.c_uint64(0)
        st = L.rc_decompress(1, hip.ptr(src), src.size, None, 0, C.byref(n))
        assert st == hip.RC_ERR_OUT_TOO_SMALL and len(data) <= n.value < len(data) + W.TILE, (name, st, n.value, len(data))
        st, need, _ = _decompress(hip, frame, len(data) - 1)
        assert st == hip.RC_ERR_OUT_TOO_SMALL and need == len(data), (name, st, need, len(data))


def test_rc_decompress_with_both_buffers_in_device_memory(hip, frames):
    import torch
    L = hip.lib()
    for name, data, frame, _ in frames[1::5]:
        src = torch.zeros(len(frame) + 64, dtype=torch.uint8, device="cuda")
        src[:len(frame)].copy_(torch.from_numpy(np.frombuffer(frame, np.uint8).copy()))
        dst = torch.full((len(data) + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        n = C.c_uint64(0)
        st = L.rc_decompress(1, src.data_ptr(), len(frame), dst.data_ptr(), len(data), C.byref(n))
        assert st == hip.RC_OK and n.value == len(data), (name, st, hip.last_error())
        got = dst.cpu().numpy()
        assert got[:len(data)].tobytes() == data, name
        assert (got[len(data):] == 0xA5).all(), name


def _stored_batch(orc, ny, nx, d, n, seed, sparsity, bitmaps=None):
    """n stored frames whose two streams the WRITER compressed: the binary map in 512-byte blocks of any type (frame 1: blocks of any
    size, which takes the reader's full-entry lists instead of its compact ones), the value stream as Raw / RLE / literals-only
    Compressed blocks; other choices for every frame.  -> blob, sizes, the oracle's triplets, their prefix"""
    dark, frames = synth_frames(seed, n, ny, nx, sparsity, d)
    if n > 2:
        frames[2] = 0                                                     # an empty frame: no value stream bytes at all
    thr = orc.threshold(dark, 0)
    parts, sizes, want, prefix = [], np.zeros((n, 3), np.uint32), [], [0]
    for z in range(n):
        binary, pix = orc.binarize_l1(frames[z], thr)
        bitmap = orc.pack_binary_frame(binary).tobytes()
        packed = orc.bit_pack(pix, d).tobytes()
        bm, _ = W.write_frame(bitmap, {"seed": 100 * seed + z, "cut": "any" if z == 1 else "tiles"})
        if bitmaps is not None:
            bitmaps.append(bitmap)
        pv, _ = W.write_frame(packed, {"seed": 100 * seed + 50 + z, "cut": "literals_only"})
        parts += [bm, pv]
        sizes[z] = (len(bm), len(pv), len(packed))
        t = orc.unpack_frame_sparse(nx, ny, d, np.frombuffer(bitmap, np.uint8), np.frombuffer(packed, np.uint8), 1)
        want.append(t)
        prefix.append(prefix[-1] + t.shape[0])
    blob = np.frombuffer(b"".join(parts), np.uint8).copy()
    return blob, sizes, np.concatenate(want), prefix


GEOMETRIES = [(64, 512, 12, 0.03), (70, 300, 9, 0.04), (37, 53, 16, 0.10), (128, 512, 16, 0.30), (96, 341, 12, 0.005)]


@pytest.mark.parametrize("ny,nx,d,sparsity", GEOMETRIES)   # ny * nx / 8: 4096, 2625, 245.1, 8192, 4092 bytes
def test_expand_frames_on_streams_the_writer_compressed(hip, orc, ny, nx, d, sparsity):
    """rc_expand_frames / rc_expand_frames_coo (scheme 1) on stored frames built by hand from oracle data, against orc.unpack_frame_sparse"""
    n = 4
    L = hip.lib()
    blob, sizes, want, prefix = _stored_batch(orc, ny, nx, d, n, 31 + d + ny, sparsity)
    total = prefix[-1]
    got_prefix, got = np.zeros(n + 1, np.uint64), np.zeros((max(total, 1), 3), np.uint64)
    hip.check(L.rc_expand_frames(nx, ny, d, 1, 1, 1, hip.ptr(blob), hip.ptr(sizes), n, hip.ptr(got_prefix), hip.ptr(got), total))
    assert list(got_prefix) == prefix
    assert np.array_equal(got[:total], want)
    cap = total + 5
    coo = np.full(10 * cap + 16, 0xA5, np.uint8)
    got_prefix[:] = 0
    hip.check(L.rc_expand_frames_coo(nx, ny, d, 1, 1, 1, hip.ptr(blob), hip.ptr(sizes), n, hip.ptr(got_prefix), hip.ptr(coo), cap))
    assert list(got_prefix) == prefix
    rows, cols, vals = coo[:4 * cap].view(np.int32)[:total], coo[4 * cap:8 * cap].view(np.int32)[:total], coo[8 * cap:10 * cap].view(np.uint16)[:total]
    assert np.array_equal(rows, want[:, 0].astype(np.int32)) and np.array_equal(cols, want[:, 1].astype(np.int32))
    assert np.array_equal(vals, want[:, 2].astype(np.uint16))
    assert (coo[10 * cap:] == 0xA5).all()


# block types of the binary map's tiles, in turn, and the sequence-table modes of those with sequences: the first keeps to one set of
# tables (the reader's compact lists: k_bitmap_decode_c reads type and modes from the block itself), the second repeats the
# PREDEFINED tables (full block entries: k_block_decode and k_block_copy)
ROUTES = {"compact": ["predefined", "described", "repeat", "repeat"] + ["predefined"] * 8, "full_entries": ["predefined", "repeat"]}


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_expand_frames_takes_both_bitmap_routes_with_mixed_block_types(hip, orc, route):
    ny, nx, d, n = 96, 512, 12, 2                                        # 6144 bytes: twelve tiles per binary map
    L = hip.lib()
    dark, frames = synth_frames(91, n, ny, nx, 0.02, d)
    thr = orc.threshold(dark, 0)
    parts, sizes, want, prefix = [], np.zeros((n, 3), np.uint32), [], [0]
    for z in range(n):
        frames[z, 24:32] = frames[z, 72:80] = 0                           # tiles 3 and 9 all zero: RLE blocks
        binary, pix = orc.binarize_l1(frames[z], thr)
        bitmap = orc.pack_binary_frame(binary).tobytes()
        packed = orc.bit_pack(pix, d).tobytes()
        bm, census = W.write_frame(bitmap, {"seed": 7 + z, "cut": "tiles", "block": ["seq", "raw", "seq", "rle", "lits", "seq"],
                                            "seq_mode": ROUTES[route]})
        c = census["counts"]
        assert c["block:sequences"] >= 4 and c["block:raw"] >= 2 and c["block:rle"] >= 2 and c["block:literals_only"] >= 2, c
        assert ("repeat_of:predefined" in c) == (route == "full_entries") and (route == "full_entries" or c["repeat_of:described"] >= 2), c
        pv, _ = W.write_frame(packed, {"seed": 70 + z, "cut": "literals_only"})
        parts += [bm, pv]
        sizes[z] = (len(bm), len(pv), len(packed))
        t = orc.unpack_frame_sparse(nx, ny, d, np.frombuffer(bitmap, np.uint8), np.frombuffer(packed, np.uint8), 1)
        want.append(t)
        prefix.append(prefix[-1] + t.shape[0])
    blob = np.frombuffer(b"".join(parts), np.uint8).copy()
    total = prefix[-1]
    got_prefix, got = np.zeros(n + 1, np.uint64), np.zeros((total, 3), np.uint64)
    hip.check(L.rc_expand_frames(nx, ny, d, 1, 1, 1, hip.ptr(blob), hip.ptr(sizes), n, hip.ptr(got_prefix), hip.ptr(got), total))
    assert list(got_prefix) == prefix
    assert np.array_equal(got, np.concatenate(want))


def test_expand_frames_submit_wait_on_both_slots(hip, orc):
    import torch
    ny, nx, d, n = 70, 300, 12, 3
    L = hip.lib()
    batches = []
    for seed in (61, 62):
        blob, sizes, want, prefix = _stored_batch(orc, ny, nx, d, n, seed, 0.03)
        pin = hip.PinnedBuffer(blob.size)
        pin.array[:] = blob
        batches.append((pin, sizes, want, prefix, torch.zeros((prefix[-1], 3), dtype=torch.int64, device="cuda")))
    for slot, (pin, sizes, want, prefix, out) in enumerate(batches):
        hip.check(L.rc_expand_frames_submit(slot, nx, ny, d, 1, 1, 1, hip.ptr(pin.array), hip.ptr(sizes), n, out.data_ptr(), prefix[-1]))
    for slot, (pin, sizes, want, prefix, out) in enumerate(batches):
        got_prefix = np.zeros(n + 1, np.uint64)
        hip.check(L.rc_expand_frames_wait(slot, hip.ptr(got_prefix)))
        assert list(got_prefix) == prefix
        assert np.array_equal(out.cpu().numpy().view(np.uint64), want)
    for b in batches:
        b[0].close()


# what rc_decompress answers to a LEGAL frame one feature outside the subset (tests/test_zstd_frame_writer_cpu.py states the host walk's
# verdicts): UNSUPPORTED where the host sees the feature or the block is too long for the decoder's rows, CORRUPT where only the
# device's own checks stand in the way
def _near_miss_status(hip):
    U, X = hip.RC_ERR_UNSUPPORTED, hip.RC_ERR_CORRUPT
    return {"four_stream_literals": U, "real_offset": U, "literal_length_zero": X, "second_tree": U, "second_described_tables": U,
            "rle_length_modes": U, "length_modes_differ": U, "checksum": U, "midframe_short_sequence_block": X,
            "literals_block_above_1024": U, "two_frames": U}


def test_near_miss_frames_are_refused_and_decoded_by_the_fallback(hip):
    """Never RC_OK with other bytes.  literal_length_zero matters most: legal zstd in which "offset code 0" means the SECOND repeat offset
    - the plaintext differs from what "the byte in front" would give - and only the device's check of the literal length sees it."""
    from pyrecode_amd import recode_compressors as rcomp
    data = W.near_miss_plaintext()
    expect = _near_miss_status(hip)
    assert set(expect) == set(W.NEAR_MISS_FEATURES)
    for feature in W.NEAR_MISS_FEATURES:
        frame = W.write_near_miss(data, feature)
        st, n, out = _decompress(hip, frame, len(data) + W.TILE)
        assert st == expect[feature], (feature, st, hip.last_error())
        assert rcomp.de_compress(1, frame, None) == data, feature
    frame = W.write_repeat_offsets_without_table(data)                   # not legal zstd: refused here, and by the stock decoder behind it
    st, _, _ = _decompress(hip, frame, len(data) + W.TILE)
    assert st == hip.RC_ERR_CORRUPT
    with pytest.raises(ValueError):
        rcomp.de_compress(1, frame, None)
