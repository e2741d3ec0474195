"""What tests/test_gpu_lz4_forms.py and tests/test_gpu_blosc_forms.py share: a batch of stored frames built around given binary-map streams,
its expectation from the oracle, and the calls that compare the batched reader and rc_decompress with it.  No test lives here."""
import ctypes as C

import numpy as np

import blosc_chunk_writer as bw
import lz4_block_writer as lzw


def value_stream(scheme, packed):
    """the bytes of a frame's value stream the way the batched reader takes them: one stored block (scheme 2), a memcpyed chunk (scheme 8)"""
    if scheme == 2:
        return lzw.frame([("stored", packed)] if packed else [])
    return bw.chunk(packed, 8, 512, bw.BITSHUFFLE, False, memcpyed=True)


def records(orc, scheme, level, d, nx, ny, frames, seed):
    """frames: [(map stream, map bytes)] -> (blob, sizes, expected triplets uint64[nnz][3], expected prefix): every set pixel of a level-1
    frame gets a random d-bit value, the expectation is oracle.unpack_frame_sparse of the map's own bytes"""
    rng = np.random.default_rng(seed)
    n = len(frames)
    parts, sizes, want, prefix = [], np.zeros((n, 3), np.uint32), [], [0]
    for z, (stream, bitmap) in enumerate(frames):
        bm = np.frombuffer(bitmap, np.uint8)
        assert bm.size * 8 == nx * ny
        packed = None
        if level == 1:
            nnz = int(np.unpackbits(bm).sum())
            packed = orc.bit_pack(rng.integers(1, 1 << d, nnz).astype(np.uint16), d).tobytes()
            pv = value_stream(scheme, packed)
            parts += [stream, pv]
            sizes[z] = (len(stream), len(pv), len(packed))
        else:
            parts.append(stream)
            sizes[z, 0] = len(stream)
        t = orc.unpack_frame_sparse(nx, ny, d, bm, np.frombuffer(packed, np.uint8) if packed else None, level)
        want.append(t)
        prefix.append(prefix[-1] + t.shape[0])
    blob = np.frombuffer(b"".join(parts), np.uint8).copy()
    return blob, sizes, np.concatenate(want), np.array(prefix, np.uint64)


def check_expand(hip, geom, blob, sizes, want, want_prefix, label):
    """rc_expand_frames (counting call, then triplets) and rc_expand_frames_coo against the expectation; nothing behind the last entry is touched"""
    L = hip.lib()
    n = len(want_prefix) - 1
    nnz = int(want_prefix[n])
    src = (hip.ptr(blob), hip.ptr(sizes), n)
    prefix = np.zeros(n + 1, np.uint64)
    hip.check(L.rc_expand_frames(*geom, *src, hip.ptr(prefix), None, 0), label)
    assert np.array_equal(prefix, want_prefix), label
    cap = nnz + 5
    trip = np.full((cap, 3), 0xA5A5, np.uint64)
    prefix[:] = 0
    hip.check(L.rc_expand_frames(*geom, *src, hip.ptr(prefix), hip.ptr(trip), cap), label)
    assert np.array_equal(prefix, want_prefix), label
    assert np.array_equal(trip[:nnz], want), label
    assert (trip[nnz:] == 0xA5A5).all(), label
    coo = np.full(10 * cap + 16, 0xA5, np.uint8)
    prefix[:] = 0
    hip.check(L.rc_expand_frames_coo(*geom, *src, hip.ptr(prefix), hip.ptr(coo), cap), label)
    assert np.array_equal(prefix, want_prefix), label
    assert np.array_equal(coo[:4 * cap].view(np.int32)[:nnz], want[:, 0].astype(np.int32)), label
    assert np.array_equal(coo[4 * cap:8 * cap].view(np.int32)[:nnz], want[:, 1].astype(np.int32)), label
    assert np.array_equal(coo[8 * cap:10 * cap].view(np.uint16)[:nnz], want[:, 2].astype(np.uint16)), label
    assert (coo[10 * cap:] == 0xA5).all(), label


def check_refused(hip, geom, bad_blob, bad_sizes, good, label):
    """a one-frame level-3 batch the device must refuse as corrupt: nothing is written, and a good batch goes through afterwards"""
    L = hip.lib()
    cap = geom[0] * geom[1]                                 # (room for every pixel: too little room is not what is refused here)
    out = np.full(10 * cap + 16, 0xA5, np.uint8)
    prefix = np.zeros(2, np.uint64)
    assert L.rc_expand_frames_coo(*geom, hip.ptr(bad_blob), hip.ptr(bad_sizes), 1, hip.ptr(prefix), hip.ptr(out), cap) == hip.RC_ERR_CORRUPT, label
    assert (out == 0xA5).all(), label
    check_expand(hip, geom, *good, label + ": the good batch afterwards")


def decompress_raw(hip, scheme, stream, cap):
    """rc_decompress into a buffer of sentinels -> (status, bytes reported, the buffer)"""
    src = np.frombuffer(bytes(stream), np.uint8).copy()
    dst = np.full(cap, 0xA5, np.uint8)
    n = C.c_uint64(0)
    st = hip.lib().rc_decompress(scheme, hip.ptr(src), src.size, hip.ptr(dst), cap, C.byref(n))
    return st, n.value, dst
