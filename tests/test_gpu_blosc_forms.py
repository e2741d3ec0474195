"""The device blosc1 decoders on every form the chunk format admits, not only on what this library's encoder writes:
  the wave decoder  rc_blosc.hip::lz4_block_decode_wave + the 64 x 64 bit transpose of k_blosc_decode_blocks, behind rc_expand_frames,
                    _coo and _l2 with scheme 8 (host walk: rc_reader.hip::blosc_index_stream),
  seam 2            rc_codec_api.hip::blosc_decompress (k_lz4_decode + k_blosc_unshuffle) behind de_compress(8, ...).
The chunks come from tests/blosc_chunk_writer.py and hold the LZ4 blocks of tests/lz4_block_writer.py, stock liblz4's, or stored bytes
(judged by the oracle's from-spec decoder in tests/test_blosc_chunk_writer_cpu.py); expectations are the payloads the chunks were made from
and oracle.unpack_frame_sparse, never a device call.  Every comparison is exact."""
import struct

import numpy as np
import pytest

import blosc_chunk_writer as bw
import lz4_block_writer as lzw
from forms_gpu_helpers import check_expand, check_refused, decompress_raw, records

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


# ---- the wave decoder -----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def map_cases():
    return {c[0]: c for c in bw.map_chunk_cases()}


def _block_sources(blob, sizes, level):
    """where every LZ4 / stored block of every map chunk starts inside the blob (the address the decoding wave stages from)"""
    out, o = [], 0
    for cb, cp, _ in sizes:
        c = blob[o:o + int(cb)].tobytes()
        if not c[2] & 2:
            out += [o + s + 4 for s in bw.bstarts(c)]
        o += int(cb) + (int(cp) if level != 3 else 0)
    return out


@pytest.mark.parametrize("level", [1, 3])
@pytest.mark.parametrize("label", bw.MAP_CHUNK_LABELS)
def test_wave_decoder_decodes_the_catalogue_in_chunks(hip, orc, map_cases, label, level):
    """Binary maps as blosc1 chunks of typesize 8 and 512-byte blocks.  catalogue/*: the catalogue's blocks ARE the chunk's blocks - their
    decoded bytes are the bit-shuffled (or, flags 0x30, unshuffled) tile, the map is numpy's un-shuffle of them.  stock-motif/*: stock
    liblz4's blocks.  order: blocks laid out back to front and at random, found through bstarts alone.  gap: unused bytes between blocks,
    so that blocks start at every address modulo 4.  memcpyed: the map as a memcpyed chunk.  lastN/*: a last block of N bytes, alone
    (blocksize == N) and behind one whole tile - as a catalogue block, as stock liblz4's, stored, and as a literals-only block (csize > N)."""
    label, nx, ny, frames = map_cases[label]
    d = 12
    blob, sizes, want, prefix = records(orc, 8, level, d, nx, ny, frames, 17)
    if label == "gap":
        assert {s % 4 for s in _block_sources(blob, sizes, level)} == {0, 1, 2, 3}
    if label == "order":
        starts = [bw.bstarts(f[0]) for f in frames]
        assert starts[0] == sorted(starts[0], reverse=True) and all(s != sorted(s) and s != sorted(s, reverse=True) for s in starts[1:])
    if label.startswith("catalogue/"):
        csizes = [struct.unpack_from("<i", f[0], s)[0] for f in frames for s in bw.bstarts(f[0])]
        assert 515 in csizes and 512 not in csizes                                            # a block larger than its 512 bytes; none stored
    check_expand(hip, (nx, ny, d, level, 1, 8), blob, sizes, want, prefix, label)


def test_wave_decoder_level2_with_memcpyed_statistics(hip, orc, map_cases):
    """rc_expand_frames_l2 on catalogue chunks: rows and columns of the maps, and the statistics stream - a memcpyed chunk of 12-bit fields -
    unpacked to uint16"""
    L = hip.lib()
    nx, ny, d = 512, 64, 12
    frames = map_cases["catalogue/bitshuffle"][3]
    rng = np.random.default_rng(23)
    n = len(frames)
    parts, sizes, rows, cols, stats, prefix = [], np.zeros((n, 3), np.uint32), [], [], [], [0]
    for z, (c, data) in enumerate(frames):
        st = rng.integers(0, 1 << d, 2 * (37 + 100 * z)).astype(np.uint16)                      # (an even count: whole bytes)
        packed = orc.bit_pack(st, d).tobytes()
        pv = bw.chunk(packed, 8, 512, bw.BITSHUFFLE, False, memcpyed=True)
        parts += [c, pv]
        sizes[z] = (len(c), len(pv), len(packed))
        t = orc.unpack_frame_sparse(nx, ny, d, np.frombuffer(data, np.uint8), None, 3)
        rows.append(t[:, 0].astype(np.int32))
        cols.append(t[:, 1].astype(np.int32))
        stats.append(st)
        prefix.append(prefix[-1] + t.shape[0])
    blob = np.frombuffer(b"".join(parts), np.uint8).copy()
    rows, cols, stats, want_prefix = np.concatenate(rows), np.concatenate(cols), np.concatenate(stats), np.array(prefix, np.uint64)
    nnz, ns = int(want_prefix[n]), stats.size
    cap = nnz + 3
    rc = np.full(2 * cap + 4, -7, np.int32)
    st = np.full(ns + 4, 0xBEEF, np.uint16)
    got_prefix = np.zeros(n + 1, np.uint64)
    hip.check(L.rc_expand_frames_l2(nx, ny, d, 1, 8, hip.ptr(blob), hip.ptr(sizes), n, hip.ptr(got_prefix), hip.ptr(rc), cap, hip.ptr(st), ns))
    assert np.array_equal(got_prefix, want_prefix)
    assert np.array_equal(rc[:nnz], rows) and np.array_equal(rc[cap:cap + nnz], cols)
    assert (rc[nnz:cap] == -7).all() and (rc[cap + nnz:] == -7).all()
    assert np.array_equal(st[:ns], stats) and (st[ns:] == 0xBEEF).all()


def test_wave_decoder_refuses_malformed_blocks(hip, orc):
    """Each defect as block 3 of an 8-block chunk, bit-shuffled and not: RC_ERR_CORRUPT (rc_blosc.hip::lz4_block_decode_wave:
    `off == 0 || off > op || op + ml > cap`, `ip + lit > n`, `ip >= n` inside a length), no output entry written, a good batch right after."""
    nx, ny, d = 512, 64, 12
    geom = (nx, ny, d, 3, 1, 8)
    t512 = lzw.tiles(512)[:8]
    for shuffle in (bw.BITSHUFFLE, bw.NOSHUFFLE):
        good = records(orc, 8, 3, d, nx, ny, [bw.catalogue_chunk(t512, shuffle)], 5)
        payload = b"".join(bw.unshuffled(c.decoded, 8, shuffle) for c in t512)
        for name, blk in lzw.defects(512).items():
            bad = bw.chunk(payload, 8, 512, shuffle, False, lambda s, b, j: blk if b == 3 else t512[b].block)
            bad = np.frombuffer(bad, np.uint8).copy()
            check_refused(hip, geom, bad, np.array([[bad.size, 0, 0]], np.uint32), good, "shuffle %d/%s" % (shuffle, name))


# ---- seam 2 ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blocksize", bw.BLOCKSIZES)
@pytest.mark.parametrize("typesize", bw.TYPESIZES)
def test_seam_decodes_every_chunk_form(hip, typesize, blocksize):
    """de_compress(8): no shuffle, byte shuffle, bit shuffle; split (where c-blosc's rule allows it) and whole blocks; streams stored, stock
    liblz4's, or both; a leftover block of whole elements that are no multiple of 8, of a ragged length, and shorter than one element; a
    payload shorter than one element"""
    from pyrecode_amd import recode_compressors as rcmp
    count = 0
    for label, c, payload in bw.seam_chunks(typesize, blocksize):
        assert rcmp.de_compress(8, c, None) == payload, label
        count += 1
    assert count >= 27


def test_seam_decodes_the_map_chunks_too(hip, map_cases):
    """the wave decoder's chunks (permuted and gapped bstarts, csize > blocksize, memcpyed) through de_compress(8)"""
    from pyrecode_amd import recode_compressors as rcmp
    for label, nx, ny, frames in map_cases.values():
        for c, data in frames:
            assert rcmp.de_compress(8, c, None) == data, label


def test_seam_refuses_chunks_whose_blocks_leave_the_chunk(hip):
    """a bstart behind the chunk's end and a csize that runs past it (rc_codec_api.hip::blosc_decompress: `pos + 4 > n`, `pos + cs > n`):
    RC_ERR_CORRUPT on the host walk, nothing written"""
    payload = bw.seam_payload(8, 512, 1500)
    good = bw.chunk(payload, 8, 512, bw.SHUFFLE, False, bw.stock_lz4)
    for what in ("bstart", "csize"):
        c = bytearray(good)
        if what == "bstart":
            c[20:24] = struct.pack("<i", len(good) - 2)
        else:
            c[bw.bstarts(good)[2]:bw.bstarts(good)[2] + 4] = struct.pack("<i", 476 + 1 + 16)   # (the bound of a 476-byte block: only the chunk's end stops it)
        st, n, dst = decompress_raw(hip, 8, bytes(c), 4096)
        assert st == hip.RC_ERR_CORRUPT and (dst == 0xA5).all(), what
    st, n, dst = decompress_raw(hip, 8, good, 4096)
    hip.check(st)
    assert n == 1500 and dst[:n].tobytes() == payload and (dst[n:] == 0xA5).all()
