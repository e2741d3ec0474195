"""The device LZ4 decoders on every form the block format admits, not only on what this library's encoders write:
  the thread decoder  rc_lz4.hip::lz4_block_walk        behind de_compress(2, ...),
  the lane decoder    rc_zstd_dec.hip::lz4_block_decode behind rc_expand_frames / _coo with scheme 2 - its compact-list kernel
                      (k_bitmap_decode_c: one block per 512-byte tile) and its full-entry kernel (k_block_decode: any other layout), each from
                      LDS and from global memory.
The blocks come from tests/lz4_block_writer.py (judged by stock liblz4 in tests/test_lz4_block_writer_cpu.py); expectations are the writer's
serial replay and oracle.unpack_frame_sparse, never a device call.  Every comparison is exact.  (The wave decoder of rc_blosc.hip gets the
same catalogue in tests/test_gpu_blosc_forms.py.)"""
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


# ---- the thread decoder ---------------------------------------------------------------------------------------------------------------------------
def test_thread_decoder_decodes_every_catalogue_block(hip):
    """de_compress(2): every catalogue block as a frame of its own, then all of them in one frame of independent blocks with stored blocks
    (17, 512, 1 and 700 bytes) in between"""
    from pyrecode_amd import recode_compressors as rcmp
    for c in lzw.CASES:
        assert rcmp.de_compress(2, lzw.frame([c.block]), None) == c.decoded, c.name
    f, want = lzw.mixed_frame()
    assert f.count(struct.pack("<I", 700 | 0x80000000)) >= 1 and rcmp.de_compress(2, f, None) == want


def test_thread_decoder_follows_linked_blocks_into_the_block_before(hip):
    """two linked 64 KiB blocks: the second opens with a match at offset 65535 (and, in the other frame, at offsets 1, 7, 65) into the
    first, which is an LZ4 block in one frame and a stored block in the other"""
    from pyrecode_amd import recode_compressors as rcmp
    for name, f, want in lzw.linked_frames():
        assert len(want) == 128 * 1024
        assert rcmp.de_compress(2, f, None) == want, name


def test_thread_decoder_refuses_malformed_blocks(hip):
    """Each defect of lz4_block_writer.defects(), as the middle block of an LZ4 frame and as a block of a blosc1 chunk: RC_ERR_CORRUPT from
    the sizing pass (rc_lz4.hip::lz4_block_walk: `off == 0 || off > op`, `ip + lit > n`, `ip >= n` inside a length; rc_codec_api.hip: a
    blosc block that does not decode to its size, an LZ4 block that decodes beyond the frame's block maximum), so not one output byte is
    written; the good stream decodes right after.  A block that merely decodes to 513 bytes is no error inside an LZ4 frame - a frame does
    not announce its blocks' sizes - and must decode."""
    good = lzw.tiles(512)[0]
    d512 = lzw.defects(512)
    for name, blk in d512.items():
        f = lzw.frame([good.block, blk, good.block])
        st, n, dst = decompress_raw(hip, 2, f, 4096)
        if name == "match_past_end":
            hip.check(st)
            seqs, tail = lzw.parse(blk)
            assert n == 1024 + 513 and dst[:n].tobytes() == good.decoded + lzw.replay(seqs, tail) + good.decoded
            assert (dst[n:] == 0xA5).all()
        else:
            assert st == hip.RC_ERR_CORRUPT, name
            assert (dst == 0xA5).all(), name
        payload = good.decoded + bytes(512) + good.decoded
        c = bw.chunk(payload, 8, 512, bw.NOSHUFFLE, False, lambda s, b, j: blk if b == 1 else good.block)
        st, n, dst = decompress_raw(hip, 8, c, 4096)
        assert st == hip.RC_ERR_CORRUPT, name
        assert (dst == 0xA5).all(), name
        st, n, dst = decompress_raw(hip, 2, lzw.frame([good.block] * 3), 4096)
        hip.check(st)
        assert n == 1536 and dst[:n].tobytes() == good.decoded * 3 and (dst[n:] == 0xA5).all()
    # a match that runs past the largest block the frame's descriptor allows (BD 0x40: 64 KiB)
    lit = good.decoded[:20]
    over = lzw.encode([(lit, 7, 65536 - 20 + 1)], b"")
    st, n, dst = decompress_raw(hip, 2, lzw.frame([over]), 70000)
    assert st == hip.RC_ERR_CORRUPT and (dst == 0xA5).all()
    fits, want = lzw.block([(lit, 7, 65536 - 20 - 12)], good.decoded[:12])
    st, n, dst = decompress_raw(hip, 2, lzw.frame([fits]), 70000)
    hip.check(st)
    assert n == 65536 and dst[:n].tobytes() == want and (dst[n:] == 0xA5).all()


# ---- the lane decoder -----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def map_cases():
    return {c[0]: c for c in lzw.map_frame_cases()}


@pytest.mark.parametrize("level", [1, 3])
@pytest.mark.parametrize("label", lzw.MAP_FRAME_LABELS)
def test_lane_decoder_decodes_the_catalogue_as_binary_maps(hip, orc, map_cases, label, level):
    """Binary maps whose 512-byte tiles are the catalogue's decoded blocks (8 tiles to a 64 x 512 frame; a shorter last block behind two
    tiles), one LZ4 block per tile: `uniform` streams go through the compact-list kernel, `split-first` ones - the first tile stored in two
    halves - through the full-entry kernel.  The value stream of a level-1 frame is one stored block."""
    label, nx, ny, frames = map_cases[label]
    d = 12
    blob, sizes, want, prefix = records(orc, 2, level, d, nx, ny, frames, 7)
    assert int(prefix[-1]) > 0
    check_expand(hip, (nx, ny, d, level, 1, 2), blob, sizes, want, prefix, label)


@pytest.mark.parametrize("layout", ["uniform", "split-first"])
def test_lane_decoder_reads_blocks_behind_the_staged_span_from_global_memory(hip, orc, layout):
    """512 x 1024 pixels: 128 tiles, one workgroup.  The first 70 are literals-only blocks of 515 bytes, so the size word of every later block
    lies more than SPAN bytes behind the first one's: the whole catalogue and 40 stock-liblz4 blocks are decoded by the global-memory copy of
    the decoder."""
    f, data, offs = lzw.big_map_frame(layout)
    extra = layout != "uniform"
    assert len(offs) == 128 + extra
    word = {q: struct.unpack_from("<I", f, q)[0] for q in offs}
    # Which lanes read global memory, restated from each kernel's own `in_lds` test (the map stream is the first thing in the blob, so an
    # offset in the frame is an address in `data`; the test cannot see which instantiation ran, it makes sure by construction):
    if layout == "uniform":
        # k_bitmap_decode_c: one workgroup = the 128 blocks, header to next header; span0 = first header & ~15;
        # in_lds = next header - span0 <= min(span rounded up to 16, SPAN)
        span0, end = offs[0] & ~15, len(f) - 4
        staged = min((end - span0 + 15) & ~15, lzw.SPAN)
        behind = [q for q, nxt in zip(offs, offs[1:] + [end]) if nxt - span0 > staged]
    else:
        # k_block_decode: the two stored halves go to the copy list, one workgroup = the 127 LZ4 blocks, src = the bytes behind the size
        # word; span0 = first src & ~15; in_lds = src - span0 + csize <= min(span rounded up to 16, SPAN)
        comp = [q for q in offs if not word[q] >> 31]
        assert len(comp) == 127
        span0, end = (comp[0] + 4) & ~15, comp[-1] + 4 + word[comp[-1]]
        staged = min((end - span0 + 15) & ~15, lzw.SPAN)
        behind = [q for q in comp if q + 4 - span0 + word[q] > staged]
    assert end - span0 > lzw.SPAN                                                             # the workgroup's span exceeds what it stages
    assert behind == offs[-len(behind):] and offs[70 + extra] in behind                       # every block behind the 70 literal ones:
    assert len(behind) >= 58 and not any(word[q] >> 31 for q in behind)                       # the catalogue and stock blocks, none stored
    nx, ny, d = 1024, 512, 12
    for level in (1, 3):
        blob, sizes, want, prefix = records(orc, 2, level, d, nx, ny, [(f, data)], 11)
        check_expand(hip, (nx, ny, d, level, 1, 2), blob, sizes, want, prefix, layout)


@pytest.mark.parametrize("layout", ["uniform", "split-first"])
def test_lane_decoder_refuses_malformed_blocks(hip, orc, layout):
    """Each defect as tile 3 of an 8-tile map, in both kernels: RC_ERR_CORRUPT (rc_zstd_dec.hip::lz4_block_decode: `off == 0 || off > o.op`,
    `o.op + ml > cap`, `ip + lit > n`, `ip >= n` inside a length), no output entry written, a good batch right after."""
    nx, ny, d = 512, 64, 12
    geom = (nx, ny, d, 3, 1, 2)
    t512 = lzw.tiles(512)[:8]
    good = records(orc, 2, 3, d, nx, ny, [lzw.map_frame(t512, layout)], 5)
    for name, blk in lzw.defects(512).items():
        blocks = [c.block for c in t512]
        blocks[3] = blk
        if layout == "split-first":
            blocks[0:1] = [("stored", t512[0].decoded[:256]), ("stored", t512[0].decoded[256:])]
        bad = np.frombuffer(lzw.frame(blocks), np.uint8).copy()
        check_refused(hip, geom, bad, np.array([[bad.size, 0, 0]], np.uint32), good, "%s/%s" % (layout, name))
