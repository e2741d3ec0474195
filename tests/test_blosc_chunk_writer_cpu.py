"""tests/blosc_chunk_writer.py judged before any device code sees its chunks: the oracle's from-spec decoder (oracle.blosc1_decode, LZ4 blocks
through its C decoder) must expand every chunk of both catalogues to the payload it was made from, and the numpy shuffles must be the
transforms the format documents describe.  c-blosc itself has NEVER judged these chunks: python-blosc is not installed where this suite is
developed, so the variants that call blosc.decompress skip there and run wherever it is present."""
import struct

import numpy as np
import pytest

import blosc_chunk_writer as bw
import lz4_block_writer as lzw


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    oracle.lib()
    return oracle


def test_shuffles_are_the_documented_transforms():
    """bit shuffle, element by element and bit by bit, straight from its definition (row 8 * k + b = bit b of byte k of every element; S
    rounded DOWN to a multiple of 8, the rest copied); byte shuffle likewise; both undone by their inverses; a clear flag shuffles nothing"""
    rng = np.random.default_rng(3)
    for typesize in (1, 2, 3, 4, 8, 16):
        for n in (0, 1, typesize - 1, typesize, 7 * typesize, 8 * typesize, 8 * typesize + 1, 9 * typesize, 15 * typesize + 3, 16 * typesize, 512, 438):
            blk = rng.integers(0, 256, n).astype(np.uint8).tobytes()
            S = (n // typesize) // 8 * 8
            want = bytearray(blk)
            for i in range(S):
                for k in range(typesize):
                    for b in range(8):
                        bit = (blk[i * typesize + k] >> b) & 1
                        at = (8 * k + b) * (S // 8) + i // 8
                        want[at] = (want[at] & ~(1 << (i % 8))) | (bit << (i % 8))
            assert bw.bit_shuffle(blk, typesize) == bytes(want), (typesize, n)
            assert bw.bit_unshuffle(bytes(want), typesize) == blk
            ne = n // typesize
            wb = bytearray(blk)
            for i in range(ne):
                for k in range(typesize):
                    wb[k * ne + i] = blk[i * typesize + k]
            assert bw.byte_shuffle(blk, typesize) == bytes(wb), (typesize, n)
            assert bw.byte_unshuffle(bytes(wb), typesize) == blk
            assert bw.shuffled(blk, typesize, bw.NOSHUFFLE) == blk == bw.unshuffled(blk, typesize, bw.NOSHUFFLE)
    assert bw.bit_shuffle(bytes(range(15 * 8)), 8)[64:] == bytes(range(64, 120))          # 15 elements: 8 shuffled, 7 copied


def test_chunk_layout():
    """header, flags, bstarts under `order` and `gap`, the split rule, stored streams"""
    payload = bytes(range(256)) * 5
    c = bw.chunk(payload, 8, 512, bw.BITSHUFFLE, False, bw.stored)
    assert c[:4] == bytes([2, 1, 0x34, 8]) and struct.unpack_from("<iii", c, 4) == (1280, 512, len(c))
    assert bw.bstarts(c) == [28, 28 + 516, 28 + 2 * 516]
    c = bw.chunk(payload, 8, 512, bw.NOSHUFFLE, False, bw.stored, order=[2, 0, 1], gap=lambda b: b + 1)
    assert c[2] == 0x30 and bw.bstarts(c) == [28 + 3 + 260 + 1, 28 + 3 + 260 + 1 + 516 + 2, 28 + 3]
    assert struct.unpack_from("<i", c, 28 + 3)[0] == 256 and c[28 + 3 + 4:28 + 3 + 260] == payload[1024:]
    c = bw.chunk(payload, 2, 512, bw.SHUFFLE, True, bw.stored)
    assert c[2] == 0x21 and struct.unpack_from("<i", c, bw.bstarts(c)[0])[0] == 256 and struct.unpack_from("<i", c, bw.bstarts(c)[2])[0] == 256
    assert len(c) == 16 + 12 + 2 * (2 * 260) + 260                                           # two split blocks, the leftover one whole
    with pytest.raises(ValueError):
        bw.chunk(payload, 8, 512, bw.SHUFFLE, True, bw.stored)                               # 64 elements a block: c-blosc never splits that
    c = bw.chunk(payload, 8, 512, bw.BITSHUFFLE, False, memcpyed=True)
    assert c[2] & 2 and c[16:] == payload and len(c) == 16 + len(payload)


@pytest.mark.parametrize("blocksize", bw.BLOCKSIZES)
@pytest.mark.parametrize("typesize", bw.TYPESIZES)
def test_the_oracle_decodes_every_seam_chunk(orc, typesize, blocksize):
    labels, lz4_streams, stored_streams = [], 0, 0
    for label, c, payload in bw.seam_chunks(typesize, blocksize):
        assert len(payload) <= 100000
        assert orc.blosc1_decode(c) == payload, label
        labels.append(label)
        lz4_streams += sum(1 for cs, n in bw.streams(c) if cs != n)
        stored_streams += sum(1 for cs, n in bw.streams(c) if cs == n)
    for word in ("shuffle0", "shuffle1", "shuffle4", "split0", " stored ", " stock_lz4 ", " mixed ", "whole-elements", "ragged", "short"):
        assert any(word in x for x in labels), word
    assert any("split1" in x for x in labels) == bw.may_split(typesize, blocksize)
    assert lz4_streams >= 40 and stored_streams >= 40


def test_the_oracle_decodes_every_map_chunk(orc):
    cases = bw.map_chunk_cases()
    labels = [c[0] for c in cases]
    assert labels == list(bw.MAP_CHUNK_LABELS)
    for n in bw.LAST_BLOCKS:
        assert "last%d/single" % n in labels and "last%d/behind-a-tile" % n in labels
    assert set((1, 7, 8, 13, 56, 63, 64, 71, 72, 127, 438)) <= set(bw.LAST_BLOCKS)
    for label, nx, ny, frames in cases:
        for c, data in frames:
            assert len(data) * 8 == nx * ny, label
            assert orc.blosc1_decode(c) == data, label
            assert c[3] == 8 and struct.unpack_from("<i", c, 8)[0] == min(512, len(data)), label
    # the catalogue's blocks really are the chunks' blocks: csize 515 (a block larger than its 512 bytes) is among them
    c, _ = bw.catalogue_chunk(lzw.tiles(512)[8:16], bw.BITSHUFFLE)
    assert 515 in [struct.unpack_from("<i", c, s)[0] for s in bw.bstarts(c)]


def _blosc_or_skip():
    return pytest.importorskip("blosc")


def test_stock_blosc_decodes_every_seam_chunk():
    """the same chunks through c-blosc's own decoder - only where python-blosc is installed (it is not where this suite was written: until
    this test has run somewhere, c-blosc itself has not judged the writer)"""
    blosc = _blosc_or_skip()
    for typesize in bw.TYPESIZES:
        for blocksize in bw.BLOCKSIZES:
            for label, c, payload in bw.seam_chunks(typesize, blocksize):
                assert bytes(blosc.decompress(c)) == payload, label


def test_stock_blosc_decodes_every_map_chunk():
    """as above, for the binary-map chunks (csize > blocksize, permuted and gapped bstarts included)"""
    blosc = _blosc_or_skip()
    for label, nx, ny, frames in bw.map_chunk_cases():
        for c, data in frames:
            assert bytes(blosc.decompress(c)) == data, label
