"""blosc1 chunks (LZ4 codec) written block by block, for the tests of the device blosc decoders (rc_blosc.hip::k_blosc_decode_blocks behind
rc_expand_frames scheme 8, rc_blosc.hip::k_blosc_unshuffle behind de_compress(8)).  The layout is the one at the head of rc_blosc.hip and in
c-blosc 1.x's README_CHUNK_FORMAT.rst / blosc.c:

  header 16 B: version 2 | versionlz 1 | flags | typesize | int32 nbytes | int32 blocksize | int32 cbytes
  flags: 0x01 byte shuffle | 0x02 memcpyed (the payload follows the header as it is) | 0x04 bit shuffle | 0x10 blocks not split | 0x20 LZ4
  int32 bstarts[nblocks], then the blocks wherever bstarts says: per stream int32 csize + csize bytes, csize == the stream's size: stored.
  A block that is not the leftover one holds `typesize` streams when the chunk is split (allowed where typesize <= 16 and
  blocksize / typesize >= 128), one otherwise.

numpy does the shuffles; the expectation of a chunk is always the payload it was made from.  No project code, no device.
"""
import struct

import numpy as np

import lz4_block_writer as lzw
from lz4_block_writer import stock_lz4

NOSHUFFLE, SHUFFLE, BITSHUFFLE = 0, 1, 4


def bit_shuffle(block, typesize):
    """c-blosc's blosc_internal_bitshuffle (bitshuffle's bshuf_trans_bit_elem): with S elements - rounded DOWN to a multiple of 8 - row
    r = 8 * k + b of the output holds bit b of byte k of every element, S / 8 bytes, element i at bit i % 8 of byte i / 8; the bytes behind
    the S elements are copied.  A block shorter than an element is left alone."""
    a = np.frombuffer(bytes(block), np.uint8)
    if a.size < typesize:
        return a.tobytes()
    S = (a.size // typesize) // 8 * 8
    if not S:
        return a.tobytes()
    bits = np.unpackbits(a[:S * typesize].reshape(S, typesize), axis=1, bitorder="little")      # [element][8 * k + b]
    rows = np.packbits(bits.T, axis=1, bitorder="little")                                        # [8 * k + b][S / 8]
    return rows.tobytes() + a[S * typesize:].tobytes()


def bit_unshuffle(block, typesize):
    a = np.frombuffer(bytes(block), np.uint8)
    if a.size < typesize:
        return a.tobytes()
    S = (a.size // typesize) // 8 * 8
    if not S:
        return a.tobytes()
    rows = np.unpackbits(a[:S * typesize].reshape(8 * typesize, S // 8), axis=1, bitorder="little")   # [8 * k + b][element]
    return np.packbits(rows.T, axis=1, bitorder="little").tobytes() + a[S * typesize:].tobytes()


def byte_shuffle(block, typesize):
    """c-blosc's shuffle: byte k of every whole element, element after element, for k = 0 .. typesize - 1; the rest of the block is copied"""
    a = np.frombuffer(bytes(block), np.uint8)
    ne = a.size // typesize
    if typesize <= 1 or not ne:
        return a.tobytes()
    return a[:ne * typesize].reshape(ne, typesize).T.tobytes() + a[ne * typesize:].tobytes()


def byte_unshuffle(block, typesize):
    a = np.frombuffer(bytes(block), np.uint8)
    ne = a.size // typesize
    if typesize <= 1 or not ne:
        return a.tobytes()
    return a[:ne * typesize].reshape(typesize, ne).T.tobytes() + a[ne * typesize:].tobytes()


def shuffled(block, typesize, shuffle):
    return bit_shuffle(block, typesize) if shuffle == BITSHUFFLE else byte_shuffle(block, typesize) if shuffle == SHUFFLE else bytes(block)


def unshuffled(block, typesize, shuffle):
    return bit_unshuffle(block, typesize) if shuffle == BITSHUFFLE else byte_unshuffle(block, typesize) if shuffle == SHUFFLE else bytes(block)


def may_split(typesize, blocksize):
    """blosc.c's rule for the blocks in front of the leftover one"""
    return typesize <= 16 and blocksize // typesize >= 128


# ---- how a stream (a block, or one of a split block's `typesize` parts) is written: f(stream bytes, block index, part index) -> bytes ------
def stored(stream, b=0, j=0):
    return bytes(stream)


def mixed(stream, b=0, j=0):
    """stored and stock-compressed streams side by side"""
    return stored(stream) if (b + j) % 3 == 1 else stock_lz4(stream)


def chunk(payload, typesize=8, blocksize=512, shuffle=BITSHUFFLE, split=False, encode=stock_lz4, order=None, memcpyed=False, gap=0):
    """-> the chunk's bytes.  order: the blocks' places in the body (a permutation of their indices: order[0] is written first); gap: unused
    bytes in front of every block (an int, or a function of the block's index)."""
    payload = bytes(payload)
    nbytes = len(payload)
    bs = min(blocksize, nbytes) if nbytes else blocksize
    flags = (shuffle & 5) | (0 if split else 0x10) | 0x20 | (0x02 if memcpyed else 0)
    if split and not may_split(typesize, bs):
        raise ValueError("c-blosc does not split blocks of %d bytes at typesize %d" % (bs, typesize))
    head = bytes([2, 1, flags, typesize])
    if memcpyed:
        return head + struct.pack("<iii", nbytes, bs, 16 + nbytes) + payload
    nblocks = -(-nbytes // bs) if nbytes else 0
    bodies = []
    for b in range(nblocks):
        raw = payload[b * bs:(b + 1) * bs]
        sh = shuffled(raw, typesize, shuffle)
        nsplits = typesize if split and len(raw) == bs else 1
        ne = len(raw) // nsplits
        assert ne * nsplits == len(raw)
        body = b""
        for j in range(nsplits):
            stream = sh[j * ne:(j + 1) * ne]
            c = encode(stream, b, j)
            assert c and (len(c) != len(stream) or c == stream), "a stream of its own size must be the stored stream"
            body += struct.pack("<i", len(c)) + c
        bodies.append(body)
    order = list(range(nblocks)) if order is None else list(order)
    assert sorted(order) == list(range(nblocks))
    pos, bstarts, out = 16 + 4 * nblocks, [0] * nblocks, bytearray()
    for b in order:
        g = gap(b) if callable(gap) else gap
        out += b"\xee" * g
        pos += g
        bstarts[b] = pos
        out += bodies[b]
        pos += len(bodies[b])
    return head + struct.pack("<iii", nbytes, bs, pos) + struct.pack("<%di" % nblocks, *bstarts) + bytes(out)


def bstarts(chunk_bytes):
    nbytes, bs = struct.unpack_from("<ii", chunk_bytes, 4)
    nblocks = -(-nbytes // bs) if nbytes else 0
    return list(struct.unpack_from("<%di" % nblocks, chunk_bytes, 16))


# ---- chunks for de_compress(8, ...): every typesize, blocksize, shuffle, split and stream form -----------------------------------------------
TYPESIZES = (1, 2, 4, 8, 16)
BLOCKSIZES = (64, 512, 4096, 32768)


def seam_payload(typesize, blocksize, nbytes):
    """counters of `typesize` bytes (what a shuffle helps), sparse bytes, and a stretch of noise (streams that do not shrink: stored)"""
    rng = np.random.default_rng([typesize, blocksize, nbytes])
    a = np.where(rng.random(nbytes) < 0.1, rng.integers(1, 256, nbytes), 0).astype(np.uint8)
    q = nbytes // 4
    a[:q] = (np.arange(q) // typesize) % 251
    a[2 * q:3 * q] = rng.integers(0, 256, q)
    return a.tobytes()


def seam_chunks(typesize, blocksize):
    """yields (label, chunk, payload).  Lengths: whole blocks and a leftover block that is (a) a multiple of typesize but not of 8 x typesize,
    (b) no multiple of typesize, (c) shorter than typesize (typesize 1: no leftover at all); and, once per typesize, a payload shorter than
    one element."""
    nfull = 3 if blocksize <= 4096 else 2
    k = 11 if 11 * typesize < blocksize else 3
    tails = {"whole-elements": k * typesize, "ragged": k * typesize + (typesize - 1 if typesize > 1 else 5), "short": typesize - 1}
    for shuffle in (NOSHUFFLE, SHUFFLE, BITSHUFFLE):
        for split in (False, True):
            if split and not may_split(typesize, blocksize):
                continue
            for enc in (stored, stock_lz4, mixed):
                for tname, tail in tails.items():
                    payload = seam_payload(typesize, blocksize, nfull * blocksize + tail)
                    label = "ts%d bs%d shuffle%d split%d %s %s" % (typesize, blocksize, shuffle, split, enc.__name__, tname)
                    yield label, chunk(payload, typesize, blocksize, shuffle, split, enc), payload
    if blocksize == BLOCKSIZES[0] and typesize > 1:
        payload = seam_payload(typesize, blocksize, 64)[10:10 + typesize - 1]
        for shuffle in (NOSHUFFLE, SHUFFLE, BITSHUFFLE):
            for enc in (stored, lambda s, b, j: lzw.block([], s)[0]):
                yield "ts%d tiny shuffle%d" % (typesize, shuffle), chunk(payload, typesize, blocksize, shuffle, False, enc), payload


# ---- binary maps for the wave decoder (rc_expand_frames, scheme 8): typesize 8, blocks of 512 bytes -------------------------------------------
LAST_BLOCKS = (1, 7, 8, 13, 56, 63, 64, 71, 72, 127, 128, 135, 438)   # 63 | 64 and 127 | 128: either side of 8 and of 16 shuffled elements


def _from_catalogue(cases):
    """the LZ4 block of tile b is the catalogue's block: its decoded bytes must be the stream the chunk holds there"""
    def enc(stream, b, j):
        assert stream == cases[b].decoded, cases[b].name
        return cases[b].block
    return enc


def catalogue_chunk(cases, shuffle, **kw):
    """-> (chunk, map bytes): the catalogue's decoded blocks are the chunk's (shuffled) blocks, so the map is their un-shuffled image"""
    payload = b"".join(unshuffled(c.decoded, 8, shuffle) for c in cases)
    assert all(c.size == 512 for c in cases[:-1])
    return chunk(payload, 8, 512, shuffle, False, _from_catalogue(cases), **kw), payload


MAP_CHUNK_LABELS = (["%s/%s" % (kind, name) for name in ("bitshuffle", "noshuffle") for kind in ("catalogue", "stock-motif")] + ["order", "gap", "memcpyed"] +
                    ["last%d/%s" % (n, tag) for n in LAST_BLOCKS for tag in ("single", "behind-a-tile")])   # (what map_chunk_cases() yields)


def map_chunk_cases():
    """-> [(label, nx, ny, [(chunk, map bytes), ...])]: what the GPU test feeds rc_expand_frames with scheme 8, and the CPU test feeds the
    from-spec decoder first.  Frames of 64 x 512 pixels hold 8 tiles."""
    rng = np.random.default_rng(88)
    t512 = lzw.tiles(512)
    sets = [t512[i:i + 8] for i in range(0, len(t512), 8)]
    sets[-1] = sets[-1] + t512[:8 - len(sets[-1])]
    out = []
    for shuffle, name in ((BITSHUFFLE, "bitshuffle"), (NOSHUFFLE, "noshuffle")):
        out.append(("catalogue/" + name, 512, 64, [catalogue_chunk(s, shuffle) for s in sets]))
        motif = [lzw.motif_map(64, 512, z) for z in range(2)]
        out.append(("stock-motif/" + name, 512, 64, [(chunk(m, 8, 512, shuffle, False, stock_lz4), m) for m in motif]))
    perm = [int(i) for i in rng.permutation(8)]
    assert perm != sorted(perm) and perm != sorted(perm, reverse=True)
    out.append(("order", 512, 64, [catalogue_chunk(sets[0], BITSHUFFLE, order=list(range(7, -1, -1))), catalogue_chunk(sets[1], BITSHUFFLE, order=perm),
                                   catalogue_chunk(sets[2], NOSHUFFLE, order=perm[::-1], gap=3)]))
    out.append(("gap", 512, 64, [catalogue_chunk(sets[1], BITSHUFFLE, gap=lambda b: b % 4), catalogue_chunk(sets[0], BITSHUFFLE, gap=1),
                                 catalogue_chunk(sets[2], BITSHUFFLE, gap=lambda b: 3 - b % 4)]))
    sparse = np.where(rng.random(4096) < 0.1, rng.integers(1, 256, 4096), 0).astype(np.uint8).tobytes()
    out.append(("memcpyed", 512, 64, [(chunk(sparse, 8, 512, BITSHUFFLE, False, memcpyed=True), sparse), catalogue_chunk(sets[0], BITSHUFFLE),
                                      (chunk(sparse[::-1], 8, 512, NOSHUFFLE, False, memcpyed=True), sparse[::-1])]))
    for n in LAST_BLOCKS:
        small = [c for c in lzw.CASES if c.size == n]
        data = np.where(rng.random(n) < 0.3, rng.integers(1, 256, n), 0).astype(np.uint8).tobytes()
        for lead, tag in (([], "single"), ([t512[13]], "behind-a-tile")):
            frames = []
            for shuffle in (BITSHUFFLE, NOSHUFFLE):
                if small:
                    frames.append(catalogue_chunk(lead + small[:1], shuffle))
                head = unshuffled(lead[0].decoded, 8, shuffle) if lead else b""
                payload = head + data
                frames.append((chunk(payload, 8, 512, shuffle, False, stock_lz4), payload))
                frames.append((chunk(payload, 8, 512, shuffle, False, stored), payload))
                frames.append((chunk(payload, 8, 512, shuffle, False, lambda s, b, j: lzw.block([], s)[0]), payload))   # literals only: csize > size
            out.append(("last%d/%s" % (n, tag), len(lead) * 512 + n, 8, frames))
    return out


def streams(chunk_bytes):
    """-> [(csize, the stream's decoded size), ...] of a chunk that is not memcpyed, block after block"""
    flags, typesize = chunk_bytes[2], chunk_bytes[3]
    nbytes, bs = struct.unpack_from("<ii", chunk_bytes, 4)
    out = []
    for b, pos in enumerate(bstarts(chunk_bytes)):
        bsize = min(bs, nbytes - b * bs)
        nsplits = typesize if not flags & 0x10 and may_split(typesize, bs) and bsize == bs else 1
        for _ in range(nsplits):
            csize, = struct.unpack_from("<i", chunk_bytes, pos)
            out.append((csize, bsize // nsplits))
            pos += 4 + csize
    return out
