"""LZ4 blocks and frames written sequence by sequence, for the tests of the three device LZ4 decoders (rc_lz4.hip::lz4_block_walk,
rc_zstd_dec.hip::lz4_block_decode, rc_blosc.hip::lz4_block_decode_wave).  Pure Python, no device, no project code: the formats are
lz4_Block_format.md and lz4_Frame_format.md, nothing else (the system's liblz4 comes in only where a test wants a stock encoder's blocks).

  block(seqs, tail)    -> (block bytes, decoded bytes)   seqs = [(literal bytes, offset, match length), ...], tail = the closing literals
  frame(blocks)        -> an LZ4 frame of these blocks (independent, or linked: every block may reach into the ones before it)
  CASES                -> the named catalogue: blocks that decode to 512 bytes (a binary map's tile) and to the smaller sizes a last
                          block takes, each with the set of features it exercises;  coverage(CASES) must equal FEATURES
  defects(size)        -> malformed blocks that claim `size` bytes, one per check a decoder must make
  mixed_frame(), linked_frames(), map_frame_cases(), big_map_frame() -> the frames the GPU tests decode and the CPU tests judge first

The expectation of a block never comes from a decoder under test: it is replay() of the sequence list, and parse() - a from-spec reader
of the emitted bytes - must give that list back (block() asserts it), so token nibbles, extension bytes and the +4 of a match length are
written and read once each, in this file, and judged by stock liblz4 in tests/test_lz4_block_writer_cpu.py.
"""
import ctypes as C
import ctypes.util
import random
import struct

MINMATCH = 4

# what the catalogue must reach (the lengths are those at which a nibble, an extension byte or a 64-lane trip begins or ends)
LIT_RUNS = (0, 14, 15, 16, 64, 65, 269, 270, 271)             # 15 = nibble 15 + byte 0, 270 = 15 + 255 + 0
MATCH_LENS = (4, 18, 19, 20, 64, 65, 129, 273, 274, 275)      # 19 = 4 + 15 + 0, 274 = 4 + 15 + 255 + 0
OFFSETS = (1, 2, 3, 5, 7, 8, 9, 63, 64, 65, "op")             # "op": the offset equals the bytes written so far (reaches the block's first byte)
RELATIONS = ("lt", "eq", "gt", "gt64")                        # match length <, ==, > its offset, >= offset + 64
SIZES = (1, 7, 8, 13, 56, 63, 64, 71, 72, 127, 438, 512)      # decoded sizes: a tile, and the last blocks the blosc tests ask for


def _feasible(off, rel):
    """a match is at least 4 bytes: no `lt` below offset 5, no `eq` below 4"""
    lo = 4 if off == "op" else off
    return rel in ("gt", "gt64") or (rel == "lt" and (off == "op" or lo > 4)) or (rel == "eq" and (off == "op" or lo >= 4))


FEATURES = tuple(
    ["lit:%d" % n for n in LIT_RUNS] + ["ml:%d" % n for n in MATCH_LENS] +
    ["off:%s:%s" % (o, r) for o in OFFSETS for r in RELATIONS if _feasible(o, r)] +
    ["size:%d" % n for n in SIZES] +
    ["literals-only", "literals-only:512",           # no match at all; 512 bytes of them: 515 compressed bytes, more than the block holds
     "off2..7:ragged",                                # offset 2..7 with a length that is no multiple of it
     "chain:mm",                                      # a match directly behind a match (zero literals)
     "chain:near-then-off1:zero", "chain:near-then-off1:nonzero",   # offset 2..7 then offset 1, the copied byte in front zero / not zero
     "chain:far-then-off1:zero", "chain:far-then-off1:nonzero",     # the same behind an offset >= 8 (whole 8-byte steps, then a short one)
     "off1-after-lit:zero", "off1-after-lit:nonzero",  # offset 1 behind a literal that ends in 0 / in something else
     "src:allzero",                                   # offset > 1, every source byte zero (bytes a sparse sink never stored)
     "src:straddle-unaligned"])                       # offset > 1, source holds zero and non-zero bytes and starts off an 8-byte boundary


def _ext(n):
    """the bytes behind a nibble of 15 for a length of 15 + n"""
    return b"\xff" * (n // 255) + bytes([n % 255])


def encode(seqs, tail):
    """token, literal-length bytes, literals, little-endian offset, match-length bytes - per sequence; the last sequence is literals alone.
    Nothing is checked: defects() uses this to write blocks no decoder may accept."""
    out = bytearray()
    for lit, off, ml in seqs:
        m = ml - MINMATCH
        out.append((min(len(lit), 15) << 4) | min(m, 15))
        if len(lit) >= 15:
            out += _ext(len(lit) - 15)
        out += lit
        out += struct.pack("<H", off)
        if m >= 15:
            out += _ext(m - 15)
    out.append(min(len(tail), 15) << 4)
    if len(tail) >= 15:
        out += _ext(len(tail) - 15)
    out += tail
    return bytes(out)


def parse(blk):
    """block bytes -> (seqs, tail), reading what encode() wrote by the format document; ValueError where the bytes run out"""
    seqs, ip, n = [], 0, len(blk)

    def more(v):
        nonlocal ip
        while True:
            if ip >= n:
                raise ValueError("length bytes cut off")
            x = blk[ip]
            ip += 1
            v += x
            if x != 255:
                return v
    while True:
        if ip >= n:
            raise ValueError("no closing literals")
        token = blk[ip]
        ip += 1
        lit = token >> 4
        if lit == 15:
            lit = more(lit)
        if ip + lit > n:
            raise ValueError("literals run past the block")
        data = bytes(blk[ip:ip + lit])
        ip += lit
        if ip == n:
            return seqs, data
        if ip + 2 > n:
            raise ValueError("offset cut off")
        off = blk[ip] | (blk[ip + 1] << 8)
        ip += 2
        ml = token & 15
        if ml == 15:
            ml = more(ml)
        ml = ml + MINMATCH
        seqs.append((data, off, ml))


def replay(seqs, tail, history=b""):
    """the bytes the sequences stand for: a plain serial copy into a zeroed buffer; history = what a linked block may reach back into"""
    base = len(history)
    out = bytearray(history) + bytearray(sum(len(lit) + ml for lit, _, ml in seqs) + len(tail))
    op = base
    for lit, off, ml in seqs:
        out[op:op + len(lit)] = lit
        op += len(lit)
        if off < 1 or off > op:
            raise ValueError("offset %d with %d bytes in front" % (off, op))
        src = out[op - off:op + ml]                     # the `off` bytes in front (and the zeros behind them), as they are BEFORE the copy
        for i in range(ml):
            out[op + i] = src[i % off]
        op += ml
    out[op:op + len(tail)] = tail
    return bytes(out[base:])


def conforms(seqs, tail):
    """the end-of-block rules an encoder keeps so that every stock decoder may use its fast paths: the last 5 bytes are literals, the last
    match starts at least 12 bytes before the end (blocks under 13 bytes hold no match)"""
    if not seqs:
        return True
    total = sum(len(lit) + ml for lit, _, ml in seqs) + len(tail)
    last_start = total - len(tail) - seqs[-1][2]
    return len(tail) >= 5 and last_start <= total - 12


def block(seqs, tail, history=b""):
    """-> (block bytes, decoded bytes)"""
    blk = encode(seqs, tail)
    got_seqs, got_tail = parse(blk)
    assert got_seqs == [(bytes(a), b, c) for a, b, c in seqs] and got_tail == bytes(tail)
    return blk, replay(got_seqs, got_tail, history)


MAGIC = b"\x04\x22\x4d\x18"
DESCRIPTOR = {False: b"\x60\x40\x82", True: b"\x40\x40\xc0"}   # FLG (version 01, independent or not), BD (64 KiB blocks), header checksum


def frame(blocks, linked=False):
    """blocks: LZ4 block bytes, or ("stored", bytes) for an uncompressed block (bit 31 of its size word)"""
    out = bytearray(MAGIC + DESCRIPTOR[bool(linked)])
    for b in blocks:
        if isinstance(b, tuple):
            out += struct.pack("<I", len(b[1]) | 0x80000000) + b[1]
        else:
            out += struct.pack("<I", len(b)) + b
    return bytes(out + struct.pack("<I", 0))


# ---- the catalogue -----------------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, name, seqs, tail):
        self.name, self.seqs, self.tail = name, seqs, tail
        self.block, self.decoded = block(seqs, tail)
        self.size = len(self.decoded)
        self.features = features_of(seqs, tail)
        assert conforms(seqs, tail), name
        assert len(self.block) != self.size, name       # (a blosc block of exactly its decoded size means "stored")

    def __repr__(self):
        return "Case(%s)" % self.name


def features_of(seqs, tail):
    """what a sequence list exercises, worked out from the list itself (and the bytes it stands for)"""
    f = set()
    out = replay(seqs, tail)
    f.add("size:%d" % len(out))
    if not seqs:
        f.add("literals-only")
        if len(out) == 512:
            f.add("literals-only:512")
    op, prev_off = 0, None
    for idx, (lit, off, ml) in enumerate(seqs):
        if len(lit) in LIT_RUNS:
            f.add("lit:%d" % len(lit))
        op += len(lit)
        if ml in MATCH_LENS:
            f.add("ml:%d" % ml)
        rel = "lt" if ml < off else "eq" if ml == off else "gt" if ml < off + 64 else "gt64"
        if off in OFFSETS:
            f.add("off:%d:%s" % (off, rel))
        if off == op:
            f.add("off:op:%s" % rel)
        if 2 <= off <= 7 and ml % off:
            f.add("off2..7:ragged")
        if not lit and idx:
            f.add("chain:mm")
            if off == 1 and prev_off >= 2:
                f.add("chain:%s-then-off1:%s" % ("near" if prev_off < 8 else "far", "zero" if out[op - 1] == 0 else "nonzero"))
        if lit and off == 1:
            f.add("off1-after-lit:%s" % ("zero" if lit[-1] == 0 else "nonzero"))
        src = out[op - off:op - off + min(off, ml)]
        if off > 1 and not any(src):
            f.add("src:allzero")
        if off > 1 and any(src) and 0 in src and (op - off) % 8:
            f.add("src:straddle-unaligned")
        op += ml
        prev_off = off
    return f


def build(name, size, ops, seed=0):
    """ops: ("L", n) n random non-zero literal bytes | ("Z", n) n zero literal bytes | ("S", n) n sparse ones (mostly zero) |
    ("B", bytes) these literal bytes | ("M", offset or "op", length).  Literal ops in a row make one run; the tail is filled up to `size`
    with sparse bytes (what a binary map looks like) that end in a non-zero one."""
    r = random.Random("%s/%d" % (name, seed))

    def some(kind, n):
        if kind == "L":
            return bytes(r.randrange(1, 256) for _ in range(n))
        if kind == "Z":
            return bytes(n)
        return bytes(r.randrange(1, 256) if r.random() < 0.15 else 0 for _ in range(n))
    seqs, lit, op = [], bytearray(), 0
    for o in ops:
        if o[0] == "M":
            off = op if o[1] == "op" else o[1]
            seqs.append((bytes(lit), off, o[2]))
            lit = bytearray()
            op += o[2]
        else:
            data = o[1] if o[0] == "B" else some(o[0], o[1])
            lit += data
            op += len(data)
    assert op <= size, (name, op, size)
    fill = bytearray(some("S", size - op))
    if fill:
        fill[-1] = fill[-1] or 0x81
    return Case(name, seqs, bytes(lit + fill))


def _grid_cases():
    """every (offset, relation) pair with a length from MATCH_LENS where one fits, packed into 512-byte blocks; the four blocks open with
    the off == op matches"""
    want = {  # (offset, relation) -> match length
        "lt": {5: 4, 7: 4, 8: 4, 9: 4, 63: 18, 64: 19, 65: 64},
        "eq": {5: 5, 7: 7, 8: 8, 9: 9, 63: 63, 64: 64, 65: 65},
        "gt": {1: 4, 2: 5, 3: 20, 5: 18, 7: 20, 8: 19, 9: 65, 63: 64, 64: 65, 65: 100},
        "gt64": {1: 65, 2: 129, 3: 273, 5: 274, 7: 275, 8: 129, 9: 129, 63: 129, 64: 129, 65: 129},
    }
    entries = [(off, ml) for rel in RELATIONS for off, ml in want[rel].items()]
    openers = [[("L", 6), ("M", "op", 4)], [("L", 5), ("M", "op", 5)], [("L", 3), ("M", "op", 20)], [("L", 2), ("M", "op", 129)]]
    gaps = [1, 2, 14, 3, 15, 1, 16, 5]
    cases, ops, op, k = [], [], 0, 0

    def close():
        nonlocal ops, op
        cases.append(build("grid%d" % len(cases), 512, ops))
        ops, op = [], 0
    for off, ml in entries:
        while True:
            if not ops and openers:
                ops = list(openers.pop(0))
                op = ops[0][1] + ops[1][2]
            lit = max(gaps[k % len(gaps)], off - op)
            if op + lit + ml + 12 <= 512:
                break
            close()
        ops += [("L", lit), ("M", off, ml)]
        op += lit + ml
        k += 1
    close()
    while openers:
        ops = list(openers.pop(0))
        close()
    return cases


def _make_cases():
    c = _grid_cases()
    # literal runs in front of a match: every length of LIT_RUNS (0 = the match follows a match)
    c.append(build("lit_0_14_15_16_64_65", 512, [("L", 14), ("M", 7, 4), ("L", 15), ("M", 9, 5), ("L", 16), ("M", 8, 4), ("M", 2, 6), ("L", 64),
                                               ("M", 63, 4), ("L", 65), ("M", 65, 4)]))
    c.append(build("lit_269", 512, [("S", 268), ("L", 1), ("M", 64, 18)]))
    c.append(build("lit_270", 512, [("S", 269), ("L", 1), ("M", 1, 19)]))
    c.append(build("lit_271", 512, [("S", 270), ("L", 1), ("M", 3, 20)]))
    c.append(build("literals_512", 512, []))
    # zero-literal chains; the byte in front of the offset-1 match is the last one the match before it copied
    c.append(build("chain_near", 512, [("B", b"\x11\x22\x00\x33\x44"), ("M", 5, 8), ("M", 1, 5),                # copies 11 22 00 33 44 11 22 00: ends on zero
                                       ("L", 3), ("B", b"\x55\x66\x77\x00\x88"), ("M", 5, 8), ("M", 1, 6),      # ends on 77
                                       ("L", 2), ("M", 2, 5), ("M", 1, 4), ("M", 3, 7), ("M", 9, 11)]))
    c.append(build("chain_far", 512, [("B", b"\x01\x02\x03\x04\x05\x06\x07\x08\x09\x0a\x00\x0c"), ("M", 12, 11), ("M", 1, 9),   # ends on the 00
                                      ("L", 1), ("B", b"\x21\x22\x23\x24\x25\x26\x27\x28\x29\x2a\x2b"), ("M", 11, 19), ("M", 1, 7),  # 8 + 8 + 3: ends on 28
                                      ("L", 9), ("M", 64, 70), ("M", 1, 18), ("M", 65, 64)]))
    c.append(build("off1_after_literal", 512, [("L", 3), ("B", b"\x00"), ("M", 1, 40), ("L", 5), ("M", 1, 64), ("Z", 2), ("M", 1, 200), ("B", b"\x7f"),
                                               ("M", 1, 5)]))
    # sources the sparse sink never stored, and sources that straddle stored and skipped bytes away from an 8-byte boundary
    c.append(build("zero_sources", 512, [("L", 3), ("Z", 16), ("M", 9, 20), ("M", 30, 45), ("L", 1), ("Z", 70), ("M", 65, 129), ("L", 2), ("M", 200, 64)]))
    c.append(build("straddle", 512, [("B", b"\xa1\xa2\xa3\x00\x00\x00\x00\x00\x00\x00\x00\xb1\xb2\x00\x00\x00\x00\x00\xc1"), ("M", 17, 30), ("L", 1),
                                     ("M", 9, 9), ("Z", 5), ("B", b"\xd1"), ("M", 3, 17), ("Z", 11), ("M", 13, 65), ("L", 1), ("M", 127, 100)]))
    c.append(build("zeros", 512, [("Z", 1), ("M", 1, 499), ("Z", 12)]))                   # this library's own dialect: [literal 0][offset 1]
    # the sizes of a last block: nothing but literals under 13 bytes, the same ideas where they fit
    c.append(build("size1", 1, []))
    c.append(build("size7", 7, []))
    c.append(build("size8", 8, []))
    c.append(build("size13", 13, [("L", 1), ("M", 1, 7)]))
    c.append(build("size56", 56, [("L", 2), ("M", 2, 19), ("Z", 3), ("M", 5, 18)]))
    c.append(build("size63", 63, [("L", 5), ("M", "op", 7), ("M", 1, 4), ("L", 15), ("M", 3, 20)]))
    c.append(build("size64", 64, [("L", 3), ("M", 3, 20), ("L", 2), ("M", 1, 4), ("Z", 14), ("M", 9, 9)]))
    c.append(build("size71", 71, [("L", 7), ("M", 7, 18), ("M", 1, 19), ("L", 1), ("M", 8, 4)]))
    c.append(build("size72", 72, [("L", 16), ("M", 9, 19), ("L", 14), ("M", 2, 5)]))
    c.append(build("size127", 127, [("S", 15), ("L", 1), ("M", 5, 65), ("M", 64, 20)]))
    c.append(build("size438", 438, [("L", 15), ("M", 2, 129), ("L", 16), ("M", 64, 65), ("S", 64), ("L", 1), ("M", 1, 64), ("M", 63, 18), ("L", 1), ("M", 300, 20)]))
    return c


def coverage(cases):
    out = set()
    for c in cases:
        out |= c.features
    return out


CASES = _make_cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def tiles(size=512):
    """the catalogue's cases that decode to `size` bytes, in catalogue order"""
    return [c for c in CASES if c.size == size]


# ---- blocks no decoder may accept ----------------------------------------------------------------------------------------------------------
def defects(size=512):
    """name -> block bytes that claim to hold `size` decoded bytes (size >= 64), each wrong in one way; every decoder must refuse each through
    the check named here:
      offset0            off == 0
      offset_past_start  off == op + 1 (one byte in front of the block)
      match_past_end     the last match ends one byte behind `size`
      literals_past_end  a literal run longer than the bytes left in the block
      length_cut         the block ends inside the extension bytes of a length"""
    r = random.Random("defects/%d" % size)
    lit = bytes(r.randrange(1, 256) for _ in range(20))
    fill = bytes(r.randrange(1, 256) for _ in range(size))
    good = encode([(lit, 7, 20)], fill[:size - 40])
    assert len(replay(*parse(good))) == size
    out = {
        "offset0": encode([(lit, 0, 20)], fill[:size - 40]),
        "offset_past_start": encode([(lit, 21, 20)], fill[:size - 40]),
        "match_past_end": encode([(lit, 7, 20), (fill[:size - 60], 9, 21)], b""),   # 20 + 20 + (size - 60) + 21 = size + 1, nothing behind it
        "literals_past_end": good[:-5],                                              # the closing run announces 5 bytes more than there are
        "length_cut": encode([(lit, 7, 20)], b"")[:-1] + b"\xf0\xff",                # ... token 15|0, one length byte 255, end
    }
    assert len(replay(*parse(out["match_past_end"]))) == size + 1
    return out


# ---- frames the thread decoder (de_compress(2, ...)) must take ------------------------------------------------------------------------------
def mixed_frame():
    """-> (frame, decoded): every catalogue block in one frame of independent blocks, a stored block behind every third"""
    r = random.Random("mixed")
    blocks, decoded = [], b""
    for i, c in enumerate(CASES):
        blocks.append(c.block)
        decoded += c.decoded
        if i % 3 == 2:
            raw = bytes(r.randrange(256) for _ in range((17, 512, 1, 700)[(i // 3) % 4]))
            blocks.append(("stored", raw))
            decoded += raw
    return frame(blocks), decoded


def linked_frames():
    """-> [(name, frame, decoded)]: two linked blocks of 64 KiB each; the second opens with a match (no literal in front) that reaches into
    the first - at offset 65535, the format's largest, and at small offsets - and keeps reaching back further on.  The first block is once
    an LZ4 block and once stored."""
    r = random.Random("linked")
    lit = bytes(r.randrange(1, 256) if r.random() < 0.3 else 0 for _ in range(1000))
    rest = bytes(r.randrange(1, 256) if r.random() < 0.3 else 0 for _ in range(65536 - 1000 - 30000 - 5 - 20000))
    first_blk, first = block([(lit, 999, 30000), (b"\x01\x02\x03\x04\x05", 1, 20000)], rest)
    assert len(first) == 65536
    out = []
    for name, opening in (("far", [(b"", 65535, 30000), (b"\x0a\x0b\x0c", 3, 10), (b"", 65535, 30000), (b"\x0d\x0e", 40000, 5000)]),
                          ("near", [(b"", 1, 9), (b"", 7, 30), (b"\x21", 65, 129), (b"", 65535, 65000)])):
        used = sum(len(a) + c for a, _, c in opening)
        tail = bytes(r.randrange(1, 256) for _ in range(65536 - used))
        second_blk, second = block(opening, tail, history=first)
        assert len(second) == 65536 and conforms(opening, tail)
        out.append((name + "/compressed-first", frame([first_blk, second_blk], linked=True), first + second))
        out.append((name + "/stored-first", frame([("stored", first), second_blk], linked=True), first + second))
    return out


# ---- stock liblz4, where a test wants blocks a real encoder chose ---------------------------------------------------------------------------
_LZ4 = None


def liblz4():
    """the system's liblz4; the tests that need it fail without it (it is their judge)"""
    global _LZ4
    if _LZ4 is None:
        name = ctypes.util.find_library("lz4")
        if not name:
            raise RuntimeError("liblz4 not found")
        L = C.CDLL(name)
        L.LZ4_compress_default.restype = C.c_int
        L.LZ4_compress_default.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int]
        L.LZ4_decompress_safe.restype = C.c_int
        L.LZ4_decompress_safe.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int]
        _LZ4 = L
    return _LZ4


def stock_lz4(stream, b=0, j=0):
    """LZ4_compress_default, and the bytes themselves where that does not shrink them - what c-blosc does"""
    stream = bytes(stream)
    dst = C.create_string_buffer(len(stream) + len(stream) // 255 + 32)
    k = liblz4().LZ4_compress_default(stream, dst, len(stream), len(dst))
    assert k > 0
    return dst.raw[:k] if k < len(stream) else stream


# ---- binary maps for the lane decoder (rc_expand_frames, scheme 2): LZ4 frames of independent blocks, one block per 512-byte tile -----------
def motif_map(ny=64, nx=512, z=0):
    """the bytes of a ny x nx binary map of repeated small motifs: stock liblz4 finds matches at many offsets inside every tile"""
    rows = []
    for y in range(ny):
        row = [0] * nx
        if y % 2 == 0:
            for x in range((7 * y + 3 * z) % 16, nx, 16):
                row[x] = 1
            for x in range((5 * y + z) % 48, nx, 48):
                row[x] = 1
        rows += row
    return bytes(sum(rows[8 * i + k] << k for k in range(8)) for i in range(len(rows) // 8))


def map_frame(tiles_, layout="uniform"):
    """tiles_: per tile a Case, ("stored", bytes), ("stock", bytes) or ("literal", bytes) -> (LZ4 frame, the map's bytes).
    layout "split-first": the first tile goes as two stored halves, so the stream is no longer one block per tile of 512 bytes."""
    blocks, decoded = [], b""
    for i, t in enumerate(tiles_):
        if isinstance(t, Case):
            blk, data = t.block, t.decoded
        elif t[0] == "stock":
            data = bytes(t[1])
            blk = stock_lz4(data)
            blk = ("stored", data) if blk == data else blk
        elif t[0] == "literal":
            blk, data = block([], bytes(t[1]))
        else:
            blk, data = ("stored", bytes(t[1])), bytes(t[1])
        if i == 0 and layout == "split-first":
            h = len(data) // 2
            blocks += [("stored", data[:h]), ("stored", data[h:])]
        else:
            blocks.append(blk)
        decoded += data
    return frame(blocks), decoded


MAP_FRAME_LABELS = (["catalogue/uniform", "catalogue/split-first", "catalogue/stored-between"] +
                    ["last%d/%s" % (n, layout) for n in (438, 71, 13, 1) for layout in ("uniform", "split-first")])   # (what map_frame_cases() yields)


def map_frame_cases():
    """-> [(label, nx, ny, [(LZ4 frame, map bytes), ...])]: what the GPU test feeds rc_expand_frames with scheme 2, and the CPU test feeds
    liblz4 first.  Frames of 64 x 512 pixels hold 8 tiles."""
    r = random.Random("maps")
    t512 = tiles(512)
    sets = [t512[i:i + 8] for i in range(0, len(t512), 8)]
    sets[-1] = sets[-1] + t512[:8 - len(sets[-1])]
    rnd = bytes(r.randrange(256) for _ in range(512))
    out = []
    for layout in ("uniform", "split-first"):
        out.append(("catalogue/" + layout, 512, 64, [map_frame(s, layout) for s in sets]))
    with_stored = [t512[0], ("stored", rnd), t512[11], ("stored", bytes(512)), t512[12], t512[13], ("stored", rnd[::-1]), t512[6]]
    out.append(("catalogue/stored-between", 512, 64, [map_frame(with_stored)]))
    for last in (438, 71, 13, 1):                                       # a last block of fewer bytes behind two whole tiles
        small = [c for c in CASES if c.size == last][0]
        for layout in ("uniform", "split-first"):
            out.append(("last%d/%s" % (last, layout), 1024 + last, 8, [map_frame([t512[3], t512[13], small], layout)]))
    return out


# Bytes of a workgroup's compressed blocks the lane decoder stages in LDS; lanes whose block lies behind them read global memory.  This restates
# the last template argument of rc_zstd_dec.hip's launches `k_block_decode<EMIT_LZ4, true, 128, 32768>` and `k_bitmap_decode_c<EMIT_LZ4, 128, 32768>`
# (128 = blocks per workgroup): if that changes there, change it here, or big_map_frame() no longer reaches the global-memory copy.
SPAN = 32768


def big_map_frame(layout="uniform"):
    """-> (LZ4 frame, map bytes, offset of every block's size word in the frame): 512 x 1024 pixels = 128 tiles = ONE workgroup of the lane
    decoder.  Tiles 0..69 are literals-only blocks (515 bytes each: 70 x 519 > SPAN), so every later tile - the whole catalogue, then stock
    liblz4 blocks of the motif map - is decoded from global memory."""
    r = random.Random("big")
    t512 = tiles(512)
    motif = motif_map(8 * 40, 512, 1)                                   # 64 bytes a row: 8 rows a tile
    spec = [("literal", bytes(r.randrange(1, 256) if r.random() < 0.1 else 0 for _ in range(512))) for _ in range(70)]
    spec += t512
    spec += [("stock", motif[512 * i:512 * (i + 1)]) for i in range(128 - len(spec))]
    assert len(spec) == 128
    f, data = map_frame(spec, layout)
    offs, q = [], 7
    while True:
        w, = struct.unpack_from("<I", f, q)
        if w == 0:
            break
        offs.append(q)
        q += 4 + (w & 0x7FFFFFFF)
    return f, data, offs
