"""Serial restatement (test infrastructure) of the batched device inflate (pyrecode_amd/csrc/rc_inflate.h, rc_inflate.hip): how the
reader finds the units of a zlib stream the device DEFLATE encoder wrote without walking it.

    1. candidates   every byte position that may start a unit: offset 2, behind the empty stored block 00 00 FF FF that closes a coded
                    unit, behind a full stored unit (00, LEN = U, NLEN = ~U at p - 5 - U); U = 512 (binary map) or 32768 (values)
    2. decode       every candidate on its own -> (end, bytes, BFINAL) or None; a false candidate fails or ends somewhere: no error
    3. chain        end -> candidate from the candidate at offset 2: the real units, in order.  Exactly max(ceil(size / U), 1) of
                    them, U bytes each and the last one the rest, BFINAL on the last only, the chain ends 4 bytes before the stream's end
                    (the Adler-32, which is not checked).  Anything else: Refused - "not this encoder's stream, use the stock decoder".

The subset: stored blocks with zero padding bits; in a map stream fixed-Huffman blocks whose matches stay inside the unit; in a value
stream dynamic-Huffman blocks of literals only (HLIT 0, HDIST 0, lengths <= 12).  Also the catalogue of frames the CPU test
(test_inflate_chain_cpu.py: this model and the C++ core against zlib.decompress) and the GPU test (test_gpu_inflate.py: the kernels
against the same frames read from their uncompressed pieces) share."""
import zlib

import numpy as np

import deflate_block_model as dbm
import deflate_values_model as dvm

MAP, VALUES = 0, 1
UNIT = {MAP: 512, VALUES: 1 << 15}
MARKER = b"\x00\x00\xff\xff"
CAND_EXTRA = 64
MAXBITS = dvm.MAXBITS


class Refused(Exception):
    pass


def units_of(size, kind):
    return max((size + UNIT[kind] - 1) // UNIT[kind], 1)


def candidates(s, kind):
    U, n = UNIT[kind], len(s)
    H = 5 + U
    full = bytes([0, U & 255, U >> 8, ~U & 255, (~U >> 8) & 255])
    out = []
    for p in range(2, n - 4):
        if p == 2 or (p >= 6 and s[p - 4:p] == MARKER) or (p >= 2 + H and s[p - H:p - H + 5] == full):
            out.append(p)
    return out


class _Bits:
    """LSB-first reader; bits behind the trailer's start are an error (Refused is raised by the callers on None)"""

    def __init__(self, s, pos):
        self.s, self.p, self.lim = s, 8 * pos, 8 * (len(s) - 4)

    def get(self, n):
        if self.p + n > self.lim:
            raise EOFError
        v = 0
        for i in range(n):
            v |= ((self.s[self.p >> 3] >> (self.p & 7)) & 1) << i
            self.p += 1
        return v

    def code(self, n):              # Huffman codes arrive most significant bit first
        v = 0
        for _ in range(n):
            v = (v << 1) | self.get(1)
        return v

    def align(self):
        self.p = (self.p + 7) & ~7
        if self.p > self.lim:
            raise EOFError


def _close(r, bfinal):
    if bfinal:
        r.align()
        return True
    if r.get(3) != 0:
        return False
    r.align()
    return bytes(r.get(8) for _ in range(4)) == MARKER


def _stored(r, U):
    h = r.get(8)
    if h > 1:
        return None
    ln, nl = r.get(16), r.get(16)
    if ln ^ nl != 0xFFFF or ln > U:
        return None
    return bytes(r.get(8) for _ in range(ln)), h


def _fixed_symbol(r):
    c = r.code(7)
    if c <= 23:
        return 256 + c
    c = (c << 1) | r.get(1)
    if c <= 0xBF:
        return c - 0x30
    if c <= 0xC7:
        return 280 + c - 0xC0
    return 144 + ((c << 1) | r.get(1)) - 0x190


def _fixed(r, U):
    out = bytearray()
    while True:
        sym = _fixed_symbol(r)
        if sym < 256:
            if len(out) >= U:
                return None
            out.append(sym)
            continue
        if sym == 256:
            return bytes(out)
        if sym > 285:
            return None
        if sym < 265:
            ln = sym - 254
        elif sym == 285:
            ln = 258
        else:
            e = (sym - 261) >> 2
            ln = 3 + ((4 + ((sym - 261) & 3)) << e) + r.get(e)
        ds = r.code(5)
        if ds > 29:
            return None
        if ds < 4:
            dist = ds + 1
        else:
            de = (ds >> 1) - 1
            dist = 1 + ((2 + (ds & 1)) << de) + r.get(de)
        if dist > len(out) or len(out) + ln > U:       # a match never leaves the unit
            return None
        for _ in range(ln):
            out.append(out[-dist])


def _dynamic(r, U):
    if r.get(5) != 0 or r.get(5) != 0:                 # HLIT 0, HDIST 0: literals and the end-of-block code, one distance code
        return None
    hclen = r.get(4) + 4
    cl_len = [0] * 19
    for s in dvm.CL_ORDER[:hclen]:
        cl_len[s] = r.get(3)
    if sum(1 << (7 - l) for l in cl_len if l) != 1 << 7:     # a complete code-length code
        return None
    cl_dec = {(l, c): s for s, (l, c) in enumerate(zip(cl_len, dvm.canonical_codes(cl_len))) if l}
    lens = []
    while len(lens) < 258:
        code, n = 0, 0
        while (n, code) not in cl_dec:
            if n == 7:
                return None
            code, n = (code << 1) | r.get(1), n + 1
        s = cl_dec[(n, code)]
        if s < 16:
            lens.append(s)
            continue
        if s == 16:
            if not lens:
                return None
            run = [lens[-1]] * (3 + r.get(2))
        else:
            run = [0] * ((3 + r.get(3)) if s == 17 else (11 + r.get(7)))
        if len(lens) + len(run) > 258:
            return None
        lens += run
    lens = lens[:257]
    if max(lens) > MAXBITS or lens[256] == 0 or sum(1 << (MAXBITS - l) for l in lens if l) > 1 << MAXBITS:
        return None
    dec = {(l, c): s for s, (l, c) in enumerate(zip(lens, dvm.canonical_codes(lens))) if l}
    out = bytearray()
    while True:
        code, n = 0, 0
        while (n, code) not in dec:
            if n == MAXBITS:
                return None
            code, n = (code << 1) | r.get(1), n + 1
        s = dec[(n, code)]
        if s == 256:
            return bytes(out)
        if len(out) >= U:
            return None
        out.append(s)


def decode_candidate(s, p, kind):
    """(end, bytes, BFINAL) of the unit that starts at byte p, or None"""
    U = UNIT[kind]
    r = _Bits(s, p)
    try:
        btype = (s[p] >> 1) & 3
        if btype == 0:
            got = _stored(r, U)
            return None if got is None else (r.p >> 3, got[0], got[1])
        if btype != (1 if kind == MAP else 2):
            return None
        bfinal = r.get(1)
        r.get(2)
        data = _fixed(r, U) if kind == MAP else _dynamic(r, U)
        if data is None or not _close(r, bfinal):
            return None
        return r.p >> 3, data, bfinal
    except EOFError:
        return None


def host_refuses(s, kind):
    """the host's cheap refusal (rc_reader.hip): the zlib header and the type of the first block"""
    return len(s) < 8 or s[:2] != b"\x78\x01" or (s[2] & 6) not in (0, 2 if kind == MAP else 4)


def inflate(s, size, kind):
    """-> (the stream's bytes, units, candidates); Refused when the stream is not in the subset"""
    s = bytes(s)
    if host_refuses(s, kind):
        raise Refused("header")
    U, want = UNIT[kind], units_of(size, kind)
    cand = candidates(s, kind)
    if len(cand) > 2 * want + CAND_EXTRA:
        raise Refused("too many candidates")
    res = {p: decode_candidate(s, p, kind) for p in cand}          # every candidate on its own
    out, p, k = bytearray(), 2, 0
    while True:
        got = res.get(p)
        if got is None or k >= want:
            raise Refused("chain breaks at %d" % p)
        end, data, bfinal = got
        last = k + 1 == want
        if len(data) != (size - U * k if last else U) or bool(bfinal) != last:
            raise Refused("unit %d: %d bytes, BFINAL %d" % (k, len(data), bfinal))
        out += data
        k += 1
        if end == len(s) - 4:
            break
        p = end
    if k != want:
        raise Refused("%d units, not %d" % (k, want))
    return bytes(out), k, len(cand)


# ---- the catalogue: frames (binary map + packed values) whose streams cover the scheme's cases -----------------------------------------
def _bitmap_from_bytes(nx, ny, by):
    nb = (nx * ny + 7) // 8
    by = bytearray(by[:nb].ljust(nb, b"\0"))
    if (nx * ny) % 8:
        by[-1] &= (1 << ((nx * ny) % 8)) - 1          # pixels behind the frame's end are clear
    return bytes(by)


def _popcount(by):
    return int(np.unpackbits(np.frombuffer(by, np.uint8)).sum())


def _sparse(rng, nbytes, p):
    return np.packbits(rng.random(8 * nbytes) < p, bitorder="little").tobytes()


def _low_entropy(rng, n):
    return bytes(rng.choice(np.array([0, 1, 2, 3, 7, 16, 200], np.uint8), n, p=[.4, .25, .15, .1, .05, .03, .02]))


def _frame(name, nx, ny, d, bitmap, values=None, lengths=None, rng=None):
    bitmap = _bitmap_from_bytes(nx, ny, bitmap)
    npk = (_popcount(bitmap) * d + 7) // 8
    if values is None:
        values = rng.integers(0, 256, npk, dtype=np.uint8).tobytes()
    values = bytes(values[:npk].ljust(npk, b"\x55"))
    return dict(name=name, nx=nx, ny=ny, d=d, bitmap=bitmap, values=values, map_stream=dbm.bitmap_stream(bitmap),
                val_stream=dvm.encode_values(values, lengths))


def catalogue():
    rng = np.random.default_rng(20261018)
    out = []
    out.append(_frame("one_tile", 64, 64, 12, _sparse(rng, 512, 0.02), rng=rng))
    out.append(_frame("short_last_tile", 64, 65, 12, _sparse(rng, 520, 0.02), rng=rng))
    out.append(_frame("smaller_than_a_tile", 3, 5, 16, b"\x15\x42", rng=rng))
    out.append(_frame("no_set_pixel", 64, 64, 16, bytes(512), rng=rng))                  # a value stream of 0 bytes
    dense = rng.integers(0, 256, 512, dtype=np.uint8).tobytes()
    out.append(_frame("stored_then_coded", 128, 64, 8, dense + _sparse(rng, 512, 0.02), rng=rng))
    # a stored tile whose bytes hold the closing marker: 4-aligned and not, and once followed by a complete fixed block with its own marker
    inner = dbm.emit_fixed(b"\x01\x00\x00\x00\x00\x00\x00\x09", [], False)
    t = bytearray(rng.integers(1, 256, 512, dtype=np.uint8).tobytes())
    t[8:12] = MARKER
    t[101:105] = MARKER
    t[200:204] = MARKER
    t[204:204 + len(inner)] = inner
    t[301:305] = MARKER
    t[305:305 + len(inner)] = inner
    out.append(_frame("marker_in_stored_tile", 128, 96, 8, _sparse(rng, 512, 0.02) + bytes(t) + _sparse(rng, 512, 0.03), rng=rng))
    # values: coded / stored / coded chunks under one table; the map of such a frame is all stored tiles
    bm = _sparse(rng, 32768, 0.145)
    npk = _popcount(_bitmap_from_bytes(512, 512, bm)) * 2
    vals = _low_entropy(rng, 32768) + rng.integers(0, 256, 32768, dtype=np.uint8).tobytes() + _low_entropy(rng, npk - 65536)
    lengths = dvm.fit_lengths(dvm.sample_hist(vals[:32768]))
    out.append(_frame("values_coded_stored_coded", 512, 512, 16, bm, vals, lengths))
    # values: stored chunks (compression_level 1), one of which holds the marker - also right behind a chunk's header
    bm = _sparse(rng, 8192, 0.55)
    npk = _popcount(_bitmap_from_bytes(256, 256, bm)) * 2
    v = bytearray(rng.integers(0, 256, npk, dtype=np.uint8).tobytes())
    v[0:4] = MARKER
    v[1001:1005] = MARKER
    v[32768 + 77:32768 + 81] = MARKER
    out.append(_frame("marker_in_stored_chunk", 256, 256, 16, bm, bytes(v)))
    for name, d, cnt in (("values_32768", 16, 16384), ("values_32769", 8, 32769)):
        bits = np.zeros(256 * 256, bool)
        bits[rng.choice(bits.size, cnt, replace=False)] = True
        bm = np.packbits(bits, bitorder="little").tobytes()
        npk = cnt * d // 8
        vals = _low_entropy(rng, npk)
        out.append(_frame(name + "_coded", 256, 256, d, bm, vals, dvm.fit_lengths(dvm.sample_hist(vals))))
        out.append(_frame(name + "_stored", 256, 256, d, bm, rng.integers(0, 256, npk, dtype=np.uint8).tobytes()))
    return out


def refused_catalogue(frames):
    """(name, frame with one stream replaced): streams the reader must refuse.  Sizes follow the streams."""
    by = {f["name"]: f for f in frames}
    out = []

    def variant(name, base, **kw):
        f = dict(by[base], **kw)
        f["name"] = name
        out.append(f)
    for lvl in (1, 6):
        variant("stock_zlib_%d_map" % lvl, "short_last_tile", map_stream=zlib.compress(by["short_last_tile"]["bitmap"], lvl))
        variant("stock_zlib_%d_values" % lvl, "values_coded_stored_coded", val_stream=zlib.compress(by["values_coded_stored_coded"]["values"], lvl))
    for base in ("short_last_tile", "stored_then_coded", "values_coded_stored_coded"):
        variant("truncated_map_" + base, base, map_stream=by[base]["map_stream"][:-1])
        variant("truncated_values_" + base, base, val_stream=by[base]["val_stream"][:-1])
    for bit in (0, 1, 2):
        for base in ("one_tile", "short_last_tile", "stored_then_coded"):
            s = bytearray(by[base]["map_stream"])
            s[2] ^= 1 << bit
            variant("flip_map_bit%d_%s" % (bit, base), base, map_stream=bytes(s))
        for base in ("values_coded_stored_coded", "marker_in_stored_chunk", "values_32768_coded"):
            s = bytearray(by[base]["val_stream"])
            s[2] ^= 1 << bit
            variant("flip_values_bit%d_%s" % (bit, base), base, val_stream=bytes(s))
    # a header bit of a unit in the middle of the chain
    f = by["values_coded_stored_coded"]
    _, _, _ = inflate(f["val_stream"], len(f["values"]), VALUES)
    second = decode_candidate(f["val_stream"], 2, VALUES)[0]
    s = bytearray(f["val_stream"])
    s[second] ^= 1
    variant("flip_values_second_unit", "values_coded_stored_coded", val_stream=bytes(s))
    return out
