"""Serial restatement (test infrastructure) of the device DEFLATE encoder's residual stream at compression_level >= 2
(pyrecode_amd/csrc/rc_deflate_model.h: the table, rc_pix_deflate.hip: the kernels).

The stream: `78 01`, one image per 32 KiB chunk of the packed residuals, Adler-32 of the packed residuals (big-endian).  A coded chunk is a
dynamic-Huffman block (RFC 1951, BTYPE 10) of literals and the end-of-block code only:
    [BFINAL, BTYPE 10][HLIT 0, HDIST 0, HCLEN 15][19 x 3 bits: the code-length code][the 258 lengths, run-length coded][literals][EOB]
followed, unless it is the stream's last, by an empty stored block (000, pad, 00 00 FF FF) so that the next image starts on a byte; the last
one carries BFINAL and is padded to the byte.  A chunk whose image would not be smaller than its stored form (n + 5 bytes) is a stored block,
so a stream in which no chunk pays IS deflate_block_model.stored_stream.

The table: one per ctx, 257 symbols (256 literals + EOB), lengths <= 12, fitted to a byte histogram of a sample; every symbol has a code.
The distance alphabet is one code of length zero (RFC 1951 3.2.7: literal-only data); the 258 lengths are written with symbol 16 (repeat the
previous length 3..6 times) as the only run symbol - no literal has length zero, so 17 / 18 never apply."""
import deflate_block_model as dbm

CHUNK = dbm.CHUNK
MAXBITS = 12        # a `code | len << 12` entry fits 16 bits
CL_MAXBITS = 7      # the code-length code's lengths travel in 3 bits
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)


def huf_lengths(hist, maxbits):
    """rc_zstd_model.h::zm_huf_lengths_n: code lengths 1..maxbits for EVERY symbol (counts smoothed x256 + 1), Kraft sum exactly one"""
    n = len(hist)
    w = [int(h) * 256 + 1 for h in hist]
    left, right = [-1] * n, [-1] * n
    live = list(range(n))
    while len(live) > 1:
        live.sort(key=lambda i: (w[i], i), reverse=True)
        a = live.pop()
        b = live.pop()
        w.append(w[a] + w[b]); left.append(a); right.append(b)
        live.append(len(w) - 1)
    depth = [0] * len(w)
    for i in range(len(w) - 1, n - 1, -1):
        depth[left[i]] = depth[i] + 1
        depth[right[i]] = depth[i] + 1
    ln = [min(max(depth[s], 1), maxbits) for s in range(n)]
    kraft = sum(1 << (maxbits - l) for l in ln)
    one = 1 << maxbits
    order = sorted(range(n), key=lambda s: (int(hist[s]), -s))          # rarest first
    while kraft > one:
        moved = False
        for s in order:
            if ln[s] < maxbits:
                kraft -= 1 << (maxbits - ln[s] - 1)
                ln[s] += 1
                moved = True
                if kraft <= one:
                    break
        if not moved:
            break
    while kraft < one:
        moved = False
        for s in reversed(order):
            gain = 1 << (maxbits - ln[s])
            if ln[s] > 1 and gain <= one - kraft:
                ln[s] -= 1
                kraft += gain
                moved = True
                break
        if not moved:
            break
    return ln


def sample_hist(sample):
    """the 257-entry histogram the ctx fits its table to: the sample's bytes and one end-of-block per 32 KiB of it"""
    hist = [0] * 257
    for b in bytes(sample):
        hist[b] += 1
    hist[256] = max(len(sample) >> 15, 1)
    return hist


def fit_lengths(hist):
    """257 code lengths (<= 12, none zero) from a histogram of 256 byte counts (+ optionally the end-of-block count)"""
    hist = [int(h) for h in hist]
    if len(hist) == 256:
        hist.append(max(sum(hist) >> 15, 1))
    assert len(hist) == 257
    return huf_lengths(hist, MAXBITS)


def usable(hist, lengths):
    """the ctx keeps the stored form when the code would not take 3 % off the sample (the rule of the modelled zstd encoder)"""
    total = sum(int(h) for h in hist[:256])
    bits = sum(int(h) * l for h, l in zip(hist[:256], lengths))
    return total != 0 and bits <= total * 8 * 97 // 100


def canonical_codes(lengths):
    """RFC 1951 3.2.2: code values, as they are read MSB-first"""
    maxl = max(lengths)
    count = [0] * (maxl + 2)
    for l in lengths:
        if l:
            count[l] += 1
    code, nxt = 0, [0] * (maxl + 2)
    for b in range(1, maxl + 1):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = []
    for l in lengths:
        if l:
            out.append(nxt[l]); nxt[l] += 1
        else:
            out.append(0)
    return out


def cl_symbols(lengths):
    """the 257 literal/length lengths and the single zero distance length as code-length symbols: [(symbol, extra bits, extra value)]"""
    seq = list(lengths) + [0]
    out, i = [], 0
    while i < len(seq):
        v = seq[i]
        out.append((v, 0, 0))
        i += 1
        run = 0
        while i + run < len(seq) and seq[i + run] == v:
            run += 1
        while run >= 3:
            r = min(run, 6)
            out.append((16, 2, r - 3))
            run -= r
            i += r
    return out


def header_bits(lengths):
    """(value, nbits): the block's bits in front of its first literal, LSB-first, with BFINAL clear"""
    assert len(lengths) == 257 and all(1 <= l <= MAXBITS for l in lengths)
    syms = cl_symbols(lengths)
    clhist = [0] * 19
    for s, _, _ in syms:
        clhist[s] += 1
    cl_len = huf_lengths(clhist, CL_MAXBITS)
    cl_code = canonical_codes(cl_len)
    w = dbm.BitWriter()
    w.put(0, 1); w.put(2, 2)
    w.put(0, 5); w.put(0, 5); w.put(15, 4)
    for s in CL_ORDER:
        w.put(cl_len[s], 3)
    for s, e, ev in syms:
        w.put_code(cl_code[s], cl_len[s])
        w.put(ev, e)
    nbits = w.bits()
    w.align()
    return int.from_bytes(bytes(w.out), "little"), nbits


def encode_chunk(block, last, lengths, codes, hdr, use):
    n = len(block)
    hv, hn = hdr
    bits = hn + sum(lengths[b] for b in block) + lengths[256]
    size = (bits + 7) // 8 if last else (bits + 3 + 7) // 8 + 4
    if not use or n == 0 or size >= n + 5:
        return dbm.stored(block, last)
    rev = [int(format(c, "0%db" % l)[::-1], 2) for c, l in zip(codes, lengths)]     # codes enter the stream MSB-first
    w = dbm.BitWriter()
    w.put(hv | (1 if last else 0), hn)
    for b in block:
        w.put(rev[b], lengths[b])
    w.put(rev[256], lengths[256])
    if not last:
        w.put(0, 3)
        w.align()
        w.out += b"\x00\x00\xff\xff"
    else:
        w.align()
    assert len(w.out) == size
    return bytes(w.out)


def encode_values(data, lengths, usable=True):
    """the zlib stream of the packed residuals under the ctx's table (lengths None or usable False: the stored stream)"""
    data = bytes(data)
    if lengths is None or not usable:
        return dbm.stored_stream(data)
    codes, hdr = canonical_codes(lengths), header_bits(lengths)
    nch = max((len(data) + CHUNK - 1) // CHUNK, 1)
    out = bytearray(b"\x78\x01")
    for k in range(nch):
        out += encode_chunk(data[k * CHUNK:(k + 1) * CHUNK], k + 1 == nch, lengths, codes, hdr, True)
    return bytes(out) + dbm.adler32(data).to_bytes(4, "big")


class _BitReader:
    def __init__(self, data, pos):
        self.d, self.p = data, 8 * pos

    def get(self, n):
        v = 0
        for i in range(n):
            v |= ((self.d[self.p >> 3] >> (self.p & 7)) & 1) << i
            self.p += 1
        return v


def _read_lengths(stream, pos):
    r = _BitReader(stream, pos)
    r.get(3)
    hlit, hdist, hclen = r.get(5) + 257, r.get(5) + 1, r.get(4) + 4
    assert (hlit, hdist) == (257, 1)
    cl_len = [0] * 19
    for s in CL_ORDER[:hclen]:
        cl_len[s] = r.get(3)
    cl_code = canonical_codes(cl_len)
    dec = {(cl_len[s], cl_code[s]): s for s in range(19) if cl_len[s]}
    out = []
    while len(out) < hlit + hdist:
        code, n = 0, 0
        while (n, code) not in dec:
            code = (code << 1) | r.get(1)
            n += 1
            assert n <= 7
        s = dec[(n, code)]
        if s < 16:
            out.append(s)
        elif s == 16:
            out += [out[-1]] * (3 + r.get(2))
        else:
            out += [0] * ((3 + r.get(3)) if s == 17 else (11 + r.get(7)))
    assert len(out) == 258 and out[257] == 0
    return out[:257]


def parse_table(stream):
    """the 257 lengths of the first coded block of a stream encode_values describes; None when every chunk is stored"""
    stream = bytes(stream)
    pos = 2
    while pos < len(stream) - 4:
        b = stream[pos]
        if ((b >> 1) & 3) == 2:
            return _read_lengths(stream, pos)
        assert (b & 6) == 0, "neither a stored nor a dynamic block at a chunk border"
        n = stream[pos + 1] | (stream[pos + 2] << 8)
        pos += 5 + n
        if b & 1:
            break
    return None
