"""Test infrastructure: a Zstandard frame WRITER made from RFC 8878 alone (plain Python / numpy; nothing of the library under test is
imported, and nothing here is derived from its encoder).  It writes frames that stay inside the subset the batched reader's device
decoder documents (pyrecode_amd/csrc/rc_zstd_dec.h) but takes, at every point where that subset allows an alternative, ANY of the
alternatives - including ones no sensible encoder would pick - so that a decoder which misreads a form its own encoder never writes
is found out.  The same standing as lz4_parse_model.py and deflate_block_model.py.

    write_frame(plaintext, choices)      -> (frame bytes, census)
    write_near_miss(plaintext, feature)  -> legal zstd that leaves the subset by exactly the named feature (NEAR_MISS_FEATURES)
    write_repeat_offsets_without_table() -> a frame whose legality the stock decoder has to judge (see there)

choices: an int seed, a numpy Generator, or a dict {"seed": int, "cut": "any" | "tiles" | "literals_only", <point>: <alternative>}.
A dict entry for a decision point ("block", "lit", "tree", "seq_mode", "of_mode", "header", "fcs", "lit_sf", "nseq_bytes", "match",
"huf_assign", "ncount_style", ...) is honoured wherever that alternative is legal; everything else is drawn from the seeded source.
    cut "any"            blocks of any size and type (what rc_decompress takes)
    cut "tiles"          every block regenerates 512 bytes, the last one the rest (a stored binary map)
    cut "literals_only"  Raw, RLE and literals-only Compressed blocks (a stored value stream)
    "lits_size": n       literals-only blocks of n bytes;  "rle_size": "whole"  RLE blocks of the whole run

census: {"counts": {"<point>:<alternative>": n}, "blocks": [per block: type, regen, seq, tables, tree_skip, seq_skip], "regen": n}.

Limits honoured (the library's documented subset): one Huffman tree and one set of described sequence tables per frame; a block with
sequences regenerates 512 bytes unless it is the frame's last; Compressed blocks regenerate at most 1024 bytes (1023 with Huffman
literals); literal-length and match-length modes are equal; offsets are RLE code 0 with predefined tables, RLE code 0 or Repeat with
described ones, Repeat with repeated ones; every sequence has at least one literal and copies the byte in front of it."""
import bisect
from collections import Counter

import numpy as np

MAGIC = b"\x28\xb5\x2f\xfd"
TILE = 512
BLOCK_MAX = 1 << 17

# RFC 8878 3.1.1.3.2.1.1: code -> baseline, extra bits
LL_BASE = list(range(16)) + [16, 18, 20, 22, 24, 28, 32, 40, 48, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536]
LL_BITS = [0] * 16 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
ML_BASE = list(range(3, 35)) + [35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027, 2051, 4099, 8195, 16387, 32771, 65539]
ML_BITS = [0] * 32 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
# RFC 8878 3.1.1.3.2.2: default distributions, accuracy log 6
LL_DEFAULT = [4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1]
ML_DEFAULT = [1, 4, 3, 2, 2, 2, 2, 2, 2] + [1] * 37 + [-1] * 7
assert len(LL_BASE) == len(LL_BITS) == len(LL_DEFAULT) == 36 and len(ML_BASE) == len(ML_BITS) == len(ML_DEFAULT) == 53

NEAR_MISS_FEATURES = ("four_stream_literals", "real_offset", "literal_length_zero", "second_tree", "second_described_tables",
                      "rle_length_modes", "length_modes_differ", "checksum", "midframe_short_sequence_block",
                      "literals_block_above_1024", "two_frames")


class _Chooser:
    def __init__(self, choices):
        self.fixed = {}
        if isinstance(choices, dict):
            self.fixed = dict(choices)
            self.rng = np.random.default_rng(self.fixed.pop("seed", 0))
        elif isinstance(choices, np.random.Generator):
            self.rng = choices
        else:
            self.rng = np.random.default_rng(choices)
        self.cut = self.fixed.pop("cut", "any")
        self.counts = Counter()
        self.calls = Counter()

    def pick(self, point, options, weights=None, count=True):
        options = list(options)
        want = self.fixed.get(point)
        k = self.calls[point]
        self.calls[point] += 1
        if isinstance(want, (list, tuple)):
            want = want[k % len(want)]
        if want in options:
            c = want
        elif weights is None:
            c = options[int(self.rng.integers(len(options)))]
        else:
            w = np.asarray(weights, float)
            c = options[int(self.rng.choice(len(options), p=w / w.sum()))]
        if count:
            self.note(point, c)
        return c

    def note(self, point, alternative, n=1):
        self.counts["%s:%s" % (point, alternative)] += n

    def integer(self, lo, hi):
        return int(self.rng.integers(lo, hi + 1))

    def chance(self, p):
        return bool(self.rng.random() < p)


# ---- bit streams -----------------------------------------------------------------------------------------------------------------

class _FwdBits:
    """little-endian bit stream read from its first bit on (FSE table descriptions, RFC 8878 4.1.1)"""
    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, v, nb):
        assert 0 <= v < (1 << nb) or (nb == 0 and v == 0), (v, nb)
        self.acc |= v << self.n
        self.n += nb

    def bytes(self):
        return self.acc.to_bytes((self.n + 7) // 8, "little")


def _backward_stream(items):
    """items: (value, bits) in the order the decoder READS them.  The decoder starts below the highest set bit of the last byte and
    reads downwards (RFC 8878 4.1 / 4.2.2), so what it reads first lies highest."""
    acc, n = 0, 0
    for v, nb in reversed(items):
        assert 0 <= v < (1 << nb) or (nb == 0 and v == 0), (v, nb)
        acc |= v << n
        n += nb
    acc |= 1 << n                                   # the end mark
    return acc.to_bytes(n // 8 + 1, "little")


# ---- FSE (RFC 8878 4.1) ----------------------------------------------------------------------------------------------------------

def fse_decode_table(norm, log):
    """state -> (symbol, bits to read, baseline) of a normalised distribution (-1 = "less than one")"""
    size = 1 << log
    assert sum(abs(c) for c in norm) == size, (norm, log)
    sym = [None] * size
    high = size - 1
    for s, c in enumerate(norm):
        if c == -1:
            sym[high] = s
            high -= 1
    pos, step, mask = 0, (size >> 1) + (size >> 3) + 3, size - 1
    for s, c in enumerate(norm):
        for _ in range(max(c, 0)):
            sym[pos] = s
            pos = (pos + step) & mask
            while pos > high:
                pos = (pos + step) & mask
    assert pos == 0
    nxt = [1 if c == -1 else c for c in norm]
    table = []
    for u in range(size):
        s = sym[u]
        x = nxt[s]
        nxt[s] += 1
        nb = log - (x.bit_length() - 1)
        table.append((s, nb, (x << nb) - size))
    return table


RLE_TABLE = lambda code: [(code, 0, 0)]             # accuracy log 0: one state, no bits


def _fse_states(table, symbols, ch, last_needs_bits=False):
    """the decoder's state in front of every symbol.  The state of the LAST symbol is free (any state that carries the symbol): taken
    at random.  last_needs_bits: only states that read at least one bit (a stream that ends by running out of bits)."""
    by_sym = {}
    for u, (s, nb, base) in enumerate(table):
        by_sym.setdefault(s, []).append(u)
    cands = by_sym[symbols[-1]]
    if last_needs_bits:
        cands = [u for u in cands if table[u][1] > 0]
    states = [cands[ch.integer(0, len(cands) - 1)]]
    for s in reversed(symbols[:-1]):
        nxt = states[-1]
        for u in by_sym[s]:
            _, nb, base = table[u]
            if base <= nxt < base + (1 << nb):
                states.append(u)
                break
        else:
            raise AssertionError("no state of symbol %d leads to state %d" % (s, nxt))
    states.reverse()
    return states


def write_ncount(norm, log):
    """FSE table description (RFC 8878 4.1.1) of a normalised distribution whose last entry is not zero"""
    assert norm[-1] != 0 and 5 <= log
    b = _FwdBits()
    b.put(log - 5, 4)
    remaining, threshold, nbits = (1 << log) + 1, 1 << log, log + 1
    s, n = 0, len(norm)
    flags = {"lt1": 0, "zero_run": 0, "zero_run_long": 0}
    while remaining > 1:
        count = norm[s]
        s += 1
        c = count + 1
        mx = (2 * threshold - 1) - remaining
        if c < mx:
            b.put(c, nbits - 1)
        elif c < threshold:
            b.put(c, nbits)
        else:
            b.put(c + mx, nbits)
        remaining -= abs(count)
        flags["lt1"] += count == -1
        while remaining < threshold:
            nbits -= 1
            threshold >>= 1
        if count == 0:
            z = 0
            while norm[s] == 0:
                z += 1
                s += 1
            flags["zero_run"] += 1
            flags["zero_run_long"] += z >= 3
            while z >= 3:
                b.put(3, 2)
                z -= 3
            b.put(z, 2)
    assert remaining == 1 and s == n, (remaining, s, n)
    return b.bytes(), flags


def _random_norm(freq, max_sym, logs, ch, point):
    """a normalised distribution that covers the symbols of freq (symbol -> occurrences): any legal accuracy log, "less than one"
    counts and unused symbols drawn on purpose"""
    present = set(freq)
    for _ in range(ch.integer(0, 3)):                                    # symbols nobody uses
        present.add(ch.integer(0, max_sym))
    while len(present) < 2:
        present.add(ch.integer(0, max_sym))
    logs = [l for l in logs if (1 << l) >= len(present) + 1]
    log = ch.pick(point + "_log", logs)
    size = 1 << log
    present = sorted(present)
    style = ch.pick("ncount_style", ["fitted", "flat", "random"])
    lt1 = [s for s in present if ch.chance(0.5 if freq.get(s, 0) <= 1 else 0.1)]
    pos = [s for s in present if s not in lt1]
    if not pos:
        pos, lt1 = [lt1[0]], lt1[1:]
    mass = size - len(lt1) - len(pos)
    assert mass >= 0
    if style == "fitted":
        w = np.array([freq.get(s, 0) + 0.25 for s in pos], float)
    elif style == "flat":
        w = np.ones(len(pos))
    else:
        w = ch.rng.random(len(pos)) ** 3 + 1e-3
    extra = ch.rng.multinomial(mass, w / w.sum())
    norm = [0] * (present[-1] + 1)
    for s in lt1:
        norm[s] = -1
    for s, e in zip(pos, extra):
        norm[s] = 1 + int(e)
    if max(norm) == size:                                                # one symbol with all the mass is RLE mode's business
        raise AssertionError("degenerate distribution")
    return norm, log


# ---- Huffman (RFC 8878 4.2) ------------------------------------------------------------------------------------------------------

def _huf_lengths(freq, ch):
    """any complete prefix code over the symbols of freq with a maximum length drawn from 1..11 (not the optimal one)"""
    syms = sorted(freq)
    n = len(syms)
    assert n >= 2
    lo = max(1, (n - 1).bit_length())
    hi = min(11, n - 1)
    tl = ch.pick("huf_log", list(range(lo, hi + 1)), count=False)
    leaves = [1, 1]
    while max(leaves) < tl and len(leaves) < n:                          # a chain down to the wanted depth
        i = leaves.index(max(leaves))
        leaves[i:i + 1] = [leaves[i] + 1] * 2
    while len(leaves) < n:
        open_ = [i for i, l in enumerate(leaves) if l < tl]
        i = open_[ch.integer(0, len(open_) - 1)]
        leaves[i:i + 1] = [leaves[i] + 1] * 2
    assert max(leaves) == tl and sum(1 << (tl - l) for l in leaves) == 1 << tl
    leaves.sort()
    if ch.pick("huf_assign", ["by_frequency", "shuffled"]) == "by_frequency":
        order = sorted(syms, key=lambda s: -freq[s])
    else:
        order = [syms[i] for i in ch.rng.permutation(n)]
    return {s: l for s, l in zip(order, leaves)}, tl


def _huf_codes(lens, tl):
    """symbol -> (code, length): by increasing weight, then by symbol, codes counted up from zero (RFC 8878 4.2.1.3)"""
    pos, codes = 0, {}
    for w, s in sorted((tl + 1 - l, s) for s, l in lens.items()):
        codes[s] = (pos >> (w - 1), tl + 1 - w)
        pos += 1 << (w - 1)
    assert pos == 1 << tl
    return codes


def _huf_tree_description(lens, tl, ch):
    """weights of all symbols below the last present one; that one's weight is implied (RFC 8878 4.2.1.1)"""
    last = max(lens)
    weights = [tl + 1 - lens[s] if s in lens else 0 for s in range(last)]
    forms = []
    if last <= 128:
        forms.append("direct")
    fse = None
    if len(weights) >= 2:
        freq = Counter(weights)
        for _ in range(4):                                               # (a drawn distribution may code too long: draw again)
            try:
                norm, log = _random_norm(freq, 11, [5, 6], ch, "weights")   # weights 0..11 (Max_Number_of_Bits 11)
            except AssertionError:
                continue
            desc, _ = write_ncount(norm, log)
            table = fse_decode_table(norm, log)
            s1 = _fse_states(table, weights[0::2], ch, last_needs_bits=True)
            s2 = _fse_states(table, weights[1::2], ch, last_needs_bits=True)
            items = [(s1[0], log), (s2[0], log)]
            for i in range(len(weights)):
                st = (s1, s2)[i & 1]
                j = i >> 1
                if j + 1 < len(st):
                    _, nb, base = table[st[j]]
                    items.append((st[j + 1] - base, nb))
            body = desc + _backward_stream(items)
            if len(body) < 128:
                fse = bytes([len(body)]) + body
                forms.append("fse")
                break
    if not forms:
        return None, None
    form = ch.pick("tree", forms, count=False)
    if form == "fse":
        return fse, form
    nib = weights + [0] * (len(weights) & 1)
    return bytes([127 + len(weights)]) + bytes((nib[i] << 4) | nib[i + 1] for i in range(0, len(nib), 2)), form


def _huf_stream(lits, codes):
    return _backward_stream([codes[b] for b in lits])


# ---- sections and blocks -----------------------------------------------------------------------------------------------------------

def _code_of(v, base):
    return bisect.bisect_right(base, v) - 1


def _raw_rle_literals_header(lt, size, sf):
    if sf in (0, 2):                                 # the one-byte form: bit 2 clear, the size from bit 3 on - so "0" or "2" is the size's parity
        assert size < 32 and sf == 2 * (size & 1)
        return bytes([lt | (size << 3)])
    if sf == 1:
        assert size < 4096
        return (lt | (1 << 2) | (size << 4)).to_bytes(2, "little")
    return (lt | (3 << 2) | (size << 4)).to_bytes(3, "little")


def _raw_rle_literals(lits, rle, ch):
    n = len(lits)
    sf = ch.pick("lit_sf", ([2 * (n & 1)] if n < 32 else []) + ([1] if n < 4096 else []) + [3], count=False)
    ch.note("lit_sf", "%s:%d" % ("rle" if rle else "raw", sf))
    if rle:
        assert n and lits == lits[:1] * n
        return _raw_rle_literals_header(1, n, sf) + lits[:1]
    return _raw_rle_literals_header(0, n, sf) + lits


def _huf_literals_header(lt, streams4, regen, csize):
    assert regen < 1024 and csize < 1024
    return (lt | ((1 if streams4 else 0) << 2) | (regen << 4) | (csize << 14)).to_bytes(3, "little")


def _sequence_bits(seqs, ll_table, ll_log, ml_table, ml_log, ch, of_extra=None):
    """the sequences' bitstream: initial states (literal length, [offset], match length), then per sequence the extra bits (offset,
    match length, literal length) and - except behind the last - the state updates (literal length, match length, [offset])"""
    llc = [_code_of(l, LL_BASE) for l, _ in seqs]
    mlc = [_code_of(m, ML_BASE) for _, m in seqs]
    sl, sm = _fse_states(ll_table, llc, ch), _fse_states(ml_table, mlc, ch)
    items = [(sl[0], ll_log), (sm[0], ml_log)]
    for i, (l, m) in enumerate(seqs):
        if of_extra:
            items.append(of_extra)
        items.append((m - ML_BASE[mlc[i]], ML_BITS[mlc[i]]))
        items.append((l - LL_BASE[llc[i]], LL_BITS[llc[i]]))
        if i + 1 < len(seqs):
            _, nb, base = ll_table[sl[i]]
            items.append((sl[i + 1] - base, nb))
            _, nb, base = ml_table[sm[i]]
            items.append((sm[i + 1] - base, nb))
    return _backward_stream(items)


def _nseq_bytes(n, two):
    if two:
        assert n < 0x7F00
        return bytes([128 + (n >> 8), n & 255])
    assert n < 128
    return bytes([n])


def _block(last, btype, size, content):
    assert size <= BLOCK_MAX and len(content) <= BLOCK_MAX
    return ((1 if last else 0) | (btype << 1) | (size << 3)).to_bytes(3, "little") + content


def _frame_header(n, ch, need_window):
    """single-segment or windowed, content size in any field that can hold it.  need_window: the largest block (regenerated or stored
    size) - a single-segment frame's window is its content size."""
    forms = ["windowed"] + (["single"] if need_window <= n else [])
    form = ch.pick("header", forms)
    fields = [4, 8] + ([2] if 256 <= n < 65536 + 256 else [])
    if form == "single":
        if n < 256:
            fields.append(1)
    else:
        fields.append(0)
    fcs = ch.pick("fcs", fields)
    code = {0: 0, 1: 0, 2: 1, 4: 2, 8: 3}[fcs]
    out = bytes([(code << 6) | ((1 if form == "single" else 0) << 5)])
    if form == "windowed":
        exp = max(0, (max(need_window, 1) - 1).bit_length() - 10) + ch.integer(0, 2)
        out += bytes([(exp << 3) | ch.integer(0, 7)])
    if fcs == 2:
        out += (n - 256).to_bytes(2, "little")
    elif fcs:
        out += n.to_bytes(fcs, "little")
    return MAGIC + out


def _run_lengths(data):
    """rl[p] = number of bytes equal to data[p] from p on"""
    a = np.frombuffer(data, np.uint8)
    n = a.size
    rl = np.ones(n, np.int64)
    if n > 1:
        change = np.flatnonzero(a[1:] != a[:-1]) + 1
        ends = np.concatenate([change, [n]])
        starts = np.concatenate([[0], change])
        for s, e in zip(starts, ends):
            rl[s:e] = np.arange(e - s, 0, -1)
    return rl


def _has_match(rl, lo, hi):
    """a literal and a match of three behind it fit into [lo, hi)"""
    return hi - lo >= 4 and bool((np.minimum(rl[lo:hi], hi - np.arange(lo, hi)) >= 4).any())


def _parse(block, ch):
    """any cover of the block by literal runs and matches of the byte in front, at least one literal in front of every match: matches
    of the whole run, of three bytes only, of any part of it (the rest becomes literals or further matches), runs left as literals"""
    rl = _run_lengths(block)
    n = len(block)
    p_match = ch.pick("match_rate", [0.25, 0.6, 1.0], count=False)
    seqs, lits, p, run = [], bytearray(), 0, 0
    while p < n:
        if run >= 1 and block[p] == block[p - 1] and rl[p] >= 3:
            if ch.chance(p_match):
                style = ch.pick("match", ["whole", "three", "part"])
                m = int(rl[p]) if style == "whole" else 3 if style == "three" else ch.integer(3, int(rl[p]))
                seqs.append((run, m))
                p += m
                run = 0
                continue
            ch.note("match", "left_as_literals")
        lits.append(block[p])
        p += 1
        run += 1
    return seqs, bytes(lits)


def _greedy_parse(block):
    rl = _run_lengths(block)
    seqs, lits, p, run = [], bytearray(), 0, 0
    while p < len(block):
        if run >= 1 and block[p] == block[p - 1] and rl[p] >= 3:
            seqs.append((run, int(rl[p])))
            p += int(rl[p])
            run = 0
            continue
        lits.append(block[p])
        p += 1
        run += 1
    return seqs, bytes(lits)


def _cut(data, ch):
    """blocks (kind, start, size): kind raw | rle | lits (literals-only Compressed) | seq (Compressed with sequences)"""
    n = len(data)
    rl = _run_lengths(data) if n else None
    blocks, pos = [], 0
    while pos < n:
        rem = n - pos
        run = int(rl[pos])
        if ch.cut == "tiles":
            size = min(TILE, rem)
            opts = ["raw", "lits"] + (["rle"] if run >= size else []) + (["seq"] * 3 if _has_match(rl, pos, pos + size) else [])
            kind = ch.pick("block", opts, count=False)
        else:
            seq_size = min(TILE, rem)
            opts, w = ["raw", "lits", "rle"], [1.0, 2.0, 0.3 if run < 16 else 3.0]
            if ch.cut != "literals_only" and _has_match(rl, pos, pos + seq_size):
                opts.append("seq")
                w.append(4.0)
            kind = ch.pick("block", opts, w, count=False)
            if kind == "seq":
                size = seq_size
            elif kind == "rle":
                size = min(run, BLOCK_MAX) if ch.pick("rle_size", ["whole", "part"], count=False) == "whole" else ch.integer(1, min(run, BLOCK_MAX))
            elif kind == "lits":
                size = ch.integer(1, min(rem, 1024)) if ch.chance(0.7) else min(rem, 1024)
                if isinstance(ch.fixed.get("lits_size"), int):
                    size = min(rem, ch.fixed["lits_size"])
            else:
                how = ch.pick("raw_size", ["small", "medium", "maximum"], [6, 2, 1], count=False)
                size = min(rem, {"small": ch.integer(1, 700), "medium": ch.integer(700, 9000), "maximum": BLOCK_MAX}[how])
        blocks.append([kind, pos, size])
        pos += size
    # an empty Raw block may close a frame (legal zstd); not behind a short block with sequences, which has to be the last
    if not blocks or (ch.cut == "any" and ch.chance(0.06) and not (blocks[-1][0] == "seq" and blocks[-1][2] < TILE)):
        blocks.append(["raw", n, 0])
        ch.note("block", "empty_last")
    return blocks


def _assemble(data, ch, plan):
    """plan: list of dicts (kind, start, size, and for Compressed blocks seqs / lits / lit / seq_mode / of_mode) -> frame bytes, census"""
    n = len(data)
    # ---- literals: one tree over every Huffman-coded block of the frame
    huf = [b for b in plan if b.get("lit") == "huf"]
    tree = None
    while huf:
        freq = Counter()
        for b in huf:
            freq.update(b["lits"])
        while len(freq) < 2:
            freq[ch.integer(0, 255)] += 0
        lens, tl = _huf_lengths(freq, ch)
        codes = _huf_codes(lens, tl)
        desc, form = _huf_tree_description(lens, tl, ch)
        if desc is None:
            for b in huf:
                b["lit"] = "raw"
            break
        keep = []
        for b in huf:
            b["stream"] = _huf_stream(b["lits"], codes)
            if len(b["stream"]) + (0 if keep else len(desc)) < 1024:
                keep.append(b)
            else:
                b["lit"] = "raw"                                         # (does not fit the 10-bit size field)
        if keep and len(keep) == len(huf):
            tree = (desc, form, tl, lens)
            break
        if keep and keep[0] is huf[0]:
            tree = (desc, form, tl, lens)
            huf = keep
            break
        huf = keep                                                       # the block that was to carry the tree dropped out: once more
    if tree:
        desc, form, tl, lens = tree
        ch.note("tree", form)
        ch.note("huf_log", tl)
        if any(s not in lens for s in range(max(lens))):
            ch.note("tree", "alphabet_with_gaps")
        first = plan.index(huf[0])
        for b in huf[1:]:
            ch.note("treeless_distance", min(plan.index(b) - first, 4))
    # ---- sequences: table modes, then the frame's described tables over every block that uses them
    last, described, prev_of = None, False, None
    for b in plan:
        if b["kind"] != "seq":
            continue
        opts = ["predefined"] + ([] if described else ["described"]) + (["repeat"] if last is not None else [])
        mode = ch.pick("seq_mode", opts, count=False)
        if mode == "described":
            b["of_mode"] = ch.pick("of_mode", ["rle"] + (["repeat"] if last is not None else []), count=False)
            b["tables"], described = 1, True
        elif mode == "predefined":
            b["of_mode"], b["tables"] = "rle", 0
        else:
            b["of_mode"], b["tables"] = "repeat", last
            ch.note("repeat_of", "described" if last else "predefined")
        b["seq_mode"] = mode
        ch.note("seq_mode", mode)
        ch.note("of_mode", b["of_mode"] + ("_with_described" if mode == "described" else ""))
        if last is not None and prev_of != b["of_mode"]:
            ch.note("of_mode", b["of_mode"] + "_after_" + prev_of)
        prev_of = b["of_mode"]
        last = b["tables"]
    ll_pre, ml_pre = fse_decode_table(LL_DEFAULT, 6), fse_decode_table(ML_DEFAULT, 6)
    ll_own = ml_own = None
    if described:
        fl, fm = Counter(), Counter()
        for b in plan:
            if b["kind"] == "seq" and b["tables"] == 1:
                fl.update(_code_of(l, LL_BASE) for l, _ in b["seqs"])
                fm.update(_code_of(m, ML_BASE) for _, m in b["seqs"])
        ll_norm, ll_log = _random_norm(fl, 35, [5, 6, 7, 8, 9], ch, "ll")
        ml_norm, ml_log = _random_norm(fm, 52, [5, 6, 7, 8, 9], ch, "ml")
        ll_desc, f1 = write_ncount(ll_norm, ll_log)
        ml_desc, f2 = write_ncount(ml_norm, ml_log)
        for k in f1:
            if f1[k] + f2[k]:
                ch.note("ncount", k, f1[k] + f2[k])
        if len(ll_norm) < 36 or len(ml_norm) < 53:
            ch.note("ncount", "fewer_symbols_than_maximum")
        ll_own, ml_own = (fse_decode_table(ll_norm, ll_log), ll_log), (fse_decode_table(ml_norm, ml_log), ml_log)
    # ---- blocks
    body, rows, need_window = [], [], 1
    for i, b in enumerate(plan):
        kind, start, size = b["kind"], b["start"], b["size"]
        piece = data[start:start + size]
        is_last = i + 1 == len(plan)
        row = {"type": 2, "regen": size, "seq": kind == "seq", "tables": 0, "tree_skip": 0, "seq_skip": 0}
        if kind == "raw":
            body.append(_block(is_last, 0, size, piece))
            row["type"] = 0
            ch.note("block", "raw_maximum" if size == BLOCK_MAX else "raw")
        elif kind == "rle":
            body.append(_block(is_last, 1, size, piece[:1]))
            row["type"] = 1
            ch.note("block", "rle" if size <= 1024 else "rle_above_1024")
            if size == BLOCK_MAX:
                ch.note("block", "rle_maximum")
        else:
            lits = b["lits"]
            if b["lit"] == "huf":
                with_tree = b is huf[0]
                payload = (tree[0] if with_tree else b"") + b["stream"]
                sec = _huf_literals_header(2 if with_tree else 3, False, len(lits), len(payload)) + payload
                row["tree_skip"] = len(tree[0]) if with_tree else 0
                ch.note("lit", "huffman_with_tree" if with_tree else "huffman_treeless")
                if kind == "lits" and len(lits) > TILE:
                    ch.note("lit", "huffman_literals_only_above_512")
                if kind == "lits" and len(lits) == 1023:
                    ch.note("lit", "huffman_literals_only_1023")
            else:
                sec = _raw_rle_literals(lits, b["lit"] == "rle", ch)
                ch.note("lit", b["lit"])
            seqs = b["seqs"]
            if seqs:
                two = ch.pick("nseq_bytes", [2] + ([1] if len(seqs) < 128 else [])) == 2
                sec += _nseq_bytes(len(seqs), two)
                llm = {"predefined": 0, "described": 2, "repeat": 3}[b["seq_mode"]]
                ofm = 1 if b["of_mode"] == "rle" else 3
                sec += bytes([(llm << 6) | (ofm << 4) | (llm << 2)])
                skip = b""
                if llm == 2:
                    skip = ll_desc + (b"\x00" if ofm == 1 else b"") + ml_desc
                elif llm == 0:
                    skip = b"\x00"
                (lt_, ll_), (mt_, ml_) = (ll_own, ml_own) if b["tables"] else ((ll_pre, 6), (ml_pre, 6))
                sec += skip + _sequence_bits(seqs, lt_, ll_, mt_, ml_, ch)
                row["tables"], row["seq_skip"] = b["tables"], len(skip)
                if seqs[0][0] >= 16 or seqs[0][1] >= 35:
                    ch.note("codes", "extra_bits_in_first_sequence")
                if seqs[-1][0] >= 16 or seqs[-1][1] >= 35:
                    ch.note("codes", "extra_bits_in_last_sequence")
                if any(l >= 16 for l, _ in seqs):
                    ch.note("codes", "literal_length_with_extra_bits")
                if any(m >= 35 for _, m in seqs):
                    ch.note("codes", "match_length_with_extra_bits")
                if len(seqs) >= 128:
                    ch.note("nseq", "128_or_more")
                if size < TILE:
                    ch.note("block", "short_last_with_sequences")
                ch.note("block", "sequences")
            else:
                sec += b"\x00"
                ch.note("block", "literals_only")
            body.append(_block(is_last, 2, len(sec), sec))
            need_window = max(need_window, len(sec))
        need_window = max(need_window, size)
        rows.append(row)
    frame = _frame_header(n, ch, need_window) + b"".join(body)
    return frame, {"counts": dict(ch.counts), "blocks": rows, "regen": n}


def write_frame(plaintext, choices=0):
    data = bytes(plaintext)
    ch = choices if isinstance(choices, _Chooser) else _Chooser(choices)
    plan = []
    for kind, start, size in _cut(data, ch):
        b = {"kind": kind, "start": start, "size": size, "seqs": [], "lits": b""}
        piece = data[start:start + size]
        if kind == "seq":
            for _ in range(50):
                b["seqs"], b["lits"] = _parse(piece, ch)
                if b["seqs"]:
                    break
            else:
                b["seqs"], b["lits"] = _greedy_parse(piece)
            assert b["seqs"]
        elif kind == "lits":
            b["lits"] = piece
        if kind in ("seq", "lits"):
            lits = b["lits"]
            opts, w = ["raw"], [1.0]
            if lits and lits == lits[:1] * len(lits):
                opts.append("rle")
                w.append(2.0)
            if 1 <= len(lits) < 1024:
                opts.append("huf")
                w.append(3.0)
            b["lit"] = ch.pick("lit", opts, w, count=False)
        plan.append(b)
    return _assemble(data, ch, plan)


# ---- frames just outside the subset ------------------------------------------------------------------------------------------------

def _xxh64(data, seed=0):
    """XXH64 (the frame checksum of RFC 8878 3.1.1 is its low 32 bits)"""
    M = (1 << 64) - 1
    P1, P2, P3, P4, P5 = 11400714785074694791, 14029467366897019727, 1609587929392839161, 9650029242287828579, 2870177450012600261
    rotl = lambda x, r: ((x << r) | (x >> (64 - r))) & M
    rnd = lambda acc, v: (rotl((acc + v * P2) & M, 31) * P1) & M
    merge = lambda h, v: ((h ^ rnd(0, v)) * P1 + P4) & M
    n, p = len(data), 0
    if n >= 32:
        v = [(seed + P1 + P2) & M, (seed + P2) & M, seed & M, (seed - P1) & M]
        while p + 32 <= n:
            for k in range(4):
                v[k] = rnd(v[k], int.from_bytes(data[p + 8 * k:p + 8 * k + 8], "little"))
            p += 32
        h = (rotl(v[0], 1) + rotl(v[1], 7) + rotl(v[2], 12) + rotl(v[3], 18)) & M
        for k in range(4):
            h = merge(h, v[k])
    else:
        h = (seed + P5) & M
    h = (h + n) & M
    while p + 8 <= n:
        h = (rotl(h ^ rnd(0, int.from_bytes(data[p:p + 8], "little")), 27) * P1 + P4) & M
        p += 8
    if p + 4 <= n:
        h = (rotl(h ^ (int.from_bytes(data[p:p + 4], "little") * P1) & M, 23) * P2 + P3) & M
        p += 4
    while p < n:
        h = (rotl(h ^ (data[p] * P5) & M, 11) * P1) & M
        p += 1
    h ^= h >> 33
    h = (h * P2) & M
    h ^= h >> 29
    h = (h * P3) & M
    h ^= h >> 32
    return h


def _plain_header(n, checksum=False):
    """single-segment, 8-byte content size"""
    return MAGIC + bytes([(3 << 6) | (1 << 5) | (4 if checksum else 0)]) + n.to_bytes(8, "little")


def _plain_seq_block(piece, last, ch, modes=(0, 1, 0), tables=b"\x00", ll=None, ml=None, seqs_lits=None, of_extra=None):
    """raw literals, greedy parse; by default predefined tables and RLE offset code 0"""
    seqs, lits = seqs_lits if seqs_lits else _greedy_parse(piece)
    assert seqs
    pre = (fse_decode_table(LL_DEFAULT, 6), 6), (fse_decode_table(ML_DEFAULT, 6), 6)
    (lt_, ll_), (mt_, ml_) = ll or pre[0], ml or pre[1]
    sec = _raw_rle_literals_header(0, len(lits), 3) + lits + _nseq_bytes(len(seqs), len(seqs) >= 128)
    sec += bytes([(modes[0] << 6) | (modes[1] << 4) | (modes[2] << 2)]) + tables
    sec += _sequence_bits(seqs, lt_, ll_, mt_, ml_, ch, of_extra)
    return _block(last, 2, len(sec), sec)


def _plain_blocks(data, start, ch):
    """the rest of a frame in the plainest in-subset form: 512-byte blocks, with sequences where a match exists, else Raw"""
    out, n = [], len(data)
    if start >= n:
        return [_block(True, 0, 0, b"")]
    for p in range(start, n, TILE):
        piece = data[p:p + TILE]
        last = p + TILE >= n
        if _greedy_parse(piece)[0]:
            out.append(_plain_seq_block(piece, last, ch))
        else:
            out.append(_block(last, 0, len(piece), piece))
    return out


def _described(seqs, ch):
    fl = Counter(_code_of(l, LL_BASE) for l, _ in seqs)
    fm = Counter(_code_of(m, ML_BASE) for _, m in seqs)
    (ln, ll_log), (mn, ml_log) = _random_norm(fl, 35, [6], ch, "ll"), _random_norm(fm, 52, [6], ch, "ml")
    return (write_ncount(ln, ll_log)[0], (fse_decode_table(ln, ll_log), ll_log)), (write_ncount(mn, ml_log)[0], (fse_decode_table(mn, ml_log), ml_log))


def _huf_block(piece, last, ch, streams4=False):
    """literals-only Compressed block, Huffman literals with their own tree"""
    freq = Counter(piece)
    while len(freq) < 2:
        freq[(piece[0] + 1 + len(freq)) & 255] += 0
    lens, tl = _huf_lengths(freq, ch)
    codes = _huf_codes(lens, tl)
    desc, _ = _huf_tree_description(lens, tl, ch)
    if desc is None:
        raise ValueError("no tree description for this alphabet")
    if streams4:
        seg = (len(piece) + 3) // 4
        parts = [_huf_stream(piece[k * seg:(k + 1) * seg], codes) for k in range(3)] + [_huf_stream(piece[3 * seg:], codes)]
        payload = desc + b"".join(len(s).to_bytes(2, "little") for s in parts[:3]) + b"".join(parts)
    else:
        payload = desc + _huf_stream(piece, codes)
    if len(payload) >= 1024:
        raise ValueError("literals do not fit the 10-bit size field")
    sec = _huf_literals_header(2, streams4, len(piece), len(payload)) + payload + b"\x00"
    return _block(last, 2, len(sec), sec)


def write_near_miss(plaintext, feature, seed=0):
    """A LEGAL zstd frame of the plaintext, in the plainest in-subset form except for the one named feature.  ValueError when the
    plaintext cannot carry the feature (no run to match, too short)."""
    data = bytes(plaintext)
    n = len(data)
    ch = _Chooser({"seed": seed, "huf_assign": "by_frequency"})
    if feature == "two_frames":
        h = n // 2
        return b"".join(_plain_header(len(d)) + b"".join(_plain_blocks(d, 0, ch)) for d in (data[:h], data[h:]))
    if feature == "checksum":
        return _plain_header(n, True) + b"".join(_plain_blocks(data, 0, ch)) + (_xxh64(data) & 0xFFFFFFFF).to_bytes(4, "little")
    first = data[:TILE]
    more = n > TILE
    seqs, lits = _greedy_parse(first)
    need_seqs = feature not in ("four_stream_literals", "second_tree", "literals_block_above_1024")
    if need_seqs and not seqs:
        raise ValueError("the first 512 bytes hold no run to match")
    if feature == "four_stream_literals":
        if n < 64:
            raise ValueError("too short")
        k = min(n, 600)
        blocks = [_huf_block(data[:k], k == n, ch, streams4=True)] + (_plain_blocks(data, k, ch) if k < n else [])
    elif feature == "second_tree":
        if n < 8:
            raise ValueError("too short")
        k = min(n // 2, 600)
        e = min(n, 2 * k)
        blocks = [_huf_block(data[:k], False, ch), _huf_block(data[k:e], e == n, ch)] + (_plain_blocks(data, e, ch) if e < n else [])
    elif feature == "literals_block_above_1024":
        if n <= 1024:
            raise ValueError("too short")
        k = min(n, 1500)
        sec = _raw_rle_literals_header(0, k, 3) + data[:k] + b"\x00"
        blocks = [_block(k == n, 2, len(sec), sec)] + (_plain_blocks(data, k, ch) if k < n else [])
    elif feature == "real_offset":
        # offset code 2 with extra bits 00: Offset_Value 4, an explicit offset of 1 - the same bytes, said another way
        blocks = [_plain_seq_block(first, not more, ch, tables=b"\x02", of_extra=(0, 2))] + (_plain_blocks(data, TILE, ch) if more else [])
    elif feature == "rle_length_modes":
        l, m = seqs[0]
        rest = first[l + m:]
        one = ([(l, m)], first[:l] + rest)
        lc, mc = _code_of(l, LL_BASE), _code_of(m, ML_BASE)
        blocks = [_plain_seq_block(first, not more, ch, modes=(1, 1, 1), tables=bytes([lc, 0, mc]), ll=(RLE_TABLE(lc), 0), ml=(RLE_TABLE(mc), 0),
                                   seqs_lits=one)] + (_plain_blocks(data, TILE, ch) if more else [])
    elif feature == "length_modes_differ":
        _, (md, mt) = _described(seqs, ch)
        blocks = [_plain_seq_block(first, not more, ch, modes=(0, 1, 2), tables=b"\x00" + md, ml=mt)] + (_plain_blocks(data, TILE, ch) if more else [])
    elif feature == "second_described_tables":
        second = data[TILE:2 * TILE]
        if not _greedy_parse(second)[0]:
            raise ValueError("the second 512 bytes hold no run to match")
        blocks = []
        for k, piece in enumerate((first, second)):
            (ld, lt), (md, mt) = _described(_greedy_parse(piece)[0], ch)
            blocks.append(_plain_seq_block(piece, n <= 2 * TILE and k == 1, ch, modes=(2, 1, 2), tables=ld + b"\x00" + md, ll=lt, ml=mt))
        if n > 2 * TILE:
            blocks += _plain_blocks(data, 2 * TILE, ch)
    elif feature == "midframe_short_sequence_block":
        if n <= 300 or not _greedy_parse(data[:300])[0]:
            raise ValueError("needs more than 300 bytes with a run in the first 300")
        blocks = [_plain_seq_block(data[:300], False, ch)] + _plain_blocks(data, 300, ch)
    elif feature == "literal_length_zero":
        # a match of three, then a sequence with NO literal and offset code 0: the second repeat offset (4 at a frame's start), which
        # becomes the first - a later sequence with literals and offset code 0 then copies from four bytes back, not from one
        rl = _run_lengths(first)
        at = [i for i in range(len(first)) if rl[i] >= 7]
        if not at:
            raise ValueError("the first 512 bytes hold no run of seven")
        i = at[0]
        sq, lt, p = [(i + 1, 3), (0, 3)], bytearray(first[:i + 1]), i + 7
        for q in range(p + 1, len(first) - 2):
            if q >= 4 and first[q:q + 3] == first[q - 4:q - 1] and first[q:q + 3] != first[q - 1:q] * 3:
                m = 3
                while q + m < len(first) and first[q + m] == first[q + m - 4]:
                    m += 1
                sq.append((q - p, m))
                lt += first[p:q]
                p = q + m
                break
        lt += first[p:]
        blocks = [_plain_seq_block(first, not more, ch, seqs_lits=(sq, bytes(lt)))]
        if more:   # no sequences behind it: their offset code 0 would no longer mean "the byte in front"
            blocks += [_block(p + TILE >= n, 0, len(data[p:p + TILE]), data[p:p + TILE]) for p in range(TILE, n, TILE)]
    else:
        raise KeyError(feature)
    return _plain_header(n) + b"".join(blocks)


def write_repeat_offsets_without_table(plaintext, seed=0):
    """NOT known to be legal: described literal-length / match-length tables with the Repeat offsets mode in the FIRST block with
    sequences of a frame, where no offsets table exists to repeat.  The stock decoder is the judge (tests/test_zstd_frame_writer_cpu.py)."""
    data = bytes(plaintext)
    ch = _Chooser(seed)
    first = data[:TILE]
    seqs, _ = _greedy_parse(first)
    if not seqs:
        raise ValueError("the first 512 bytes hold no run to match")
    (ld, lt), (md, mt) = _described(seqs, ch)
    more = len(data) > TILE
    blocks = [_plain_seq_block(first, not more, ch, modes=(2, 3, 2), tables=ld + md, ll=lt, ml=mt)]
    if more:
        blocks += [_block(p + TILE >= len(data), 0, len(data[p:p + TILE]), data[p:p + TILE]) for p in range(TILE, len(data), TILE)]
    return _plain_header(len(data)) + b"".join(blocks)


# ---- the seeded corpus both test modules use -------------------------------------------------------------------------------------

def corpus_plaintexts():
    """(name, bytes): packed sparse bitmaps from empty to half full, constant bytes, packed d-bit residuals (high entropy), small
    alphabets (short Huffman codes, direct weights), lengths around the 512-byte block and beyond"""
    rng = np.random.default_rng(20240)
    out = []
    for n in (1, 511, 512, 513, 3000, 6001):
        for dens in (0.0, 0.0005, 0.005, 0.03, 0.15, 0.5):
            out.append(("bitmap_%g_%d" % (dens, n), np.packbits(rng.random(n * 8) < dens, bitorder="little").tobytes()))
        out.append(("ones_%d" % n, b"\xff" * n))
        out.append(("byte7_%d" % n, b"\x07" * n))
        for d in (9, 12):
            vals = rng.integers(0, 1 << d, (n * 8) // d + 1)
            bits = ((vals[:, None] >> np.arange(d)) & 1).astype(np.uint8).ravel()
            out.append(("residuals_d%d_%d" % (d, n), np.packbits(bits, bitorder="little").tobytes()[:n]))
        for k in (2, 3, 7, 20, 60):
            runs = np.repeat(rng.integers(0, k, n, dtype=np.uint8), rng.integers(1, 6, n))[:n]
            out.append(("alphabet%d_%d" % (k, n), runs.tobytes()))
    out.append(("quads_2048", np.repeat(np.arange(512, dtype=np.uint8) % 251, 4).tobytes()))          # 128 sequences in every 512 bytes
    big = np.packbits(rng.random(140000 * 8) < 0.01, bitorder="little")
    big[20000:60000] = 0
    big[70000:75000] = 0xA5
    out.append(("big_140000", big.tobytes()))
    out.append(("const_140000", b"\x3c" * 140000))
    return out


CORPUS_FORCED = (   # on top of the seeded draws: alternatives that need a nudge to occur often enough
    {"tree": "direct", "lit": "huf"}, {"tree": "fse", "lit": "huf"}, {"seq_mode": ["predefined", "repeat", "described", "repeat"]},
    {"seq_mode": ["predefined", "described", "repeat"], "of_mode": "repeat"}, {"block": "seq", "match": "whole", "match_rate": 1.0, "nseq_bytes": 1},
    {"block": "lits", "lit": "huf"}, {"block": "raw", "raw_size": "maximum"}, {"block": ["rle", "seq", "raw", "lits"]}, {"header": "single", "fcs": 1},
    {"block": "seq", "lit": "rle"}, {"lit": "raw", "lit_sf": 1}, {"lit": "raw", "lit_sf": 3},
)


def corpus(seeds=2):
    """(name, plaintext, frame, census) - deterministic"""
    k = 0
    for name, data in corpus_plaintexts():
        big = len(data) > 100000
        variants = [{"seed": 1000 * s + k} for s in range(1 if big else seeds)]
        forced = CORPUS_FORCED[k % len(CORPUS_FORCED)]
        variants.append(dict(forced, seed=77 + k))
        if name.startswith("const_"):
            variants = [{"seed": 3, "block": "rle", "rle_size": "whole"}, {"seed": 4, "block": ["rle", "raw", "seq"], "rle_size": "whole"},
                        {"seed": 5, "block": ["rle", "lits", "rle"], "rle_size": "whole", "lit": "rle"}]
        elif big:
            variants += [{"seed": 7, "block": ["raw", "rle"], "rle_size": "whole"},{"seed": 5, "block": "raw", "raw_size": "maximum"}, {"seed": 6, "block": ["raw", "seq", "lits"], "raw_size": "maximum"}]
        if name in ("bitmap_0.03_3000", "alphabet7_3000", "alphabet20_6001", "bitmap_0.005_6001"):
            variants.append({"seed": 12 + k, "block": "lits", "lits_size": 1023, "lit": "huf", "huf_assign": "by_frequency"})
        if name in ("byte7_511", "byte7_513", "ones_3000", "bitmap_0_512"):           # RLE literals and short raw ones in every header form
            variants += [{"seed": 40 + k, "block": "lits", "lits_size": sz, "lit": lit} for sz in (6, 7, 30, 31) for lit in ("raw", "rle")]
        if name.startswith("quads"):
            variants += [{"seed": 8, "cut": "tiles", "block": "seq", "match": "whole", "match_rate": 1.0},
                         {"seed": 9, "block": "seq", "match": "whole", "match_rate": 1.0, "lit": "huf"}]
        for v in variants:
            frame, census = write_frame(data, dict(v))
            yield "%s/%s" % (name, ",".join("%s=%s" % kv for kv in sorted(v.items(), key=str))), data, frame, census
        k += 1


def near_miss_plaintext():
    """carries every feature of NEAR_MISS_FEATURES: runs in every 512 bytes, a run of seven followed by bytes that repeat at distance
    four but not at distance one (so that reading "literal length 0, offset code 0" as "the byte in front" gives OTHER bytes)"""
    rng = np.random.default_rng(4)
    return b"\x05" * 8 + b"aaaaaaaBaaaBxyz" + np.packbits(rng.random(3000 * 8) < 0.02, bitorder="little").tobytes()
