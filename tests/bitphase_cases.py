"""Case builders for the bit-phase tests (numpy only: no GPU, no import of the library or the oracle).

Residual streams are d-bit fields packed LSB first, value after value (recode_writer.py:637-652), and the device writes a frame's stream
tile by tile (4096 pixels a tile).  A tile whose last stream byte is only partly its own - the SHARED byte, holding the top `avail` bits of
its last value(s) - has that byte completed from the leading bits of the tiles behind it (rc_gather.hip, k_gather).  The builders here
produce data on which those bytes are never zero by accident, and a census that says, from the geometry alone, which way every shared
byte is completed:
  a  by two or more later tiles of the same item (d < 8: one-event tiles)
  b  by the first tile of the next item (k_gather's ext_cnt / ext_first)
  c  through the tile_next walk (the next item's first tile empty, or not enough bits in it)
  d  a tile whose bits all lie in an earlier tile's byte (n == 0 in resid_geom)
  e  by nothing: the frame ends on a partial byte
  f  a tile above the combined-slot capacity next to a one-event tile (residual_src alternates between the combined slot and pix_slots)
  g  inside the item, past one or more empty tiles (the nonempty ballot)
"""
import numpy as np

TILE = 4096                   # pixels a tile (rc_device.h: TILE_BM = 512 bitmap bytes)
COMB_RESID_BITS = 896 * 8     # a tile with more residual bits than this never fits the combined slot (1536 bytes, block image <= 640)

# the GPU test's tile-chain matrix (tests/test_gpu_bit_phases.py); the CPU census test walks the same one
CHAIN_DEPTHS = {"uint16": list(range(1, 8)) + list(range(9, 16)), "uint8": list(range(1, 8)), "uint32": [17, 19, 20, 23, 25, 28, 31]}
TPI_GEOMETRY = {8: (4, 8 * 9 + 3), 16: (16, 63 * 16 + 8), 32: (16, 63 * 32 + 16), 64: (16, 63 * 64 + 32)}   # tpi: (frames a batch, tiles a frame)
TPI64_DEPTHS = {"uint16": [3, 13], "uint8": [5], "uint32": [19]}


def gather_tpi(B, ntiles):
    """Tiles per k_gather item: restates launch_gather's rule (pyrecode_amd/csrc/rc_gather.hip, `uint32_t tpi = 64; while ...`)."""
    tpi = 64
    while tpi > 8 and B * (-(-ntiles // tpi)) < 1024:
        tpi >>= 1
    return tpi


def chain_matrix():
    """(dtype name, d, tpi) for every tile-chain case of the GPU test."""
    out = []
    for dt, ds in CHAIN_DEPTHS.items():
        for tpi in TPI_GEOMETRY:
            for d in ds:
                if tpi < 64 or d in TPI64_DEPTHS[dt]:
                    out.append((dt, d, tpi))
    return out


# ---- plain restatements of the packing (np.unpackbits based), independent of the oracle ------------------------------------------
def np_bit_pack(vals, d):
    """The low d bits of every value, LSB first, value after value; zero bits up to the next byte."""
    v = np.ascontiguousarray(vals, dtype=np.uint64).astype("<u8")
    bits = np.unpackbits(v.view(np.uint8).reshape(-1, 8), axis=1, bitorder="little")[:, :d]
    return np.packbits(bits.reshape(-1), bitorder="little")


def np_bit_unpack(packed, n, d):
    bits = np.unpackbits(np.asarray(packed, np.uint8), bitorder="little")[: n * d].reshape(n, d).astype(np.uint64)
    return (bits << np.arange(d, dtype=np.uint64)).sum(axis=1).astype(np.uint64) if n else np.zeros(0, np.uint64)


def np_threshold(dark, eps, dtype):
    """dark + eps in the source dtype: wraps mod 2^8 / 2^16 / 2^32 (recode_writer.py:127 under NumPy 2)."""
    m = int(np.iinfo(dtype).max) + 1
    return ((np.asarray(dark).astype(np.int64) + int(eps)) % m).astype(dtype)


# ---- full-range residuals -----------------------------------------------------------------------------------------------------------
def full_range_frames(seed, nz, ny, nx, sparsity, d, dtype=np.uint16, eps=0, overflow=False):
    """(dark, frames): residuals uniform over [1, 2^d - 1], an eighth of them exactly 2^d - 1 and an eighth 2^(d-1); dark levels over the
    dtype's whole range - most low enough for any residual, some anywhere, some where dark + eps wraps (eps > 0), some at the maximum.
    overflow: a third of the events instead take any value up to the dtype's maximum (bits at and above d are dropped by the packer)."""
    dtype = np.dtype(dtype)
    M = int(np.iinfo(dtype).max)
    top = (1 << d) - 1
    rng = np.random.default_rng(seed)
    kind = rng.random((ny, nx))
    low = rng.integers(0, max(M - top - eps, 0) + 1, (ny, nx), dtype=np.int64)
    dark = np.where(kind < 0.6, low, rng.integers(0, M + 1, (ny, nx), dtype=np.int64))
    if eps > 0:
        dark = np.where((kind >= 0.8) & (kind < 0.9), rng.integers(M - eps + 1, M + 1, (ny, nx), dtype=np.int64), dark)   # dark + eps wraps
    dark = np.where(kind >= 0.97, M, dark).astype(dtype)
    thr = np_threshold(dark, eps, dtype).astype(np.int64)
    frames = np.empty((nz, ny, nx), dtype)
    for z in range(nz):
        mask = (rng.random((ny, nx)) < sparsity) & (thr < M)
        r = rng.integers(1, top + 1, (ny, nx), dtype=np.int64)
        pick = rng.random((ny, nx))
        r = np.where(pick < 0.125, top, np.where(pick < 0.25, 1 << (d - 1), r))
        r = np.minimum(r, M - thr)                                     # (pixels whose threshold leaves less room)
        ev = thr + r
        if overflow:
            hi = thr + 1 + (rng.random((ny, nx)) * (M - thr)).astype(np.int64)
            ev = np.where(pick > 0.67, np.where(pick > 0.95, M, hi), ev)
        below = (rng.random((ny, nx)) * (thr + 1)).astype(np.int64)
        frames[z] = np.where(mask, ev, np.minimum(below, thr)).astype(dtype)
    return dark, frames


# ---- structured tile chains -----------------------------------------------------------------------------------------------------------
def _geom(coff, cnt, d):
    """resid_geom (rc_gather.hip): (b_lo, n, avail) with avail > 0 only where the tile owns a shared byte."""
    dbit, nbits = coff * d, cnt * d
    b_lo, b_hi = (dbit + 7) >> 3, (dbit + nbits + 7) >> 3
    n, avail = b_hi - b_lo, (dbit + nbits) & 7
    if avail and n:
        n -= 1
    else:
        avail = 0
    return b_lo, n, avail


def chain_counts(d, tpi, ntiles, rng):
    """Per-tile event counts of one frame, chosen left to right against the running bit offset so that every case of the census occurs."""
    counts = np.zeros(ntiles, np.int64)
    state = {"t": 0, "coff": 0}

    def put(c):
        t = state["t"]
        if t < ntiles:
            counts[t] = c
            state["coff"] += c
            state["t"] = t + 1

    def partial(lo):
        """a count >= lo whose tile ends on a shared byte, the smallest avail first (d < 8: leaves room for one-event successors)"""
        best = None
        for c in range(lo, lo + 8):
            _, _, avail = _geom(state["coff"], c, d)
            if avail and (best is None or avail < best[1]):
                best = (c, avail)
        put(best[0] if best else lo)

    big = min(TILE, COMB_RESID_BITS // d + 200 if d > 1 else 600)
    to_bits8 = -(-8 // d) + 1
    scripts = [
        # item 0: a tile above the combined slot, one-event tiles (a, d, f), a partial byte completed past an empty tile (g)
        [("p", big - 8), 1, 1, 1, ("p", 3), 0, 1, ("p", 2)],
        # item 1: (b) behind item 0; its last tile's byte leads into two entirely empty items (c)
        [to_bits8, 0, 1, ("p", big - 8), 1, 0, 2, ("p", 1)],
        [], [],
        # item 4: first tiles empty; its last tile's byte: a one-event ext tile, then the walk (b, then c)
        [0, 0, 0, 3, 1, 0, 1, ("p", 1)],
        # item 5: the next item's first tile empty, the walk ends inside it (c)
        [1, 0, 1, 2, 0, 0, 1, ("p", 1)],
        [0, 0, 4, 1, 1, 0, 0, ("p", 2)],
    ]
    nitems = -(-ntiles // tpi)
    for item in range(nitems):
        base = item * tpi
        state["t"] = base
        last = min(base + tpi, ntiles) - 1
        if item < len(scripts):
            sc = scripts[item]
        elif item == nitems - 1 or rng.random() < 0.15:
            sc = [int(x) for x in rng.choice([0, 0, 1, 1, 2, 5], min(tpi, 8) - 1)] + [("p", 1)]
        else:
            sc = []
        for k, s in enumerate(sc):
            if state["t"] > last:
                break
            if k == len(sc) - 1 and isinstance(s, tuple):
                while state["t"] < last:   # filler up to the item's last tile, which ends on a shared byte
                    put(int(rng.choice([0, 0, 0, 1, 3])) if tpi > 8 else 0)
            if isinstance(s, tuple):
                partial(s[1])
            else:
                put(s)
    # (e): the frame's last tile ends on a partial byte with nothing behind it
    state["coff"] = int(counts[:ntiles - 1].sum())
    state["t"] = ntiles - 1
    partial(2)
    return counts


def event_values(rng, n, d):
    """values in [2^(d-1), 2^d - 1]: the top bit set, so a shared byte's own bits are never all zero"""
    if d == 1:
        return np.ones(n, np.uint64)
    return ((1 << (d - 1)) | rng.integers(0, 1 << (d - 1), n, dtype=np.int64)).astype(np.uint64)


def tile_chain_frames(d, ntiles, dtype, B=1, tpi=None, seed=0, last_tile_pixels=3072):
    """B frames of ntiles tiles (nx = 1024, the last tile `last_tile_pixels` long) with chain_counts' structure.  Returns a dict:
    ny, nx, N, counts [B][ntiles], dark (uint of dtype, [N]; eps 0, so the threshold is the dark frame), idx (per frame, sorted
    pixel indices of the events), vals (per frame, the residuals, uint64).  Non-event pixels equal the threshold (strict > leaves them out)."""
    dtype = np.dtype(dtype)
    tpi = tpi or gather_tpi(B, ntiles)
    assert last_tile_pixels % 1024 == 0 and 0 < last_tile_pixels <= TILE
    nx = 1024
    N = (ntiles - 1) * TILE + last_tile_pixels
    rng = np.random.default_rng(seed * 1000 + d)
    dark = rng.integers(0, min(20, int(np.iinfo(dtype).max) - ((1 << d) - 1)) + 1, N).astype(dtype)   # (dark + value fits the dtype)
    counts, idx, vals = [], [], []
    for _ in range(B):
        c = chain_counts(d, tpi, ntiles, rng)
        pos = []
        for t in np.flatnonzero(c):
            lo, hi = t * TILE, min((t + 1) * TILE, N)
            k = int(min(c[t], hi - lo))
            c[t] = k
            ends = [lo, hi - 1] if k >= 2 else [lo if rng.random() < 0.5 else hi - 1]
            rest = rng.choice(np.arange(lo + 1, hi - 1), k - len(ends), replace=False) if k > len(ends) else np.zeros(0, np.int64)
            pos.append(np.concatenate([np.asarray(ends, np.int64), rest.astype(np.int64)]))
        p = np.sort(np.concatenate(pos)) if pos else np.zeros(0, np.int64)
        counts.append(c)
        idx.append(p)
        vals.append(event_values(rng, p.size, d))
    return {"ny": N // nx, "nx": nx, "N": N, "counts": np.stack(counts), "dark": dark, "idx": idx, "vals": vals, "dtype": dtype, "tpi": tpi, "d": d}


def chain_host_frames(cs):
    """The frames of a tile_chain_frames set as a host array [B][ny][nx] (small sets only)."""
    fr = np.tile(cs["dark"], (len(cs["idx"]), 1))
    for z, (p, v) in enumerate(zip(cs["idx"], cs["vals"])):
        fr[z, p] = (cs["dark"][p].astype(np.uint64) + v).astype(cs["dtype"])
    return fr.reshape(-1, cs["ny"], cs["nx"])


def chain_census(tile_counts, d, tpi):
    """Classify every tile's shared byte (and the n == 0 tiles) of one frame into the cases of the module docstring, from the geometry
    alone: counts x d, prefix offsets, 4096-pixel tiles, tpi.  Returns {case: [(tile, stream byte, avail)]} plus "empty_items": the most
    entirely empty items one (c) chain crossed."""
    cnt = np.asarray(tile_counts, np.int64)
    nt = cnt.size
    coff = np.concatenate([[0], np.cumsum(cnt)[:-1]])
    out = {k: [] for k in "abcdefg"}
    out["empty_items"] = 0
    for t in range(nt):
        if cnt[t] == 0:
            continue
        b_lo, n, avail = _geom(int(coff[t]), int(cnt[t]), d)
        if n == 0 and (b_lo * 8 - coff[t] * d) >= cnt[t] * d:
            out["d"].append((t, b_lo - 1, 0))
        if cnt[t] * d > COMB_RESID_BITS and ((t > 0 and cnt[t - 1] == 1) or (t + 1 < nt and cnt[t + 1] == 1)):
            out["f"].append((t, b_lo, 0))
        if not avail:
            continue
        fin_b = b_lo + n
        item, got, tiles = t // tpi, avail, []
        u = t + 1
        while got < 8 and u < nt:
            if cnt[u]:
                tiles.append(u)
                got += min(8 - got, int(cnt[u]) * d)
            u += 1
        rec = (t, fin_b, avail)
        if not tiles:
            out["e"].append(rec)
            continue
        inside = [u for u in tiles if u // tpi == item]
        outside = [u for u in tiles if u // tpi != item]
        if len(inside) >= 2:
            out["a"].append(rec)
        if inside and (inside[0] > t + 1 or any(b - a > 1 for a, b in zip(inside, inside[1:]))):
            out["g"].append(rec)
        ext = (item + 1) * tpi
        if outside and outside[0] == ext:
            out["b"].append(rec)
        if outside and (outside[0] != ext or len(outside) >= 2):
            out["c"].append(rec)
            first_item = outside[0] // tpi if outside[0] != ext else outside[-1] // tpi
            crossed = sum(1 for it in range(item + 1, first_item) if not cnt[it * tpi:(it + 1) * tpi].any())
            out["empty_items"] = max(out["empty_items"], crossed)
        if got < 8:
            out["e"].append(rec)
    return out


def census_cases_expected(d):
    """Which cases the census must find at depth d.  (a) needs a shared byte of avail bits that one d-bit value cannot complete:
    avail + d < 8 with avail a multiple of gcd(d, 8) - d in {1, 2, 3, 5}; (d) needs d <= 7; (f) a tile of more than COMB_RESID_BITS
    bits - d >= 2.  (b), (c), (e), (g) occur at every depth the matrix uses."""
    g = int(np.gcd(d, 8))
    want = set("bceg")
    if g + d < 8:
        want.add("a")
    if d < 8:
        want.add("d")
    if TILE * d > COMB_RESID_BITS:
        want.add("f")
    return want
