"""The exact model of electron counting (pyrecode_amd/csrc/rc_count.hip, rc_count.h) - CPU code, numpy and scipy.

count_frame is the specification the device is compared with by `==`: components from scipy.ndimage.label with the 3 x 3 structure (so
their order is scipy's), per-label sums in int64 (enough for every shape of the tests: 65 535^2 x 274 010 < 2^63), centroids as the exact
rational rounded half to even from divmod.  stored_batch builds what rc_count_frames takes with op_mode 0.  float32_frame restates the
reference's accumulation (utils/converters.py:167-197: float32 sums in raster order, a float32 division, np.round) for the cross-check
that ties the exact definition to it where its rounding cannot matter."""
import numpy as np
import scipy.ndimage as nd

EIGHT = np.ones((3, 3), int)
METHODS = ("weighted_average", "unweighted_average", "max")


def rhe(S, w):
    """S / w (integer arrays, w > 0) to the nearest integer, ties to the even one"""
    q, r = np.divmod(np.asarray(S, np.int64), np.asarray(w, np.int64))
    up = (2 * r > w) | ((2 * r == w) & (q % 2 == 1))
    return q + up


def count_frame(binary, value, method="weighted_average", area_threshold=0):
    """(rows int32, cols int32, area uint32, weight uint64) of one frame: binary bool[ny, nx] is the foreground, value the stored values
    (read at set pixels only; a stored 0 is allowed)"""
    assert method in METHODS
    binary = np.asarray(binary, bool)
    labels, n = nd.label(binary, structure=EIGHT)
    if n == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.uint32), np.zeros(0, np.uint64)
    r, c = np.nonzero(binary)                                   # raster order
    lab = labels[r, c] - 1
    v = np.asarray(value)[r, c].astype(np.int64)
    r, c = r.astype(np.int64), c.astype(np.int64)

    def total(x):
        out = np.zeros(n, np.int64)
        np.add.at(out, lab, x)
        return out
    area, weight = total(np.ones_like(v)), total(v)
    ur, uc = rhe(total(r), area), rhe(total(c), area)
    if method == "unweighted_average":
        row, col = ur, uc
    elif method == "weighted_average":
        safe = np.maximum(weight, 1)
        heavy = weight > 0
        row, col = np.where(heavy, rhe(total(v * r), safe), ur), np.where(heavy, rhe(total(v * c), safe), uc)
    else:
        # the largest v, the first in raster order among equals: a stable sort by (label, -v) keeps raster order inside a tie
        order = np.lexsort((-v, lab))
        first = order[np.searchsorted(lab[order], np.arange(n))]
        row, col = r[first], c[first]
    keep = area > area_threshold
    return row[keep].astype(np.int32), col[keep].astype(np.int32), area[keep].astype(np.uint32), weight[keep].astype(np.uint64)


def count_batch(frames, method="weighted_average", area_threshold=0):
    """frames = [(binary, value)]: (prefix uint64[n + 1], rows, cols, area, weight) as rc_count_frames returns them"""
    got = [count_frame(b, v, method, area_threshold) for b, v in frames]
    prefix = np.zeros(len(frames) + 1, np.uint64)
    prefix[1:] = np.cumsum([g[0].size for g in got])
    cat = lambda k, dt: np.concatenate([g[k] for g in got]).astype(dt) if got else np.zeros(0, dt)   # noqa: E731
    return prefix, cat(0, np.int32), cat(1, np.int32), cat(2, np.uint32), cat(3, np.uint64)


def pack_values(vals, d):
    """d-bit fields, LSB first, zero-padded to a byte"""
    vals = np.asarray(vals, np.uint32)
    assert d >= 1 and (vals.size == 0 or int(vals.max()) < 1 << d)
    bits = ((vals[:, None] >> np.arange(d, dtype=np.uint32)) & 1).astype(np.uint8).reshape(-1)
    return np.packbits(bits, bitorder="little")


def stored_batch(frames, level, d):
    """frames = [(binary, value)] as the stored pieces of a batch (op_mode 0): (bytes uint8, sizes uint32[n][3]).  Level 1: the packed map,
    then the set pixels' values in raster order as d-bit fields.  Level 3: the map.  Level 2: the map, then a statistics stream of one
    d-bit field per component - the counting steps over it."""
    parts, sizes = [], np.zeros((len(frames), 3), np.uint32)
    for i, (binary, value) in enumerate(frames):
        binary = np.asarray(binary, bool)
        parts.append(np.packbits(binary.ravel(), bitorder="little"))
        sizes[i, 0] = parts[-1].size
        if level == 1:
            parts.append(pack_values(np.asarray(value)[binary], d))
        elif level == 2:
            n = nd.label(binary, structure=EIGHT)[1]
            parts.append(pack_values(np.arange(n, dtype=np.uint32) % (1 << d), d))
        if level in (1, 2):
            sizes[i, 1] = sizes[i, 2] = parts[-1].size
    return np.ascontiguousarray(np.concatenate(parts)), sizes


def float32_frame(binary, value, area_threshold=0):
    """the weighted average as the reference's helper accumulates it: float32 sums of v * r, v * c, v (each add made in float64, stored
    as float32) in raster order per label, a float32 quotient, np.round.  Returns (rows, cols) int64 in label order.  Components of weight 0
    are outside this restatement (the reference divides by zero there)."""
    binary = np.asarray(binary, bool)
    labels, n = nd.label(binary, structure=EIGHT)
    acc = np.zeros((n, 4), np.float32)
    rr, cc = np.nonzero(binary)
    for r, c in zip(rr.tolist(), cc.tolist()):
        k = labels[r, c] - 1
        v = float(value[r, c])
        for j, term in enumerate((v * r, v * c, v, 1.0)):          # the add is made in float64 and stored as float32
            acc[k, j] = np.float32(float(acc[k, j]) + term)
    keep = acc[:, 3] > area_threshold
    acc = acc[keep]
    return np.round(acc[:, 0] / acc[:, 2]).astype(np.int64), np.round(acc[:, 1] / acc[:, 2]).astype(np.int64)


def bernoulli_frame(ny, nx, d, p, seed, zero_fraction=0.0):
    """(binary, value): pixels set with probability p, values uniform in 1 .. 2^d - 1, a fraction of the set ones forced to 0"""
    rng = np.random.default_rng([seed, ny, nx, d])
    binary = rng.random((ny, nx)) < p
    value = rng.integers(1, 1 << d, (ny, nx)).astype(np.uint16)
    if zero_fraction:
        value[rng.random((ny, nx)) < zero_fraction] = 0
    return binary, value
