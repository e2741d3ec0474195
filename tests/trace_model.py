"""The exact model of rc_trace_frames: a batch of STORED frames (op_mode 0: the binary map, then the packed values or a level-2 statistics
stream) and k int32 weight planes -> int64[n, 4 + k], summed in Python integers, and the no-wrap rule of pyrecode_amd/csrc/rc_trace.h
restated in Python integers.  The GPU tests (tests/test_gpu_traces.py) compare with it; tests/test_trace_cpu.py checks it against
hand-written literals and the C++ against the restatement."""
import numpy as np

from dense_model import unpack_fields

LIMIT = (1 << 63) - 1


def exact_sum(products):
    """the sum of an int64 array as a Python integer, whatever its size: the high and the low 32 bits of every element are summed apart -
    each of those sums fits an int64 for fewer than 2^31 elements -, and put together in Python integers (>> is arithmetic: x == (x >> 32)
    * 2^32 + (x & 0xFFFFFFFF) for negative x too).  The elements themselves are exact: a value below 2^16 times a weight of at most 2^31."""
    products = np.asarray(products, np.int64)
    assert products.size < 1 << 31
    return (int((products >> 32).sum(dtype=np.int64)) << 32) + int((products & 0xFFFFFFFF).sum(dtype=np.int64))


def trace_model(blob, sizes, ny, nx, d, level, planes=None):
    """out[f] = [set pixels, sum v, sum v * row, sum v * col, sum v * planes[m][row][col] ...] of frame f, v = the pixel's d-bit field at
    level 1 and 1 at levels 2 and 3.  Returns (out int64[n, 4 + k], set-pixel prefix uint64[n + 1]).  The products are int64 (exact: a value below 2^16 times an
    int32), their sums Python integers (exact_sum), which must fit an int64: the caller keeps to the no-wrap rule."""
    planes = np.zeros((0, ny, nx), np.int32) if planes is None else np.asarray(planes).reshape(-1, ny, nx)
    k, n, at = planes.shape[0], sizes.shape[0], 0
    flat = planes.reshape(k, ny * nx).astype(np.int64)
    out, prefix = np.zeros((n, 4 + k), np.int64), np.zeros(n + 1, np.uint64)
    for f in range(n):
        sz_map, sz_val = int(sizes[f, 0]), int(sizes[f, 1])
        mask = np.unpackbits(blob[at:at + sz_map], bitorder="little")[:ny * nx].astype(bool)
        idx = np.flatnonzero(mask)
        vals = unpack_fields(blob[at + sz_map:at + sz_map + sz_val], idx.size, d) if level == 1 else np.ones(idx.size, np.uint64)
        assert vals.size == 0 or int(vals.max()) < 1 << 16
        v = vals.astype(np.int64)
        row = [idx.size] + [exact_sum(v * w) for w in [np.ones(idx.size, np.int64), idx // nx, idx % nx] + [flat[m][idx] for m in range(k)]]
        assert all(-LIMIT - 1 <= x <= LIMIT for x in row), "the model's batch does not keep to the no-wrap rule"
        out[f] = row
        prefix[f + 1] = prefix[f] + np.uint64(idx.size)
        at += sz_map + sz_val
    return out, prefix


def weight_bounds(planes):
    """max |w| of every plane as Python integers: INT32_MIN counts as 2^31"""
    return [max(abs(int(p.min())), abs(int(p.max()))) if p.size else 0 for p in np.asarray(planes)]


def frame_pixels(nx, ny, level, d, packed_bytes):
    """the set pixels a frame can hold: all of them - at level 1 no more than its value stream has fields for"""
    return nx * ny if level != 1 else min(nx * ny, 8 * int(packed_bytes) // d)


def batch_fits(nx, ny, level, d, bounds, packed_bytes):
    """the no-wrap rule: a * vmax * P_f <= 2^63 - 1 for every column's largest weight a and every frame f of the batch"""
    vmax = (1 << d) - 1 if level == 1 else 1
    weights = [1, 1, ny - 1, nx - 1] + [int(b) for b in bounds]
    return all(a * vmax * frame_pixels(nx, ny, level, d, b) <= LIMIT for a in weights for b in packed_bytes)
