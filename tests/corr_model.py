"""The exact model of rc_corr_frames: a batch of STORED frames (op_mode 0: the binary map, then the packed values or a level-2 statistics
stream), a reference image T and a radius R -> int64[n, S, S], S = 2 R + 1, from a zero-padded T and one gather per offset, summed in
Python integers; the index and workspace arithmetic of pyrecode_amd/csrc/rc_corr.h restated in Python integers; and estimate_shifts
restated: the tie-break as a sort key, the parabola as a Fraction.  The GPU tests (tests/test_gpu_corr.py) compare with it;
tests/test_corr_cpu.py checks it against hand-written literals and the C++ against the restatement."""
from fractions import Fraction

import numpy as np

from dense_model import unpack_fields
from trace_model import LIMIT, exact_sum, frame_pixels

TARGET_WGS = 4096      # rc_corr.h: CORR_TARGET_WGS


def corr_of_pixels(idx, vals, T, R):
    """int64[S, S] of one frame: idx its set pixels (row-major indices, ascending), vals their values, T int[ny, nx]"""
    ny, nx = T.shape
    S = 2 * R + 1
    pad = np.zeros((ny + 2 * R, nx + 2 * R), np.int64)
    pad[R:R + ny, R:R + nx] = T
    row, col, v = idx // nx, idx % nx, np.asarray(vals).astype(np.int64)
    out = np.zeros((S, S), np.int64)
    for iy in range(S):               # (iy = dy + R: T[row + dy] sits in padded row row + iy)
        for ix in range(S):
            cell = exact_sum(v * pad[row + iy, col + ix])
            assert -LIMIT - 1 <= cell <= LIMIT, "the model's batch does not keep to the no-wrap rule"
            out[iy, ix] = cell
    return out


def corr_model(blob, sizes, ny, nx, d, level, T, R):
    """out[f, dy + R, dx + R] = sum over frame f's set pixels (row, col) of v * T[row + dy, col + dx], T outside the image 0; v = the pixel's
    d-bit field at level 1 and 1 at levels 2 and 3.  Returns (out int64[n, S, S], set-pixel prefix uint64[n + 1])."""
    T = np.asarray(T).reshape(ny, nx)
    n, at, S = sizes.shape[0], 0, 2 * R + 1
    out, prefix = np.zeros((n, S, S), np.int64), np.zeros(n + 1, np.uint64)
    for f in range(n):
        sz_map, sz_val = int(sizes[f, 0]), int(sizes[f, 1])
        idx = np.flatnonzero(np.unpackbits(blob[at:at + sz_map], bitorder="little")[:ny * nx])
        vals = unpack_fields(blob[at + sz_map:at + sz_map + sz_val], idx.size, d) if level == 1 else np.ones(idx.size, np.uint64)
        assert vals.size == 0 or int(vals.max()) < 1 << 16
        out[f] = corr_of_pixels(idx, vals, T, R)
        prefix[f + 1] = prefix[f] + np.uint64(idx.size)
        at += sz_map + sz_val
    return out, prefix


def corr_of_frames(frames, T, R):
    """the same from dense frames int[n, ny, nx] (0 = not set)"""
    frames = np.asarray(frames)
    return np.stack([corr_of_pixels(np.flatnonzero(fr.reshape(-1)), fr.reshape(-1)[np.flatnonzero(fr.reshape(-1))], np.asarray(T), R) for fr in frames])


def reference_bound(T):
    """max |T| as a Python integer: INT32_MIN counts as 2^31"""
    T = np.asarray(T)
    return max(abs(int(T.min())), abs(int(T.max()))) if T.size else 0


def batch_fits(nx, ny, level, d, bound, packed_bytes):
    """the no-wrap rule: max|T| * vmax * P_f <= 2^63 - 1 for every frame f of the batch"""
    vmax = (1 << d) - 1 if level == 1 else 1
    return all(int(bound) * vmax * frame_pixels(nx, ny, level, d, b) <= LIMIT for b in packed_bytes)


# ---- rc_corr.h's host arithmetic --------------------------------------------------------------------------------------------------------
def side(R):
    return 2 * R + 1


def lane_cells(R):
    return -(-side(R) ** 2 // 64)


def padded_cells(nx, ny, R):
    return (nx + 2 * R) * (ny + 2 * R)


def window_base(row, col, nx, R):
    return row * (nx + 2 * R) + col


def cell_offset(cell, nx, R):
    return (cell // side(R)) * (nx + 2 * R) + cell % side(R)


def chunks(nblk, n):
    """(blocks a workgroup walks, workgroups per frame)"""
    want = max(1, min(nblk, -(-TARGET_WGS // n)))
    bpc = -(-nblk // want) if nblk else 1
    return bpc, (-(-nblk // bpc) if nblk else 1)


def workspace_bytes(nb8, n, R, wg=256):
    return n * chunks(-(-nb8 // wg), n)[1] * side(R) ** 2 * 8


# ---- estimate_shifts, restated ----------------------------------------------------------------------------------------------------------
def shifts_model(corr, group=1):
    """per frame (dy, dx, peak, on_border, valid, refined_y, refined_x) - refined as Fractions -, every frame of a group carrying the
    group's; ValueError when the group's sum could pass 2^63 - 1"""
    corr = np.asarray(corr)
    n, S = corr.shape[0], corr.shape[1]
    R = S // 2
    cells = [[[int(x) for x in r] for r in f] for f in corr]
    if n and group * max(abs(x) for f in cells for r in f for x in r) > LIMIT:
        raise ValueError("the sum of the group's surfaces could pass 2^63 - 1")
    out = []
    for a in range(0, n, group):
        g = [[sum(f[iy][ix] for f in cells[a:a + group]) for ix in range(S)] for iy in range(S)]
        peak = max(max(r) for r in g)
        dy, dx = min(((iy - R) ** 2 + (ix - R) ** 2, iy - R, ix - R) for iy in range(S) for ix in range(S) if g[iy][ix] == peak)[1:]
        border = abs(dy) == R or abs(dx) == R
        fy, fx = Fraction(dy), Fraction(dx)
        if not border:
            iy, ix = dy + R, dx + R
            den = 2 * (g[iy - 1][ix] - 2 * peak + g[iy + 1][ix])
            fy += Fraction(g[iy - 1][ix] - g[iy + 1][ix], den) if den else 0
            den = 2 * (g[iy][ix - 1] - 2 * peak + g[iy][ix + 1])
            fx += Fraction(g[iy][ix - 1] - g[iy][ix + 1], den) if den else 0
        out += [(dy, dx, peak, border, peak > 0, fy, fx)] * len(cells[a:a + group])
    return out
