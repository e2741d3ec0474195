"""The exact model of rc_bins_frames: a batch of STORED frames (op_mode 0: the binary map, then the packed values or a level-2 statistics
stream) and a label map -> int64[n, 2, B] - per frame and bin the number of set pixels and the sum of their values -, added per bin in
int64 (exact: a sum stays below 2^48); the chunking and workspace arithmetic of pyrecode_amd/csrc/rc_bins.h restated in Python integers;
and radial_labels restated as a pixel loop with math.isqrt.  The GPU tests (tests/test_gpu_bins.py) compare with it; tests/test_bins_cpu.py checks it against
hand-written literals and the C++ against the restatement."""
import math

import numpy as np

from dense_model import unpack_fields

IGNORE = 0xFFFF
BINS_MAX = 4096              # rc_bins.h: BINS_MAX
TARGET_WGS = 4096            # rc_bins.h: BINS_TARGET_WGS
PARTIAL_BUDGET = 32 << 20    # rc_bins.h: BINS_PARTIAL_BUDGET


def bins_of_pixels(idx, vals, labels, B):
    """int64[2, B] of one frame: idx its set pixels (row-major indices), vals their values, labels int[ny * nx].  np.add.at adds int64 to
    int64 one element at a time - exact, and a bin's sum stays below 2^48 (65535 * 65535 * 65535)."""
    out = np.zeros((2, B), np.int64)
    lab = np.asarray(labels).reshape(-1)[idx].astype(np.int64)
    keep = lab != IGNORE
    assert (lab[keep] < B).all(), "a label at or above B that is not 0xFFFF"
    np.add.at(out[0], lab[keep], 1)
    np.add.at(out[1], lab[keep], np.asarray(vals).astype(np.int64)[keep])
    return out


def bins_model(blob, sizes, ny, nx, d, level, labels, B):
    """out[f, 0, b] = frame f's set pixels with labels[row, col] == b, out[f, 1, b] = the sum of their values - the d-bit field at level 1,
    1 at levels 2 and 3 (a level-2 statistics stream is stepped over).  Returns (out int64[n, 2, B], set-pixel prefix uint64[n + 1])."""
    labels = np.asarray(labels).reshape(ny * nx)
    n, at = sizes.shape[0], 0
    out, prefix = np.zeros((n, 2, B), np.int64), np.zeros(n + 1, np.uint64)
    for f in range(n):
        sz_map, sz_val = int(sizes[f, 0]), int(sizes[f, 1])
        idx = np.flatnonzero(np.unpackbits(blob[at:at + sz_map], bitorder="little")[:ny * nx])
        vals = unpack_fields(blob[at + sz_map:at + sz_map + sz_val], idx.size, d) if level == 1 else np.ones(idx.size, np.uint64)
        assert vals.size == 0 or int(vals.max()) < 1 << 16
        out[f] = bins_of_pixels(idx, vals, labels, B)
        prefix[f + 1] = prefix[f] + np.uint64(idx.size)
        at += sz_map + sz_val
    return out, prefix


def bins_of_frames(frames, labels, B):
    """the same from dense frames int[n, ny, nx] (0 = not set), with numpy: bincount with integer weights would go through float64, so the
    sums are added per bin with np.add.at on int64 (a sum stays below 2^48)"""
    frames = np.asarray(frames)
    lab = np.asarray(labels).reshape(-1).astype(np.int64)
    out = np.zeros((len(frames), 2, B), np.int64)
    for f, fr in enumerate(frames):
        flat = fr.reshape(-1).astype(np.int64)
        at = np.flatnonzero((flat != 0) & (lab != IGNORE))
        assert (lab[at] < B).all()
        np.add.at(out[f, 0], lab[at], 1)
        np.add.at(out[f, 1], lab[at], flat[at])
    return out


def one_hot_planes(labels, B):
    """int32[B, ny, nx]: plane b is labels == b - what the traces take as weights for the second identity"""
    labels = np.asarray(labels)
    return np.stack([(labels == b).astype(np.int32) for b in range(B)])


# ---- rc_bins.h's host arithmetic --------------------------------------------------------------------------------------------------------
def tier(B):
    return 256 if B <= 256 else 1024 if B <= 1024 else 4096


def lds_bytes(B, level):
    return tier(B) * (12 if level == 1 else 4)


def target_wgs(B):
    return min(TARGET_WGS, PARTIAL_BUDGET // (16 * B))


def chunks(nblk, n, B):
    """(blocks a workgroup walks, workgroups per frame)"""
    want = max(1, min(nblk, -(-target_wgs(B) // n)))
    bpc = -(-nblk // want) if nblk else 1
    return bpc, (-(-nblk // bpc) if nblk else 1)


def workspace_bytes(nb8, n, B, wg=256):
    return n * chunks(-(-nb8 // wg), n, B)[1] * 2 * B * 8


# ---- radial_labels, restated --------------------------------------------------------------------------------------------------------------
def radial_model(ny, nx, cy2, cx2, bin_width, n_bins):
    """uint16[ny, nx] by a pixel loop: cy2, cx2 are TWICE the centre (integers)"""
    out = np.zeros((ny, nx), np.uint16)
    for r in range(ny):
        for c in range(nx):
            b = math.isqrt((2 * r - cy2) ** 2 + (2 * c - cx2) ** 2) // (2 * bin_width)
            out[r, c] = b if b < n_bins else IGNORE
    return out
