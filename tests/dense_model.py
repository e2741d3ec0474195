"""The model of rc_expand_frames_dense in numpy: a batch of STORED frames (op_mode 0: the binary map, then the packed values or a level-2
statistics stream) and a region -> array[n, h, w].  The GPU tests (tests/test_gpu_dense.py) compare with it; tests/test_dense_plan_cpu.py
checks it against hand-written literals."""
import numpy as np


def unpack_fields(stream, count, d):
    """the first `count` d-bit LSB-first fields of a packed stream (recode_writer.py:637-652)"""
    bits = np.unpackbits(np.asarray(stream, np.uint8), bitorder="little")[:count * d].reshape(count, d).astype(np.uint64)
    return (bits << np.arange(d, dtype=np.uint64)).sum(1, dtype=np.uint64)


def dense_model(blob, sizes, ny, nx, d, level, region, dtype):
    """out[f, j, i] = the value of pixel (y0 + j * step_y, x0 + i * step_x) of frame f: its d-bit field at level 1, 1 at levels 2 and 3, 0
    where the pixel is not set.  Returns (out, set-pixel prefix over the whole frames uint64[n + 1])."""
    x0, y0, w, h, sx, sy = region
    n, at = sizes.shape[0], 0
    out, prefix = np.zeros((n, h, w), dtype), np.zeros(n + 1, np.uint64)
    for f in range(n):
        sz_map, sz_val = int(sizes[f, 0]), int(sizes[f, 1])
        mask = np.unpackbits(blob[at:at + sz_map], bitorder="little")[:ny * nx].astype(bool)
        frame = np.zeros(ny * nx, np.uint64)
        frame[mask] = unpack_fields(blob[at + sz_map:at + sz_map + sz_val], int(mask.sum()), d) if level == 1 else 1
        out[f] = frame.reshape(ny, nx)[y0:y0 + (h - 1) * sy + 1:sy, x0:x0 + (w - 1) * sx + 1:sx].astype(dtype)
        prefix[f + 1] = prefix[f] + np.uint64(mask.sum())
        at += sz_map + sz_val
    return out, prefix
