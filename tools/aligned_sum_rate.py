"""Development: frames/s of three ways to the ALIGNED summed views of a file - 4096 x 4096, 12 bit, 1 % of the pixels set, written by this
library with LZ4, views of 64 frames, every frame translated by a seeded random-walk drift within +-8 pixels - interleaved in ONE process on
one GPU with the file in the page cache:
  (a) shifted_sum           ReCoDeReader.iter_frame_sums(64, shifts=drift): decoded, counted, translated and ADDED on the device (k_sum_shift)
  (b) unshifted_sum         the same without shifts: k_expand_sum_b, a path this change does not touch - the yardstick
  (c) coo_plus_host_shift   iter_frames_coo(batch=64), the coordinates shifted and np.add.at into a uint32 image per view on the host: what a
                            caller with per-frame shifts had to do before
and the same trio for counted views at upsample 2 (shifts in fine cells, twice the drift):
  (a) counted_shifted       iter_frame_sums_counted(64, upsample=2, shifts=2 * drift)
  (b) counted_unshifted     the same without shifts
  (c) events_plus_host_add  iter_frames_counted(batch=64), the events' pixels put on the fine grid, shifted and np.add.at on the host (whole-pixel
                            positions: the events carry no sub-pixel centroid - the device's view is finer than anything this path can give)
Before anything is timed: (a) against numpy slice arithmetic on the source frames of a slab of 8; (c) against the same; the counted (a) at
upsample 1 against (c)'s arithmetic on the events, and at upsample 2 frame by frame against the unshifted view translated with numpy.  A timed
window repeats whole passes over the file until it is at least 0.5 s long and ends behind a call that has waited for the device.  Prints one
JSON line per window and one summary line (median, min .. max) per path.
usage: aligned_sum_rate.py [frames 256] [view 64] [repetitions 5] [ppm 10000] [scheme lz4|zstd]   (SUM_RATE_SIDE=n in the environment: n x n frames)"""
import json, os, shutil, statistics, sys, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from pyrecode_amd import _lib
from pyrecode_amd.params import InputParams
from pyrecode_amd.recode_reader import ReCoDeReader, merge_parts
from pyrecode_amd.recode_writer import ReCoDeWriter

nz = int(sys.argv[1]) if len(sys.argv) > 1 else 256
view = int(sys.argv[2]) if len(sys.argv) > 2 else 64
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
ppm = int(sys.argv[4]) if len(sys.argv) > 4 else 10000
scheme_name = sys.argv[5] if len(sys.argv) > 5 else "lz4"
scheme = {"lz4": 2, "zstd": 1}[scheme_name]
ny = nx = int(os.environ.get("SUM_RATE_SIDE", "4096"))
UP = 2
CHUNK = 32
MIN_WINDOW = 0.5
if _lib.device_count() == 0:
    raise SystemExit("aligned_sum_rate.py: no GPU visible - there is nothing to measure without one")
import torch  # noqa: E402  (the frames are drawn on the device: 256 frames of 4096 x 4096 take minutes with numpy)


def chunk_of_frames(dark_dev, first, k):
    g = torch.Generator(device="cuda").manual_seed(1000 + first)
    hit = torch.rand((k, ny, nx), device="cuda", generator=g) < ppm * 1e-6
    amp = torch.randint(1, 2048, (k, ny, nx), device="cuda", generator=g, dtype=torch.int32)
    fr = torch.where(hit, dark_dev.to(torch.int32) + amp, dark_dev.to(torch.int32) // 2)
    return fr.to(torch.int16).cpu().numpy().view(np.uint16)          # (12-bit values)


def write_file(tmp, dark, dark_dev):
    ip = InputParams()
    ip._param_map.update(dict(reduction_level=1, rc_operation_mode=1, calibration_threshold_epsilon=0, target_bit_depth=12, source_bit_depth=12,
                              num_cols=nx, num_rows=ny, num_frames=1, frame_offset=0, num_calibration_frames=1, calibration_frame_offset=0,
                              keep_part_files=1, num_threads=1, l2_statistics=0, l4_centroiding=0, compression_scheme=scheme, compression_level=1,
                              source_file_type=0, source_header_length=0, keep_calibration_data=0, calibration_file_type=0, source_data_type=0,
                              target_data_type=0))
    base = "s%d" % scheme
    w = ReCoDeWriter(base, dark_data=dark, output_directory=tmp, input_params=ip, mode="stream", validation_frame_gap=-1, node_id=0, run_name=base)
    w.start()
    slab = None
    for a in range(0, nz, CHUNK):
        fr = chunk_of_frames(dark_dev, a, min(CHUNK, nz - a))
        if slab is None:
            slab = fr[:8].copy()
        w.run(fr)
    w.close()
    merge_parts(tmp, base + ".rc1", 1)
    return os.path.join(tmp, base + ".rc1"), slab


def translated(img, dy, dx):
    """img moved by (dy, dx), what leaves is dropped, zeros come in"""
    out = np.zeros_like(img)
    h, w = img.shape
    if abs(dy) < h and abs(dx) < w:
        r0, r1, c0, c1 = max(0, dy), min(h, h + dy), max(0, dx), min(w, w + dx)
        out[r0:r1, c0:c1] = img[r0 - dy:r1 - dy, c0 - dx:c1 - dx]
    return out


def add_shifted_points(out, rows, cols, vals, pre, shifts):
    """(c)'s host work for one batch: frame i's points are [pre[i], pre[i + 1]); each is moved by its frame's shift and added if it stays inside"""
    per = np.diff(pre.astype(np.int64))
    r = rows.astype(np.int64) + np.repeat(shifts[:, 0], per)
    c = cols.astype(np.int64) + np.repeat(shifts[:, 1], per)
    ok = (r >= 0) & (r < out.shape[0]) & (c >= 0) & (c < out.shape[1])
    np.add.at(out, (r[ok], c[ok]), vals[ok] if vals is not None else 1)


def host_shift_add(rd, a, n, out, drift):
    for first, pre, (rows, cols, vals) in rd.iter_frames_coo(a, n, batch=64):
        add_shifted_points(out, rows, cols, vals, pre, drift[first:first + len(pre) - 1])


def host_event_add(rd, a, n, out, fine, s):
    for first, pre, rows, cols, _area, _weight in rd.iter_frames_counted(a, n, batch=64):
        add_shifted_points(out, s * rows.astype(np.int64) + (s - 1) // 2, s * cols.astype(np.int64) + (s - 1) // 2, None, pre, fine[first:first + len(pre) - 1])


tmp = tempfile.mkdtemp(dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
try:
    dark_dev = torch.randint(80, 121, (ny, nx), device="cuda", dtype=torch.int32)
    dark = dark_dev.cpu().numpy().astype(np.uint16)
    drift = np.clip(np.cumsum(np.random.default_rng(2024).integers(-1, 2, (nz, 2)), 0), -8, 8).astype(np.int64)      # within +-8 pixels
    fine = UP * drift
    path, slab = write_file(tmp, dark, dark_dev)
    rd = ReCoDeReader(path)
    rd.open(print_header=False)
    rd._ra_off = True
    # ---- correctness on a slab of 8 frames, before anything is timed ----
    k = min(8, nz)
    vals = np.where(slab[:k] > dark, slab[:k].astype(np.int64) - dark, 0).astype(np.uint32)
    want = sum(translated(vals[f], int(drift[f, 0]), int(drift[f, 1])).astype(np.uint64) for f in range(k))
    got_a = rd.sum_frames(0, k, shifts=drift[:k])
    path_a = rd.last_batch_path
    got_c = np.zeros((ny, nx), np.uint32)
    host_shift_add(rd, 0, k, got_c, drift)
    if not (np.array_equal(got_a, want) and np.array_equal(got_c, want)):
        raise SystemExit("aligned_sum_rate.py: the plain paths disagree with numpy on the first %d frames" % k)
    ev = np.zeros((ny, nx), np.uint32)
    host_event_add(rd, 0, k, ev, drift, 1)
    if not np.array_equal(rd.sum_frames_counted(0, k, upsample=1, shifts=drift[:k]), ev):
        raise SystemExit("aligned_sum_rate.py: the counted paths disagree at upsample 1 on the first %d frames" % k)
    for f in (k - 1,):
        plain = rd.sum_frames_counted(f, 1, upsample=UP)
        moved = rd.sum_frames_counted(f, 1, upsample=UP, shifts=fine[f:f + 1])
        if not np.array_equal(moved, translated(plain, int(fine[f, 0]), int(fine[f, 1]))):
            raise SystemExit("aligned_sum_rate.py: the counted view of frame %d at upsample %d is not the unshifted one translated" % (f, UP))
    del plain, moved, ev, got_a, got_c, want

    def run_sums(it):
        cells = 0
        for a, n, img in it:
            cells += img.size
        return cells

    def coo_plus_host_shift():
        img = np.zeros((ny, nx), np.uint32)
        for a in range(0, nz, view):
            img[:] = 0
            host_shift_add(rd, a, min(view, nz - a), img, drift)
        return int(img.size)

    def events_plus_host_add():
        img = np.zeros((UP * ny, UP * nx), np.uint32)
        for a in range(0, nz, view):
            img[:] = 0
            host_event_add(rd, a, min(view, nz - a), img, fine, UP)
        return int(img.size)
    methods = [("shifted_sum", lambda: run_sums(rd.iter_frame_sums(view, 0, nz, shifts=drift))),
               ("unshifted_sum", lambda: run_sums(rd.iter_frame_sums(view, 0, nz))),
               ("coo_plus_host_shift", coo_plus_host_shift),
               ("counted_shifted", lambda: run_sums(rd.iter_frame_sums_counted(view, 0, nz, upsample=UP, shifts=fine))),
               ("counted_unshifted", lambda: run_sums(rd.iter_frame_sums_counted(view, 0, nz, upsample=UP))),
               ("events_plus_host_add", events_plus_host_add)]
    routes = {}
    for m, fn in methods:
        fn()                                    # warm: buffers, the library's workspaces, every kernel's code object
        routes[m] = rd.last_batch_path
    rates = {m: [] for m, _ in methods}
    for r in range(reps):
        for m, fn in methods:
            passes, t0 = 0, time.perf_counter()
            while True:
                fn()                            # (every path ends with a call that has waited for the device: a fetch, or the last batch's wait)
                passes += 1
                dt = time.perf_counter() - t0
                if dt >= MIN_WINDOW:
                    break
            rates[m].append(passes * nz / dt)
            print(json.dumps(dict(scheme=scheme_name, path=m, rep=r, frames=passes * nz, seconds=round(dt, 4), frames_per_s=round(passes * nz / dt, 1))), flush=True)
    for m, _ in methods:
        v = rates[m]
        print(json.dumps(dict(scheme=scheme_name, path=m, median_frames_per_s=round(statistics.median(v), 1), min=round(min(v), 1), max=round(max(v), 1),
                              reps=reps, frames=nz, view=view, side=nx, ppm=ppm, upsample=UP if "count" in m or "event" in m else 1, route=routes[m],
                              slab_route=path_a)), flush=True)
    rd.close()
finally:
    shutil.rmtree(tmp, ignore_errors=True)
