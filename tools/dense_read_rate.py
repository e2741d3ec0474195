"""Development: frames/s of four ways from a level-1 file to its pixels as arrays - one file of detector-like events (the clustered generator
bench.py --clustered uses: 4096 x 4096, d = 12, 64 frames, ~4.3 % of the pixels set in clusters of 1..6), written by ReCoDeWriter with LZ4 -
interleaved in ONE process on one GPU with the file in the page cache:
  (a) dense_host     ReCoDeReader.iter_frames_dense(): whole frames written by the device, 2 bytes per PIXEL come back (32 MiB a frame)
  (b) coo_scatter    iter_frames_coo(batch), then per frame np.zeros and a scatter on the host: what callers do today (frame.toarray())
  (c) dense_roi      (a) with a 512 x 512 region in the middle of the frame: only its cells are written and come back
  (d) dense_device   get_frames_dense(out=a device tensor), batch by batch: nothing comes back at all
and the write-only floor of (d)'s kernel on this box: torch's zero_() of one batch's output, per frame.
Before anything is timed the four are compared on the first frames with one another and with plain numpy on the source frames.  A timed
window repeats whole passes over the file until it is at least 0.5 s long and ends behind a call that has waited for the device.  Prints one
JSON line per window and one summary line (median, min .. max) per way.
usage: dense_read_rate.py [frames 64] [repetitions 5] [seeds_ppm 11000] [coo batch 16]   (DENSE_RATE_SIDE=n: n x n frames, the region n/8 x n/8)"""
import json, os, shutil, statistics, sys, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from pyrecode_amd import _lib
from pyrecode_amd.params import InputParams
from pyrecode_amd.recode_reader import ReCoDeReader, merge_parts
from pyrecode_amd.recode_writer import ReCoDeWriter

nz = int(sys.argv[1]) if len(sys.argv) > 1 else 64
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
ppm = int(sys.argv[3]) if len(sys.argv) > 3 else 11000
coo_batch = int(sys.argv[4]) if len(sys.argv) > 4 else 16
ny = nx = int(os.environ.get("DENSE_RATE_SIDE", "4096"))
CHUNK = 16
MIN_WINDOW = 0.5
if _lib.device_count() == 0:
    raise SystemExit("dense_read_rate.py: no GPU visible - there is nothing to measure without one")
import torch  # noqa: E402  (the frames are drawn on the device by the library's own generator)


def write_file(tmp):
    L = _lib.lib()
    N = ny * nx
    dark_dev = torch.empty(N, dtype=torch.int16, device="cuda")
    _lib.check(L.rc_synth_dark(0, 20261020, N, dark_dev.data_ptr()))
    dark = dark_dev.cpu().numpy().view(np.uint16).reshape(ny, nx)
    ip = InputParams()
    ip._param_map.update(dict(reduction_level=1, rc_operation_mode=1, calibration_threshold_epsilon=0, target_bit_depth=12, source_bit_depth=12,
                              num_cols=nx, num_rows=ny, num_frames=1, frame_offset=0, num_calibration_frames=1, calibration_frame_offset=0,
                              keep_part_files=1, num_threads=1, l2_statistics=0, l4_centroiding=0, compression_scheme=2, compression_level=1,
                              source_file_type=0, source_header_length=0, keep_calibration_data=0, calibration_file_type=0, source_data_type=0,
                              target_data_type=0))
    w = ReCoDeWriter("d", dark_data=dark, output_directory=tmp, input_params=ip, mode="stream", validation_frame_gap=-1, node_id=0, run_name="d")
    w.start()
    first = None
    for a in range(0, nz, CHUNK):
        k = min(CHUNK, nz - a)
        stack = torch.empty((k, N), dtype=torch.int16, device="cuda")
        _lib.check(L.rc_synth_frames_clustered(0, 20261020, a, k, nx, ny, ppm, dark_dev.data_ptr(), stack.data_ptr()))
        torch.cuda.synchronize()
        fr = stack.cpu().numpy().view(np.uint16).reshape(k, ny, nx)
        if first is None:
            first = fr[:2].copy()
        w.run(fr)
    w.close()
    merge_parts(tmp, "d.rc1", 1)
    return os.path.join(tmp, "d.rc1"), np.where(first > dark, first - dark, 0).astype(np.uint16)


tmp = tempfile.mkdtemp(dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
try:
    path, want = write_file(tmp)
    rd = ReCoDeReader(path)
    rd.open(print_header=False)
    rd._ra_off = True
    side = nx // 8
    roi = (slice((ny - side) // 2, (ny - side) // 2 + side), slice((nx - side) // 2, (nx - side) // 2 + side))
    dt = np.dtype(rd._numpy_dtype)
    dev_batch = rd._dense_batch(rd._dense_region(None), dt)
    dev_out = torch.empty((dev_batch, ny, nx), dtype=torch.int16, device="cuda")
    scratch = np.zeros((ny, nx), dt)

    def dense_host():
        cells = 0
        for _, arr in rd.iter_frames_dense(0, nz):
            cells += arr.size
        return cells

    def coo_scatter(keep=None):
        for a, pre, (rows, cols, vals) in rd.iter_frames_coo(0, nz, batch=coo_batch):
            for i in range(len(pre) - 1):
                lo, hi = int(pre[i]), int(pre[i + 1])
                frame = np.zeros((ny, nx), dt)
                frame[rows[lo:hi], cols[lo:hi]] = vals[lo:hi]
                if keep is not None and a + i < len(keep):
                    keep[a + i] = frame
        return nz * ny * nx

    def dense_roi():
        cells = 0
        for _, arr in rd.iter_frames_dense(0, nz, roi=roi):
            cells += arr.size
        return cells

    def dense_device():
        for a in range(0, nz, dev_batch):
            k = min(dev_batch, nz - a)
            rd.get_frames_dense(a, k, out=dev_out[:k])          # (synchronous: has waited for the device when it returns)
        return nz * ny * nx

    def memset_floor():
        for a in range(0, nz, dev_batch):
            dev_out[:min(dev_batch, nz - a)].zero_()
        torch.cuda.synchronize()
        return nz * ny * nx
    # ---- the ways against numpy on the first two frames, before anything is timed ----
    got_b = [None, None]
    coo_scatter(got_b)
    got_a = next(iter(rd.iter_frames_dense(0, 2)))[1].copy()
    got_c = next(iter(rd.iter_frames_dense(0, 2, roi=roi)))[1].copy()
    rd.get_frames_dense(0, 2, out=dev_out[:2])
    got_d = dev_out[:2].cpu().numpy().view(np.uint16)
    if not (np.array_equal(got_a, want) and np.array_equal(np.stack(got_b), want) and np.array_equal(got_c, want[(slice(None),) + roi]) and
            np.array_equal(got_d, want)):
        raise SystemExit("dense_read_rate.py: the ways disagree with numpy on the first 2 frames")
    route = rd.last_batch_path
    methods = [("dense_host", dense_host), ("coo_scatter", coo_scatter), ("dense_roi", dense_roi), ("dense_device", dense_device),
               ("memset_floor", memset_floor)]
    for _, fn in methods:
        fn()                                    # warm: buffers, the library's workspaces, every kernel's code object
    rates = {m: [] for m, _ in methods}
    for r in range(reps):
        for m, fn in methods:
            passes, t0 = 0, time.perf_counter()
            while True:
                fn()                            # (every way ends with a call that has waited for the device)
                passes += 1
                dt_s = time.perf_counter() - t0
                if dt_s >= MIN_WINDOW:
                    break
            rates[m].append(passes * nz / dt_s)
            print(json.dumps(dict(way=m, rep=r, frames=passes * nz, seconds=round(dt_s, 4), frames_per_s=round(passes * nz / dt_s, 1))), flush=True)
    for m, _ in methods:
        v = rates[m]
        med = statistics.median(v)
        cells = (side * side if m == "dense_roi" else ny * nx)
        print(json.dumps(dict(way=m, median_frames_per_s=round(med, 1), min=round(min(v), 1), max=round(max(v), 1), reps=reps, frames=nz, side=nx,
                              seeds_ppm=ppm, output_GB_per_s=round(med * cells * dt.itemsize / 1e9, 2), dense_batch=dev_batch, route=route)), flush=True)
    rd.close()
finally:
    shutil.rmtree(tmp, ignore_errors=True)
