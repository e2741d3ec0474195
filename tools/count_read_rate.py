"""Development: frames/s of two ways from a level-1 file to its counted electrons - one file of detector-like events (the clustered
generator bench.py --clustered uses: 4096 x 4096, d = 12, 64 frames, ~4.3 % of the pixels set in clusters of 1..6), written by ReCoDeWriter
with LZ4 - interleaved in ONE process on one GPU with the file in the page cache:
  (a) counted        ReCoDeReader.iter_frames_counted(batch): decoded, labelled and reduced on the device, 20 bytes per EVENT come back
  (b) coo_then_host  iter_frames_coo(batch), then the host's way per frame: scipy.ndimage.label on the dense map and np.bincount centroids -
                     what a caller had to do before; every set pixel crosses the link (10 bytes each)
(b) labels a 16 Mpixel frame in a fraction of a second, so a window of (b) covers `host_frames` frames and one of (a) whole passes over the
file; both are repeated `repetitions` times in turn and the medians are reported.  Before anything is timed the two are compared on the
first frames: the same number of events, the same total weight.  A measurement, not a gate: no test depends on a rate.
usage: count_read_rate.py [frames 64] [batch 16] [repetitions 5] [host_frames 4] [seeds_ppm 11000]   (COUNT_RATE_SIDE=n: n x n frames)"""
import json, os, shutil, statistics, sys, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import scipy.ndimage as nd
from pyrecode_amd import _lib
from pyrecode_amd.params import InputParams
from pyrecode_amd.recode_reader import ReCoDeReader, merge_parts
from pyrecode_amd.recode_writer import ReCoDeWriter

nz = int(sys.argv[1]) if len(sys.argv) > 1 else 64
batch = int(sys.argv[2]) if len(sys.argv) > 2 else 16
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
host_frames = min(int(sys.argv[4]) if len(sys.argv) > 4 else 4, nz)
ppm = int(sys.argv[5]) if len(sys.argv) > 5 else 11000
ny = nx = int(os.environ.get("COUNT_RATE_SIDE", "4096"))
CHUNK = 16
MIN_WINDOW = 0.5
EIGHT = np.ones((3, 3), int)
if _lib.device_count() == 0:
    raise SystemExit("count_read_rate.py: no GPU visible - there is nothing to measure without one")
import torch  # noqa: E402  (the frames are drawn on the device by the library's own generator)


def write_file(tmp):
    L = _lib.lib()
    N = ny * nx
    dark_dev = torch.empty(N, dtype=torch.int16, device="cuda")
    _lib.check(L.rc_synth_dark(0, 20261003, N, dark_dev.data_ptr()))
    dark = dark_dev.cpu().numpy().view(np.uint16).reshape(ny, nx)
    ip = InputParams()
    ip._param_map.update(dict(reduction_level=1, rc_operation_mode=1, calibration_threshold_epsilon=0, target_bit_depth=12, source_bit_depth=12,
                              num_cols=nx, num_rows=ny, num_frames=1, frame_offset=0, num_calibration_frames=1, calibration_frame_offset=0,
                              keep_part_files=1, num_threads=1, l2_statistics=0, l4_centroiding=0, compression_scheme=2, compression_level=1,
                              source_file_type=0, source_header_length=0, keep_calibration_data=0, calibration_file_type=0, source_data_type=0,
                              target_data_type=0))
    w = ReCoDeWriter("c", dark_data=dark, output_directory=tmp, input_params=ip, mode="stream", validation_frame_gap=-1, node_id=0, run_name="c")
    w.start()
    for a in range(0, nz, CHUNK):
        k = min(CHUNK, nz - a)
        stack = torch.empty((k, N), dtype=torch.int16, device="cuda")
        _lib.check(L.rc_synth_frames_clustered(0, 20261003, a, k, nx, ny, ppm, dark_dev.data_ptr(), stack.data_ptr()))
        torch.cuda.synchronize()
        w.run(stack.cpu().numpy().view(np.uint16).reshape(k, ny, nx))
    w.close()
    merge_parts(tmp, "c.rc1", 1)
    return os.path.join(tmp, "c.rc1")


def host_count(rows, cols, vals):
    """the host's way for one frame: label the dense map, then per-label sums with np.bincount (float64) and the weighted average"""
    dense = np.zeros((ny, nx), bool)
    dense[rows, cols] = True
    labels, n = nd.label(dense, structure=EIGHT)
    lab = labels[rows, cols]
    v = vals.astype(np.float64)
    w = np.bincount(lab, v, n + 1)[1:]
    r = np.bincount(lab, v * rows, n + 1)[1:] / w
    c = np.bincount(lab, v * cols, n + 1)[1:] / w
    return np.round(r).astype(np.int32), np.round(c).astype(np.int32), w


tmp = tempfile.mkdtemp(dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
try:
    rd = ReCoDeReader(write_file(tmp))
    rd.open(print_header=False)
    rd._ra_off = True

    def counted():
        events = 0
        for item in rd.iter_frames_counted(0, nz, batch=batch):
            events += int(item[1][-1])
        return nz, events

    def coo_then_host():
        events = 0
        for _, pre, (rows, cols, vals) in rd.iter_frames_coo(0, host_frames, batch=min(batch, host_frames)):
            for f in range(len(pre) - 1):
                lo, hi = int(pre[f]), int(pre[f + 1])
                events += host_count(rows[lo:hi], cols[lo:hi], vals[lo:hi])[0].size
        return host_frames, events

    # ---- the two ways on the first frames, before anything is timed ----
    prefix, _, _, area, weight = rd.get_frames_counted(0, host_frames)
    _, host_events = coo_then_host()
    pre, (rows, cols, vals) = rd.get_frames_coo(0, host_frames)
    if int(prefix[-1]) != host_events or int(weight.sum()) != int(vals.astype(np.int64).sum()) or int(area.sum()) != int(pre[-1]):
        raise SystemExit("count_read_rate.py: the two ways disagree on the first %d frames" % host_frames)
    route = rd.last_batch_path
    set_fraction = int(pre[-1]) / (host_frames * ny * nx)
    methods = [("counted", counted), ("coo_then_host", coo_then_host)]
    counted()                                        # warm: buffers, the library's workspaces, every kernel's code object
    rates = {m: [] for m, _ in methods}
    for r in range(reps):
        for m, fn in methods:
            frames, t0 = 0, time.perf_counter()
            while True:
                frames += fn()[0]                    # (both end behind a call that has waited for the device)
                dt = time.perf_counter() - t0
                if dt >= MIN_WINDOW:
                    break
            rates[m].append(frames / dt)
            print(json.dumps(dict(path=m, rep=r, frames=frames, seconds=round(dt, 4), frames_per_s=round(frames / dt, 2))), flush=True)
    med = {m: statistics.median(v) for m, v in rates.items()}
    for m, _ in methods:
        v = rates[m]
        print(json.dumps(dict(path=m, median_frames_per_s=round(med[m], 2), min=round(min(v), 2), max=round(max(v), 2), reps=reps, frames=nz,
                              batch=batch, side=nx, seeds_ppm=ppm, set_fraction=round(set_fraction, 4), events_per_frame=round(host_events / host_frames),
                              route=route if m == "counted" else rd.last_batch_path)), flush=True)
    print(json.dumps(dict(ratio_counted_over_host=round(med["counted"] / med["coo_then_host"], 1))), flush=True)
    rd.close()
finally:
    shutil.rmtree(tmp, ignore_errors=True)
