"""Development: frames/s of three ways from a level-1 file to the counted image of its frames - the file of tools/count_read_rate.py
(the clustered generator bench.py --clustered uses: 4096 x 4096, d = 12, 64 frames, ~4.3 % of the pixels set in clusters of 1..6, written
by ReCoDeWriter with LZ4) - interleaved in ONE process on one GPU with the file in the page cache:
  (A) counted_view_s1, _s2   ReCoDeReader.iter_frame_sums_counted(64 frames per view, batch, upsample 1 and 2): decoded, labelled, reduced
                             and ADDED UP on the device; 4 bytes per cell of the view come back once per view
  (B) events_then_host       iter_frames_counted(batch), then the host's np.add.at of the events into the same image: what a caller had to
                             do before; 20 bytes per event cross the link
  (C) events_only            iter_frames_counted(batch) alone - (A) does strictly less device work than this: no event is written or copied
Each way is repeated `repetitions` times in turn, a window of at least 0.5 s each, and medians and ranges are reported.  Before anything
is timed (A) at upsample 1 and (B) are compared on the whole file: the same image.  A measurement, not a gate: no test depends on a rate.
usage: counted_view_rate.py [frames 64] [batch 16] [repetitions 5] [seeds_ppm 11000]   (COUNT_RATE_SIDE=n: n x n frames)"""
import json, os, shutil, statistics, sys, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from pyrecode_amd import _lib
from pyrecode_amd.params import InputParams
from pyrecode_amd.recode_reader import ReCoDeReader, merge_parts
from pyrecode_amd.recode_writer import ReCoDeWriter

nz = int(sys.argv[1]) if len(sys.argv) > 1 else 64
batch = int(sys.argv[2]) if len(sys.argv) > 2 else 16
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
ppm = int(sys.argv[4]) if len(sys.argv) > 4 else 11000
ny = nx = int(os.environ.get("COUNT_RATE_SIDE", "4096"))
CHUNK = 16
MIN_WINDOW = 0.5
if _lib.device_count() == 0:
    raise SystemExit("counted_view_rate.py: no GPU visible - there is nothing to measure without one")
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


tmp = tempfile.mkdtemp(dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
try:
    rd = ReCoDeReader(write_file(tmp))
    rd.open(print_header=False)
    rd._ra_off = True
    host_image = np.zeros((ny, nx), np.uint32)
    last = {}

    def counted_view(s, keep=False):
        def run():
            for _, _, img in rd.iter_frame_sums_counted(nz, 0, nz, batch=batch, upsample=s):
                if keep:                             # (img is a view of page-locked memory that goes away with the generator: the fetch
                    last["view"] = img.copy()        # has happened either way)
            return nz
        return run

    def events_then_host():
        host_image[:] = 0
        for item in rd.iter_frames_counted(0, nz, batch=batch):
            np.add.at(host_image, (item[2], item[3]), 1)
        return nz

    def events_only():
        events = 0
        for item in rd.iter_frames_counted(0, nz, batch=batch):
            events += int(item[1][-1])
        last["events"] = events
        return nz

    # ---- (A) at upsample 1 and (B) on the whole file, before anything is timed ----
    counted_view(1, keep=True)()
    image_a = last.pop("view")
    events_then_host()
    events_only()
    if not np.array_equal(image_a, host_image) or int(image_a.sum(dtype=np.uint64)) != last["events"]:
        raise SystemExit("counted_view_rate.py: the device's view and the host's accumulation of the events disagree")
    route = rd.last_batch_path
    methods = [("counted_view_s1", counted_view(1)), ("counted_view_s2", counted_view(2)), ("events_then_host", events_then_host),
               ("events_only", events_only)]
    counted_view(2)()                                # warm: buffers, the library's workspaces, every kernel's code object
    rates = {m: [] for m, _ in methods}
    for r in range(reps):
        for m, fn in methods:
            frames, t0 = 0, time.perf_counter()
            while True:
                frames += fn()                       # (every way ends behind a call that has waited for the device)
                dt = time.perf_counter() - t0
                if dt >= MIN_WINDOW:
                    break
            rates[m].append(frames / dt)
            print(json.dumps(dict(path=m, rep=r, frames=frames, seconds=round(dt, 4), frames_per_s=round(frames / dt, 2))), flush=True)
    med = {m: statistics.median(v) for m, v in rates.items()}
    for m, _ in methods:
        v = rates[m]
        print(json.dumps(dict(path=m, median_frames_per_s=round(med[m], 2), min=round(min(v), 2), max=round(max(v), 2), reps=reps, frames=nz,
                              batch=batch, side=nx, seeds_ppm=ppm, events_per_frame=round(last["events"] / nz), route=route)), flush=True)
    print(json.dumps(dict(ratio_view_s1_over_events_then_host=round(med["counted_view_s1"] / med["events_then_host"], 2),
                          ratio_view_s1_over_events_only=round(med["counted_view_s1"] / med["events_only"], 3),
                          ratio_view_s2_over_view_s1=round(med["counted_view_s2"] / med["counted_view_s1"], 3))), flush=True)
    rd.close()
finally:
    shutil.rmtree(tmp, ignore_errors=True)
