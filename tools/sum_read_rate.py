"""Development: frames/s of three ways to the summed views of a file - 4096 x 4096, 12 bit, 1 % of the pixels set, written by this library
with LZ4 and with zstd, views of 64 frames - interleaved in ONE process on one GPU with the file in the page cache:
  (a) sum_frames            ReCoDeReader.iter_frame_sums(64): decoded, counted and ADDED on the device, 4 bytes per pixel come back per view
  (b) coo_only              iter_frames_coo(batch=64) alone: the set pixels cross the link (10 bytes each) and nobody adds them up - the
                            yardstick, a path this library had before the summed views and that they do not touch
  (c) coo_plus_host_add     (b) followed by np.add.at into a uint32 image per view: what a caller had to do for the same result
Before anything is timed the three are compared on a slab of 8 frames with plain numpy on the source frames.  A timed window repeats whole
passes over the file until it is at least 0.5 s long and ends behind a call that has waited for the device.  Prints one JSON line per window
and one summary line (median, min .. max) per scheme and path.
usage: sum_read_rate.py [frames 256] [view 64] [repetitions 5] [ppm 10000]   (SUM_RATE_SIDE=n in the environment: n x n frames)"""
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
ny = nx = int(os.environ.get("SUM_RATE_SIDE", "4096"))
CHUNK = 32
MIN_WINDOW = 0.5
if _lib.device_count() == 0:
    raise SystemExit("sum_read_rate.py: no GPU visible - there is nothing to measure without one")
import torch  # noqa: E402  (the frames are drawn on the device: 256 frames of 4096 x 4096 take minutes with numpy)


def chunk_of_frames(dark_dev, first, k):
    g = torch.Generator(device="cuda").manual_seed(1000 + first)
    hit = torch.rand((k, ny, nx), device="cuda", generator=g) < ppm * 1e-6
    amp = torch.randint(1, 2048, (k, ny, nx), device="cuda", generator=g, dtype=torch.int32)
    fr = torch.where(hit, dark_dev.to(torch.int32) + amp, dark_dev.to(torch.int32) // 2)
    return fr.to(torch.int16).cpu().numpy().view(np.uint16)          # (12-bit values)


def write_file(tmp, scheme, dark, dark_dev):
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


def host_add(rd, a, n, out):
    """(c)'s work for frames a .. a+n-1: the COO batches added into out (uint32[ny, nx]) on the host"""
    for _, pre, (rows, cols, vals) in rd.iter_frames_coo(a, n, batch=64):
        np.add.at(out, (rows, cols), vals)


tmp = tempfile.mkdtemp(dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
try:
    dark_dev = torch.randint(80, 121, (ny, nx), device="cuda", dtype=torch.int32)
    dark = dark_dev.cpu().numpy().astype(np.uint16)
    summary = []
    for scheme, name in ((2, "lz4"), (1, "zstd")):
        path, slab = write_file(tmp, scheme, dark, dark_dev)
        rd = ReCoDeReader(path)
        rd.open(print_header=False)
        rd._ra_off = True
        # ---- the three paths against numpy on a small slab, before anything is timed ----
        want = np.where(slab > dark, slab.astype(np.int64) - dark, 0).sum(0).astype(np.uint64)
        got_a = rd.sum_frames(0, 8)
        got_c = np.zeros((ny, nx), np.uint32)
        host_add(rd, 0, 8, got_c)
        if not (np.array_equal(got_a, want) and np.array_equal(got_c, want)):
            raise SystemExit("sum_read_rate.py: the paths disagree with numpy on the first 8 frames (%s)" % name)
        path_a = rd.last_batch_path

        def sum_frames():
            cells = 0
            for a, k, img in rd.iter_frame_sums(view, 0, nz):
                cells += img.size
            return cells

        def coo_only():
            got = 0
            for _, pre, _arrays in rd.iter_frames_coo(0, nz, batch=64):
                got += int(pre[-1])
            return got

        def coo_plus_host_add():
            img = np.zeros((ny, nx), np.uint32)
            for a in range(0, nz, view):
                img[:] = 0
                host_add(rd, a, min(view, nz - a), img)
            return int(img.size)
        methods = [("sum_frames", sum_frames), ("coo_only", coo_only), ("coo_plus_host_add", coo_plus_host_add)]
        for _, fn in methods:
            fn()                                    # warm: buffers, the library's workspaces, every kernel's code object
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
                print(json.dumps(dict(scheme=name, path=m, rep=r, frames=passes * nz, seconds=round(dt, 4), frames_per_s=round(passes * nz / dt, 1))), flush=True)
        for m, _ in methods:
            v = rates[m]
            summary.append(dict(scheme=name, path=m, median_frames_per_s=round(statistics.median(v), 1), min=round(min(v), 1), max=round(max(v), 1),
                                reps=reps, frames=nz, view=view, side=nx, ppm=ppm, route=path_a if m == "sum_frames" else rd.last_batch_path))
        rd.close()
        os.remove(path)
    for line in summary:
        print(json.dumps(line), flush=True)
finally:
    shutil.rmtree(tmp, ignore_errors=True)
