"""Development: frames/s of the ways to the per-frame, per-bin counts and sums of a file - 4096 x 4096, 12 bit, 1 % of the pixels set, written by
this library with LZ4 - interleaved in ONE process on one GPU with the file in the page cache:
  (a) bins_B                ReCoDeReader.iter_frame_bins(batch=64, labels=a FrameBins): decoded, counted and BINNED on the device, 16 * B
                            bytes per frame come back.  B = 64: a grid of 8 x 8 segments; B = 2896: a radial map of width 1 about the
                            frame's middle; B = 16: a grid of 4 x 4 segments, beside (b'); B = 1: every pixel in the one
                            bin - all of a wave's adds go to one address
  (b) traces_16             iter_frame_traces(batch=64, weights=16 planes): the yardstick, untouched - the neighbouring final kernel on the
                            same batches
  (b') traces_16_one_hot    the same call with the 16 one-hot planes of the B = 16 grid: what a caller could do for up to 16 bins before
  (c) coo_bincount_B        what a caller did before for any B: iter_frames_coo(batch=64) - the set pixels cross the link, 10 bytes each -
                            and on the host labels[rows, cols] and two np.bincount per frame
Before anything is timed (a) and (c) are compared on the first 8 frames for every B, and (a) at B = 16 with (b')'s weighted columns: they
must be equal.  A timed window repeats whole passes over the path's frames - the whole file for the device paths, the first `host frames`
for (c) - until it is at least 0.5 s long, and ends behind a call that has waited for the device.  Prints one JSON line per window and one
summary line (median, min .. max) per path, and the verdict: (a)'s slowest window against (c)'s fastest, for B = 64 and B = 2896.
usage: bins_read_rate.py [frames 256] [repetitions 5] [ppm 10000] [host frames 64]   (BINS_RATE_SIDE=n in the environment: n x n frames;
BINS_RATE_KERNELS=1: no windows - two passes of every device path, for a kernel trace of its own)"""
import json, os, shutil, statistics, sys, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from pyrecode_amd import _lib
from pyrecode_amd.params import InputParams
from pyrecode_amd.reader_batched import radial_labels
from pyrecode_amd.recode_reader import ReCoDeReader, merge_parts
from pyrecode_amd.recode_writer import ReCoDeWriter

nz = int(sys.argv[1]) if len(sys.argv) > 1 else 256
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
ppm = int(sys.argv[3]) if len(sys.argv) > 3 else 10000
host_frames = min(nz, int(sys.argv[4]) if len(sys.argv) > 4 else 64)
ny = nx = int(os.environ.get("BINS_RATE_SIDE", "4096"))
kernels_only = os.environ.get("BINS_RATE_KERNELS") == "1"
CHUNK, BATCH, MIN_WINDOW, IGNORE = 32, 64, 0.5, 0xFFFF
if _lib.device_count() == 0:
    raise SystemExit("bins_read_rate.py: no GPU visible - there is nothing to measure without one")
import torch  # noqa: E402  (the frames and the yardstick's weights are drawn on the device)


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
                              keep_part_files=1, num_threads=1, l2_statistics=0, l4_centroiding=0, compression_scheme=2, compression_level=1,
                              source_file_type=0, source_header_length=0, keep_calibration_data=0, calibration_file_type=0, source_data_type=0,
                              target_data_type=0))
    w = ReCoDeWriter("t", dark_data=dark, output_directory=tmp, input_params=ip, mode="stream", validation_frame_gap=-1, node_id=0, run_name="t")
    w.start()
    for a in range(0, nz, CHUNK):
        w.run(chunk_of_frames(dark_dev, a, min(CHUNK, nz - a)))
    w.close()
    merge_parts(tmp, "t.rc1", 1)
    return os.path.join(tmp, "t.rc1")


def grid_labels(side):
    """a grid of side x side segments over the frame"""
    r, c = np.arange(ny) * side // ny, np.arange(nx) * side // nx
    return (r[:, None] * side + c[None, :]).astype(np.uint16)


def host_bins(rd, a, n, lab, B):
    """(c)'s work for frames a .. a+n-1: int64[n, 2, B] from the COO stream, labels[rows, cols] and two np.bincount per frame (the weighted
    one sums in float64: exact here, a bin's sum is far below 2^53)"""
    out, at = np.zeros((n, 2, B), np.int64), 0
    for _, pre, (rows, cols, vals) in rd.iter_frames_coo(a, n, batch=BATCH):
        pre = pre.astype(np.int64)
        bins = lab[rows, cols]
        for f in range(len(pre) - 1):
            b, v = bins[pre[f]:pre[f + 1]], vals[pre[f]:pre[f + 1]]
            keep = b != IGNORE
            b = b[keep]
            out[at, 0] = np.bincount(b, minlength=B)
            out[at, 1] = np.bincount(b, weights=v[keep], minlength=B).astype(np.int64)
            at += 1
    return out


def device_bins(rd, a, n, fb):
    out, at = np.zeros((n, 2, fb.n_bins), np.int64), 0
    for _, t in rd.iter_frame_bins(a, n, batch=BATCH, labels=fb):
        m = len(t["frame_ids"])
        out[at:at + m, 0], out[at:at + m, 1] = t["count"], t["sum"]
        at += m
    return out


def device_traces(rd, a, n, ft):
    return np.concatenate([t["weighted"] for _, t in rd.iter_frame_traces(a, n, batch=BATCH, weights=ft)])


tmp = tempfile.mkdtemp(dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
try:
    dark_dev = torch.randint(80, 121, (ny, nx), device="cuda", dtype=torch.int32)
    dark = dark_dev.cpu().numpy().astype(np.uint16)
    path = write_file(tmp, dark, dark_dev)
    rd = ReCoDeReader(path)
    rd.open(print_header=False)
    rd._ra_off = True
    radial = radial_labels(ny, nx, (ny - 1) / 2, (nx - 1) / 2)
    maps = {64: grid_labels(8), int(radial.max()) + 1: radial}
    BS = tuple(maps)                                   # (64, 2896 at 4096 x 4096)
    maps[16] = grid_labels(4)
    maps[1] = np.zeros((ny, nx), np.uint16)
    EXTRA = (16, 1)                                    # (timed and checked, not part of the verdict)
    handles = {B: _lib.FrameBins(nx, ny, lab, B) for B, lab in maps.items()}
    g = torch.Generator(device="cuda").manual_seed(7)
    w_dev = torch.randint(-(1 << 20), 1 << 20, (16, ny, nx), device="cuda", dtype=torch.int32, generator=g)
    ft = _lib.FrameTrace(nx, ny, w_dev)
    hot_dev = (torch.from_numpy(maps[16].astype(np.int32)).cuda()[None] == torch.arange(16, device="cuda", dtype=torch.int32)[:, None, None]).to(torch.int32)
    ft_hot = _lib.FrameTrace(nx, ny, hot_dev)
    del w_dev, hot_dev
    torch.cuda.empty_cache()
    # ---- the paths against each other on the first 8 frames, before anything is timed ----
    slab = min(8, nz)
    for B in BS + EXTRA:
        got_a = device_bins(rd, 0, slab, handles[B])
        path_a = rd.last_batch_path
        got_c = host_bins(rd, 0, slab, maps[B], B)
        if not (np.array_equal(got_a, got_c) and got_a.any(axis=(1, 2)).all()):
            raise SystemExit("bins_read_rate.py: the two paths disagree on the first 8 frames (B = %d)" % B)
        if B == 16 and not np.array_equal(got_a[:, 1], device_traces(rd, 0, slab, ft_hot)):
            raise SystemExit("bins_read_rate.py: B = 16 and the traces under 16 one-hot planes disagree on the first 8 frames")

    def bins(B):
        return lambda: device_bins(rd, 0, nz, handles[B]).shape[0]

    def coo_bincount(B):
        return lambda: host_bins(rd, 0, host_frames, maps[B], B).shape[0]

    def traces(handle):
        return lambda: sum(len(t["count"]) for _, t in rd.iter_frame_traces(0, nz, batch=BATCH, weights=handle))
    device = [("bins_%d" % B, bins(B)) for B in BS + EXTRA] + [("traces_16", traces(ft)), ("traces_16_one_hot", traces(ft_hot))]
    host = [("coo_bincount_%d" % B, coo_bincount(B)) for B in BS]
    if kernels_only:
        for _, fn in device:
            fn()
            fn()
        print(json.dumps(dict(kernels_only=True, frames=nz, batch=BATCH, side=nx, ppm=ppm, bins=BS + EXTRA, route=path_a)), flush=True)
    else:
        for _, fn in device + host:
            fn()                                    # warm: buffers, the library's workspaces, every kernel's code object
        methods = device + host
        rates = {m: [] for m, _ in methods}
        for r in range(reps):
            for m, fn in methods:                   # interleaved: every path in every repetition
                frames, t0 = 0, time.perf_counter()
                while True:
                    frames += fn()                  # (every path ends with a call that has waited for the device)
                    dt = time.perf_counter() - t0
                    if dt >= MIN_WINDOW:
                        break
                rates[m].append(frames / dt)
                print(json.dumps(dict(path=m, rep=r, frames=frames, seconds=round(dt, 4), frames_per_s=round(frames / dt, 1))), flush=True)
        for m, _ in methods:
            v = rates[m]
            print(json.dumps(dict(path=m, median_frames_per_s=round(statistics.median(v), 1), min=round(min(v), 1), max=round(max(v), 1), reps=reps,
                                  frames=nz, batch=BATCH, side=nx, ppm=ppm, route=path_a)), flush=True)
        med = {m: statistics.median(v) for m, v in rates.items()}
        for B in BS:
            slowest_a, fastest_c = min(rates["bins_%d" % B]), max(rates["coo_bincount_%d" % B])
            print(json.dumps(dict(bins=B, bins_slowest=round(slowest_a, 1), coo_bincount_fastest=round(fastest_c, 1), ratio=round(slowest_a / fastest_c, 1),
                                  bins_over_traces_16=round(med["bins_%d" % B] / med["traces_16"], 3), device_is_faster=bool(slowest_a > fastest_c))), flush=True)
        print(json.dumps(dict(bins=16, bins_16_over_traces_16_one_hot=round(med["bins_16"] / med["traces_16_one_hot"], 3),
                              bins_16_over_traces_16=round(med["bins_16"] / med["traces_16"], 3), bins_1_over_traces_16=round(med["bins_1"] / med["traces_16"], 3))), flush=True)
    for fb in handles.values():
        fb.close()
    ft.close()
    ft_hot.close()
    rd.close()
finally:
    shutil.rmtree(tmp, ignore_errors=True)
