"""Development: frames/s of two ways to the frame traces of a file - 4096 x 4096, 12 bit, 1 % of the pixels set, written by this library with
LZ4 - interleaved in ONE process on one GPU with the file in the page cache, for k = 0, 1, 8 and 16 weight planes:
  (a) traces_k              ReCoDeReader.iter_frame_traces(batch=64, weights=a FrameTrace of k planes): decoded, counted and REDUCED on the
                            device, 8 * (4 + k) bytes per frame come back
  (b) coo_plus_host_k       what a caller did before for the same numbers: iter_frames_coo(batch=64) - the set pixels cross the link, 10
                            bytes each - and on the host np.add.reduceat over nnz_prefix for the four moments, W[:, rows, cols] gathered,
                            multiplied and reduced the same way for the weighted sums
  (c) sum_frames            iter_frame_sums(64), for scale: the neighbouring final kernel (k_expand_sum_b) on the same batches
Before anything is timed (a) and (b) are compared on the first 8 frames for every k: they must be equal.  A timed window repeats whole passes
over the file until it is at least 0.5 s long and holds at least two passes, and ends behind a call that has waited for the device.  Prints one JSON line per window and one
summary line (median, min .. max) per path.
usage: trace_read_rate.py [frames 128] [repetitions 5] [ppm 10000]   (TRACE_RATE_SIDE=n in the environment: n x n frames;
TRACE_RATE_KERNELS=1: no windows - two passes of (a) for every k and of (c), for a kernel trace of its own)"""
import json, os, shutil, statistics, sys, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from pyrecode_amd import _lib
from pyrecode_amd.params import InputParams
from pyrecode_amd.recode_reader import ReCoDeReader, merge_parts
from pyrecode_amd.recode_writer import ReCoDeWriter

nz = int(sys.argv[1]) if len(sys.argv) > 1 else 128
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
ppm = int(sys.argv[3]) if len(sys.argv) > 3 else 10000
ny = nx = int(os.environ.get("TRACE_RATE_SIDE", "4096"))
kernels_only = os.environ.get("TRACE_RATE_KERNELS") == "1"
PLANES = (0, 1, 8, 16)
CHUNK, BATCH, MIN_WINDOW, MIN_PASSES = 32, 64, 0.5, 2
if _lib.device_count() == 0:
    raise SystemExit("trace_read_rate.py: no GPU visible - there is nothing to measure without one")
import torch  # noqa: E402  (the frames and the weights are drawn on the device)


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


def per_frame(products, pre):
    """sums of `products` (int64[..., nnz]) over every frame's range of nnz_prefix: reduceat, with the empty frames - for which reduceat
    returns the element at the index instead of 0 - put to zero"""
    starts = pre[:-1].astype(np.int64)
    counts = np.diff(pre.astype(np.int64))
    if products.shape[-1] == 0:
        return np.zeros(products.shape[:-1] + (len(counts),), np.int64)
    out = np.add.reduceat(products, np.minimum(starts, products.shape[-1] - 1), axis=-1)
    out[..., counts == 0] = 0
    return out


def host_traces(rd, a, n, w_host):
    """(b)'s work for frames a .. a+n-1: int64[n, 4 + k]"""
    k = 0 if w_host is None else w_host.shape[0]
    out, at = np.zeros((n, 4 + k), np.int64), 0
    for _, pre, (rows, cols, vals) in rd.iter_frames_coo(a, n, batch=BATCH):
        m = len(pre) - 1
        v = vals.astype(np.int64)
        out[at:at + m, 0] = np.diff(pre.astype(np.int64))
        out[at:at + m, 1] = per_frame(v, pre)
        out[at:at + m, 2] = per_frame(v * rows, pre)
        out[at:at + m, 3] = per_frame(v * cols, pre)
        if k:
            out[at:at + m, 4:] = per_frame(w_host[:, rows, cols].astype(np.int64) * v, pre).T
        at += m
    return out


def device_traces(rd, a, n, ft):
    out, at = np.zeros((n, ft.columns), np.int64), 0
    for _, t in rd.iter_frame_traces(a, n, batch=BATCH, weights=ft):
        m = len(t["count"])
        out[at:at + m, 0], out[at:at + m, 1], out[at:at + m, 2], out[at:at + m, 3] = t["count"], t["sum"], t["sum_row"], t["sum_col"]
        out[at:at + m, 4:] = t["weighted"]
        at += m
    return out


tmp = tempfile.mkdtemp(dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
try:
    dark_dev = torch.randint(80, 121, (ny, nx), device="cuda", dtype=torch.int32)
    dark = dark_dev.cpu().numpy().astype(np.uint16)
    path = write_file(tmp, dark, dark_dev)
    rd = ReCoDeReader(path)
    rd.open(print_header=False)
    rd._ra_off = True
    # weights of 20 bits, signed, drawn on the device; the handles keep their own interleaved copies, the host keeps the planes for (b)
    w_dev = torch.randint(-(1 << 20), 1 << 20, (max(PLANES), ny, nx), device="cuda", dtype=torch.int32,
                          generator=torch.Generator(device="cuda").manual_seed(7))
    w_host = w_dev.cpu().numpy()
    handles = {k: _lib.FrameTrace(nx, ny, w_dev[:k] if k else None) for k in PLANES}
    del w_dev
    torch.cuda.empty_cache()
    # ---- the two paths against each other on the first 8 frames, before anything is timed ----
    for k in PLANES:
        got_a = device_traces(rd, 0, 8, handles[k])
        path_a = rd.last_batch_path
        got_b = host_traces(rd, 0, 8, w_host[:k] if k else None)
        if not (np.array_equal(got_a, got_b) and got_a[:, 0].all() and (k == 0 or got_a[:, 4:].any())):
            raise SystemExit("trace_read_rate.py: the two paths disagree on the first 8 frames (k = %d)" % k)

    def traces(k):
        return lambda: device_traces(rd, 0, nz, handles[k]).shape[0]

    def coo_plus_host(k):
        return lambda: host_traces(rd, 0, nz, w_host[:k] if k else None).shape[0]

    def sum_frames():
        cells = 0
        for a, m, img in rd.iter_frame_sums(BATCH, 0, nz):
            cells += img.size
        return cells
    methods = [("traces_%d" % k, traces(k)) for k in PLANES] + [("sum_frames", sum_frames)]
    if kernels_only:
        for _, fn in methods:
            fn()
            fn()
        print(json.dumps(dict(kernels_only=True, frames=nz, batch=BATCH, side=nx, ppm=ppm, route=path_a)), flush=True)
    else:
        methods += [("coo_plus_host_%d" % k, coo_plus_host(k)) for k in PLANES]
        for _, fn in methods:
            fn()                                    # warm: buffers, the library's workspaces, every kernel's code object
        rates = {m: [] for m, _ in methods}
        for r in range(reps):
            for m, fn in methods:                   # interleaved: every path in every repetition
                passes, t0 = 0, time.perf_counter()
                while True:
                    fn()                            # (every path ends with a call that has waited for the device)
                    passes += 1
                    dt = time.perf_counter() - t0
                    if dt >= MIN_WINDOW and passes >= MIN_PASSES:
                        break
                rates[m].append(passes * nz / dt)
                print(json.dumps(dict(path=m, rep=r, frames=passes * nz, seconds=round(dt, 4), frames_per_s=round(passes * nz / dt, 1))), flush=True)
        for m, _ in methods:
            v = rates[m]
            print(json.dumps(dict(path=m, median_frames_per_s=round(statistics.median(v), 1), min=round(min(v), 1), max=round(max(v), 1), reps=reps,
                                  frames=nz, batch=BATCH, side=nx, ppm=ppm, route=path_a)), flush=True)
    for ft in handles.values():
        ft.close()
    rd.close()
finally:
    shutil.rmtree(tmp, ignore_errors=True)
