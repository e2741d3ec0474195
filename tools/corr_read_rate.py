"""Development: frames/s of the ways to the per-frame correlation surfaces of a file - 4096 x 4096, 12 bit, 1 % of the pixels set, written by
this library with LZ4 - interleaved in ONE process on one GPU with the file in the page cache, for the radii given (8 and 16):
  (a) corr_R                ReCoDeReader.iter_frame_correlations(batch=64, reference=a FrameCorrelation of radius R): decoded, counted and
                            CORRELATED on the device, 8 * (2 R + 1)^2 bytes per frame come back
  (b) traces_16             iter_frame_traces(batch=64, weights=16 planes): the yardstick, untouched - the neighbouring final kernel on the
                            same batches
  (c) coo_plus_host_R       what a caller did before for the same numbers without an FFT: iter_frames_coo(batch=64) - the set pixels cross
                            the link, 10 bytes each - and on the host one numpy gather on the zero-padded reference per offset of the window,
                            multiplied and reduced over nnz_prefix.  It is slow - (2 R + 1)^2 passes over the batch's pixels -, so its
                            window is ONE pass over the first `host frames` frames.
Before anything is timed (a) and (c) are compared on the first 8 frames for every radius: they must be equal.  A timed window of (a) and (b)
repeats whole passes over the file until it is at least 0.5 s long and holds at least two passes, and ends behind a call that has waited
for the device.  Prints one JSON line per window and one summary line (median, min .. max) per path, and the verdict: (a)'s slowest
window against (c)'s fastest.
usage: corr_read_rate.py [frames 256] [repetitions 5] [ppm 10000] [radii 8,16] [host frames 8]   (CORR_RATE_SIDE=n in the environment:
n x n frames; CORR_RATE_KERNELS=1: no windows - two passes of (a) for every radius and of (b), for a kernel trace of its own)"""
import json, os, shutil, statistics, sys, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from pyrecode_amd import _lib
from pyrecode_amd.params import InputParams
from pyrecode_amd.recode_reader import ReCoDeReader, merge_parts
from pyrecode_amd.recode_writer import ReCoDeWriter

nz = int(sys.argv[1]) if len(sys.argv) > 1 else 256
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
ppm = int(sys.argv[3]) if len(sys.argv) > 3 else 10000
RADII = tuple(int(r) for r in (sys.argv[4] if len(sys.argv) > 4 else "8,16").split(","))
host_frames = min(nz, int(sys.argv[5]) if len(sys.argv) > 5 else 8)
ny = nx = int(os.environ.get("CORR_RATE_SIDE", "4096"))
kernels_only = os.environ.get("CORR_RATE_KERNELS") == "1"
CHUNK, BATCH, MIN_WINDOW, MIN_PASSES = 32, 64, 0.5, 2
if _lib.device_count() == 0:
    raise SystemExit("corr_read_rate.py: no GPU visible - there is nothing to measure without one")
import torch  # noqa: E402  (the frames, the reference and the yardstick's weights are drawn on the device)


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
    """sums of `products` (int64[nnz]) over every frame's range of nnz_prefix: reduceat, with the empty frames - for which reduceat returns the
    element at the index instead of 0 - put to zero"""
    starts = pre[:-1].astype(np.int64)
    counts = np.diff(pre.astype(np.int64))
    if products.shape[-1] == 0:
        return np.zeros(len(counts), np.int64)
    out = np.add.reduceat(products, np.minimum(starts, products.shape[-1] - 1))
    out[counts == 0] = 0
    return out


def host_corr(rd, a, n, pad, R):
    """(c)'s work for frames a .. a+n-1: int64[n, S, S] from the COO stream and the padded reference (int64[ny + 2 R, nx + 2 R])"""
    S = 2 * R + 1
    out, at = np.zeros((n, S, S), np.int64), 0
    for _, pre, (rows, cols, vals) in rd.iter_frames_coo(a, n, batch=BATCH):
        m = len(pre) - 1
        v, r, c = vals.astype(np.int64), rows.astype(np.int64), cols.astype(np.int64)
        for iy in range(S):
            for ix in range(S):
                out[at:at + m, iy, ix] = per_frame(pad[r + iy, c + ix] * v, pre)
        at += m
    return out


def device_corr(rd, a, n, fc):
    out, at = np.zeros((n, fc.side, fc.side), np.int64), 0
    for _, t in rd.iter_frame_correlations(a, n, batch=BATCH, reference=fc):
        m = len(t["count"])
        out[at:at + m] = t["corr"]
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
    # the reference: what a summed fraction looks like - 16 frames' worth of 12-bit values in 15 % of the cells -, drawn on the device
    g = torch.Generator(device="cuda").manual_seed(7)
    t_dev = torch.where(torch.rand((ny, nx), device="cuda", generator=g) < 0.15, torch.randint(1, 4096, (ny, nx), device="cuda", dtype=torch.int32, generator=g), 0)
    t_dev = t_dev.to(torch.int32)
    t_host = t_dev.cpu().numpy().astype(np.int64)
    corrs = {R: _lib.FrameCorrelation(nx, ny, t_dev, R) for R in RADII}
    pads = {R: np.pad(t_host, R) for R in RADII}
    w_dev = torch.randint(-(1 << 20), 1 << 20, (16, ny, nx), device="cuda", dtype=torch.int32, generator=g)
    ft = _lib.FrameTrace(nx, ny, w_dev)
    del w_dev, t_dev
    torch.cuda.empty_cache()
    # ---- the two paths against each other on the first 8 frames, before anything is timed ----
    for R in RADII:
        got_a = device_corr(rd, 0, min(8, nz), corrs[R])
        path_a = rd.last_batch_path
        got_c = host_corr(rd, 0, min(8, nz), pads[R], R)
        if not (np.array_equal(got_a, got_c) and got_a.any(axis=(1, 2)).all()):
            raise SystemExit("corr_read_rate.py: the two paths disagree on the first 8 frames (R = %d)" % R)

    def corr(R):
        return lambda: device_corr(rd, 0, nz, corrs[R]).shape[0]

    def coo_plus_host(R):
        return lambda: host_corr(rd, 0, host_frames, pads[R], R).shape[0]

    def traces():
        return sum(len(t["count"]) for _, t in rd.iter_frame_traces(0, nz, batch=BATCH, weights=ft))
    device = [("corr_%d" % R, corr(R)) for R in RADII] + [("traces_16", traces)]
    host = [("coo_plus_host_%d" % R, coo_plus_host(R)) for R in RADII]
    if kernels_only:
        for _, fn in device:
            fn()
            fn()
        print(json.dumps(dict(kernels_only=True, frames=nz, batch=BATCH, side=nx, ppm=ppm, radii=RADII, route=path_a)), flush=True)
    else:
        for _, fn in device:
            fn()                                    # warm: buffers, the library's workspaces, every kernel's code object ((c) ran above)
        methods = device + host
        rates = {m: [] for m, _ in methods}
        for r in range(reps):
            for m, fn in methods:                   # interleaved: every path in every repetition
                one_pass = m.startswith("coo_plus_host")
                frames, t0 = 0, time.perf_counter()
                while True:
                    frames += fn()                  # (every path ends with a call that has waited for the device)
                    dt = time.perf_counter() - t0
                    if one_pass or (dt >= MIN_WINDOW and frames >= MIN_PASSES * nz):
                        break
                rates[m].append(frames / dt)
                print(json.dumps(dict(path=m, rep=r, frames=frames, seconds=round(dt, 4), frames_per_s=round(frames / dt, 1))), flush=True)
        for m, _ in methods:
            v = rates[m]
            print(json.dumps(dict(path=m, median_frames_per_s=round(statistics.median(v), 1), min=round(min(v), 1), max=round(max(v), 1), reps=reps,
                                  frames=nz, batch=BATCH, side=nx, ppm=ppm, route=path_a)), flush=True)
        for R in RADII:
            slowest_a, fastest_c = min(rates["corr_%d" % R]), max(rates["coo_plus_host_%d" % R])
            print(json.dumps(dict(radius=R, corr_slowest=round(slowest_a, 1), coo_plus_host_fastest=round(fastest_c, 2), ratio=round(slowest_a / fastest_c, 1),
                                  corr_over_traces_16=round(statistics.median(rates["corr_%d" % R]) / statistics.median(rates["traces_16"]), 3),
                                  device_is_faster=bool(slowest_a > fastest_c))), flush=True)
    for fc in corrs.values():
        fc.close()
    ft.close()
    rd.close()
finally:
    shutil.rmtree(tmp, ignore_errors=True)
