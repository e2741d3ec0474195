"""Development: what the calibration kernels cost on a device-resident stack (default: 100 frames of 4096 x 4096 uint16, 3.4 GB), against
numpy on the host and against one plain read of the same bytes.

  rc_calib_stats      per-pixel median / std / range over all frames (one read of the stack on the LDS path)
  rc_calib_histogram  100 bins of frame - median over the last n_stats frames
  host                np.median / np.std(axis=0) on a slab of --host-rows rows of the same stack, scaled to the whole frame (the whole
                      stack takes minutes on the host; the slab's pixels are independent columns like all others)
  plain read          tools/bw_probe's "linear read" rate (a child process, when the probe is built:
                      hipcc -O3 --offload-arch=gfx950 tools/bw_probe.hip -o tools/bw_probe) -> the time one read of the stack takes at that rate

Every pointer handed to the library is device memory, so a call is its kernel plus one stream synchronise.  Timing: the host clock around
WINDOWS of back-to-back calls (each call returns after its synchronise), every window at least half a second long, `--reps` windows after a
warm-up call; ms per call as median and min .. max over the windows.  It is the cost of a call, not a kernel time (no HIP events: the
entry points run on the library's own stream and take none from the caller).
Results are checked against numpy on the slab before anything is timed.  Prints one JSON line.
usage: calibration_rate.py [--frames 100] [--ny 4096] [--nx 4096] [--stats 10] [--reps 5] [--host-rows 128]"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import numpy as np   # noqa: E402


def plain_read_rate():
    """TB/s of bw_probe's linear reads, measured in a child process BEFORE this process opens the GPU's memory for the stack"""
    exe = os.path.join(HERE, "bw_probe")
    if not os.path.exists(exe):
        return None
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300).stdout
    rates = [float(m.group(1)) for m in re.finditer(r"^linear read.*?([0-9.]+) TB/s", out, re.M)]
    return max(rates) if rates else None


def timed(fn, batches, window_s=0.5):
    """ms per call: after one warm-up call, `batches` windows of back-to-back calls, each window at least `window_s` long (the number of
    calls per window comes from the warm-up's own time), so that what a single call adds around its kernel - launch, the closing stream
    synchronise, pointer queries, the utility context's lock - is spread over many calls' device time and a window is long against the
    clock and the scheduler.  The figure is therefore the cost of a CALL (kernel + that overhead), not a kernel time."""
    t0 = time.perf_counter()
    fn()
    once = time.perf_counter() - t0
    calls = max(10, int(window_s / max(once, 1e-6)) + 1)
    ms = []
    for _ in range(batches):
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        ms.append((time.perf_counter() - t0) * 1e3 / calls)
    return {"calls_per_window": calls, "windows": batches, "median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--ny", type=int, default=4096)
    ap.add_argument("--nx", type=int, default=4096)
    ap.add_argument("--stats", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-rows", type=int, default=128)
    a = ap.parse_args()
    read_tbs = plain_read_rate()
    import torch
    from pyrecode_amd import _lib as hip
    if hip.device_count() == 0:
        raise SystemExit("no GPU visible: nothing to measure")
    n, ny, nx, N = a.frames, a.ny, a.nx, a.ny * a.nx
    gen = torch.Generator(device="cuda").manual_seed(1)
    offset = torch.randint(80, 121, (N,), device="cuda", generator=gen).float()
    stack = torch.empty((n, N), dtype=torch.int16, device="cuda")
    for f in range(n):       # offsets 80..120, Gaussian noise of sigma 6, 1 % events of +60..2000
        v = offset + 6.0 * torch.randn(N, device="cuda", generator=gen)
        ev = torch.rand(N, device="cuda", generator=gen) < 0.01
        v = torch.where(ev, v + torch.randint(60, 2001, (N,), device="cuda", generator=gen).float(), v)
        stack[f] = v.round().clamp(0, 32767).to(torch.int16)
    torch.cuda.synchronize()     # the library reads on its own streams: the generator's kernels must be done (include/recode_hip.h)
    med, std = torch.empty(N, dtype=torch.float32, device="cuda"), torch.empty(N, dtype=torch.float32, device="cuda")
    rng = torch.zeros(2, dtype=torch.int32, device="cuda")
    counts = torch.zeros(100, dtype=torch.int64, device="cuda")
    L = hip.lib()

    def stats():
        hip.check(L.rc_calib_stats(stack.data_ptr(), n, N, a.stats, med.data_ptr(), std.data_ptr(), rng.data_ptr()), "rc_calib_stats")
    stats()
    r2 = rng.cpu().numpy()
    edges = np.histogram_bin_edges(np.array([r2[0] / 2.0, r2[1] / 2.0]), bins=100)
    d_edges = torch.from_numpy(edges).cuda()
    torch.cuda.synchronize()

    def histogram():
        hip.check(L.rc_calib_histogram(stack.data_ptr() + 2 * N * (n - a.stats), a.stats, N, med.data_ptr(), d_edges.data_ptr(), 100, counts.data_ptr()),
                  "rc_calib_histogram")
    histogram()
    # ---- the same on the host, on a slab; it is also the check ----------------------------------------------------------------------
    rows = min(a.host_rows, ny)
    slab = stack[:, :rows * nx].cpu().numpy().view(np.uint16)
    t0 = time.perf_counter()
    h_med = np.median(slab, axis=0)
    h_std = np.std(slab, axis=0)
    host_s = (time.perf_counter() - t0) * ny / rows
    assert np.array_equal(med[:rows * nx].cpu().numpy(), h_med.astype(np.float32)), "median differs from numpy"
    ulp = np.abs(std[:rows * nx].cpu().numpy().view(np.int32).astype(np.int64) - h_std.astype(np.float32).view(np.int32).astype(np.int64))
    assert ulp.max() <= 1, "std differs from numpy by %d ulp" % ulp.max()
    assert int(counts.sum()) == a.stats * N
    res = {"frames": n, "ny": ny, "nx": nx, "n_stats": a.stats, "stack_bytes": 2 * n * N, "lds_path": n <= L.rc_calib_lds_max_frames(),
           "stats": timed(stats, a.reps), "histogram": timed(histogram, a.reps),
           "host_median_std_s_scaled_from_rows": [host_s, rows], "plain_read_TBps": read_tbs}
    res["stats"]["stack_GBps"] = 2 * n * N / (res["stats"]["median_ms"] * 1e-3) / 1e9
    res["histogram"]["values_per_s"] = a.stats * N / (res["histogram"]["median_ms"] * 1e-3)
    if read_tbs:
        res["plain_read_of_the_stack_ms"] = 2 * n * N / (read_tbs * 1e12) * 1e3
    print(json.dumps(res))


if __name__ == "__main__":
    main()
