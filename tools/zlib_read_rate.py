"""Development: read rate of a device-zlib file (4096 x 4096, 1 % of the pixels set, 16 bit, reduction level 1, compression_scheme 0
written with device_zlib=True) through iter_frames_triplets two ways, interleaved on one box with the file in the page cache:
device_zlib=False (the stock inflate on the host's worker threads, then one device expand per batch: the path such files took before the
batched device inflate, and the yardstick) and device_zlib=True (rc_inflate.hip).  Once at compression_level 1 (stored values) and once
at 6 (Huffman-coded values).  Prints one JSON line per repetition and one summary line per method and level.
With `phases` as the last argument: RC_READ_TIMING is set, every batch goes through the synchronous call, and the medians of the
kernel times the library prints are reported instead (the calls are then not pipelined: no rates).
usage: zlib_read_rate.py [nframes 256] [batch 64] [repetitions 5] [ppm 10000] [phases]"""
import json, os, re, shutil, statistics, sys, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
args = [a for a in sys.argv[1:] if a != "phases"]
phases = "phases" in sys.argv[1:]
if phases:
    os.environ["RC_READ_TIMING"] = "1"          # (read once, by the library's first call)
import numpy as np
from pyrecode_amd import synth
from pyrecode_amd.params import InputParams
from pyrecode_amd.recode_reader import ReCoDeReader, merge_parts
from pyrecode_amd.recode_writer import ReCoDeWriter

nz = int(args[0]) if len(args) > 0 else 256
batch = int(args[1]) if len(args) > 1 else 64
reps = int(args[2]) if len(args) > 2 else 5
ppm = int(args[3]) if len(args) > 3 else 10000
ny = nx = 4096
N = ny * nx
dark = synth.dark_frame(3, N)
distinct = synth.frames(3, 0, min(nz, 16), N, ppm, dark)          # (a file of nz frames that repeats 16: the host generator takes 0.5 s a frame)
data = distinct[np.arange(nz) % distinct.shape[0]].reshape(nz, ny, nx)
del distinct
tmp = tempfile.mkdtemp(dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
try:
    readers = {}
    for clevel in (1, 6):
        ip = InputParams()
        ip._param_map.update(dict(reduction_level=1, rc_operation_mode=1, calibration_threshold_epsilon=0, target_bit_depth=16, source_bit_depth=16,
                                  num_cols=nx, num_rows=ny, num_frames=nz, frame_offset=0, num_calibration_frames=1, calibration_frame_offset=0,
                                  keep_part_files=1, num_threads=1, l2_statistics=0, l4_centroiding=0, compression_scheme=0, compression_level=clevel,
                                  source_file_type=0, source_header_length=0, keep_calibration_data=0, calibration_file_type=0, source_data_type=0,
                                  target_data_type=0))
        name = "z%d" % clevel
        w = ReCoDeWriter(name + ".bin", dark_data=dark.reshape(ny, nx), output_directory=tmp, input_params=ip, mode="batch", node_id=0, device_zlib=True)
        w.start()
        w.run(data)
        w.close()
        merge_parts(tmp, name + ".rc1", 1)
        rd = ReCoDeReader(os.path.join(tmp, name + ".rc1"))
        rd.open(print_header=False)
        rd._ra_off = True
        readers[clevel] = rd
        print(json.dumps(dict(compression_level=clevel, frames=rd._batch_frames(), file_bytes=os.path.getsize(os.path.join(tmp, name + ".rc1")))))
    del data

    def run(rd, device):
        got, paths = 0, set()
        if phases:                               # the synchronous call prints its phases
            for a in range(0, rd._batch_frames(), batch):
                prefix, _ = rd.get_frames_triplets(a, min(batch, rd._batch_frames() - a), coo=True, device_zlib=device)
                got += int(prefix[-1])
                paths.add(rd.last_batch_path)
            return got, "+".join(sorted(paths))
        for item in rd.iter_frames_triplets(0, rd._batch_frames(), batch=batch, coo=True, device_zlib=device):
            got += int(item[1][-1])
            paths.add(rd.last_batch_path)
        return got, "+".join(sorted(paths))
    methods = [("host inflate, clevel %d" % c, readers[c], False) for c in (1, 6)] + [("device inflate, clevel %d" % c, readers[c], True) for c in (1, 6)]
    if phases:
        err_path = os.path.join(tmp, "stderr.txt")
        keep = os.dup(2)
        for name, rd, device in methods[2:]:
            run(rd, device)                      # warm
            fd = os.open(err_path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC)
            os.dup2(fd, 2)
            try:
                for _ in range(reps):
                    run(rd, device)
            finally:
                os.dup2(keep, 2)
                os.close(fd)
            cols = {}
            for line in open(err_path):
                if line.startswith("rc_inflate:"):
                    for key, val in re.findall(r"([a-z ]+?) ([0-9.]+)(?: ms)?(?:,|$)", line.split(",", 1)[1].strip()):
                        cols.setdefault(key.strip(), []).append(float(val))
                elif line.startswith("rc_expand_frames:"):
                    for key, val in re.findall(r"([a-z+() ]+?) ([0-9.]+)(?: ms)?(?:,|$)", line.split(":", 1)[1].strip()):
                        cols.setdefault("call: " + key.strip(), []).append(float(val))
            print(json.dumps(dict(method=name, batch=batch, calls=len(next(iter(cols.values()), [])), median_ms={k: round(statistics.median(v), 3) for k, v in cols.items()})))
    else:
        for _, rd, device in methods:
            run(rd, device)                      # warm: file cache, buffers, the library's workspaces
        rates = {name: [] for name, _, _ in methods}
        for r in range(reps):
            for name, rd, device in methods:
                t0 = time.perf_counter()
                nnz, path = run(rd, device)
                dt = time.perf_counter() - t0
                n = rd._batch_frames()
                rates[name].append(n / dt)
                print(json.dumps(dict(method=name, rep=r, frames=n, batch=batch, seconds=round(dt, 5), frames_per_s=round(n / dt, 1), set_pixels=nnz, path=path)))
        for name, _, _ in methods:
            v = rates[name]
            print(json.dumps(dict(method=name, median_frames_per_s=round(statistics.median(v), 1), min=round(min(v), 1), max=round(max(v), 1), reps=reps)))
    for rd in readers.values():
        rd.close()
finally:
    shutil.rmtree(tmp, ignore_errors=True)
