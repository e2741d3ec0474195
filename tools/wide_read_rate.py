"""Development: read rate of a file of more than 16 bits (4096 x 4096 uint32 frames, 1 % of the pixels set, 20-bit values, LZ4 on the
device) two ways: iter_frames_coo in batches, and a sequential get_frame loop.  The file is written once and kept; every `read` is a process
of its own, and --tree lets it import pyrecode_amd from ANOTHER checkout (with its library built), so two commits are compared on one box
by alternating processes over the same file in the page cache.  `read` prints one JSON line per repetition and one summary line per
method (median and min..max frames/s); the first pass of each method warms file cache, buffers and workspaces and is not counted.
usage: wide_read_rate.py write FILE [nframes 128]
       wide_read_rate.py read FILE [batch 64] [repetitions 5] [--tree DIR] [--label NAME]"""
import json, os, statistics, sys, time

argv = sys.argv[1:]


def option(name, default):
    if name in argv:
        i = argv.index(name)
        value = argv[i + 1]
        del argv[i:i + 2]
        return value
    return default


tree = option("--tree", os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
label = option("--label", os.path.basename(os.path.abspath(tree)))
sys.path.insert(0, os.path.abspath(tree))
import numpy as np
from pyrecode_amd.params import InputParams
from pyrecode_amd.recode_reader import ReCoDeReader, merge_parts
from pyrecode_amd.recode_writer import ReCoDeWriter

ny = nx = 4096
N = ny * nx
D, PPM, CHUNK = 20, 10000, 16


def write(path, nz):
    folder = os.path.dirname(os.path.abspath(path))
    rng = np.random.default_rng(11)
    dark = rng.integers(1000, 70000, N).astype(np.uint32)
    below = dark // 2
    ip = InputParams()
    ip._param_map.update(dict(reduction_level=1, rc_operation_mode=1, calibration_threshold_epsilon=0, target_bit_depth=D, source_bit_depth=D,
                              num_cols=nx, num_rows=ny, num_frames=1, frame_offset=0, num_calibration_frames=1, calibration_frame_offset=0,
                              keep_part_files=1, num_threads=1, l2_statistics=0, l4_centroiding=0, compression_scheme=2, compression_level=1,
                              source_file_type=0, source_header_length=0, keep_calibration_data=0, calibration_file_type=0, source_data_type=0,
                              target_data_type=0))
    w = ReCoDeWriter("wide", dark_data=dark.reshape(ny, nx), output_directory=folder, input_params=ip, mode="stream", run_name="wide", node_id=0,
                     batch_size=CHUNK)
    w.start()
    set_pixels = 0
    for a in range(0, nz, CHUNK):
        k = min(CHUNK, nz - a)
        chunk = np.empty((k, N), np.uint32)
        for z in range(k):
            idx = np.unique(rng.integers(0, N, N * PPM // 1000000))
            chunk[z] = below
            chunk[z, idx] = dark[idx] + rng.integers(1, (1 << D) - 70000, idx.size).astype(np.uint32)
            set_pixels += idx.size
        w.run(chunk.reshape(k, ny, nx))
    w.close()
    merge_parts(folder, "wide.rc1", 1)                       # (the part file is wide.rc1_part000)
    os.replace(os.path.join(folder, "wide.rc1"), path)
    os.remove(os.path.join(folder, "wide.rc1_part000"))
    print(json.dumps(dict(written=path, frames=nz, set_pixels=set_pixels, bytes=os.path.getsize(path))))


def read(path, batch, reps):
    rd = ReCoDeReader(path)
    rd.open(print_header=False)
    nz = int(rd._header["nz"])

    def iter_coo():
        got, dtype = 0, None
        for a, prefix, (rows, cols, vals) in rd.iter_frames_coo(0, nz, batch=batch):
            got += int(prefix[-1])
            dtype = vals.dtype
        return got, "%s, values %s" % (rd.last_batch_path, dtype)

    def get_frame_loop():
        got = 0
        for z in range(nz):
            got += rd.get_frame(z)[z]["data"].nnz
        return got, "read-ahead served %d" % rd.readahead_frames_served
    methods = [("iter_frames_coo", iter_coo), ("get_frame loop", get_frame_loop)]
    for _, fn in methods:
        fn()
    rates = {name: [] for name, _ in methods}
    for r in range(reps):
        for name, fn in methods:
            t0 = time.perf_counter()
            nnz, how = fn()
            dt = time.perf_counter() - t0
            rates[name].append(nz / dt)
            print(json.dumps(dict(tree=label, method=name, rep=r, frames=nz, batch=batch, seconds=round(dt, 5), frames_per_s=round(nz / dt, 1),
                                  set_pixels=nnz, how=how)))
    for name, _ in methods:
        v = rates[name]
        print(json.dumps(dict(tree=label, method=name, median_frames_per_s=round(statistics.median(v), 1), min=round(min(v), 1), max=round(max(v), 1),
                              reps=reps)))
    rd.close()


if argv and argv[0] == "write":
    write(argv[1], int(argv[2]) if len(argv) > 2 else 128)
elif argv and argv[0] == "read":
    read(argv[1], int(argv[2]) if len(argv) > 2 else 64, int(argv[3]) if len(argv) > 3 else 5)
else:
    sys.exit(__doc__)
