"""Development: read rate of a BASELINE-configuration-4-shaped file (4096 x 4096, 0.1 % of the pixels set, reduction level 2, blosc-LZ4)
three ways, interleaved on one box with the file in the page cache: get_frames_triplets (the frame-at-a-time path such files take through
that call), get_frames_l2 and iter_frames_l2 (the batched device path).  Prints one JSON line per repetition and one summary line per
method (median and min..max frames/s).
usage: l2_read_rate.py [nframes 64] [batch 32] [repetitions 5] [ppm 1000]"""
import json, os, shutil, statistics, sys, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from pyrecode_amd import synth
from pyrecode_amd.params import InputParams
from pyrecode_amd.recode_reader import ReCoDeReader, merge_parts
from pyrecode_amd.recode_writer import ReCoDeWriter

nz = int(sys.argv[1]) if len(sys.argv) > 1 else 64
batch = int(sys.argv[2]) if len(sys.argv) > 2 else 32
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
ppm = int(sys.argv[4]) if len(sys.argv) > 4 else 1000
ny = nx = 4096
N = ny * nx
dark = synth.dark_frame(3, N)
frames = synth.frames(3, 0, nz, N, ppm, dark)
ip = InputParams()
ip._param_map.update(dict(reduction_level=2, rc_operation_mode=1, calibration_threshold_epsilon=0, target_bit_depth=12, source_bit_depth=12,
                          num_cols=nx, num_rows=ny, num_frames=nz, frame_offset=0, num_calibration_frames=1, calibration_frame_offset=0,
                          keep_part_files=1, num_threads=1, l2_statistics=2, l4_centroiding=0, compression_scheme=8, compression_level=1,
                          source_file_type=0, source_header_length=0, keep_calibration_data=0, calibration_file_type=0, source_data_type=0,
                          target_data_type=0))
tmp = tempfile.mkdtemp(dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
try:
    w = ReCoDeWriter("c4.bin", dark_data=dark.reshape(ny, nx), output_directory=tmp, input_params=ip, mode="batch", node_id=0)
    w.start(); w.run(frames.reshape(nz, ny, nx)); w.close()
    merge_parts(tmp, "c4.rc2", 1)
    del frames
    rd = ReCoDeReader(os.path.join(tmp, "c4.rc2"))
    rd.open(print_header=False)
    rd._ra_off = True

    def per_frame():
        prefix, _ = rd.get_frames_triplets(0, nz)
        return int(prefix[nz]), rd.last_batch_path

    def l2_call():
        got = 0
        for a in range(0, nz, batch):
            got += int(rd.get_frames_l2(a, min(batch, nz - a))[0][-1])
        return got, rd.last_batch_path

    def l2_iter():
        got = 0
        for item in rd.iter_frames_l2(0, nz, batch=batch):
            got += int(item[1][-1])
        return got, rd.last_batch_path
    methods = [("get_frames_triplets", per_frame), ("get_frames_l2", l2_call), ("iter_frames_l2", l2_iter)]
    for _, fn in methods:
        fn()                                    # warm: file cache, buffers, the library's workspaces
    rates = {name: [] for name, _ in methods}
    for r in range(reps):
        for name, fn in methods:
            t0 = time.perf_counter()
            nnz, path = fn()
            dt = time.perf_counter() - t0
            rates[name].append(nz / dt)
            print(json.dumps(dict(method=name, rep=r, frames=nz, batch=batch, seconds=round(dt, 5), frames_per_s=round(nz / dt, 1), set_pixels=nnz, path=path)))
    for name, _ in methods:
        v = rates[name]
        print(json.dumps(dict(method=name, median_frames_per_s=round(statistics.median(v), 1), min=round(min(v), 1), max=round(max(v), 1), reps=reps)))
    rd.close()
finally:
    shutil.rmtree(tmp, ignore_errors=True)
