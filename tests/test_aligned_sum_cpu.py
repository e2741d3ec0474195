"""Aligned views on the CPU: the exact model (tests/aligned_sum_model.py) on literals, pyrecode_amd/csrc/rc_shift.h as the C++ itself
(tests/native/shift_window_check.cpp - a stand-alone program, also under AddressSanitizer / UBSan) against a loop over the pixels and
against its restatement in Python integers, the four entry points' argument checks that come before the device, the ValueErrors of
`shifts=` at the reader and the viewer, the viewer's id lookup, and loud failure without a GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import aligned_sum_model as am
from conftest import GOLDEN, REPO, load_npz

SRC = os.path.join(REPO, "tests", "native", "shift_window_check.cpp")
FILES = os.path.join(GOLDEN, "files")
INT32_MIN, INT32_MAX = am.INT32_MIN, am.INT32_MAX


def test_model_on_literals():
    """2 x 3 frames.  Frame 0 = [[1, 2, 3], [4, 5, 6]] one row down and one column left: row 0 of the source lands in row 1, columns 1..2 in
    columns 0..1 - [[0, 0, 0], [2, 3, 0]].  Frame 1 = all 7 shifted (0, 2): only column 0 survives, in column 2.  Frame 2 is out of the view
    in y, frame 3 carries the int32 extremes."""
    vals = np.array([[[1, 2, 3], [4, 5, 6]], [[7, 7, 7], [7, 7, 7]], [[9, 9, 9], [9, 9, 9]], [[9, 9, 9], [9, 9, 9]]], np.uint32)
    shifts = [(1, -1), (0, 2), (2, 0), (INT32_MAX, INT32_MIN)]
    assert am.shifted_sum(vals[:1], shifts[:1]).tolist() == [[0, 0, 0], [2, 3, 0]]
    assert am.shifted_sum(vals, shifts).tolist() == [[0, 0, 7], [2, 3, 7]]
    assert np.array_equal(am.shifted_sum(vals, [(0, 0)] * 4), vals.sum(0, dtype=np.uint64))
    # one pixel of value 5 at (1, 2): upsample 2 places its centre between fine cells 2, 3 (rows) and 4, 5 (columns), ties to the even one
    b = np.zeros((2, 3), bool)
    b[1, 2] = True
    v = np.full((2, 3), 5, np.uint16)
    assert np.argwhere(am.shifted_counted_view([(b, v)], [(0, 0)], s=2)).tolist() == [[2, 4]]
    assert np.argwhere(am.shifted_counted_view([(b, v)], [(1, -4)], s=2)).tolist() == [[3, 0]]
    assert not am.shifted_counted_view([(b, v)], [(2, 0)], s=2).any() and not am.shifted_counted_view([(b, v)], [(0, -5)], s=2).any()
    assert not am.shifted_counted_view([(b, v)], [(INT32_MIN, INT32_MAX)], s=2).any()
    both = am.shifted_counted_view([(b, v), (b, v)], [(-2, -4), (-2, -4)], s=2)
    assert int(both[0, 0]) == 2 and int(both.sum()) == 2


def test_restated_arithmetic_on_literals():
    assert am.shift_offset(-1, 3, 130) == -127 and am.shift_offset(INT32_MIN, INT32_MIN, 65535) == -(1 << 31) * 65536
    assert am.shift_funnel(0) == (0, 0) and am.shift_funnel(1) == (-1, 63) and am.shift_funnel(-1) == (0, 1)
    assert am.shift_funnel(64) == (-1, 0) and am.shift_funnel(65) == (-2, 63) and am.shift_funnel(-64) == (1, 0)
    assert am.shift_col_mask(0, 64, 0) == (1 << 64) - 1 and am.shift_col_mask(0, 64, 1) == (1 << 64) - 2
    assert am.shift_col_mask(0, 64, -1) == (1 << 63) - 1 and am.shift_col_mask(0, 64, 64) == 0
    assert am.shift_col_mask(0, 21, 1) == sum(1 << j for j in range(64) if j % 21 != 0)          # (three rows and a bit in one word)
    assert am.shift_col_mask(62, 130, -2) == ((1 << 64) - 1)           # columns 62 .. 125 all below 128
    assert am.shift_col_mask(126, 130, -2) == ((1 << 64) - 1) & ~0b1100  # columns 126, 127 stay; 128, 129 go; then row 2 from column 0
    assert am.shift_col_mask(126, 130, -2) & 0b1111 == 0b0011


@pytest.mark.parametrize("build", ["plain", "sanitized"])
def test_shift_header_against_a_pixel_loop_and_python_integers(tmp_path, build):
    """"sanitized": built with -fsanitize=address,undefined - skipped, and reported as skipped, where the toolchain has no sanitizer
    runtimes ("plain" still runs there).  The program itself compares the header with the per-pixel loop (its exit status); its table is
    compared here with the Python restatement, line for line."""
    exe = tmp_path / "shift_window_check"
    flags = []
    if build == "sanitized":
        flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
        probe = subprocess.run(["g++", "-x", "c++", "-", "-o", str(tmp_path / "probe")] + flags, input=b"int main(){return 0;}", capture_output=True)
        if probe.returncode != 0:
            pytest.skip("this toolchain cannot link -fsanitize=address,undefined: the sanitizer run did not take place")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-o", str(exe), SRC] + flags)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    got = r.stdout.splitlines()
    cases = am.shift_cases()
    assert got[-1] == "ok" and len(got) == len(cases) + 1
    want = [am.shift_table_line(*c) for c in cases]
    wrong = [(g, w) for g, w in zip(got, want) if g != w]
    assert not wrong, wrong[:5]
    assert len(cases) > 7000 and any(c[2] == INT32_MIN for c in cases) and any(c[3] == INT32_MAX for c in cases)
    survive = [line.split()[7] for line in got[:-1]]
    assert min(survive.count("0"), survive.count("1")) > 1000          # (both answers are well represented)


def test_argument_checks_come_before_the_device():
    """What the four entry points refuse from their arguments alone, with or without a GPU.  `fake` is zeroed memory in the place of a
    handle: the checks below read no more of it than its shape (0 x 0 - "a handle of the wrong shape" for any stored frame) and its device."""
    from pyrecode_amd import _lib
    L, p = _lib.lib(), _lib.ptr
    bad = _lib.RC_ERR_BAD_ARG
    fake_mem = (C.c_uint8 * 256)()
    fake = C.addressof(fake_mem)
    data, sizes, shifts = np.zeros(64, np.uint8), np.array([[4, 0, 0]], np.uint32), np.zeros((1, 2), np.int32)
    plain = (12, 1, 0, 0, p(data), p(sizes), 1)
    counted = lambda s=1, method=0: (8, 4, s, 12, 1, 0, 0, p(data), p(sizes), 1, method, 0)      # noqa: E731
    # NULL shifts
    assert L.rc_sum_add_frames_shifted(fake, *plain, None, None) == bad and "shifts" in _lib.last_error()
    assert L.rc_sum_add_frames_shifted_submit(fake, 0, *plain, None) == bad and "shifts" in _lib.last_error()
    assert L.rc_sum_add_counted_shifted(fake, *counted(), None, None) == bad and "shifts" in _lib.last_error()
    assert L.rc_sum_add_counted_shifted_submit(fake, 1, *counted(), None) == bad and "shifts" in _lib.last_error()
    # a slot above 1
    assert L.rc_sum_add_frames_shifted_submit(fake, 2, *plain, p(shifts)) == bad and "slot" in _lib.last_error()
    assert L.rc_sum_add_counted_shifted_submit(fake, 2, *counted(), p(shifts)) == bad and "slot" in _lib.last_error()
    # no handle, upsample 0 and 17, method 3
    assert L.rc_sum_add_frames_shifted(None, *plain, p(shifts), None) == bad
    assert L.rc_sum_add_counted_shifted(None, *counted(), p(shifts), None) == bad
    for s in (0, 17):
        assert L.rc_sum_add_counted_shifted(fake, *counted(s), p(shifts), None) == bad and "upsample" in _lib.last_error()
        assert L.rc_sum_add_counted_shifted_submit(fake, 0, *counted(s), p(shifts)) == bad and "upsample" in _lib.last_error()
    assert L.rc_sum_add_counted_shifted(fake, *counted(1, 3), p(shifts), None) == bad and "method" in _lib.last_error()
    assert L.rc_sum_add_counted_shifted_submit(fake, 0, *counted(1, 3), p(shifts)) == bad and "method" in _lib.last_error()
    # a handle of the wrong shape: stored frames of 4 map bytes into a view of 0 x 0
    assert L.rc_sum_add_frames_shifted(fake, *plain, p(shifts), None) == bad and "geometry" in _lib.last_error()
    assert L.rc_sum_add_frames_shifted_submit(fake, 0, *plain, p(shifts)) == bad and "geometry" in _lib.last_error()
    # bit depths as for the unshifted calls
    assert L.rc_sum_add_frames_shifted(fake, 20, 1, 0, 0, p(data), p(sizes), 1, p(shifts), None) == _lib.RC_ERR_UNSUPPORTED
    assert L.rc_sum_add_frames_shifted(fake, 0, 1, 0, 0, p(data), p(sizes), 1, p(shifts), None) == bad
    # ... and then the device: the counted call has passed every check that needs none
    if _lib.device_count() == 0:
        assert L.rc_sum_add_counted_shifted(fake, *counted(), p(shifts), None) == _lib.RC_ERR_DEVICE
        assert L.rc_sum_add_counted_shifted_submit(fake, 0, *counted(), p(shifts)) == _lib.RC_ERR_DEVICE
        empty = np.array([[0, 0, 0]], np.uint32)               # (a map of 0 bytes is the 0 x 0 view's own geometry)
        assert L.rc_sum_add_frames_shifted(fake, 12, 1, 0, 0, p(data), p(empty), 1, p(shifts), None) == _lib.RC_ERR_DEVICE
        assert L.rc_sum_add_frames_shifted_submit(fake, 0, 12, 1, 0, 0, p(data), p(empty), 1, p(shifts)) == _lib.RC_ERR_DEVICE
    else:
        assert L.rc_sum_add_counted_shifted(fake, *counted(), p(shifts), None) == bad and "shape" in _lib.last_error()


BAD_SHIFTS = [np.zeros((8, 2), np.float64), np.zeros((8, 2), np.float32), np.zeros((7, 2), np.int32), np.zeros((8, 3), np.int32), np.zeros(16, np.int32),
              np.array([[1 << 31, 0]] * 8, np.int64), np.array([[0, INT32_MIN - 1]] * 8, np.int64), np.full((8, 2), 1 << 31, np.uint32),
              np.zeros((8, 2), bool), [[0.5, 0]] * 8]


def test_shift_rows():
    from pyrecode_amd._lib import shift_rows
    got = shift_rows([[INT32_MIN, INT32_MAX], [0, -1]], 2)
    assert got.dtype == np.int32 and got.flags["C_CONTIGUOUS"] and got.tolist() == [[INT32_MIN, INT32_MAX], [0, -1]]
    assert shift_rows(np.array([[3, 4]], np.uint8)).tolist() == [[3, 4]] and shift_rows(np.zeros((0, 2), np.int64), 0).shape == (0, 2)
    assert shift_rows(np.arange(12, dtype=np.int64).reshape(6, 2)[::2], 3).tolist() == [[0, 1], [4, 5], [8, 9]]       # (a strided view is copied)
    for bad in BAD_SHIFTS:
        with pytest.raises(ValueError):
            shift_rows(bad, 8)


def test_reader_and_viewer_refuse_bad_shifts_before_the_device(tmp_path):
    from pyrecode_amd.recode_reader import ReCoDeReader
    from pyrecode_amd.utils.viewer import ReCoDeViewer
    rd = ReCoDeReader(os.path.join(FILES, "g3_l1z12.rc1"))
    rd.open(print_header=False)
    try:
        assert rd._batch_frames() == 8
        for bad in BAD_SHIFTS:
            with pytest.raises(ValueError):
                rd.sum_frames(shifts=bad)
            with pytest.raises(ValueError):
                rd.sum_frames_counted(upsample=2, shifts=bad)
            with pytest.raises(ValueError):
                next(rd.iter_frame_sums(4, shifts=bad))
            with pytest.raises(ValueError):
                next(rd.iter_frame_sums_counted(4, upsample=2, shifts=bad))
        with pytest.raises(ValueError):
            rd.sum_frames(2, 5, shifts=np.zeros((8, 2), np.int32))           # (one row per frame of the CALL)
    finally:
        rd.close()
    for bad in (np.zeros((20, 2), np.float64), np.zeros((20, 3), np.int32), np.zeros(40, np.int32), np.full((20, 2), 1 << 31, np.int64)):
        with pytest.raises(ValueError):
            ReCoDeViewer(str(tmp_path), "g7_stream.rc1", 2, 5, shifts=bad)


def test_viewer_id_lookup_on_g7s_ids():
    """the shift table is indexed by frame ID: each part's share of a window takes the rows of its ids, gaps and all"""
    from pyrecode_amd.utils.viewer import plan_view, shifts_for_ids
    g = load_npz("g7_stream.npz")
    ids = [g["ids_part0"], g["ids_part1"]]
    top = max(int(a.max()) for a in ids)
    table = np.stack([np.arange(top + 1) * 3 - 7, 100 - np.arange(top + 1)], 1).astype(np.int32)
    seen = []
    start = 0
    while True:
        plan = plan_view(ids, start, 5)
        if plan is None:
            break
        ranges, _, start = plan
        for part, (lo, hi) in zip(ids, ranges):
            rows = shifts_for_ids(table, part[lo:hi])
            assert rows.shape == (hi - lo, 2) and rows.tolist() == [[3 * int(i) - 7, 100 - int(i)] for i in part[lo:hi]]
            seen += part[lo:hi].tolist()
    assert sorted(seen) == sorted(np.concatenate(ids).tolist()) and len(seen) > 10
    assert shifts_for_ids(table, np.zeros(0, np.int64)).shape == (0, 2)
    with pytest.raises(ValueError, match="frame id %d" % top):
        shifts_for_ids(table[:top], ids[0] if top in ids[0] else ids[1])


def test_no_gpu_means_loud_failure_not_fallback():
    from pyrecode_amd import _lib
    from pyrecode_amd.recode_reader import ReCoDeReader
    if _lib.device_count() > 0:
        pytest.skip("a GPU is visible")
    rd = ReCoDeReader(os.path.join(FILES, "g3_l1z12.rc1"))
    rd.open(print_header=False)
    try:
        with pytest.raises(RuntimeError) as e:
            rd.sum_frames(shifts=np.zeros((8, 2), np.int32))
        assert not isinstance(e.value, (NotImplementedError, ValueError))
        with pytest.raises(RuntimeError):
            next(rd.iter_frame_sums_counted(4, upsample=2, shifts=np.zeros((8, 2), np.int64)))
    finally:
        rd.close()
