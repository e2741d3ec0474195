"""Dense frame batches on the CPU: plan_sub_volume against numpy's own indexing, the numpy model of rc_expand_frames_dense against hand-written
literals, the region arithmetic of pyrecode_amd/csrc/rc_dense.h as the C++ itself (tests/native/dense_region_check.cpp - a stand-alone program,
also under AddressSanitizer / UBSan) against a double loop, and the new entry points' argument checks and loud failure without a GPU."""
import itertools
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, REPO

SRC = os.path.join(REPO, "tests", "native", "dense_region_check.cpp")
STARTS, STOPS, STEPS, INTS = (None, 0, 2, -3), (None, 4, -1, 100), (None, 1, 2, 3, -1, -2), (0, 3, -1)
AXIS_KEYS = [slice(a, b, c) for a in STARTS for b in STOPS for c in STEPS] + list(INTS)


def apply_plan(stack, plan):
    """what a reader does with a plan: take the indices walking forwards, flip, drop"""
    for axis, (start, count, step, flip, drop) in enumerate(plan):
        assert step > 0 and count >= 0 and (count == 0 or 0 <= start <= start + (count - 1) * step < stack.shape[axis])
        stack = np.take(stack, start + step * np.arange(count), axis=axis)
        if flip:
            stack = np.flip(stack, axis)
    return stack[tuple(0 if drop else slice(None) for _, _, _, _, drop in plan)]


def test_plan_sub_volume_is_numpy_indexing():
    """every combination, per axis, of start in {None, 0, 2, -3}, stop in {None, 4, -1, 100}, step in {None, 1, 2, 3, -1, -2} and the
    integers {0, 3, -1}: 99 keys an axis, 99^3 keys of an arange stack of shape (5, 7, 9) - the plan is per axis, so every axis is checked
    against every key alone and a seeded tenth of the triples together"""
    from pyrecode_amd.reader_batched import plan_sub_volume
    shape = (5, 7, 9)
    stack = np.arange(5 * 7 * 9).reshape(shape)
    full = slice(None)
    for axis in range(3):
        for k in AXIS_KEYS:
            key = tuple(k if a == axis else full for a in range(3))
            got = apply_plan(stack, plan_sub_volume(key, shape))
            assert got.shape == stack[key].shape and np.array_equal(got, stack[key]), key
    rng = np.random.default_rng(3)
    n = 0
    for key in itertools.product(AXIS_KEYS, repeat=3):
        if rng.random() < 0.1:
            got = apply_plan(stack, plan_sub_volume(key, shape))
            assert got.shape == stack[key].shape and np.array_equal(got, stack[key]), key
            n += 1
    assert n > 90000


def test_plan_sub_volume_refuses_what_numpy_refuses():
    from pyrecode_amd.reader_batched import plan_sub_volume
    full = slice(None)
    for bad in (5, -6, 100):
        with pytest.raises(IndexError):
            plan_sub_volume((bad, full, full), (5, 7, 9))
    with pytest.raises(IndexError):
        plan_sub_volume((full, 7, full), (5, 7, 9))
    with pytest.raises(IndexError):
        plan_sub_volume((full, full, -10), (5, 7, 9))
    with pytest.raises(IndexError):
        plan_sub_volume((full, full), (5, 7, 9))
    with pytest.raises(TypeError):
        plan_sub_volume((full, 1.5, full), (5, 7, 9))
    assert plan_sub_volume((np.int64(-1), full, full), (5, 7, 9))[0] == (4, 1, 1, False, True)
    assert plan_sub_volume((slice(None, None, -2), full, full), (5, 7, 9))[0] == (0, 3, 2, True, False)
    assert plan_sub_volume((slice(3, None, -2), full, full), (5, 7, 9))[0] == (1, 2, 2, True, False)


def test_model_on_a_hand_written_frame():
    """3 x 5, 5-bit values.  Frame 0 has pixels (0, 1) = 7, (1, 4) = 31, (2, 0) = 1, (2, 4) = 16: the map's bits 1, 9, 10, 14 - bytes
    0x02, 0x46 - and the fields 7, 31, 1, 16 LSB first: 7 | 31 << 5 | 1 << 10 | 16 << 15 = 0x0807E7 - bytes 0xE7, 0x07, 0x08.  Frame 1 is
    empty.  At level 3 the same map gives ones."""
    from dense_model import dense_model, unpack_fields
    blob = np.array([0x02, 0x46, 0xE7, 0x07, 0x08, 0x00, 0x00], np.uint8)
    sizes = np.array([[2, 3, 3], [2, 0, 0]], np.uint32)
    assert unpack_fields(blob[2:5], 4, 5).tolist() == [7, 31, 1, 16]
    out, prefix = dense_model(blob, sizes, 3, 5, 5, 1, (0, 0, 5, 3, 1, 1), np.uint8)
    assert out.dtype == np.uint8 and prefix.tolist() == [0, 4, 4]
    assert out.tolist() == [[[0, 7, 0, 0, 0], [0, 0, 0, 0, 31], [1, 0, 0, 0, 16]], [[0] * 5] * 3]
    out, _ = dense_model(blob, sizes, 3, 5, 5, 1, (0, 0, 3, 2, 2, 2), np.uint16)         # rows 0, 2; columns 0, 2, 4
    assert out.dtype == np.uint16 and out[0].tolist() == [[0, 0, 0], [1, 0, 16]]
    out, _ = dense_model(blob, sizes, 3, 5, 5, 1, (4, 1, 1, 2, 3, 1), np.uint8)          # column 4 of rows 1, 2
    assert out[0].tolist() == [[31], [16]]
    blob3, sizes3 = np.array([0x02, 0x46, 0x00, 0x00], np.uint8), np.array([[2, 0, 0], [2, 0, 0]], np.uint32)
    out, prefix = dense_model(blob3, sizes3, 3, 5, 0, 3, (1, 0, 4, 3, 1, 1), np.uint8)
    assert out[0].tolist() == [[1, 0, 0, 0], [0, 0, 0, 1], [0, 0, 0, 1]] and not out[1].any() and prefix.tolist() == [0, 4, 4]


@pytest.mark.parametrize("build", ["plain", "sanitized"])
def test_region_arithmetic_against_a_double_loop(tmp_path, build):
    """"sanitized": built with -fsanitize=address,undefined - skipped, and reported as skipped, where the toolchain has no sanitizer
    runtimes ("plain" still runs there)"""
    exe = tmp_path / "dense_region_check"
    flags = []
    if build == "sanitized":
        flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
        probe = subprocess.run(["g++", "-x", "c++", "-", "-o", str(tmp_path / "probe")] + flags, input=b"int main(){return 0;}", capture_output=True)
        if probe.returncode != 0:
            pytest.skip("this toolchain cannot link -fsanitize=address,undefined: the sanitizer run did not take place")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-o", str(exe), SRC] + flags)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.count(" 0 wrong") == 6 and "(2, 20000) seeded sample" in r.stdout and "(5, 65) all regions" in r.stdout


def _call(L, p, nx=8, ny=4, d=12, level=1, n=1, region=(0, 0, 8, 4, 1, 1), cell=2, out="own", cells=None, slot=None, data="own", sizes="own"):
    buf = np.zeros(4096, np.uint8)
    out = p(buf) if isinstance(out, str) else out
    data = p(np.zeros(64, np.uint8)) if isinstance(data, str) else data
    sizes = p(np.array([[4, 0, 0]] * max(n, 1), np.uint32)) if isinstance(sizes, str) else sizes
    cells = n * region[2] * region[3] if cells is None else cells
    args = (nx, ny, d, level, 0, 0, data, sizes, n) + tuple(region) + (cell, out, cells)
    return L.rc_expand_frames_dense(*args, None) if slot is None else L.rc_expand_frames_dense_submit(slot, *args)


@pytest.mark.parametrize("slot", [None, 0])
def test_argument_checks_come_before_the_device(slot):
    """every refusal that is known from the arguments alone, in both forms, on a machine with or without a GPU"""
    from pyrecode_amd import _lib
    L, p = _lib.lib(), _lib.ptr
    bad, uns, small = _lib.RC_ERR_BAD_ARG, _lib.RC_ERR_UNSUPPORTED, _lib.RC_ERR_OUT_TOO_SMALL
    assert _call(L, p, slot=slot, region=(0, 0, 8, 4, 0, 1)) == bad and "positive" in _lib.last_error()
    assert _call(L, p, slot=slot, region=(0, 0, 8, 4, 1, 0)) == bad
    assert _call(L, p, slot=slot, region=(0, 0, 0, 4, 1, 1), cells=32) == bad
    assert _call(L, p, slot=slot, region=(0, 0, 8, 0, 1, 1), cells=32) == bad
    assert _call(L, p, slot=slot, region=(1, 0, 8, 4, 1, 1)) == bad and "leaves the frame" in _lib.last_error()
    assert _call(L, p, slot=slot, region=(0, 1, 8, 4, 1, 1)) == bad
    assert _call(L, p, slot=slot, region=(2, 0, 4, 4, 2, 1)) == bad            # 2 + 3 * 2 = 8 = nx (1 + 3 * 2 = 7 is inside: below)
    assert _call(L, p, slot=slot, region=(0, 1, 8, 2, 1, 3)) == bad            # 1 + 1 * 3 = 4 = ny
    assert _call(L, p, slot=slot, region=(0, 0, 2, 1, 0xFFFFFFFF, 1)) == bad   # (no 32-bit wrap in the check)
    for cell in (0, 3, 8):
        assert _call(L, p, slot=slot, cell=cell) == bad
    assert _call(L, p, slot=slot, d=9, cell=1) == bad and _call(L, p, slot=slot, d=17, cell=2) == bad
    assert _call(L, p, slot=slot, d=33, cell=4) == uns and _call(L, p, slot=slot, d=40, cell=2) == uns
    assert _call(L, p, slot=slot, cells=31) == small and _call(L, p, slot=slot, n=3, cells=95) == small
    assert _call(L, p, slot=slot, out=None) == bad and _call(L, p, slot=slot, n=0, cells=32) == bad
    assert _call(L, p, slot=slot, data=None) == bad and _call(L, p, slot=slot, sizes=None) == bad
    assert _call(L, p, slot=slot, nx=70000, region=(0, 0, 8, 4, 1, 1)) == bad
    assert _call(L, p, slot=slot, level=4) == uns
    buf = np.zeros(64, np.uint8)
    assert _call(L, p, slot=slot, out=p(buf) + 1, cell=2) == bad and "aligned" in _lib.last_error()
    if slot is not None:
        assert _call(L, p, slot=2) == bad and "slot" in _lib.last_error()
        return
    # what the checks let through reaches the device: done there, or RC_ERR_DEVICE where there is none (the synchronous form only: a
    # submitted batch would stay queued, and its output must be page-locked)
    through = (_lib.RC_OK, _lib.RC_ERR_DEVICE)
    assert _call(L, p, region=(7, 3, 1, 1, 0xFFFFFFFF, 0xFFFFFFFF)) in through      # (a step larger than the frame: one cell)
    assert _call(L, p, region=(1, 0, 4, 4, 2, 1)) in through and _call(L, p, region=(0, 0, 8, 2, 1, 3)) in through
    assert _call(L, p, d=8, cell=1) in through and _call(L, p, d=32, cell=4) in through
    assert _call(L, p, d=33, level=3, cell=1) in through     # (the bit depth of a bitmap-only file is not a cell's)


def test_no_gpu_means_loud_failure_not_fallback():
    from pyrecode_amd import _lib
    from pyrecode_amd.recode_reader import ReCoDeReader
    if _lib.device_count() > 0:
        pytest.skip("a GPU is visible")
    L, p = _lib.lib(), _lib.ptr
    assert _call(L, p) == _lib.RC_ERR_DEVICE
    assert _call(L, p, slot=1) == _lib.RC_ERR_DEVICE
    assert _call(L, p, level=3, d=0, cell=1, region=(3, 1, 2, 2, 4, 2)) == _lib.RC_ERR_DEVICE
    rd = ReCoDeReader(os.path.join(GOLDEN, "files", "g3_l1z12.rc1"))
    rd.open(print_header=False)
    try:
        with pytest.raises(RuntimeError) as e:
            rd.get_sub_volume(slice(0, 2), slice(None), slice(None))
        assert not isinstance(e.value, NotImplementedError)
        with pytest.raises(RuntimeError):
            rd.get_frames_dense(0, 2, roi=(slice(1, 5), slice(None, None, 2)))
    finally:
        rd.close()
