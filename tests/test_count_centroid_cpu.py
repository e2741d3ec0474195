"""Electron counting on the CPU: the arithmetic the kernels finish a component with (pyrecode_amd/csrc/rc_count.h: the round-half-even
division, the three methods, the weight-0 fallback) as the C++ itself, through tests/native/count_centroid_check.cpp - a stand-alone program,
also under AddressSanitizer / UBSan - against 128-bit arithmetic; and the new entry points' argument checks and loud failure without a GPU."""
import os
import subprocess

import numpy as np
import pytest

from conftest import REPO

SRC = os.path.join(REPO, "tests", "native", "count_centroid_check.cpp")


@pytest.mark.parametrize("build", ["plain", "sanitized"])
def test_division_and_finish_against_128_bit_arithmetic(tmp_path, build):
    """"sanitized": built with -fsanitize=address,undefined - skipped, and reported as skipped, where the toolchain has no sanitizer
    runtimes ("plain" still runs there)"""
    exe = tmp_path / "count_centroid_check"
    flags = []
    if build == "sanitized":
        flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
        probe = subprocess.run(["g++", "-x", "c++", "-", "-o", str(tmp_path / "probe")] + flags, input=b"int main(){return 0;}", capture_output=True)
        if probe.returncode != 0:
            pytest.skip("this toolchain cannot link -fsanitize=address,undefined: the sanitizer run did not take place")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-o", str(exe), SRC] + flags)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:] + r.stderr[-2000:]
    assert "seeded pairs" in r.stdout and " 0 wrong" in r.stdout


def test_the_python_model_divides_like_the_header():
    """the model's rhe (divmod) on the operands the C++ program's hand-written cases use"""
    import centroid_model as cm
    assert cm.rhe(np.array([25, 3, 7, 3, 3, 6, 5, 7]), np.array([14, 14, 5, 5, 3, 3, 2, 2])).tolist() == [2, 0, 1, 1, 1, 2, 2, 4]


def test_argument_checks_come_before_the_device():
    from pyrecode_amd import _lib
    L = _lib.lib()
    data, sizes, prefix = np.zeros(16, np.uint8), np.array([[1, 0, 0]], np.uint32), np.zeros(2, np.uint64)
    p = _lib.ptr
    assert L.rc_count_frames(2, 2, 12, 1, 0, 0, p(data), p(sizes), 1, 3, 0, p(prefix), None, 0) == _lib.RC_ERR_BAD_ARG
    assert L.rc_count_frames(2, 2, 17, 1, 0, 0, p(data), p(sizes), 1, 0, 0, p(prefix), None, 0) == _lib.RC_ERR_UNSUPPORTED
    assert L.rc_count_frames(70000, 2, 12, 1, 0, 0, p(data), p(sizes), 1, 0, 0, p(prefix), None, 0) == _lib.RC_ERR_BAD_ARG
    assert L.rc_count_frames_submit(2, 2, 2, 12, 1, 0, 0, p(data), p(sizes), 1, 0, 0, p(data), 1) == _lib.RC_ERR_BAD_ARG
    assert L.rc_count_frames_submit(0, 2, 2, 12, 1, 0, 0, p(data), p(sizes), 1, 0, 0, None, 1) == _lib.RC_ERR_BAD_ARG


def test_no_gpu_means_loud_failure_not_fallback():
    from pyrecode_amd import _lib
    from pyrecode_amd.utils import l1_to_l4_converter
    from scipy.sparse import coo_matrix
    if _lib.device_count() > 0:
        pytest.skip("a GPU is visible")
    L = _lib.lib()
    data, sizes, prefix = np.zeros(16, np.uint8), np.array([[1, 0, 0]], np.uint32), np.zeros(2, np.uint64)
    assert L.rc_count_frames(2, 2, 12, 3, 0, 0, _lib.ptr(data), _lib.ptr(sizes), 1, 0, 0, _lib.ptr(prefix), None, 0) == _lib.RC_ERR_DEVICE
    frames = {0: {'metadata': {'frame_id': 0}, 'data': coo_matrix(np.eye(4, dtype=np.uint16))}}
    with pytest.raises(RuntimeError):
        l1_to_l4_converter(frames, (4, 4))


def test_converter_refuses_what_it_cannot_count_exactly():
    from pyrecode_amd.utils import l1_to_l4_converter
    from scipy.sparse import coo_matrix
    for bad in (np.eye(4, dtype=np.int16), np.eye(4, dtype=np.float32), np.eye(4, dtype=np.uint32) * 70000):
        with pytest.raises(NotImplementedError):
            l1_to_l4_converter({0: {'data': coo_matrix(bad)}}, (4, 4))
    with pytest.raises(ValueError):
        l1_to_l4_converter({0: {'data': coo_matrix(np.eye(4, dtype=np.uint16))}}, (4, 4), method='median')
