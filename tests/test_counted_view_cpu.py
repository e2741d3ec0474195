"""Counted views on the CPU: the placement on a finer grid (pyrecode_amd/csrc/rc_count.h: cnt_place, cnt_finish_fine) as the C++ itself,
through tests/native/count_place_check.cpp - a stand-alone program, also under AddressSanitizer / UBSan - against 128-bit arithmetic; the
Python model (tests/counted_view_model.py) against the counting model it extends; and the new entry points' argument checks and loud
failure without a GPU."""
import os
import subprocess

import numpy as np
import pytest

import centroid_model as cm
import counted_view_model as cv
from conftest import REPO

SRC = os.path.join(REPO, "tests", "native", "count_place_check.cpp")


@pytest.mark.parametrize("build", ["plain", "sanitized"])
def test_placement_against_128_bit_arithmetic(tmp_path, build):
    """"sanitized": built with -fsanitize=address,undefined - skipped, and reported as skipped, where the toolchain has no sanitizer
    runtimes ("plain" still runs there)"""
    exe = tmp_path / "count_place_check"
    flags = []
    if build == "sanitized":
        flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
        probe = subprocess.run(["g++", "-x", "c++", "-", "-o", str(tmp_path / "probe")] + flags, input=b"int main(){return 0;}", capture_output=True)
        if probe.returncode != 0:
            pytest.skip("this toolchain cannot link -fsanitize=address,undefined: the sanitizer run did not take place")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-o", str(exe), SRC] + flags)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:] + r.stderr[-2000:]
    assert "seeded pairs" in r.stdout and "corners of the domain" in r.stdout and "s q odd and even" in r.stdout
    assert r.stdout.count(" 0 wrong") == 6
    seeded = [line for line in r.stdout.splitlines() if line.startswith("seeded pairs")][0]
    assert int(seeded.split()[2]) >= 10 ** 6


def test_place_at_upsample_1_is_the_counting_models_division():
    rng = np.random.default_rng(5)
    w = rng.integers(1, 1 << 40, 4000)
    S = (rng.random(4000) * 65535 * w).astype(np.int64)
    S[:500], w[:500] = np.arange(500) * 7 + 7, 14                     # ties among them
    want = cm.rhe(S, w)
    assert [cv.place(a, b, 1) for a, b in zip(S.tolist(), w.tolist())] == want.tolist()
    assert sum(cv.is_tie(a, b, 1) for a, b in zip(S.tolist(), w.tolist())) >= 250
    # by hand: 25 / 14 and 3 / 14 at upsample 4 (8.64, 2.36); 3 / 2 at 3 (5.5: the total's parity, not the inner quotient's)
    assert (cv.place(25, 14, 4), cv.place(3, 14, 4), cv.place(3, 2, 3), cv.place(1, 2, 3)) == (9, 2, 6, 2)
    # the centre of pixel x on a grid s times finer: cells s x .. s x + s - 1, the middle one (the even one of the middle two)
    for s in range(1, 17):
        for x in (0, 1, 6, 65534):
            k = cv.place(x, 1, s)
            assert s * x <= k <= s * x + s - 1 and abs(2 * k - (2 * s * x + s - 1)) <= 1 and (s % 2 == 1 or k % 2 == 0)


@pytest.mark.parametrize("method", cm.METHODS)
def test_counted_view_at_upsample_1_is_the_events_added_up(method):
    frames = [cm.bernoulli_frame(37, 45, 12, p, seed, zero_fraction=0.2) for seed, p in ((1, 0.05), (2, 0.3), (3, 0.6))]
    frames.append((np.ones((37, 45), bool), np.full((37, 45), 4095, np.uint16)))
    frames.append((np.zeros((37, 45), bool), np.zeros((37, 45), np.uint16)))
    for thr in (0, 2):
        _, rows, cols, _, _ = cm.count_batch(frames, method, thr)
        want = np.zeros((37, 45), np.uint64)
        np.add.at(want, (rows, cols), 1)
        got = cv.counted_view(frames, method, thr, 1)
        assert got.dtype == np.uint64 and np.array_equal(got, want) and int(got.sum()) == rows.size > 0


def test_a_domino_of_equal_values_is_a_tie_at_every_upsample():
    """a horizontal two-pixel component of equal values at columns x, x + 1: its centroid x + 1 / 2 is s x + s - 1 / 2 on the finer grid,
    half-way between two cell centres for every s - checked for 1..8, both averages, even and odd x"""
    for s in range(1, 9):
        for x in (0, 3, 4, 11):
            b, v = np.zeros((3, 16), bool), np.full((3, 16), 9, np.uint16)
            b[1, x:x + 2] = True
            for method in ("weighted_average", "unweighted_average"):
                comps, ties = cv.frame_components(b, v, method, 0), []
                w = 18 if method == "weighted_average" else 2
                assert comps == [(w, (2 * x + 1) * (w // 2), w)]
                view = cv.view_of([comps], (3, 16), s, ties)
                assert ties == [1] and int(view.sum()) == 1, (s, x, method)
                (k,) = np.flatnonzero(view.sum(0))
                assert k % 2 == 0 and abs(2 * k - (2 * s * x + 2 * s - 1)) == 1           # the even one of the two nearest


def test_grows_by_counted_restates_the_c_rule():
    from pyrecode_amd._lib import FrameSum
    sizes = np.array([[10, 3, 3], [10, 600, 600], [10, 0, 0]], np.uint32)
    # 5 x 7 pixels: 3 * 4 = 12 aligned 2 x 2 blocks; 12-bit fields: 2, 400 and 0 of them fit
    assert FrameSum.grows_by_counted((7, 5, 12, 1, 0, 0), sizes, 3) == 2 + 12 + 0
    assert FrameSum.grows_by_counted((7, 5, 12, 1, 0, 0), sizes, 2) == 2 + 12
    assert FrameSum.grows_by_counted((7, 5, 12, 3, 0, 0), sizes, 3) == 36
    assert FrameSum.grows_by_counted((7, 5, 12, 2, 0, 0), sizes, 3) == 36
    assert FrameSum.grows_by_counted((1, 1, 16, 1, 0, 0), sizes, 3) == 1 + 1 + 0


def _handle_stand_in():
    """memory the library may read as a handle: the checks that come before the device never look inside it"""
    return np.zeros(64, np.uint64)


def test_argument_checks_come_before_the_device():
    from pyrecode_amd import _lib
    L = _lib.lib()
    data, sizes, prefix, h = np.zeros(16, np.uint8), np.array([[1, 0, 0]], np.uint32), np.zeros(2, np.uint64), _handle_stand_in()
    p = _lib.ptr
    tail = (p(data), p(sizes), 1)
    for up in (0, 17):
        assert L.rc_sum_add_counted(p(h), 2, 2, up, 12, 1, 0, 0, *tail, 0, 0, p(prefix)) == _lib.RC_ERR_BAD_ARG
        assert L.rc_sum_add_counted_submit(p(h), 0, 2, 2, up, 12, 1, 0, 0, *tail, 0, 0) == _lib.RC_ERR_BAD_ARG
        assert "upsample" in _lib.last_error()
    assert L.rc_sum_add_counted(p(h), 2, 2, 1, 12, 1, 0, 0, *tail, 3, 0, p(prefix)) == _lib.RC_ERR_BAD_ARG
    assert L.rc_sum_add_counted_submit(p(h), 1, 2, 2, 1, 12, 1, 0, 0, *tail, 3, 0) == _lib.RC_ERR_BAD_ARG
    assert L.rc_sum_add_counted_submit(p(h), 2, 2, 2, 1, 12, 1, 0, 0, *tail, 0, 0) == _lib.RC_ERR_BAD_ARG
    assert "slot" in _lib.last_error()
    assert L.rc_sum_add_counted(None, 2, 2, 1, 12, 1, 0, 0, *tail, 0, 0, p(prefix)) == _lib.RC_ERR_BAD_ARG
    assert L.rc_sum_add_counted_submit(None, 0, 2, 2, 1, 12, 1, 0, 0, *tail, 0, 0) == _lib.RC_ERR_BAD_ARG
    assert L.rc_sum_add_counted(p(h), 2, 2, 1, 17, 1, 0, 0, *tail, 0, 0, p(prefix)) == _lib.RC_ERR_UNSUPPORTED
    assert L.rc_sum_add_counted(p(h), 70000, 2, 1, 12, 1, 0, 0, *tail, 0, 0, p(prefix)) == _lib.RC_ERR_BAD_ARG
    assert not h.any()


def test_python_side_argument_checks():
    from pyrecode_amd import reader_batched as rb
    for bad in (dict(upsample=0), dict(upsample=17), dict(area_threshold=-1), dict(area_threshold=1 << 32)):
        with pytest.raises(ValueError):
            rb._CountedAdder(**dict(dict(method="max", area_threshold=0, upsample=1), **bad))
    with pytest.raises(ValueError):
        rb._CountedAdder("median", 0, 1)
    assert rb._CountedAdder("max", 3, 4).view_shape(5, 7) == (20, 28) and rb._PlainAdder.view_shape(5, 7) == (5, 7)
    from pyrecode_amd.utils.viewer import ReCoDeViewer
    with pytest.raises(ValueError, match="unknown keys"):
        ReCoDeViewer("/nonexistent", "x.rc1", 1, 5, counting=dict(upsampling=2))


def test_no_gpu_means_loud_failure_not_fallback():
    from pyrecode_amd import _lib
    if _lib.device_count() > 0:
        pytest.skip("a GPU is visible")
    L = _lib.lib()
    data, sizes, prefix, h = np.zeros(16, np.uint8), np.array([[1, 0, 0]], np.uint32), np.zeros(2, np.uint64), _handle_stand_in()
    p = _lib.ptr
    assert L.rc_sum_add_counted(p(h), 2, 2, 2, 12, 3, 0, 0, p(data), p(sizes), 1, 0, 0, p(prefix)) == _lib.RC_ERR_DEVICE
    assert L.rc_sum_add_counted_submit(p(h), 0, 2, 2, 2, 12, 3, 0, 0, p(data), p(sizes), 1, 0, 0) == _lib.RC_ERR_DEVICE
    with pytest.raises(_lib.RecodeHipError):
        _lib.FrameSum(4, 4)
