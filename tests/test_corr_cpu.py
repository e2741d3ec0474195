"""Correlation surfaces on the CPU: the exact model (tests/corr_model.py) against a hand-written frame with literal expectations and its two
identities - the centre cell is the trace under the plane T, a smaller radius is the centre crop of a larger one -, estimate_shifts on
literals (unique peak, every tie-break rule, the all-zero surface, a peak on the border, the group sum, the wrap refusal, the parabola
against Fraction literals), the planted-drift property on the model alone, the index and workspace arithmetic of
pyrecode_amd/csrc/rc_corr.h as the C++ itself (tests/native/corr_index_check.cpp - a stand-alone program, also under AddressSanitizer /
UBSan) against its restatement in Python integers, the entry points' argument checks that come before the device, and loud failure
without a GPU."""
import ctypes as C
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import corr_model as cm
from conftest import REPO
from corr_model import corr_model, corr_of_frames, shifts_model
from trace_model import LIMIT, trace_model

SRC = os.path.join(REPO, "tests", "native", "corr_index_check.cpp")
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1
# 3 x 4, 5-bit values: frame 0 has pixels (0, 1) = 7 and (2, 3) = 31 - bits 1 and 11 of the map, the fields 7 | 31 << 5 = 0x3E7 -, frame 1 is empty
BLOB = np.array([0x02, 0x08, 0xE7, 0x03, 0x00, 0x00], np.uint8)
SIZES = np.array([[2, 2, 2], [2, 0, 0]], np.uint32)
T34 = np.array([[1, 2, 3, 4], [5, 6, 7, 8], [9, 10, 11, -12]], np.int32)


def test_model_on_a_hand_written_frame():
    """C[dy + 1][dx + 1] = 7 * T[0 + dy][1 + dx] + 31 * T[2 + dy][3 + dx], T outside the image 0.  dy = -1: the first pixel looks above the
    image, the second at T[1][2], T[1][3] and past the right edge: 217, 248, 0.  dy = 0: 7 * 1 + 31 * 11 = 348, 7 * 2 + 31 * -12 = -358,
    7 * 3 + 0 = 21.  dy = 1: the second pixel looks below the image: 35, 42, 49.  At level 3 the same map with every value 1."""
    out, prefix = corr_model(BLOB, SIZES, 3, 4, 5, 1, T34, 1)
    assert out.dtype == np.int64 and out.shape == (2, 3, 3) and prefix.tolist() == [0, 2, 2]
    assert out[0].tolist() == [[217, 248, 0], [348, -358, 21], [35, 42, 49]] and not out[1].any()
    out0, _ = corr_model(BLOB, SIZES, 3, 4, 5, 1, T34, 0)
    assert out0.tolist() == [[[-358]], [[0]]]
    blob3, sizes3 = np.array([0x02, 0x08, 0x00, 0x00], np.uint8), np.array([[2, 0, 0], [2, 0, 0]], np.uint32)
    out3, prefix = corr_model(blob3, sizes3, 3, 4, 0, 3, T34, 1)
    assert out3[0].tolist() == [[7, 8, 0], [1 + 11, 2 - 12, 3], [5, 6, 7]] and prefix.tolist() == [0, 2, 2]
    low = np.zeros((3, 4), np.int32)
    low[2, 3] = INT32_MIN
    assert corr_model(BLOB, SIZES, 3, 4, 5, 1, low, 1)[0][0, 1, 1] == 31 * INT32_MIN == -66571993088 and cm.reference_bound(low) == 1 << 31
    dense = np.zeros((1, 3, 4), np.int64)
    dense[0, 0, 1], dense[0, 2, 3] = 7, 31
    assert np.array_equal(corr_of_frames(dense, T34, 1), out[:1])


def test_the_two_identities():
    """on random frames of 13 x 17, 9 bits, a reference over the whole int32 range: the centre cell equals the traces' weighted column under
    W = T; the surface of radius 2 is the centre crop of radius 5's, which reaches past every edge of the image"""
    from test_gpu_frame_sums import _stored_batch          # (numpy only: the stored batches of the summed views' tests)
    rng = np.random.default_rng(1)
    ny, nx, d, n = 13, 17, 9, 4
    T = rng.integers(INT32_MIN, INT32_MAX + 1, (ny, nx), dtype=np.int64).astype(np.int32)
    vals = np.where(rng.random((n, ny, nx)) < 0.2, rng.integers(1, 1 << d, (n, ny, nx)), 0).astype(np.uint32)
    vals[2] = 0
    blob, sizes, _ = _stored_batch(vals, d, 1, rng)
    big, prefix = corr_model(blob, sizes, ny, nx, d, 1, T, 5)
    traces, counts = trace_model(blob, sizes, ny, nx, d, 1, T)
    assert np.array_equal(big[:, 5, 5], traces[:, 4]) and np.array_equal(prefix, counts) and big[0].all() and not big[2].any()
    small, _ = corr_model(blob, sizes, ny, nx, d, 1, T, 2)
    assert np.array_equal(small, big[:, 3:8, 3:8])
    assert np.array_equal(corr_model(blob, sizes, ny, nx, d, 1, T, 0)[0][:, 0, 0], traces[:, 4])
    assert np.array_equal(big, corr_of_frames(vals, T, 5))


def _es(corr, group=1):
    from pyrecode_amd.reader_batched import estimate_shifts
    got = estimate_shifts(np.asarray(corr, np.int64), group)
    assert sorted(got) == ["on_border", "peak", "refined", "shifts", "valid"]
    assert got["shifts"].dtype == np.int32 and got["peak"].dtype == np.int64 and got["on_border"].dtype == bool and got["valid"].dtype == bool
    assert got["refined"].dtype == np.float64
    want = shifts_model(np.asarray(corr, np.int64), group)
    assert got["shifts"].tolist() == [[w[0], w[1]] for w in want] and got["peak"].tolist() == [w[2] for w in want]
    assert got["on_border"].tolist() == [w[3] for w in want] and got["valid"].tolist() == [w[4] for w in want]
    assert got["refined"].tolist() == [[float(w[5]), float(w[6])] for w in want]
    return got


def test_estimate_shifts_on_literals():
    z = np.zeros((5, 5), np.int64)
    one = z.copy()
    one[1, 3], one[0, 3], one[2, 3], one[1, 2], one[1, 4] = 100, 40, 20, 70, 10       # a unique peak at (dy, dx) = (-1, 1)
    got = _es([one])
    assert got["shifts"].tolist() == [[-1, 1]] and got["peak"].tolist() == [100] and got["on_border"].tolist() == [False] and got["valid"].tolist() == [True]
    # the parabola: rows (40, 100, 20) -> (40 - 20) / (2 * (40 - 200 + 20)) = -1/14; columns (70, 100, 10) -> 60 / (2 * -120) = -1/4
    assert got["refined"].tolist() == [[float(Fraction(-1) + Fraction(-1, 14)), float(Fraction(1) + Fraction(-1, 4))]] == [[-15 / 14, 0.75]]
    # ties: the smallest dy^2 + dx^2 wins ...
    tie = z.copy()
    tie[0, 0] = tie[2, 3] = tie[4, 4] = 9
    assert _es([tie])["shifts"].tolist() == [[0, 1]]
    # ... then the smallest dy ((-1, 0), (0, -1), (0, 1), (1, 0) are equally far) ...
    tie = z.copy()
    tie[1, 2] = tie[2, 1] = tie[2, 3] = tie[3, 2] = 9
    assert _es([tie])["shifts"].tolist() == [[-1, 0]]
    tie[1, 2] = 0
    # ... then the smallest dx
    assert _es([tie])["shifts"].tolist() == [[0, -1]]
    tie = z.copy()
    tie[1, 1] = tie[1, 3] = tie[3, 1] = tie[3, 3] = 9
    assert _es([tie])["shifts"].tolist() == [[-1, -1]]
    # an all-zero surface: (0, 0), not valid, refined (0, 0) - the denominators are 0; an all-negative one: valid is False as well
    got = _es([z, z - 3])
    assert got["shifts"].tolist() == [[0, 0], [0, 0]] and got["valid"].tolist() == [False, False] and got["refined"].tolist() == [[0.0, 0.0]] * 2
    assert got["peak"].tolist() == [0, -3]
    # a peak on the border: flagged, no sub-pixel offset on either axis
    edge = z.copy()
    edge[4, 1], edge[4, 0], edge[4, 2] = 50, 30, 10
    got = _es([edge])
    assert got["shifts"].tolist() == [[2, -1]] and got["on_border"].tolist() == [True] and got["refined"].tolist() == [[2.0, -1.0]]
    corner = z.copy()
    corner[0, 0] = 1
    assert _es([corner])["shifts"].tolist() == [[-2, -2]]
    # groups: the surfaces of a run are summed - two frames that peak apart agree on a third cell; the last group is short
    a, b = z.copy(), z.copy()
    a[1, 1], a[2, 3] = 10, 8
    b[3, 3], b[2, 3] = 10, 8
    got = _es([a, b, one, a, b], group=2)
    assert got["shifts"].tolist() == [[0, 1], [0, 1], [-1, 1], [-1, 1], [1, 1]] and got["peak"].tolist() == [16, 16, 100, 100, 10]
    assert _es([a, b, one, a, b], group=1)["shifts"].tolist() == [[-1, -1], [1, 1], [-1, 1], [-1, -1], [1, 1]]
    assert _es([a, b, one, a, b], group=7)["peak"].tolist() == [100] * 5
    # a radius-0 surface: one cell, on the border by definition
    got = _es(np.array([[[5]], [[0]]]))
    assert got["shifts"].tolist() == [[0, 0], [0, 0]] and got["on_border"].tolist() == [True, True] and got["valid"].tolist() == [True, False]
    assert _es(np.zeros((0, 3, 3), np.int64))["shifts"].shape == (0, 2)


def test_estimate_shifts_refuses_a_sum_that_could_wrap():
    from pyrecode_amd.reader_batched import estimate_shifts
    big = np.zeros((2, 3, 3), np.int64)
    big[0, 1, 1] = LIMIT // 2 + 1
    with pytest.raises(ValueError, match="2\\^63"):
        estimate_shifts(big, group=2)
    with pytest.raises(ValueError):
        shifts_model(big, group=2)
    big[0, 1, 1] = LIMIT // 2
    assert estimate_shifts(big, group=2)["peak"].tolist() == [LIMIT // 2] * 2
    big[1, 0, 0] = -(LIMIT // 2) - 1
    with pytest.raises(ValueError):
        estimate_shifts(big, group=2)
    assert estimate_shifts(big, group=1)["peak"].tolist() == [LIMIT // 2, 0]
    assert estimate_shifts({"corr": big})["shifts"].tolist() == [[0, 0], [0, 0]]          # (the readers' dict is taken as it is)
    for bad in (np.zeros((2, 3, 4), np.int64), np.zeros((2, 4, 4), np.int64), np.zeros((3, 3), np.int64), np.zeros((2, 3, 3), np.float64)):
        with pytest.raises(ValueError):
            estimate_shifts(bad)
    with pytest.raises(ValueError):
        estimate_shifts(np.zeros((2, 3, 3), np.int64), group=0)


@pytest.mark.parametrize("ny,nx,R,density,d", [(127, 130, 3, 0.01, 12), (192, 256, 8, 0.01, 12), (64, 64, 8, 0.02, 0)])
def test_planted_drift_on_the_model(ny, nx, R, density, d):
    """A random sparse pattern with a margin of R clear at every edge, so nothing leaves the frame; frame f is the pattern rolled by a known
    s_f with |s_f| <= R - both corners of the window among them - and T is the pattern: the peak is unique (the pattern's energy, by
    Cauchy-Schwarz, met only where the frame lies on T) and estimate_shifts returns exactly -s_f."""
    from pyrecode_amd.reader_batched import estimate_shifts
    rng = np.random.default_rng(ny + R)
    pattern = np.zeros((ny, nx), np.int64)
    inner = (ny - 2 * R, nx - 2 * R)
    pattern[R:ny - R, R:nx - R] = np.where(rng.random(inner) < density, rng.integers(1, 1 << d, inner) if d else 1, 0)
    drifts = [(R, R), (-R, -R), (R, -R), (0, 0), (1, -2 if R > 1 else 0)] + [tuple(int(v) for v in rng.integers(-R, R + 1, 2)) for _ in range(3)]
    frames = np.stack([np.roll(pattern, s, (0, 1)) for s in drifts])
    assert all(fr.sum() == pattern.sum() for fr in frames)
    corr = corr_of_frames(frames, pattern, R)
    energy = int((pattern * pattern).sum())
    got = estimate_shifts(corr)
    assert got["shifts"].tolist() == [[-s[0], -s[1]] for s in drifts] and got["valid"].all() and got["peak"].tolist() == [energy] * len(drifts)
    assert [(c == energy).sum() for c in corr] == [1] * len(drifts)                       # (a unique peak)
    assert got["on_border"].tolist() == [abs(s[0]) == R or abs(s[1]) == R for s in drifts]


def _cases():
    """(lines for the program, the answers of the Python restatement)"""
    lines, want = [], []
    for R in range(17):
        lines.append("s %d" % R)
        want.append("%d %d %d" % (cm.side(R), cm.side(R) ** 2, cm.lane_cells(R)))
    assert want[8] == "17 289 5" and want[16] == "33 1089 18" and want[3] == "7 49 1" and want[0] == "1 1 1"
    rng = np.random.default_rng(5)
    geoms = [(1, 1, 0, 0, 0, 0), (1, 1, 16, 0, 0, 1088), (65535, 65535, 16, 65534, 65534, 1088), (65535, 65535, 16, 65534, 65534, 0),
             (4096, 4096, 8, 4095, 4095, 288), (21, 3, 3, 2, 20, 48)]
    for _ in range(2000):
        nx, ny, R = int(rng.integers(1, 65536)), int(rng.integers(1, 65536)), int(rng.integers(0, 17))
        geoms.append((nx, ny, R, int(rng.integers(0, ny)), int(rng.integers(0, nx)), int(rng.integers(0, cm.side(R) ** 2))))
    for nx, ny, R, row, col, cell in geoms:
        lines.append("g %d %d %d %d %d %d" % (nx, ny, R, row, col, cell))
        want.append("%d %d %d" % (cm.padded_cells(nx, ny, R), cm.window_base(row, col, nx, R), cm.cell_offset(cell, nx, R)))
        # the cell is inside the padded copy, and it is T[row + dy][col + dx]'s place: padded (row + dy + R, col + dx + R)
        dy, dx = cell // cm.side(R) - R, cell % cm.side(R) - R
        at = cm.window_base(row, col, nx, R) + cm.cell_offset(cell, nx, R)
        assert at < cm.padded_cells(nx, ny, R) and at == (row + dy + R) * (nx + 2 * R) + col + dx + R
    assert want[17 + 2].split()[0] == str(65567 * 65567) and int(want[17 + 2].split()[1]) + int(want[17 + 2].split()[2]) == 65567 * 65567 - 1
    works = [(1, 1, 0), (1, 64, 8), (262144, 64, 8), (262144, 64, 16), (262144, 1, 16), (262144, 4096, 8), (625, 2048, 3), (625, 4096, 3), (67092481, 1, 16)]
    for _ in range(2000):
        works.append((int(2.0 ** rng.uniform(0, 26)), int(2.0 ** rng.uniform(0, 13)), int(rng.integers(0, 17))))
    for nb8, n, R in works:
        lines.append("w %d %d %d" % (nb8, n, R))
        bpc, nchunk = cm.chunks(-(-nb8 // 256), n)
        want.append("%d %d %d" % (bpc, nchunk, cm.workspace_bytes(nb8, n, R)))
        nblk = -(-nb8 // 256)
        assert (nchunk - 1) * bpc < nblk <= nchunk * bpc and nchunk <= -(-4096 // n)          # every block is walked, by no more workgroups than aimed for
        assert cm.workspace_bytes(nb8, n, R) <= (n + 4096) * cm.side(R) ** 2 * 8
    # 64 frames of 4096 x 4096: 1024 blocks a frame in 64 chunks of 16 - 9.5 MB of partial rows at R = 8, 35.7 MB at R = 16
    assert want[17 + len(geoms) + 2] == "16 64 %d" % (64 * 64 * 289 * 8) and want[17 + len(geoms) + 3] == "16 64 %d" % (64 * 64 * 1089 * 8)
    assert want[17 + len(geoms) + 6] == "2 2 %d" % (2048 * 2 * 49 * 8) and want[17 + len(geoms) + 7] == "3 1 %d" % (4096 * 49 * 8)
    for nx, ny, level, d, bound, packed in [(65535, 3, 1, 16, INT32_MAX, [2 * 196605]), (65535, 3, 1, 16, INT32_MAX, [20]), (65535, 3, 1, 16, INT32_MAX, [20, 2 * 196605]),
                                            (65535, 65535, 1, 8, 1 << 31, [16843009]), (65535, 65535, 1, 8, 1 << 31, [16843010]), (65535, 65535, 3, 0, 1 << 31, [0]),
                                            (65535, 65535, 1, 16, 0, [0xFFFFFFFF]), (4096, 4096, 1, 12, 4095 * 64, [1 << 25])]:
        lines.append("b %d %d %d %d %d %d %s" % (nx, ny, level, d, bound, len(packed), " ".join(str(b) for b in packed)))
        want.append(str(int(cm.batch_fits(nx, ny, level, d, bound, packed))))
    assert want[-8:] == ["0", "1", "0", "1", "0", "1", "1", "1"]
    return lines, want


@pytest.mark.parametrize("build", ["plain", "sanitized"])
def test_index_arithmetic_against_python_integers(tmp_path, build):
    """"sanitized": built with -fsanitize=address,undefined - skipped, and reported as skipped, where the toolchain has no sanitizer
    runtimes ("plain" still runs there)"""
    exe = tmp_path / "corr_index_check"
    flags = []
    if build == "sanitized":
        flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
        probe = subprocess.run(["g++", "-x", "c++", "-", "-o", str(tmp_path / "probe")] + flags, input=b"int main(){return 0;}", capture_output=True)
        if probe.returncode != 0:
            pytest.skip("this toolchain cannot link -fsanitize=address,undefined: the sanitizer run did not take place")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-o", str(exe), SRC] + flags)
    lines, want = _cases()
    r = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    got = r.stdout.strip().split("\n")
    assert got[-1] == "ok" and len(got) == len(want) + 1
    wrong = [(line, g, w) for line, g, w in zip(lines, got, want) if g != w]
    assert not wrong, wrong[:5]


def _create(L, nx, ny, radius, reference):
    st = C.c_int(12345)
    h = L.rc_corr_create(nx, ny, radius, reference, C.byref(st))
    return h, st.value


def test_argument_checks_come_before_the_device():
    """what rc_corr_create refuses from its arguments alone, and what the two frame calls refuse without looking at a handle - on a machine
    with or without a GPU; with one, the checks that need a handle as well (tests/test_gpu_corr.py runs those in any case)"""
    from pyrecode_amd import _lib
    L, p = _lib.lib(), _lib.ptr
    bad = _lib.RC_ERR_BAD_ARG
    ref = np.ones((4, 8), np.int32)
    assert _create(L, 8, 4, 17, p(ref)) == (None, bad) and "16" in _lib.last_error()
    assert _create(L, 0, 4, 1, p(ref)) == (None, bad) and _create(L, 8, 0, 1, p(ref)) == (None, bad)
    assert _create(L, 65536, 4, 1, p(ref)) == (None, bad) and _create(L, 8, 70000, 1, p(ref)) == (None, bad)
    assert _create(L, 8, 4, 1, None) == (None, bad) and "NULL" in _lib.last_error()
    assert L.rc_corr_create(0, 0, 0, None, None) is None                                    # (status may be NULL)
    assert L.rc_corr_destroy(None) == _lib.RC_OK and L.rc_corr_side(None) == 0 and L.rc_corr_reference_bound(None) == 0
    data, sizes, out = np.zeros(64, np.uint8), np.array([[4, 0, 0]], np.uint32), np.zeros(9, np.int64)
    assert L.rc_corr_frames(None, 12, 1, 0, 0, p(data), p(sizes), 1, p(out), 9, None) == bad
    assert L.rc_corr_frames_submit(None, 0, 12, 1, 0, 0, p(data), p(sizes), 1, p(out), 9) == bad
    assert L.rc_corr_frames_submit(None, 2, 12, 1, 0, 0, p(data), p(sizes), 1, p(out), 9) == bad and "slot" in _lib.last_error()
    for reference in (np.ones((4, 8), np.float32), np.ones((4, 9), np.int32), np.ones((2, 4, 8), np.int8), np.full((4, 8), 1 << 31, np.int64),
                      np.full((4, 8), INT32_MIN - 1, np.int64), np.full((4, 8), 1 << 31, np.uint32), [[1] * 8] * 4, None):
        with pytest.raises(ValueError):
            _lib.FrameCorrelation(8, 4, reference)
    for radius in (-1, 17):
        with pytest.raises(ValueError, match="radius"):
            _lib.FrameCorrelation(8, 4, ref, radius)
    h, st = _create(L, 8, 4, 1, p(ref))
    if _lib.device_count() == 0:
        assert (h, st) == (None, _lib.RC_ERR_DEVICE)
        return
    assert h and st == _lib.RC_OK and L.rc_corr_side(h) == 3 and L.rc_corr_reference_bound(h) == 1 and L.rc_corr_destroy(h) == _lib.RC_OK
    check_frame_call_arguments(_lib)


def check_frame_call_arguments(hip):
    """Every refusal of rc_corr_frames / _submit that is known from the arguments and the handle alone: nothing is queued and `out` keeps
    its fill.  Needs a handle, so a GPU."""
    L, p = hip.lib(), hip.ptr
    bad, uns, small = hip.RC_ERR_BAD_ARG, hip.RC_ERR_UNSUPPORTED, hip.RC_ERR_OUT_TOO_SMALL
    fc = hip.FrameCorrelation(8, 4, np.ones((4, 8), np.int16), 1)
    assert fc.side == 3 == L.rc_corr_side(fc.handle) and fc.radius == 1 and fc.reference_bound() == 1
    data, sizes = np.zeros(64, np.uint8), np.array([[4, 0, 0], [4, 0, 0]], np.uint32)
    out = np.full(32, -0x5A5A5A5A5A5A5A5B, np.int64)

    def call(slot, d=12, level=1, mode=0, n=2, cells=18, data=data, sizes=sizes, dst=out):
        args = (d, level, mode, 0, p(data), p(sizes), n, p(dst) if isinstance(dst, np.ndarray) else dst, cells)
        return L.rc_corr_frames(fc.handle, *args, None) if slot is None else L.rc_corr_frames_submit(fc.handle, slot, *args)
    for slot in (None, 0, 1):
        assert call(slot, cells=17) == small and "(2 R + 1)^2" in hip.last_error()
        assert call(slot, n=1, cells=8) == small
        assert call(slot, d=20) == uns and "16" in hip.last_error()
        assert call(slot, d=17) == uns and call(slot, d=0) == bad
        assert call(slot, level=4) == uns and call(slot, level=0) == uns
        assert call(slot, n=0) == bad and call(slot, data=None) == bad and call(slot, sizes=None) == bad and call(slot, dst=None) == bad
        assert call(slot, dst=p(out) + 4) == bad and "aligned" in hip.last_error()
        assert call(slot, sizes=np.array([[4, 0, 0], [5, 0, 0]], np.uint32)) == bad and "geometry" in hip.last_error()
    assert call(2) == bad and "slot" in hip.last_error()
    fc.close()
    # the no-wrap refusal: 3 x 65535, 16 bits, a reference of INT32_MAX, a frame whose value stream has room for every pixel
    fc = hip.FrameCorrelation(65535, 3, np.full((3, 65535), INT32_MAX, np.int32), 0)
    assert fc.reference_bound() == INT32_MAX
    nb = (3 * 65535 + 7) // 8
    full = np.array([[nb, 2 * 196605, 2 * 196605]], np.uint32)
    for slot in (None, 1):
        args = (16, 1, 0, 0, p(data), p(full), 1, p(out), 1)
        st = L.rc_corr_frames(fc.handle, *args, None) if slot is None else L.rc_corr_frames_submit(fc.handle, slot, *args)
        assert st == small and "2^63" in hip.last_error()
    fc.close()
    assert (out == -0x5A5A5A5A5A5A5A5B).all()
    for slot in (0, 1):      # nothing was queued by any of the refusals
        assert L.rc_expand_frames_wait(slot, p(np.zeros(4, np.uint64))) == bad


def test_no_gpu_means_loud_failure_not_fallback():
    from pyrecode_amd import _lib
    from pyrecode_amd.recode_reader import ReCoDeReader
    from conftest import GOLDEN
    if _lib.device_count() > 0:
        pytest.skip("a GPU is visible")
    with pytest.raises(_lib.RecodeHipError, match="no CPU path"):
        _lib.FrameCorrelation(64, 64, np.ones((64, 64), np.int32))
    rd = ReCoDeReader(os.path.join(GOLDEN, "files", "g3_l1z12.rc1"))
    rd.open(print_header=False)
    try:
        ref = np.ones((int(rd._header["ny"]), int(rd._header["nx"])), np.int32)
        with pytest.raises(RuntimeError) as e:
            rd.get_frame_correlations(0, 2, ref)
        assert not isinstance(e.value, NotImplementedError)
        with pytest.raises(RuntimeError):
            next(rd.iter_frame_correlations(batch=2, reference=ref))
    finally:
        rd.close()
