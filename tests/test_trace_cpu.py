"""Frame traces on the CPU: the exact model (tests/trace_model.py) against a hand-written frame with literal expectations, the no-wrap rule of
pyrecode_amd/csrc/rc_trace.h as the C++ itself (tests/native/trace_bound_check.cpp - a stand-alone program, also under AddressSanitizer /
UBSan) against its restatement in Python integers, the entry points' argument checks that come before the device, centre_of_mass on
literals, and loud failure without a GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import REPO
from trace_model import LIMIT, batch_fits, frame_pixels, trace_model, weight_bounds

SRC = os.path.join(REPO, "tests", "native", "trace_bound_check.cpp")
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1


def test_model_on_a_hand_written_frame():
    """3 x 5, 5-bit values.  Frame 0 has pixels (0, 1) = 7, (1, 4) = 31, (2, 0) = 1, (2, 4) = 16 (the bytes are those of
    test_dense_plan_cpu.py::test_model_on_a_hand_written_frame); frame 1 is empty.  4 set pixels; 7 + 31 + 1 + 16 = 55; by row 0 * 7 + 1 * 31
    + 2 * 1 + 2 * 16 = 65; by column 1 * 7 + 4 * 31 + 0 * 1 + 4 * 16 = 195.  Planes: ones (55 again); 10 row + col - 7, which is -6, 7, 13, 17
    at the four pixels: -42 + 217 + 13 + 272 = 460; INT32_MIN at (1, 4) alone: 31 * -2^31.  At level 3 the same map with every value 1."""
    blob = np.array([0x02, 0x46, 0xE7, 0x07, 0x08, 0x00, 0x00], np.uint8)
    sizes = np.array([[2, 3, 3], [2, 0, 0]], np.uint32)
    ramp = (10 * np.arange(3)[:, None] + np.arange(5)[None, :] - 7).astype(np.int32)
    low = np.zeros((3, 5), np.int32)
    low[1, 4] = INT32_MIN
    planes = np.stack([np.ones((3, 5), np.int32), ramp, low])
    out, prefix = trace_model(blob, sizes, 3, 5, 5, 1)
    assert out.dtype == np.int64 and out.tolist() == [[4, 55, 65, 195], [0, 0, 0, 0]] and prefix.tolist() == [0, 4, 4]
    out, _ = trace_model(blob, sizes, 3, 5, 5, 1, planes)
    assert out.tolist() == [[4, 55, 65, 195, 55, 460, 31 * INT32_MIN], [0] * 7] and 31 * INT32_MIN == -66571993088
    out, _ = trace_model(blob, sizes, 3, 5, 5, 1, ramp)                 # (one plane, given as (ny, nx))
    assert out.tolist() == [[4, 55, 65, 195, 460], [0] * 5]
    blob3, sizes3 = np.array([0x02, 0x46, 0x00, 0x00], np.uint8), np.array([[2, 0, 0], [2, 0, 0]], np.uint32)
    out, prefix = trace_model(blob3, sizes3, 3, 5, 0, 3, planes)
    assert out.tolist() == [[4, 4, 5, 9, 4, -6 + 7 + 13 + 17, INT32_MIN], [0] * 7] and prefix.tolist() == [0, 4, 4]
    assert weight_bounds(planes) == [1, 17, 1 << 31]


def test_the_no_wrap_cases_of_the_gpu_test_lie_on_either_side_of_the_bound():
    """3 x 65535, 16 bits, one plane of INT32_MAX: a frame with every pixel set could reach 196605 * 65535 * (2^31 - 1), about 2.8e19, above
    2^63 - 1; a frame whose value stream has room for 10 set pixels at most 10 * 65535 * (2^31 - 1), about 1.4e15, below it"""
    assert 196605 * 65535 * INT32_MAX > LIMIT > 10 * 65535 * INT32_MAX
    assert not batch_fits(65535, 3, 1, 16, [INT32_MAX], [2 * 196605]) and batch_fits(65535, 3, 1, 16, [INT32_MAX], [20])
    assert not batch_fits(65535, 3, 1, 16, [INT32_MAX], [20, 2 * 196605, 20])              # (any frame of the batch)
    assert frame_pixels(65535, 3, 1, 16, 20) == 10 and frame_pixels(65535, 3, 1, 16, 1 << 30) == 196605


def _bound_cases():
    """(lines for the program, the answers of the Python restatement)"""
    lines, want = [], []

    def column(a, vmax, pixels):
        lines.append("c %d %d %d" % (a, vmax, pixels))
        want.append(str(int(a * vmax * pixels <= LIMIT)))

    def batch(nx, ny, level, d, bounds, packed):
        lines.append("f %d %d %d %d %d %d %s" % (nx, ny, level, d, len(bounds), len(packed), " ".join(str(v) for v in list(bounds) + list(packed))))
        want.append(str(int(batch_fits(nx, ny, level, d, bounds, packed))))
    # exactly at 2^63 - 1 = 7^2 * 73 * 127 * 337 * 92737 * 649657 and one past it, with the factors dealt out three ways
    for a, vmax in ((49 * 73 * 127 * 337, 92737), (649657, 49 * 73), (1, 1)):
        pixels = LIMIT // (a * vmax)
        assert a * vmax * pixels == LIMIT
        for extra in (0, 1):
            column(a, vmax, pixels + extra)
            column(a + extra, vmax, pixels)
            column(a, vmax + extra, pixels)
    column(1 << 31, 65535, 1 << 32)                              # (the largest product the entry points can meet: 2^79)
    column((1 << 64) - 1, (1 << 64) - 1, (1 << 64) - 1)
    for zero in ((0, 5, 5), (5, 0, 5), (5, 5, 0)):
        column(*zero)
    # INT32_MIN counts as 2^31; 8 bits: the last batch that fits has floor((2^63 - 1) / (2^31 * 255)) = 16843009 fields a frame
    edge = LIMIT // ((1 << 31) * 255)
    assert edge == 16843009
    for packed in (edge, edge + 1):
        batch(65535, 65535, 1, 8, [1 << 31], [packed])
        batch(65535, 65535, 1, 8, [3, 1 << 31, 0], [1, packed, 0])
    batch(65535, 65535, 1, 8, [INT32_MAX], [edge + 1])          # (2^31 - 1 is one less: this one still fits)
    # k = 0: the row and column weights alone.  65534 * 65535 * P fits up to P = 2147581955, a little above 2^31 - and a uint32 of packed
    # bytes has room for 2^31 - 1 sixteen-bit fields at most: without planes every batch fits
    edge = LIMIT // (65534 * 65535)
    assert edge == 2147581955 > 8 * 0xFFFFFFFF // 16
    column(65534, 65535, edge)
    column(65534, 65535, edge + 1)
    batch(65535, 65535, 1, 16, [], [0xFFFFFFFF])
    batch(65535, 65535, 1, 16, [], [0xFFFFFFFF, 0, 17])
    batch(65535, 65535, 3, 0, [], [0])
    batch(1, 1, 1, 16, [], [2])
    # P_f from a short value stream: the frame has 196605 pixels, the stream room for fewer
    batch(65535, 3, 1, 16, [INT32_MAX], [2 * 196605])
    batch(65535, 3, 1, 16, [INT32_MAX], [20])
    batch(65535, 3, 1, 12, [INT32_MAX], [3 * 65535 + 1])
    batch(65535, 3, 3, 0, [INT32_MAX], [0])
    rng = np.random.default_rng(77)

    def log_uniform(top):
        return min(top, int(2.0 ** rng.uniform(0, np.log2(top) + 0.5)))
    for _ in range(4000):
        level = int(rng.integers(1, 4))
        d = int(rng.integers(1, 17))
        bounds = [log_uniform(1 << 31) if rng.random() < 0.8 else int(rng.choice([0, 1, INT32_MAX, 1 << 31])) for _ in range(int(rng.integers(0, 17)))]
        packed = [log_uniform(0xFFFFFFFF) for _ in range(int(rng.integers(1, 5)))]
        batch(log_uniform(65535), log_uniform(65535), level, d, bounds, packed)
    # ... and 2000 aimed at the bound: the largest frames, a plane of 2^20 .. 2^31 and a value stream with room for about as many fields as
    # the plane admits - a few fields either way, or a few per cent
    for _ in range(2000):
        d = int(rng.integers(8, 17))
        a = int(2.0 ** rng.uniform(20, 31))
        room = LIMIT // (a * ((1 << d) - 1))
        fields = max(0, room + (int(rng.integers(-3, 4)) if rng.random() < 0.5 else int(room * rng.uniform(-0.05, 0.05))))
        packed = [min(0xFFFFFFFF, (fields * d + 7) // 8)] + [log_uniform(1 << 16) for _ in range(int(rng.integers(0, 3)))]
        batch(65535, 65535, 1, d, [log_uniform(1 << 20) for _ in range(int(rng.integers(0, 4)))] + [a], packed)
    for w in (0, 1, -1, INT32_MAX, INT32_MIN, INT32_MIN + 1, -65536):
        lines.append("a %d" % w)
        want.append(str(abs(w)))
    for case in ((130, 127, 1, 12, 100), (130, 127, 1, 12, 1 << 30), (130, 127, 2, 12, 7), (5, 3, 1, 5, 3), (65535, 65535, 1, 1, 0xFFFFFFFF)):
        lines.append("p %d %d %d %d %d" % case)
        want.append(str(frame_pixels(*case)))
    return lines, want


@pytest.mark.parametrize("build", ["plain", "sanitized"])
def test_bound_rule_against_python_integers(tmp_path, build):
    """"sanitized": built with -fsanitize=address,undefined - skipped, and reported as skipped, where the toolchain has no sanitizer
    runtimes ("plain" still runs there)"""
    exe = tmp_path / "trace_bound_check"
    flags = []
    if build == "sanitized":
        flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
        probe = subprocess.run(["g++", "-x", "c++", "-", "-o", str(tmp_path / "probe")] + flags, input=b"int main(){return 0;}", capture_output=True)
        if probe.returncode != 0:
            pytest.skip("this toolchain cannot link -fsanitize=address,undefined: the sanitizer run did not take place")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-o", str(exe), SRC] + flags)
    lines, want = _bound_cases()
    r = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    got = r.stdout.split()
    assert got[-1] == "ok" and len(got) == len(want) + 1
    wrong = [(line, g, w) for line, g, w in zip(lines, got, want) if g != w]
    assert not wrong, wrong[:5]
    answers = [w for line, w in zip(lines, want) if line[0] == "f"]
    assert len(answers) > 4000 and min(answers.count("0"), answers.count("1")) > 500          # (both answers are well represented)


def test_centre_of_mass_on_literals():
    from pyrecode_amd.reader_batched import centre_of_mass
    row, col = centre_of_mass({"sum": np.array([4, 0, 10], np.int64), "sum_row": np.array([6, 0, 25], np.int64), "sum_col": np.array([2, 0, 5], np.int64)})
    assert row.dtype == np.float64 and col.dtype == np.float64
    assert row[0] == 1.5 and col[0] == 0.5 and row[2] == 2.5 and col[2] == 0.5
    assert np.isnan(row[1]) and np.isnan(col[1])
    row, col = centre_of_mass({"sum": np.zeros(0, np.int64), "sum_row": np.zeros(0, np.int64), "sum_col": np.zeros(0, np.int64)})
    assert row.shape == (0,) and col.shape == (0,)


def _create(L, nx, ny, k, planes):
    st = C.c_int(12345)
    h = L.rc_trace_create(nx, ny, k, planes, C.byref(st))
    return h, st.value


def test_argument_checks_come_before_the_device():
    """what rc_trace_create refuses from its arguments alone, and what the two frame calls refuse without looking at a handle - on a machine
    with or without a GPU; with one, the checks that need a handle as well (tests/test_gpu_traces.py runs those in any case)"""
    from pyrecode_amd import _lib
    L, p = _lib.lib(), _lib.ptr
    bad = _lib.RC_ERR_BAD_ARG
    plane = np.ones((4, 8), np.int32)
    assert _create(L, 8, 4, 17, p(np.ones((17, 4, 8), np.int32))) == (None, bad) and "16" in _lib.last_error()
    assert _create(L, 0, 4, 0, None) == (None, bad) and _create(L, 8, 0, 0, None) == (None, bad)
    assert _create(L, 65536, 4, 0, None) == (None, bad) and _create(L, 8, 70000, 1, p(plane)) == (None, bad)
    assert _create(L, 8, 4, 1, None) == (None, bad) and "NULL" in _lib.last_error()
    assert L.rc_trace_create(0, 0, 0, None, None) is None                                   # (status may be NULL)
    assert L.rc_trace_destroy(None) == _lib.RC_OK and L.rc_trace_columns(None) == 0 and L.rc_trace_weight_bound(None, 0) == 0
    data, sizes, out = np.zeros(64, np.uint8), np.array([[4, 0, 0]], np.uint32), np.zeros(8, np.int64)
    assert L.rc_trace_frames(None, 12, 1, 0, 0, p(data), p(sizes), 1, p(out), 8, None) == bad
    assert L.rc_trace_frames_submit(None, 0, 12, 1, 0, 0, p(data), p(sizes), 1, p(out), 8) == bad
    assert L.rc_trace_frames_submit(None, 2, 12, 1, 0, 0, p(data), p(sizes), 1, p(out), 8) == bad and "slot" in _lib.last_error()
    for weights in (np.ones((4, 8), np.float32), np.ones((4, 9), np.int32), np.ones((17, 4, 8), np.int8), np.full((4, 8), 1 << 31, np.int64),
                    np.full((4, 8), INT32_MIN - 1, np.int64), np.full((4, 8), 1 << 31, np.uint32), [[1] * 8] * 4, np.ones((2, 1, 4, 8), np.int32)):
        with pytest.raises(ValueError):
            _lib.FrameTrace(8, 4, weights)
    h, st = _create(L, 8, 4, 1, p(plane))
    if _lib.device_count() == 0:
        assert (h, st) == (None, _lib.RC_ERR_DEVICE)
        return
    assert h and st == _lib.RC_OK and L.rc_trace_destroy(h) == _lib.RC_OK
    check_frame_call_arguments(_lib)


def check_frame_call_arguments(hip):
    """Every refusal of rc_trace_frames / _submit that is known from the arguments and the handle alone: nothing is queued and `out` keeps
    its fill.  Needs a handle, so a GPU."""
    L, p = hip.lib(), hip.ptr
    bad, uns, small = hip.RC_ERR_BAD_ARG, hip.RC_ERR_UNSUPPORTED, hip.RC_ERR_OUT_TOO_SMALL
    ft = hip.FrameTrace(8, 4, np.ones((2, 4, 8), np.int16))
    assert ft.columns == 6 == L.rc_trace_columns(ft.handle)
    data, sizes = np.zeros(64, np.uint8), np.array([[4, 0, 0], [4, 0, 0]], np.uint32)
    out = np.full(32, -0x5A5A5A5A5A5A5A5B, np.int64)

    def call(slot, d=12, level=1, mode=0, n=2, cells=12, data=data, sizes=sizes, dst=out):
        args = (d, level, mode, 0, p(data), p(sizes), n, p(dst) if isinstance(dst, np.ndarray) else dst, cells)
        return L.rc_trace_frames(ft.handle, *args, None) if slot is None else L.rc_trace_frames_submit(ft.handle, slot, *args)
    for slot in (None, 0, 1):
        assert call(slot, cells=11) == small and "4 + k" in hip.last_error()
        assert call(slot, n=1, cells=5) == small
        assert call(slot, d=20) == uns and "16" in hip.last_error()
        assert call(slot, d=17) == uns and call(slot, d=0) == bad
        assert call(slot, level=4) == uns and call(slot, level=0) == uns
        assert call(slot, n=0) == bad and call(slot, data=None) == bad and call(slot, sizes=None) == bad and call(slot, dst=None) == bad
        assert call(slot, dst=p(out) + 4) == bad and "aligned" in hip.last_error()
        assert call(slot, sizes=np.array([[4, 0, 0], [5, 0, 0]], np.uint32)) == bad and "geometry" in hip.last_error()
    assert call(2) == bad and "slot" in hip.last_error()
    ft.close()
    # the no-wrap refusal: 3 x 65535, 16 bits, one plane of INT32_MAX, a frame whose value stream has room for every pixel
    ft = hip.FrameTrace(65535, 3, np.full((3, 65535), INT32_MAX, np.int32))
    assert ft.weight_bounds() == [INT32_MAX]
    nb = (3 * 65535 + 7) // 8
    full = np.array([[nb, 2 * 196605, 2 * 196605]], np.uint32)
    for slot in (None, 1):
        args = (16, 1, 0, 0, p(data), p(full), 1, p(out), 5)
        st = L.rc_trace_frames(ft.handle, *args, None) if slot is None else L.rc_trace_frames_submit(ft.handle, slot, *args)
        assert st == small and "2^63" in hip.last_error()
    ft.close()
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
        _lib.FrameTrace(64, 64)
    rd = ReCoDeReader(os.path.join(GOLDEN, "files", "g3_l1z12.rc1"))
    rd.open(print_header=False)
    try:
        with pytest.raises(RuntimeError) as e:
            rd.get_frame_traces(0, 2)
        assert not isinstance(e.value, NotImplementedError)
        with pytest.raises(RuntimeError):
            next(rd.iter_frame_traces(batch=2))
    finally:
        rd.close()
