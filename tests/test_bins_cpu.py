"""Binned frame traces on the CPU: the exact model (tests/bins_model.py) against a hand-written frame with literal expectations and its two
identities - over the bins, plane 0 plus the ignored pixels is the trace's count and plane 1 the trace's sum; for B <= 16 plane 1 is the
trace's weighted columns under the one-hot planes -, radial_labels against a pixel loop with math.isqrt (an integer centre, a half centre),
bin_areas, the chunking and workspace arithmetic of pyrecode_amd/csrc/rc_bins.h as the C++ itself (tests/native/bins_index_check.cpp - a
stand-alone program, also under AddressSanitizer / UBSan) against its restatement in Python integers, the entry points' argument checks
that come before the device, and loud failure without a GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bins_model as bm
from bins_model import IGNORE, bins_model, bins_of_frames, one_hot_planes
from conftest import REPO
from trace_model import trace_model

SRC = os.path.join(REPO, "tests", "native", "bins_index_check.cpp")
# 3 x 4, 5-bit values: frame 0 has pixels (0, 1) = 7, (1, 2) = 3 and (2, 3) = 31 - bits 1, 6 and 11 of the map, the fields 7 | 3 << 5 | 31 << 10 =
# 0x7C67 -, frame 1 is empty
BLOB = np.array([0x42, 0x08, 0x67, 0x7C, 0x00, 0x00], np.uint8)
SIZES = np.array([[2, 2, 2], [2, 0, 0]], np.uint32)
LAB34 = np.array([[0, 2, 2, 1], [1, 1, IGNORE, 0], [IGNORE, 0, 0, 2]], np.uint16)


def test_model_on_a_hand_written_frame():
    """(0, 1) = 7 lies in bin 2, (1, 2) = 3 in no bin, (2, 3) = 31 in bin 2: counts [0, 0, 2], sums [0, 0, 38].  With bin 2 moved to bin 0
    for the last pixel: counts [1, 0, 1], sums [31, 0, 7].  At level 3 the same map with every value 1: the sums are the counts."""
    out, prefix = bins_model(BLOB, SIZES, 3, 4, 5, 1, LAB34, 3)
    assert out.dtype == np.int64 and out.shape == (2, 2, 3) and prefix.tolist() == [0, 3, 3]
    assert out[0].tolist() == [[0, 0, 2], [0, 0, 38]] and not out[1].any()
    lab = LAB34.copy()
    lab[2, 3] = 0
    assert bins_model(BLOB, SIZES, 3, 4, 5, 1, lab, 3)[0][0].tolist() == [[1, 0, 1], [31, 0, 7]]
    assert bins_model(BLOB, SIZES, 3, 4, 5, 1, lab, 5)[0][0].tolist() == [[1, 0, 1, 0, 0], [31, 0, 7, 0, 0]]      # (bins nobody is in)
    lab[:] = 0
    assert bins_model(BLOB, SIZES, 3, 4, 5, 1, lab, 1)[0].tolist() == [[[3], [41]], [[0], [0]]]                    # (one bin: the trace's count and sum)
    lab[:] = IGNORE
    assert not bins_model(BLOB, SIZES, 3, 4, 5, 1, lab, 2)[0].any()
    blob3, sizes3 = np.array([0x42, 0x08, 0x00, 0x00], np.uint8), np.array([[2, 0, 0], [2, 0, 0]], np.uint32)
    out3, prefix = bins_model(blob3, sizes3, 3, 4, 0, 3, LAB34, 3)
    assert out3[0].tolist() == [[0, 0, 2], [0, 0, 2]] and prefix.tolist() == [0, 3, 3]
    with pytest.raises(AssertionError):
        bins_model(BLOB, SIZES, 3, 4, 5, 1, LAB34, 2)                                                              # (a label of 2 with two bins)
    dense = np.zeros((2, 3, 4), np.int64)
    dense[0, 0, 1], dense[0, 1, 2], dense[0, 2, 3] = 7, 3, 31
    assert np.array_equal(bins_of_frames(dense, LAB34, 3), out)


@pytest.mark.parametrize("level,d", [(1, 9), (1, 16), (3, 0), (2, 12)])
def test_the_two_identities(level, d):
    """on random frames of 13 x 17 and random labels with a fifth of the pixels in no bin.  (1) For B = 40: summed over the bins, plane 0
    plus the set pixels under the ignore label is the trace's count, plane 1 plus their values its sum - both read off the traces under
    the plane labels == 0xFFFF.  (2) For B = 16 plane 1 is the traces' 16 weighted columns under the one-hot planes, and plane 0 the same
    at level 3 (every value 1)."""
    from test_gpu_frame_sums import _stored_batch          # (numpy only: the stored batches of the summed views' tests)
    rng = np.random.default_rng(1)
    ny, nx, n = 13, 17, 4
    top = (1 << d) - 1 if level == 1 else 1
    vals = np.where(rng.random((n, ny, nx)) < 0.3, rng.integers(1, top + 1, (n, ny, nx)) if level == 1 else 1, 0).astype(np.uint32)
    vals[2] = 0
    blob, sizes, _ = _stored_batch(vals, d, level, rng)
    for B in (40, 16):
        labels = np.where(rng.random((ny, nx)) < 0.2, IGNORE, rng.integers(0, B, (ny, nx))).astype(np.uint16)
        out, prefix = bins_model(blob, sizes, ny, nx, d, level, labels, B)
        ignored = (labels == IGNORE).astype(np.int32)
        traces, counts = trace_model(blob, sizes, ny, nx, d, level, ignored[None])
        assert np.array_equal(prefix, counts) and out[0].any() and not out[2].any()
        assert np.array_equal(out[:, 1].sum(1) + traces[:, 4], traces[:, 1])
        ones, _ = trace_model(blob, sizes, ny, nx, 0, 3, ignored[None])                  # (the map alone, every value 1: the ignored PIXELS)
        assert np.array_equal(out[:, 0].sum(1) + ones[:, 4], traces[:, 0])
        if B == 16:
            hot, _ = trace_model(blob, sizes, ny, nx, d, level, one_hot_planes(labels, B))
            assert np.array_equal(out[:, 1], hot[:, 4:])
            assert np.array_equal(out[:, 0], trace_model(blob, sizes, ny, nx, 0, 3, one_hot_planes(labels, B))[0][:, 4:])
        assert np.array_equal(out, bins_of_frames(vals, labels, B))


@pytest.mark.parametrize("ny,nx,cy,cx,w", [(9, 12, 4, 5, 1), (9, 12, 3.5, 6.5, 1), (33, 40, 16, 19.5, 3), (7, 5, 0, 0, 2), (6, 6, -0.5, 8.5, 1), (1, 1, 0, 0, 1)])
def test_radial_labels_against_a_pixel_loop(ny, nx, cy, cx, w):
    from pyrecode_amd.reader_batched import bin_areas, radial_labels
    got = radial_labels(ny, nx, cy, cx, w)
    full = bm.radial_model(ny, nx, int(2 * cy), int(2 * cx), w, 4096)
    assert got.dtype == np.uint16 and got.shape == (ny, nx) and np.array_equal(got, full) and not (got == IGNORE).any()
    B = int(full.max()) + 1
    for keep in {1, max(1, B // 2), B, B + 3}:
        cut = radial_labels(ny, nx, cy, cx, w, n_bins=keep)
        assert np.array_equal(cut, bm.radial_model(ny, nx, int(2 * cy), int(2 * cx), w, keep))
        assert ((cut == IGNORE) == (full >= keep)).all()
        areas = bin_areas(cut, keep)
        assert areas.dtype == np.int64 and areas.tolist() == [int((full == b).sum()) for b in range(keep)]


def test_radial_labels_literals_and_refusals():
    from pyrecode_amd.reader_batched import radial_labels
    # an integer centre: distances 0, 1, sqrt 2 -> 1, 2, sqrt 5 -> 2, sqrt 8 -> 2
    assert radial_labels(3, 3, 0, 0).tolist() == [[0, 1, 2], [1, 1, 2], [2, 2, 2]]
    # a half centre: every pixel of a 2 x 2 frame is sqrt(1/2) away; of a 4 x 4 frame the corners 3 / sqrt 2 = 2.12
    assert radial_labels(2, 2, 0.5, 0.5).tolist() == [[0, 0], [0, 0]]
    assert radial_labels(4, 4, 1.5, 1.5).tolist() == [[2, 1, 1, 2], [1, 0, 0, 1], [1, 0, 0, 1], [2, 1, 1, 2]]
    assert radial_labels(1, 5, 0, 0, 2).tolist() == [[0, 0, 1, 1, 2]] and radial_labels(1, 5, 0, 0, 2, n_bins=2).tolist() == [[0, 0, 1, 1, IGNORE]]
    # the largest frame: the corner of 65535 x 2 from its other end, in exact integers
    far = radial_labels(2, 65535, 0, 0, 16)
    assert int(far[1, 65534]) == 65534 // 16 and far.max() == 4095
    for bad in ((3, 3, 0.25, 0), (3, 3, 0, 1.1), (0, 3, 0, 0), (3, 3, 0, 0, 0), (3, 3, 0, 0, 1.5), (3, 3, 0, 0, 1, 0), (3, 3, 0, 0, 1, 4097), (2, 65535, 0, 0, 1)):
        with pytest.raises(ValueError):
            radial_labels(*bad)


def test_bin_areas():
    from pyrecode_amd.reader_batched import bin_areas
    assert bin_areas(LAB34, 3).tolist() == [4, 3, 3] and bin_areas(LAB34, 5).tolist() == [4, 3, 3, 0, 0]
    assert bin_areas(LAB34, 2).tolist() == [4, 3]                    # (labels at or above n_bins are in no bin)
    assert bin_areas(LAB34.astype(np.int64), 3).tolist() == [4, 3, 3] and bin_areas(np.full((2, 2), IGNORE, np.uint16), 1).tolist() == [0]
    assert bin_areas(np.array([[-1, 0]]), 1).tolist() == [1]
    with pytest.raises(ValueError):
        bin_areas(LAB34.astype(np.float32), 3)


def _cases():
    """(lines for the program, the answers of the Python restatement)"""
    lines, want = [], []
    for B in (1, 2, 16, 17, 255, 256, 257, 512, 513, 1024, 1025, 2896, 4095, 4096):
        for level in (1, 2, 3):
            lines.append("t %d %d" % (B, level))
            want.append("%d %d %d" % (bm.tier(B), bm.lds_bytes(B, level), bm.target_wgs(B)))
            assert bm.target_wgs(B) * 16 * B <= bm.PARTIAL_BUDGET and 512 <= bm.target_wgs(B) <= 4096
    assert want[0] == "256 3072 4096" and want[1] == "256 1024 4096" and want[-3] == "4096 49152 512" and want[-1] == "4096 16384 512"
    assert want[3 * 7] == "1024 12288 4096" and want[3 * 8] == "1024 12288 %d" % ((32 << 20) // (16 * 513)) == "1024 12288 4088"      # B = 512, 513
    head = len(lines)
    rng = np.random.default_rng(5)
    works = [(1, 1, 1), (1, 64, 4096), (262144, 64, 64), (262144, 64, 2896), (262144, 64, 4096), (262144, 1, 4096), (262144, 4096, 4096), (768, 2048, 17),
             (768, 2048, 4096), (625, 2048, 256), (67092481, 1, 4096), (67092481, 4096, 1)]
    for _ in range(3000):
        works.append((int(2.0 ** rng.uniform(0, 26)), int(2.0 ** rng.uniform(0, 13)), int(2.0 ** rng.uniform(0, 12.0001))))
    for nb8, n, B in works:
        B = min(B, 4096)
        lines.append("w %d %d %d" % (nb8, n, B))
        nblk = -(-nb8 // 256)
        bpc, nchunk = bm.chunks(nblk, n, B)
        want.append("%d %d %d" % (bpc, nchunk, bm.workspace_bytes(nb8, n, B)))
        assert (nchunk - 1) * bpc < nblk <= nchunk * bpc and nchunk <= -(-bm.target_wgs(B) // n)       # every block is walked, by no more workgroups than aimed for
        # the bound the header states: the output's own size plus the budget, whatever the frame's size
        assert bm.workspace_bytes(nb8, n, B) <= (n + bm.target_wgs(B)) * 16 * B <= n * 16 * B + bm.PARTIAL_BUDGET
    # 64 frames of 4096 x 4096 (1024 blocks): 64 chunks of 16 blocks at B = 64 (4 MiB of rows), 12 chunks of 86 at B = 2896 (724 workgroups
    # aimed for: 35.6 MB), 8 chunks of 128 at B = 4096 (512 aimed for: 32 MiB)
    assert want[head + 2] == "16 64 %d" % (64 * 64 * 2 * 64 * 8)
    assert want[head + 3] == "86 12 %d" % (64 * 12 * 2 * 2896 * 8) and bm.target_wgs(2896) == 724
    assert want[head + 4] == "128 8 %d" % (64 * 8 * 2 * 4096 * 8) == "128 8 33554432"
    # 2048 frames of 192 x 256 (three blocks): two chunks - blocks 0, 1 and block 2 - at B = 17, one chunk at B = 4096 (512 workgroups aimed for)
    assert want[head + 7] == "2 2 %d" % (2048 * 2 * 2 * 17 * 8) and want[head + 8] == "3 1 %d" % (2048 * 2 * 4096 * 8)
    return lines, want


@pytest.mark.parametrize("build", ["plain", "sanitized"])
def test_index_arithmetic_against_python_integers(tmp_path, build):
    """"sanitized": built with -fsanitize=address,undefined - skipped, and reported as skipped, where the toolchain has no sanitizer
    runtimes ("plain" still runs there)"""
    exe = tmp_path / "bins_index_check"
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


def _create(L, nx, ny, n_bins, labels):
    st = C.c_int(12345)
    h = L.rc_bins_create(nx, ny, n_bins, labels, C.byref(st))
    return h, st.value


def test_argument_checks_come_before_the_device():
    """what rc_bins_create refuses from its arguments alone - a label at or above n_bins in host memory among them -, and what the two frame
    calls refuse without looking at a handle - on a machine with or without a GPU; with one, the checks that need a handle as well
    (tests/test_gpu_bins.py runs those in any case)"""
    from pyrecode_amd import _lib
    L, p = _lib.lib(), _lib.ptr
    bad = _lib.RC_ERR_BAD_ARG
    lab = np.zeros((4, 8), np.uint16)
    lab[3, 7], lab[0, 0] = 5, IGNORE
    assert _create(L, 8, 4, 0, p(lab)) == (None, bad) and "4096" in _lib.last_error()
    assert _create(L, 8, 4, 4097, p(lab)) == (None, bad) and "4096" in _lib.last_error()
    assert _create(L, 0, 4, 6, p(lab)) == (None, bad) and _create(L, 8, 0, 6, p(lab)) == (None, bad)
    assert _create(L, 65536, 4, 6, p(lab)) == (None, bad) and _create(L, 8, 70000, 6, p(lab)) == (None, bad)
    assert _create(L, 8, 4, 6, None) == (None, bad) and "NULL" in _lib.last_error()
    assert _create(L, 8, 4, 5, p(lab)) == (None, bad) and "0xFFFF" in _lib.last_error()           # the label 5 with five bins, in host memory
    lab[3, 7] = 0xFFFE
    assert _create(L, 8, 4, 4096, p(lab)) == (None, bad) and "0xFFFF" in _lib.last_error()
    lab[3, 7] = 5
    assert L.rc_bins_create(0, 0, 0, None, None) is None                                          # (status may be NULL)
    assert L.rc_bins_destroy(None) == _lib.RC_OK and L.rc_bins_count(None) == 0
    data, sizes, out = np.zeros(64, np.uint8), np.array([[4, 0, 0]], np.uint32), np.zeros(12, np.int64)
    assert L.rc_bins_frames(None, 12, 1, 0, 0, p(data), p(sizes), 1, p(out), 12, None) == bad
    assert L.rc_bins_frames_submit(None, 0, 12, 1, 0, 0, p(data), p(sizes), 1, p(out), 12) == bad
    assert L.rc_bins_frames_submit(None, 2, 12, 1, 0, 0, p(data), p(sizes), 1, p(out), 12) == bad and "slot" in _lib.last_error()
    for labels in (np.ones((4, 8), np.float32), np.ones((4, 9), np.uint16), np.ones((2, 4, 8), np.uint8), np.full((4, 8), 1 << 16, np.int64),
                   np.full((4, 8), -1, np.int16), [[1] * 8] * 4, None):
        with pytest.raises(ValueError):
            _lib.FrameBins(8, 4, labels)
    for n_bins in (0, 4097, 5):                                                                    # (5: the label 5 needs six bins)
        with pytest.raises(ValueError, match="n_bins"):
            _lib.FrameBins(8, 4, lab, n_bins)
    with pytest.raises(ValueError, match="n_bins"):
        _lib.FrameBins(8, 4, np.full((4, 8), 4096, np.uint16))                                     # (the default: 4097 bins)
    h, st = _create(L, 8, 4, 6, p(lab))
    if _lib.device_count() == 0:
        assert (h, st) == (None, _lib.RC_ERR_DEVICE)
        return
    assert h and st == _lib.RC_OK and L.rc_bins_count(h) == 6 and L.rc_bins_destroy(h) == _lib.RC_OK
    check_frame_call_arguments(_lib)


def check_frame_call_arguments(hip):
    """Every refusal of rc_bins_frames / _submit that is known from the arguments and the handle alone: nothing is queued and `out` keeps
    its fill.  Needs a handle, so a GPU."""
    L, p = hip.lib(), hip.ptr
    bad, uns, small = hip.RC_ERR_BAD_ARG, hip.RC_ERR_UNSUPPORTED, hip.RC_ERR_OUT_TOO_SMALL
    lab = np.zeros((4, 8), np.int32)
    lab[1, 1], lab[0, 0] = 2, IGNORE
    fb = hip.FrameBins(8, 4, lab)
    assert fb.n_bins == 3 == L.rc_bins_count(fb.handle)
    data, sizes = np.zeros(64, np.uint8), np.array([[4, 0, 0], [4, 0, 0]], np.uint32)
    out = np.full(32, -0x5A5A5A5A5A5A5A5B, np.int64)

    def call(slot, d=12, level=1, mode=0, n=2, cells=12, data=data, sizes=sizes, dst=out):
        args = (d, level, mode, 0, p(data), p(sizes), n, p(dst) if isinstance(dst, np.ndarray) else dst, cells)
        return L.rc_bins_frames(fb.handle, *args, None) if slot is None else L.rc_bins_frames_submit(fb.handle, slot, *args)
    for slot in (None, 0, 1):
        assert call(slot, cells=11) == small and "n * 2 * n_bins" in hip.last_error()
        assert call(slot, n=1, cells=5) == small
        assert call(slot, d=20) == uns and "16" in hip.last_error()
        assert call(slot, d=17) == uns and call(slot, d=0) == bad
        assert call(slot, level=4) == uns and call(slot, level=0) == uns
        assert call(slot, n=0) == bad and call(slot, data=None) == bad and call(slot, sizes=None) == bad and call(slot, dst=None) == bad
        assert call(slot, dst=p(out) + 4) == bad and "aligned" in hip.last_error()
        assert call(slot, sizes=np.array([[4, 0, 0], [5, 0, 0]], np.uint32)) == bad and "geometry" in hip.last_error()
    assert call(2) == bad and "slot" in hip.last_error()
    fb.close()
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
        _lib.FrameBins(64, 64, np.zeros((64, 64), np.uint16))
    rd = ReCoDeReader(os.path.join(GOLDEN, "files", "g3_l1z12.rc1"))
    rd.open(print_header=False)
    try:
        lab = np.zeros((int(rd._header["ny"]), int(rd._header["nx"])), np.uint16)
        with pytest.raises(RuntimeError) as e:
            rd.get_frame_bins(0, 2, lab)
        assert not isinstance(e.value, NotImplementedError)
        with pytest.raises(RuntimeError):
            next(rd.iter_frame_bins(batch=2, labels=lab))
    finally:
        rd.close()
