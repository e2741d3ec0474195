"""Calibration on the CPU: the per-column selection the kernels are built from - as a Python model (tests/calib_select_model.py) and as the
C++ itself (pyrecode_amd/csrc/rc_calib.h through tests/native/calib_select_check.cpp, a stand-alone program under AddressSanitizer / UBSan) -
against np.sort / np.median / np.std; the host half of the fit against the reference's results (tests/golden/calibration/g13_calib_*.npz, written by
tests/golden/make_golden_calibration.py); and the new entry points' argument checks and their loud failure without a GPU."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import calib_select_model as csm
from conftest import REPO, load_npz

SRC = os.path.join(REPO, "tests", "native", "calib_select_check.cpp")
COLUMNS = csm.columns()
FIXTURES = ("a", "b", "dead", "neg")


def _ulps(a, b):
    a, b = np.float32(a), np.float32(b)
    return abs(int(a.view(np.int32)) - int(b.view(np.int32)))


def test_catalogue_covers_the_cases():
    by = dict(COLUMNS)
    assert {len(by[k]) for k in ("n1", "n2", "n3")} == {1, 2, 3}
    assert set(by["extremes_even"].tolist()) == {0, 65535} and len(set(by["all_equal_even"].tolist())) == 1
    s = np.sort(by["ties_straddle_middle"])
    assert s[len(s) // 2 - 1] == s[len(s) // 2] and s[0] != s[len(s) // 2] != s[-1]
    s = np.sort(by["second_rank_equals_first"])
    assert s[1] == s[2]
    assert any(len(c) == 64 for _, c in COLUMNS) and any(len(c) == 65 for _, c in COLUMNS)


@pytest.mark.parametrize("name,col", COLUMNS, ids=[n for n, _ in COLUMNS])
def test_model_selects_what_sorting_selects(name, col):
    n = len(col)
    for r in range(n):
        assert csm.select_pair(col, r) == csm.reference_pair(col, r), r
    med = csm.median(col)
    want = np.median(col).astype(np.float32)
    assert med.tobytes() == want.tobytes()                                   # bit-exact
    assert _ulps(csm.std(col), np.std(col).astype(np.float32)) <= 1
    for k in range(0, n + 1):                                                # k = 1 and k = n - 1 among them; 0 and n are never defined
        got, ref = csm.top_pair(col, med, k), csm.reference_top_pair(col, med, k)
        assert (got is None) == (ref is None) and (got is None or got.tobytes() == ref.tobytes()), k
    assert csm.top_pair(col, med, 0) is None and csm.top_pair(col, med, n) is None


@pytest.mark.parametrize("build", ["plain", "sanitized"])
def test_core_selects_what_sorting_selects(tmp_path, build):
    """every column of the catalogue, every rank and every k through the host build of rc_calib.h as a stand-alone program; its answers are
    compared with numpy here (and with std::sort by the program).  "sanitized": built with -fsanitize=address,undefined - skipped, and
    reported as skipped, where the toolchain has no sanitizer runtimes ("plain" still runs there, vector::at still checks)"""
    exe = tmp_path / "calib_select_check"
    flags = []
    if build == "sanitized":
        flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
        probe = subprocess.run(["g++", "-x", "c++", "-", "-o", str(tmp_path / "probe")] + flags, input=b"int main(){return 0;}", capture_output=True)
        if probe.returncode != 0:
            pytest.skip("this toolchain cannot link -fsanitize=address,undefined: the sanitizer run did not take place")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-o", str(exe), SRC] + flags)
    asked = []
    with open(tmp_path / "records.bin", "wb") as f:
        for _, col in COLUMNS:
            n = len(col)
            for r in range(n):
                k = (1, n - 1, max(n // 4, 1), n)[r % 4]
                asked.append((col, r, k))
                f.write(struct.pack("<III", n, r, k) + col.astype("<u2").tobytes())
    run = subprocess.run([str(exe), str(tmp_path / "records.bin")], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    lines = run.stdout.splitlines()
    assert lines[-1] == "records %d ok" % len(asked)
    for (col, r, k), line in zip(asked, lines):
        lo, hi, m2, std_bits, ok, top_bits = (int(v) for v in line.split())
        assert (lo, hi) == csm.reference_pair(col, r)
        med = np.median(col).astype(np.float32)
        assert np.float32(0.5 * m2).tobytes() == med.tobytes()
        assert _ulps(np.uint32(std_bits).view(np.float32), np.std(col).astype(np.float32)) <= 1
        ref = csm.reference_top_pair(col, med, k)
        assert bool(ok) == (ref is not None)
        assert np.uint32(top_bits).view(np.float32) == (ref if ref is not None else np.float32(65535))


@pytest.mark.parametrize("name", FIXTURES)
def test_host_half_of_the_fit_gives_the_references_sigma_and_thresholds(name):
    from pyrecode_amd.utils import calibration as cal
    g = load_npz("calibration/g13_calib_%s.npz" % name)
    fit_std, p0, popt = cal.fit_sigma(g["hist"], g["edges"])
    want = float(g["fit_std"])
    assert abs(fit_std - want) <= 1e-6 * abs(want)
    assert (fit_std < 0) == (name == "neg")
    for i in range(int(g["n_sigmas"])):
        t = cal.threshold_frame(g["median"], fit_std, i, np.uint16)
        assert t.dtype == np.uint16 and np.array_equal(t, g["thresholds"][i])
    # the edges the host makes from the range are numpy's own
    d = g["stack"][-int(g["n_stats"]):].astype(np.float64) - g["median"]
    assert np.array_equal(np.histogram_bin_edges(np.array([d.min(), d.max()]), bins=100), g["edges"])


def test_entry_points_check_sizes_before_any_device_work():
    from pyrecode_amd import _lib
    L = _lib.lib()
    assert L.rc_calib_lds_max_frames() == 512
    stack = np.zeros((4, 64), np.uint16)
    med, std, acc = np.zeros(64, np.float32), np.zeros(64, np.float32), np.zeros(64, np.float32)
    rng, cnt, und = np.zeros(2, np.int32), np.zeros(100, np.uint64), np.zeros(1, np.uint64)
    edges = np.linspace(0, 1, 101)
    p = lambda a: a.ctypes.data   # noqa: E731
    bad = _lib.RC_ERR_BAD_ARG
    assert L.rc_calib_stats(p(stack), 0, 64, 0, p(med), p(std), p(rng)) == bad                    # n == 0
    assert L.rc_calib_stats(p(stack), 65536, 64, 1, p(med), p(std), p(rng)) == bad                # n > 65535
    assert L.rc_calib_stats(p(stack), 4, 64, 5, p(med), p(std), p(rng)) == bad                    # n_stats > n
    assert L.rc_calib_stats(p(stack), 4, 0, 1, p(med), p(std), p(rng)) == bad                     # no pixels
    assert L.rc_calib_histogram(p(stack), 4, 64, p(med), p(edges), 0, p(cnt)) == bad              # n_bins == 0
    assert L.rc_calib_histogram(p(stack), 0, 64, p(med), p(edges), 100, p(cnt)) == bad
    assert L.rc_calib_top_thresholds(p(stack), 0, 64, p(med), 2, p(acc), p(und)) == bad
    assert L.rc_calib_top_thresholds(p(stack), 65536, 64, p(med), 2, p(acc), p(und)) == bad
    assert L.rc_calib_top_thresholds(p(stack), 4, 64, p(med), 0, p(acc), p(und)) == bad
    assert L.rc_calib_stats(None, 4, 64, 1, p(med), p(std), p(rng)) == bad
    with pytest.raises(ValueError):
        _lib.check(L.rc_calib_stats(p(stack), 4, 64, 5, p(med), p(std), p(rng)))


def test_no_gpu_means_loud_failure_not_fallback():
    from pyrecode_amd import _lib
    from pyrecode_amd.utils import calibrate
    if _lib.device_count() > 0:
        pytest.skip("a GPU is visible")
    L = _lib.lib()
    stack = np.full((4, 64), 7, np.uint16)
    med, std, acc = np.full(64, -1, np.float32), np.zeros(64, np.float32), np.zeros(64, np.float32)
    rng, cnt, und = np.zeros(2, np.int32), np.zeros(100, np.uint64), C.c_uint64(0)
    edges = np.linspace(-1, 1, 101)
    p = lambda a: a.ctypes.data   # noqa: E731
    assert L.rc_calib_stats(p(stack), 4, 64, 2, p(med), p(std), p(rng)) == _lib.RC_ERR_DEVICE
    assert L.rc_calib_histogram(p(stack), 4, 64, p(med), p(edges), 100, p(cnt)) == _lib.RC_ERR_DEVICE
    assert L.rc_calib_top_thresholds(p(stack), 4, 64, p(med), 2, p(acc), C.addressof(und)) == _lib.RC_ERR_DEVICE
    assert (med == -1).all() and not cnt.any()                                # nothing computed on the host
    with pytest.raises(_lib.RecodeHipError):
        calibrate(stack.reshape(4, 8, 8), 2, 2)


def test_other_dtypes_are_refused():
    from pyrecode_amd.utils import calibrate, make_calibration_frames   # noqa: F401
    for dt in (np.int16, np.uint8, np.float32, np.uint32):
        with pytest.raises(NotImplementedError):
            calibrate(np.zeros((3, 4, 4), dt), 2, 2)


def test_committed_fixtures_are_what_the_reference_returns_today(tmp_path):
    """the pin: where the reference is present, tests/golden/make_golden_calibration.py is run again into a scratch directory and every
    array it writes is compared with the committed fixtures"""
    import sys
    ref = os.environ.get("RECODE_REFERENCE", "/root/reference")
    if not os.path.isfile(os.path.join(ref, "pyrecode", "utils", "calibration.py")):
        pytest.skip("the reference is not present here: the fixtures cannot be regenerated")
    golden = os.path.join(REPO, "tests", "golden")
    r = subprocess.run([sys.executable, os.path.join(golden, "make_golden_calibration.py")], env=dict(os.environ, RC_GOLDEN_OUT=str(tmp_path)),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    made = sorted(f for f in os.listdir(tmp_path) if f.endswith(".npz"))
    assert made == sorted(os.listdir(os.path.join(golden, "calibration"))) == ["g13_calib_%s.npz" % n for n in sorted(FIXTURES)]
    for fn in made:
        with np.load(tmp_path / fn, allow_pickle=False) as a, np.load(os.path.join(golden, "calibration", fn), allow_pickle=False) as b:
            assert sorted(a.files) == sorted(b.files), fn
            for k in a.files:
                assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), "%s[%s] differs" % (fn, k)
