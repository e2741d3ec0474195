"""-m gpu: calibration on the device (rc_calib.hip through the C ABI and pyrecode_amd.utils.calibration) against numpy and against what the
reference's own functions returned (tests/golden/calibration/g13_calib_*.npz, written by tests/golden/make_golden_calibration.py).
Median, range, histogram, thresholds and event counts are compared exactly; the standard deviation to one float32 ulp (numpy's is a
two-pass float64 computation whose last bits may differ before the rounding to float32), the fitted sigma to 1e-6 relative."""
import ctypes as C
import functools
import os
import warnings

import numpy as np
import pytest

from conftest import load_npz

pytestmark = pytest.mark.gpu

FIXTURES = ("a", "b", "dead", "neg")
N_BINS = 100


@pytest.fixture(scope="module")
def hip():
    from pyrecode_amd import _lib
    if _lib.device_count() == 0:
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    return _lib


@functools.lru_cache(maxsize=None)
def _fixture(name):
    return load_npz("calibration/g13_calib_%s.npz" % name)


def _make_stack(n, ny, nx, seed):
    """full-range values; and columns that are constant, tied (four neighbouring values), 0 / 65535 only, and noise with rare events"""
    rng = np.random.default_rng(seed)
    N = ny * nx
    d = rng.integers(0, 65536, (n, N)).astype(np.uint16)
    kind = rng.integers(0, 5, N)
    d[:, kind == 1] = rng.integers(0, 65536, N).astype(np.uint16)[kind == 1][None]
    d[:, kind == 2] = (rng.integers(100, 104, (n, N))).astype(np.uint16)[:, kind == 2]
    d[:, kind == 3] = (rng.integers(0, 2, (n, N)) * 65535).astype(np.uint16)[:, kind == 3]
    noise = np.clip(np.rint(100 + rng.normal(0, 6, (n, N)) + (rng.random((n, N)) < 0.01) * 1500), 0, 65535).astype(np.uint16)
    d[:, kind == 4] = noise[:, kind == 4]
    return d.reshape(n, ny, nx)


def _ulps(a, b):
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def _stats(hip, stack_address, n, N, n_stats):
    med, std, rng = np.full(N, -1, np.float32), np.full(N, -1, np.float32), np.zeros(2, np.int32)
    hip.check(hip.lib().rc_calib_stats(stack_address, n, N, n_stats, hip.ptr(med), hip.ptr(std), hip.ptr(rng)), "rc_calib_stats")
    return med, std, rng


def _check_stats(hip, stack, n_stats, address=None):
    n, N = stack.shape[0], stack[0].size
    med, std, rng = _stats(hip, stack.ctypes.data if address is None else address, n, N, n_stats)
    want_med = np.median(stack, axis=0).astype(np.float32).ravel()
    want_std = np.std(stack, axis=0).astype(np.float32).ravel()
    assert med.tobytes() == want_med.tobytes(), "median differs at pixels %s" % np.flatnonzero(med != want_med)[:8]
    worst = int(_ulps(std, want_std).max())
    print("n %d N %d: std within %d ulp" % (n, N, worst))
    assert worst <= 1
    d2 = 2 * stack[n - n_stats:].reshape(n_stats, N).astype(np.int64) - np.rint(2 * want_med.astype(np.float64)).astype(np.int64)
    assert rng.tolist() == [int(d2.min()), int(d2.max())]
    return med, std, rng


@pytest.mark.parametrize("shape", [(37, 53), (8, 200), (5, 24)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("n", [1, 2, 3, 20, 21, 64, 65])
def test_median_std_range_equal_numpy(hip, n, shape):
    """37 x 53: 1961 pixels, no multiple of anything (a lane per pixel loads); 8 x 200: whole tiles of 64 pixels, 16-byte loads; 5 x 24: 16-byte
    loads with a last tile that is not full"""
    stack = _make_stack(n, shape[0], shape[1], 100 * n + shape[1])
    _check_stats(hip, stack, max(1, n // 3))
    if n == 21:
        _check_stats(hip, stack, n)                                          # the range over every frame


def test_columns_too_long_for_lds_take_the_global_path(hip):
    n = hip.lib().rc_calib_lds_max_frames() + 1
    _check_stats(hip, _make_stack(n, 8, 8, 7), 5)
    _check_stats(hip, _make_stack(n - 1, 8, 8, 8), 5)                         # the longest column the LDS path takes


def test_device_stack_that_starts_off_a_16_byte_boundary(hip):
    import torch
    stack = _make_stack(20, 8, 200, 3)
    t = torch.zeros(stack.size + 8, dtype=torch.int16, device="cuda")
    t[1:1 + stack.size] = torch.from_numpy(stack.view(np.int16).ravel()).cuda()
    torch.cuda.synchronize()            # the library reads on its own streams: the copy above must be complete (include/recode_hip.h)
    _check_stats(hip, stack, 6, address=t.data_ptr() + 2)


@pytest.mark.parametrize("name", FIXTURES)
def test_stats_equal_the_references(hip, name):
    g = _fixture(name)
    stack = np.ascontiguousarray(g["stack"])
    med, std, _ = _check_stats(hip, stack, int(g["n_stats"]))
    assert med.tobytes() == g["median"].astype(np.float32).tobytes()
    assert int(_ulps(std, g["std"].astype(np.float32).ravel()).max()) <= 1


def _range_and_histogram(hip, stack, n_stats):
    """what calibrate does: range from the device, edges from numpy, counts from the device"""
    n, N = stack.shape[0], stack[0].size
    med, _, rng = _stats(hip, stack.ctypes.data, n, N, n_stats)
    edges = np.histogram_bin_edges(np.array([rng[0] / 2.0, rng[1] / 2.0]), bins=N_BINS)
    counts = np.zeros(N_BINS, np.uint64)
    frames = np.ascontiguousarray(stack[n - n_stats:])
    hip.check(hip.lib().rc_calib_histogram(frames.ctypes.data, n_stats, N, hip.ptr(med), hip.ptr(edges), N_BINS, hip.ptr(counts)), "rc_calib_histogram")
    dsd = frames.astype(np.float64) - med.reshape(stack.shape[1:])
    want, want_edges = np.histogram(dsd.flatten(), bins=N_BINS)
    assert np.array_equal(edges, want_edges)
    assert np.array_equal(counts.astype(np.int64), want), np.flatnonzero(counts.astype(np.int64) != want)
    assert int(counts.sum()) == n_stats * N
    return counts, edges


@pytest.mark.parametrize("name", FIXTURES)
def test_range_and_histogram_equal_the_references(hip, name):
    g = _fixture(name)
    counts, edges = _range_and_histogram(hip, np.ascontiguousarray(g["stack"]), int(g["n_stats"]))
    assert np.array_equal(edges, g["edges"]) and np.array_equal(counts.astype(np.int64), g["hist"])


def test_histogram_of_a_constant_stack(hip):
    """lo == hi: numpy widens the range to +-0.5 and everything lands in one bin"""
    counts, edges = _range_and_histogram(hip, np.full((5, 9, 31), 500, np.uint16), 3)
    assert edges[0] == -0.5 and edges[-1] == 0.5 and int(counts.max()) == 3 * 9 * 31


def _histogram(hip, frames, med, edges):
    counts = np.full(len(edges) - 1, 99, np.uint64)
    hip.check(hip.lib().rc_calib_histogram(frames.ctypes.data, frames.shape[0], frames[0].size, hip.ptr(med), hip.ptr(edges), len(edges) - 1,
                                           hip.ptr(counts)), "rc_calib_histogram")
    want = np.histogram((frames.astype(np.float64) - med).flatten(), bins=edges)[0]
    assert np.array_equal(counts.astype(np.int64), want)
    return counts


def test_histogram_with_every_value_in_one_bin_and_on_the_last_edge(hip):
    rng = np.random.default_rng(5)
    med = (100 + 0.5 * rng.integers(0, 2, (7, 45))).astype(np.float32)
    frames = (np.floor(med)[None] + rng.integers(1, 6, (4, 7, 45))).astype(np.uint16)      # frame - median in [0.5, 5]
    counts = _histogram(hip, frames, med, np.linspace(-1000.0, 1000.0, 101))
    assert np.count_nonzero(counts) == 1 and int(counts[50]) == frames.size
    # values exactly on edges: on the last one (counted by the last bin), on inner ones (counted by the bin they open), outside (by none)
    med = np.full((7, 45), 100, np.float32)
    frames = (100 + rng.integers(0, 12, (4, 7, 45))).astype(np.uint16)                      # 0 .. 11 on edges 0, 1, .. 10
    frames[0, 0, 0] = 110
    counts = _histogram(hip, frames, med, np.linspace(0.0, 10.0, 11))
    assert int(counts[9]) == int(((frames == 109) | (frames == 110)).sum()) and int(counts.sum()) == int((frames <= 110).sum())
    frames[...] = 100
    frames[3, 6, 44] = 110                                                                  # ONE value on the last edge
    assert _histogram(hip, frames, med, np.linspace(0.0, 10.0, 11)).tolist() == [frames.size - 1] + [0] * 8 + [1]


def _calibrate(name, as_tensor=False, **kw):
    from pyrecode_amd.utils import calibrate
    g = _fixture(name)
    data = np.ascontiguousarray(g["stack"])
    if as_tensor == "contiguous":
        import torch
        data = torch.from_numpy(data.view(np.int16)).cuda().view(torch.uint16)
    elif as_tensor == "permuted":
        # a view that is NOT contiguous, made by device work that is still queued when calibrate is called: calibrate must make its own
        # contiguous copy and wait for both before the library reads the frames on its own streams
        import torch
        stored = torch.from_numpy(np.ascontiguousarray(data.transpose(1, 0, 2)).view(np.int16)).cuda()      # [ny][n][nx]
        data = (stored + 0).view(torch.uint16).permute(1, 0, 2)
        assert not data.is_contiguous()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        res = calibrate(data, int(g["n_stats"]), int(g["n_sigmas"]), **kw)
    return g, res, [w for w in caught if issubclass(w.category, RuntimeWarning) and "negative sigma" in str(w.message)]


def _check_against_fixture(g, res):
    want = float(g["fit_std"])
    assert abs(float(res["fit_std"]) - want) <= 1e-6 * abs(want)
    assert res["median"].tobytes() == g["median"].tobytes() and np.array_equal(res["hist"], g["hist"]) and np.array_equal(res["edges"], g["edges"])
    assert int(_ulps(res["std"].ravel(), g["std"].ravel()).max()) <= 1
    assert len(res["thresholds"]) == int(g["n_sigmas"])
    n_pixels = g["median"].size
    for i, t in enumerate(res["thresholds"]):
        assert t.dtype == np.uint16 and np.array_equal(t, g["thresholds"][i]), i
        print("sigma %d: events %r (reference %r), foreground %r (reference %r)" % (
            i, res["avg_n_events"][i], float(g["avg_n_events"][i]), res["avg_p_foreground_pixels"][i], float(g["avg_p_foreground_pixels"][i])))
        assert res["avg_n_events"][i] == float(g["avg_n_events"][i]) == g["events"][i].sum() / int(g["n_stats"])
        assert res["avg_p_foreground_pixels"][i] == float(g["avg_p_foreground_pixels"][i])
        assert res["dose_rate"][i] == float(g["avg_n_events"][i]) / n_pixels


@pytest.mark.parametrize("name", FIXTURES)
def test_calibrate_equals_the_reference(hip, name):
    g, res, negative = _calibrate(name)
    _check_against_fixture(g, res)
    assert bool(negative) == (name == "neg") == (float(res["fit_std"]) < 0)
    assert "acc_threshold" not in res and "expected_n_events" not in res
    if name == "neg":
        assert res["avg_p_foreground_pixels"][3] > 0.95          # thresholds below the median: the map is nearly completely set


@pytest.mark.parametrize("layout", ["contiguous", "permuted"])
def test_calibrate_takes_a_device_tensor(hip, layout):
    g, res, _ = _calibrate("a", as_tensor=layout)
    _check_against_fixture(g, res)


@pytest.mark.parametrize("name", ["a", "b", "dead"])
def test_accurate_thresholds_equal_the_references_where_they_are_defined(hip, name):
    g, res, _ = _calibrate(name, use_acc=True, sigma_acc=int(_fixture(name)["sigma_acc"]))
    _check_against_fixture(g, res)
    assert res["expected_n_events"] == int(g["expected_n_events"]) >= 2
    und = g["acc_undefined"]
    acc = res["acc_threshold"]
    assert acc.dtype == np.float32 and acc.shape == und.shape
    assert np.array_equal(acc[~und], g["acc"][~und])
    assert res["n_undefined_pixels"] == int(und.sum()) and (acc[und] == 65535).all()
    assert (name == "dead") == bool(und.any())
    # the entry point itself, at the ranks nearest the ends: k = 1 and k = n - 1 (never defined: at most half the values exceed the median)
    stack = np.ascontiguousarray(g["stack"])
    n, N = stack.shape[0], stack[0].size
    for k in (1, n - 1):
        out, cnt = np.zeros(N, np.float32), C.c_uint64(0)
        hip.check(hip.lib().rc_calib_top_thresholds(stack.ctypes.data, n, N, hip.ptr(res["median"]), k, hip.ptr(out), C.addressof(cnt)))
        s = np.sort(stack.reshape(n, N), axis=0).astype(np.float32)
        defined = (stack.reshape(n, N) > res["median"].ravel()).sum(axis=0) >= k + 1
        want = np.where(defined, (s[n - k - 1] + s[n - k]) / np.float32(2), np.float32(65535))
        assert np.array_equal(out, want) and cnt.value == int((~defined).sum())
        assert defined.any() == (k == 1)


def test_too_few_events_for_the_accurate_step(hip, capsys):
    g, res, _ = _calibrate("neg", use_acc=True, sigma_acc=int(_fixture("neg")["sigma_acc"]))
    assert res["expected_n_events"] == int(g["expected_n_events"]) < 2 and "acc_threshold" not in res
    assert "Unable to compute accurate thresholds: too few events in dataset" in capsys.readouterr().out


def test_make_calibration_frames_writes_the_references_files(hip, tmp_path, capsys):
    """file names and bytes; then one threshold file back into the writer as dark_data: three frames read back as the residuals above it"""
    from test_em_reader import write_mrc
    from pyrecode_amd.params import InputParams
    from pyrecode_amd.recode_reader import ReCoDeReader, merge_parts
    from pyrecode_amd.recode_writer import ReCoDeWriter
    from pyrecode_amd.utils import make_calibration_frames
    g = _fixture("dead")
    stack = g["stack"]
    n, ny, nx = stack.shape
    src = str(tmp_path / "flat.mrc")
    write_mrc(src, stack, 6)
    out = tmp_path / "cal"
    out.mkdir()
    sa = int(g["sigma_acc"])
    res = make_calibration_frames(src, np.uint16, n, int(g["n_stats"]), int(g["n_sigmas"]), savepath=str(out), filename_prefix="det", use_acc=True, sigma_acc=sa)
    _check_against_fixture(g, res)
    names = ["det__dark_ref_%d.bin" % i for i in range(int(g["n_sigmas"]))] + ["det__dark_ref_%dA.bin" % sa]
    assert sorted(os.listdir(out)) == sorted(names)
    for i in range(int(g["n_sigmas"])):
        assert (out / names[i]).read_bytes() == g["thresholds"][i].astype(np.uint16).tobytes()
    und = g["acc_undefined"]
    want_acc = np.where(und, 65535, np.where(und, 0, g["acc"]).astype(np.uint16)).astype(np.uint16)
    assert (out / names[-1]).read_bytes() == want_acc.tobytes()
    printed = capsys.readouterr().out
    for piece in ("\n Fit Result \n Init params=", "\nAvg. std.dev. per pixel:", "Global intensity std. dev.:", "Calibration time:",
                  "Avg. prop. foreground pixels for sigma=0 is: ", "Avg. electron count for sigma=3 is: ", "Avg. dose rate for sigma=1 is: "):
        assert piece in printed
    # a prefix that already ends in '_' gets no second one from the prefix rule (the name part still starts with its own)
    make_calibration_frames(src, np.uint16, n, int(g["n_stats"]), 1, savepath=str(out), filename_prefix="x_")
    assert (out / "x__dark_ref_0.bin").read_bytes() == g["thresholds"][0].tobytes()

    t = np.fromfile(out / names[2], np.uint16).reshape(ny, nx)
    cfg = dict(zip(load_npz("g3_l1z12.npz")["cfg_keys"].tolist(), (int(v) for v in load_npz("g3_l1z12.npz")["cfg_vals"])))
    cfg.update(num_rows=ny, num_cols=nx, num_frames=3, num_threads=1, compression_scheme=2, source_bit_depth=12, target_bit_depth=12,
               calibration_threshold_epsilon=0, reduction_level=1, rc_operation_mode=1)
    p = tmp_path / "params.txt"
    p.write_text("".join("%s = %d\n" % kv for kv in cfg.items()))
    ip = InputParams()
    ip.load(str(p))
    frames = np.ascontiguousarray(stack[-3:])
    assert int(frames.max()) < 4096
    w = ReCoDeWriter("flat", dark_data=t, output_directory=str(tmp_path), input_params=ip, mode="batch", validation_frame_gap=-1, node_id=0)
    w.start()
    w.run(frames)
    w.close()
    merge_parts(str(tmp_path), "flat.rc1", 1)
    rd = ReCoDeReader(str(tmp_path / "flat.rc1"), is_intermediate=False)
    rd.open(print_header=False)
    want = np.where(frames > t, frames - t, 0).astype(np.uint16)
    assert want.any()
    for z in range(3):
        assert np.array_equal(np.asarray(rd.get_frame(z)[z]["data"].todense()), want[z])
    rd.close()
