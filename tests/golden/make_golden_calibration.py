#!/usr/bin/env python3
"""Generate the calibration fixtures tests/golden/calibration/g13_calib_*.npz by RUNNING THE REFERENCE's pyrecode/utils/calibration.py.

Test infrastructure, run once where the reference exists; the committed outputs are all the tests ever see.  Nothing of the reference
is copied: a fixture holds a seeded input stack and what the reference's functions returned for it.  (A directory of their own:
tests/golden/*.npz is the set tests/golden/make_golden.py writes, and tests/test_oracle_golden.py pins exactly that set;
tests/test_calibration_cpu.py pins this one the same way.)

How the reference is run: its module imports `numba` and `pims`, both absent.  Stand-ins placed in sys.modules (numba: `jit` = identity,
`prange` = range; pims: empty) let it import, its @jit loops then run as the plain Python they are written in.  Called:
  _median_std_nb (:48-57), _get_fit_params (:64-84, its histogram is reproduced beside it with the same np.histogram call to record counts
  and edges), _count_events (:19-23), _get_pixel_thresh_2 (:26-45); thresholds and averages as make_calibration_frames (:113-131) computes
  them - that function itself opens its file through pims and cannot run.

Stacks: per-pixel offsets 80..120, Gaussian noise of sigma 6, 1 % events of +60..2000.
  a     37 x 53, n = 20, n_stats = 6
  b     48 x 72, n = 21, n_stats = 5 (odd n)
  dead  24 x 40, n = 20, n_stats = 6, three constant columns of pixels: no value above the median, the accurate threshold is undefined there
  neg   a stack on which curve_fit ends on the NEGATIVE root of sigma^2 (kept on purpose: the reference uses it as it comes)
"""
import contextlib
import importlib.util
import io
import os
import sys
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("RECODE_REFERENCE", "/root/reference")
OUT = os.environ.get("RC_GOLDEN_OUT") or os.path.join(HERE, "calibration")
N_SIGMAS = 4


def load_reference():
    numba = types.ModuleType("numba")
    numba.jit = lambda *a, **k: (lambda f: f)
    numba.prange = range
    sys.modules.setdefault("numba", numba)
    sys.modules.setdefault("pims", types.ModuleType("pims"))
    spec = importlib.util.spec_from_file_location("ref_calibration", os.path.join(REF, "pyrecode", "utils", "calibration.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def make_stack(seed, n, ny, nx, dead_columns=()):
    rng = np.random.default_rng(seed)
    offset = rng.integers(80, 121, (ny, nx)).astype(np.float64)
    d = offset[None] + rng.normal(0.0, 6.0, (n, ny, nx))
    events = rng.random((n, ny, nx)) < 0.01
    d = np.where(events, d + rng.integers(60, 2001, (n, ny, nx)), d)
    d = np.clip(np.rint(d), 0, 65535).astype(np.uint16)
    for c in dead_columns:
        d[:, :, c] = offset[:, c].astype(np.uint16)[None]
    return d


def run_reference(ref, d, n_stats, sigma_acc):
    n, ny, nx = d.shape
    with contextlib.redirect_stdout(io.StringIO()), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        # (the reference names the first frame axis nx and the second ny; only their order matters)
        m, s = ref._median_std_nb(d, ny, nx)
        fit_std = ref._get_fit_params(d, n, n_stats, nx, ny, m)
        dsd = np.zeros((n_stats, ny, nx))
        for i, f in enumerate(range(n - n_stats, n)):
            dsd[i] = d[f] - m
        hist, edges = np.histogram(dsd.flatten(), bins=100, density=False)
        n_pixels = ny * nx
        thr, events, pixels, avg_e, avg_p = [], [], [], [], []
        for i in range(N_SIGMAS):
            t = np.floor(m + fit_std * i).astype(np.uint16)
            thr.append(t)
            ne, npx, n_events, p_fg = [], [], 0, 0
            for f in range(n - n_stats, n):
                n_e, n_fp = ref._count_events(d[f], t)
                ne.append(n_e)
                npx.append(n_fp)
                n_events += n_e
                p_fg += (n_fp / n_pixels)
            events.append(ne)
            pixels.append(npx)
            avg_e.append(n_events / n_stats)
            avg_p.append(p_fg / n_stats)
        expected = int(np.ceil(n * (avg_e[sigma_acc] / n_pixels)))
        out = dict(stack=d, n_stats=n_stats, n_sigmas=N_SIGMAS, median=m, std=s, fit_std=np.float64(fit_std), hist=hist.astype(np.int64), edges=edges,
                   thresholds=np.stack(thr), events=np.array(events, np.int64), pixels=np.array(pixels, np.int64),
                   avg_n_events=np.array(avg_e, np.float64), avg_p_foreground_pixels=np.array(avg_p, np.float64),
                   sigma_acc=sigma_acc, expected_n_events=expected)
        if expected >= 2:
            acc = ref._get_pixel_thresh_2(d, ny, nx, expected, m)
            out["acc"] = acc
            out["acc_undefined"] = acc < 0            # np.finfo(float32).min took part: the reference's value means nothing
    return out


def check_margins(name, g, want_negative):
    """a last-bit difference in curve_fit on another machine must not move a threshold"""
    fs = float(g["fit_std"])
    assert (fs < 0) == want_negative, "%s: fit_std = %r" % (name, fs)
    for i in range(N_SIGMAS):
        for x in (fs * i, fs * i + 0.5):
            fr = x - np.floor(x)
            assert i == 0 or 1e-3 <= fr <= 1 - 1e-3, "%s: frac(%r) = %r is too close to an integer" % (name, x, fr)


CASES = [   # name, seed, (n, ny, nx), n_stats, dead columns, sigma_acc, negative sigma expected
    ("a", 1301, (20, 37, 53), 6, (), 1, False),
    ("b", 1302, (21, 48, 72), 5, (), 1, False),
    ("dead", 1303, (20, 24, 40), 6, (3, 17, 39), 1, False),
    ("neg", 1480, (20, 24, 40), 6, (), 1, True),     # (found by trying seeds 1400.. until the fit came out negative)
]


def main():
    os.makedirs(OUT, exist_ok=True)
    ref = load_reference()
    for name, seed, shape, n_stats, dead, sigma_acc, negative in CASES:
        g = run_reference(ref, make_stack(seed, *shape, dead_columns=dead), n_stats, sigma_acc)
        check_margins(name, g, negative)
        g["seed"] = seed
        if dead:
            assert g["expected_n_events"] >= 2 and g["acc_undefined"][:, list(dead)].all()
        path = os.path.join(OUT, "g13_calib_%s.npz" % name)
        np.savez_compressed(path, **g)
        print("%-5s seed %d  fit_std %.6f  expected_n_events %d  undefined %s  %d bytes" % (
            name, seed, float(g["fit_std"]), g["expected_n_events"], int(g["acc_undefined"].sum()) if "acc_undefined" in g else "-", os.path.getsize(path)))


if __name__ == "__main__":
    main()
