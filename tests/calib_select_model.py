"""A serial Python model of the calibration kernels' per-column logic (pyrecode_amd/csrc/rc_calib.h): two neighbouring ranks of a column of
uint16 values by 16-step bitwise bisection, np.median from them, the exact-integer standard deviation, and the "accurate" threshold (the
mean of the (k+1)-th and k-th largest values, defined when k + 1 values lie above the median).  Plus the catalogue of columns the CPU
tests run through the model and through the C++ itself."""
import math

import numpy as np


def select_pair(col, r):
    """(value of ascending rank r, value of rank r + 1 - or the same value when r + 1 == n)"""
    col = [int(v) for v in col]
    n = len(col)
    assert 0 <= r < n
    prefix, same = 0, n
    for b in range(15, -1, -1):
        want = prefix >> b
        c = sum(1 for v in col if (v >> b) == want)
        if r < c:
            same = c
        else:
            r -= c
            same -= c
            prefix |= 1 << b
    if r + 1 < same:
        return prefix, prefix
    above = [v for v in col if v > prefix]
    return prefix, (min(above) if above else prefix)


def median(col):
    n = len(col)
    lo, hi = select_pair(col, (n - 1) // 2)
    return np.float32(0.5 * (2 * lo if n & 1 else lo + hi))


def std(col):
    n = len(col)
    s1 = sum(int(v) for v in col)
    s2 = sum(int(v) * int(v) for v in col)
    return np.float32(math.sqrt(float(n * s2 - s1 * s1)) / n)


def top_pair(col, med, k):
    """None where fewer than k + 1 values exceed the median"""
    n = len(col)
    above = sum(1 for v in col if np.float32(v) > np.float32(med))
    if k == 0 or k + 1 > above:
        return None
    lo, hi = select_pair(col, n - k - 1)
    return (np.float32(lo) + np.float32(hi)) / np.float32(2)


def columns():
    """(name, column) - every shape of column the selection can go wrong on"""
    rng = np.random.default_rng(77)
    out = [
        ("n1", [40000]), ("n1_zero", [0]), ("n2", [7, 65535]), ("n2_equal", [9, 9]), ("n3", [5, 1, 3]), ("n3_ties", [4, 4, 9]),
        ("all_equal_even", [1234] * 8), ("all_equal_odd", [65535] * 7), ("all_zero", [0] * 6),
        ("extremes_even", [0, 65535] * 5), ("extremes_odd", [0, 65535] * 5 + [0]), ("extremes_more_high", [65535] * 6 + [0] * 4),
        ("ties_straddle_middle", [3, 8, 8, 8, 8, 20]), ("ties_below_middle", [8, 8, 8, 9, 10, 11]), ("ties_above_middle", [1, 2, 3, 8, 8, 8]),
        ("second_rank_equals_first", [1, 5, 5, 9]), ("second_rank_is_next", [1, 5, 6, 9]), ("second_rank_far", [0, 1, 65535, 65535]),
        ("one_bit_apart", [32767, 32768] * 4), ("descending", list(range(20, 0, -1))), ("ascending_odd", list(range(1, 22))),
        ("high_bit_only", [32768, 0, 32768, 0, 32768]),
    ]
    for n in (4, 5, 20, 21, 64, 65, 100):
        out.append(("random_full_n%d" % n, rng.integers(0, 65536, n).tolist()))
        out.append(("random_narrow_n%d" % n, rng.integers(100, 104, n).tolist()))
    return [(name, np.array(c, np.uint16)) for name, c in out]


def reference_pair(col, r):
    s = np.sort(np.asarray(col))
    return int(s[r]), int(s[min(r + 1, len(s) - 1)])


def reference_top_pair(col, med, k):
    """the reference's _get_pixel_thresh_2 for one pixel, restated by intent: pull the largest value above the median k + 1 times"""
    v = sorted((int(x) for x in col if np.float32(x) > np.float32(med)), reverse=True)
    if k == 0 or len(v) < k + 1:
        return None
    return (np.float32(v[k]) + np.float32(v[k - 1])) / np.float32(2)
