"""The exact model of electron counting (tests/centroid_model.py) is itself under test: hand-worked cases with their expectations written
out, the model against the closed forms of the level-2 topology catalogue (no labelling routine on that side), and its weighted average
against a float32 restatement of the reference's accumulation on inputs where the reference's rounding cannot matter."""
import numpy as np
import pytest

import centroid_model as cm
import l2_topologies as lt


def frame(ny, nx, cells):
    """cells = {(row, col): value}"""
    b, v = np.zeros((ny, nx), bool), np.zeros((ny, nx), np.uint16)
    for (r, c), x in cells.items():
        b[r, c], v[r, c] = True, x
    return b, v


def events(b, v, method="weighted_average", thr=0):
    rows, cols, area, weight = cm.count_frame(b, v, method, thr)
    return list(zip(rows.tolist(), cols.tolist(), area.tolist(), weight.tolist()))


def test_rhe_rounds_ties_to_even():
    assert cm.rhe(np.array([0, 1, 2, 3, 5, 7, 9, 10]), np.array([2, 2, 2, 2, 2, 2, 2, 4])).tolist() == [0, 0, 1, 2, 2, 4, 4, 2]
    assert cm.rhe(np.array([7, 8, 10, 11]), np.array([3, 3, 4, 4])).tolist() == [2, 3, 2, 3]


def test_single_pixel():
    b, v = frame(4, 5, {(2, 3): 9})
    for m in cm.METHODS:
        assert events(b, v, m) == [(2, 3, 1, 9)]
    assert events(b, v, thr=1) == []


def test_vertical_pair_ties_go_to_the_even_row():
    for r, want in ((2, 2), (3, 4)):                  # rows (2, 3): 2.5 -> 2; rows (3, 4): 3.5 -> 4
        b, v = frame(7, 3, {(r, 1): 5, (r + 1, 1): 5})
        assert events(b, v) == [(want, 1, 2, 10)]
        assert events(b, v, "unweighted_average") == [(want, 1, 2, 10)]
        assert events(b, v, "max") == [(r, 1, 2, 10)]


def test_weights_three_to_one():
    b, v = frame(3, 8, {(1, 2): 3, (1, 3): 1})       # col = (6 + 3) / 4 = 2.25 -> 2; unweighted 2.5 -> 2
    assert events(b, v) == [(1, 2, 2, 4)]
    b, v = frame(3, 8, {(1, 2): 1, (1, 3): 3})       # col = (2 + 9) / 4 = 2.75 -> 3
    assert events(b, v) == [(1, 3, 2, 4)]
    assert events(b, v, "unweighted_average") == [(1, 2, 2, 4)]
    assert events(b, v, "max") == [(1, 3, 2, 4)]


def test_l_shape():
    # (0,0) (1,0) (2,0) (2,1) (2,2), all 1: rows 7 / 5 = 1.4 -> 1, cols 3 / 5 = 0.6 -> 1: the event lies OUTSIDE the component
    b, v = frame(4, 4, {(0, 0): 1, (1, 0): 1, (2, 0): 1, (2, 1): 1, (2, 2): 1})
    assert events(b, v) == [(1, 1, 5, 5)]
    # the corner weighs 10: rows (1 + 20 + 2 + 2) / 14 = 25 / 14 -> 2, cols (1 + 2) / 14 -> 0
    v[2, 0] = 10
    assert events(b, v) == [(2, 0, 5, 14)]
    assert events(b, v, "max") == [(2, 0, 5, 14)]
    assert events(b, v, thr=4) == [(2, 0, 5, 14)] and events(b, v, thr=5) == []


def test_two_components_land_on_one_pixel_and_both_stay():
    # a ring's hole holds a single pixel: both centroids are (2, 2); the ring's first pixel comes first
    cells = {(r, c): 1 for r in range(5) for c in range(5) if r in (0, 4) or c in (0, 4)}
    cells[(2, 2)] = 7
    b, v = frame(5, 5, cells)
    assert events(b, v) == [(2, 2, 16, 16), (2, 2, 1, 7)]


def test_weight_zero_falls_back_to_the_unweighted_average():
    b, v = frame(4, 6, {(1, 1): 0, (1, 2): 0, (1, 3): 0, (3, 5): 0})
    assert events(b, v) == [(1, 2, 3, 0), (3, 5, 1, 0)]
    assert events(b, v, "max") == [(1, 1, 3, 0), (3, 5, 1, 0)]
    b, v = frame(4, 6, {(1, 1): 0, (1, 2): 0, (1, 3): 4})      # one weight is enough: the zeros no longer count
    assert events(b, v) == [(1, 3, 3, 4)]


def test_max_takes_the_first_of_equal_maxima():
    b, v = frame(3, 6, {(1, 1): 2, (1, 2): 9, (1, 3): 9, (0, 4): 9})      # raster order: (0, 4) is first
    assert events(b, v, "max") == [(0, 4, 4, 29)]
    b, v = frame(3, 6, {(1, 1): 2, (1, 2): 9, (1, 3): 9})
    assert events(b, v, "max") == [(1, 2, 3, 20)]


def test_no_link_wraps_around_a_row_end():
    b, v = frame(3, 4, {(0, 3): 1, (1, 0): 1})
    assert events(b, v) == [(0, 3, 1, 1), (1, 0, 1, 1)]


@pytest.mark.parametrize("ny,nx", [lt.SMALL, (127, 130)])
@pytest.mark.parametrize("name", list(lt.CLOSED_FORM))
def test_model_weight_and_count_are_the_closed_forms(name, ny, nx):
    t = lt.CLOSED_FORM[name](ny, nx, 1)
    c = t.stats(t.value)
    for m in cm.METHODS:
        rows, cols, area, weight = cm.count_frame(t.binary, t.value, m)
        assert rows.size == c.count
        assert np.array_equal(weight.astype(np.int64), c.total)
        assert int(area.sum()) == int(t.binary.sum())
    if c.count:     # the events' order is the order of the components' first pixels: 'max' over an image that peaks there says so
        peak = np.zeros((ny, nx), np.uint16)
        peak.ravel()[c.first] = 1
        rows, cols, _, _ = cm.count_frame(t.binary, peak, "max")
        assert np.array_equal(rows.astype(np.int64) * nx + cols, c.first)


FLOAT32_CASES = [((192, 256), 12, 0.01), ((127, 130), 12, 0.04), ((192, 256), 16, 0.04), ((66, 4100), 16, 0.02), ((530, 517), 16, 0.03)]


@pytest.mark.parametrize("shape,d,p", FLOAT32_CASES)
def test_exact_model_is_the_float32_accumulation_where_rounding_cannot_matter(shape, d, p):
    """small components of values below 2^16: the float32 sums are exact or nearly so, and a centroid is never within float32's error of a
    tie that the sums do not hit exactly - 0 differences"""
    b, v = cm.bernoulli_frame(shape[0], shape[1], d, p, seed=7)
    rows, cols, _, weight = cm.count_frame(b, v)
    assert rows.size > 400 and weight.min() > 0
    frows, fcols = cm.float32_frame(b, v)
    assert int((frows != rows).sum() + (fcols != cols).sum()) == 0
