"""The exact model of counted views (rc_count.h: cnt_place, cnt_finish_fine; rc_count.hip: k_cnt_place) - CPU code,
numpy, scipy and Python's unbounded integers.  Not a test.

place is the definition itself: pixel centres at integers, fine cell k of an axis with its centre at (k - (s - 1) / 2) / s, the cell
whose centre is nearest to the centroid S / w, ties to the even index - the rational (2 s S + (s - 1) w) / (2 w) rounded half to even.
counted_view is what rc_sum_add_counted adds to a zeroed handle, compared by `==`: components, sums, the weight-0 fallback and the
maximum's raster rule as in centroid_model.count_frame."""
import numpy as np
import scipy.ndimage as nd

import centroid_model as cm


def place(S, w, s):
    """index on the grid s times finer of the cell nearest to S / w (Python integers, w > 0)"""
    S, w, s = int(S), int(w), int(s)
    num, den = 2 * s * S + (s - 1) * w, 2 * w
    q, r = divmod(num, den)
    if 2 * r > den or (2 * r == den and q % 2 == 1):
        q += 1
    return q


def is_tie(S, w, s):
    """whether place(S, w, s) had two nearest cells to choose from"""
    num, den = 2 * int(s) * int(S) + (int(s) - 1) * int(w), 2 * int(w)
    return 2 * (num % den) == den


def frame_components(binary, value, method="weighted_average", area_threshold=0):
    """[(row numerator, col numerator, denominator)] - Python integers - of one frame's kept components, in scipy's label order: the sums
    the method divides, the unweighted ones for a weighted component of weight 0, (row, col, 1) of the winning pixel for the maximum"""
    assert method in cm.METHODS
    binary = np.asarray(binary, bool)
    labels, n = nd.label(binary, structure=cm.EIGHT)
    if n == 0:
        return []
    r, c = np.nonzero(binary)                                   # raster order
    lab = labels[r, c] - 1
    v = np.asarray(value)[r, c].astype(np.int64)
    r, c = r.astype(np.int64), c.astype(np.int64)

    def total(x):
        out = np.zeros(n, np.int64)
        np.add.at(out, lab, x)
        return out.tolist()
    area, weight = total(np.ones_like(v)), total(v)
    sr, sc, wr, wc = total(r), total(c), total(v * r), total(v * c)
    if method == "max":
        order = np.lexsort((-v, lab))                           # the largest v, the first in raster order among equals
        hit = order[np.searchsorted(lab[order], np.arange(n))]
        comps = [(int(r[i]), int(c[i]), 1) for i in hit]
    elif method == "weighted_average":
        comps = [(wr[k], wc[k], weight[k]) if weight[k] > 0 else (sr[k], sc[k], area[k]) for k in range(n)]
    else:
        comps = [(sr[k], sc[k], area[k]) for k in range(n)]
    return [comps[k] for k in range(n) if area[k] > area_threshold]


def components(frames, method="weighted_average", area_threshold=0):
    """frames = [(binary, value)]: frame_components of each - what does not depend on the upsampling"""
    return [frame_components(b, v, method, area_threshold) for b, v in frames]


def view_of(comps, shape, s=1, ties=None):
    """uint64[s * ny, s * nx], one count per component of components(); ties: a list that receives the number placed on a tie"""
    ny, nx = shape
    view = np.zeros((s * ny, s * nx), np.uint64)
    n_ties = 0
    for frame in comps:
        for a, b, w in frame:
            view[place(a, w, s), place(b, w, s)] += 1          # (an index outside the view raises: a centroid lies inside its frame)
            n_ties += is_tie(a, w, s) or is_tie(b, w, s)
    if ties is not None:
        ties.append(n_ties)
    return view


def counted_view(frames, method="weighted_average", area_threshold=0, s=1, ties=None):
    """frames = [(binary, value)] of one shape: what rc_sum_add_counted adds to a zeroed handle of (s * nx) x (s * ny) cells"""
    return view_of(components(frames, method, area_threshold), np.shape(frames[0][0]), s, ties)


def events_prefix(frames, method="weighted_average", area_threshold=0):
    """uint64[n + 1]: the frames' event prefix, as rc_sum_add_counted returns it"""
    return cm.count_batch(frames, method, area_threshold)[0]
