"""Converters between reduction levels (reference: pyrecode/utils/converters.py).  l1_to_l4_converter counts electrons - every 8-connected
puddle of a level-1 frame's set pixels becomes one event at its centroid - with the labelling and the per-component sums on the device
(rc_count_frames); the reference labels with scipy and sums in numba, a frame at a time on the host.
recalibrate_l1 is not offered: it adds a calibration difference to EVERY pixel, unset ones included, so it works on dense frames -
which the reader can deliver now (ReCoDeReader.get_frames_dense), but re-thresholding and re-encoding them is a
feature of its own."""
import copy
from datetime import datetime

import numpy as np
from scipy.sparse import coo_matrix

from .. import _lib
from ..reader_batched import count_frames_now, count_method

_BATCH_FRAMES = 64            # frames per device call ...
_BATCH_PIXELS = 1 << 28       # ... as long as their binary maps stay within this many pixels


def _stored_batch(frames, shape):
    """the frames (COO matrices of one shape, unsigned values) as the stored pieces of a level-1 batch - per frame the binary map, packed
    LSB first, then its values in raster order as d-bit fields at the narrowest d that holds the batch's largest value (the layout
    recode_writer.py:637-652 packs): (d, bytes, sizes uint32[k][3])"""
    ny, nx = shape
    nb = (ny * nx + 7) // 8
    cells = []
    for m in frames:
        m = m.tocoo()
        if m.dtype.kind != 'u':
            raise NotImplementedError('l1_to_l4_converter: frames of unsigned integer values (got %s)' % m.dtype)
        if m.shape != (ny, nx):
            raise ValueError('l1_to_l4_converter: a frame of shape %s, frame_shape is %s' % (m.shape, (ny, nx)))
        idx = m.row.astype(np.int64) * nx + m.col
        if idx.size and np.unique(idx).size != idx.size:
            m = m.copy()
            m.sum_duplicates()
            idx = m.row.astype(np.int64) * nx + m.col
        order = np.argsort(idx, kind='stable')
        cells.append((idx[order], m.data[order].astype(np.uint32)))
    top = max([int(v.max()) for _, v in cells if v.size] + [1])
    if top >= 1 << 16:
        raise NotImplementedError('l1_to_l4_converter: values of more than 16 bits')
    d = max(top.bit_length(), 1)
    shifts = np.arange(d, dtype=np.uint32)
    sizes, parts = np.zeros((len(cells), 3), np.uint32), []
    for i, (idx, vals) in enumerate(cells):
        dense = np.zeros(ny * nx, bool)
        dense[idx] = True
        packed = np.packbits(((vals[:, None] >> shifts) & 1).astype(np.uint8).reshape(-1), bitorder='little')
        parts += [np.packbits(dense, bitorder='little'), packed]
        sizes[i] = nb, packed.size, packed.size
    return d, np.ascontiguousarray(np.concatenate(parts)), sizes


def l1_to_l4_converter(l1_frames, frame_shape, n_frames=-1, area_threshold=0, verbosity=0, method='weighted_average', in_place=False):
    """The reference's l1_to_l4_converter (utils/converters.py:59-123), signature, prints and result: l1_frames is the dictionary a
    reader's get_frame / get_frames builds, {frame_id: {'metadata': ..., 'data': COO}}; returned is {frame_id: {the frame's other entries -
    deep copies, or with in_place the frame's own dictionary, whose 'data' is replaced -, 'data': coo_matrix of bool, shape frame_shape}}
    with one True per event.  Two events of a frame on one pixel are two entries of the matrix.
    The frames' stored pieces are rebuilt from the matrices and go to rc_count_frames in batches; there is no CPU path (no GPU:
    RuntimeError).  Deliberate differences from the reference:
    - foreground is what the matrix STORES (the binary map of a level-1 frame), a stored zero included; the reference takes frame > 0;
    - the sums are exact integers and the centroid is the exact rational rounded half to even; the reference accumulates in float32;
    - an event is at (row, col); the reference hands (col, row) to coo_matrix as (row, col) (:100-101);
    - 'unweighted_average' and 'max' do what _get_centroids_2d_nb_u / _nb_m were written for; the reference sends every name to the
      weighted helper (:157-164);
    - n_frames > 0 converts the first n_frames frames; the reference converts n_frames + 1 (:119-120).
    Values that are not unsigned integers, or wider than 16 bits, raise NotImplementedError."""
    code = count_method(method)
    ny, nx = int(frame_shape[0]), int(frame_shape[1])
    n_pixels = ny * nx * 1.
    keys = list(l1_frames.keys())
    if n_frames > 0:
        keys = keys[:n_frames]
    per_call = max(1, min(_BATCH_FRAMES, _BATCH_PIXELS // max(ny * nx, 1)))
    cd = {}
    stats_shown = False
    avg_dose_rate = 0.0
    frame_count = 0
    start_time = datetime.now()
    for a in range(0, len(keys), per_call):
        s1 = datetime.now()
        batch = keys[a:a + per_call]
        k = len(batch)
        d, pieces, sizes = _stored_batch([l1_frames[key]['data'] for key in batch], (ny, nx))
        geom = (nx, ny, d, 1, 0, 0)
        st, prefix, events = count_frames_now(geom, pieces, sizes, k, code, int(area_threshold))
        _lib.check(st, 'rc_count_frames')
        features = prefix
        if area_threshold > 0:      # (the dose rate counts every component, as the reference's num_features does)
            features = np.zeros(k + 1, np.uint64)
            _lib.check(_lib.lib().rc_count_frames(*geom, _lib.ptr(pieces), _lib.ptr(sizes), k, code, 0, _lib.ptr(features), None, 0), 'rc_count_frames')
        rows, cols = events[0], events[1]
        t1 = (datetime.now() - s1) / k
        for i, key in enumerate(batch):
            lo, hi = int(prefix[i]), int(prefix[i + 1])
            if in_place:
                cd[key] = l1_frames[key]
            else:
                cd[key] = {name: copy.deepcopy(value) for name, value in l1_frames[key].items() if name != 'data'}
            if hi > lo:
                cd[key]['data'] = coo_matrix((np.ones(hi - lo, bool), (rows[lo:hi].copy(), cols[lo:hi].copy())), shape=(ny, nx), dtype=bool)
            else:
                cd[key]['data'] = coo_matrix((ny, nx), dtype=bool)
            num_features = int(features[i + 1] - features[i])
            if verbosity > 0:
                print(key)
                print('Dose Rate =', num_features / n_pixels)
                print('Processing time: ' + str(t1) + ' (per frame of its batch)')
            else:
                avg_dose_rate += num_features / n_pixels
                if isinstance(key, (int, np.integer)) and key > 100 and not stats_shown and frame_count:
                    print('Avg. Dose Rate (First {0:d} frames) = {1:0.4f}'.format(frame_count, avg_dose_rate / frame_count))
                    print('Processing time  (First ' + str(frame_count) + ' frames) = ' + str(datetime.now() - start_time))
                    stats_shown = True
            frame_count += 1
    print('Total processing time: ' + str(datetime.now() - start_time))
    return cd
