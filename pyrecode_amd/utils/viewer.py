"""ReCoDeViewer: summed views over the part files of a run - the reference's pyrecode/utils/viewer.py on the device.

The reference reads `fractionation` frames ahead from every part file, picks the frames whose ids fall into the window
[start, start + fractionation) and adds their dense forms on the host (viewer.py:40-75).  Here a part file's share of a window is one
contiguous range of its records (ids ascend inside a part - the reference's stated assumption, viewer.py:58), every part adds its range into
ONE device accumulator (ReCoDeReader.sum_frames(into=FrameSum)), and the view that comes back is 4 bytes per pixel.

Deviations from the reference, both on purpose:
  * the view is (ny, nx); the reference allocates np.zeros((nx, ny)) and can therefore only add square frames (viewer.py:65-68)
  * only part files that are complete when the viewer opens them are read: a part's records are indexed once, at open, and a file that is
    still growing is seen as it was then.  (The reference's _get_next_frame_safely is a stub that does not handle it either.)
get_next_view() returns None once every part is exhausted, where the reference raises on np.max of nothing (viewer.py:73).
The device's cells are uint32 and never wrap: a window whose sum COULD pass 2^32 - 1 - fractionation * (2^bit_depth - 1) at level 1, i.e.
more than 65 537 frames of 16 bits, or 1 048 832 of 12 - raises ValueError; the view is reset and the window stays the next one.

counting (not in the reference): ReCoDeViewer(..., counting=dict(area_threshold=0, method='weighted_average', upsample=1)) - any subset of
the keys - makes every view the COUNTED image of its window (ReCoDeReader.sum_frames_counted): one count per electron event, on a grid
`upsample` times finer than the sensor's; get_shape() is then (upsample * ny, upsample * nx).

shifts (not in the reference): ReCoDeViewer(..., shifts=table) - an integer array indexed by frame ID, shape (>= largest id + 1, 2), row id =
(dy, dx) - makes every view an ALIGNED one: each frame is translated by its row before it is added, what leaves the view is dropped
(ReCoDeReader.sum_frames(shifts=)).  Whole pixels for plain views; with counting= the units are fine cells (1 / upsample pixel).  An id beyond
the table is a ValueError at the window that needs it.
"""
import os

import numpy as np


def plan_view(part_ids, start, fractionation):
    """The window [start, start + fractionation) over the parts' frame ids - a pure function of the id arrays (ascending inside a part).
    Returns None when no part holds an id >= start (exhausted), else (ranges, n_frames, next_start): ranges[i] = (lo, hi), the records of
    part i inside the window; n_frames their number; next_start the largest id found plus one (viewer.py:73) - or, for a window that no
    frame falls into while later ones exist, the window's end."""
    start, stop = int(start), int(start) + int(fractionation)
    if fractionation <= 0:
        raise ValueError('fractionation must be positive')
    ranges, last, left = [], -1, False
    for ids in part_ids:
        ids = np.asarray(ids)
        lo, hi = int(np.searchsorted(ids, start, 'left')), int(np.searchsorted(ids, stop, 'left'))
        ranges.append((lo, hi))
        left = left or lo < len(ids)
        if hi > lo:
            last = max(last, int(ids[hi - 1]))
    if not left:
        return None
    n_frames = sum(hi - lo for lo, hi in ranges)
    return ranges, n_frames, (last + 1 if n_frames else stop)


def shifts_for_ids(table, ids):
    """rows of the viewer's shift table for the frame ids of a part's share of a window - a pure function.  ValueError: an id the table
    does not reach."""
    ids = np.asarray(ids, np.int64)
    if ids.size and (int(ids.max()) >= table.shape[0] or int(ids.min()) < 0):
        raise ValueError('shifts: frame id %d needs a table of at least %d rows, it has %d'
                         % (int(ids.max()), int(ids.max()) + 1, table.shape[0]))
    return table[ids]


class ReCoDeViewer:

    def __init__(self, folder_path, base_filename, num_parts, fractionation, counting=None, shifts=None):
        from .. import _lib
        from ..recode_reader import ReCoDeReader
        self._fractionation = int(fractionation)
        self._counting = None
        if counting is not None:
            unknown = set(counting) - {'area_threshold', 'method', 'upsample'}
            if unknown:
                raise ValueError('counting: unknown keys %s' % sorted(unknown))
            self._counting = dict(dict(area_threshold=0, method='weighted_average', upsample=1), **counting)
        self._shifts = None
        if shifts is not None:
            self._shifts = _lib.shift_rows(shifts, None, 'ReCoDeViewer: shifts')
        self._readers = []
        self._frame_start = 0
        self._sum = None
        try:
            for i in range(int(num_parts)):
                rd = ReCoDeReader(os.path.join(folder_path, '%s_part%03d' % (base_filename, i)), is_intermediate=True)
                rd.open(print_header=False)
                self._readers.append(rd)
                rd._batch_frames()                               # indexes the part's records: part_frame_ids
            s = int(self._counting['upsample']) if self._counting else 1
            _, self._ny, self._nx = (s * int(v) for v in self._readers[0].get_shape())
            self._sum = _lib.FrameSum(self._nx, self._ny)
        except Exception:
            self.close()
            raise

    def get_shape(self):
        """(ny, nx) of a view"""
        return self._ny, self._nx

    def get_next_view(self):
        plan = plan_view([rd.part_frame_ids for rd in self._readers], self._frame_start, self._fractionation)
        if plan is None:
            return None
        ranges, n_frames, next_start = plan
        # (every part's rows before anything is added: an id the table does not reach leaves the view untouched)
        shifted = [None if self._shifts is None or hi <= lo else shifts_for_ids(self._shifts, rd.part_frame_ids[lo:hi])
                   for rd, (lo, hi) in zip(self._readers, ranges)]
        try:
            for rd, (lo, hi), rows in zip(self._readers, ranges, shifted):
                if hi > lo and self._counting:
                    rd.sum_frames_counted(lo, hi - lo, into=self._sum, shifts=rows, **self._counting)
                elif hi > lo:
                    rd.sum_frames(lo, hi - lo, into=self._sum, shifts=rows)
        except Exception:
            self._sum.fetch_view(reset=True)                     # (what earlier parts added is no view: start the window afresh)
            raise
        if n_frames < self._fractionation:                       # (the reference's message, viewer.py:62-63)
            print("Warning: read fewer frames (%d) than requested (%d)." % (n_frames, self._fractionation))
        view = self._sum.fetch_view(reset=True).astype(np.float64)    # (exact: the cells are integers below 2^32)
        out = {'start': self._frame_start, 'n_Frames': n_frames, 'view': view}
        self._frame_start = next_start
        return out

    def close(self):
        for rd in self._readers:
            rd.close()
        self._readers = []
        if self._sum is not None:
            self._sum.close()
            self._sum = None
