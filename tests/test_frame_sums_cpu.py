"""Summed views without a GPU: the viewer's window plan is a pure function of the part files' frame-id arrays, and the device accumulator
fails loudly where there is no device."""
import numpy as np
import pytest

from conftest import load_npz


def test_window_plan_over_part_files_with_gaps_in_their_ids():
    """G7's two part files (the reference's stream-mode writer on 2 nodes: ids ascend inside a part, with gaps) under fractionation 5: the
    windows [0, 5), [5, 10), [10, 15) hold five frames each, [15, 20) the one that is left; a part's share of a window is one contiguous
    record range; the next window starts behind the largest id found; then the plan is exhausted."""
    from pyrecode_amd.utils.viewer import plan_view
    g = load_npz("g7_stream.npz")
    ids = [g["ids_part0"], g["ids_part1"]]
    assert ids[0].tolist() == [0, 1, 2, 5, 6, 9, 10, 11, 12] and ids[1].tolist() == [3, 4, 7, 8, 13, 14, 15]
    want = [(0, [(0, 3), (0, 2)], 5, 5), (5, [(3, 6), (2, 4)], 5, 10), (10, [(6, 9), (4, 6)], 5, 15), (15, [(9, 9), (6, 7)], 1, 16)]
    start, seen = 0, []
    for at, ranges, count, nxt in want:
        assert start == at
        got = plan_view(ids, start, 5)
        assert got == (ranges, count, nxt)
        for part, (lo, hi) in zip(ids, got[0]):
            assert all(start <= int(i) < start + 5 for i in part[lo:hi])
            seen += part[lo:hi].tolist()
        start = got[2]
    assert sorted(seen) == list(range(16))
    assert plan_view(ids, start, 5) is None
    # a window no frame falls into, with frames behind it: nothing to add, and the plan moves on by one window
    assert plan_view([np.array([0, 1, 40])], 2, 5) == ([(2, 2)], 0, 7)
    with pytest.raises(ValueError):
        plan_view(ids, 0, 0)


def test_frame_sum_without_a_gpu_fails_loudly():
    from pyrecode_amd import _lib
    if _lib.device_count() > 0:
        pytest.skip("a GPU is visible")
    with pytest.raises(_lib.RecodeHipError, match="no CPU path"):
        _lib.FrameSum(64, 64)
