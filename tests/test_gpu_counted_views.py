"""-m gpu: counted views (rc_sum_add_counted / _submit, pyrecode_amd/csrc/rc_count.hip: k_cnt_place).  Stored batches built with numpy
through the C ABI at every level, depth, upsampling and method; ties, stored zeros, cells that several components share, the area
threshold; what a handle does across calls, slots and kinds of add; the refusals; ReCoDeReader.sum_frames_counted /
iter_frame_sums_counted on golden files; ReCoDeViewer with counting.  The expectation is the exact model (tests/counted_view_model.py),
every comparison is np.array_equal on the whole view."""
import os
import shutil

import numpy as np
import pytest

import centroid_model as cm
import counted_view_model as cv
import l2_topologies as lt
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
FILES = os.path.join(GOLDEN, "files")


@pytest.fixture(scope="module")
def hip():
    from pyrecode_amd import _lib
    if _lib.device_count() == 0:
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    return _lib


def _geom(shape, level, d):
    return (shape[1], shape[0], d, level, 0, 0)


def _model_frames(frames, level):
    return frames if level == 1 else [(b, np.ones(np.shape(b), np.uint16)) for b, _ in frames]


class _Views:
    """one handle per upsampling of a shape, reset between uses"""

    def __init__(self, hip, shape):
        self.hip, self.shape, self.fs = hip, shape, {}

    def __call__(self, s):
        if s not in self.fs:
            self.fs[s] = self.hip.FrameSum(s * self.shape[1], s * self.shape[0])
        return self.fs[s]

    def close(self):
        for fs in self.fs.values():
            fs.close()


def _check(hip, views, level, d, frames, thr=0, methods=(0, 1, 2), ups=(1, 2, 3, 4), ties=None):
    """frames = [(binary, value)] through the synchronous call for each method and upsampling, into a zeroed handle, against the model:
    the view, the event prefix and the bound's growth"""
    shape = views.shape
    data, sizes = cm.stored_batch(frames, level, d)
    n = len(frames)
    grow = hip.FrameSum.grows_by_counted(_geom(shape, level, d), sizes, n)
    want = None
    for method in methods:
        comps = cv.components(_model_frames(frames, level), cm.METHODS[method], thr)
        prefix_want = np.concatenate([[0], np.cumsum([len(c) for c in comps])]).astype(np.uint64)
        for s in ups:
            want = cv.view_of(comps, shape, s, ties)
            fs = views(s)
            prefix = np.full(n + 1, 77, np.uint64)
            st = fs.add_counted_status(_geom(shape, level, d), data, sizes, n, method, thr, s, prefix)
            assert st == hip.RC_OK, (st, hip.last_error())
            assert fs.bound() == grow
            got = fs.fetch(reset=True)
            assert fs.bound() == 0
            assert np.array_equal(prefix, prefix_want), (method, s, prefix, prefix_want)
            assert got.shape == want.shape and np.array_equal(got, want), "method %d, upsample %d: %d cells differ, first at %s" % (
                method, s, int((got != want).sum()), np.argwhere(got != want)[:4].tolist())
    return want


# ---- 1. stored streams through the C ABI -------------------------------------------------------------------------------------------------
def _kind(k, ny, nx, d, seed):
    """the frame kinds of a batch in turn: 4 % Bernoulli, a tenth of the set values 0 | every pixel at 2^d - 1 | empty"""
    if k % 3 == 0:
        return cm.bernoulli_frame(ny, nx, d, 0.04, seed, zero_fraction=0.1)
    if k % 3 == 1:
        return np.ones((ny, nx), bool), np.full((ny, nx), (1 << d) - 1, np.uint16)
    return np.zeros((ny, nx), bool), np.zeros((ny, nx), np.uint16)


@pytest.mark.parametrize("level,d", [(1, 9), (1, 12), (1, 16), (2, 12), (3, 0)])
@pytest.mark.parametrize("shape", [(1, 1), (3, 21), (5, 65), (127, 130), (530, 517)])
def test_stored_streams(hip, shape, level, d):
    """less than a word; one column past a word; rows that are not word-aligned, 2 blocks; 17 blocks with components that span workgroups.
    Batches of 1 and 3 frames - random, full (one component, the sums at their largest), empty -, every method, upsample 1..4, and 16 at
    (3, 21)."""
    ny, nx = shape
    dv = d if level == 1 else 8
    frames = [_kind(k, ny, nx, dv, 200 + k) for k in range(3)]
    views = _Views(hip, shape)
    try:
        _check(hip, views, level, d if d else 8, frames[:1])
        _check(hip, views, level, d if d else 8, frames)
        _check(hip, views, level, d if d else 8, frames[1:2], ups=(1, 3))          # the full frame alone
        if shape == (3, 21):
            _check(hip, views, level, d if d else 8, frames, ups=(16,))
    finally:
        views.close()


# ---- 2. constructed inputs ---------------------------------------------------------------------------------------------------------------
def test_ties(hip):
    """equal-valued dominoes at even and at odd x (and y), horizontal and vertical: the centroid lies half-way between two cell centres at
    every upsampling, and the model says so before the device is asked"""
    shape = (12, 70)
    b, v = np.zeros(shape, bool), np.full(shape, 7, np.uint16)
    for k, x in enumerate((0, 3, 10, 63, 64, 67)):          # horizontal, even and odd x
        b[3 * (k % 4), x:x + 2] = True
    for k, (y, x) in enumerate(((0, 20), (3, 23), (6, 26), (9, 29), (4, 40), (7, 43))):      # vertical, even and odd y
        b[y:y + 2, x] = True
    n_dominoes = 12
    views = _Views(hip, shape)
    try:
        for level in (1, 3):
            ties = []
            _check(hip, views, level, 12, [(b, v)], methods=(0, 1), ups=(1, 2, 3, 4, 5, 8), ties=ties)
            assert ties == [n_dominoes] * 12
    finally:
        views.close()


def test_stored_zeros_take_the_unweighted_fallback(hip):
    shape = (20, 66)
    b, v = cm.bernoulli_frame(20, 66, 12, 0.2, 9)
    v[:, :40] = 0                                          # components of nothing but stored zeros, and mixed ones at the seam
    comps_w, comps_u = cv.frame_components(b, v, "weighted_average"), cv.frame_components(b, v, "unweighted_average")
    assert sum(cw == cu for cw, cu in zip(comps_w, comps_u)) > 20 and comps_w != comps_u
    views = _Views(hip, shape)
    try:
        _check(hip, views, 1, 12, [(b, v), (b, np.zeros(shape, np.uint16))])
    finally:
        views.close()


def test_components_that_share_a_cell(hip):
    """nested rings have one centroid: the model's view holds a cell of at least 2 before the device's is compared with it"""
    t = lt.CATALOGUE["rings"](lt.SMALL[0], lt.SMALL[1], 0)
    views = _Views(hip, lt.SMALL)
    try:
        for s in (1, 2, 3, 4):
            assert int(cv.counted_view([(t.binary, t.value)], "unweighted_average", 0, s).max()) >= 2
        _check(hip, views, 1, 16, [(t.binary, t.value)], methods=(1,))
        _check(hip, views, 1, 16, [(t.binary, t.value)] * 3)
    finally:
        views.close()
    shape = (7, 9)                                         # a ring around a dot
    b = np.zeros(shape, bool)
    b[1:6, 2:7] = True
    b[2:5, 3:6] = False
    b[3, 4] = True
    views = _Views(hip, shape)
    try:
        assert int(cv.counted_view([(b, b.astype(np.uint16))], "unweighted_average", 0, 4).max()) == 2
        _check(hip, views, 3, 8, [(b, b.astype(np.uint16))], methods=(0, 1))
    finally:
        views.close()


def test_area_threshold(hip):
    shape = (40, 70)
    b, v = np.zeros(shape, bool), np.random.default_rng(4).integers(1, 4096, shape).astype(np.uint16)
    for k in range(25):              # horizontal runs of 1 .. 5 pixels, apart
        r, c, area = 2 * (k // 5) + 1, 13 * (k % 5) + 1, 1 + k % 5
        b[r, c:c + area] = True
    views = _Views(hip, shape)
    try:
        for thr, kept in ((0, 25), (1, 20), (3, 10), (1000, 0)):
            want = _check(hip, views, 1, 12, [(b, v), (b[::-1].copy(), v)], thr=thr, ups=(1, 3))
            assert int(want.sum()) == 2 * kept
    finally:
        views.close()


# ---- 3. the handle -----------------------------------------------------------------------------------------------------------------------
def _batches(shape, d, count, n=3, p=0.03):
    return [[cm.bernoulli_frame(shape[0], shape[1], d, p, 10 * j + z) for z in range(n)] for j in range(count)]


def test_calls_add_up_and_plain_and_counted_adds_share_a_handle(hip):
    shape, d = (127, 130), 12
    a, b = _batches(shape, d, 2)
    g = _geom(shape, 1, d)
    fs = hip.FrameSum(130, 127)
    try:
        grown = 0
        for frames, method in ((a, 0), (b, 2)):
            data, sizes = cm.stored_batch(frames, 1, d)
            prefix = fs.add_counted(g, data, sizes, 3, method, 0, 1)
            assert np.array_equal(prefix, cv.events_prefix(frames, cm.METHODS[method]))
            grown += hip.FrameSum.grows_by_counted(g, sizes, 3)
            assert fs.bound() == grown
        want = cv.counted_view(a, "weighted_average") + cv.counted_view(b, "max")
        assert np.array_equal(fs.fetch(), want)
        data, sizes = cm.stored_batch(a, 1, d)
        fs.add(g, data, sizes, 3)                                          # the plain sum of the same frames, on top
        want = want + sum(np.where(bb, vv, 0).astype(np.uint64) for bb, vv in a)
        assert fs.bound() == grown + 3 * 4095 and np.array_equal(fs.fetch(), want)
        assert np.array_equal(fs.fetch(reset=True), want) and fs.bound() == 0 and not fs.fetch().any()
        fs.add_counted(g, data, sizes, 3, 1, 2, 1)
        assert np.array_equal(fs.fetch(), cv.counted_view(a, "unweighted_average", 2))
    finally:
        fs.close()


def test_bound_grows_by_the_stated_rule(hip):
    """per frame min(ceil(nx / 2) * ceil(ny / 2), floor(8 * value bytes / depth)) at level 1 - restated here, not taken from the binding -,
    the first term alone at levels 2 and 3"""
    shape = (5, 65)
    blocks = 3 * 33
    sparse = np.zeros(shape, bool)
    sparse[2, 3:8] = True
    frames = [(sparse, np.full(shape, 5, np.uint16)), (np.ones(shape, bool), np.full(shape, 5, np.uint16)), (np.zeros(shape, bool), np.zeros(shape, np.uint16))]
    fs = hip.FrameSum(2 * 65, 2 * 5)
    try:
        for level, d, want in ((1, 12, min(blocks, 8 * 8 // 12) + blocks + 0), (1, 9, min(blocks, 8 * 6 // 9) + blocks + 0), (3, 8, 3 * blocks), (2, 12, 3 * blocks)):
            data, sizes = cm.stored_batch(frames, level, d)
            before = fs.bound()
            fs.add_counted(_geom(shape, level, d), data, sizes, 3, 0, 0, 2)
            assert fs.bound() - before == want == hip.FrameSum.grows_by_counted(_geom(shape, level, d), sizes, 3), (level, d)
    finally:
        fs.close()


def test_two_slots_into_one_handle_with_a_refused_batch_in_the_middle(hip):
    shape, d, n, s = (127, 130), 12, 3, 2
    L = hip.lib()
    batches = _batches(shape, d, 5)
    stored = [cm.stored_batch(fr, 1, d) for fr in batches]
    data2, sizes2 = stored[2]
    cut = int(sizes2[0, 0] + sizes2[0, 1]) - 1                      # batch 2: frame 0's value stream one byte short
    bad = sizes2.copy()
    bad[0, 1] -= 1
    bad[0, 2] -= 1
    stored[2] = (np.delete(data2, cut), bad)
    g = _geom(shape, 1, d)
    fs = hip.FrameSum(s * 130, s * 127)
    try:
        def submit(j):
            hip.check(fs.submit_counted_status(j & 1, g, stored[j][0], stored[j][1], n, 0, 1, s), "submit")
        submit(0)
        for j in range(5):
            if j + 1 < 5:
                submit(j + 1)
            prefix = np.zeros(n + 1, np.uint64)
            st = L.rc_expand_frames_wait(j & 1, hip.ptr(prefix))
            if j == 2:
                assert st == hip.RC_ERR_CORRUPT
                continue
            assert st == hip.RC_OK, hip.last_error()
            assert np.array_equal(prefix, cv.events_prefix(batches[j], "weighted_average", 1))
        want = sum(cv.counted_view(batches[j], "weighted_average", 1, s) for j in (0, 1, 3, 4))
        assert np.array_equal(fs.fetch(), want) and int(want.sum()) > 100
        assert fs.bound() == sum(hip.FrameSum.grows_by_counted(g, sz, n) for _, sz in stored)      # (an upper bound: the refused batch was counted)
    finally:
        fs.close()


# ---- 4. refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals(hip):
    shape, d = (127, 130), 12
    L, p = hip.lib(), hip.ptr
    frames = _batches(shape, d, 1, p=0.04)[0]
    data, sizes = cm.stored_batch(frames, 1, d)
    g = _geom(shape, 1, d)
    want = cv.counted_view(frames, "weighted_average", 0, 2)
    fs = hip.FrameSum(2 * 130, 2 * 127)
    try:
        fs.add_counted(g, data, sizes, 3, 0, 0, 2)
        bound = fs.bound()

        def unchanged():
            return fs.bound() == bound and np.array_equal(fs.fetch(), want)
        assert unchanged()
        # a handle of the wrong shape: upsample 1 and 3 into the view of upsample 2, and the transposed frame
        for nx, ny, s in ((130, 127, 1), (130, 127, 3), (127, 130, 2)):
            assert L.rc_sum_add_counted(fs.handle, nx, ny, s, d, 1, 0, 0, p(data), p(sizes), 3, 0, 0, None) == hip.RC_ERR_BAD_ARG and "shape" in hip.last_error()
            assert L.rc_sum_add_counted_submit(fs.handle, 0, nx, ny, s, d, 1, 0, 0, p(data), p(sizes), 3, 0, 0) == hip.RC_ERR_BAD_ARG
        assert unchanged()
        with pytest.raises(ValueError, match="upsample 3"):
            fs.add_counted(g, data, sizes, 3, 0, 0, 3)
        # frame 1's value stream one byte short (its sizes say so; the bytes behind it move up)
        cut = int(sizes[0].sum() - sizes[0, 2] + sizes[1, 0] + sizes[1, 1]) - 1
        short, ssz = np.delete(data, cut), sizes.copy()
        ssz[1, 1] -= 1
        ssz[1, 2] -= 1
        assert fs.add_counted_status(g, short, ssz, 3, 0, 0, 2) == hip.RC_ERR_CORRUPT
        assert unchanged()
        assert fs.add_counted_status((130, 127, 17, 1, 0, 0), data, sizes, 3, 0, 0, 2) == hip.RC_ERR_UNSUPPORTED
        assert fs.add_counted_status(g, data, sizes, 3, 3, 0, 2) == hip.RC_ERR_BAD_ARG
        assert unchanged()
        fs.add_counted(g, data, sizes, 3, 0, 0, 2)                   # and the call after the refusals is right
        assert fs.bound() == 2 * bound and np.array_equal(fs.fetch(), 2 * want)
    finally:
        fs.close()


def test_no_silent_wrap(hip):
    """One pixel.  65 535 + 2 plain frames of 65 535 take the cell and the bound to 2^32 - 1 exactly; one more count would wrap the cell:
    RC_ERR_OUT_TOO_SMALL before anything is queued, cell and bound unchanged; after a reset the same add is taken."""
    n = 65535
    blob = np.tile(np.array([1, 0xFF, 0xFF], np.uint8), n)
    sizes = np.tile(np.array([1, 2, 2], np.uint32), (n, 1))
    g = (1, 1, 16, 1, 0, 0)
    fs = hip.FrameSum(1, 1)
    try:
        fs.add(g, blob, sizes, n)
        fs.add(g, blob[:6], sizes[:2], 2)
        assert fs.bound() == 0xFFFFFFFF == int(fs.fetch()[0, 0])
        assert fs.add_counted_status(g, blob[:3], sizes[:1], 1, 0, 0, 1) == hip.RC_ERR_OUT_TOO_SMALL
        assert fs.submit_counted_status(1, g, blob[:3], sizes[:1], 1, 0, 0, 1) == hip.RC_ERR_OUT_TOO_SMALL
        assert hip.lib().rc_expand_frames_wait(1, hip.ptr(np.zeros(4, np.uint64))) == hip.RC_ERR_BAD_ARG      # (nothing was queued)
        assert fs.bound() == 0xFFFFFFFF == int(fs.fetch(reset=True)[0, 0])
        assert fs.add_counted(g, blob[:3], sizes[:1], 1, 0, 0, 1).tolist() == [0, 1]
        assert fs.bound() == 1 == int(fs.fetch()[0, 0])
    finally:
        fs.close()


# ---- 5. the reader -----------------------------------------------------------------------------------------------------------------------
def _open(path, part=False):
    from pyrecode_amd.recode_reader import ReCoDeReader
    rd = ReCoDeReader(path, is_intermediate=part)
    rd.open(print_header=False)
    return rd


def _frames_of(rd, z0, n):
    """[(binary, value)] of records z0 .. z0+n-1 from the reader's own COO expansion (a stored 0 at a set pixel stays a set pixel)"""
    ny, nx = int(rd._header['ny']), int(rd._header['nx'])
    prefix, (rows, cols, vals) = rd.get_frames_coo(z0, n)
    frames = []
    for i in range(n):
        a, b = int(prefix[i]), int(prefix[i + 1])
        binary, value = np.zeros((ny, nx), bool), np.zeros((ny, nx), np.uint16)
        binary[rows[a:b], cols[a:b]] = True
        value[rows[a:b], cols[a:b]] = vals[a:b]
        frames.append((binary, value))
    return frames


@pytest.mark.parametrize("name,part", [("g3_l1z12.rc1", False), ("g3_l1z16.rc1", False), ("g3_l1ro16.rc1", False), ("g3_l3z.rc3", False),
                                       ("g9_l1lzma.rc1_part000", True), ("g9_l1lzma.rc1_part001", True), ("g3_l1z12.rc1_part000", True),
                                       ("g3_l1z12.rc1_part001", True), ("g3_l1z12.rc1_part002", True)])
def test_reader_on_golden_files(hip, name, part):
    rd = _open(os.path.join(FILES, name), part)
    try:
        n = rd._batch_frames()
        frames = _frames_of(rd, 0, n)
        rd.sum_frames()
        path = rd.last_batch_path
        if "lzma" in name:
            assert path == "host-decode + device-expand"
        comps = cv.components(frames, "weighted_average", 0)
        assert sum(len(c) for c in comps) > 0
        for s in (1, 2):
            for batch in (1, 3):
                got = rd.sum_frames_counted(batch=batch, upsample=s)
                assert got.dtype == np.uint64 and np.array_equal(got, cv.view_of(comps, np.shape(frames[0][0]), s)) and rd.last_batch_path == path
                seen = []
                for a, k, img in rd.iter_frame_sums_counted(2, batch=batch, upsample=s):
                    assert img.dtype == np.uint32 and np.array_equal(img, cv.view_of(comps[a:a + k], np.shape(frames[0][0]), s))
                    seen.append((a, k))
                assert seen == [(a, min(2, n - a)) for a in range(0, n, 2)] and rd.last_batch_path == path
        z0 = 1 if n > 1 else 0
        got = rd.sum_frames_counted(z0, n - z0, area_threshold=1, method="max", upsample=3)
        assert np.array_equal(got, cv.counted_view(frames[z0:], "max", 1, 3))
        fs = hip.FrameSum(2 * int(rd._header['nx']), 2 * int(rd._header['ny']))
        try:
            assert rd.sum_frames_counted(0, n, upsample=2, into=fs) == n and rd.sum_frames_counted(0, 1, upsample=2, into=fs) == 1
            assert np.array_equal(fs.fetch(), cv.view_of(comps + comps[:1], np.shape(frames[0][0]), 2))
        finally:
            fs.close()
    finally:
        rd.close()


def test_reader_refuses_files_of_more_than_16_bits(hip):
    rd = _open(os.path.join(FILES, "g11_u32d20.rc1"))
    try:
        with pytest.raises(NotImplementedError, match="16 bits"):
            rd.sum_frames_counted(0, 1)
        with pytest.raises(NotImplementedError, match="16 bits"):
            next(rd.iter_frame_sums_counted(2))
    finally:
        rd.close()


# ---- 6. the viewer -----------------------------------------------------------------------------------------------------------------------
def test_viewer_with_counting(hip, tmp_path):
    """over the parts of g3_l1z12, fractionation 3: every view is the model's counted view of the window plan_view gives; without
    `counting` the views are the plain sums"""
    from pyrecode_amd.utils.viewer import ReCoDeViewer, plan_view
    for node in range(3):
        shutil.copy(os.path.join(FILES, "g3_l1z12.rc1_part%03d" % node), str(tmp_path))
    parts = [_open(os.path.join(FILES, "g3_l1z12.rc1_part%03d" % node), True) for node in range(3)]
    try:
        frames = [_frames_of(rd, 0, rd._batch_frames()) for rd in parts]
        ids = [rd.part_frame_ids for rd in parts]
    finally:
        for rd in parts:
            rd.close()
    ny, nx = np.shape(frames[0][0][0])
    for counting in (dict(upsample=2, area_threshold=1), None):
        v = ReCoDeViewer(str(tmp_path), "g3_l1z12.rc1", 3, 3, counting=counting)
        try:
            assert v.get_shape() == ((2 * ny, 2 * nx) if counting else (ny, nx))
            start, views = 0, 0
            while True:
                plan = plan_view(ids, start, 3)
                view = v.get_next_view()
                if plan is None:
                    assert view is None
                    break
                ranges, n_frames, nxt = plan
                window = [f for fr, (lo, hi) in zip(frames, ranges) for f in fr[lo:hi]]
                if counting:
                    want = cv.counted_view(window, "weighted_average", 1, 2) if window else np.zeros((2 * ny, 2 * nx), np.uint64)
                else:
                    want = sum((np.where(b, val, 0).astype(np.uint64) for b, val in window), np.zeros((ny, nx), np.uint64))
                assert view["start"] == start and view["n_Frames"] == n_frames and view["view"].dtype == np.float64
                assert np.array_equal(view["view"], want.astype(np.float64))
                start, views = nxt, views + 1
            assert views >= 2
        finally:
            v.close()
