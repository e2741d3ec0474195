"""-m gpu: electron counting (rc_count_frames, pyrecode_amd/csrc/rc_count.hip).  Stored streams built with numpy through the C ABI, the
level-2 topology catalogue, row ends and frame boundaries, the area threshold, the refusals, the submit / wait form with a rejected batch
in the middle, ReCoDeReader.get_frames_counted / iter_frames_counted on golden files and on files this library writes, and
l1_to_l4_converter.  The expectation is the exact model (tests/centroid_model.py); every comparison is np.array_equal on (prefix, rows, cols,
area, weight), the output is pre-filled with a sentinel and everything behind the last event must still be the sentinel."""
import os

import numpy as np
import pytest

import centroid_model as cm
import l2_topologies as lt
from conftest import GOLDEN, load_npz

pytestmark = pytest.mark.gpu
FILES = os.path.join(GOLDEN, "files")
SENTINEL = 0xA5
PATHS = {"device", "device-inflate", "host-decode + device-expand", "per-frame"}


@pytest.fixture(scope="module")
def hip():
    from pyrecode_amd import _lib
    if _lib.device_count() == 0:
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    return _lib


def _views(buf, cap, total):
    """(rows, cols, area, weight) of rc_count_frames' output, and whether everything behind entry `total` of each array is the sentinel"""
    w, r, c, a = buf[:8 * cap], buf[8 * cap:12 * cap], buf[12 * cap:16 * cap], buf[16 * cap:20 * cap]
    clean = all((part[total * size:] == SENTINEL).all() for part, size in ((w, 8), (r, 4), (c, 4), (a, 4)))
    return (r.view(np.int32)[:total], c.view(np.int32)[:total], a.view(np.uint32)[:total], w.view(np.uint64)[:total]), clean


def _call(hip, shape, level, d, data, sizes, n, method, thr, cap, counting=False):
    ny, nx = shape
    buf = np.full(20 * max(cap, 1), SENTINEL, np.uint8)
    prefix = np.zeros(n + 1, np.uint64)
    st = hip.lib().rc_count_frames(nx, ny, d, level, 0, 0, hip.ptr(data), hip.ptr(sizes), n, method, thr, hip.ptr(prefix),
                                   None if counting else hip.ptr(buf), 0 if counting else cap)
    return st, prefix, buf


def _check(hip, shape, level, d, frames, thr=0, methods=(0, 1, 2), slack=3):
    """frames = [(binary, value)] through the synchronous call for each method, against the model"""
    data, sizes = cm.stored_batch(frames, level, d)
    n = len(frames)
    model_frames = frames if level == 1 else [(b, np.ones(np.shape(b), np.uint16)) for b, _ in frames]
    for method in methods:
        want = cm.count_batch(model_frames, cm.METHODS[method], thr)
        total = int(want[0][n])
        cap = total + slack
        st, prefix, buf = _call(hip, shape, level, d, data, sizes, n, method, thr, cap)
        assert st == hip.RC_OK, (st, hip.last_error())
        got, clean = _views(buf, cap, int(prefix[n]))
        assert np.array_equal(prefix, want[0]), (method, prefix, want[0])
        for k, name in enumerate(("rows", "cols", "area", "weight")):
            assert np.array_equal(got[k], want[1 + k]), "%s differ (method %d): first at event %s" % (
                name, method, np.flatnonzero(got[k] != want[1 + k])[:4])
        assert clean, "bytes behind the last event were written"
    return want


# ---- 1. stored streams through the C ABI -------------------------------------------------------------------------------------------------
def _kind(k, ny, nx, d, seed):
    """the frame kinds of a batch in turn: 1 % Bernoulli | empty | every pixel at 2^d - 1 | only the last pixel | 4 % Bernoulli, a tenth of
    the set values 0"""
    if k % 5 == 0:
        return cm.bernoulli_frame(ny, nx, d, 0.01, seed)
    if k % 5 == 1:
        return np.zeros((ny, nx), bool), np.zeros((ny, nx), np.uint16)
    if k % 5 == 2:
        return np.ones((ny, nx), bool), np.full((ny, nx), (1 << d) - 1, np.uint16)
    if k % 5 == 3:
        b = np.zeros((ny, nx), bool)
        b[-1, -1] = True
        return b, np.full((ny, nx), 1 + (seed % ((1 << d) - 1)), np.uint16)
    return cm.bernoulli_frame(ny, nx, d, 0.04, seed, zero_fraction=0.1)


@pytest.mark.parametrize("level,d", [(1, 9), (1, 12), (1, 16), (3, 0), (2, 12)])
@pytest.mark.parametrize("shape", [(1, 1), (3, 21), (127, 130), (192, 256)])
def test_stored_streams(hip, shape, level, d):
    """less than a word, two blocks with nx % 64 = 2 and N % 8 = 6, three blocks; batches of 1, 3 and 11 frames of every kind; the full
    frame is one component with the sums at their largest and, where ny and nx are even, ties in both axes"""
    ny, nx = shape
    dv = d if level == 1 else 8
    frames = [_kind(k, ny, nx, dv, 100 + k) for k in range(11)]
    for n in (1, 3, 11):
        _check(hip, shape, level, d if d else 8, frames[:n])
    _check(hip, shape, level, d if d else 8, [frames[2]])       # the full frame alone
    _check(hip, shape, level, d if d else 8, [frames[4]], methods=(0,))


# ---- 2. topologies -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [lt.SMALL, (127, 130), (530, 517)])
@pytest.mark.parametrize("name", list(lt.CATALOGUE))
def test_topologies(hip, name, shape):
    """every entry with its own value image at d = 16 (zeros at set bits included); (530, 517): 17 blocks, nx % 64 = 5, components that
    cross words, rows and blocks and merge late.  One frame per call, and three seeds' frames in one batch."""
    ts = [lt.CATALOGUE[name](shape[0], shape[1], seed) for seed in (0, 1, 2)]
    frames = [(t.binary, t.value) for t in ts]
    _check(hip, shape, 1, 16, frames[:1])
    _check(hip, shape, 1, 16, frames)


# ---- 3. edges ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(9, 11), (5, 64), (5, 65)])
def test_no_link_wraps_from_the_last_column_to_the_first(hip, shape):
    ny, nx = shape
    b = np.zeros(shape, bool)
    b[0::2, nx - 1] = True          # (r, nx - 1) and (r + 1, 0) are neighbours in the bit stream, not in the frame
    b[1::2, 0] = True
    v = np.arange(1, ny * nx + 1, dtype=np.uint16).reshape(shape)
    want = _check(hip, shape, 1, 16, [(b, v)])
    assert int(want[0][1]) == int(b.sum()) == ny and (want[3] == 1).all()


def test_no_link_crosses_a_frame_boundary(hip):
    shape = (4, 70)
    last, first = np.zeros(shape, bool), np.zeros(shape, bool)
    last[-1, :], first[0, :] = True, True
    v = np.full(shape, 3, np.uint16)
    want = _check(hip, shape, 1, 12, [(last, v), (first, v)])
    assert want[0].tolist() == [0, 1, 2] and want[3].tolist() == [70, 70]


@pytest.mark.parametrize("nx", [64, 128])
def test_rows_of_whole_words(hip, nx):
    for name in ("diagonals", "columns", "checkerboard", "percolating_041"):
        t = lt.CATALOGUE[name](6, nx, 1)
        _check(hip, (6, nx), 1, 16, [(t.binary, t.value)])


# ---- 4. area_threshold -------------------------------------------------------------------------------------------------------------------
def test_area_threshold(hip):
    shape = (40, 70)
    b, v = np.zeros(shape, bool), np.random.default_rng(4).integers(1, 4096, shape).astype(np.uint16)
    for k in range(25):              # horizontal runs of 1 .. 5 pixels, apart
        r, c, area = 2 * (k // 5) + 1, 13 * (k % 5) + 1, 1 + k % 5
        b[r, c:c + area] = True
    for thr, kept in ((0, 25), (1, 20), (3, 10), (5, 0), (1000, 0)):
        want = _check(hip, shape, 1, 12, [(b, v), (b[::-1].copy(), v)], thr=thr)
        assert want[0].tolist() == [0, kept, 2 * kept]


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals(hip):
    shape = (127, 130)
    frames = [cm.bernoulli_frame(127, 130, 12, 0.04, s) for s in (1, 2, 3)]
    data, sizes = cm.stored_batch(frames, 1, 12)
    want = cm.count_batch(frames)
    total = int(want[0][3])
    st, prefix, buf = _call(hip, shape, 1, 12, data, sizes, 3, 0, 0, total - 1)
    assert st == hip.RC_ERR_OUT_TOO_SMALL and np.array_equal(prefix, want[0]) and (buf == SENTINEL).all()
    st, prefix, _ = _call(hip, shape, 1, 12, data, sizes, 3, 0, 0, 0, counting=True)
    assert st == hip.RC_OK and np.array_equal(prefix, want[0])
    st, prefix, buf = _call(hip, shape, 1, 12, data, sizes, 3, 0, 0, total)          # exactly enough
    assert st == hip.RC_OK and np.array_equal(_views(buf, total, total)[0][3], want[4])
    # frame 1's value stream one byte short (its sizes say so; the bytes behind it move up)
    cut = int(sizes[0].sum() - sizes[0, 2] + sizes[1, 0] + sizes[1, 1]) - 1
    short, ssz = np.delete(data, cut), sizes.copy()
    ssz[1, 1] -= 1
    ssz[1, 2] -= 1
    st, _, buf = _call(hip, shape, 1, 12, short, ssz, 3, 0, 0, total + 8)
    assert st == hip.RC_ERR_CORRUPT and (buf == SENTINEL).all()
    st, _, buf = _call(hip, shape, 1, 17, data, sizes, 3, 0, 0, total)
    assert st == hip.RC_ERR_UNSUPPORTED and (buf == SENTINEL).all()
    st, _, buf = _call(hip, shape, 1, 12, data, sizes, 3, 3, 0, total)
    assert st == hip.RC_ERR_BAD_ARG and (buf == SENTINEL).all()
    st, prefix, buf = _call(hip, shape, 1, 12, data, sizes, 3, 0, 0, total)          # and the call after the refusals is right
    assert st == hip.RC_OK and np.array_equal(prefix, want[0])


# ---- 6. submit and wait ------------------------------------------------------------------------------------------------------------------
def test_submit_wait_with_a_refused_batch_in_the_middle(hip):
    shape, d, n = (127, 130), 12, 3
    L = hip.lib()
    batches = [[cm.bernoulli_frame(127, 130, d, 0.03, 10 * j + z) for z in range(n)] for j in range(5)]
    stored = [cm.stored_batch(fr, 1, d) for fr in batches]
    data2, sizes2 = stored[2]
    cut = int(sizes2[0, 0] + sizes2[0, 1]) - 1                      # batch 2: frame 0's value stream one byte short
    bad = sizes2.copy()
    bad[0, 1] -= 1
    bad[0, 2] -= 1
    stored[2] = (np.delete(data2, cut), bad)
    wants = [cm.count_batch(fr, "weighted_average", 1) for fr in batches]
    cap = max(int(w[0][n]) for w in wants) + 5
    outs = [hip.PinnedBuffer(20 * cap), hip.PinnedBuffer(20 * cap)]

    def submit(j):
        outs[j & 1].array[:] = SENTINEL
        data, sizes = stored[j]
        hip.check(L.rc_count_frames_submit(j & 1, 130, 127, d, 1, 0, 0, hip.ptr(data), hip.ptr(sizes), n, 0, 1, outs[j & 1]._p, cap), "submit")
    try:
        submit(0)
        for j in range(5):
            if j + 1 < 5:
                submit(j + 1)
            prefix = np.zeros(n + 1, np.uint64)
            st = L.rc_expand_frames_wait(j & 1, hip.ptr(prefix))
            buf = outs[j & 1].array
            if j == 2:
                assert st == hip.RC_ERR_CORRUPT and (buf == SENTINEL).all()
                continue
            assert st == hip.RC_OK, hip.last_error()
            got, clean = _views(buf, cap, int(prefix[n]))
            assert np.array_equal(prefix, wants[j][0]) and clean
            assert all(np.array_equal(got[k], wants[j][1 + k]) for k in range(4))
    finally:
        for o in outs:
            o.close()


# ---- 7. the reader -----------------------------------------------------------------------------------------------------------------------
def _open(path, part=False):
    from pyrecode_amd.recode_reader import ReCoDeReader
    rd = ReCoDeReader(path, is_intermediate=part)
    rd.open(print_header=False)
    return rd


def _model_of_reader(rd, n, method="weighted_average", thr=0):
    """the model on what the reader's own frames hold (get_frames: the dictionary get_frame builds, for part files too)"""
    frames = []
    for entry in rd.get_frames(0, n).values():
        dense = entry['data'].toarray()
        frames.append((dense != 0, dense))
    return cm.count_batch(frames, method, thr)


def _same(got, want):
    return len(got) == 5 and all(np.array_equal(g, w) and g.dtype == w.dtype for g, w in zip(got, want))


def _reader_checks(rd, n):
    want = _model_of_reader(rd, n)
    assert int(want[0][n]) > 0
    got = rd.get_frames_counted(0, n)
    assert _same(got, want) and rd.last_batch_path in PATHS
    for batch in (1, 3):
        items = list(rd.iter_frames_counted(batch=batch))
        assert [it[0] for it in items] == list(range(0, n, batch)) and rd.last_batch_path in PATHS
        for k in range(1, 5):
            assert np.array_equal(np.concatenate([it[1 + k] for it in items]), want[k])
        assert np.array_equal(np.concatenate([[0]] + [np.diff(it[1].astype(np.int64)) for it in items]).cumsum(), want[0].astype(np.int64))
    for method, thr in (("max", 0), ("unweighted_average", 1)):
        assert _same(rd.get_frames_counted(0, n, area_threshold=thr, method=method), _model_of_reader(rd, n, method, thr))
    return rd.last_batch_path


@pytest.mark.parametrize("name,part", [("g3_l1z12.rc1", False), ("g3_l1z16.rc1", False), ("g3_l1ro16.rc1", False), ("g3_l3z.rc3", False),
                                       ("g9_l1lzma.rc1_part000", True), ("g9_l1lzma.rc1_part001", True), ("g3_l1z12.rc1_part000", True),
                                       ("g3_l1z12.rc1_part001", True), ("g3_l1z12.rc1_part002", True)])
def test_reader_on_golden_files(hip, name, part):
    rd = _open(os.path.join(FILES, name), part)
    try:
        path = _reader_checks(rd, rd._batch_frames())
        if "lzma" in name:
            assert path == "host-decode + device-expand"
    finally:
        rd.close()


def test_reader_refuses_files_of_more_than_16_bits(hip):
    rd = _open(os.path.join(FILES, "g11_u32d20.rc1"))
    try:
        with pytest.raises(NotImplementedError, match="16 bits"):
            rd.get_frames_counted(0, 1)
        with pytest.raises(NotImplementedError, match="16 bits"):
            next(rd.iter_frames_counted())
    finally:
        rd.close()


def _clustered_stack(nz=8, ny=127, nx=130, seed=33):
    """detector-like frames: seeds at 1.2 % light a 2 x 3 window's cells with probability 5 / 8 (the shape of bench.py --clustered)"""
    rng = np.random.default_rng(seed)
    dark = rng.integers(80, 121, (ny, nx)).astype(np.uint16)
    ev = np.zeros((nz, ny, nx), bool)
    seeds = rng.random((nz, ny, nx)) < 0.012
    for dy in range(2):
        for dx in range(3):
            lit = seeds & ((rng.random((nz, ny, nx)) < 0.625) | (dy + dx == 0))
            ev[:, dy:, dx:] |= lit[:, :ny - dy, :nx - dx]
    frames = np.where(ev, dark + rng.integers(1, 2048, (nz, ny, nx)), dark // 2).astype(np.uint16)
    return dark, frames


def _write(tmp, dark, frames, level, scheme):
    from pyrecode_amd.params import InputParams
    from pyrecode_amd.recode_reader import merge_parts
    from pyrecode_amd.recode_writer import ReCoDeWriter
    g = load_npz("g3_l1z12.npz")
    nz, ny, nx = frames.shape
    cfg = dict(zip(g["cfg_keys"].tolist(), (int(v) for v in g["cfg_vals"])))
    cfg.update(num_rows=ny, num_cols=nx, num_frames=nz, num_threads=2, compression_scheme=scheme, reduction_level=level,
               calibration_threshold_epsilon=0)
    (tmp / "params.txt").write_text("".join("%s = %d\n" % kv for kv in cfg.items()))
    for node in range(2):
        ip = InputParams()
        ip.load(str(tmp / "params.txt"))
        w = ReCoDeWriter("s", dark_data=dark, output_directory=str(tmp), input_params=ip, mode="batch", validation_frame_gap=-1, node_id=node,
                         batch_size=4)
        w.start()
        w.run(frames)
        w.close()
    merge_parts(str(tmp), "s.rc%d" % level, 2)
    return str(tmp / ("s.rc%d" % level))


@pytest.mark.parametrize("scheme", [0, 1, 2, 8])
def test_reader_on_this_librarys_files(hip, tmp_path, scheme):
    dark, frames = _clustered_stack()
    rd = _open(_write(tmp_path, dark, frames, 1, scheme))
    try:
        _reader_checks(rd, 8)
        # against the frames themselves, not only against the reader's own expansion
        want = cm.count_batch([(f > dark, (f.astype(np.int64) - dark).clip(0).astype(np.uint16)) for f in frames])
        assert _same(rd.get_frames_counted(0, 8), want) and int((want[3] > 1).sum()) > 50
    finally:
        rd.close()


# ---- 8. l1_to_l4_converter ---------------------------------------------------------------------------------------------------------------
def test_l1_to_l4_converter(hip, capsys):
    from pyrecode_amd.utils import l1_to_l4_converter
    rd = _open(os.path.join(FILES, "g3_l1z12.rc1"))
    try:
        n = rd._batch_frames()
        l1 = rd.get_frames(0, n)
        shape = (int(rd._header['ny']), int(rd._header['nx']))
    finally:
        rd.close()
    for method, thr in (("weighted_average", 0), ("max", 1)):
        out = l1_to_l4_converter(l1, shape, area_threshold=thr, method=method)
        assert list(out) == list(l1) and "Total processing time" in capsys.readouterr().out
        for key in l1:
            dense = l1[key]['data'].toarray()
            rows, cols, _, _ = cm.count_frame(dense != 0, dense, method, thr)
            m = out[key]['data']
            assert m.shape == shape and m.dtype == bool and m.format == 'coo' and m.data.all()
            assert sorted(zip(m.row.tolist(), m.col.tolist())) == sorted(zip(rows.tolist(), cols.tolist()))
            assert out[key] is not l1[key] and out[key]['metadata'] is not l1[key]['metadata']
            assert {k: v for k, v in out[key].items() if k != 'data'}.keys() == {k: v for k, v in l1[key].items() if k != 'data'}.keys()
            assert all(out[key]['metadata'][f] == l1[key]['metadata'][f] for f in l1[key]['metadata'])
    some = l1_to_l4_converter(l1, shape, n_frames=2, verbosity=1)
    assert list(some) == list(l1)[:2] and "Dose Rate =" in capsys.readouterr().out
    keep = {key: l1[key]['metadata'] for key in l1}
    same = l1_to_l4_converter(l1, shape, in_place=True)
    assert all(same[key] is l1[key] and same[key]['metadata'] is keep[key] and same[key]['data'].dtype == bool for key in l1)
