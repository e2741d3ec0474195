"""-m gpu: reduction level 2 (rc_l2.hip) on the topology catalogue (tests/l2_topologies.py) - components that span work items, merge late,
run longer than a tile, fill a tile with roots; and the validation frames' ROI count (k_roi_components) on long thin components.
Whole records byte for byte against scipy.ndimage.label (test_gpu_parity._l2_expected) and, where the catalogue has one, against the
closed form, so that a failure does not hang on scipy alone.  No tolerance, no sampling: every frame of every batch is compared."""
import functools
import struct

import numpy as np
import pytest

import l2_topologies as lt
from test_gpu_parity import _l2_expected, _zstd_system_decode

pytestmark = pytest.mark.gpu

MAX, SUM = 1, 2                      # rc_ctx_set_l2_statistics codes
BIG = lt.MULTI_ITEM[0]               # 530 x 517: two items, nx % 64 = 5


@pytest.fixture(scope="module")
def hip():
    from pyrecode_amd import _lib
    if _lib.device_count() == 0:
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    return _lib


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    oracle.lib()
    return oracle


@functools.lru_cache(maxsize=None)
def _dark(ny, nx, dtype=np.uint16):
    d = lt.dark_image(ny, nx, 1, dtype)
    d.setflags(write=False)
    return d


def _frames(topos, dark):
    return np.stack([lt.frame_of(t, dark) for t in topos])


def _pieces(orc, topo, frame, thr, stat, d):
    """(bitmap bytes, packed statistics) of one frame: scipy's - after the closed form's, where there is one, has agreed with it"""
    wide = frame.astype(np.uint16)
    binary, vals = _l2_expected(wide, thr.astype(np.uint16), stat, d)
    assert np.array_equal(binary, topo.binary)
    if topo.closed is not None:
        c = topo.stats(frame)
        own = ((c.maximum if stat != SUM else c.total) & ((1 << d) - 1)).astype(np.uint16)
        assert c.count == own.size == vals.size and np.array_equal(own, vals), "%s: the closed form and scipy disagree" % topo.name
        vals = own
    return orc.pack_binary_frame(topo.binary).tobytes(), orc.bit_pack(vals, d).tobytes()


def _explain(orc, r, bitmap, packed, d):
    """what differs, in components rather than bytes"""
    if len(r) < 8 + len(bitmap):
        return "the record is %d bytes, header and binary map alone are %d" % (len(r), 8 + len(bitmap))
    if r[8:8 + len(bitmap)] != bitmap:
        return "the binary map differs"
    n_got, n_want = (len(r) - 8 - len(bitmap)) * 8 // d, len(packed) * 8 // d
    got, want = orc.bit_unpack(np.frombuffer(r[8 + len(bitmap):], np.uint8), n_got, d), orc.bit_unpack(np.frombuffer(packed, np.uint8), n_want, d)
    m = min(n_got, n_want)
    bad = np.flatnonzero(got[:m] != want[:m])
    return "%d statistics of %d bits, expected %d; %d of the common ones differ, the first at component %s (got %s, expected %s)" % (
        n_got, d, n_want, bad.size, bad[0] if bad.size else "-", got[bad[0]] if bad.size else "-", want[bad[0]] if bad.size else "-")


def _check_reduce_only(orc, out, rec, topos, frames, thr, stat, d, what, first_id=0, cache=None):
    for z, (t, f) in enumerate(zip(topos, frames)):
        key = (t.name, t.binary.shape, t.seed, stat, d)
        if cache is None or key not in cache:
            pieces = _pieces(orc, t, f, thr, stat, d)
            if cache is not None:
                cache[key] = pieces
        bitmap, packed = pieces if cache is None else cache[key]
        r = bytes(out[int(rec[z]):int(rec[z + 1])])
        same = r == struct.pack("<II", first_id + z, len(packed)) + bitmap + packed
        assert same, "%s, frame %d (%s, planted at %s): %s" % (what, z, t.name, t.plant, _explain(orc, r, bitmap, packed, d))


@functools.lru_cache(maxsize=None)
def _noise(ny, nx):
    """the batch between two structured ones: Bernoulli noise below, near and above the percolation threshold"""
    return tuple(lt.bernoulli(p)(ny, nx, 40 + i) for i, p in enumerate((0.02, 0.30, 0.55)))


_NOISE_PIECES = {}

EVERYWHERE = [n for n in lt.CATALOGUE if n not in ("empty", "bernoulli_050")]
CASES = [(name, ny, nx) for name in EVERYWHERE for ny, nx in lt.MULTI_ITEM + [lt.THREE_ITEM]]
CASES = [(name, ny, nx, (16, 12, 9)[i % 3]) for i, (name, ny, nx) in enumerate(CASES)]   # (four geometries a name: every geometry sees every d)


@pytest.mark.parametrize("name,ny,nx,d", CASES)
def test_every_topology_across_work_items(hip, orc, name, ny, nx, d):
    """Both statistics over one ctx, three batches each: the structured one (three frames: the planted maximum at the component's first
    pixel, its last and a middle one), noise, the structured one again.  The second and the third find out whether a batch that wrote
    nearly every node put them all back to rest."""
    assert lt.n_items(ny, nx) >= 2
    dark = _dark(ny, nx)
    thr = orc.threshold(dark, 0)
    topos = [lt.CATALOGUE[name](ny, nx, seed) for seed in (0, 1, 2)]
    frames, noise = _frames(topos, dark), _noise(ny, nx)
    noise_frames = _frames(noise, dark)
    ctx = hip.ReduceContext(nx, ny, d, 2, 0, 0, 1, 0, max_batch=3)
    ctx.set_dark(dark, 0)
    own = {}
    for stat in (MAX, SUM):
        ctx.set_l2_statistics(stat)
        for k, (tt, ff, cache) in enumerate(((topos, frames, own), (noise, noise_frames, _NOISE_PIECES), (topos, frames, own))):
            out, rec, md = ctx.reduce_compress_batch(ff, first_frame_id=0)
            _check_reduce_only(orc, out, rec, tt, ff, thr, stat, d, "%s %dx%d stat %d d %d batch %d" % (name, ny, nx, stat, d, k), cache=cache)
    ctx.close()


@pytest.mark.parametrize("ny,nx,d", [(128, 128, 16), (256, 128, 12), (256, 128, 9)])
def test_lattice_tiles_of_exactly_one_emit_round(hip, orc, ny, nx, d):
    """Every tile holds exactly L2_ROUND = 1024 set pixels and every one of them is a root: k_l2_emit's whole-tile rounds with a full list,
    one tile and eight; both statistics, then again over the same nodes."""
    assert set(lt.tile_counts(lt.lattice(ny, nx).binary)) == {lt.L2_ROUND}
    dark = _dark(ny, nx)
    thr = orc.threshold(dark, 0)
    topos = [lt.lattice(ny, nx, seed) for seed in (0, 1, 2)]
    frames = _frames(topos, dark)
    ctx = hip.ReduceContext(nx, ny, d, 2, 0, 0, 1, 0, max_batch=3)
    ctx.set_dark(dark, 0)
    for k, stat in enumerate((MAX, SUM, MAX)):
        ctx.set_l2_statistics(stat)
        out, rec, md = ctx.reduce_compress_batch(frames, first_frame_id=0)
        _check_reduce_only(orc, out, rec, topos, frames, thr, stat, d, "lattice %dx%d stat %d d %d batch %d" % (ny, nx, stat, d, k))
    ctx.close()


@pytest.mark.parametrize("stat,d", [(MAX, 12), (SUM, 16)])
def test_four_topologies_share_one_batch(hip, orc, stat, d):
    """The frames of a batch share the kernels' grid: an item index must map to the right frame - an empty frame and a full one among
    lattices and diagonals, then the same ctx with the frames in another order."""
    ny, nx = BIG
    dark = _dark(ny, nx)
    thr = orc.threshold(dark, 0)
    ctx = hip.ReduceContext(nx, ny, d, 2, 0, 0, 1, 0, max_batch=4)
    ctx.set_dark(dark, 0)
    ctx.set_l2_statistics(stat)
    for k, names in enumerate((("empty", "full", "checkerboard", "diagonals"), ("lattice", "serpentine", "empty", "rings"),
                               ("full", "empty", "diagonals_mirror", "comb_down"))):
        topos = [lt.CATALOGUE[n](ny, nx, k + z) for z, n in enumerate(names)]
        frames = _frames(topos, dark)
        out, rec, md = ctx.reduce_compress_batch(frames, first_frame_id=7)
        _check_reduce_only(orc, out, rec, topos, frames, thr, stat, d, "mixed batch %d stat %d" % (k, stat), first_id=7)
    ctx.close()


PHASE_NX = list(range(1, 67)) + [127, 128, 129, 191, 4095, 4096, 4097]


@pytest.mark.parametrize("nx", PHASE_NX)
def test_every_word_phase(hip, orc, nx):
    """Every nx % 64, several rows per word, rows longer than a tile: the first / last column masks, the funnel shift of the row above
    and its continuation word - on frames of two or three tiles; both statistics over one ctx."""
    ny = -(-6000 // nx)
    assert lt.TILE_PX < ny * nx <= 3 * lt.TILE_PX + 2
    d = (16, 12, 9)[nx % 3]
    dark = _dark(ny, nx)
    thr = orc.threshold(dark, 0)
    topos = [make(ny, nx, nx + z) for z, make in enumerate((lt.checkerboard, lt.rows, lt.bernoulli_050, lt.rows_odd))]
    frames = _frames(topos, dark)
    ctx = hip.ReduceContext(nx, ny, d, 2, 0, 0, 1, 0, max_batch=4)
    ctx.set_dark(dark, 0)
    for stat in (MAX, SUM):
        ctx.set_l2_statistics(stat)
        out, rec, md = ctx.reduce_compress_batch(frames, first_frame_id=0)
        _check_reduce_only(orc, out, rec, topos, frames, thr, stat, d, "nx %d ny %d stat %d d %d" % (nx, ny, stat, d))
    ctx.close()


@pytest.mark.parametrize("scheme,stat,d", [(2, SUM, 12), (8, MAX, 16)])
def test_serpentine_and_checkerboard_through_a_codec(hip, orc, scheme, stat, d):
    ny, nx = BIG
    dark = _dark(ny, nx)
    thr = orc.threshold(dark, 0)
    topos = [lt.serpentine(ny, nx, 1), lt.checkerboard(ny, nx, 2)]
    frames = _frames(topos, dark)
    ctx = hip.ReduceContext(nx, ny, d, 2, 1, scheme, 1, 0, max_batch=2)
    ctx.set_dark(dark, 0)
    ctx.set_l2_statistics(stat)
    out, rec, md = ctx.reduce_compress_batch(frames, first_frame_id=0)
    dec = {2: lambda b, n: orc.lz4f_decode(b, n + 8), 1: lambda b, n: _zstd_system_decode(b), 8: lambda b, n: orc.blosc1_decode(b)}[scheme]
    for z, t in enumerate(topos):
        bitmap, packed = _pieces(orc, t, frames[z], thr, stat, d)
        r = out[int(rec[z]):int(rec[z + 1])].tobytes()
        fid, cb, cp, npk = struct.unpack_from("<IIII", r, 0)
        assert fid == z and npk == len(packed) and len(r) == 16 + cb + cp
        assert dec(r[16:16 + cb], len(bitmap)) == bitmap, t.name
        assert dec(r[16 + cb:], len(packed)) == packed, t.name
    ctx.close()


@pytest.mark.parametrize("stat", [MAX, SUM])
def test_checkerboard_and_lattice_from_uint8_sources(hip, orc, stat):
    ny, nx, d = BIG + (8,)
    dark = _dark(ny, nx, np.uint8)
    thr = orc.threshold(dark, 0)
    topos = [lt.checkerboard(ny, nx, 0), lt.lattice(ny, nx, 1), lt.checkerboard(ny, nx, 2)]
    frames = _frames(topos, dark)
    assert frames.dtype == np.uint8
    ctx = hip.ReduceContext(nx, ny, d, 2, 0, 0, 1, 0, max_batch=3, src_dtype=np.uint8)
    ctx.set_dark(dark, 0)
    ctx.set_l2_statistics(stat)
    for k in range(2):
        out, rec, md = ctx.reduce_compress_batch(frames, first_frame_id=0)
        _check_reduce_only(orc, out, rec, topos, frames, thr, stat, d, "uint8 stat %d batch %d" % (stat, k))
    ctx.close()


@pytest.mark.parametrize("stat,d", [(MAX, 9), (SUM, 12)])
def test_pipelined_batches_alternate_node_workspaces(hip, orc, stat, d):
    """rc_reduce_compress_batch_async in pipelined mode: consecutive batches label in two node workspaces in turn.  Six batches, so that
    each workspace takes a comb (every node written), then percolating noise, then the other again - and must have been left at rest
    every time."""
    import torch
    ny, nx = BIG
    dark = _dark(ny, nx)
    thr = orc.threshold(dark, 0)
    comb = [lt.comb_down(ny, nx, s) for s in (0, 1, 2)]
    perc = [lt.percolating_041(ny, nx, 0), lt.percolating_045(ny, nx, 1), lt.percolating_045(ny, nx, 2), lt.percolating_041(ny, nx, 3)]
    A, B, B2, A2 = [comb[0], comb[1]], [perc[0], perc[1]], [perc[2], perc[3]], [comb[2], perc[0]]
    batches = [A, B, B2, A2, A, B]                      # workspace 0: A, B2, A; workspace 1: B, A2, B
    ctx = hip.ReduceContext(nx, ny, d, 2, 0, 0, 1, 0, max_batch=2)
    ctx.set_dark(dark, 0)
    ctx.set_l2_statistics(stat)
    ctx.set_pipelined(True)
    dev = torch.device("cuda", 0)
    host = [_frames(b, dark) for b in batches]
    fr_d = [torch.from_numpy(h.view(np.int16)).to(dev) for h in host]
    cap = int(ctx.out_capacity(2))
    outs = [torch.zeros(cap, dtype=torch.uint8, device=dev) for _ in batches]
    recs = [torch.zeros(3, dtype=torch.int64, device=dev) for _ in batches]
    mds = [torch.zeros((2, 3), dtype=torch.int32, device=dev) for _ in batches]
    torch.cuda.synchronize()
    for b in range(len(batches)):
        ctx.enqueue(fr_d[b].data_ptr(), 2, 2 * b, outs[b].data_ptr(), cap, recs[b].data_ptr(), mds[b].data_ptr())
    ctx.sync()
    cache = {}
    for b, topos in enumerate(batches):
        _check_reduce_only(orc, outs[b].cpu().numpy(), recs[b].cpu().numpy(), topos, host[b], thr, stat, d,
                           "pipelined batch %d stat %d" % (b, stat), first_id=2 * b, cache=cache)
    ctx.set_pipelined(False)
    ctx.close()


ROI_TOPOLOGIES = ("spiral", "serpentine", "checkerboard", "lattice", "rings", "comb_down")


@pytest.mark.parametrize("h,w,y0,x0", [(128, 128, 11, 21), (37, 128, 57, 21), (128, 1, 11, 85)])
def test_roi_component_count_on_long_thin_components(hip, orc, h, w, y0, x0):
    """k_roi_components (rc_ctx_set_validation / rc_pipe_validation) sweeps until nothing changes: a spiral and a serpentine are the longest
    paths an ROI admits.  Every pixel outside the ROI is set: the kernel loads only the ROI's own pixels, so these tell when it loads from the
    wrong place (an offset or a row stride off) - the count of the all-set surroundings is 1.  Every second frame is a validation frame;
    the others must read 0xFFFFFFFF."""
    import scipy.ndimage as nd
    ny, nx, gap = 150, 170, 2
    dark = _dark(ny, nx)
    n = 2 * len(ROI_TOPOLOGIES)
    frames = np.empty((n, ny, nx), np.uint16)
    want = []
    for k, name in enumerate(ROI_TOPOLOGIES):
        t = lt.CATALOGUE[name](h, w, k)
        inside = np.ones((ny, nx), bool)
        inside[y0:y0 + h, x0:x0 + w] = t.binary
        frames[2 * k] = frames[2 * k + 1] = np.where(inside, dark + 1 + (t.value[0, 0] & 1023), dark // 2)
        count = nd.label((frames[2 * k] > dark)[y0:y0 + h, x0:x0 + w], structure=np.ones((3, 3), int))[1]
        assert count == t.closed.count, name
        want.append(count)
    ctx = hip.ReduceContext(nx, ny, 12, 1, 1, 2, 1, 0, max_batch=n)
    ctx.set_dark(dark, 0)
    ctx.set_validation(gap, x0, y0, w, h)
    dst = np.empty(ctx.out_capacity(n), np.uint8)
    for slot, first_id in ((0, 1), (1, 2)):          # ids 1 .. 12: the odd indices are validation frames; ids 2 .. 13: the even ones
        ctx.pipe_submit(slot, frames, n, first_id)
        rec, md, total = ctx.pipe_result(slot, n)
        counts = ctx.pipe_validation(slot, n)
        ctx.pipe_fetch(slot, dst, total)
        ctx.pipe_fetch_wait(slot)
        for i in range(n):
            if (first_id + i) % gap == 0:
                assert counts[i] == want[i // 2], "%s in a %d x %d ROI: %d components, expected %d" % (ROI_TOPOLOGIES[i // 2], h, w, counts[i], want[i // 2])
            else:
                assert counts[i] == 0xFFFFFFFF
    ctx.close()
