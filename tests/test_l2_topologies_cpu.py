"""The level-2 topology catalogue (tests/l2_topologies.py) is itself under test: its closed forms against scipy.ndimage.label at every
geometry the GPU tests use, scipy against a serial flood fill on small maps, and the properties the GPU tests rely on."""
import numpy as np
import pytest
import scipy.ndimage as nd

import l2_topologies as lt

EIGHT = np.ones((3, 3), int)
GEOMETRIES = lt.MULTI_ITEM + [lt.THREE_ITEM, lt.SMALL, (128, 128), (37, 128), (128, 1), (1, 300), (2, 4097), (3, 2)]
FLOOD_GEOMETRIES = [lt.SMALL, (1, 70), (70, 1), (37, 128), (64, 65), (13, 300), (2, 2)]    # at most 5000 pixels each


def flood_fill(binary):
    """Plain serial labelling: components in raster order of their first pixel, an explicit stack, 8 neighbours."""
    ny, nx = binary.shape
    labels = [[0] * nx for _ in range(ny)]
    grid = binary.tolist()
    n = 0
    for y0 in range(ny):
        for x0 in range(nx):
            if not grid[y0][x0] or labels[y0][x0]:
                continue
            n += 1
            labels[y0][x0] = n
            stack = [(y0, x0)]
            while stack:
                y, x = stack.pop()
                for dy in (-1, 0, 1):
                    for dx in (-1, 0, 1):
                        yy, xx = y + dy, x + dx
                        if 0 <= yy < ny and 0 <= xx < nx and grid[yy][xx] and not labels[yy][xx]:
                            labels[yy][xx] = n
                            stack.append((yy, xx))
    return np.array(labels, np.int64).reshape(ny, nx), n


def scipy_form(binary, image):
    labels, n = nd.label(binary, structure=EIGHT)
    idx = np.arange(1, n + 1)
    f = image.astype(np.int64)
    flat = labels.ravel()
    pos = np.flatnonzero(flat)
    _, first_at = np.unique(flat[pos], return_index=True)                      # labels ascend: one first pixel per label, in label order
    first = pos[first_at]
    mx = np.asarray(nd.maximum(f, labels, idx), np.int64) if n else np.zeros(0, np.int64)
    total = np.asarray(nd.sum(f, labels, idx), np.int64) if n else np.zeros(0, np.int64)
    return n, first, mx, total


@pytest.mark.parametrize("ny,nx", GEOMETRIES)
@pytest.mark.parametrize("name", list(lt.CLOSED_FORM))
def test_closed_forms_are_what_scipy_labels(name, ny, nx):
    for seed in (0, 1, 2) if ny * nx <= 5000 else (0,):                          # (the planted maximum moves with the seed)
        t = lt.CLOSED_FORM[name](ny, nx, seed)
        assert t.binary.shape == (ny, nx) and t.value.dtype == np.uint16 and t.value.shape == (ny, nx)
        n, first, mx, total = scipy_form(t.binary, t.value)
        c = t.closed
        assert c.count == n == c.first.size, "%s %dx%d: the formula says %d components, the key %d, scipy %d" % (name, ny, nx, c.count, c.first.size, n)
        assert np.array_equal(c.first, first) and np.all(np.diff(c.first) > 0)
        assert np.array_equal(c.maximum, mx) and np.array_equal(c.total, total)
        if seed > 0:
            continue
        # the same for an image that is not the entry's own (the GPU tests take the closed form of the raw frame)
        frame = lt.frame_of(t, lt.dark_image(ny, nx, 5))
        assert np.array_equal(frame > lt.dark_image(ny, nx, 5), t.binary)
        n, first, mx, total = scipy_form(t.binary, frame)
        c = t.stats(frame)
        assert c.count == n and np.array_equal(c.first, first) and np.array_equal(c.maximum, mx) and np.array_equal(c.total, total)


@pytest.mark.parametrize("ny,nx", lt.MULTI_ITEM[:2] + [lt.SMALL, (128, 1), (1, 300)])
@pytest.mark.parametrize("name", list(lt.CATALOGUE))
def test_planted_maximum_sits_where_the_seed_says(name, ny, nx):
    """Full-range values, and the planted maximum at the first, the last and a middle pixel of one large component."""
    seen = set()
    for seed in (0, 1, 2):
        t = lt.CATALOGUE[name](ny, nx, seed)
        if not t.binary.any():
            assert t.plant is None
            continue
        assert t.binary.ravel()[t.plant] and t.value.ravel()[t.plant] == lt.PLANTED
        assert int(t.value.max()) == lt.PLANTED and int((t.value == lt.PLANTED).sum()) == 1
        if t.closed is not None:
            labels, n = nd.label(t.binary, structure=EIGHT)
            sizes = np.bincount(labels.ravel())[1:]
            members = np.flatnonzero(labels.ravel() == labels.ravel()[t.plant])
            assert members.size == sizes.max()
        else:
            members = t.pos
        assert t.plant == (members[0], members[-1], members[members.size // 2])[seed]
        seen.add(t.plant)
        for dtype in (np.uint16, np.uint8):
            dark = lt.dark_image(ny, nx, 3, dtype)
            frame = lt.frame_of(t, dark)
            assert frame.dtype == dtype and np.array_equal(frame > dark, t.binary)
            assert int(np.argmax(frame)) == t.plant and int((frame == frame.max()).sum()) == 1
    if name in lt.ONE_COMPONENT and (ny, nx) in lt.MULTI_ITEM:
        assert len(seen) == 3


@pytest.mark.parametrize("ny,nx", FLOOD_GEOMETRIES)
def test_scipy_agrees_with_a_serial_flood_fill(ny, nx):
    assert ny * nx <= 5000
    for name, make in lt.CATALOGUE.items():
        t = make(ny, nx, 1)
        want, n = flood_fill(t.binary)
        labels, m = nd.label(t.binary, structure=EIGHT)
        assert m == n and np.array_equal(labels, want), "%s %dx%d" % (name, ny, nx)
        if t.closed is not None:
            assert t.closed.count == n
            assert np.array_equal(t.closed.first, [int(np.flatnonzero(want.ravel() == k)[0]) for k in range(1, n + 1)])


def test_geometries_make_the_items_the_gpu_tests_count_on():
    assert [lt.n_items(ny, nx) for ny, nx in lt.MULTI_ITEM] == [2, 2, 2]
    assert [nx % 64 for _, nx in lt.MULTI_ITEM] == [5, 4, 33]
    assert lt.n_items(*lt.THREE_ITEM) == 3 and lt.THREE_ITEM[1] % 64 in (0, 1, 63)
    assert lt.n_items(*lt.SMALL) == 1
    for ny, nx in lt.MULTI_ITEM:     # the smallest: a tile less and one item would do
        assert (ny * nx + lt.TILE_PX - 1) // lt.TILE_PX <= lt.ITEM_TILES + 4


@pytest.mark.parametrize("ny,nx", lt.MULTI_ITEM + [lt.THREE_ITEM])
def test_one_component_entries_reach_every_item(ny, nx):
    for name in lt.ONE_COMPONENT:
        t = lt.CATALOGUE[name](ny, nx, 0)
        assert t.closed.count == 1
        per_item = lt.item_counts(t.binary)
        assert per_item.size == lt.n_items(ny, nx) and (per_item > 0).all(), "%s %dx%d: %s" % (name, ny, nx, per_item)
        assert t.plant < lt.ITEM_PX                                       # seed 0: in the first item,
        assert lt.CATALOGUE[name](ny, nx, 1).plant >= (lt.n_items(ny, nx) - 1) * lt.ITEM_PX   # seed 1: in the last
    for name in ("diagonals", "diagonals_mirror", "rings"):               # components that are each in more than one item
        t = lt.CATALOGUE[name](ny, nx, 0)
        labels, n = nd.label(t.binary, structure=EIGHT)
        items = [np.unique(np.flatnonzero(labels.ravel() == k) // lt.ITEM_PX).size for k in range(1, n + 1, max(1, n // 40))]
        assert max(items) >= 2, (name, items)


@pytest.mark.parametrize("ny,nx", lt.MULTI_ITEM + [lt.THREE_ITEM])
def test_ringed_entries_hold_two_components_whose_first_and_last_pixels_nest(ny, nx):
    for name, make in lt.RINGED.items():
        t = make(ny, nx, 0)
        assert t.closed.count == 2 and t.closed.first[0] == 0
        labels, n = nd.label(t.binary, structure=EIGHT)
        last = [int(np.flatnonzero(labels.ravel() == k)[-1]) for k in (1, 2)]
        assert last[0] == ny * nx - 1 > last[1] > t.closed.first[1]
        assert (lt.item_counts(labels == 1) > 0).all()
        if ny * nx - lt.ITEM_PX >= 3 * nx:                                   # (66 x 4100 has two rows in its second item: the ring's)
            assert (lt.item_counts(labels == 2) > 0).sum() >= 2, name       # the inner component is in more than one item too


def test_lattice_tiles_sit_at_the_emit_round():
    """k_l2_emit walks L2_ROUND = 1024 pixels a round: a list that is all roots at exactly that boundary, and tiles on both sides of it."""
    assert set(lt.tile_counts(lt.lattice(128, 128).binary)) == {lt.L2_ROUND}
    assert lt.tile_counts(lt.lattice(256, 128).binary).tolist() == [lt.L2_ROUND] * 8
    c = lt.tile_counts(lt.lattice(530, 517).binary)[:-1]                  # (the last tile is partial)
    assert c.min() < lt.L2_ROUND < c.max() and (c.min(), c.max()) == (1016, 1036)


def test_rows_run_longer_than_a_tile_at_every_phase():
    t = lt.rows(66, 4100)
    assert lt.longest_run(t.binary) == 4100 > lt.TILE_PX
    starts = np.arange(0, 66, 2) * 4100
    assert len(set(starts % 64)) == 8 and len(set(starts % lt.TILE_PX)) == 33    # runs begin at many word phases and tile phases
    for ny, nx in lt.MULTI_ITEM:                                                   # the odd rows: one run crosses the item boundary
        assert (lt.ITEM_PX // nx) % 2 == 1 and lt.ITEM_PX % nx != 0
        b = lt.rows_odd(ny, nx).binary.ravel()
        assert b[lt.ITEM_PX - 1] and b[lt.ITEM_PX]
    assert lt.longest_run(lt.rows_odd(66, 4100).binary) == 4100
    assert lt.longest_run(lt.serpentine(66, 4100).binary) == 4100


def test_dense_entries_take_the_big_tile_paths():
    """checkerboard: half of every tile set - more than k_l2_emit's round and more linked pixels per 64 words than k_l2_link lists."""
    c = lt.tile_counts(lt.checkerboard(530, 517).binary)[:-1]
    assert c.min() >= 2047 > lt.L2_ROUND
    assert set(lt.tile_counts(lt.full(530, 517).binary)[:-1]) == {lt.TILE_PX}


def test_percolating_entries_hold_components_of_many_items():
    for make, least in ((lt.percolating_041, 20000), (lt.percolating_045, 100000)):
        t = make(530, 517, 0)
        labels, n = nd.label(t.binary, structure=EIGHT)
        sizes = np.bincount(labels.ravel())[1:]
        big = np.flatnonzero(labels.ravel() == 1 + int(np.argmax(sizes)))
        assert sizes.max() >= least and np.unique(big // lt.ITEM_PX).size == 2 and n > 1000
