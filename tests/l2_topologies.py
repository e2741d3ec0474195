"""A named catalogue of binary maps for reduction level 2 (pyrecode_amd/csrc/rc_l2.hip) - CPU code, numpy only.

The labelling stage cuts a frame three ways: 64-pixel words, tiles of 4096 pixels, work items of 64 tiles that belong to one workgroup each.
Bernoulli noise below the percolation threshold (about 0.41 for 8-connectivity) never makes a component that leaves its neighbourhood,
so it never makes two workgroups link into the same component.  The maps here do: long thin paths, combs that merge late, lattices
of roots, nested rings, runs longer than a tile.

Every entry is a function of (ny, nx, seed) and returns a Topology: the boolean map, a uint16 value image and - where the construction
gives one - the closed form: the number of components and, per component in raster order of its first pixel, that first pixel
(linear index), the maximum and the sum of the value image.  The closed form comes from the construction alone: an entry states which
set pixels belong together by an analytic KEY (the row of a `rows` map, (y + x) // 3 of a diagonal, the distance to the border of a
ring, ...) and how many components that makes by a formula; no labelling routine takes part.  tests/test_l2_topologies_cpu.py holds
the catalogue against scipy.ndimage.label and a serial flood fill.

Values are seeded and span the uint16 range whatever the packing depth d is, so that maxima exceed 2^d - 1 and sums wrap.  One large
component carries a planted maximum, at a position that seed % 3 selects: 0 its first pixel (the root of its tree), 1 its last pixel in
raster order (in the last work item wherever the component reaches it), 2 a pixel in the middle of its pixel list.
"""
import collections

import numpy as np

WORD_PX = 64
TILE_PX = 4096          # rc_device.h TILE_PX
ITEM_TILES = 64         # rc_l2.hip: a work item is 64 consecutive tiles of one frame
ITEM_PX = TILE_PX * ITEM_TILES
L2_ROUND = 1024         # rc_l2.hip: pixels k_l2_emit walks per round

# the smallest shapes with two work items (more than 262 144 pixels) at three word phases, one with three items, one single-item map
MULTI_ITEM = [(530, 517), (66, 4100), (8200, 33)]     # nx % 64 = 5; rows longer than a tile, nx % 64 = 4; several rows per word
THREE_ITEM = (1371, 383)                              # 129 tiles, nx % 64 = 63
SMALL = (9, 11)

VALUE_TOP = 64000       # ordinary values: 0 .. VALUE_TOP
PLANTED = 65300         # the planted maximum (frame = dark + 1 + value stays inside uint16 for dark <= 200)
DARK_TOP = 200

Closed = collections.namedtuple("Closed", "count first maximum total")   # first: int64 linear indices; maximum, total: int64


def n_items(ny, nx):
    return ((ny * nx + TILE_PX - 1) // TILE_PX + ITEM_TILES - 1) // ITEM_TILES


def tile_counts(binary):
    """Set pixels per tile of 4096 pixels (the last tile may be partial)."""
    flat = np.ascontiguousarray(binary, bool).ravel()
    pad = (-flat.size) % TILE_PX
    return np.concatenate([flat, np.zeros(pad, bool)]).reshape(-1, TILE_PX).sum(axis=1)


def item_counts(binary):
    """Set pixels per work item."""
    t = tile_counts(binary)
    pad = (-t.size) % ITEM_TILES
    return np.concatenate([t, np.zeros(pad, t.dtype)]).reshape(-1, ITEM_TILES).sum(axis=1)


def longest_run(binary):
    """Length of the longest horizontal run of set pixels."""
    best = 0
    for row in np.ascontiguousarray(binary, bool):
        edges = np.flatnonzero(np.diff(np.concatenate([[0], row.astype(np.int8), [0]])))
        if edges.size:
            best = max(best, int((edges[1::2] - edges[0::2]).max()))
    return best


class Topology:
    """binary: bool[ny, nx]; value: uint16[ny, nx]; closed: Closed of the value image, or None; plant: linear index of the planted maximum
    (or None: an empty map).  key / count: the construction's statement of the components (None for the ragged entries)."""

    def __init__(self, name, binary, key, count, seed):
        self.name, self.binary, self.key, self.count, self.seed = name, np.ascontiguousarray(binary, bool), key, count, seed
        ny, nx = self.binary.shape
        self.pos = np.flatnonzero(self.binary.ravel())
        self._comp = None
        if key is not None:
            # components in raster order of their first pixel: pos ascends, so np.unique's first occurrence is the first pixel
            _, first_at, inv = np.unique(np.asarray(key).ravel()[self.pos], return_index=True, return_inverse=True)
            order = np.argsort(first_at, kind="stable")
            rank = np.empty(order.size, np.int64)
            rank[order] = np.arange(order.size)
            self._comp = rank[inv.ravel()]
            self._first = self.pos[first_at[order]].astype(np.int64)
        rng = np.random.default_rng([int(seed), ny, nx, sum(name.encode())])
        self.value = rng.integers(0, VALUE_TOP + 1, (ny, nx)).astype(np.uint16)
        self.plant = None
        if self.pos.size:
            members = self.pos
            if self._comp is not None:
                big = int(np.argmax(np.bincount(self._comp)))        # the largest component (the earliest of equals)
                members = self.pos[self._comp == big]
            self.plant = int((members[0], members[-1], members[members.size // 2])[int(seed) % 3])
            self.value.ravel()[self.plant] = PLANTED
        self.closed = self.stats(self.value) if key is not None else None

    def stats(self, image):
        """The closed form of any image over this map: per component its first pixel, maximum and sum (int64)."""
        if self._comp is None:
            return None
        n = self._first.size
        v = np.asarray(image).ravel()[self.pos].astype(np.int64)
        mx = np.full(n, -1, np.int64)
        np.maximum.at(mx, self._comp, v)
        total = np.zeros(n, np.int64)
        np.add.at(total, self._comp, v)
        return Closed(int(self.count), self._first, mx, total)


# ---- frames --------------------------------------------------------------------------------------------------------------------
def dark_image(ny, nx, seed, dtype=np.uint16):
    top = DARK_TOP if np.dtype(dtype) == np.uint16 else 1
    return np.random.default_rng([int(seed), ny, nx, 77]).integers(0, top + 1, (ny, nx)).astype(dtype)


def frame_of(topo, dark):
    """dark + 1 + value at set pixels, <= dark elsewhere: with epsilon 0, frame > dark is the map and the raw frame value the statistic's
    input.  uint8 darks: the value image scaled to the byte (the planted maximum stays the strict maximum)."""
    rng = np.random.default_rng([int(topo.seed), 99])
    below = np.floor(rng.random(dark.shape) * (dark.astype(np.float64) + 1)).astype(np.int64)
    value = topo.value.astype(np.int64) if dark.dtype == np.uint16 else topo.value.astype(np.int64) // 260
    frame = np.where(topo.binary, dark.astype(np.int64) + 1 + value, below)
    assert frame.max() <= np.iinfo(dark.dtype).max
    return frame.astype(dark.dtype)


# ---- the entries ---------------------------------------------------------------------------------------------------------------
def _one(binary):
    return np.zeros(binary.shape, np.int64), 1 if binary.any() else 0


def _yx(ny, nx):
    return np.mgrid[:ny, :nx]


def serpentine(ny, nx, seed=0):
    """Every other row full, joined alternately at the right and the left end: one path of about N / 2 pixels."""
    b = np.zeros((ny, nx), bool)
    b[::2, :] = True
    for k, y in enumerate(range(1, ny - 1, 2)):
        b[y, nx - 1 if k % 2 == 0 else 0] = True
    return Topology("serpentine", b, *_one(b), seed)


def comb_down(ny, nx, seed=0):
    """Every other column full, joined by a full LAST row: every tooth is a root until the last row merges them."""
    b = np.zeros((ny, nx), bool)
    b[:, ::2] = True
    b[ny - 1, :] = True
    return Topology("comb_down", b, *_one(b), seed)


def comb_up(ny, nx, seed=0):
    """Every other column full, joined by a full FIRST row: every tooth hangs on the first run from the start."""
    b = np.zeros((ny, nx), bool)
    b[:, ::2] = True
    b[0, :] = True
    return Topology("comb_up", b, *_one(b), seed)


def checkerboard(ny, nx, seed=0):
    """(y + x) % 2 == 0: diagonal neighbours only.  One component - unless the map is one pixel wide or high: then no two set pixels touch."""
    y, x = _yx(ny, nx)
    b = (y + x) % 2 == 0
    if min(ny, nx) >= 2:
        return Topology("checkerboard", b, *_one(b), seed)
    return Topology("checkerboard", b, y * nx + x, (max(ny, nx) + 1) // 2, seed)


def lattice(ny, nx, seed=0):
    """[::2, ::2]: every set pixel a component of its own, the statistics are the values in raster order."""
    y, x = _yx(ny, nx)
    b = (y % 2 == 0) & (x % 2 == 0)
    return Topology("lattice", b, y * nx + x, ((ny + 1) // 2) * ((nx + 1) // 2), seed)


def diagonals(ny, nx, seed=0):
    """(y + x) % 3 == 0: anti-diagonals two pixels apart, one component per value of y + x (NE links only)."""
    y, x = _yx(ny, nx)
    return Topology("diagonals", (y + x) % 3 == 0, (y + x) // 3, (ny + nx - 1 + 2) // 3, seed)


def diagonals_mirror(ny, nx, seed=0):
    """The mirror image of `diagonals`: NW links only."""
    y, x = _yx(ny, nx)
    s = y + (nx - 1 - x)
    return Topology("diagonals_mirror", s % 3 == 0, s // 3, (ny + nx - 1 + 2) // 3, seed)


def rings(ny, nx, seed=0):
    """One-pixel rectangles nested at spacing 2: the pixels whose distance to the border is even; one component per such distance."""
    y, x = _yx(ny, nx)
    dist = np.minimum(np.minimum(y, ny - 1 - y), np.minimum(x, nx - 1 - x))
    return Topology("rings", dist % 2 == 0, dist // 2, (min(ny, nx) + 3) // 4, seed)


def spiral(ny, nx, seed=0):
    """A rectangular spiral, one pixel wide with a gap of one: the longest path a frame admits."""
    b = np.zeros((ny, nx), bool)
    top, left, bot, right = 0, 0, ny - 1, nx - 1
    b[top, left:right + 1] = True
    while True:
        b[top:bot + 1, right] = True                 # down the right side
        if right - left < 2 or bot - top < 2:
            break
        b[bot, left:right + 1] = True                # back along the bottom
        top += 2
        if bot < top:
            break
        b[top:bot + 1, left] = True                  # up the left side, to two rows under the turn before
        right -= 2
        if right < left:
            break
        b[top, left:right + 1] = True                # and in again
        bot -= 2
        if bot < top:
            break
        left += 2
    return Topology("spiral", b, *_one(b), seed)


def rows(ny, nx, seed=0):
    """Every other row full, not joined: one component per full row, one run each."""
    y, x = _yx(ny, nx)
    return Topology("rows", y % 2 == 0, y, (ny + 1) // 2, seed)


def rows_odd(ny, nx, seed=0):
    """The other phase of `rows`: the odd rows.  At the multi-item geometries the row that crosses the boundary between the first two
    work items is an odd one, so here one run begins in one item and ends in the next."""
    y, x = _yx(ny, nx)
    return Topology("rows_odd", y % 2 == 1, y, ny // 2, seed)


def columns(ny, nx, seed=0):
    """Every other column full: one component per column, N links only."""
    y, x = _yx(ny, nx)
    return Topology("columns", x % 2 == 0, x, (nx + 1) // 2, seed)


def vee(ny, nx, seed=0):
    """Two chains from the top of the frame that meet in the middle of the last row: one late merge.  A chain moves at most one column
    per row (frames higher than wide: vertical stretches with diagonal steps), so it is 8-connected all the way."""
    b = np.zeros((ny, nx), bool)
    c = (nx - 1) // 2
    k = np.arange(ny)                                                # rows above the last one
    dx = k if c >= ny - 1 else (k * c) // max(ny - 1, 1)
    b[ny - 1 - k, c - dx] = True
    b[ny - 1 - k, c + dx] = True
    return Topology("vee", b, *_one(b), seed)


def full(ny, nx, seed=0):
    b = np.ones((ny, nx), bool)
    return Topology("full", b, *_one(b), seed)


def empty(ny, nx, seed=0):
    b = np.zeros((ny, nx), bool)
    return Topology("empty", b, *_one(b), seed)


def ringed(inner):
    """`inner` two pixels inside a one-pixel ring along the frame's border.  A one-component entry gives one number whichever of its
    pixels ends up as the root of its tree; with the ring around it there are two components, and the ring's first pixel is the frame's
    first while its last is the frame's last: statistics listed in the order of any pixel but the first come out swapped."""
    def make(ny, nx, seed=0):
        b = np.zeros((ny, nx), bool)
        b[0, :] = b[ny - 1, :] = b[:, 0] = b[:, nx - 1] = True
        key, count = np.zeros((ny, nx), np.int64), 1
        if ny > 4 and nx > 4:
            t = inner(ny - 4, nx - 4, seed)
            b[2:ny - 2, 2:nx - 2] = t.binary
            key[2:ny - 2, 2:nx - 2] = np.asarray(t.key) + 1
            count += t.count
        return Topology(make.__name__, b, key, count, seed)
    make.__name__ = "ringed_" + inner.__name__
    make.__doc__ = "%s inside a ring along the border." % inner.__name__
    return make


def bernoulli(p, name=None):
    def make(ny, nx, seed=0):
        b = np.random.default_rng([int(seed), ny, nx, int(p * 1000)]).random((ny, nx)) < p
        return Topology(make.__name__, b, None, None, seed)
    make.__name__ = name or "bernoulli_%03d" % round(p * 100)
    make.__doc__ = "Bernoulli noise at p = %.2f (no closed form: checked against scipy only)." % p
    return make


percolating_041 = bernoulli(0.41, "percolating_041")   # at the site-percolation threshold of 8-connectivity: ragged components of every size
percolating_045 = bernoulli(0.45, "percolating_045")   # above it: one component holds most of the set pixels
bernoulli_050 = bernoulli(0.50)


def clustered(ny, nx, seed=0):
    """The workload's own shape (pyrecode_amd.synth.frames_clustered, 11 000 ppm of seed pixels) - no closed form."""
    from pyrecode_amd import synth
    dark = synth.dark_frame(seed, ny * nx)
    frame = synth.frames_clustered(seed, 0, 1, nx, ny, 11000, dark).reshape(ny, nx)
    return Topology("clustered", frame > dark.reshape(ny, nx), None, None, seed)


ONE_COMPONENT = ("serpentine", "comb_down", "comb_up", "checkerboard", "spiral", "vee", "full")   # at the multi-item geometries
RINGED = collections.OrderedDict((f.__name__, f) for f in (ringed(globals()[n]) for n in ONE_COMPONENT))
CLOSED_FORM = collections.OrderedDict((f.__name__, f) for f in (
    serpentine, comb_down, comb_up, checkerboard, lattice, diagonals, diagonals_mirror, rings, spiral, rows, rows_odd, columns, vee, full, empty)
    + tuple(RINGED.values()))
RAGGED = collections.OrderedDict((f.__name__, f) for f in (percolating_041, percolating_045, bernoulli_050, clustered))
CATALOGUE = collections.OrderedDict(list(CLOSED_FORM.items()) + list(RAGGED.items()))
