"""-m gpu: every route through expand_run (pyrecode_amd/csrc/rc_reader.hip) on one tiny batch - 3 frames of 65 x 3 pixels (195: no multiple
of 8 or 64), level 1 at 12 bits as stored streams and as streams of the device zlib encoder (the one codec whose page-locked triplets and COO
are filled by rc_expand_frames_wait and not by an eager copy), and a stored level-2 form for the statistics kind.  Every result kind, in the
synchronous form and as submit + wait, into device, page-locked and pageable memory where the form admits it, against numpy and the CPU
models of the counting tests: status, prefix and the output over the entries the prefix announces.  Then the refusals - capacity one
entry short, the last value stream one field short, both - with their status and a fragment of rc_last_error per kind and form.

The statuses of "both at once" are the answers of the library as it was before expand_run took one request (commit 4090e1e): this file
was run against that library first and passed there unchanged."""
import zlib

import numpy as np
import pytest

import centroid_model as cm
import counted_view_model as cv
from test_gpu_dense import _Out                                  # an output between guard cells, prefilled with 0xA5
from test_gpu_frame_sums import _pack_fields, _stored_batch
from test_gpu_inflate import _device_records

pytestmark = pytest.mark.gpu
NY, NX, D, N = 3, 65, 12, 3
NB = (NY * NX + 7) // 8
WHERES = ("device", "pinned", "host")
SHORT = "value stream shorter"
FEWER = "triplets holds fewer"


@pytest.fixture(scope="module")
def hip():
    import torch  # noqa: F401 - before the library: one HIP runtime per process
    from pyrecode_amd import _lib
    if _lib.device_count() == 0:
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    return _lib


@pytest.fixture(scope="module")
def batch(hip):
    """the frames (20 random pixels | the first and the last pixel | 30 random pixels and a run of 30 across a word boundary), their stored
    and device-zlib streams, the level-2 form (the same maps; 2, 1 and 3 statistics), and what every kind has to give"""
    rng = np.random.default_rng(NY * NX)
    vals = np.zeros((N, NY * NX), np.uint32)
    for z, k in ((0, 20), (2, 30)):
        at = rng.choice(NY * NX, k, replace=False)
        vals[z, at] = rng.integers(1, 1 << D, k)
    vals[1, 0], vals[1, -1] = 7, (1 << D) - 1
    vals = vals.reshape(N, NY, NX)
    vals[2, 1, 10:40] = 9
    b = {"vals": vals}
    blob, sizes, where = _stored_batch(vals, D, 1, rng)
    b["stored"] = (0, 0, blob, sizes)
    zblobs, zsizes = _device_records(hip, vals.astype(np.uint16), np.zeros((NY, NX), np.uint16), D, 1, 1)
    for z in range(N):          # the device encoder's streams hold the stored pieces: one expectation serves both sets
        cb, cp = int(zsizes[z, 0]), int(zsizes[z, 1])
        at, size = where[z]
        assert zlib.decompress(zblobs[z][:cb].tobytes()) == blob[at - NB:at].tobytes()
        assert zlib.decompress(zblobs[z][cb:cb + cp].tobytes()) == blob[at:at + size].tobytes() and int(zsizes[z, 2]) == size
    b["zdev"] = (1, hip.RC_SCHEME_ZLIB_DEVICE, np.ascontiguousarray(np.concatenate(zblobs)), zsizes)
    # one field short: the last frame's value bytes and its sizes entries together - the mode-0 size check still passes
    at, size = where[N - 1]
    keep = ((int((vals[N - 1] != 0).sum()) - 1) * D + 7) // 8
    assert keep < size and at + size == blob.size
    short_sizes = sizes.copy()
    short_sizes[N - 1, 1] = short_sizes[N - 1, 2] = keep
    b["short"] = (0, 0, np.ascontiguousarray(blob[:at + keep]), short_sizes)
    stats = [rng.integers(0, 1 << D, k).astype(np.uint16) for k in (2, 1, 3)]
    parts, sizes2 = [], np.zeros((N, 3), np.uint32)
    for z in range(N):
        packed = _pack_fields(stats[z], D)
        parts += [blob[where[z][0] - NB:where[z][0]], packed]
        sizes2[z] = (NB, packed.size, packed.size)
    b["l2"] = (0, 0, np.ascontiguousarray(np.concatenate(parts)), sizes2)
    b["stats"] = np.concatenate(stats)
    rows, cols = zip(*(np.nonzero(v) for v in vals))
    b["prefix"] = np.concatenate([[0], np.cumsum([r.size for r in rows])]).astype(np.uint64)
    b["rows"], b["cols"] = np.concatenate(rows), np.concatenate(cols)
    b["v"] = np.concatenate([v[v != 0] for v in vals])
    frames = [(v != 0, v.astype(np.uint16)) for v in vals]
    b["events"] = cm.count_batch(frames, cm.METHODS[0], 0)
    comps = cv.components(frames, cm.METHODS[0], 0)
    b["counted"] = cv.view_of(comps, (NY, NX), 1)
    yy, xx = np.mgrid[:NY, :NX]
    v64 = vals.astype(np.int64)
    b["trace"] = np.stack([(vals != 0).reshape(N, -1).sum(1), v64.reshape(N, -1).sum(1), (v64 * yy).reshape(N, -1).sum(1), (v64 * xx).reshape(N, -1).sum(1)], 1)
    return b


def _body(out):
    return (out.t.cpu().numpy() if out.where == "device" else out.a)[out.lo:out.lo + out.cells]


class _Kind:
    """one result kind on one set of streams: sync(prefix, cap) and submit(slot, cap) call the library, check(cap) judges what it left.
    esz: bytes per entry (0: no capacity); cells: bytes of an output whose size the arguments give; total: the entries a good batch has"""
    esz, cells, level, sets = 0, 0, 1, ("stored", "zdev")
    cap_fragment = FEWER

    def __init__(self, hip, b, src, where):
        self.hip, self.L, self.b, self.where = hip, hip.lib(), b, where
        self.mode, self.scheme, self.blob, self.sizes = b[src]
        self.src = (self.mode, self.scheme, hip.ptr(self.blob), hip.ptr(self.sizes), N)
        self.geom = (NX, NY, D, self.level)
        self.total = int(b["prefix"][N])
        self.want_prefix = b["prefix"]
        self.out = None

    def room(self, cap):
        if self.out is not None:
            self.out.close()
        self.cap = cap
        self.out = _Out(self.hip, max(cap * self.esz + self.cells, 1), np.uint8, self.where)

    def close(self):
        if self.out is not None:
            self.out.close()

    def arrays(self, widths):
        """the arrays of a COO-like output, cap entries apart: the `total` entries the prefix announces (what lies behind them is not judged:
        a submit's eager copy brings all cap entries of the staging buffer)"""
        body, at, got = _body(self.out), 0, []
        for dt in widths:
            size = np.dtype(dt).itemsize
            got.append(body[at:at + self.total * size].view(dt))
            at += self.cap * size
        self.out.check(body)          # (the guard cells)
        return got


class _Triplets(_Kind):
    esz, fn = 24, "rc_expand_frames"

    def sync(self, prefix):
        return getattr(self.L, self.fn)(*self.geom, *self.src, self.hip.ptr(prefix), self.out.ptr, self.cap)

    def submit(self, slot):
        return getattr(self.L, self.fn + "_submit")(slot, *self.geom, *self.src, self.out.ptr, self.cap)

    def check(self):
        t = _body(self.out)[:self.total * 24].view(np.uint64)
        self.out.check(_body(self.out))
        assert np.array_equal(t.reshape(-1, 3), np.stack([self.b["rows"], self.b["cols"], self.b["v"]], 1).astype(np.uint64))


class _Coo16(_Triplets):
    esz, fn, vt = 10, "rc_expand_frames_coo", np.uint16

    def check(self):
        r, c, v = self.arrays([np.int32, np.int32, self.vt])
        assert np.array_equal(r, self.b["rows"]) and np.array_equal(c, self.b["cols"]) and np.array_equal(v, self.b["v"])


class _Coo32(_Coo16):
    esz, fn, vt = 12, "rc_expand_frames_coo32", np.uint32


class _L2(_Kind):
    esz, level, sets = 8, 2, ("l2",)

    st = None

    def room(self, cap):
        super().room(cap)
        if self.st is not None:
            self.st.close()
        self.ns = self.b["stats"].size
        self.st = _Out(self.hip, self.ns, np.uint16, self.where)

    def close(self):
        super().close()
        self.st.close()

    def sync(self, prefix):
        return self.L.rc_expand_frames_l2(NX, NY, D, *self.src, self.hip.ptr(prefix), self.out.ptr, self.cap, self.st.ptr, self.ns)

    def submit(self, slot):
        return self.L.rc_expand_frames_l2_submit(slot, NX, NY, D, *self.src, self.out.ptr, self.cap, self.st.ptr, self.ns)

    def check(self):
        r, c = self.arrays([np.int32, np.int32])
        assert np.array_equal(r, self.b["rows"]) and np.array_equal(c, self.b["cols"])
        self.st.check(self.b["stats"])


class _Events(_Kind):
    esz, cap_fragment = 20, "rc_count_frames: events holds fewer"

    def __init__(self, *a):
        super().__init__(*a)
        self.want_prefix = self.b["events"][0]
        self.total = int(self.want_prefix[N])

    def sync(self, prefix):
        return self.L.rc_count_frames(*self.geom, *self.src, 0, 0, self.hip.ptr(prefix), self.out.ptr, self.cap)

    def submit(self, slot):
        return self.L.rc_count_frames_submit(slot, *self.geom, *self.src, 0, 0, self.out.ptr, self.cap)

    def check(self):
        w, r, c, a = self.arrays([np.uint64, np.int32, np.int32, np.uint32])
        _, rows, cols, area, weight = self.b["events"]
        assert np.array_equal(r, rows) and np.array_equal(c, cols) and np.array_equal(a, area) and np.array_equal(w, weight)


class _Sum(_Kind):
    fs = None

    def room(self, cap):
        self.fs = self.fs or self.hip.FrameSum(NX, NY)

    def close(self):
        self.fs.close()

    def sync(self, prefix):
        return self.fs.add_status(self.geom + (self.mode, self.scheme), self.blob, self.sizes, N, prefix)

    def submit(self, slot):
        return self.fs.submit_status(slot, self.geom + (self.mode, self.scheme), self.blob, self.sizes, N)

    def check(self):
        assert np.array_equal(self.fs.fetch(reset=True), self.b["vals"].sum(0, dtype=np.uint32))


class _Counted(_Sum):
    def __init__(self, *a):
        super().__init__(*a)
        self.want_prefix = self.b["events"][0]

    def sync(self, prefix):
        return self.fs.add_counted_status(self.geom + (self.mode, self.scheme), self.blob, self.sizes, N, 0, 0, 1, prefix)

    def submit(self, slot):
        return self.fs.submit_counted_status(slot, self.geom + (self.mode, self.scheme), self.blob, self.sizes, N, 0, 0, 1)

    def check(self):
        assert np.array_equal(self.fs.fetch(reset=True), self.b["counted"].astype(np.uint32))


class _Dense(_Kind):
    cells = N * NY * NX * 2

    def sync(self, prefix):
        return self.L.rc_expand_frames_dense(*self.geom, *self.src, 0, 0, NX, NY, 1, 1, 2, self.out.ptr, N * NY * NX, self.hip.ptr(prefix))

    def submit(self, slot):
        return self.L.rc_expand_frames_dense_submit(slot, *self.geom, *self.src, 0, 0, NX, NY, 1, 1, 2, self.out.ptr, N * NY * NX)

    def check(self):
        self.out.check(self.b["vals"].astype(np.uint16).view(np.uint8))


class _Trace(_Kind):
    cells = N * 4 * 8

    ft = None

    def room(self, cap):
        super().room(cap)
        self.ft = self.ft or self.hip.FrameTrace(NX, NY)

    def close(self):
        super().close()
        self.ft.close()

    def sync(self, prefix):
        return self.ft.frames_status(self.geom + (self.mode, self.scheme), self.blob, self.sizes, N, self.out.ptr, N * 4, prefix)

    def submit(self, slot):
        return self.ft.submit_status(slot, self.geom + (self.mode, self.scheme), self.blob, self.sizes, N, self.out.ptr, N * 4)

    def check(self):
        self.out.check(self.b["trace"].astype(np.int64).view(np.uint8))


KINDS = [_Triplets, _Coo16, _Coo32, _L2, _Events, _Sum, _Counted, _Dense, _Trace]


def _run(k, slot):
    """the synchronous form (slot None), or submit - with a second submit to the held slot refused - and wait: (status, prefix)"""
    hip = k.hip
    prefix = np.full(N + 1, 77, np.uint64)
    if slot is None:
        return k.sync(prefix), prefix
    st = k.submit(slot)
    if st != hip.RC_OK:
        return st, None
    assert k.submit(slot) == hip.RC_ERR_BAD_ARG and "submitted batch" in hip.last_error()
    return hip.lib().rc_expand_frames_wait(slot, hip.ptr(prefix)), prefix


@pytest.mark.parametrize("kind", KINDS, ids=lambda k: k.__name__[1:].lower())
def test_every_kind_form_and_destination(hip, batch, kind):
    """OK, the prefix and the output - with room for three entries more than the batch has, and with none to spare"""
    for src in kind.sets:
        for where in WHERES if kind.esz or kind.cells else ("device",):
            for slot in (None, 1):
                k = kind(hip, batch, src, where)
                for spare in (3, 0):
                    k.room(k.total + spare)
                    st, prefix = _run(k, slot)
                    if slot is not None and where == "host":
                        assert st == hip.RC_ERR_BAD_ARG and "page-locked" in hip.last_error(), (src, st, hip.last_error())
                        assert hip.lib().rc_expand_frames_wait(slot, hip.ptr(np.zeros(N + 1, np.uint64))) == hip.RC_ERR_BAD_ARG     # (nothing was queued)
                        continue
                    assert st == hip.RC_OK, (src, where, slot, spare, st, hip.last_error())
                    assert np.array_equal(prefix, k.want_prefix), (src, where, slot, prefix)
                    k.check()
                k.close()


# (status, fragment of rc_last_error) of the synchronous form and of rc_expand_frames_wait
S, C = -2, -6          # RC_ERR_OUT_TOO_SMALL, RC_ERR_CORRUPT
REFUSALS = {
    # capacity one entry short           the last value stream one field short      both at once (the earlier library's answers)
    _Triplets: (((S, FEWER), (S, FEWER)), ((C, SHORT), (C, SHORT)), ((S, FEWER), (S, FEWER))),
    _Coo16: (((S, FEWER), (S, FEWER)), ((C, SHORT), (C, SHORT)), ((S, FEWER), (S, FEWER))),
    _Coo32: (((S, FEWER), (S, FEWER)), ((C, SHORT), (C, SHORT)), ((S, FEWER), (S, FEWER))),
    _L2: (((S, FEWER), (S, FEWER)), None, None),                  # (level 2: the statistics stream has no field per set pixel)
    _Events: (((S, _Events.cap_fragment), (S, FEWER)), ((C, SHORT), (C, SHORT)), ((C, SHORT), (C, SHORT))),
    _Sum: (None, ((C, SHORT), (C, SHORT)), None),
    _Counted: (None, ((C, SHORT), (C, SHORT)), None),
    _Dense: (None, ((C, SHORT), (C, SHORT)), None),
    _Trace: (None, ((C, SHORT), (C, SHORT)), None),
}


@pytest.mark.parametrize("kind", KINDS, ids=lambda k: k.__name__[1:].lower())
def test_refusals_by_kind_and_form(hip, batch, kind):
    assert (S, C) == (hip.RC_ERR_OUT_TOO_SMALL, hip.RC_ERR_CORRUPT)
    for case, (want, src, short_by) in enumerate(zip(REFUSALS[kind], (kind.sets[0], "short", "short"), (1, 0, 1))):
        if want is None:
            continue
        for where in ("device", "pinned", "host") if kind.esz or kind.cells else ("device",):
            for slot in (None, 0) if where != "host" else (None,):
                k = kind(hip, batch, src, where)
                k.room(k.total - short_by)
                st, _ = _run(k, slot)
                status, fragment = want[slot is not None]
                assert st == status and fragment in hip.last_error(), (case, where, slot, st, hip.last_error())
                k.close()
