"""Life cycle of the host layer behind the C ABI (rc_api.hip, rc_codec_api.hip): every byte a ctx allocates comes back when it is
destroyed, a refused rc_ctx_create leaves nothing behind, "the most recent batch" is the scratch set that batch used, and the stateless
seams 2 and 3 give the same bytes and statuses for host and device pointers at the sizes where their shared skeleton can go wrong."""
import ctypes as C
import ctypes.util

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NX, NY, B = 256, 250, 4            # N = 64 000: 3 whole tiles of 16 384 pixels and a partial one
WARM, CYCLES = 1, 8

# The frame of the memory test.  At 256 x 250 the bound below would not stay under the buffers it has to see, so the frame is enlarged until
# every buffer that scales with the geometry is one: 64 x hipMalloc(n) lowered free device memory by nothing for n = 16 .. 4096 and by
# 64 x 65 536 for n = 65 536 (MI355X, 2026-10-17) - the HIP runtime carves blocks below 64 KiB out of chunks of its own -, and the smallest
# geometry-scaled buffers are the per-tile dword arrays of a scratch set, max_batch * ntiles * 4 bytes: 4 * 4103 * 4 = 65 648 here.
# N = 16 805 900 is 4102 whole tiles and a partial one.  A batch is one frame; every buffer is sized by max_batch.
MEM_NX, MEM_NY = 4100, 4099

# Free device memory may fall by this much over CYCLES create / batch / sync / destroy cycles after the warm one: twice the fall of this
# same loop with the library of the commit before the memory owners (per-buffer free lists in rc_ctx_destroy).
# Measured on an MI355X on 2026-10-17, three runs of this module: 0 bytes in every one of the eight cycles of every form, and 0 for the refused creates; twice that is 0.  (Without
# the runtime_warm fixture, at 256 x 250, the first form of a process and the pipe-slot form each fell by 8 388 608 bytes, the eleven
# others by 0.)  The library with the owners gives the same figures.  A forgotten buffer of 64 KiB costs 8 x 64 KiB here.
# What the figure cannot see, at any frame size, because the allocation stays below 64 KiB or is not device memory: a set's status word,
# frame_nnz, frame_cbytes, frame_pbytes (max_batch * 4), zl_acc (max_batch * 32) and scan_part (2 176 bytes here); the ctx's first-error
# word, d_rec_off, d_md, zstd tables, model and sample; a pipe slot's d_rec, d_md and d_val; and every page-locked allocation (h_status,
# h_model, h_sample, a slot's h_rec, h_md, h_stat, h_val).  Those are checked by reading: each goes through the same owner as the rest.
SLACK_BYTES = 0


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


@pytest.fixture(scope="module")
def stacks():
    """Source stacks per pixel size, made once: {itemsize: (dark, frames[3 * B])} - three batches of distinct frames."""
    rng = np.random.default_rng(2026)
    out = {}
    for dt, lo, top in ((np.uint8, 10, 100), (np.uint16, 80, 2000), (np.uint32, 80, 500000)):
        dark = rng.integers(lo, lo + 40, (NY, NX)).astype(dt)
        hit = rng.random((3 * B, NY, NX)) < np.repeat([0.01, 0.02, 0.04], B)[:, None, None]   # (batches of clearly different record sizes)
        frames = np.where(hit, dark + rng.integers(1, top, (3 * B, NY, NX)), dark // 2).astype(dt)
        out[np.dtype(dt).itemsize] = (dark, frames)
    return out


@pytest.fixture(scope="module")
def big_stacks():
    """{itemsize: (dark, frames[1])} at the memory test's frame."""
    rng = np.random.default_rng(4100)
    out = {}
    for dt, lo, top in ((np.uint8, 10, 100), (np.uint16, 80, 2000), (np.uint32, 80, 500000)):
        dark = rng.integers(lo, lo + 40, (MEM_NY, MEM_NX), dtype=np.uint32).astype(dt)
        hit = rng.random((1, MEM_NY, MEM_NX), dtype=np.float32) < 0.02
        frames = np.where(hit, dark + rng.integers(1, top, (1, MEM_NY, MEM_NX), dtype=np.uint32), dark // 2).astype(dt)
        out[np.dtype(dt).itemsize] = (dark, frames)
    return out


@pytest.fixture(scope="module")
def runtime_warm(hip, big_stacks):
    """The HIP runtime grows pools of its own the first time a process runs a batch and the first time it uses the copy streams and
    page-locked slot buffers of the streaming form (8 MiB each, seen at the parent commit and at this one alike): both happen here, once,
    before anything is measured."""
    for form in ("l1-lz4", "l1-lz4-pipe-slots"):
        for _ in range(WARM + CYCLES):
            _cycle(hip, big_stacks, form)


def _free_bytes():
    import torch
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info(0)[0]


# name -> (depth, level, op_mode, scheme, clevel, dtype, mode); mode: "sync", "pipelined" (rc_ctx_set_pipelined(1) first) or "pipe" (rc_pipe_*)
FORMS = {
    "l1-lz4": (12, 1, 1, 2, 1, np.uint16, "sync"),
    "l1-zstd-fast": (12, 1, 1, 1, 0, np.uint16, "sync"),
    "l1-zstd-modelled": (12, 1, 1, 1, 1, np.uint16, "sync"),
    "l1-blosc": (12, 1, 1, 8, 1, np.uint16, "sync"),
    "l1-device-zlib": (12, 1, 1, 0x100, 1, np.uint16, "sync"),
    "l1-no-device-codec": (12, 1, 0, 0, 1, np.uint16, "sync"),
    "l3-lz4": (12, 3, 1, 2, 1, np.uint16, "sync"),
    "u8-l1-lz4": (8, 1, 1, 2, 1, np.uint8, "sync"),
    "u32-l1-zstd": (20, 1, 1, 1, 1, np.uint32, "sync"),     # (created as a modelled-zstd uint16 ctx: rc_ctx_set_source_bytes replaces and frees)
    "u32-l3-zstd": (20, 3, 1, 1, 1, np.uint32, "sync"),
    "l2-plain": (12, 2, 1, 2, 1, np.uint16, "sync"),
    "l2-pipelined": (12, 2, 1, 2, 1, np.uint16, "pipelined"),   # the second chain's workspace exists
    "l1-lz4-pipe-slots": (12, 1, 1, 2, 1, np.uint16, "pipe"),
}


def _cycle(hip, stacks, form):
    depth, level, op_mode, scheme, clevel, dt, mode = FORMS[form]
    dark, frames = stacks[np.dtype(dt).itemsize]
    ctx = hip.ReduceContext(MEM_NX, MEM_NY, depth, level, op_mode, scheme, clevel, 0, max_batch=B, src_dtype=dt)
    ctx.set_dark(dark, 0)
    if mode == "pipelined":
        ctx.set_pipelined(True)
    if mode == "pipe":
        ctx.set_validation(1, 0, 0, 64, 64)
        dst = np.empty(ctx.out_capacity(1), np.uint8)
        for slot in range(hip.PIPE_SLOTS):
            ctx.pipe_submit(slot, frames, 1, slot)
        for slot in range(hip.PIPE_SLOTS):
            rec, md, total = ctx.pipe_result(slot, 1)
            assert rec[0] == 0 and int(rec[1]) == total and total > 0
            assert (ctx.pipe_validation(slot, 1) != 0xFFFFFFFF).all()
            ctx.pipe_fetch(slot, dst, total)
            ctx.pipe_fetch_wait(slot)
    else:
        out, rec, md = ctx.reduce_compress_batch(frames, first_frame_id=0)
        assert rec[0] == 0 and rec[1] > 0
    ctx.sync()
    ctx.close()


@pytest.mark.parametrize("form", list(FORMS))
def test_destroy_returns_every_byte_a_ctx_allocated(hip, big_stacks, runtime_warm, form):
    for _ in range(WARM):
        _cycle(hip, big_stacks, form)
    free = [_free_bytes()]
    for _ in range(CYCLES):
        _cycle(hip, big_stacks, form)
        free.append(_free_bytes())
    fall = free[0] - free[-1]
    print("lifecycle %-20s free memory fell by %d bytes over %d cycles (per cycle: %s)" % (form, fall, CYCLES, [a - b for a, b in zip(free, free[1:])]))
    assert fall <= SLACK_BYTES


def test_a_refused_create_leaves_nothing_behind(hip):
    L = hip.lib()
    _free_bytes()
    before = _free_bytes()
    refused = [(0, NY, 12, 1), (NX, NY, 12, 4), (65536, 65536, 12, 1), (NX, NY, 33, 1), (70000, 8, 12, 2)]   # nx, ny, depth, level
    for nx, ny, depth, level in refused:
        st = C.c_int(0)
        assert not L.rc_ctx_create(nx, ny, depth, level, 1, 2, 1, 0, B, C.byref(st))
        assert st.value in (hip.RC_ERR_BAD_ARG, hip.RC_ERR_UNSUPPORTED) and hip.last_error() != ""
    fall = before - _free_bytes()
    print("lifecycle refused creates: free memory fell by %d bytes" % fall)
    assert fall <= SLACK_BYTES


def _async_buffers(frames):
    import torch
    dev = torch.device("cuda", 0)
    view = {1: np.uint8, 2: np.int16, 4: np.int32}[frames.dtype.itemsize]
    cap = B * NY * NX * frames.dtype.itemsize
    bufs = [(torch.zeros(cap, dtype=torch.uint8, device=dev), torch.zeros(B + 1, dtype=torch.int64, device=dev),
             torch.zeros((B, 3), dtype=torch.int32, device=dev)) for _ in range(2)]
    fr_d = torch.from_numpy(frames.view(view)).to(dev)
    torch.cuda.synchronize()
    return fr_d, bufs, cap


def _batch_and_check_maps(ctx, orc, fr_d, bufs, cap, frames, thr, b):
    out, rec, md = bufs[b & 1]
    ctx.enqueue(fr_d[b * B].data_ptr(), B, b * B, out.data_ptr(), cap, rec.data_ptr(), md.data_ptr())
    ctx.wait_results()
    for i in range(B):
        assert np.array_equal(ctx.binary_map(i), orc.pack_binary_frame(frames[b * B + i] > thr)), "batch %d frame %d" % (b, i)


def test_most_recent_batch_is_the_set_that_batch_used(hip, orc, stacks):
    """Pipelined, binary maps kept: consecutive batches alternate between the two scratch sets; rc_get_binary_map and the status word
    rc_ctx_sync reads belong to the batch enqueued last.  The three batches' records differ clearly in size (1 %, 2 %, 4 % of the pixels
    set), so a status word taken from the other set shows: the synchronous call copies exactly `status.total` bytes to a host caller, and
    the streaming form hands `status.total` out as a slot's total."""
    dark, frames = stacks[2]
    thr = orc.threshold(dark, 0)
    ctx = hip.ReduceContext(NX, NY, 12, 1, 1, 2, 1, 0, max_batch=B)
    ctx.set_threshold(thr)
    ctx.keep_binary_maps(True)
    ctx.set_pipelined(True)
    fr_d, bufs, cap = _async_buffers(frames)
    for b in range(3):
        _batch_and_check_maps(ctx, orc, fr_d, bufs, cap, frames, thr, b)
    ctx.sync()
    ctx.set_pipelined(False)
    # What the asynchronous batches 1 and 2 left on the device (set 1, set 0) is the independent figure.  The synchronous call for batch 1
    # runs in set 1 while set 0 still holds batch 2's larger total, the one for batch 2 runs in set 0 while set 1 holds batch 1's smaller
    # one: a status word from the other set copies too much (the sentinel behind the records is overwritten) or too little.
    want = {b: bufs[b & 1][0][:int(bufs[b & 1][1][B])].cpu().numpy() for b in (1, 2)}
    totals = {}
    assert want[1].size > 0 and want[2].size > 1.3 * want[1].size
    for b in (1, 2):
        out = np.full(cap, 0xA5, np.uint8)
        out, rec, md = ctx.reduce_compress_batch(frames[b * B:(b + 1) * B], first_frame_id=b * B, out=out)
        totals[b] = int(rec[B])
        assert totals[b] == want[b].size and np.array_equal(out[:totals[b]], want[b]) and (out[totals[b]:] == 0xA5).all(), "batch %d" % b
        for i in range(B):
            assert np.array_equal(ctx.binary_map(i), orc.pack_binary_frame(frames[b * B + i] > thr))
    ctx.close()
    # the streaming form: slot k's batch runs in set k & 1, and its total is the status word of that batch
    ctx = hip.ReduceContext(NX, NY, 12, 1, 1, 2, 1, 0, max_batch=B)
    ctx.set_threshold(thr)
    order = (2, 1, 2)                       # batches by slot: sets 0, 1, 0
    for slot, b in enumerate(order):
        ctx.pipe_submit(slot, frames[b * B:(b + 1) * B], B, b * B)
    for slot, b in enumerate(order):
        rec, md, total = ctx.pipe_result(slot, B)
        assert total == totals[b] and int(rec[B]) == totals[b], "slot %d" % slot
        ctx.pipe_fetch_wait(slot)
    ctx.sync()
    ctx.close()


@pytest.mark.parametrize("n_before", [1, 2])
def test_level2_second_chain_switch_keeps_the_most_recent_set(hip, orc, stacks, n_before):
    """Level 2: the first rc_ctx_set_pipelined(1) gives scratch set 1 a workspace of its own (l2_second_chain).  Made after an odd and
    after an even number of batches - the most recent batch then lies in set 0 and in set 1 -, the maps before and after the switch are the
    ones of the batch enqueued last."""
    dark, frames = stacks[2]
    thr = orc.threshold(dark, 0)
    ctx = hip.ReduceContext(NX, NY, 12, 2, 1, 2, 1, 0, max_batch=B)
    ctx.set_threshold(thr)
    fr_d, bufs, cap = _async_buffers(frames)
    for b in range(n_before):
        _batch_and_check_maps(ctx, orc, fr_d, bufs, cap, frames, thr, b)
    ctx.set_pipelined(True)
    last = n_before - 1
    for i in range(B):
        assert np.array_equal(ctx.binary_map(i), orc.pack_binary_frame(frames[last * B + i] > thr)), "after the switch, frame %d" % i
    for b in range(n_before, 3):
        _batch_and_check_maps(ctx, orc, fr_d, bufs, cap, frames, thr, b)
    ctx.sync()
    ctx.close()


# ---- seams 2 and 3 ---------------------------------------------------------------------------------------------------------
def _check_stock_lz4(comp, data):
    """stock liblz4, where the machine has it, expands the frame to the input (the judge test_gpu_parity.py uses)"""
    if ctypes.util.find_library("lz4"):
        from test_gpu_parity import _lz4_system_decode
        assert _lz4_system_decode(comp, len(data)) == data


def _payloads():
    rng = np.random.default_rng(513)
    return [b"", b"\x5a", np.packbits(rng.random(513 * 8) < 0.05, bitorder="little").tobytes(),   # 513: two tiles of 512 bytes, the second partial
            np.packbits(rng.random(4096 * 8) < 0.02, bitorder="little").tobytes()]


class _Mem:
    """A byte buffer in host (numpy) or device (torch) memory with one way to fill, address and read it."""

    def __init__(self, device, nbytes, data=b""):
        import torch
        self.device = device
        host = np.zeros(max(nbytes, 16), np.uint8)
        host[:len(data)] = np.frombuffer(data, np.uint8)
        self.a = torch.from_numpy(host).to("cuda:0") if device else host

    def ptr(self):
        return self.a.data_ptr() if self.device else self.a.ctypes.data

    def bytes(self, n):
        return (self.a[:n].cpu().numpy() if self.device else self.a[:n]).tobytes()


UNTOUCHED = 0xABCDEF0123   # *out_n as the caller left it


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("scheme,level", [(2, 0), (2, 1), (1, 1), (8, 1)], ids=["lz4-runs", "lz4-events", "zstd", "blosc"])
def test_seam2_round_trips_at_the_skeletons_edges(hip, orc, scheme, level, device):
    """rc_compress / rc_decompress on an empty buffer, one byte, two tiles with a partial second one and 4 096 sparse bytes, source and
    destination both in host or both in device memory.  One byte short: RC_ERR_OUT_TOO_SMALL, and *out_n as the library before the
    shared skeleton left it - rc_compress does not touch it, rc_decompress has stored the decoded size."""
    from pyrecode_amd.recode_compressors import _zstd_host_decompress
    L = hip.lib()
    for data in _payloads():
        n = len(data)
        bound = L.rc_compress_bound(scheme, n) + 16
        src, dst = _Mem(device, n, data), _Mem(device, bound)
        out_n = C.c_uint64(UNTOUCHED)
        hip.check(L.rc_compress(scheme, level, src.ptr(), n, dst.ptr(), bound, C.byref(out_n)), "rc_compress")
        cn = out_n.value
        comp = dst.bytes(cn)
        if scheme == 2:
            assert orc.lz4f_decode(comp, n + 64) == data
            _check_stock_lz4(comp, data)
        elif scheme == 1:
            assert _zstd_host_decompress(comp) == data
        else:
            assert orc.blosc1_decode(comp) == data
        out_n = C.c_uint64(UNTOUCHED)
        assert L.rc_compress(scheme, level, src.ptr(), n, dst.ptr(), cn - 1, C.byref(out_n)) == hip.RC_ERR_OUT_TOO_SMALL
        assert out_n.value == UNTOUCHED
        csrc, back = _Mem(device, cn, comp), _Mem(device, n + 16)
        out_n = C.c_uint64(UNTOUCHED)
        hip.check(L.rc_decompress(scheme, csrc.ptr(), cn, back.ptr(), n, C.byref(out_n)), "rc_decompress")
        assert out_n.value == n and back.bytes(n) == data
        if n:
            out_n = C.c_uint64(UNTOUCHED)
            assert L.rc_decompress(scheme, csrc.ptr(), cn, back.ptr(), n - 1, C.byref(out_n)) == hip.RC_ERR_OUT_TOO_SMALL
            assert out_n.value == n


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_seam3_pack_unpack_and_sparse_expand(hip, orc, device):
    """rc_bit_pack, rc_bit_unpack and rc_unpack_frame_sparse with 100 values at depth 12, host and device pointers."""
    L = hip.lib()
    rng = np.random.default_rng(12)
    d, nv, nx, ny = 12, 100, 40, 30
    vals = rng.integers(0, 1 << d, nv).astype(np.uint16)
    packed = orc.bit_pack(vals, d)
    assert packed.size == 150
    src, dst = _Mem(device, 2 * nv, vals.tobytes()), _Mem(device, packed.size)
    hip.check(L.rc_bit_pack(src.ptr(), nv, d, dst.ptr(), packed.size), "rc_bit_pack")
    assert dst.bytes(packed.size) == packed.tobytes()
    back = _Mem(device, 8 * nv)
    hip.check(L.rc_bit_unpack(dst.ptr(), packed.size, nv, d, back.ptr()), "rc_bit_unpack")
    assert np.array_equal(np.frombuffer(back.bytes(8 * nv), np.uint64), vals.astype(np.uint64))
    binary = np.zeros(nx * ny, bool)
    binary[rng.choice(nx * ny, nv, replace=False)] = True
    bitmap = orc.pack_binary_frame(binary)
    want = orc.unpack_frame_sparse(nx, ny, d, bitmap, packed)
    bm, px, trip = _Mem(device, bitmap.size, bitmap.tobytes()), _Mem(device, packed.size, packed.tobytes()), _Mem(device, 24 * nv)
    assert L.rc_unpack_frame_sparse(nx, ny, d, bm.ptr(), px.ptr(), packed.size, None, 0, 1) == nv        # the counting call
    assert L.rc_unpack_frame_sparse(nx, ny, d, bm.ptr(), px.ptr(), packed.size, trip.ptr(), nv, 1) == nv
    assert np.array_equal(np.frombuffer(trip.bytes(24 * nv), np.uint64).reshape(nv, 3), want)
    assert L.rc_unpack_frame_sparse(nx, ny, d, bm.ptr(), px.ptr(), packed.size, trip.ptr(), nv - 1, 1) == hip.RC_ERR_OUT_TOO_SMALL
