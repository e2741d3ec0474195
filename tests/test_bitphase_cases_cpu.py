"""The bit-phase case builders (tests/bitphase_cases.py) and the oracle on full-range data, without a GPU: the census finds every case
the tile-chain matrix of tests/test_gpu_bit_phases.py is meant to reach, the full-range generator reaches every bit, and the oracle's
packing agrees with a plain np.unpackbits restatement where the residuals use all d bits (a full-range oracle mistake would otherwise
make the GPU tests pass on wrong bytes)."""
import struct

import numpy as np
import pytest

import bitphase_cases as bc


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    oracle.lib()
    return oracle


@pytest.mark.parametrize("dt,d,tpi", bc.chain_matrix(), ids=lambda v: str(v))
def test_census_finds_every_case_of_the_tile_chain_matrix(dt, d, tpi):
    B, nt = bc.TPI_GEOMETRY[tpi]
    assert bc.gather_tpi(B, nt) == tpi
    assert nt % tpi != 0                                 # (e): the last item is partial
    cs = bc.tile_chain_frames(d, nt, dt, B=min(B, 2), tpi=tpi, seed=3)
    want = bc.census_cases_expected(d)
    assert {"b", "c", "e"} <= want and (d > 8 or {"d"} <= want) and (d < 8 or not {"a", "d"} & want)
    for z in range(len(cs["idx"])):
        counts, p, v = cs["counts"][z], cs["idx"][z], cs["vals"][z]
        assert np.array_equal(np.bincount(p // bc.TILE, minlength=nt), counts)
        census = bc.chain_census(counts, d, tpi)
        found = {k for k in "abcdefg" if census[k]}
        assert want <= found, "frame %d: missing %s" % (z, sorted(want - found))
        assert census["empty_items"] >= 2                  # one (c) chain crosses two or more entirely empty items
        packed = bc.np_bit_pack(v, d)
        coff = np.concatenate([[0], np.cumsum(counts)])
        for case in "abceg":
            for t, b, avail in census[case]:
                own = int(packed[b]) & ((1 << avail) - 1)
                assert own != 0, "case %s tile %d: the shared byte's own bits are zero" % (case, t)
                assert (int(coff[t + 1]) * d) // 8 == b
        # the events sit on their tiles' first and last pixels
        for t in np.flatnonzero(counts >= 2):
            lo, hi = t * bc.TILE, min((t + 1) * bc.TILE, cs["N"])
            assert lo in set(p[(p >= lo) & (p < hi)]) and hi - 1 in set(p[(p >= lo) & (p < hi)])


def test_gather_tpi_restates_launch_gather():
    assert bc.gather_tpi(9, 16) == 8                       # nine 512 x 512 frames: eight tiles an item (rc_gather.hip's comment)
    assert bc.gather_tpi(64, 4096) == 64
    assert bc.gather_tpi(16, 63 * 64 + 32) == 64 and bc.gather_tpi(16, 63 * 64) == 32
    assert bc.gather_tpi(1, 1) == 8


@pytest.mark.parametrize("dtype,d,eps", [(np.uint8, 1, 3), (np.uint8, 7, 9), (np.uint8, 8, 1), (np.uint16, 9, 5), (np.uint16, 13, 2),
                                         (np.uint16, 16, 7), (np.uint32, 17, 11), (np.uint32, 25, 4), (np.uint32, 31, 1), (np.uint32, 32, 2)])
def test_full_range_frames_reach_every_bit_and_wrap(dtype, d, eps):
    dark, frames = bc.full_range_frames(7 + d, 3, 90, 110, 0.2, d, dtype, eps)
    M = int(np.iinfo(dtype).max)
    thr = bc.np_threshold(dark, eps, dtype)
    assert (dark.astype(np.int64) + eps > M).any()                       # wrapped thresholds
    assert (dark == M).any()
    ev = frames > thr
    r = (frames.astype(np.int64) - thr.astype(np.int64))[ev]
    assert r.min() >= 1 and r.max() <= (1 << d) - 1
    for b in range(d):
        assert ((r >> b) & 1).any(), "bit %d never set" % b
    assert (r == (1 << d) - 1).any() and (r == 1 << (d - 1)).any()
    if d < np.iinfo(dtype).bits:   # (at the dtype's full width most thresholds leave less room than 2^d - 1)
        assert (r == (1 << d) - 1).sum() > 0.01 * r.size and (r == 1 << (d - 1)).sum() > 0.01 * r.size
    _, over = bc.full_range_frames(7 + d, 3, 90, 110, 0.2, d, dtype, eps, overflow=True)
    rv = (over.astype(np.int64) - thr.astype(np.int64))[over > thr]
    if d < np.iinfo(dtype).bits:
        assert (rv > (1 << d) - 1).any()                                  # bits at and above d: dropped by the packer
    assert (over == M).any()


def _np_l1_mode0(frame, thr, d, fid):
    binary = frame > thr
    pix = (frame.astype(np.int64) - thr.astype(np.int64))[binary]
    bitmap = np.packbits(binary.reshape(-1), bitorder="little").tobytes()
    if d % 8 == 0 and frame.dtype == np.uint32:
        packed = pix.astype("<u4").tobytes()                             # (recode_writer.py:463-464: .tobytes() when d % 8 == 0)
    else:
        packed = bc.np_bit_pack(pix.astype(np.uint64), d).tobytes()
    return struct.pack("<II", fid, len(packed)) + bitmap + packed


@pytest.mark.parametrize("dtype,depths", [(np.uint8, range(1, 9)), (np.uint16, range(1, 17)), (np.uint32, range(17, 33))])
def test_oracle_agrees_with_plain_numpy_on_full_range_frames(orc, dtype, depths):
    ny, nx = 37, 61
    for d in depths:
        for overflow in (False, True):
            eps = 1 + d % 5
            dark, frames = bc.full_range_frames(100 + d, 2, ny, nx, 0.3, d, dtype, eps, overflow)
            thr = orc.threshold32(dark, eps) if dtype == np.uint32 else orc.threshold(dark, eps)
            assert np.array_equal(np.asarray(thr).astype(np.int64), bc.np_threshold(dark, eps, dtype).astype(np.int64)), d
            for z in range(2):
                tag = "%s d %d overflow %s frame %d" % (np.dtype(dtype).name, d, overflow, z)
                want = _np_l1_mode0(frames[z], thr, d, z)
                rec = (orc.l1_record32 if dtype == np.uint32 else orc.l1_record)(frames[z], thr, d, z, mode=0)[0]
                assert rec == want, tag
                binary = frames[z] > thr
                vals = (frames[z].astype(np.int64) - np.asarray(thr).astype(np.int64))[binary].astype(np.uint64) & ((1 << d) - 1)
                if dtype == np.uint32:
                    packed = orc.bit_pack32(vals.astype(np.uint32), d)
                    if d % 8:
                        assert np.array_equal(packed, bc.np_bit_pack(vals, d)), tag
                else:
                    packed = orc.bit_pack(vals.astype(np.uint16), d)
                    assert np.array_equal(packed, bc.np_bit_pack(vals, d)), tag
                    assert np.array_equal(orc.bit_unpack(packed, vals.size, d), vals), tag
                if dtype == np.uint32 and d % 8 == 0 and d != 32:
                    continue   # (four bytes a value at d = 24: the reference writes what its own reader would not read as 24-bit fields)
                assert np.array_equal(bc.np_bit_unpack(packed, vals.size, d), vals), tag
                bitmap = np.packbits(binary.reshape(-1), bitorder="little")
                trip = orc.unpack_frame_sparse(nx, ny, d, bitmap, packed)
                rows, cols = np.nonzero(binary)
                assert np.array_equal(trip, np.stack([rows, cols, vals]).T.astype(np.uint64)), tag


@pytest.mark.parametrize("d", [1, 3, 5, 7, 9, 12, 15, 16])
def test_oracle_packs_tile_chain_frames_like_plain_numpy(orc, d):
    cs = bc.tile_chain_frames(d, 75, np.uint16, B=2, tpi=8, seed=5)
    frames = bc.chain_host_frames(cs)
    thr = cs["dark"].reshape(cs["ny"], cs["nx"])
    for z in range(2):
        rec = orc.l1_record(frames[z], thr, d, z, mode=0)[0]
        bitmap = np.zeros(cs["N"], bool)
        bitmap[cs["idx"][z]] = True
        want = bc.np_bit_pack(cs["vals"][z], d).tobytes()
        assert rec == struct.pack("<II", z, len(want)) + np.packbits(bitmap, bitorder="little").tobytes() + want
