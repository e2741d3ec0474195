"""The host layer of the uint32-valued COO output (no GPU): the two calls' signatures and _BatchOut's 12-byte layout."""
import numpy as np
import pytest


def test_signatures_hold_the_coo32_pair_with_the_coo_pairs_arguments():
    from pyrecode_amd import _lib
    S = _lib.SIGNATURES
    assert S["rc_expand_frames_coo32"] == S["rc_expand_frames_coo"]
    assert S["rc_expand_frames_coo32_submit"] == S["rc_expand_frames_coo_submit"]
    assert len(S["rc_expand_frames_coo32"][1]) == 12 and len(S["rc_expand_frames_coo32_submit"][1]) == 12


class _Calls:
    """stands in for the loaded library: fn() only picks an attribute"""
    def __getattr__(self, name):
        return name


@pytest.mark.parametrize("value_bytes,vt", [(2, np.uint16), (4, np.uint32)])
def test_batch_out_lays_out_three_arrays_of_the_value_width(value_bytes, vt):
    from pyrecode_amd.reader_batched import _BatchOut
    cap, total = 11, 7
    dst = _BatchOut(True, None, value_bytes).room(cap)
    assert dst.esz == 8 + value_bytes and dst.buf.nbytes == cap * dst.esz and dst.cap == cap
    dst.buf[:] = 0xEE
    dst.buf[:4 * cap].view(np.int32)[:] = np.arange(cap)
    dst.buf[4 * cap:8 * cap].view(np.int32)[:] = 100 + np.arange(cap)
    vals = (np.arange(cap, dtype=np.uint64) * 0x11111111 + 0xF0000001) & (0xFFFFFFFF if value_bytes == 4 else 0xFFFF)
    dst.buf[8 * cap:].view(vt)[:] = vals.astype(vt)
    rows, cols, v = dst.result(total)
    assert (rows.dtype, cols.dtype, v.dtype) == (np.int32, np.int32, np.dtype(vt))
    assert len(rows) == len(cols) == len(v) == total
    base = dst.buf.ctypes.data
    assert (rows.ctypes.data - base, cols.ctypes.data - base, v.ctypes.data - base) == (0, 4 * cap, 8 * cap)
    assert np.array_equal(rows, np.arange(total)) and np.array_equal(cols, 100 + np.arange(total)) and np.array_equal(v, vals[:total].astype(vt))
    suffix = {2: "_coo", 4: "_coo32"}[value_bytes]
    assert dst.fn(_Calls()) == "rc_expand_frames" + suffix and dst.fn(_Calls(), submit=True) == "rc_expand_frames" + suffix + "_submit"
    trip = _BatchOut(False).room(cap)
    assert trip.esz == 24 and trip.fn(_Calls()) == "rc_expand_frames" and trip.fn(_Calls(), submit=True) == "rc_expand_frames_submit"
    assert trip.result(total).shape == (total, 3) and trip.result(total).dtype == np.uint64


def test_batch_out_width_follows_the_file():
    from pyrecode_amd.reader_batched import _BatchOut
    widths = {(level, d): _BatchOut.for_file({"reduction_level": level, "target_bit_depth": d}, True).value_bytes
              for level in (1, 3) for d in (12, 16, 17, 32)}
    assert widths == {(1, 12): 2, (1, 16): 2, (1, 17): 4, (1, 32): 4, (3, 12): 2, (3, 16): 2, (3, 17): 2, (3, 32): 2}
    with pytest.raises(ValueError):
        _BatchOut(True, None, 8)


def test_from_triplets_keeps_a_full_uint32_value():
    from pyrecode_amd.reader_batched import _BatchOut
    trip = np.array([[3, 5, 0xFFFFFFFF], [4, 0, 0x10000], [69, 299, 1]], np.uint64)
    rows, cols, vals = _BatchOut.from_triplets(trip, True, 4)
    assert (rows.dtype, cols.dtype, vals.dtype) == (np.int32, np.int32, np.uint32)
    assert rows.tolist() == [3, 4, 69] and cols.tolist() == [5, 0, 299] and vals.tolist() == [0xFFFFFFFF, 0x10000, 1]
    assert _BatchOut.from_triplets(trip, True, 2)[2].dtype == np.uint16
    assert _BatchOut.from_triplets(trip, False) is trip
