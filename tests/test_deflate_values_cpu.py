"""CPU: the residual stream of the device DEFLATE encoder at compression_level >= 2, as tests/deflate_values_model.py states it.  Stock zlib
must expand every stream the model emits (format conformance, the zero-length distance code included); the model's size is held against
stock zlib-1 on the oracle's packed residuals; the C++ host half (pyrecode_amd/csrc/rc_deflate_model.h) must build the model's table."""
import ctypes as C
import os
import subprocess
import zlib

import numpy as np
import pytest

import deflate_block_model as dbm
import deflate_values_model as m
from conftest import REPO, synth_frames

LENGTHS = (0, 1, 32767, 32768, 32769, 3 * 32768, 3 * 32768 + 5)


def _residual_bytes(seed, n):
    """n bytes that look like uint16 residuals in [1, 2047]"""
    v = np.random.default_rng(seed).integers(1, 2048, (n + 1) // 2).astype("<u2")
    return v.tobytes()[:n]


def _tables():
    sample = _residual_bytes(1, 40000)
    skew = [1 << min(i, 30) for i in range(256)]            # Fibonacci-like growth: the plain pairing gives lengths far above 12
    return {"sample": m.fit_lengths(m.sample_hist(sample)), "zeros": m.fit_lengths([0] * 256), "limit": m.fit_lengths(skew)}


TABLES = _tables()


@pytest.mark.parametrize("name", sorted(TABLES))
def test_tables_are_complete_codes_within_the_limit(name):
    L = TABLES[name]
    assert len(L) == 257 and min(L) >= 1 and max(L) <= m.MAXBITS
    assert sum(1 << (m.MAXBITS - l) for l in L) == 1 << m.MAXBITS
    assert m.header_bits(L)[1] <= 96 * 32
    if name == "limit":
        assert max(L) == m.MAXBITS


@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("name", sorted(TABLES))
def test_zlib_expands_the_model(name, n):
    L = TABLES[name]
    for data in (_residual_bytes(n + 7, n), b"\xff" * n, b"\x07" * n):     # like the sample; unlike it: all 0xFF, one value
        s = m.encode_values(data, L)
        assert zlib.decompress(s) == data
        assert len(s) <= len(dbm.stored_stream(data))
        t = m.parse_table(s)
        assert t is None or t == L
        if t is None:
            assert s == dbm.stored_stream(data)
    assert m.encode_values(_residual_bytes(3, n), L, usable=False) == dbm.stored_stream(_residual_bytes(3, n))


def test_coded_chunks_exist_and_the_empty_stream_is_one_stored_block():
    L = TABLES["sample"]
    data = _residual_bytes(5, 3 * 32768 + 5)
    s = m.encode_values(data, L)
    assert m.parse_table(s) == L and len(s) < 0.9 * len(data)
    assert m.encode_values(b"", L) == b"\x78\x01\x01\x00\x00\xff\xff\x00\x00\x00\x01"


def test_incompressible_stream_is_the_stored_stream():
    data = np.random.default_rng(11).integers(0, 256, 3 * 32768 + 5).astype(np.uint8).tobytes()
    for L in TABLES.values():
        assert m.encode_values(data, L) == dbm.stored_stream(data)
    assert not m.usable(m.sample_hist(data), m.fit_lengths(m.sample_hist(data)))


@pytest.mark.parametrize("d", [16, 14, 12])
def test_size_against_stock_zlib_level_1(d):
    """The acceptance number: the oracle's packed residuals of conftest.synth_frames (>= 128 KiB a stream), table fitted to the first frame;
    the coded stream may be at most 1.02 x stock zlib-1's (a ctx-wide sampled table against zlib's per-block ones) and never above the
    stored stream."""
    from oracle import oracle as orc
    orc.lib()
    ny, nx, s = 512, 1024, 0.2
    dark, frames = synth_frames(300 + d, 3, ny, nx, s, d)
    thr = orc.threshold(dark, 0)
    packed = [orc.bit_pack(orc.binarize_l1(f, thr)[1], d).tobytes() for f in frames]
    assert min(len(p) for p in packed) >= 128 * 1024
    hist = m.sample_hist(packed[0])
    L = m.fit_lengths(hist)
    use = m.usable(hist, L)        # (the ctx's 97 % rule: where the byte-wise code does not pay - d = 12 - the stream stays stored)
    got = ref = 0
    for p in packed:
        s = m.encode_values(p, L, use)
        assert zlib.decompress(s) == p
        assert len(s) <= len(dbm.stored_stream(p))
        got += len(s)
        ref += len(zlib.compress(p, 1))
    print("d = %d: table %s, coded %d B, zlib-1 %d B, ratio %.4f" % (d, "used" if use else "not used (stored)", got, ref, got / ref))
    assert got <= 1.02 * ref


@pytest.fixture(scope="module")
def native(tmp_path_factory):
    so = tmp_path_factory.mktemp("dmchk") / "libdeflate_model_check.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", str(so), os.path.join(REPO, "tests", "native", "deflate_model_check.cpp")])
    L = C.CDLL(str(so))
    L.deflate_model_check.restype = C.c_int
    L.deflate_model_check.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    return L


def _hists():
    rng = np.random.default_rng(2)
    return {"sample": m.sample_hist(_residual_bytes(1, 40000))[:256], "zeros": [0] * 256, "limit": [1 << min(i, 30) for i in range(256)],
            "random": list(np.bincount(rng.integers(0, 256, 100000), minlength=256)), "one": [0] * 7 + [500000] + [0] * 248,
            "packed12": list(np.bincount(np.frombuffer(np.packbits(rng.integers(0, 2, 12 * 30000).astype(np.uint8)).tobytes(), np.uint8), minlength=256))}


@pytest.mark.parametrize("name", sorted(_hists()))
def test_host_half_builds_the_models_table(native, name):
    hist = _hists()[name]
    h = np.asarray(hist, np.uint32)
    ln, code, hdr = np.zeros(257, np.uint8), np.zeros(257, np.uint16), np.zeros(384, np.uint8)
    nbits, use = C.c_uint32(0), C.c_uint32(0)
    assert native.deflate_model_check(h.ctypes.data, ln.ctypes.data, code.ctypes.data, hdr.ctypes.data, hdr.size, C.byref(nbits), C.byref(use)) == 0
    L = m.fit_lengths(hist)
    assert list(ln) == L
    rev = [int(format(c, "0%db" % l)[::-1], 2) | (l << 12) for c, l in zip(m.canonical_codes(L), L)]
    assert [int(c) for c in code] == rev
    hv, hn = m.header_bits(L)
    assert nbits.value == hn
    assert int.from_bytes(hdr.tobytes(), "little") == hv
    assert bool(use.value) == m.usable(m.sample_hist(b"")[:0] + list(hist) + [1], L)
