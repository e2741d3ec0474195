"""The candidate / chain scheme of the batched device inflate, on the CPU: the serial model (tests/inflate_chain_model.py) and the C++
decoding core the kernels are built from (pyrecode_amd/csrc/rc_inflate.h through tests/native/inflate_chain_check.cpp) must both
give zlib.decompress's bytes, with the right number of units, for every stream of the catalogue - and refuse every stream of the refused
catalogue.  The core also runs as a stand-alone program under AddressSanitizer / UBSan on damaged and random input."""
import ctypes as C
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import inflate_chain_model as icm

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "native", "inflate_chain_check.cpp")

FRAMES = icm.catalogue()
REFUSED = icm.refused_catalogue(FRAMES)


def _streams(f):
    return ((icm.MAP, f["map_stream"], f["bitmap"]), (icm.VALUES, f["val_stream"], f["values"]))


@pytest.fixture(scope="module")
def native(tmp_path_factory):
    so = tmp_path_factory.mktemp("infchk") / "libinflate_chain_check.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", str(so), SRC])
    L = C.CDLL(str(so))
    L.inflate_chain_check.restype = C.c_int
    L.inflate_chain_check.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]

    def run(stream, size, kind, misalign=0):
        out = np.zeros(size + 1, np.uint8)
        units, ncand = C.c_uint32(0), C.c_uint32(0)
        st = L.inflate_chain_check(bytes(stream), len(stream), size, kind, misalign, out.ctypes.data, C.byref(units), C.byref(ncand))
        return st, out[:size].tobytes(), units.value, ncand.value
    return run


def test_catalogue_covers_the_cases():
    by = {f["name"]: f for f in FRAMES}
    assert len(by["one_tile"]["bitmap"]) == 512 and len(by["short_last_tile"]["bitmap"]) == 520 and len(by["smaller_than_a_tile"]["bitmap"]) == 2
    s = by["stored_then_coded"]["map_stream"]
    assert s[2] == 0 and (s[2 + 5 + 512] & 7) == 3                      # a stored tile, then the last, coded one
    assert by["no_set_pixel"]["values"] == b"" and by["no_set_pixel"]["val_stream"] == b"\x78\x01\x01\x00\x00\xff\xff\x00\x00\x00\x01"
    assert len(by["values_32768_coded"]["values"]) == 32768 and len(by["values_32769_stored"]["values"]) == 32769
    # coded / stored / coded
    s, ends, p = by["values_coded_stored_coded"]["val_stream"], [], 2
    kinds = []
    while p != len(s) - 4:
        kinds.append((s[p] >> 1) & 3)
        p = icm.decode_candidate(s, p, icm.VALUES)[0]
    assert kinds == [2, 0, 2]
    # the marker inside a stored tile: at a 4-aligned stream offset and at others, and false candidates that decode as complete blocks
    s = by["marker_in_stored_tile"]["map_stream"]
    false = [p for p in icm.candidates(s, icm.MAP) if s[p - 4:p] == icm.MARKER and p not in _chain(s, icm.MAP)]
    assert len(false) >= 4 and len({p % 4 for p in false}) >= 2
    assert sum(icm.decode_candidate(s, p, icm.MAP) is not None for p in false) >= 2
    s = by["marker_in_stored_chunk"]["val_stream"]
    assert len([p for p in icm.candidates(s, icm.VALUES) if p not in _chain(s, icm.VALUES)]) >= 3


def _chain(s, kind):
    out, p = [], 2
    while p != len(s) - 4:
        out.append(p)
        p = icm.decode_candidate(s, p, kind)[0]
    return out


@pytest.mark.parametrize("frame", FRAMES, ids=lambda f: f["name"])
def test_model_inflates_own_streams(frame):
    for kind, stream, raw in _streams(frame):
        assert zlib.decompress(stream) == raw
        got, units, ncand = icm.inflate(stream, len(raw), kind)
        assert got == raw
        assert units == max(-(-len(raw) // icm.UNIT[kind]), 1) and ncand >= units


@pytest.mark.parametrize("frame", FRAMES, ids=lambda f: f["name"])
def test_core_inflates_own_streams(native, frame):
    for kind, stream, raw in _streams(frame):
        _, units, ncand = icm.inflate(stream, len(raw), kind)
        for mis in range(4):
            st, got, u, c = native(stream, len(raw), kind, mis)
            assert st == 0 and got == raw and (u, c) == (units, ncand)


@pytest.mark.parametrize("frame", REFUSED, ids=lambda f: f["name"])
def test_foreign_and_damaged_streams_are_refused(native, frame):
    refused = 0
    for kind, stream, raw in _streams(frame):
        try:
            got, _, _ = icm.inflate(stream, len(raw), kind)
            assert got == raw               # (the stream this variant left alone)
            assert native(stream, len(raw), kind)[0] == 0
        except icm.Refused:
            refused += 1
            assert native(stream, len(raw), kind)[0] == -2
    assert refused == 1


def test_core_under_sanitizers_on_damaged_input(tmp_path):
    """the stand-alone program: every catalogue stream, 48 damaged copies of each and 400 random inputs through the C++ core built with
    -fsanitize=address,undefined; a read outside the stream's dwords or a write outside a unit ends it"""
    exe = tmp_path / "inflate_chain_check"
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    probe = subprocess.run(["g++", "-x", "c++", "-", "-o", str(tmp_path / "probe")] + flags, input=b"int main(){return 0;}", capture_output=True)
    if probe.returncode != 0:
        flags = []                          # (a toolchain without the sanitizer runtimes: the program still runs, vector::at still checks)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-DINFLATE_CHECK_MAIN", "-o", str(exe), SRC] + flags)
    rec = tmp_path / "records.bin"
    with open(rec, "wb") as f:
        for fr in FRAMES:
            for kind, stream, raw in _streams(fr):
                f.write(struct.pack("<III", kind, len(stream), len(raw)) + stream)
    r = subprocess.run([str(exe), str(rec)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("records %d ok" % (2 * len(FRAMES)))
