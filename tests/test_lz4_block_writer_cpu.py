"""tests/lz4_block_writer.py judged before any device code sees its blocks: stock liblz4 (LZ4_decompress_safe, LZ4F_decompress) and the
oracle's from-spec decoders must expand every catalogue block, frame and binary-map stream to the writer's own serial replay, and the
catalogue must reach every feature the device decoders' tests rely on.  liblz4 is the judge: without it these tests fail, they do not skip."""
import ctypes as C

import pytest

import lz4_block_writer as lzw
from test_gpu_parity import _lz4_system_decode


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    oracle.lib()
    return oracle


def _safe(blk, cap):
    """LZ4_decompress_safe -> bytes, or None where liblz4 refuses the block"""
    dst = C.create_string_buffer(cap + 1)
    k = lzw.liblz4().LZ4_decompress_safe(bytes(blk), dst, len(blk), cap)
    return None if k < 0 else dst.raw[:k]


def test_catalogue_reaches_every_feature():
    """The union of the cases' features - each worked out from the case's own sequence list - is the full list: a case that goes, or a
    length that shifts, shows here."""
    assert lzw.coverage(lzw.CASES) == set(lzw.FEATURES)
    assert len(set(lzw.FEATURES)) == len(lzw.FEATURES)
    assert {c.size for c in lzw.CASES} == set(lzw.SIZES)
    # (cases whose features others share too are pinned by name: taking one out must not go unnoticed either)
    assert len(lzw.CASES) == 29 and len(lzw.tiles(512)) == 18
    assert {"grid6", "off1_after_literal", "zero_sources", "straddle", "zeros", "chain_near", "chain_far", "literals_512"} <= set(lzw.BY_NAME)
    for needed in ("lit:0", "lit:15", "lit:270", "ml:19", "ml:274", "off:op:eq", "off:2:gt64", "off:65:lt", "chain:near-then-off1:zero",
                   "chain:far-then-off1:nonzero", "src:allzero", "src:straddle-unaligned", "literals-only:512", "size:438"):
        assert needed in lzw.FEATURES
    by = lzw.BY_NAME
    assert len(by["literals_512"].block) == 515 and by["literals_512"].block[:3] == b"\xf0\xff\xf2"          # 15 + 255 + 242
    assert lzw.encode([(b"a" * 15, 1, 19)], b"") == b"\xff\x00" + b"a" * 15 + b"\x01\x00\x00" + b"\x00"       # 15 + 0 both ways
    assert lzw.encode([(b"a" * 270, 1, 274)], b"") == b"\xff\xff\x00" + b"a" * 270 + b"\x01\x00\xff\x00" + b"\x00"   # 15 + 255 + 0 both ways


@pytest.mark.parametrize("case", lzw.CASES, ids=lambda c: c.name)
def test_stock_liblz4_and_the_oracle_decode_every_block(orc, case):
    assert len(case.decoded) == case.size and lzw.conforms(case.seqs, case.tail)
    assert lzw.replay(case.seqs, case.tail) == case.decoded
    assert _safe(case.block, case.size) == case.decoded
    assert _safe(case.block, case.size - 1) is None                       # (not one byte less)
    assert orc.lz4_block_decode(case.block, case.size) == case.decoded
    f = lzw.frame([case.block])
    assert orc.lz4f_decode(f, case.size + 8) == case.decoded
    assert _lz4_system_decode(f, case.size) == case.decoded


def test_stock_liblz4_and_the_oracle_decode_the_frames(orc):
    """the mixed frame (stored blocks between the catalogue's) and the linked frames: LZ4F_decompress checks the header checksum, so this
    also pins the two descriptor constants"""
    f, want = lzw.mixed_frame()
    assert f[4:7] == b"\x60\x40\x82"
    assert orc.lz4f_decode(f, len(want) + 8) == want
    assert _lz4_system_decode(f, len(want)) == want
    frames = lzw.linked_frames()
    assert len(frames) == 4
    for name, f, want in frames:
        assert f[4:7] == b"\x40\x40\xc0" and len(want) == 128 * 1024, name
        assert orc.lz4f_decode(f, len(want) + 8) == want, name
        assert _lz4_system_decode(f, len(want)) == want, name
        seqs, _ = lzw.parse(f[7 + 4 + (int.from_bytes(f[7:11], "little") & 0x7FFFFFFF) + 4:-4])
        assert seqs[0][0] == b"" and seqs[0][1] in (1, 65535), name       # the second block opens with a match into the first


def test_binary_map_frames_decode_to_their_maps(orc):
    assert [c[0] for c in lzw.map_frame_cases()] == list(lzw.MAP_FRAME_LABELS)
    for label, nx, ny, frames in lzw.map_frame_cases():
        for f, data in frames:
            assert len(data) * 8 == nx * ny, label
            assert orc.lz4f_decode(f, len(data) + 8) == data, label
            assert _lz4_system_decode(f, len(data)) == data, label
    for layout in ("uniform", "split-first"):
        f, data, offs = lzw.big_map_frame(layout)
        assert len(data) == 512 * 1024 // 8 and len(offs) == 128 + (layout != "uniform")
        assert orc.lz4f_decode(f, len(data) + 8) == data
        assert _lz4_system_decode(f, len(data)) == data


def test_defects_are_refused_by_liblz4_and_the_oracle(orc):
    """each malformed block fails for the reason its name gives: the oracle's decoder reports that very check, and liblz4 refuses it too -
    but for offset 0, which lz4_Block_format.md calls invalid and LZ4_decompress_safe (1.9.x) lets through"""
    codes = {"offset0": -13, "offset_past_start": -13, "match_past_end": -15, "literals_past_end": -11, "length_cut": -10}
    for size in (512, 64):
        d = lzw.defects(size)
        assert set(d) == set(codes)
        for name, blk in d.items():
            if name != "offset0":
                assert _safe(blk, size) is None, name
            with pytest.raises(ValueError, match=r"code %d\b" % codes[name]):
                orc.lz4_block_decode(blk, size)
            assert len(blk) != size and len(blk) <= size + size // 255 + 16      # (a blosc chunk may carry it as an LZ4 block)
