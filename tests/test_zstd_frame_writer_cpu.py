"""CPU: the from-the-RFC zstd frame writer (tests/zstd_frame_writer.py) against the stock libzstd and against the batched reader's host-side
frame walker (rc_zstd_dec.h::zd_index_frame, under AddressSanitizer / UBSan).

  * every frame the writer makes - inside the device decoder's subset or just outside it - is legal zstd: libzstd decodes it to the plaintext;
  * every in-subset frame is ZD_OK for the walker, with exactly the block entries the writer knows it wrote (none FOREIGN, none CORRUPT);
  * every near-miss frame gets the verdict stated in NEAR_MISS_VERDICTS;
  * a frame with described length tables and Repeat_Mode offsets in its first block with sequences is refused by libzstd, so by the walker;
  * over the committed corpus every alternative the subset admits occurs (CENSUS_MINIMUM)."""
import ctypes as C
import ctypes.util
import os
import struct
import subprocess
from collections import Counter

import numpy as np
import pytest

import zstd_frame_writer as W
from conftest import REPO

ZD_OK, ZD_CORRUPT, ZD_FOREIGN = 0, -1, -2
UNKNOWN = 0xFFFFFFFFFFFFFFFF

# feature -> (walker with the decoded size unknown, as rc_decompress calls it; walker with the size known).  OK: the host cannot see
# the problem - the device's checks (literal length 0; bytes produced != bytes expected) or the caller (rows of 1024 bytes) refuse it.
NEAR_MISS_VERDICTS = {
    "four_stream_literals": (ZD_FOREIGN, ZD_FOREIGN),
    "real_offset": (ZD_FOREIGN, ZD_FOREIGN),
    "literal_length_zero": (ZD_OK, ZD_OK),
    "second_tree": (ZD_FOREIGN, ZD_FOREIGN),
    "second_described_tables": (ZD_FOREIGN, ZD_FOREIGN),
    "rle_length_modes": (ZD_FOREIGN, ZD_FOREIGN),
    "length_modes_differ": (ZD_FOREIGN, ZD_FOREIGN),
    "checksum": (ZD_FOREIGN, ZD_FOREIGN),
    "midframe_short_sequence_block": (ZD_OK, ZD_OK),           # (size known: later blocks with sequences are entered with what is left of
                                                               # the total, so the sum still fits; the device finds 300 bytes where 512 are due)
    "literals_block_above_1024": (ZD_OK, ZD_OK),
    "two_frames": (ZD_FOREIGN, ZD_FOREIGN),
}

# every alternative the issue lists occurs at least this often in the corpus (the corpus is deterministic: a later edit of the writer
# that drops a form fails here)
CENSUS_FEW = 3
CENSUS_MINIMUM = (
    ["header:single", "header:windowed", "fcs:0", "fcs:1", "fcs:2", "fcs:4", "fcs:8"]
    + ["block:raw", "block:raw_maximum", "block:rle", "block:rle_above_1024", "block:rle_maximum", "block:literals_only", "block:sequences",
       "block:short_last_with_sequences", "block:empty_last"]
    + ["lit:raw", "lit:rle", "lit:huffman_with_tree", "lit:huffman_treeless", "lit:huffman_literals_only_above_512",
       "lit:huffman_literals_only_1023"]
    + ["lit_sf:%s:%d" % (t, sf) for t in ("raw", "rle") for sf in (0, 2, 1, 3)]
    + ["tree:direct", "tree:fse", "tree:alphabet_with_gaps", "weights_log:5", "weights_log:6", "huf_assign:by_frequency", "huf_assign:shuffled"]
    + ["huf_log:%d" % k for k in range(1, 12)]
    + ["treeless_distance:%d" % k for k in (1, 2, 3, 4)]
    + ["seq_mode:predefined", "seq_mode:described", "seq_mode:repeat", "repeat_of:described", "repeat_of:predefined"]
    + ["of_mode:rle", "of_mode:rle_with_described", "of_mode:repeat", "of_mode:repeat_with_described", "of_mode:rle_after_repeat",
       "of_mode:repeat_after_rle"]
    + ["ll_log:%d" % k for k in range(5, 10)] + ["ml_log:%d" % k for k in range(5, 10)]
    + ["ncount:lt1", "ncount:zero_run", "ncount:zero_run_long", "ncount:fewer_symbols_than_maximum", "ncount_style:fitted", "ncount_style:flat",
       "ncount_style:random"]
    + ["nseq_bytes:1", "nseq_bytes:2", "nseq:128_or_more", "codes:literal_length_with_extra_bits", "codes:match_length_with_extra_bits",
       "codes:extra_bits_in_first_sequence", "codes:extra_bits_in_last_sequence"]
    + ["match:whole", "match:three", "match:part", "match:left_as_literals"]
)


@pytest.fixture(scope="module")
def libzstd():
    name = ctypes.util.find_library("zstd")
    if not name:
        pytest.skip("no libzstd: the stock decoder is this module's judge")
    z = C.CDLL(name)
    z.ZSTD_decompress.restype = C.c_size_t
    z.ZSTD_decompress.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
    z.ZSTD_isError.argtypes = [C.c_size_t]
    z.ZSTD_getErrorName.restype = C.c_char_p
    z.ZSTD_getErrorName.argtypes = [C.c_size_t]

    def decode(frame, cap):
        dst = C.create_string_buffer(cap + 64)
        r = z.ZSTD_decompress(dst, cap + 64, frame, len(frame))
        if z.ZSTD_isError(r):
            return z.ZSTD_getErrorName(r).decode()
        return dst.raw[:r]
    return decode


@pytest.fixture(scope="module")
def walker(tmp_path_factory):
    d = tmp_path_factory.mktemp("zdsubset")
    exe = d / "zd_index_harness"
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", str(exe),
                           os.path.join(REPO, "tests", "native", "zd_index_harness.cpp")])

    def run(cases):
        """cases: (frame, expect_regen, total) -> [(status, regen, [block rows])]"""
        path = d / "cases.bin"
        with open(path, "wb") as f:
            for frame, expect, total in cases:
                f.write(struct.pack("<IIQ", len(frame), expect, total) + frame)
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
        p = subprocess.run([str(exe), str(path), "blocks"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=600)
        assert p.returncode == 0, (p.returncode, p.stderr.decode()[-3000:], p.stdout.decode()[-300:])
        lines = [tuple(int(v) for v in line.split()) for line in p.stdout.decode().splitlines()]
        out, i = [], 0
        while i < len(lines):
            st, nblk, regen = lines[i]
            rows = lines[i + 1:i + 1 + nblk] if st == ZD_OK else []
            out.append((st, regen, rows))
            i += 1 + len(rows)
        assert len(out) == len(cases)
        return out
    return run


@pytest.fixture(scope="module")
def frames():
    return list(W.corpus())


def expected_rows(census, open_end):
    """the walker's block entries as the writer knows them: type, regen, seq_tables, tree_skip, seq_skip, flex.  With the decoded size
    unknown a block with sequences is entered with 512 bytes, and a frame's last one is marked flexible."""
    rows = []
    blocks = census["blocks"]
    for i, b in enumerate(blocks):
        regen = W.TILE if (open_end and b["seq"]) else b["regen"]
        flex = 1 if (open_end and b["seq"] and i + 1 == len(blocks)) else 0
        rows.append((b["type"], regen, b["tables"], b["tree_skip"], b["seq_skip"], flex))
    return rows


def test_every_written_frame_is_legal_zstd(libzstd, frames):
    assert len(frames) > 200
    for name, data, frame, _ in frames:
        assert libzstd(frame, len(data)) == data, name


def test_plaintexts_cover_the_lengths_and_kinds_asked_for():
    texts = dict(W.corpus_plaintexts())
    lengths = {len(v) for v in texts.values()}
    assert {1, 511, 512, 513}.issubset(lengths) and any(2000 < n < 10000 for n in lengths) and any(n > (1 << 17) for n in lengths)
    for kind in ("bitmap_0_", "bitmap_0.5_", "ones_", "byte7_", "residuals_d9_", "residuals_d12_"):
        assert any(k.startswith(kind) for k in texts), kind


def test_walker_accepts_every_in_subset_frame_with_the_blocks_the_writer_wrote(walker, frames):
    cases = []
    for _, data, frame, _ in frames:
        cases.append((frame, W.TILE, len(data)))
        cases.append((frame, W.TILE, UNKNOWN))
    got = walker(cases)
    refused = []
    for k, (name, data, frame, census) in enumerate(frames):
        for open_end, (st, regen, rows) in ((False, got[2 * k]), (True, got[2 * k + 1])):
            if st != ZD_OK:
                refused.append((name, open_end, st))
                continue
            want = expected_rows(census, open_end)
            assert list(rows) == want, (name, open_end, [(i, r, w) for i, (r, w) in enumerate(zip(rows, want)) if r != w][:3], len(rows), len(want))
            assert regen == sum(r[1] for r in want), (name, open_end)
            if not open_end:
                assert regen == len(data), name
            else:
                assert len(data) <= regen < len(data) + W.TILE, name
    assert not refused, refused            # the share of in-subset frames answered FOREIGN or CORRUPT is zero


def test_walker_accepts_literals_only_frames_as_a_value_stream(walker):
    """expect_regen 0 (a stored value stream: every block announces its own size) takes Raw, RLE and literals-only Compressed blocks"""
    cases, wants = [], []
    for k, (name, data) in enumerate(W.corpus_plaintexts()):
        if len(data) > 10000:
            continue
        frame, census = W.write_frame(data, {"seed": 300 + k, "cut": "literals_only"})
        cases.append((frame, 0, len(data)))
        wants.append((name, len(data), expected_rows(census, False)))
    for (st, regen, rows), (name, n, want) in zip(walker(cases), wants):
        assert st == ZD_OK and regen == n and list(rows) == want, (name, st)


def test_near_miss_frames_are_legal_zstd_and_get_the_stated_verdict(libzstd, walker):
    data = W.near_miss_plaintext()
    assert set(NEAR_MISS_VERDICTS) == set(W.NEAR_MISS_FEATURES)
    cases = []
    for feature in W.NEAR_MISS_FEATURES:
        frame = W.write_near_miss(data, feature)
        assert libzstd(frame, len(data)) == data, feature
        cases.append((frame, W.TILE, UNKNOWN))
        cases.append((frame, W.TILE, len(data)))
    got = walker(cases)
    for k, feature in enumerate(W.NEAR_MISS_FEATURES):
        assert (got[2 * k][0], got[2 * k + 1][0]) == NEAR_MISS_VERDICTS[feature], (feature, got[2 * k][0], got[2 * k + 1][0])
    # the one the host cannot see and whose misreading gives OTHER bytes: its third sequence copies from four bytes back
    k = W.NEAR_MISS_FEATURES.index("literal_length_zero")
    assert got[2 * k][2][0][:2] == (2, W.TILE)
    # a Compressed block above 1024 bytes is announced as such, for the callers to refuse
    k = W.NEAR_MISS_FEATURES.index("literals_block_above_1024")
    assert got[2 * k][2][0][:2] == (2, 1500)


def test_repeat_offsets_without_an_earlier_table_is_refused_like_libzstd_refuses_it(libzstd, walker):
    """Described literal / match length tables with Repeat_Mode offsets in a frame's FIRST block with sequences: there is no offsets
    table to repeat.  libzstd calls the frame corrupt, so the walker must not answer OK - while the same modes byte behind an earlier
    block with sequences is legal and accepted (of_mode:repeat_with_described in the corpus)."""
    data = W.near_miss_plaintext()
    frame = W.write_repeat_offsets_without_table(data)
    verdict = libzstd(frame, len(data))
    assert isinstance(verdict, str), "libzstd accepts the frame"
    for st, _, _ in walker([(frame, W.TILE, UNKNOWN), (frame, W.TILE, len(data))]):
        assert st == ZD_CORRUPT
    legal, census = W.write_frame(data, {"seed": 3, "cut": "tiles", "block": "seq", "seq_mode": ["predefined", "described"], "of_mode": "repeat"})
    assert census["counts"].get("of_mode:repeat_with_described") == 1
    assert libzstd(legal, len(data)) == data
    assert [r[0] for r in walker([(legal, W.TILE, UNKNOWN), (legal, W.TILE, len(data))])] == [ZD_OK, ZD_OK]


def test_census_every_alternative_occurs_in_the_corpus(frames):
    total = Counter()
    for _, _, _, census in frames:
        total.update(census["counts"])
    short = {k: total.get(k, 0) for k in CENSUS_MINIMUM if total.get(k, 0) < CENSUS_FEW}
    assert not short, short


def test_explicit_choices_are_honoured():
    data = dict(W.corpus_plaintexts())["bitmap_0.03_3000"]
    _, census = W.write_frame(data, {"seed": 1, "cut": "tiles", "block": "seq", "lit": "huf", "tree": "direct", "header": "windowed", "fcs": 0})
    c = census["counts"]
    assert c["header:windowed"] == 1 and c["fcs:0"] == 1 and c.get("block:raw", 0) == 0 and c["block:sequences"] == 6
    assert [b["regen"] for b in census["blocks"]] == [512] * 5 + [3000 - 5 * 512]
    again, _ = W.write_frame(data, {"seed": 1, "cut": "tiles", "block": "seq", "lit": "huf", "tree": "direct", "header": "windowed", "fcs": 0})
    assert again == W.write_frame(data, {"seed": 1, "cut": "tiles", "block": "seq", "lit": "huf", "tree": "direct", "header": "windowed", "fcs": 0})[0]
