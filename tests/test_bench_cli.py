"""CPU: bench.py's options (a plain run by default, --full, --dump-outputs) and the dump writer on host tensors - what a record dump
holds, its dtypes, its seeded sample and its size bound."""
import importlib.util
import os

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(REPO, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_plain_run_is_the_default_and_full_is_an_option(bench):
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "3"])
    assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 3
    a = bench.parse(["--full", "--dump-outputs", "out_dir"])
    assert a.full is True and a.dump_outputs == "out_dir"


def test_dump_outputs_is_refused_with_read(bench):
    with pytest.raises(SystemExit):
        bench.parse(["--read", "--dump-outputs", "out_dir"])


def _records(rng, sizes):
    import torch
    rec = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    out = rng.integers(0, 256, int(rec[-1]) + 4096, dtype=np.uint8)        # (a tail of capacity the records do not use)
    md = rng.integers(0, 1 << 32, (len(sizes), 3), dtype=np.uint64).astype(np.uint32)
    return torch.from_numpy(out), torch.from_numpy(rec), torch.from_numpy(md.view(np.int32)), out, rec, md


def _load(d):
    got = {f[:-4]: np.load(os.path.join(d, f), allow_pickle=False) for f in sorted(os.listdir(d))}
    assert sorted(got) == ["record_metadata", "record_offsets", "record_sample_bytes", "record_sample_index"]
    assert all(v.dtype in (np.float32, np.float64) for v in got.values())
    return got


def test_dump_outputs_writes_offsets_metadata_and_whole_sampled_records(bench, tmp_path):
    rng = np.random.default_rng(3)
    sizes = rng.integers(16, 5000, 64)
    out_t, rec_t, md_t, out, rec, md = _records(rng, sizes)
    bench.dump_outputs(str(tmp_path / "a"), out_t, rec_t, md_t)
    got = _load(str(tmp_path / "a"))
    assert np.array_equal(got["record_offsets"], rec.astype(np.float64))
    assert np.array_equal(got["record_metadata"], md.astype(np.float64))
    pick = got["record_sample_index"].astype(np.int64)
    assert pick.size == bench.DUMP_RECORDS and np.all(np.diff(pick) > 0) and pick[-1] < 64
    want = np.concatenate([out[rec[z]:rec[z + 1]] for z in pick]).astype(np.float32)
    assert np.array_equal(got["record_sample_bytes"], want)
    bench.dump_outputs(str(tmp_path / "b"), out_t, rec_t, md_t)              # same records: same files (the sample is seeded)
    again = _load(str(tmp_path / "b"))
    assert all(np.array_equal(got[k], again[k]) for k in got)


def test_dump_outputs_stays_within_64_mb_for_large_records(bench, tmp_path):
    rng = np.random.default_rng(4)
    sizes = np.full(4, 6 << 20)                                               # fewer records than the sample, each longer than its share
    out_t, rec_t, md_t, out, rec, md = _records(rng, sizes)
    bench.dump_outputs(str(tmp_path), out_t, rec_t, md_t)
    got = _load(str(tmp_path))
    assert np.array_equal(got["record_sample_index"], np.arange(4.0))
    cap = bench.DUMP_RECORD_BYTES // 4
    assert np.array_equal(got["record_sample_bytes"], np.concatenate([out[rec[z]:rec[z] + cap] for z in range(4)]).astype(np.float32))
    assert sum(os.path.getsize(os.path.join(str(tmp_path), f)) for f in os.listdir(str(tmp_path))) <= 64 << 20
