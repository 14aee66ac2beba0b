"""bench.py --dump-outputs: the dump of one output directory is float32/float64
.npy only, bounded, and identical for identical files (so two builds can be
compared output for output). No GPU; exercises bench.dump_outputs directly."""
import os

import numpy as np

import bench


def test_dump_outputs_sampled_and_repeatable(tmp_path):
    out = tmp_path / "out-0"
    out.mkdir()
    big = np.random.default_rng(3).integers(
        0, 256, 3 * bench.DUMP_SAMPLE_BYTES + 1234, dtype=np.uint8).tobytes()
    (out / "oa-100-big-Data.db").write_bytes(big)
    (out / "oa-100-big-Digest.crc32").write_bytes(b"4077112233")
    res = {k: i + 1 for i, k in enumerate(bench.RESULT_COUNTERS)}
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), str(out), res)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b"))
    assert names == ["counters.npy", "file_sizes.npy",
                     "oa-100-big-Data.db.npy", "oa-100-big-Digest.crc32.npy"]
    for n in names:
        x, y = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert x.dtype in (np.float32, np.float64)
        assert np.array_equal(x, y)
    data = np.load(tmp_path / "a" / "oa-100-big-Data.db.npy")
    # sampled, not whole (the file's short last block may be among the picks)
    assert bench.DUMP_SAMPLE_BYTES - bench.DUMP_SAMPLE_BLOCK < data.size <= bench.DUMP_SAMPLE_BYTES
    digest = np.load(tmp_path / "a" / "oa-100-big-Digest.crc32.npy")
    assert bytes(digest.astype(np.uint8)) == b"4077112233"  # small files whole
    assert list(np.load(tmp_path / "a" / "counters.npy")) == [1, 2, 3, 4, 5, 6, 7]
    assert list(np.load(tmp_path / "a" / "file_sizes.npy")) == [len(big), 10]
    # a changed byte inside a sampled block shows up
    blk = bench.DUMP_SAMPLE_BLOCK
    rng = np.random.default_rng(bench.DUMP_SAMPLE_SEED)
    total_blocks = (len(big) + blk - 1) // blk
    pick = int(np.sort(rng.choice(total_blocks, size=bench.DUMP_SAMPLE_BYTES // blk,
                                  replace=False))[0])
    mod = bytearray(big)
    mod[pick * blk] ^= 0xFF
    (out / "oa-100-big-Data.db").write_bytes(bytes(mod))
    bench.dump_outputs(str(tmp_path / "c"), str(out), res)
    assert not np.array_equal(np.load(tmp_path / "c" / "oa-100-big-Data.db.npy"), data)
