"""GPU tests for chunk_length_in_kb from 1 to 64 KiB: the codecs on chosen
bytes, the writer, compaction over mixed-length inputs, an explicit output
length, scrub/verify, sharding/validate, rejections and the unchanged
defaults. Every comparison is byte for byte against the CPU oracle or the
system codec libraries; inputs at other chunk lengths are built on the CPU
(chunk_helpers.rechunk) and never depend on GPU code."""
import filecmp
import json
import os
import shutil
import subprocess

import pytest

import chunk_helpers as ch
from conftest import ORACLE

pytestmark = pytest.mark.gpu

KB4, KB16, KB64 = 4096, 16384, 65536


@pytest.fixture(scope="module")
def ca(product_lib):
    import cassandra_amd as mod
    if mod.device_count() < 1:
        pytest.skip("no GPU")
    return mod


def _oracle(*args, check=True):
    return subprocess.run([ORACLE, *[str(a) for a in args]], check=check,
                          capture_output=True, text=True)


def _assert_equal(base_a, base_b, components=ch.OA_COMPONENTS):
    for c in components:
        fa, fb = f"{base_a}-{c}", f"{base_b}-{c}"
        assert os.path.exists(fa), f"missing {fa}"
        assert os.path.exists(fb), f"missing {fb}"
        if not filecmp.cmp(fa, fb, shallow=False):
            a, b = open(fa, "rb").read(), open(fb, "rb").read()
            n = min(len(a), len(b))
            i = next((j for j in range(n) if a[j] != b[j]), n)
            raise AssertionError(f"{c}: len {len(a)} vs {len(b)}, first diff at {i}")


@pytest.fixture(scope="module")
def inputs(oracle_bin, tmp_path_factory):
    """Three overlapping oracle sstables (16 KiB chunks) and their CPU-built
    re-chunks, computed once: inputs[(i, C)] is input i (1..3) at C bytes."""
    d = str(tmp_path_factory.mktemp("clen_inputs"))
    _oracle("gen", d, "seed=77", "n=3", "rows=600", "vlen=700", "overlap=30", "tomb=10",
            "pdel=2")
    m = {(i, KB16): f"{d}/oa-{i}-big" for i in (1, 2, 3)}
    for i, c in [(1, KB4), (2, KB4), (3, KB4), (1, KB64), (2, KB64)]:
        m[(i, c)] = ch.rechunk(m[(i, KB16)], f"{d}/c{c}/oa-{i}-big", c, f"{d}/tmp{c}")
    return m


# ---- 1. codec direct --------------------------------------------------------
@pytest.mark.parametrize("chunk_len", [1024, 4096, 16384, 32768, 65536])
def test_codec_direct_lz4(ca, chunk_len):
    """compress_buffer == liblz4 chunk image, offsets included: three full
    chunks and a short tail of each of the eight content modes."""
    n = chunk_len * 3 + chunk_len * 3 // 10 + 7
    for mode in range(8):
        raw = ch.content(mode, n)
        want, want_offs = ch.chunk_image(raw, chunk_len, ch.lz4_payload)
        got, offs = ca.compress_buffer(raw, chunk_length=chunk_len)
        assert offs == want_offs, (mode, offs, want_offs)
        assert got == want, (mode, len(got), len(want))


@pytest.mark.parametrize("chunk_len", [1024, 4096, 16384, 32768, 65536])
def test_codec_direct_snappy(ca, chunk_len):
    lib = ch.snappy()
    if lib is None:
        pytest.skip("libsnappy not present (the oracle route below still runs)")
    n = chunk_len * 3 + chunk_len * 3 // 10 + 7
    for mode in range(8):
        raw = ch.content(mode, n)
        want, want_offs = ch.chunk_image(raw, chunk_len, lambda c: ch.snappy_payload(c, lib))
        got, offs = ca.compress_buffer(raw, chunk_length=chunk_len, snappy=True)
        assert offs == want_offs, (mode, offs, want_offs)
        assert got == want, (mode, len(got), len(want))


@pytest.mark.parametrize("chunk_len", [1024, 65536])
@pytest.mark.parametrize("codec", ["lz4", "snappy"])
def test_codec_direct_edge_lengths(ca, codec, chunk_len):
    """Whole-buffer lengths around the encoders' fixed limits (1 byte, the
    12/13-byte minimum for a match) and around one chunk: a lone short chunk,
    a full chunk, and a full chunk with a 1-, 12- or 13-byte tail chunk
    (tests/native/chunklen_cases.h's lengths), every content mode."""
    if codec == "snappy":
        lib = ch.snappy()
        if lib is None:
            pytest.skip("libsnappy not present")
        payload = lambda c: ch.snappy_payload(c, lib)
    else:
        payload = ch.lz4_payload
    L = chunk_len
    for n in (1, 12, 13, L - 1, L, L + 1, L + 12, L + 13):
        for mode in range(8):
            raw = ch.content(mode, n)
            want, want_offs = ch.chunk_image(raw, L, payload)
            got, offs = ca.compress_buffer(raw, chunk_length=L, snappy=codec == "snappy")
            assert offs == want_offs, (n, mode, offs, want_offs)
            assert got == want, (n, mode, len(got), len(want))
    assert ca.compress_buffer(b"", chunk_length=L, snappy=codec == "snappy") == (b"", [])


@pytest.mark.parametrize("chunk_len", [4096, 65536])
def test_codec_snappy_image_through_oracle(ca, oracle_bin, tmp_path, chunk_len):
    """The GPU's Snappy image of an sstable's bytes, wrapped as that sstable,
    is what the oracle's own Snappy writer produces (roundtrip's Data.db and
    CompressionInfo.db legs); no Python binding of libsnappy needed."""
    d = str(tmp_path)
    os.makedirs(d + "/s"), os.makedirs(d + "/l")
    spec = ["seed=55", "n=1", "rows=600", "vlen=700", "tomb=10"]
    _oracle("gen", d + "/s", *spec, "snappy=1")
    _oracle("gen", d + "/l", *spec)
    raw = ch.read_uncompressed(f"{d}/l/oa-1-big")
    image, offs = ca.compress_buffer(raw, chunk_length=chunk_len, snappy=True)
    assert len(offs) == (len(raw) + chunk_len - 1) // chunk_len >= 4
    ch.write_chunked(f"{d}/s/oa-1-big", f"{d}/g/oa-1-big", raw, chunk_len, image, offs)
    r = _oracle("roundtrip", f"{d}/g/oa-1-big", check=False)
    legs = {l.split()[1]: l.split()[0] for l in r.stdout.splitlines() if l.strip()}
    for leg in ("Data(uncompressed)", "Data.db", "CompressionInfo.db"):
        assert legs.get(leg) == "OK", r.stdout + r.stderr


# ---- 2. writer parity -------------------------------------------------------
WRITER_CASES = {
    "lz4": dict(rows_per_sstable=600, value_len=700),
    "snappy": dict(rows_per_sstable=600, value_len=700, snappy=True),
    "da": dict(rows_per_sstable=600, value_len=700, bti=True),
    # incompressible values: literal runs cover whole 64 KiB chunks
    "literal": dict(rows_per_sstable=600, value_len=1024, value_repeat_pct=0),
    "repeat": dict(rows_per_sstable=600, value_len=700, value_repeat_pct=100),
    # partitions spanning many 4 KiB chunks
    "wide": dict(rows_per_sstable=40, value_len=700, clustering_rows=60),
}


@pytest.mark.parametrize("chunk_len", [KB4, KB64])
@pytest.mark.parametrize("case", sorted(WRITER_CASES))
def test_writer_parity(ca, oracle_bin, tmp_path, case, chunk_len):
    """generate(chunk_length=C) == the oracle's rewrite of the same sstable,
    every component."""
    d = str(tmp_path)
    kw = WRITER_CASES[case]
    ca.generate(d, seed=61, n_sstables=1, tombstone_pct=10, chunk_length=chunk_len, **kw)
    base = f"{d}/da-1-bti" if kw.get("bti") else f"{d}/oa-1-big"
    comps = ch.DA_COMPONENTS if kw.get("bti") else ch.OA_COMPONENTS
    assert ch.chunk_length_of(base) == chunk_len
    out = f"{d}/o/" + os.path.basename(base)
    os.makedirs(d + "/o")
    _oracle("rewrite", base, out)
    assert ch.chunk_length_of(out) == chunk_len
    _assert_equal(base, out, comps)


@pytest.mark.parametrize("chunk_len", [1024, 2048, 8192, 32768])
def test_writer_parity_every_length(ca, oracle_bin, tmp_path, chunk_len):
    """The remaining powers of two, and the written sstable reads back:
    verify() and a compaction of it equal the oracle's."""
    d = str(tmp_path)
    ca.generate(d, seed=62, n_sstables=1, rows_per_sstable=300, value_len=700,
                tombstone_pct=10, chunk_length=chunk_len)
    os.makedirs(d + "/o")
    _oracle("rewrite", f"{d}/oa-1-big", f"{d}/o/oa-1-big")
    assert ch.chunk_length_of(f"{d}/o/oa-1-big") == chunk_len
    _assert_equal(f"{d}/oa-1-big", f"{d}/o/oa-1-big")
    ca.verify(f"{d}/oa-1-big")
    _oracle("compact", f"{d}/oa-90-big", f"{d}/o/oa-1-big")
    ca.compact([f"{d}/o/oa-1-big"], f"{d}/oa-91-big")
    _assert_equal(f"{d}/oa-90-big", f"{d}/oa-91-big")


@pytest.mark.parametrize("chunk_len", [KB4, KB64])
def test_flush_table_chunk_length(ca, oracle_bin, tmp_path, chunk_len):
    """gpuc_flush_table(chunk_length=C) of the oracle's memtable dump == the
    oracle's own sstable of that content re-chunked to C."""
    d = str(tmp_path)
    _oracle("gen", d, "seed=21", "n=1", "rows=600", "vlen=700", "tomb=15", "pdel=3", "dump=1")
    want = ch.rechunk(f"{d}/oa-1-big", f"{d}/w/oa-1-big", chunk_len, f"{d}/tmp")
    os.makedirs(d + "/g")
    ca.flush_table(f"{d}/oa-1-big.memdump", f"{d}/g/oa-1-big", chunk_length=chunk_len)
    _assert_equal(f"{d}/g/oa-1-big", want)


# ---- 3. compaction over mixed-length inputs --------------------------------
@pytest.mark.parametrize("first", [KB4, KB64])
def test_compact_mixed_inputs(ca, inputs, tmp_path, first):
    """4 KiB + 64 KiB + 16 KiB inputs in one job; the output follows
    inputs[0], in both orders."""
    d = str(tmp_path)
    a, b, c = inputs[(1, KB4)], inputs[(2, KB64)], inputs[(3, KB16)]
    ins = [a, b, c] if first == KB4 else [b, a, c]
    _oracle("compact", f"{d}/oa-90-big", *ins)
    ca.compact(ins, f"{d}/oa-91-big")
    assert ch.chunk_length_of(f"{d}/oa-91-big") == first
    _assert_equal(f"{d}/oa-90-big", f"{d}/oa-91-big")


def test_compact_modes_mixed_inputs(ca, inputs, tmp_path):
    """The other compaction modes share the ingest path: garbagecollect with
    a 64 KiB tombstone source, the anticompaction split and a token range,
    each over mixed-length inputs."""
    d = str(tmp_path)
    a, b, c = inputs[(1, KB4)], inputs[(2, KB64)], inputs[(3, KB16)]
    _oracle("compact", f"{d}/oa-80-big", a, c, f"tombsrc={b}")
    ca.compact([a, c], f"{d}/oa-81-big", tombstone_sources=[b])
    _assert_equal(f"{d}/oa-80-big", f"{d}/oa-81-big")
    ranges = [(-2**62, 0), (2**61, 2**62)]
    rs = ",".join(f"{lo}:{hi}" for lo, hi in ranges)
    _oracle("compact", f"{d}/oa-82-big", b, a, c, f"ranges={rs}", "invertranges=1")
    ca.compact([b, a, c], f"{d}/oa-83-big", keep_ranges=ranges, invert_ranges=True)
    _assert_equal(f"{d}/oa-82-big", f"{d}/oa-83-big")
    _oracle("compact", f"{d}/oa-84-big", a, b, c, f"shard={-2**61}:{2**62}")
    ca.compact([a, b, c], f"{d}/oa-85-big", token_range=(-2**61, 2**62))
    _assert_equal(f"{d}/oa-84-big", f"{d}/oa-85-big")


# ---- 4. explicit output length ---------------------------------------------
@pytest.mark.parametrize("out_len", [KB4, KB64])
def test_compact_explicit_output_length(ca, inputs, tmp_path, out_len):
    d = str(tmp_path)
    ins16 = [inputs[(i, KB16)] for i in (1, 2, 3)]
    ca.compact(ins16, f"{d}/oa-91-big", output_chunk_length=out_len)
    _oracle("compact", f"{d}/oa-90-big", inputs[(1, out_len)], ins16[1], ins16[2])
    assert ch.chunk_length_of(f"{d}/oa-91-big") == out_len
    _assert_equal(f"{d}/oa-90-big", f"{d}/oa-91-big")


# ---- 5. scrub and verify ----------------------------------------------------
def _copy_sstable(src_base, dst_dir):
    os.makedirs(dst_dir)
    prefix = os.path.basename(src_base) + "-"
    for fn in os.listdir(os.path.dirname(src_base)):
        if fn.startswith(prefix):
            shutil.copyfile(os.path.join(os.path.dirname(src_base), fn),
                            os.path.join(dst_dir, fn))
    return os.path.join(dst_dir, os.path.basename(src_base))


def _flip(base, off):
    with open(base + "-Data.db", "r+b") as f:
        f.seek(off)
        b0 = f.read(1)
        f.seek(off)
        f.write(bytes([b0[0] ^ 0x10]))


def test_verify_other_lengths(ca, inputs):
    ca.verify(inputs[(1, KB4)])
    ca.verify(inputs[(2, KB64)])


def test_scrub_granularity_follows_chunk(ca, inputs, tmp_path):
    """One flipped byte: GPU scrub == oracle scrub at 4 KiB (counts, bytes,
    output verifies and keeps its chunk length), and loses fewer partitions
    than the same flip at the same offset in the 16 KiB copy."""
    d = str(tmp_path)
    b4 = _copy_sstable(inputs[(1, KB4)], d + "/k4")
    b16 = _copy_sstable(inputs[(1, KB16)], d + "/k16")
    off = min(os.path.getsize(b4 + "-Data.db"), os.path.getsize(b16 + "-Data.db")) // 2
    dropped = {}
    for tag, base in (("k4", b4), ("k16", b16)):
        _flip(base, off)
        r = _oracle("scrub", f"{d}/{tag}/oa-80-big", base)
        ores = json.loads(r.stdout.splitlines()[-1])
        kept, drop = ca.scrub(base, f"{d}/{tag}/oa-81-big")
        assert drop > 0
        assert (kept, drop) == (ores["partitions_kept"], ores["partitions_dropped"])
        _assert_equal(f"{d}/{tag}/oa-80-big", f"{d}/{tag}/oa-81-big")
        ca.verify(f"{d}/{tag}/oa-81-big")
        dropped[tag] = drop
    assert ch.chunk_length_of(f"{d}/k4/oa-81-big") == KB4
    assert dropped["k4"] < dropped["k16"], dropped


# ---- 6. sharded outputs and validate ---------------------------------------
def test_sharded_outputs_4k(ca, inputs, tmp_path):
    from cassandra_amd.sharding import split_token_range
    d = str(tmp_path)
    ins = [inputs[(i, KB4)] for i in (1, 2, 3)]
    S = 4
    ca.compact(ins, f"{d}/oa-200-big", n_output_shards=S)
    for i in range(S):
        lo, hi = split_token_range(S, i)
        _oracle("compact", f"{d}/oa-{300 + i}-big", *ins, f"shard={lo}:{hi}")
        assert ch.chunk_length_of(f"{d}/oa-{200 + i}-big") == KB4
        _assert_equal(f"{d}/oa-{300 + i}-big", f"{d}/oa-{200 + i}-big")


def test_validate_mixed_inputs(ca, inputs, tmp_path):
    d = str(tmp_path)
    ins = [inputs[(1, KB4)], inputs[(2, KB64)], inputs[(3, KB16)]]
    _oracle("validate", f"{d}/v_cpu.bin", *ins)
    n = ca.validate(ins, f"{d}/v_gpu.bin")
    a, b = open(f"{d}/v_cpu.bin", "rb").read(), open(f"{d}/v_gpu.bin", "rb").read()
    assert n == len(a) // 40 > 0 and a == b


# ---- 7. rejections ----------------------------------------------------------
@pytest.mark.parametrize("bad", [131072, 12288])
def test_reject_output_chunk_length(ca, inputs, tmp_path, bad):
    out = f"{tmp_path}/oa-91-big"
    with pytest.raises(ca.GpuCompactError, match=r"rc=3.*chunk_length"):
        ca.compact([inputs[(1, KB16)]], out, output_chunk_length=bad)
    assert not os.path.exists(out + "-Data.db")
    with pytest.raises(ca.GpuCompactError, match=r"rc=3"):
        ca.generate(str(tmp_path), n_sstables=1, rows_per_sstable=10, chunk_length=bad)
    with pytest.raises(ca.GpuCompactError, match=r"rc=3"):
        ca.compress_buffer(b"x" * 100, chunk_length=bad)


@pytest.mark.parametrize("bad,rc", [(131072, 3), (12288, 2)])
def test_reject_compression_info(ca, inputs, tmp_path, bad, rc):
    """A CompressionInfo.db naming an unsupported length is refused when it
    is parsed — before any chunk is decoded — by every ingest path."""
    base = _copy_sstable(inputs[(1, KB16)], str(tmp_path / "p"))
    with open(base + "-CompressionInfo.db", "rb") as f:
        name, opts, _cl, mc, dl, offs = ch.parse_compression_info(f.read())
    with open(base + "-CompressionInfo.db", "wb") as f:
        f.write(ch.make_compression_info(name, opts, bad, mc, dl, offs))
    out = f"{tmp_path}/oa-91-big"
    with pytest.raises(ca.GpuCompactError, match=rf"rc={rc}.*chunk_length"):
        ca.compact([inputs[(2, KB16)], base], out)
    with pytest.raises(ca.GpuCompactError, match=rf"rc={rc}.*chunk_length"):
        ca.scrub(base, out)
    with pytest.raises(ca.GpuCompactError, match=rf"rc={rc}.*chunk_length"):
        ca.verify(base)
    with pytest.raises(ca.GpuCompactError, match=rf"rc={rc}.*chunk_length"):
        ca.validate([base], f"{tmp_path}/v.bin")
    assert not os.path.exists(out + "-Data.db")


# ---- 8. defaults ------------------------------------------------------------
def test_defaults_unchanged(ca, inputs, tmp_path):
    """Every new field zero: 16 KiB in, 16 KiB out, byte-identical to the
    oracle exactly as before."""
    d = str(tmp_path)
    os.makedirs(d + "/g")
    ca.generate(d + "/g", seed=77, n_sstables=3, rows_per_sstable=600, value_len=700,
                overlap_pct=30, tombstone_pct=10, partition_del_pct=2)
    for i in (1, 2, 3):
        _assert_equal(f"{d}/g/oa-{i}-big", inputs[(i, KB16)])
    ins = [inputs[(i, KB16)] for i in (1, 2, 3)]
    _oracle("compact", f"{d}/oa-90-big", *ins)
    ca.compact(ins, f"{d}/oa-91-big")
    assert ch.chunk_length_of(f"{d}/oa-91-big") == KB16
    _assert_equal(f"{d}/oa-90-big", f"{d}/oa-91-big")
