"""GPU chunk decoders on streams from other LZ4/Snappy encoders: LZ4HC and
LZ4 fast output, transcoded LZ4 blocks (split matches, demoted match heads,
literal-only) and re-emitted Snappy fragments (widened literal fields,
copy-2/copy-4 tags, 1..3-byte copies, literal-only), over chosen plaintext
(tests/foreign_streams.py). Every stream sent to the device has passed the
CPU checks of test_foreign_streams_cpu.py's kind first; the expected bytes
come from the CPU oracle reading the canonically encoded sstable, so one
wrong decoded byte changes a compared file."""
import filecmp
import os

import pytest

import chunk_helpers as ch
import foreign_streams as fs
from conftest import oracle_run

pytestmark = pytest.mark.gpu

CASES = [(codec, name) for codec in ("lz4", "snappy") for name in fs.variant_names(codec)]


@pytest.fixture(scope="module")
def ca(product_lib):
    import cassandra_amd as mod
    if mod.device_count() < 1:
        pytest.skip("no GPU")
    return mod


@pytest.fixture(scope="module")
def corpus(oracle_bin, tmp_path_factory):
    return fs.Corpus(tmp_path_factory.mktemp("foreign_gpu"))


def _assert_equal(base_a, base_b):
    for c in ch.OA_COMPONENTS:
        fa, fb = f"{base_a}-{c}", f"{base_b}-{c}"
        assert os.path.exists(fa), f"missing {fa}"
        assert os.path.exists(fb), f"missing {fb}"
        if not filecmp.cmp(fa, fb, shallow=False):
            a, b = open(fa, "rb").read(), open(fb, "rb").read()
            n = min(len(a), len(b))
            i = next((j for j in range(n) if a[j] != b[j]), n)
            raise AssertionError(f"{c}: len {len(a)} vs {len(b)}, first diff at {i}")


def _checked_variant(corpus, codec, chunk_len, name, which="main"):
    """The variant sstable, after the CPU reference decoder and the frame
    bound have accepted every one of its streams."""
    base = corpus.variant(codec, chunk_len, name, which)
    if base is None:
        pytest.skip("libsnappy not present")
    _n, cl, _dl, payloads = fs.read_payloads(base)
    chunks = corpus.chunks(chunk_len, which)
    assert cl == chunk_len and len(payloads) == len(chunks)
    for c, v in zip(chunks, payloads):
        assert fs.run_ops(fs.parse(v, codec)) == c
        assert len(v) <= fs.frame_bound(codec, len(c))
    return base


@pytest.mark.parametrize("chunk_len", fs.CHUNK_LENGTHS)
@pytest.mark.parametrize("codec,name", CASES)
def test_verify_and_compact(ca, corpus, tmp_path, codec, name, chunk_len):
    """verify() accepts the variant, and compacting it gives the oracle's
    compaction of the canonical sstable: the value bytes go through decode,
    parse, serialize and re-compress."""
    base = _checked_variant(corpus, codec, chunk_len, name)
    ca.verify(base)
    out = f"{tmp_path}/oa-3-big"
    ca.compact([base], out)
    assert ch.chunk_length_of(out) == chunk_len
    _assert_equal(out, corpus.canon_compacted(codec, chunk_len))


@pytest.mark.parametrize("chunk_len", fs.CHUNK_LENGTHS)
@pytest.mark.parametrize("codec", ["lz4", "snappy"])
def test_single_chunk(ca, corpus, tmp_path, codec, chunk_len):
    """n == 1: the wave's second half has no chunk."""
    base = _checked_variant(corpus, codec, chunk_len, fs.HEAVIEST[codec], "tiny")
    assert len(fs.read_payloads(base)[3]) == 1
    ca.verify(base)
    out = f"{tmp_path}/oa-3-big"
    ca.compact([base], out)
    _assert_equal(out, corpus.canon_compacted(codec, chunk_len, "tiny"))


@pytest.mark.parametrize("codec", ["lz4", "snappy"])
def test_validate_and_scrub(ca, corpus, tmp_path, codec):
    """The other two ingest paths, on the most heavily split variant at 1 KiB
    chunks: repair digests equal the canonical input's and the oracle's;
    scrub keeps every partition and writes what it writes for the canonical
    input."""
    d = str(tmp_path)
    canon = corpus.canon(codec, 1024)
    base = _checked_variant(corpus, codec, 1024, fs.HEAVIEST[codec])
    oracle_run("validate", f"{d}/v_cpu.bin", canon)
    n_var = ca.validate([base], f"{d}/v_var.bin")
    n_can = ca.validate([canon], f"{d}/v_can.bin")
    want = open(f"{d}/v_cpu.bin", "rb").read()
    assert n_var == n_can == len(want) // 40 == len(fs.rows())
    assert open(f"{d}/v_var.bin", "rb").read() == want
    assert open(f"{d}/v_can.bin", "rb").read() == want
    os.makedirs(f"{d}/sv"), os.makedirs(f"{d}/sc")
    assert ca.scrub(base, f"{d}/sv/oa-5-big") == (len(fs.rows()), 0)
    assert ca.scrub(canon, f"{d}/sc/oa-5-big") == (len(fs.rows()), 0)
    _assert_equal(f"{d}/sv/oa-5-big", f"{d}/sc/oa-5-big")


def test_compact_mixed_encoders(ca, oracle_bin, tmp_path):
    """One job over a canonical 16 KiB input, an LZ4HC input at 4 KiB and a
    split-match input at 64 KiB (overlapping keys) == the oracle compacting
    the three canonical sstables."""
    d = str(tmp_path)
    oracle_run("gen", d, "seed=78", "n=3", "rows=300", "vlen=700", "overlap=30", "tomb=10",
               "pdel=2")
    a = f"{d}/oa-1-big"
    b = ch.rechunk(f"{d}/oa-2-big", f"{d}/c4/oa-2-big", 4096, f"{d}/tmp4")
    c = ch.rechunk(f"{d}/oa-3-big", f"{d}/c64/oa-3-big", 65536, f"{d}/tmp64")
    variants = fs.lz4_variants()
    raw_b, raw_c = ch.read_uncompressed(b), ch.read_uncompressed(c)
    hc = fs.write_variant(b, f"{d}/hc/oa-2-big", raw_b, 4096, variants["hc9"]())
    split = fs.write_variant(c, f"{d}/split/oa-3-big", raw_c, 65536, variants["split"]())
    for base, raw, cl in ((hc, raw_b, 4096), (split, raw_c, 65536)):
        payloads = fs.read_payloads(base)[3]
        assert payloads != fs.read_payloads(b if base is hc else c)[3]
        for chunk, v in zip(fs.split_chunks(raw, cl), payloads):
            assert fs.run_ops(fs.lz4_parse(v)) == chunk
            assert len(v) <= fs.lz4_bound(len(chunk))
    fs.oracle_compact(f"{d}/oa-90-big", a, b, c)
    ca.compact([a, hc, split], f"{d}/oa-91-big")
    _assert_equal(f"{d}/oa-90-big", f"{d}/oa-91-big")
