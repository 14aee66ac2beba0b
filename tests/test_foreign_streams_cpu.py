"""The foreign-stream corpus itself, checked on the CPU: every variant of
tests/foreign_streams.py is a valid stream of the chunk it stands for (the
plain reference decoder, the system decoder and the oracle agree, and it fits
the GPU decoders' frame bound), and together the variants contain the shapes
the GPU tests are about (census conditions). No GPU code runs here."""
import filecmp
import subprocess

import pytest

import chunk_helpers as ch
import foreign_streams as fs
from conftest import ORACLE

CASES = [(codec, name) for codec in ("lz4", "snappy") for name in fs.variant_names(codec)]


@pytest.fixture(scope="module")
def corpus(oracle_bin, tmp_path_factory):
    return fs.Corpus(tmp_path_factory.mktemp("foreign_cpu"))


def _payloads(corpus, codec, chunk_len, name):
    ps = corpus.payloads(codec, chunk_len, name)
    if ps is None:
        pytest.skip("libsnappy not present")
    return ps


def test_corpus_shape(corpus):
    """3 chunks at 64 KiB (an odd count), ~143 at 1 KiB, one chunk in the tiny
    sstable at every length."""
    assert len(corpus.chunks(65536)) == 3
    assert 140 <= len(corpus.chunks(1024)) <= 150
    for c in fs.CHUNK_LENGTHS:
        assert len(corpus.chunks(c, "tiny")) == 1


def test_emitters_invert_parsers():
    """emit(parse(x)) of a canonical stream is x again, for both codecs."""
    raw = fs.rows()[4][2] + fs.rows()[7][2] + bytes(range(256)) * 2
    p = ch.lz4_payload(raw)
    assert fs.lz4_emit(fs.lz4_parse(p)) == p
    lib = ch.snappy()
    if lib is not None:
        p = ch.snappy_payload(raw, lib)
        assert fs.snappy_emit(fs.snappy_parse(p)) == p
    ops = [("lit", b"abc"), ("copy", 3, 70), ("copy", 2, 3), ("lit", b"x" * 300)]
    for knobs in ({}, {"lit_width": 4}, {"copy_kind": 3}, {"lit_width": 2, "copy_kind": 2}):
        assert fs.run_ops(fs.snappy_parse(fs.snappy_emit(ops, knobs))) == fs.run_ops(ops)


@pytest.mark.parametrize("chunk_len", [1024, 65536])
@pytest.mark.parametrize("codec,name", CASES)
def test_variant_is_valid(corpus, tmp_path, codec, name, chunk_len):
    chunks = corpus.chunks(chunk_len)
    ps = _payloads(corpus, codec, chunk_len, name)
    assert len(ps) == len(chunks)
    for i, (c, v) in enumerate(zip(chunks, ps)):
        assert fs.run_ops(fs.parse(v, codec)) == c, i
        # a condition on the inputs: the GPU decoders refuse longer frames
        assert len(v) <= fs.frame_bound(codec, len(c)), (i, len(v), len(c))
        if codec == "lz4":
            assert fs.lz4_decompress_safe(v) == c, i
        else:
            assert fs.snappy_lib_uncompress(v) in ("absent", c), i
    base = corpus.variant(codec, chunk_len, name)
    if codec == "snappy":
        # the oracle's own Snappy decoder reads the wrapped sstable
        r = subprocess.run([ORACLE, "roundtrip", base], capture_output=True, text=True)
        legs = {l.split()[1]: l.split()[0] for l in r.stdout.splitlines() if l.strip()}
        assert legs.get("Data(uncompressed)") == "OK", r.stdout + r.stderr
    out = fs.oracle_compact(f"{tmp_path}/oa-3-big", base)
    want = corpus.canon_compacted(codec, chunk_len)
    for comp in ch.OA_COMPONENTS:
        assert filecmp.cmp(f"{out}-{comp}", f"{want}-{comp}", shallow=False), comp


def _union(corpus, codec, chunk_len, which="main"):
    total = None
    for name in fs.variant_names(codec):
        ps = corpus.payloads(codec, chunk_len, name, which)
        if ps is None:
            continue
        c = fs.census(ps, codec)
        total = c if total is None else fs.merge_census(total, c)
    return total


# The census conditions keep the GPU tests from going vacuous: if one fails,
# the row recipe or the split points change, never the condition.
@pytest.mark.parametrize("chunk_len", fs.CHUNK_LENGTHS)
def test_census_lz4(corpus, chunk_len):
    c = _union(corpus, "lz4", chunk_len)
    print("census lz4", chunk_len, c)
    assert {1, 2, 3, 5, 7} <= set(c["overlapped_offsets"]), c
    assert c["len_eq_off"] and c["len_eq_off_plus_1"], c
    assert c["zero_literal_sequences"] > 0, c
    assert c["lit_ext_ends_in_0"] > 0 and c["match_ext_ends_in_0"] > 0, c
    assert c["lit_ext_255x2"] > 0 and c["match_ext_255x2"] > 0, c
    assert c["literal_edges"] == list(fs.LIT_EDGES), c
    assert c["match_edges"] == list(fs.MATCH_EDGES), c
    if chunk_len == 65536:
        assert c["max_offset"] > 32768, c


@pytest.mark.parametrize("chunk_len", fs.CHUNK_LENGTHS)
def test_census_snappy(corpus, chunk_len):
    c = _union(corpus, "snappy", chunk_len)
    print("census snappy", chunk_len, c)
    assert c["kinds"] == [0, 1, 2, 3], c
    assert c["literal_widths"] == [0, 1, 2, 3, 4] and c["nonminimal_literals"] > 0, c
    assert c["copy2_short_lengths"] == [1, 2, 3], c
    assert {4, 11} <= set(c["copy1_lengths"]), c
    assert 1 in c["small_offsets"], c
    assert {2, 3, 4, 5, 6, 7} <= set(c["overlapped_offsets"]), c
    if chunk_len > 2047:
        # copy-1's widest offset: the row whose tail repeats its head
        assert c["copy1_max_offset"] == 2047, c


@pytest.mark.parametrize("codec", ["lz4", "snappy"])
def test_heaviest_variant_reaches_the_tiny_sstable(corpus, codec):
    """The single-chunk sstable is not literal-only under the most heavily
    split variant, so the n == 1 GPU case decodes copies."""
    ps = corpus.payloads(codec, 1024, fs.HEAVIEST[codec], "tiny")
    assert len(ps) == 1
    ops = fs.parse(ps[0], codec)
    assert fs.run_ops(ops) == corpus.raw["tiny"]
    assert sum(op[0] == "copy" for op in ops) >= 8, ops
    c = fs.census(ps, codec)
    assert {3, 7} <= set(c["overlapped_offsets"]), c


def test_alternating_chunks_differ_in_shape(corpus):
    """Chunks 2k and 2k+1 share a decode wave: even ones are one literal, odd
    ones the most heavily split."""
    for codec in ("lz4", "snappy"):
        ps = corpus.payloads(codec, 1024, "alternating")
        n_ops = [len(fs.parse(p, codec)) for p in ps]
        assert all(n == 1 for n in n_ops[0::2]), codec
        assert max(n_ops[1::2]) > 100, codec
