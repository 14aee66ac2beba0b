"""Compaction, validation, scrub, verify and flush of tables with descending
clustering columns (ReversedType), and TimestampType.

The reference of every positive case is the oracle's run over the MIRROR
tables (desc_tables.py) with the same job arguments, carried back to the real
clusterings; the engine works on the real tables and must give the same bytes
in all eight component files. test_desc_clustering_cpu.py shows that the
route is sound."""
import glob
import json
import os
import shutil
import subprocess
from dataclasses import replace

import pytest

import authored_tables as at
import desc_tables as dt
import merkle_helpers as mh
from conftest import ORACLE
from multi_cpx_helpers import COMPONENTS, assert_same_components
from size_split_helpers import cut_ranges, size_split_tool  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

ALL8 = COMPONENTS + ["TOC.txt"]
PURGE_NOW = 2000000000          # after every authored local deletion time
PURGING = at.Job(now=PURGE_NOW, gc_before=PURGE_NOW)
MIN_TOKEN, MAX_TOKEN = -2 ** 63, 2 ** 63 - 1


@pytest.fixture(scope="module")
def ca(product_lib):
    import cassandra_amd as mod
    if mod.device_count() < 1:
        pytest.skip("no GPU")
    return mod


@pytest.fixture(scope="module")
def tables(oracle_bin, tmp_path_factory):
    """case -> (DescCase, real bases, mirror bases), written once."""
    root = tmp_path_factory.mktemp("desc_gpu")
    cases = dict(dt.ALL_CASES, composite_snappy=lambda: dt.composite((False, True), snappy=1))
    out = {}
    for name, mk in cases.items():
        dc = mk()
        real, mirror = dc.write(oracle_bin, str(root / name))
        out[name] = (dc, real, mirror)
    return out


def _oracle_compact(out, inputs, *args):
    os.makedirs(os.path.dirname(out), exist_ok=True)
    r = subprocess.run([ORACLE, "compact", out, *inputs, *args], check=True, capture_output=True,
                       text=True)
    return json.loads(r.stdout.splitlines()[-1])


def _expected(dc, mirror, d, tag, *args):
    """The oracle's compaction of the mirrors, as the real sstable
    <d>/want_<tag>/oa-50-big (None when it holds no partition)."""
    o = _oracle_compact(f"{d}/cpu_{tag}/oa-50-big", mirror, *args)
    if not o["partitions_out"]:
        return None, o
    want = f"{d}/want_{tag}/oa-50-big"
    dt.expected_from_mirror(ORACLE, dc.ds, f"{d}/cpu_{tag}/oa-50-big", want)
    return want, o


def _assert_same(got, want, dc, what, d):
    try:
        assert_same_components(got, want, ALL8)
    except AssertionError as e:
        try:    # the oracle reads the tables back under their base types
            n = len(glob.glob(f"{d}/diff*"))
            os.makedirs(f"{d}/diff{n}/g"), os.makedirs(f"{d}/diff{n}/w")
            dt.to_base(dc.ds, got, f"{d}/diff{n}/g/oa-1-big")
            dt.to_base(dc.ds, want, f"{d}/diff{n}/w/oa-1-big")
            named = at.differing_cases(ORACLE, f"{d}/diff{n}/g/oa-1-big", f"{d}/diff{n}/w/oa-1-big",
                                       dc.matrix.labels, f"{d}/diff{n}")
        except Exception as e2:  # the engine's output may not even parse
            named = [f"(could not read the outputs back: {e2})"]
        raise AssertionError(
            f"{dc.name} [{what}]: {e}; {len(named)} cases differ (first file is the engine's):\n"
            + "\n".join(named[:12]))


def _compact_both(ca, dc, real, mirror, d, job, what, tag="j"):
    gpu = f"{d}/gpu_{tag}/oa-50-big"
    os.makedirs(os.path.dirname(gpu))
    want, o = _expected(dc, mirror, d, tag, *job.oracle_args())
    r = ca.compact(real, gpu, **job.gpu_kwargs())
    assert r["partitions_out"] == o["partitions_out"] and r["rows_out"] == o["rows_out"]
    if want is None:
        assert not glob.glob(gpu + "-*")
        return None
    _assert_same(gpu, want, dc, what, d)
    ca.verify(gpu)
    return gpu


# ---- compaction ---------------------------------------------------------------
@pytest.mark.parametrize("name", ["bigint", "composite_ad", "composite_da", "text", "edges_int",
                                  "edges_bigint", "blocks", "timestamp", "many",
                                  "composite_snappy"])
def test_compaction(ca, tables, tmp_path, name):
    dc, real, mirror = tables[name]
    gpu = _compact_both(ca, dc, real, mirror, str(tmp_path), at.Job(), "plain")
    hdr_ck, stats_ck, cols = dt.statistics_types(open(gpu + "-Statistics.db", "rb").read())
    assert hdr_ck == stats_ck == dc.ds.ck_strings()
    for nm in dc.ds.timestamp_cols:
        assert cols[nm] == dt.TIMESTAMP


@pytest.mark.parametrize("name", ["bigint", "text", "many"])
def test_purging_everything(ca, tables, tmp_path, name):
    """Every tombstone of the table is purgeable: rows under row deletions
    and ranges go, the markers with them."""
    dc, real, mirror = tables[name]
    _compact_both(ca, dc, real, mirror, str(tmp_path), PURGING, "purging")


def test_purge_bounds(ca, tables, tmp_path):
    """matrix_d's jobs (gc_before, now and overlaps on the stored values)."""
    dc, real, mirror = tables["purge"]
    for j, (label, job) in enumerate(dc.matrix.jobs):
        _compact_both(ca, dc, real, mirror, str(tmp_path), job, label, tag=f"j{j}")


# ---- modes that share the front end and the writer ----------------------------
def test_output_shards(ca, tables, tmp_path):
    from cassandra_amd.sharding import split_token_range
    dc, real, mirror = tables["bigint"]
    d = str(tmp_path)
    os.makedirs(f"{d}/gpu")
    r = ca.compact(real, f"{d}/gpu/oa-200-big", n_output_shards=2)
    assert r["n_outputs"] == 2
    for i in range(2):
        lo, hi = split_token_range(2, i)
        want, o = _expected(dc, mirror, d, f"s{i}", f"shard={lo}:{hi}")
        assert o["partitions_out"] > 0
        _assert_same(f"{d}/gpu/oa-{200 + i}-big", want, dc, f"shard {i}", d)
        ca.verify(f"{d}/gpu/oa-{200 + i}-big")


def test_max_output_bytes(ca, tables, size_split_tool, tmp_path):  # noqa: F811
    """Cut at an on-disk size: the cut points are those of the expected
    single output (read under its base types), every output the oracle's
    sstable of its token range."""
    dc, real, mirror = tables["bigint"]
    d = str(tmp_path)
    cap = 2000
    whole, o = _expected(dc, mirror, d, "whole")
    os.makedirs(f"{d}/wholeb")
    dt.to_base(dc.ds, whole, f"{d}/wholeb/oa-900-big")
    cuts = cut_ranges(size_split_tool, f"{d}/wholeb/oa-900-big", cap)
    os.makedirs(f"{d}/gpu")
    r = ca.compact(real, f"{d}/gpu/oa-500-big", max_output_bytes=cap)
    print("outputs", r["n_outputs"], "want", len(cuts))
    assert r["n_outputs"] >= 2 and r["n_outputs"] == len(cuts)
    assert r["partitions_out"] == o["partitions_out"]
    for k, c in enumerate(cuts):
        want, _ = _expected(dc, mirror, d, f"c{k}", f"shard={c['first_token']}:{c['last_token']}")
        _assert_same(f"{d}/gpu/oa-{500 + k}-big", want, dc, f"output {k}", d)
        ca.verify(f"{d}/gpu/oa-{500 + k}-big")
    assert not glob.glob(f"{d}/gpu/oa-{500 + len(cuts)}-big-*")


def test_routed_outputs(ca, tables, tmp_path):
    dc, real, mirror = tables["bigint"]
    d = str(tmp_path)
    os.makedirs(f"{d}/gpu")
    bases = [f"{d}/gpu/oa-10-big", f"{d}/gpu/oa-11-big"]
    r = ca.compact_routed(real, bases, [(MIN_TOKEN, -1, 0)], 1)
    assert [x["written"] for x in r["outputs"]] == [1, 1]
    for i, (lo, hi) in enumerate([(MIN_TOKEN, -1), (0, MAX_TOKEN)]):
        want, o = _expected(dc, mirror, d, f"r{i}", f"shard={lo}:{hi}")
        assert r["outputs"][i]["partitions"] == o["partitions_out"] > 0
        _assert_same(bases[i], want, dc, f"routed output {i}", d)
        ca.verify(bases[i])


def test_token_range_and_keep_ranges(ca, tables, tmp_path):
    dc, real, mirror = tables["many"]
    d = str(tmp_path)
    tokens = (-2 ** 62, 3 * 2 ** 61)
    ranges = [(-3 * 2 ** 61, -2 ** 61), (-2 ** 60, 2 ** 62)]
    os.makedirs(f"{d}/gpu")
    r = ca.compact(real, f"{d}/gpu/oa-50-big", token_range=tokens, keep_ranges=ranges)
    want, o = _expected(dc, mirror, d, "t", f"shard={tokens[0]}:{tokens[1]}",
                        "ranges=" + ",".join(f"{lo}:{hi}" for lo, hi in ranges))
    assert 0 < o["partitions_out"] == r["partitions_out"]
    _assert_same(f"{d}/gpu/oa-50-big", want, dc, "token range + kept ranges", d)


@pytest.mark.parametrize("cell_level", [0, 1])
def test_garbage_collection(ca, tables, tmp_path, cell_level):
    """A tombstone source over a descending table, ROW and CELL mode."""
    dc, real, mirror = tables["gc"]
    d = str(tmp_path)
    os.makedirs(f"{d}/gpu")
    ca.compact(real[:2], f"{d}/gpu/oa-50-big", tombstone_sources=[real[2]],
               cell_level_gc=bool(cell_level))
    want, o = _expected(dc, mirror[:2], d, "gc", f"tombsrc={mirror[2]}",
                        *(["cellgc=1"] if cell_level else []))
    assert o["partitions_out"] > 0
    _assert_same(f"{d}/gpu/oa-50-big", want, dc, f"cellgc={cell_level}", d)
    ca.verify(f"{d}/gpu/oa-50-big")


@pytest.mark.parametrize("name", ["bigint", "text", "timestamp"])
def test_validate(ca, tables, tmp_path, name):
    """The repair digests over the descending inputs equal `oracle_tool
    validate` of the expected output under its base types: the digest hashes
    clustering value bytes and stream order, not types."""
    dc, real, mirror = tables[name]
    d = str(tmp_path)
    want, _ = _expected(dc, mirror, d, "v")
    os.makedirs(f"{d}/wantb")
    dt.to_base(dc.ds, want, f"{d}/wantb/oa-50-big")
    gpu, cpu = f"{d}/gpu.digests", f"{d}/cpu.digests"
    n = ca.validate(real, gpu)
    subprocess.run([ORACLE, "validate", cpu, f"{d}/wantb/oa-50-big"], check=True,
                   capture_output=True)
    a, b = open(gpu, "rb").read(), open(cpu, "rb").read()
    assert n * 40 == len(a) and n > 0
    assert a == b
    # and reduced to Merkle leaves on the device
    trees = mh.even_split(64)
    want_leaves = mh.reduce_leaves(mh.read_records(cpu), trees)
    got = ca.validate_merkle(real, trees)
    assert (list(got[0]), list(got[1]), got[2]) == (want_leaves[0], want_leaves[1], n)


def test_scrub(ca, tables, tmp_path):
    """A clean descending input: everything kept, and the output reads back
    equal to the input."""
    dc, real, _ = tables["text"]
    d = str(tmp_path)
    os.makedirs(f"{d}/out"), os.makedirs(f"{d}/inb"), os.makedirs(f"{d}/outb")
    kept, dropped = ca.scrub(real[0], f"{d}/out/oa-81-big")
    assert (kept, dropped) == (len(dc.real_inputs()[0]), 0)
    ca.verify(f"{d}/out/oa-81-big")
    assert dt.statistics_types(open(f"{d}/out/oa-81-big-Statistics.db", "rb").read())[0] == \
        dc.ds.ck_strings()
    dt.to_base(dc.ds, real[0], f"{d}/inb/oa-1-big")
    dt.to_base(dc.ds, f"{d}/out/oa-81-big", f"{d}/outb/oa-1-big")
    a = at.read_sstable(ORACLE, f"{d}/inb/oa-1-big", f"{d}/a.memdump")
    b = at.read_sstable(ORACLE, f"{d}/outb/oa-1-big", f"{d}/b.memdump")
    assert a.keys() == b.keys() and len(a) == kept
    for n in a:
        assert at.canonical(a[n]) == at.canonical(b[n]), dc.matrix.labels[n]


@pytest.mark.parametrize("name", ["bigint", "text"])
def test_flush_table(ca, tables, tmp_path, name):
    """flush_table with the ck_types override equals fromdump + rewrite of the
    same content; the same partitions in ascending order are refused."""
    dc, real, _ = tables[name]
    d = str(tmp_path)
    parts = dc.real_inputs()[0]
    md = f"{d}/real.memdump"
    with open(md, "wb") as f:
        f.write(at.to_gmd2(dc.ds.base, parts))
    os.makedirs(f"{d}/gpu")
    ca.flush_table(md, f"{d}/gpu/oa-1-big", ck_types=dc.ds.ck_strings())
    _assert_same(f"{d}/gpu/oa-1-big", real[0], dc, "flush", d)
    ca.verify(f"{d}/gpu/oa-1-big")
    # ascending under the base type == the wrong order under the real one
    rows = lambda p: [it for it in p.items if isinstance(it, at.Row)]
    asc = [at.Partition(p.key, p.del_, p.static, list(reversed(rows(p)))) for p in parts
           if len(rows(p)) > 1]
    assert asc
    with open(f"{d}/asc.memdump", "wb") as f:
        f.write(at.to_gmd2(dc.ds.base, asc))
    os.makedirs(f"{d}/asc")
    with pytest.raises(ca.GpuCompactError, match=r"clustering order in partition \d+"):
        ca.flush_table(f"{d}/asc.memdump", f"{d}/asc/oa-1-big", ck_types=dc.ds.ck_strings())
    assert not glob.glob(f"{d}/asc/oa-1-big-*")
    # and they are a legal flush without the override
    ca.flush_table(f"{d}/asc.memdump", f"{d}/asc/oa-2-big")


# ---- refusals: GPUC_ERR_UNSUPPORTED, the message checked, no output -----------
def _rejected(ca, tmp_path, inputs, match):
    out = str(tmp_path / "out" / "oa-50-big")
    os.makedirs(os.path.dirname(out))
    with pytest.raises(ca.GpuCompactError, match=match) as e:
        ca.compact(inputs, out)
    assert "rc=3" in str(e.value)
    assert not glob.glob(out + "*"), "an output file was created"


def test_rejects_ascending_with_descending(ca, tables, tmp_path):
    """The mirror of a bigint table is a legal ascending LongType table."""
    dc, real, mirror = tables["bigint"]
    _rejected(ca, tmp_path, [real[0], mirror[1]], r"inputs differ in their clustering types")


def test_rejects_a_da_input_of_a_descending_table(ca, oracle_bin, tables, tmp_path):
    """The ascending `da` twin with its Statistics.db rewritten."""
    dc = tables["bigint"][0]
    d = str(tmp_path)
    ds = dt.DescSchema(replace(dc.ds.base, bti=1), dc.ds.desc)
    base = f"{d}/in/da-1-bti"
    dt.write_real(oracle_bin, ds, dc.mirror_inputs()[0], base)
    assert os.path.exists(base + "-Rows.db") and not os.path.exists(base + "-Index.db")
    _rejected(ca, tmp_path, [base], r"descending clustering column.*ReversedType\(.*LongType\)")
    with pytest.raises(ca.GpuCompactError, match=r"rc=3.*descending clustering column"):
        ca.verify(base)


def test_rejects_reversed_uuid(ca, tables, tmp_path):
    dc, real, _ = tables["bigint"]
    d = str(tmp_path)
    os.makedirs(f"{d}/in")
    for fn in glob.glob(real[0] + "-*"):
        shutil.copy(fn, f"{d}/in/" + os.path.basename(fn))
    base = f"{d}/in/" + os.path.basename(real[0])
    uuid = [dt.reversed_type(dt.MARSHAL + b"UUIDType")]
    data = open(base + "-Statistics.db", "rb").read()
    with open(base + "-Statistics.db", "wb") as f:
        f.write(dt.rewrite_statistics(data, dc.ds.ck_strings(), uuid))
    _rejected(ca, tmp_path, [base],
              r"unsupported clustering type org\.apache\.cassandra\.db\.marshal\.ReversedType\("
              r"org\.apache\.cassandra\.db\.marshal\.UUIDType\)")
