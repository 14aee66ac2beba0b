"""Compaction, validation, scrub, verify and flush of tables with set and
typed-key map columns and frozen columns.

The reference of every positive case is the oracle's run over the MIRROR
tables (collection_tables.py) with the same job arguments, carried back to
the real cell paths and type strings; the engine works on the real tables and
must give the same bytes in all eight component files.
test_collection_types_cpu.py shows that the route is sound. Every compaction
here fails on an engine that refuses the types; set_int_edges also fails on
one that accepts the strings but keeps the unsigned byte compare of paths."""
import glob
import json
import os
import subprocess

import pytest

import authored_tables as at
import collection_tables as ct
import desc_tables as dt
import merkle_helpers as mh
from authored_tables import BYTES, DT_LIVE, MAP_BB, Case, Matrix, Partition, Row, Schema
from conftest import ORACLE
from multi_cpx_helpers import BTI_COMPONENTS, COMPONENTS, assert_same_components
from size_split_helpers import cut_ranges, size_split_tool  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

MIN_TOKEN, MAX_TOKEN = -2 ** 63, 2 ** 63 - 1
CASES = dict(ct.ALL_CASES, set_int_edges_snappy=lambda: ct.set_int_edges(snappy=1),
             set_int_edges_da=lambda: ct.set_int_edges(bti=1))


@pytest.fixture(scope="module")
def ca(product_lib):
    import cassandra_amd as mod
    if mod.device_count() < 1:
        pytest.skip("no GPU")
    return mod


@pytest.fixture(scope="module")
def tables(oracle_bin, tmp_path_factory):
    """case -> (CollCase, real bases, mirror bases), written once."""
    root = tmp_path_factory.mktemp("coll_gpu")
    out = {}
    for name, mk in CASES.items():
        c = mk()
        real, mirror = c.write(oracle_bin, str(root / name))
        out[name] = (c, real, mirror)
    return out


def _all8(c):
    return (BTI_COMPONENTS if c.schema.bti else COMPONENTS) + ["TOC.txt"]


def _oracle_compact(out, inputs, *args):
    os.makedirs(os.path.dirname(out), exist_ok=True)
    r = subprocess.run([ORACLE, "compact", out, *inputs, *args], check=True, capture_output=True,
                       text=True)
    return json.loads(r.stdout.splitlines()[-1])


def _expected(c, mirror, d, tag, *args):
    """The oracle's compaction of the mirrors as the real sstable
    <d>/want_<tag>/<stem 50> (None when it holds no partition)."""
    o = _oracle_compact(f"{d}/cpu_{tag}/{c.stem(50)}", mirror, *args)
    if not o["partitions_out"]:
        return None, o
    want = f"{d}/want_{tag}/{c.stem(50)}"
    ct.expected(ORACLE, c, f"{d}/cpu_{tag}/{c.stem(50)}", want)
    return want, o


def _assert_same(got, want, c, what, d):
    try:
        assert_same_components(got, want, _all8(c))
    except AssertionError as e:
        try:    # the oracle reads the tables back under their base types
            n = len(glob.glob(f"{d}/diff*"))
            ct.to_base(c, got, f"{d}/diff{n}/g/{c.stem(1)}")
            ct.to_base(c, want, f"{d}/diff{n}/w/{c.stem(1)}")
            named = at.differing_cases(ORACLE, f"{d}/diff{n}/g/{c.stem(1)}",
                                       f"{d}/diff{n}/w/{c.stem(1)}", c.matrix.labels, f"{d}/diff{n}")
        except Exception as e2:  # the engine's output may not even parse
            named = [f"(could not read the outputs back: {e2})"]
        raise AssertionError(
            f"{c.name} [{what}]: {e}; {len(named)} cases differ (first file is the engine's):\n"
            + "\n".join(named[:12]))


def _compact_both(ca, c, real, mirror, d, job, what, tag="j"):
    gpu = f"{d}/gpu_{tag}/{c.stem(50)}"
    os.makedirs(os.path.dirname(gpu))
    want, o = _expected(c, mirror, d, tag, *job.oracle_args())
    r = ca.compact(real, gpu, **job.gpu_kwargs())
    assert r["partitions_out"] == o["partitions_out"] and r["rows_out"] == o["rows_out"]
    if want is None:
        assert not glob.glob(gpu + "-*")
        return None
    _assert_same(gpu, want, c, what, d)
    ca.verify(want)
    return gpu


def _header_types(base):
    return dt.statistics_types(open(base + "-Statistics.db", "rb").read())[2]


# ---- compaction ---------------------------------------------------------------
@pytest.mark.parametrize("name", ["set_text", "set_int_edges", "map_bigint_text",
                                  "map_timestamp_blob", "map_bigint_wide", "mixed", "union",
                                  "set_int_edges_snappy",
                                  "set_int_edges_da"])
def test_compaction(ca, tables, tmp_path, name):
    c, real, mirror = tables[name]
    gpu = _compact_both(ca, c, real, mirror, str(tmp_path), at.Job(), "plain")
    cols = _header_types(gpu)
    for nm in c.all_names():
        assert cols[nm] == c.types.get(nm, c.base_type(nm))


def test_union_header_order(ca, tables, tmp_path):
    """The frozen column sorts among the simple ones in the output header."""
    c, real, _ = tables["union"]
    os.makedirs(f"{tmp_path}/o")
    ca.compact(real, f"{tmp_path}/o/oa-50-big")
    assert list(_header_types(f"{tmp_path}/o/oa-50-big")) == [b"a", b"f", b"zs"]
    assert list(_header_types(real[0])) == [b"a", b"f"] and list(_header_types(real[1])) == [b"a", b"zs"]


@pytest.mark.parametrize("name", ["set_int_edges", "mixed"])
def test_purge(ca, tables, tmp_path, name):
    """Purge of everything and the gc_before bounds on the stored values."""
    c, real, mirror = tables[name]
    for j, (label, job) in enumerate(c.matrix.jobs[1:]):
        _compact_both(ca, c, real, mirror, str(tmp_path), job, label, tag=f"j{j}")


# ---- modes that share the front end and the writer ----------------------------
def test_output_shards(ca, tables, tmp_path):
    from cassandra_amd.sharding import split_token_range
    c, real, mirror = tables["mixed"]
    d = str(tmp_path)
    os.makedirs(f"{d}/gpu")
    r = ca.compact(real, f"{d}/gpu/oa-200-big", n_output_shards=2)
    assert r["n_outputs"] == 2
    for i in range(2):
        lo, hi = split_token_range(2, i)
        want, o = _expected(c, mirror, d, f"s{i}", f"shard={lo}:{hi}")
        assert o["partitions_out"] > 0
        _assert_same(f"{d}/gpu/oa-{200 + i}-big", want, c, f"shard {i}", d)
        ca.verify(f"{d}/gpu/oa-{200 + i}-big")


def test_max_output_bytes(ca, tables, size_split_tool, tmp_path):  # noqa: F811
    """Cut at an on-disk size: the cut points are those of the expected
    single output (read under its base types), every output the expected
    sstable of its token range."""
    c, real, mirror = tables["map_bigint_wide"]
    d = str(tmp_path)
    cap = 300
    whole, o = _expected(c, mirror, d, "whole")
    ct.to_base(c, whole, f"{d}/wholeb/oa-900-big")
    cuts = cut_ranges(size_split_tool, f"{d}/wholeb/oa-900-big", cap)
    os.makedirs(f"{d}/gpu")
    r = ca.compact(real, f"{d}/gpu/oa-500-big", max_output_bytes=cap)
    print("outputs", r["n_outputs"], "want", len(cuts))
    assert r["n_outputs"] >= 2 and r["n_outputs"] == len(cuts)
    assert r["partitions_out"] == o["partitions_out"]
    for k, cut in enumerate(cuts):
        want, _ = _expected(c, mirror, d, f"c{k}", f"shard={cut['first_token']}:{cut['last_token']}")
        _assert_same(f"{d}/gpu/oa-{500 + k}-big", want, c, f"output {k}", d)
    assert not glob.glob(f"{d}/gpu/oa-{500 + len(cuts)}-big-*")


def test_routed_outputs(ca, tables, tmp_path):
    c, real, mirror = tables["set_int_edges"]
    d = str(tmp_path)
    os.makedirs(f"{d}/gpu")
    bases = [f"{d}/gpu/oa-{10 + i}-big" for i in range(3)]
    a, b = -3 * 2 ** 61, 2 ** 61
    r = ca.compact_routed(real, bases, [(MIN_TOKEN, a, 0), (a + 1, b, 1)], 2)
    assert [x["written"] for x in r["outputs"]] == [1, 1, 1]
    for i, (lo, hi) in enumerate([(MIN_TOKEN, a), (a + 1, b), (b + 1, MAX_TOKEN)]):
        want, o = _expected(c, mirror, d, f"r{i}", f"shard={lo}:{hi}")
        assert r["outputs"][i]["partitions"] == o["partitions_out"] > 0
        _assert_same(bases[i], want, c, f"routed output {i}", d)
        ca.verify(bases[i])


def test_token_range_and_keep_ranges(ca, tables, tmp_path):
    c, real, mirror = tables["mixed"]
    d = str(tmp_path)
    tokens = (-2 ** 62, 3 * 2 ** 61)
    ranges = [(-3 * 2 ** 61, -2 ** 61), (-2 ** 60, 2 ** 62)]
    os.makedirs(f"{d}/gpu")
    r = ca.compact(real, f"{d}/gpu/oa-50-big", token_range=tokens, keep_ranges=ranges)
    want, o = _expected(c, mirror, d, "t", f"shard={tokens[0]}:{tokens[1]}",
                        "ranges=" + ",".join(f"{lo}:{hi}" for lo, hi in ranges))
    assert 0 < o["partitions_out"] == r["partitions_out"] < len(c.matrix.cases)
    _assert_same(f"{d}/gpu/oa-50-big", want, c, "token range + kept ranges", d)


@pytest.mark.parametrize("cell_level", [0, 1])
def test_garbage_collection(ca, tables, tmp_path, cell_level):
    """A tombstone source with a cell tombstone at a negative key and a
    complexDeletion, ROW and CELL mode (gc_path_cmp)."""
    c, real, mirror = tables["gc"]
    d = str(tmp_path)
    os.makedirs(f"{d}/gpu")
    ca.compact(real[:2], f"{d}/gpu/oa-50-big", tombstone_sources=[real[2]],
               cell_level_gc=bool(cell_level))
    want, o = _expected(c, mirror[:2], d, "gc", f"tombsrc={mirror[2]}",
                        *(["cellgc=1"] if cell_level else []))
    assert o["partitions_out"] > 0
    _assert_same(f"{d}/gpu/oa-50-big", want, c, f"cellgc={cell_level}", d)
    ca.verify(f"{d}/gpu/oa-50-big")


@pytest.mark.parametrize("name,job", [("set_int_edges", at.Job()), ("mixed", at.Job()),
                                      ("set_int_edges", at.Job(gc_before=ct.G + 1)),
                                      ("map_bigint_text", at.Job())],
                         ids=["set_int_edges", "mixed", "set_int_edges_purging", "map_bigint_text"])
def test_validate(ca, tables, tmp_path, name, job):
    """The repair digests over the real inputs equal `oracle_tool validate` of
    the single expected output under its base types, with the job's purge
    parameters; and reduced to Merkle leaves on the device."""
    c, real, mirror = tables[name]
    d = str(tmp_path)
    want, _ = _expected(c, mirror, d, "v", *job.oracle_args())
    ct.to_base(c, want, f"{d}/wantb/oa-50-big")
    gpu, cpu = f"{d}/gpu.digests", f"{d}/cpu.digests"
    kw = dict(now_sec=job.now, gc_before=job.gc_before)
    n = ca.validate(real, gpu, **kw)
    subprocess.run([ORACLE, "validate", cpu, f"{d}/wantb/oa-50-big", *job.oracle_args()],
                   check=True, capture_output=True)
    a, b = open(gpu, "rb").read(), open(cpu, "rb").read()
    assert n * 40 == len(a) and n > 0
    assert a == b
    trees = mh.even_split(64)
    want_leaves = mh.reduce_leaves(mh.read_records(cpu), trees)
    got = ca.validate_merkle(real, trees, **kw)
    assert (list(got[0]), list(got[1]), got[2]) == (want_leaves[0], want_leaves[1], n)


@pytest.mark.parametrize("name", ["set_int_edges", "mixed"])
def test_scrub(ca, tables, tmp_path, name):
    """A clean input: everything kept, the types carried over, and the output
    reads back equal to the input."""
    c, real, _ = tables[name]
    d = str(tmp_path)
    os.makedirs(f"{d}/out")
    kept, dropped = ca.scrub(real[0], f"{d}/out/oa-81-big")
    assert (kept, dropped) == (len(c.inputs()[0]), 0)
    ca.verify(f"{d}/out/oa-81-big")
    assert _header_types(f"{d}/out/oa-81-big") == _header_types(real[0])
    ct.to_base(c, real[0], f"{d}/inb/oa-1-big")
    ct.to_base(c, f"{d}/out/oa-81-big", f"{d}/outb/oa-1-big")
    a = at.read_sstable(ORACLE, f"{d}/inb/oa-1-big", f"{d}/a.memdump")
    b = at.read_sstable(ORACLE, f"{d}/outb/oa-1-big", f"{d}/b.memdump")
    assert a.keys() == b.keys() and len(a) == kept
    for n in a:
        assert at.canonical(a[n]) == at.canonical(b[n]), c.matrix.labels[n]


def test_verify_inputs(ca, tables):
    for name, (c, real, _) in tables.items():
        for base in real:
            ca.verify(base)


@pytest.mark.parametrize("name", ["set_int_edges", "map_bigint_text", "mixed"])
def test_flush_table(ca, tables, tmp_path, name):
    """flush_table(col_types=...) of the expected content equals the expected
    sstable."""
    c, real, mirror = tables[name]
    d = str(tmp_path)
    want, _ = _expected(c, mirror, d, "f")
    ct.to_base(c, want, f"{d}/wantb/oa-50-big")
    schema, stats, parts = ct.read_dump(ORACLE, f"{d}/wantb/oa-50-big", f"{d}/want.memdump")
    md = f"{d}/flush.memdump"
    with open(md, "wb") as f:
        f.write(ct.gmd2(schema, ct.narrow_values(parts), stats))
    os.makedirs(f"{d}/gpu")
    ca.flush_table(md, f"{d}/gpu/oa-50-big", col_types=c.types)
    _assert_same(f"{d}/gpu/oa-50-big", want, c, "flush", d)
    ca.verify(f"{d}/gpu/oa-50-big")


# ---- loud failures: no output file left ---------------------------------------
SET_SCHEMA = Schema(regular_cols=((b"v", BYTES), (b"zs", MAP_BB)))


def _one_row_table(d, cells, types, schema=SET_SCHEMA, stem="oa-1-big", good=ct.i4(5)):
    """Two one-row partitions under `types`: the complex column holds one cell
    at the path `good` in the first and `cells` in the second."""
    col = len(schema.regular_cols) - 1
    c = ct.CollCase(Matrix("COLL_bad", schema, 1, [
        Case("good", [Partition(b"", items=[Row((), complex={col: (DT_LIVE, [ct.LIVE(good)])})])]),
        Case("bad", [Partition(b"", items=[Row((), complex={col: (DT_LIVE, cells)})])])]), types)
    base = f"{d}/{stem}"
    parts = c.inputs()[0]
    ct.fromdump(ORACLE, ct.gmd2(schema, parts), base)
    ct.rewrite(base, schema, c.renames(c.all_names()))
    return c, base


def _refused(ca, tmp_path, inputs, match, rc=None):
    out = str(tmp_path / "out" / "oa-50-big")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with pytest.raises(ca.GpuCompactError, match=match) as e:
        ca.compact(inputs, out)
    if rc is not None:
        assert f"rc={rc}" in str(e.value)
    assert not glob.glob(out + "*"), "an output file was created"
    return str(e.value)


def test_rejects_a_short_path_in_a_set_of_int(ca, tmp_path):
    """A 3-byte path under SetType(Int32Type) is GPUC_ERR_FORMAT, in compact,
    scrub and verify; the same bytes are a legal map<blob,blob>."""
    d = str(tmp_path)
    cells = [ct.LIVE(b"\x00\x00\x07")]
    _, base = _one_row_table(f"{d}/in", cells, {b"zs": ct.set_of(ct.INT32_T)})
    _refused(ca, tmp_path, [base], r"width of its key type", rc=2)
    with pytest.raises(ca.GpuCompactError, match=r"rc=2.*width of its key type"):
        ca.scrub(base, f"{d}/out/oa-60-big")
    with pytest.raises(ca.GpuCompactError, match=r"rc=2.*width of its key type"):
        ca.verify(base)
    assert not glob.glob(f"{d}/out/oa-60-big*")
    _, legal = _one_row_table(f"{d}/legal", cells, {})
    ca.compact([legal], f"{d}/out/oa-70-big")


def test_rejects_an_empty_path_in_a_map_of_bigint(ca, tmp_path):
    _, base = _one_row_table(f"{tmp_path}/in", [ct.LIVE(b"", b"v")],
                             {b"zs": ct.map_of(ct.LONG_T, ct.UTF8_T)}, good=ct.i8(5))
    _refused(ca, tmp_path, [base], r"width of its key type", rc=2)


def test_rejects_a_set_cell_with_a_value(ca, tmp_path):
    """A set cell without the empty-value flag is GPUC_ERR_FORMAT."""
    d = str(tmp_path)
    _, base = _one_row_table(f"{d}/in", [ct.LIVE(ct.i4(1), b"value")], {b"zs": ct.set_of(ct.INT32_T)})
    _refused(ca, tmp_path, [base], r"set column carries a value", rc=2)
    _, text = _one_row_table(f"{d}/in2", [ct.LIVE(b"k", b"value")], {b"zs": ct.set_of(ct.UTF8_T)})
    _refused(ca, tmp_path, [text], r"set column carries a value", rc=2)


def test_flush_rejects_descending_set_paths(ca, tmp_path):
    """0 before -1 is ascending as bytes and descending as ints."""
    d = str(tmp_path)
    cells = [ct.LIVE(ct.i4(0)), ct.LIVE(ct.i4(-1))]
    c, _ = _one_row_table(f"{d}/in", cells, {b"zs": ct.set_of(ct.INT32_T)})
    md = f"{d}/bad.memdump"
    with open(md, "wb") as f:
        f.write(ct.gmd2(c.schema, c.inputs()[0]))
    os.makedirs(f"{d}/gpu")
    with pytest.raises(ca.GpuCompactError, match=r"CellPath order.*'zs'"):
        ca.flush_table(md, f"{d}/gpu/oa-1-big", col_types=c.types)
    assert not glob.glob(f"{d}/gpu/oa-1-big-*")
    ca.flush_table(md, f"{d}/gpu/oa-2-big")      # a legal map<blob,blob>
    # a path of the wrong width and a set cell with a value name the column too
    for bad, match in (([ct.LIVE(b"\x01\x02\x03")], r"cell path of 3 bytes in column 'zs'"),
                       ([ct.LIVE(ct.i4(3), b"v")], r"value in set column 'zs'")):
        c2, _ = _one_row_table(f"{d}/in{len(match)}", bad, {b"zs": ct.set_of(ct.INT32_T)})
        with open(md, "wb") as f:
            f.write(ct.gmd2(c2.schema, c2.inputs()[0]))
        with pytest.raises(ca.GpuCompactError, match=match):
            ca.flush_table(md, f"{d}/gpu/oa-3-big", col_types=c2.types)
        assert not glob.glob(f"{d}/gpu/oa-3-big-*")


@pytest.mark.parametrize("t", [
    ct.M + b"ListType(" + ct.UTF8_T + b")",
    ct.map_of(ct.UTF8_T, ct.INT32_T),
    ct.map_of(ct.frozen(ct.set_of(ct.UTF8_T)), ct.BYTES_T),
], ids=["list", "fixed_width_value", "frozen_key"])
def test_rejects_collection_types(ca, tables, tmp_path, t):
    """The refused type of ONE input of a job, named in full."""
    import re
    _, good = _one_row_table(f"{tmp_path}/a", [ct.LIVE(b"k")], {b"zs": ct.set_of(ct.UTF8_T)})
    _, bad = _one_row_table(f"{tmp_path}/b", [ct.LIVE(b"k")], {b"zs": t}, stem="oa-2-big")
    _refused(ca, tmp_path, [bad], "unsupported column type " + re.escape(t.decode()))
    # next to an input that holds the column as a set: the column is named
    _refused(ca, tmp_path, [good, bad], r"column 'zs'", rc=3)


def test_rejects_a_static_set(ca, tables, tmp_path):
    import re
    c, real, _ = tables["mixed"]
    d = str(tmp_path)
    ct.copy_sstable(real[0], f"{d}/in/oa-1-big")
    t = ct.set_of(ct.UTF8_T)
    ct.rewrite(f"{d}/in/oa-1-big", c.schema, {b"s": (ct.BYTES_T, t)})
    _refused(ca, tmp_path, [f"{d}/in/oa-1-big"],
             r"unsupported static column type " + re.escape(t.decode()))
    _refused(ca, tmp_path, [f"{d}/in/oa-1-big", real[1]], r"column 's'", rc=3)


def test_rejects_two_set_types_under_one_name(ca, tmp_path):
    _, a = _one_row_table(f"{tmp_path}/a", [ct.LIVE(b"abcd")], {b"zs": ct.set_of(ct.UTF8_T)})
    _, b = _one_row_table(f"{tmp_path}/b", [ct.LIVE(ct.i4(1))], {b"zs": ct.set_of(ct.INT32_T)},
                          stem="oa-2-big")
    _refused(ca, tmp_path, [a, b], r"column 'zs' is .*SetType\(.*UTF8Type\) in one input and "
                                   r".*SetType\(.*Int32Type\) in another", rc=3)
