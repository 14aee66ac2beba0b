"""Compaction of inputs whose serialization headers list different columns.

The reference of every positive case is the oracle's compaction of the WIDE
twins (every input rewritten under the union header, header_union_tables.py)
with the same job arguments; the engine compacts the NARROW inputs and must
give the same bytes in every component. test_header_union_cpu.py shows that
the twins hold the same tables and that the oracle's output is sound."""
import glob
import json
import os
import subprocess

import pytest

import authored_tables as at
import chunk_helpers as ch
import header_union_tables as hu
from conftest import ORACLE
from multi_cpx_helpers import BTI_COMPONENTS, COMPONENTS, assert_same_components
from size_split_helpers import cut_ranges, size_split_tool  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

PURGING = at.Job(now=hu.PURGE_NOW, gc_before=hu.PURGE_NOW)
UNSUPPORTED = r"rc=3\b"


@pytest.fixture(scope="module")
def ca(product_lib):
    import cassandra_amd as mod
    if mod.device_count() < 1:
        pytest.skip("no GPU")
    return mod


@pytest.fixture(scope="module")
def twins(oracle_bin, tmp_path_factory):
    """case -> (UnionCase, narrow bases, wide bases), written once."""
    root = tmp_path_factory.mktemp("header_union_gpu")
    cases = dict(hu.ALL_CASES, GC=hu.gc_case, U1da=lambda: hu.u1(bti=1, snappy=1))
    out = {}
    for name, mk in cases.items():
        uc = mk()
        narrow, wide, _ = uc.write(oracle_bin, str(root / name))
        out[name] = (uc, narrow, wide)
    return out


def _oracle_compact(out, inputs, *args):
    os.makedirs(os.path.dirname(out), exist_ok=True)
    r = subprocess.run([ORACLE, "compact", out, *inputs, *args], check=True, capture_output=True,
                       text=True)
    return json.loads(r.stdout.splitlines()[-1])


def _assert_same(got, want, uc, what, scratch):
    comps = BTI_COMPONENTS if uc.matrix.schema.bti else COMPONENTS
    try:
        assert_same_components(got, want, comps)
    except AssertionError as e:
        try:
            named = at.differing_cases(ORACLE, got, want, uc.matrix.labels, scratch)
        except Exception as e2:  # the engine's output may not even parse
            named = [f"(could not read the outputs back: {e2})"]
        raise AssertionError(
            f"{uc.name} [{what}]: {e}; {len(named)} cases differ (first file is the engine's):\n"
            + "\n".join(named[:12])
            + ("" if named else "\n(every partition reads back equal: the difference is in the encoding)"))


def _stem(uc, gen):
    return f"da-{gen}-bti" if uc.matrix.schema.bti else f"oa-{gen}-big"


def _compact_both(ca, uc, narrow, wide, d, job, what):
    gpu, cpu = f"{d}/gpu/{_stem(uc, 50)}", f"{d}/cpu/{_stem(uc, 50)}"
    os.makedirs(f"{d}/gpu")
    r = ca.compact(narrow, gpu, **job.gpu_kwargs())
    o = _oracle_compact(cpu, wide, *job.oracle_args())
    _assert_same(gpu, cpu, uc, what, d)
    assert r["partitions_out"] == o["partitions_out"] and r["rows_out"] == o["rows_out"]
    ca.verify(gpu)
    return gpu


@pytest.mark.parametrize("name", sorted(hu.ALL_CASES))
def test_plain(ca, twins, tmp_path, name):
    uc, narrow, wide = twins[name]
    _compact_both(ca, uc, narrow, wide, str(tmp_path), at.Job(), "plain")


@pytest.mark.parametrize("name", ["U1", "U4", "U8"])
def test_purging(ca, twins, tmp_path, name):
    uc, narrow, wide = twins[name]
    _compact_both(ca, uc, narrow, wide, str(tmp_path), PURGING, "purging")


def test_da_snappy(ca, twins, tmp_path):
    uc, narrow, wide = twins["U1da"]
    assert os.path.exists(narrow[0] + "-Partitions.db") and os.path.exists(wide[0] + "-Rows.db")
    _compact_both(ca, uc, narrow, wide, str(tmp_path), at.Job(), "da + Snappy")


def test_identity(ca, twins, tmp_path):
    """Inputs that all carry the union header give the same bytes as the
    narrow ones (and go through identity maps)."""
    uc, narrow, wide = twins["U1"]
    d = str(tmp_path)
    os.makedirs(f"{d}/n"), os.makedirs(f"{d}/w")
    ca.compact(narrow, f"{d}/n/oa-50-big")
    ca.compact(wide, f"{d}/w/oa-50-big")
    _assert_same(f"{d}/w/oa-50-big", f"{d}/n/oa-50-big", uc, "wide against narrow", d)


def test_output_shards(ca, twins, tmp_path):
    from cassandra_amd.sharding import split_token_range
    uc, narrow, wide = twins["U8"]
    d = str(tmp_path)
    os.makedirs(f"{d}/gpu")
    r = ca.compact(narrow, f"{d}/gpu/oa-200-big", n_output_shards=2)
    assert r["n_outputs"] >= 2
    for i in range(2):
        lo, hi = split_token_range(2, i)
        o = _oracle_compact(f"{d}/cpu/oa-{300 + i}-big", wide, f"shard={lo}:{hi}")
        assert o["partitions_out"] > 0
        _assert_same(f"{d}/gpu/oa-{200 + i}-big", f"{d}/cpu/oa-{300 + i}-big", uc, f"shard {i}", d)


def test_max_output_bytes(ca, twins, size_split_tool, tmp_path):  # noqa: F811
    """Cut at an on-disk size: every output equals the oracle's sstable of
    its token range over the wide twins (1 KiB chunks, so that the small
    table is cut at all)."""
    uc, narrow, wide = twins["U8"]
    d = str(tmp_path)
    cap = 6000
    nin = [ch.rechunk(b, f"{d}/n/" + os.path.basename(b), 1024, f"{d}/tmpn") for b in narrow]
    win = [ch.rechunk(b, f"{d}/w/" + os.path.basename(b), 1024, f"{d}/tmpw") for b in wide]
    whole = _oracle_compact(f"{d}/cpu/oa-900-big", win)
    want = cut_ranges(size_split_tool, f"{d}/cpu/oa-900-big", cap)
    os.makedirs(f"{d}/gpu")
    r = ca.compact(nin, f"{d}/gpu/oa-500-big", max_output_bytes=cap)
    print("outputs", r["n_outputs"], "want", len(want))
    assert r["n_outputs"] >= 2 and r["n_outputs"] == len(want)
    assert r["partitions_out"] == whole["partitions_out"]
    for k, o in enumerate(want):
        _oracle_compact(f"{d}/cpu/oa-{1000 + k}-big", win, f"shard={o['first_token']}:{o['last_token']}")
        _assert_same(f"{d}/gpu/oa-{500 + k}-big", f"{d}/cpu/oa-{1000 + k}-big", uc, f"output {k}", d)
    assert not glob.glob(f"{d}/gpu/oa-{500 + len(want)}-big-*")


def test_token_range_and_keep_ranges(ca, twins, tmp_path):
    uc, narrow, wide = twins["U8"]
    d = str(tmp_path)
    tokens = (-2 ** 62, 3 * 2 ** 61)
    ranges = [(-3 * 2 ** 61, -2 ** 61), (-2 ** 60, 2 ** 62)]
    os.makedirs(f"{d}/gpu")
    r = ca.compact(narrow, f"{d}/gpu/oa-50-big", token_range=tokens, keep_ranges=ranges)
    o = _oracle_compact(f"{d}/cpu/oa-50-big", wide, f"shard={tokens[0]}:{tokens[1]}",
                        "ranges=" + ",".join(f"{lo}:{hi}" for lo, hi in ranges))
    assert 0 < o["partitions_out"] == r["partitions_out"]
    _assert_same(f"{d}/gpu/oa-50-big", f"{d}/cpu/oa-50-big", uc, "token range + kept ranges", d)


@pytest.mark.parametrize("cell_level", [0, 1])
def test_garbage_collection(ca, twins, tmp_path, cell_level):
    """Data inputs {a,b} and {a}; the tombstone source's header holds b alone
    and is mapped into the union by name."""
    uc, narrow, wide = twins["GC"]
    d = str(tmp_path)
    os.makedirs(f"{d}/gpu")
    ca.compact(narrow[:2], f"{d}/gpu/oa-50-big", tombstone_sources=[narrow[2]],
               cell_level_gc=bool(cell_level))
    _oracle_compact(f"{d}/cpu/oa-50-big", wide[:2], f"tombsrc={wide[2]}",
                    *(["cellgc=1"] if cell_level else []))
    _assert_same(f"{d}/gpu/oa-50-big", f"{d}/cpu/oa-50-big", uc, f"cellgc={cell_level}", d)
    ca.verify(f"{d}/gpu/oa-50-big")


def test_validate(ca, twins, tmp_path):
    """Repair digests over the union header."""
    uc, narrow, wide = twins["U1"]
    gpu, cpu = str(tmp_path / "gpu.digests"), str(tmp_path / "cpu.digests")
    n = ca.validate(narrow, gpu)
    subprocess.run([ORACLE, "validate", cpu, *wide], check=True, capture_output=True)
    a, b = open(gpu, "rb").read(), open(cpu, "rb").read()
    assert n * 40 == len(a) and n > 0
    assert a == b


def test_scrub_and_verify_single_narrow_input(ca, twins, tmp_path):
    """The single-source path on a header that is not the first of anything:
    U4's {zm1,zm2} input, which has no simple column."""
    uc, narrow, _ = twins["U4"]
    d = str(tmp_path)
    base = narrow[1]
    ca.verify(base)
    out = subprocess.run([ORACLE, "scrub", f"{d}/oa-80-big", base], capture_output=True, text=True,
                         check=True)
    ores = json.loads(out.stdout.splitlines()[-1])
    kept, dropped = ca.scrub(base, f"{d}/oa-81-big")
    assert kept > 0
    assert (kept, dropped) == (ores["partitions_kept"], ores["partitions_dropped"])
    assert_same_components(f"{d}/oa-81-big", f"{d}/oa-80-big", COMPONENTS)
    ca.verify(f"{d}/oa-81-big")


# ---- rejections: GPUC_ERR_UNSUPPORTED, the column named, no output ----------
def _table(oracle, d, gen, schema, parts):
    os.makedirs(d, exist_ok=True)
    base = f"{d}/oa-{gen}-big"
    hu._fromdump(oracle, schema, parts, f"{d}/in{gen}.memdump", base)
    return base


def _rejected(ca, tmp_path, inputs, match, **kw):
    out = str(tmp_path / "out" / "oa-50-big")
    os.makedirs(os.path.dirname(out))
    with pytest.raises(ca.GpuCompactError, match=match) as e:
        ca.compact(inputs, out, **kw)
    assert "rc=3" in str(e.value)
    assert not glob.glob(out + "*"), "an output file was created"


def test_rejects_a_column_of_two_types(ca, oracle_bin, tmp_path):
    d = str(tmp_path)
    row = lambda cells: [at.Partition(at.case_key(1), items=[at.Row(hu.K(1), cells=cells)])]
    s1 = at.Schema(ck_types=(at.LONG,), regular_cols=((b"a", at.BYTES), (b"b", at.LONG)))
    s2 = at.Schema(ck_types=(at.LONG,), regular_cols=((b"b", at.BYTES),))
    ins = [_table(oracle_bin, d, 1, s1, row({0: at.Cell(at.T, b"x"), 1: at.Cell(at.T, hu.lng(1))})),
           _table(oracle_bin, d, 2, s2, row({0: at.Cell(at.T, b"y")}))]
    _rejected(ca, tmp_path, ins, r"column 'b'")


def test_rejects_differing_clustering_types(ca, oracle_bin, tmp_path):
    d = str(tmp_path)
    s1 = at.Schema(ck_types=(at.LONG,), regular_cols=((b"a", at.BYTES), (b"b", at.BYTES)))
    s2 = at.Schema(ck_types=(at.UTF8,), regular_cols=((b"a", at.BYTES),))
    ins = [_table(oracle_bin, d, 1, s1, [at.Partition(at.case_key(1), items=[
               at.Row(hu.K(1), cells={0: at.Cell(at.T, b"x")})])]),
           _table(oracle_bin, d, 2, s2, [at.Partition(at.case_key(1), items=[
               at.Row((b"k",), cells={0: at.Cell(at.T, b"y")})])])]
    _rejected(ca, tmp_path, ins, r"clustering types")


def test_rejects_a_tombstone_source_column_outside_the_union(ca, oracle_bin, tmp_path):
    d = str(tmp_path)
    row = lambda cells: [at.Partition(at.case_key(1), items=[at.Row(hu.K(1), cells=cells)])]
    s1 = at.Schema(ck_types=(at.LONG,), regular_cols=((b"a", at.BYTES),))
    s2 = at.Schema(ck_types=(at.LONG,), regular_cols=((b"a", at.BYTES), (b"b", at.BYTES)))
    data = _table(oracle_bin, d, 1, s1, row({0: at.Cell(at.T, b"x")}))
    tomb = _table(oracle_bin, d, 2, s2, row({1: at.Cell(at.T, b"", at.L)}))
    _rejected(ca, tmp_path, [data], r"tombstone source.*column 'b'", tombstone_sources=[tomb])
