"""Descending clustering columns: the host-side resolution and the soundness
of the reference route of test_desc_clustering_gpu.py (desc_tables.py).
Everything here runs without a GPU."""
import itertools
import json
import os
import subprocess

import pytest

import authored_tables as at
import desc_tables as dt
from conftest import REPO
from multi_cpx_helpers import COMPONENTS, assert_same_components

ALL8 = COMPONENTS + ["TOC.txt"]

NATIVE = os.path.join(REPO, "tests", "native", "desc_schema_test.cpp")
# the cases whose mirrors are compacted here (blocks and many are the large ones)
ROUTE_CASES = ["bigint", "composite_ad", "composite_da", "text", "edges_int", "edges_bigint",
               "blocks", "timestamp", "purge"]


@pytest.fixture(scope="module")
def native(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("desc_native") / "desc_schema_test")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra",
                    "-fsanitize=address,undefined", NATIVE, "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def tables(oracle_bin, tmp_path_factory):
    """case -> (DescCase, real bases, mirror bases), written once."""
    root = tmp_path_factory.mktemp("desc_cpu")
    out = {}
    for name, mk in dt.ALL_CASES.items():
        dc = mk()
        real, mirror = dc.write(oracle_bin, str(root / name))
        out[name] = (dc, real, mirror)
    return out


def test_resolve_schema_native(native):
    """The 12 accepted clustering strings with width and flag, TimestampType
    as a regular and static type, every refusal with its type string, and the
    ascending + descending job."""
    r = subprocess.run([native], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "desc_schema_test OK" in r.stdout


@pytest.mark.parametrize("name", sorted(dt.ALL_CASES))
def test_statistics_rewrite_round_trip(tables, native, name):
    """To the real types and back restores the original bytes; the engine's
    host parser reads the rewritten file and yields the real strings."""
    dc, real, mirror = tables[name]
    ds = dc.ds
    want_ck = [s.decode() for s in ds.ck_strings()]
    assert any("ReversedType(" in s for s in want_ck)
    for base in real:
        data = open(base + "-Statistics.db", "rb").read()
        hdr_ck, stats_ck, cols = dt.statistics_types(data)
        assert hdr_ck == stats_ck == ds.ck_strings()
        for nm in ds.timestamp_cols:
            assert cols[nm] == dt.TIMESTAMP
        back = dt.rewrite_statistics(data, ds.ck_strings(), ds.base_ck_strings(),
                                     ds.col_strings(to_real=False))
        again = dt.rewrite_statistics(back, ds.base_ck_strings(), ds.ck_strings(),
                                      ds.col_strings())
        assert again == data
        # `back` is what fromdump wrote: the same table under the base types
        assert dt.statistics_types(back)[0] == ds.base_ck_strings()
        assert dt.join_statistics(dt.split_statistics(back)) == back
        r = subprocess.run([native, base + "-Statistics.db"], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        lines = r.stdout.split()
        mask = sum(1 << i for i, d in enumerate(ds.desc) if d)
        assert lines == want_ck + [f"desc_mask={mask}"]


def test_rewrite_restores_fromdump_bytes(tables, oracle_bin, tmp_path):
    """The rewrite back to the base types gives exactly the file fromdump
    wrote (so nothing but the type strings, offsets and checksums moved)."""
    dc, real, _ = tables["timestamp"]
    d = str(tmp_path)
    parts = dc.real_inputs()[0]
    base = f"{d}/oa-1-big"
    dt._fromdump(oracle_bin, at.to_gmd2(dc.ds.base, parts), base + ".memdump", base)
    dt.to_base(dc.ds, real[0], f"{d}/oa-2-big")
    assert open(base + "-Statistics.db", "rb").read() == open(f"{d}/oa-2-big-Statistics.db", "rb").read()


def test_uvint_round_trip():
    for v in [0, 1, 127, 128, 16383, 16384, 2 ** 21, 2 ** 35 + 5, 2 ** 56 - 1, 2 ** 56, 2 ** 64 - 1]:
        b = dt._uvint_put(v)
        assert dt._uvint_get(b + b"\x55", 0) == (v, len(b))


@pytest.mark.parametrize("name", sorted(dt.ALL_CASES))
def test_mirror_reverses_order(name):
    """For every pair of clustering prefixes of the table, the oracle's
    comparison of the mirrors equals the descending comparison of the
    originals (component-wise negation, kinds untouched)."""
    dc = dt.ALL_CASES[name]()
    ds = dc.ds
    mirrors = dt.all_prefixes(dc.mirror_inputs())
    if len(mirrors) > 60:          # the large tables: a fixed sample of pairs
        import random
        mirrors = random.Random(7).sample(mirrors, 60)
    int32 = at.INT32 in ds.mirror.ck_types
    n = 0
    for (ka, a), (kb, b) in itertools.product(mirrors, repeat=2):
        ra, rb = dt.unmirror_ck(ds, a), dt.unmirror_ck(ds, b)
        assert dt.mirror_ck(ds, ra) == a
        want = dt.desc_compare_prefix(ds, ka, ra, kb, rb)
        if not int32:       # authored_tables orders INT32 bytes unsigned
            assert at.compare_prefix(ds.mirror.ck_types, ka, a, kb, b) == want, (ka, ra, kb, rb)
        assert dt.mirror_compare_prefix(ds, ka, a, kb, b) == want, (ka, ra, kb, rb)
        n += 1
    assert n >= 4


def test_mirror_of_prefix_pairs_and_edges():
    assert dt.mv(b"ab") < dt.mv(b"a") < dt.mv(b"") and dt.mv(b"b") < dt.mv(b"ab")
    assert dt.mv(b"12345678b") < dt.mv(b"12345678ab") < dt.mv(b"12345678a") < dt.mv(b"12345678")
    assert dt.m8(2 ** 63 - 1) == at.ck_long(-2 ** 63) and dt.m8(-2 ** 63) == at.ck_long(2 ** 63 - 1)
    with pytest.raises(AssertionError):
        dt.mv(b"a\0")


def test_real_tables_are_in_descending_order(tables):
    """The engine's inputs are legal streams under the real comparator."""
    for name, (dc, _, _) in tables.items():
        for parts in dc.real_inputs():
            for p in parts:
                for x, y in zip(p.items, p.items[1:]):
                    assert dt.desc_compare_prefix(dc.ds, at._item_kind(x), x.ck,
                                                  at._item_kind(y), y.ck) < 0, (name, x, y)


def _compact(oracle, out, inputs, *args):
    os.makedirs(os.path.dirname(out), exist_ok=True)
    r = subprocess.run([oracle, "compact", out, *inputs, *args], check=True, capture_output=True,
                       text=True)
    return json.loads(r.stdout.splitlines()[-1])


@pytest.mark.parametrize("name", ROUTE_CASES)
def test_fromdump_of_dumpsst_reproduces_the_oracle_output(tables, oracle_bin, tmp_path, name):
    """fromdump(dumpsst(O)) == O in all eight components, for the oracle's
    compaction O of the mirrors under every job of the case: the route that
    carries the expected bytes back adds nothing of its own."""
    dc, _, mirror = tables[name]
    d = str(tmp_path)
    n_data = dc.matrix.n_inputs
    for j, (label, job) in enumerate(dc.matrix.jobs):
        out = f"{d}/o{j}/oa-50-big"
        args = list(job.oracle_args())
        if dc.matrix.has_tomb_source:
            args.append(f"tombsrc={mirror[n_data]}")
        res = _compact(oracle_bin, out, mirror[:n_data], *args)
        if not res["partitions_out"]:
            continue
        md = f"{d}/o{j}/dump.memdump"
        subprocess.run([oracle_bin, "dumpsst", out, md], check=True, capture_output=True)
        schema, stats, parts = at.parse_gmd2(open(md, "rb").read())
        back = f"{d}/b{j}/oa-50-big"
        dt._fromdump(oracle_bin, dt.gmd2_with_stats(schema, parts, stats), back + ".memdump", back)
        assert_same_components(back, out, ALL8)


@pytest.mark.parametrize("name", ["bigint", "composite_da", "text", "blocks"])
def test_oracle_keeps_a_descending_single_input(tables, oracle_bin, tmp_path, name):
    """The oracle compacts ONE input whose rows are in descending order under
    an ascending header to the identical bytes, so `oracle_tool validate` of
    an expected output under base types is a reference for the digests."""
    dc, real, _ = tables[name]
    d = str(tmp_path)
    os.makedirs(f"{d}/in")
    dt.to_base(dc.ds, real[0], f"{d}/in/oa-1-big")
    _compact(oracle_bin, f"{d}/out/oa-50-big", [f"{d}/in/oa-1-big"])
    assert_same_components(f"{d}/out/oa-50-big", f"{d}/in/oa-1-big", ALL8)
