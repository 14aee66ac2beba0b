"""The four run modes of one compaction engine (written sstables, digest file,
Merkle leaves, routed outputs) used one after another in one process, a mode
call that fails half way, and a cancellation through the sharded driver.

One tiny oracle-generated table serves all three tests: 2 sstables of 300
partitions with short values, 30% key overlap, row tombstones and partition
deletions, compacted with a gc_before that purges some partitions entirely.
That is the smallest shape at which every mode still has partitions to merge
and to purge. The references are the oracle's `compact` and `validate` of the
same inputs, written once by the fixture and never modified."""
import ctypes
import glob
import os
import shutil
import subprocess

import pytest

import merkle_helpers as mh
from cassandra_amd.sharding import split_token_range
from conftest import ORACLE
from multi_cpx_helpers import COMPONENTS, assert_same_components
from route_helpers import gen, oracle_compact, route_and_check

pytestmark = pytest.mark.gpu

NOW = 1900000000
JOB = dict(now_sec=NOW, gc_before=NOW)
OARGS = [f"now={NOW}", f"gcbefore={NOW}"]
COMPS = COMPONENTS + ["TOC.txt"]
CANCELLED = 7


@pytest.fixture(scope="module")
def ca(product_lib):
    import cassandra_amd as mod
    if mod.device_count() < 1:
        pytest.skip("no GPU")
    return mod


@pytest.fixture(scope="module")
def table(oracle_bin, tmp_path_factory):
    d = str(tmp_path_factory.mktemp("modes"))
    ins = gen(f"{d}/in", "seed=171 n=2 rows=300 vlen=60 overlap=30 tomb=15 pdel=3")
    unpurged = oracle_compact(f"{d}/ref/oa-80-big", ins)
    whole = oracle_compact(f"{d}/ref/oa-90-big", ins, *OARGS)
    assert 0 < whole["partitions_out"] < unpurged["partitions_out"] < 600  # merged and purged
    vfile = f"{d}/ref/v_cpu.bin"
    subprocess.run([ORACLE, "validate", vfile, *ins, *OARGS], check=True, capture_output=True)
    records = mh.read_records(vfile)
    assert len(records) == whole["partitions_out"]
    return dict(ins=ins, whole=f"{d}/ref/oa-90-big", vfile=vfile, records=records,
                parts=whole["partitions_out"])


def _compact_is_oracles(ca, table, out, **kw):
    r = ca.compact(table["ins"], out, **JOB, **kw)
    assert r["partitions_out"] == table["parts"] and r["n_outputs"] == 1
    assert_same_components(out, table["whole"], COMPS)


def _digest_is_oracles(ca, table, out):
    assert ca.validate(table["ins"], out, **JOB) == table["parts"]
    assert open(out, "rb").read() == open(table["vfile"], "rb").read()
    assert not glob.glob(os.path.dirname(out) + "/*-Data.db")  # a digest, not an sstable


def test_modes_do_not_leak(ca, table, tmp_path):
    """validate, compact, Merkle, routed, compact, validate on one thread:
    every call produces what its own mode produces and nothing of the mode
    that ran before it."""
    d = str(tmp_path)
    T = [t for t, _ in table["records"]]
    os.makedirs(f"{d}/v1"), os.makedirs(f"{d}/v2")

    _digest_is_oracles(ca, table, f"{d}/v1/v.bin")
    _compact_is_oracles(ca, table, f"{d}/oa-91-big")

    # two trees with a gap between them, one empty leaf, one leaf of one partition
    assert all(x < y for x, y in zip(T, T[1:])) and T[42] > T[41] + 1
    trees = [(T[10], [T[40], T[41], T[41] + 1, T[200]]), (T[250], [T[-1], mh.INT64_MAX])]
    want = mh.reduce_leaves(mh.read_records(f"{d}/v1/v.bin"), trees)
    assert want[1] == [30, 1, 0, 159, len(T) - 251, 0]
    assert ca.validate_merkle(table["ins"], trees, **JOB) == want

    a, b = len(T) // 3, 2 * len(T) // 3
    ranges = [(T[5], T[a], 0), (T[a + 1], T[a + 1], 1), (T[b], mh.INT64_MAX, 1)]
    r, parts = route_and_check(ca, table["ins"], f"{d}/routed", ranges, 2, 3,
                               oracle_args=OARGS, **JOB)
    assert min(parts) > 0 and sum(parts) == table["parts"] and r["n_outputs"] == 3

    _compact_is_oracles(ca, table, f"{d}/oa-92-big")
    _digest_is_oracles(ca, table, f"{d}/v2/v.bin")
    # and neither later call wrote into an earlier call's place
    assert sorted(os.listdir(f"{d}/routed/gpu")) == sorted(
        f"oa-{g}-big-{c}" for g in (10, 11, 12) for c in COMPS)


def test_failed_mode_call_leaves_nothing_behind(ca, table, tmp_path):
    """gpuc_validate fails on a corrupt chunk; the plain compaction after it
    writes the oracle's sstable and no digest file."""
    d = str(tmp_path)
    os.makedirs(f"{d}/bad")
    for f in glob.glob(os.path.dirname(table["ins"][0]) + "/oa-*"):
        shutil.copy(f, f"{d}/bad")
    bad = [f"{d}/bad/" + os.path.basename(b) for b in table["ins"]]
    data = bad[0] + "-Data.db"
    with open(data, "r+b") as f:
        f.seek(os.path.getsize(data) // 3)
        b0 = f.read(1)
        f.seek(-1, 1)
        f.write(bytes([b0[0] ^ 0x40]))
    digest = f"{d}/v.bin"
    with pytest.raises(ca.GpuCompactError, match="gpuc_validate rc="):
        ca.validate(bad, digest, **JOB)
    assert not os.path.exists(digest)
    _compact_is_oracles(ca, table, f"{d}/oa-91-big")
    assert not os.path.exists(digest)
    assert sorted(os.listdir(d)) == sorted(["bad"] + [f"oa-91-big-{c}" for c in COMPS])


def test_cancel_through_sharded_driver(ca, table, tmp_path):
    """A set cancel_flag fails a sharded run with GPUC_ERR_CANCELLED, whichever
    worker thread meets it; cleared, the two shards match the oracle."""
    d = str(tmp_path)
    flag = ctypes.c_int32(1)
    with pytest.raises(ca.GpuCompactError, match=rf"rc={CANCELLED}\b.*cancel"):
        ca.compact(table["ins"], f"{d}/oa-100-big", n_output_shards=2,
                   cancel_flag=ctypes.pointer(flag), **JOB)
    flag.value = 0
    r = ca.compact(table["ins"], f"{d}/oa-200-big", n_output_shards=2,
                   cancel_flag=ctypes.pointer(flag), **JOB)
    assert r["n_outputs"] == 2 and r["partitions_out"] == table["parts"]
    for i in range(2):
        lo, hi = split_token_range(2, i)
        w = oracle_compact(f"{d}/cpu/oa-{300 + i}-big", table["ins"], *OARGS, f"shard={lo}:{hi}")
        assert w["partitions_out"] > 0
        assert_same_components(f"{d}/oa-{200 + i}-big", f"{d}/cpu/oa-{300 + i}-big", COMPS)
