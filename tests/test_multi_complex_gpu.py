"""Tables with several complex (map<blob,blob>) columns through the GPU
pipeline: compaction, garbage-collect, validation, verify, scrub, flush and
sharded output, each byte-for-byte against the unmodified CPU oracle. The
inputs (multi_cpx_helpers.widened) carry rows where a real complexDeletion
sits next to a live one, deletion-only columns and partly present column
sets."""
import ctypes
import json
import os
import subprocess

import pytest

import chunk_helpers as ch
from conftest import ORACLE
from multi_cpx_helpers import (CASES, assert_same_components, base_name, components,  # noqa: F401
                               widen_tool, widened)

pytestmark = pytest.mark.gpu

NOW = 2000000000


@pytest.fixture(scope="module")
def ca(product_lib):
    import cassandra_amd as mod
    if mod.device_count() < 1:
        pytest.skip("no GPU")
    return mod


def _oracle_compact(outbase, inputs, **kw):
    subprocess.run([ORACLE, "compact", outbase, *inputs, *[f"{k}={v}" for k, v in kw.items()]],
                   check=True, capture_output=True)


def _comps(case):
    return components(case) + ["TOC.txt"]


@pytest.mark.parametrize("purge", [False, True], ids=["plain", "purge"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_compaction(ca, widened, tmp_path, case, purge):
    """Three-way compaction, plain and with gc_before = now = 2000000000; the
    output also passes verify."""
    d, ins = str(tmp_path), widened[case]["bases"]
    gpu, cpu = f"{d}/{base_name(case, 60)}", f"{d}/{base_name(case, 80)}"
    if purge:
        ca.compact(ins, gpu, now_sec=NOW, gc_before=NOW)
        _oracle_compact(cpu, ins, now=NOW, gcbefore=NOW)
    else:
        ca.compact(ins, gpu)
        _oracle_compact(cpu, ins)
    assert_same_components(gpu, cpu, _comps(case))
    ca.verify(gpu)


@pytest.mark.parametrize("cell", [0, 1], ids=["row", "cell"])
def test_garbage_collect(ca, widened, tmp_path, cell):
    """Inputs 1 and 2 of case a against input 3 as the tombstone source, ROW
    and CELL mode (the per-column complex branch of removeShadowedCells)."""
    d, b = str(tmp_path), widened["a"]["bases"]
    ins, srcs = b[:2], b[2:]
    ca.compact(ins, f"{d}/oa-60-big", tombstone_sources=srcs, cell_level_gc=bool(cell))
    _oracle_compact(f"{d}/oa-80-big", ins, tombsrc=",".join(srcs), cellgc=cell)
    assert_same_components(f"{d}/oa-60-big", f"{d}/oa-80-big", _comps("a"))
    ca.verify(f"{d}/oa-60-big")


@pytest.mark.parametrize("case", ["a", "b"])
def test_validate_digests(ca, widened, tmp_path, case):
    d, ins = str(tmp_path), widened[case]["bases"]
    subprocess.run([ORACLE, "validate", f"{d}/v_cpu.bin", *ins, "now=1800000000"],
                   check=True, capture_output=True)
    n = ca.validate(ins, f"{d}/v_gpu.bin", now_sec=1800000000)
    with open(f"{d}/v_cpu.bin", "rb") as f:
        a = f.read()
    with open(f"{d}/v_gpu.bin", "rb") as f:
        b = f.read()
    assert n > 0 and n == len(a) // 40
    assert a == b, next((i for i in range(min(len(a), len(b))) if a[i] != b[i]), -1)


@pytest.mark.parametrize("case", sorted(CASES))
def test_verify_accepts_inputs(ca, widened, case):
    for b in widened[case]["bases"]:
        ca.verify(b)


def test_scrub(ca, widened, tmp_path):
    """A case-a input at 1 KiB chunks with one chunk corrupted: some
    partitions are kept, some dropped, and counts and bytes match the
    oracle's scrub."""
    d = str(tmp_path)
    base = ch.rechunk(widened["a"]["bases"][0], f"{d}/in/oa-1-big", 1024, f"{d}/tmp")
    with open(base + "-Data.db", "r+b") as f:
        f.seek(os.path.getsize(base + "-Data.db") // 2)
        b0 = f.read(1)
        f.seek(-1, 1)
        f.write(bytes([b0[0] ^ 0x10]))
    out = subprocess.run([ORACLE, "scrub", f"{d}/oa-80-big", base],
                         capture_output=True, text=True, check=True)
    ores = json.loads(out.stdout.splitlines()[-1])
    kept, dropped = ca.scrub(base, f"{d}/oa-81-big")
    assert kept > 0 and dropped > 0
    assert (kept, dropped) == (ores["partitions_kept"], ores["partitions_dropped"])
    assert_same_components(f"{d}/oa-81-big", f"{d}/oa-80-big", _comps("a"))
    ca.verify(f"{d}/oa-81-big")


@pytest.mark.parametrize("case", ["a", "c", "d"])
def test_flush_table_roundtrip(ca, widened, tmp_path, case):
    """dumpsst of a widened input, flushed through gpuc_flush_table with one
    gpuc_cpx_col per map column, is that input again."""
    d, src = str(tmp_path), widened[case]["bases"][0]
    subprocess.run([ORACLE, "dumpsst", src, f"{d}/rt.memdump"], check=True, capture_output=True)
    out = f"{d}/{base_name(case, 60)}"
    ca.flush_table(f"{d}/rt.memdump", out)
    assert_same_components(out, src, _comps(case))


def test_flush_table_refuses_bad_complex_rows(ca, widened, tmp_path):
    """Loud failures: with several map columns a row that sets has_cpx but
    gives no cpx_cols, and a column whose paths are out of CellPath order."""
    d, src = str(tmp_path), widened["a"]["bases"][0]
    subprocess.run([ORACLE, "dumpsst", src, f"{d}/rt.memdump"], check=True, capture_output=True)
    with open(f"{d}/rt.memdump", "rb") as f:
        data = f.read()

    def rows(parts, n):
        for pi in range(n):
            for ui in range(parts[pi].n_unf):
                u = parts[pi].unf[ui]
                if u.kind == 4 and u.has_cpx:
                    yield u

    S, parts, n, bufs = ca._parse_memdump(data)
    assert S.n_cpx == 3
    u = next(rows(parts, n))
    u.cpx_cols = ctypes.POINTER(ca.GpucCpxCol)()
    with pytest.raises(ca.GpuCompactError, match="cpx_cols"):
        ca._flush_table_parsed(S, parts, n, f"{d}/bad1")
    del bufs

    S, parts, n, bufs = ca._parse_memdump(data)
    col = next(u.cpx_cols[x] for u in rows(parts, n) for x in range(1, 3)
               if u.cpx_cols[x].present and u.cpx_cols[x].n_cells >= 2)
    c0, c1 = bytes(col.cells[0]), bytes(col.cells[1])
    ctypes.memmove(ctypes.byref(col.cells[0]), c1, len(c1))
    ctypes.memmove(ctypes.byref(col.cells[1]), c0, len(c0))
    with pytest.raises(ca.GpuCompactError, match="CellPath order"):
        ca._flush_table_parsed(S, parts, n, f"{d}/bad2")
    del bufs


def test_sharded_output(ca, widened, tmp_path):
    """n_output_shards=2 on case a against the oracle's shard=lo:hi outputs."""
    from cassandra_amd.sharding import split_token_range
    d, ins, S = str(tmp_path), widened["a"]["bases"], 2
    ca.compact(ins, f"{d}/oa-200-big", n_output_shards=S)
    for i in range(S):
        lo, hi = split_token_range(S, i)
        _oracle_compact(f"{d}/oa-{300 + i}-big", ins, shard=f"{lo}:{hi}")
        assert_same_components(f"{d}/oa-{200 + i}-big", f"{d}/oa-{300 + i}-big", _comps("a"))
