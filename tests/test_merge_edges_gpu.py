"""Merge, reconcile and purge edge cases on the GPU, byte for byte against the
CPU oracle: timestamp ties of every cell kind (regular, static, complex, gc
and counter copies of the tie ladder), liveness and deletion ties, range
bounds on row clusterings, and job parameters on stored values. The tables
are authored (authored_tables.py); test_merge_edges_cpu.py shows that the
oracle holds what the reference rules say on every one of these cases.

A failure names the case numbers (== partition keys) and their labels."""
import filecmp
import os
import subprocess
from dataclasses import replace

import pytest

import authored_tables as at
from conftest import ORACLE

pytestmark = pytest.mark.gpu

COMPONENTS = ["Data.db", "Index.db", "CompressionInfo.db", "Filter.db",
              "Digest.crc32", "Statistics.db", "Summary.db", "TOC.txt"]
BTI_COMPONENTS = ["Data.db", "CompressionInfo.db", "Filter.db", "Digest.crc32",
                  "Statistics.db", "Partitions.db", "Rows.db", "TOC.txt"]
MATRICES = {mk().name: mk for mk in at.ALL_MATRICES}
ALL_TOKENS = (at.NO_TS, 2 ** 63 - 1)


@pytest.fixture(scope="module")
def ca(product_lib):
    import cassandra_amd as mod
    if mod.device_count() < 1:
        pytest.skip("no GPU")
    return mod


@pytest.fixture(scope="module")
def authored(oracle_bin, tmp_path_factory):
    """Every matrix written once: name -> (matrix, input bases, tomb base, dir)."""
    root = tmp_path_factory.mktemp("authored")
    out = {}
    for name, mk in MATRICES.items():
        m = mk()
        d = str(root / name)
        bases, tbase = m.write(oracle_bin, d)
        out[name] = (m, bases, tbase, d)
    return out


def _assert_same(gpu, cpu, m, what, scratch, components=None):
    """_assert_dirs_equal, with the differing cases named."""
    components = components or (BTI_COMPONENTS if m.schema.bti else COMPONENTS)
    for c in components:
        fa, fb = f"{gpu}-{c}", f"{cpu}-{c}"
        assert os.path.exists(fa), f"{what}: missing {fa}"
        assert os.path.exists(fb), f"{what}: missing {fb}"
        if filecmp.cmp(fa, fb, shallow=False):
            continue
        try:
            named = at.differing_cases(ORACLE, gpu, cpu, m.labels, scratch)
        except Exception as e:  # the GPU output may not even parse
            named = [f"(could not read the outputs back: {e})"]
        raise AssertionError(
            f"{m.name} [{what}]: {c} differs; {len(named)} cases differ (first file is the GPU's):\n"
            + "\n".join(named[:12])
            + ("" if named else "\n(every partition reads back equal: the difference is in the encoding)"))


def _compact_both(ca, m, bases, tbase, d, tag, job, oracle_extra=(), gpu_extra=None):
    stem = "da-50-bti" if m.schema.bti else "oa-50-big"
    os.makedirs(f"{d}/gpu-{tag}"), os.makedirs(f"{d}/cpu-{tag}")
    gpu, cpu = f"{d}/gpu-{tag}/{stem}", f"{d}/cpu-{tag}/{stem}"
    kw = job.gpu_kwargs()
    kw.update(gpu_extra or {})
    if tbase:
        kw["tombstone_sources"] = [tbase]
    ca.compact(bases, gpu, **kw)
    args = job.oracle_args() + list(oracle_extra) + ([f"tombsrc={tbase}"] if tbase else [])
    subprocess.run([ORACLE, "compact", cpu, *bases, *args], check=True, capture_output=True)
    return gpu, cpu


@pytest.mark.parametrize("name", sorted(MATRICES))
def test_compaction(ca, authored, tmp_path, name):
    """Every job of the matrix: all eight components equal, and the GPU's
    output passes verify."""
    m, bases, tbase, _ = authored[name]
    for i, (jn, job) in enumerate(m.jobs):
        gpu, cpu = _compact_both(ca, m, bases, tbase, str(tmp_path), str(i), job)
        _assert_same(gpu, cpu, m, jn, str(tmp_path))
        ca.verify(gpu)


@pytest.mark.parametrize("name", ["A_i_skinny", "B_rowlevel", "C_bigint", "C_composite", "C_text"])
def test_validation(ca, authored, tmp_path, name):
    """Repair digests take the winning cell's fields."""
    m, bases, _, _ = authored[name]
    gpu, cpu = str(tmp_path / "gpu.digests"), str(tmp_path / "cpu.digests")
    n = ca.validate(bases, gpu)
    subprocess.run([ORACLE, "validate", cpu, *bases], check=True, capture_output=True)
    a, b = open(gpu, "rb").read(), open(cpu, "rb").read()
    assert n * 40 == len(a)
    if a != b:
        # digests are in token order, as the partitions of the oracle's compaction are
        out = str(tmp_path / "oa-50-big")
        subprocess.run([ORACLE, "compact", out, *bases], check=True, capture_output=True)
        subprocess.run([ORACLE, "dumpsst", out, out + ".memdump"], check=True, capture_output=True)
        order = [at.key_case(p.key) for p in at.parse_gmd2(open(out + ".memdump", "rb").read())[2]]
        rec = lambda blob: {blob[i:i + 8]: blob[i + 8:i + 40] for i in range(0, len(blob), 40)}
        ra, rb = rec(a), rec(b)
        assert len(order) == len(rb)
        bad = [f"case {n} [{m.labels[n]}]" for n, t in zip(order, sorted(rb, key=lambda t: int.from_bytes(t, "big", signed=True)))
               if ra.get(t) != rb[t]]
        extra = len(set(ra) - set(rb))
        raise AssertionError(f"{name}: {len(bad)} partition digests differ, {extra} partitions only "
                             "on the GPU:\n" + "\n".join(bad[:20]))


@pytest.mark.parametrize("name", sorted(MATRICES))
def test_flush(ca, authored, tmp_path, name):
    """flush_table of each authored memdump == the fromdump sstable."""
    m, bases, tbase, d = authored[name]
    dumps = [f"{d}/in{i + 1}.memdump" for i in range(len(bases))]
    if tbase:
        bases, dumps = bases + [tbase], dumps + [f"{d}/tomb.memdump"]
    for i, (base, dump) in enumerate(zip(bases, dumps)):
        out = str(tmp_path / f"flush{i}")
        ca.flush_table(dump, out)
        _assert_same(out, base, m, f"flush of {os.path.basename(dump)}", str(tmp_path))
        ca.verify(out)


@pytest.mark.parametrize("fmt", ["bti", "snappy"])
@pytest.mark.parametrize("name", ["A_ii_wide", "C_bigint", "C_blocks"])
def test_index_formats(ca, oracle_bin, tmp_path, name, fmt):
    """The same cases from `da` (trie-indexed) inputs and with Snappy."""
    m = MATRICES[name]()
    m.schema = replace(m.schema, **{fmt: 1})
    bases, tbase = m.write(oracle_bin, str(tmp_path / "in"))
    gpu, cpu = _compact_both(ca, m, bases, tbase, str(tmp_path), fmt, at.Job())
    _assert_same(gpu, cpu, m, fmt, str(tmp_path))
    ca.verify(gpu)


@pytest.mark.parametrize("holds_keys", [True, False], ids=["bloom-hit", "bloom-miss"])
@pytest.mark.parametrize("min_ts", [at.T, at.T + 1], ids=["min_ts=T", "min_ts=T+1"])
def test_bloom_checked_overlap(ca, authored, oracle_bin, tmp_path, min_ts, holds_keys):
    """The overlap boundary through the per-key bloom-checked evaluator: with
    the filter of a table that holds the keys, and of one that holds others."""
    m, bases, _, _ = authored["D_jobs"]
    if holds_keys:
        flt = bases[0] + "-Filter.db"
    else:
        other = [at.Partition(at.case_key(1000 + i), del_=at.DT(5, at.G)) for i in range(16)]
        (tmp_path / "other.memdump").write_bytes(at.to_gmd2(m.schema, other))
        subprocess.run([oracle_bin, "fromdump", str(tmp_path / "other.memdump"),
                        str(tmp_path / "oa-7-big")], check=True, capture_output=True)
        flt = str(tmp_path / "oa-7-big-Filter.db")
    job = at.Job(gc_before=at.G + 1)
    gpu, cpu = _compact_both(
        ca, m, bases, None, str(tmp_path), "bloom", job,
        oracle_extra=[f"ov={ALL_TOKENS[0]}:{ALL_TOKENS[1]}:{min_ts}:{flt}"],
        gpu_extra=dict(overlaps=[(*ALL_TOKENS, min_ts, flt)]))
    _assert_same(gpu, cpu, m, f"bloom overlap min_ts=T{min_ts - at.T:+d}", str(tmp_path))
    ca.verify(gpu)


def test_rejected_partition_is_a_parse_error(ca, oracle_bin, tmp_path):
    """A partition the parser rejects (a null clustering component, outside
    the engine's scope) is reported as the parse error it is. Its row count
    is never written, so nothing may be sized from the counts before the
    error is read: that used to end as an out-of-memory error."""
    s = at.Schema(ck_types=(at.LONG,))
    row = lambda ck, n: at.Row(ck, at.Live(at.T), cells={0: at.Cell(at.T, b"%d" % n)})
    parts = [at.Partition(at.case_key(n), items=[row((at.ck_long(n),), n)]) for n in range(40)]
    parts[17].items = [row((None,), 17)]
    (tmp_path / "in.memdump").write_bytes(at.to_gmd2(s, parts))
    base = str(tmp_path / "oa-1-big")
    subprocess.run([oracle_bin, "fromdump", str(tmp_path / "in.memdump"), base],
                   check=True, capture_output=True)
    with pytest.raises(ca.GpuCompactError, match="parse error code 17"):
        ca.compact([base], str(tmp_path / "oa-2-big"))
