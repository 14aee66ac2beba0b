"""CPU test of the host-only output component builders (cassandra_amd/csrc/
sstable_out.h): from what sstable_meta.h parses out of an oracle-written
sstable they must regenerate the oracle's own CompressionInfo.db, Digest.crc32,
Summary.db, Filter.db and TOC.txt, and from an `oa` Index.db the `da`
Partitions.db and Rows.db of the same table. The checks themselves are in
tests/native/sstable_out_test.cpp, built here with plain g++ (no HIP)."""
import os
import subprocess

import chunk_helpers as ch
from conftest import ORACLE, REPO

SRC = os.path.join(REPO, "tests", "native", "sstable_out_test.cpp")

ONE = ["rows=1"]                                   # one partition, one Summary entry
SIMPLE = ["rows=300", "vlen=200", "tomb=10"]       # three Summary entries at interval 128
# partitions of ~120 KB against a 64 KiB column_index_size: promoted-index
# blocks in Index.db, row-index blocks in Rows.db
WIDE = ["rows=6", "crows=400", "vlen=300", "rtomb=20"]


def _gen(d, seed, spec, *extra):
    os.makedirs(d)
    subprocess.run([ORACLE, "gen", d, f"seed={seed}", "n=1", *spec, *extra],
                   check=True, capture_output=True)
    return f"{d}/da-1-bti" if "bti=1" in extra else f"{d}/oa-1-big"


def test_sstable_out(oracle_bin, tmp_path):
    d = str(tmp_path)
    args = [_gen(f"{d}/one", 71, ONE)]
    simple = _gen(f"{d}/simple", 72, SIMPLE)
    args.append(_gen(f"{d}/simple_snappy", 72, SIMPLE, "snappy=1"))
    for cl in (1024, 65536):
        out = ch.rechunk(simple, f"{d}/c{cl}/oa-1-big", cl, f"{d}/tmp{cl}")
        assert ch.chunk_length_of(out) == cl
        args.append(out)
    # the same seed as `oa` and as `da`
    args.append("bti=" + simple + "," + _gen(f"{d}/simple_da", 72, SIMPLE, "bti=1"))
    args.append("wide=bti=" + _gen(f"{d}/wide", 73, WIDE) + "," +
                _gen(f"{d}/wide_da", 73, WIDE, "bti=1"))

    binp = str(tmp_path / "sstable_out_test")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-pthread", "-o", binp, SRC],
                   check=True)
    r = subprocess.run([binp, *args], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.splitlines()[-1].startswith("OK"), r.stdout
    assert "over 4 tables and 2 oa/da pairs" in r.stdout, r.stdout
    assert f"{d}/one/oa-1-big: 1 partitions" in r.stdout, r.stdout
    assert f"{simple}: 300 partitions" in r.stdout, r.stdout
