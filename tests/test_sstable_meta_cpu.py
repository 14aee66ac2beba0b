"""CPU test of the host-only input metadata code (cassandra_amd/csrc/
sstable_meta.h): CompressionInfo.db / Statistics.db / Index.db parsing, chunk
framing with its validation, partition windows and schema resolution, on
oracle-written sstables and on damaged copies. The checks themselves are in
tests/native/sstable_meta_test.cpp, built here with plain g++ (no HIP)."""
import glob
import os
import subprocess

import chunk_helpers as ch
from conftest import GOLDEN, ORACLE, REPO

SRC = os.path.join(REPO, "tests", "native", "sstable_meta_test.cpp")

# oracle generator arguments -> the widths resolve_schema must give:
# blob values are variable (-1), the generator's clustering column is a
# LongType (8), its static column a blob
SCHEMAS = {
    "simple": (["rows=300", "vlen=200", "tomb=10"],
               "cols=-1;ck=;st=;cpx=0;ctr=0"),
    "clust": (["rows=40", "crows=8", "vlen=120", "ncols=3", "statics=50", "rtomb=20"],
              "cols=-1,-1,-1;ck=8;st=-1;cpx=0;ctr=0"),
    "counter": (["rows=300", "counter=1", "tomb=10"],
                "cols=-1;ck=;st=;cpx=0;ctr=1"),
}


def test_sstable_meta(oracle_bin, tmp_path):
    d = str(tmp_path)
    args = []
    for i, (tag, (spec, want)) in enumerate(SCHEMAS.items()):
        for comp in ("lz4", "snappy"):
            gd = f"{d}/{tag}_{comp}"
            os.makedirs(gd)
            subprocess.run([ORACLE, "gen", gd, f"seed={61 + i}", "n=1", *spec,
                            *(["snappy=1"] if comp == "snappy" else [])],
                           check=True, capture_output=True)
            base = f"{gd}/oa-1-big"
            assert ch.chunk_length_of(base) == 16384
            args.append(f"{base}@{want}")
            if comp == "lz4":
                # 1 KiB first: its many chunks carry the damaged-table cases
                for cl in (1024, 65536):
                    out = ch.rechunk(base, f"{gd}/c{cl}/oa-1-big", cl, f"{gd}/tmp{cl}")
                    assert ch.chunk_length_of(out) == cl
                    args.insert(0, f"{out}@{want}")
    goldens = sorted(glob.glob(os.path.join(GOLDEN, "legacy_oa_*", "*-Data.db")))
    assert len(goldens) >= 4
    args += ["golden=" + g[:-len("-Data.db")] for g in goldens]

    binp = str(tmp_path / "sstable_meta_test")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-o", binp, SRC],
                   check=True)
    r = subprocess.run([binp, *args], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.splitlines()[-1].startswith("OK"), r.stdout
    assert f"over {len(args) - len(goldens)} inputs" in r.stdout, r.stdout
