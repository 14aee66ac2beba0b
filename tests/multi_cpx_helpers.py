"""Shared inputs for the multi-complex-column tests: oracle-generated
sstables widened to several map<blob,blob> columns by
tests/native/multi_cpx_widen.cpp. Built once per session and never modified
by the tests that use them."""
import os
import re
import subprocess

import pytest

from conftest import ORACLE, REPO

COMPONENTS = ["Data.db", "Index.db", "CompressionInfo.db", "Filter.db",
              "Digest.crc32", "Statistics.db", "Summary.db"]
BTI_COMPONENTS = ["Data.db", "Partitions.db", "Rows.db", "CompressionInfo.db",
                  "Filter.db", "Digest.crc32", "Statistics.db"]

# case -> (gen spec, widen args, bti)
CASES = {
    # three complex columns, so one is in the middle
    "a": ("seed=5 rows=60 vlen=60 overlap=50 tomb=15 ncols=2 colmiss=30 cpx=70 "
          "cpxdel=30 ttl=20", ["2"], False),
    # wide partitions past column_index_size, markers, statics
    "b": ("seed=6 rows=6 crows=200 vlen=400 overlap=60 rtomb=30 statics=40 cpx=60 "
          "cpxdel=30 tomb=10", ["1"], False),
    # zero simple columns
    "c": ("seed=7 rows=80 vlen=40 overlap=50 tomb=20 cpx=70 cpxdel=30", ["1", "strip"],
          False),
    # da + Snappy
    "d": ("seed=8 rows=20 crows=10 vlen=50 overlap=50 cpx=60 cpxdel=30 bti=1 snappy=1",
          ["2"], True),
}


def components(case):
    return BTI_COMPONENTS if CASES[case][2] else COMPONENTS


def base_name(case, gen):
    return f"da-{gen}-bti" if CASES[case][2] else f"oa-{gen}-big"


def assert_same_components(got_base, want_base, comps):
    for comp in comps:
        with open(f"{got_base}-{comp}", "rb") as f:
            got = f.read()
        with open(f"{want_base}-{comp}", "rb") as f:
            want = f.read()
        if got != want:
            n = min(len(got), len(want))
            i = next((j for j in range(n) if got[j] != want[j]), n)
            raise AssertionError(
                f"{comp}: got {len(got)} bytes, want {len(want)}, first diff at {i}")


@pytest.fixture(scope="session")
def widen_tool(oracle_bin, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("widen_tool") / "widen")
    src = [os.path.join(REPO, "tests/native/multi_cpx_widen.cpp")] + [
        os.path.join(REPO, "oracle/src", f)
        for f in ("sstable.cpp", "compact.cpp", "gen.cpp", "bti.cpp")]
    subprocess.run(["g++", "-O2", "-std=c++17", *src, "-o", exe, "-l:liblz4.so.1", "-ldl"],
                   check=True, capture_output=True)
    return exe


@pytest.fixture(scope="session")
def widened(widen_tool, tmp_path_factory):
    """case -> {"bases": [three widened input bases], "counts": [per input
    {mixed_del, del_only, partial}]}. Every input must exercise a real
    deletion next to a live one, a deletion-only column and a partly
    present column set."""
    out = {}
    for case, (spec, wargs, _) in CASES.items():
        raw = str(tmp_path_factory.mktemp(f"mcpx_raw_{case}"))
        wide = str(tmp_path_factory.mktemp(f"mcpx_{case}"))
        subprocess.run([ORACLE, "gen", raw, "n=3", *spec.split()], check=True,
                       capture_output=True)
        bases, counts = [], []
        for g in (1, 2, 3):
            src = os.path.join(raw, base_name(case, g))
            dst = os.path.join(wide, base_name(case, g))
            r = subprocess.run([widen_tool, src, dst, *wargs], check=True,
                               capture_output=True, text=True)
            m = re.search(r"mixed_del=(\d+) del_only=(\d+) partial=(\d+)", r.stdout)
            assert m, r.stdout + r.stderr
            c = dict(zip(("mixed_del", "del_only", "partial"), map(int, m.groups())))
            assert all(v > 0 for v in c.values()), (case, g, c)
            bases.append(dst)
            counts.append(c)
        out[case] = {"bases": bases, "counts": counts}
    return out
