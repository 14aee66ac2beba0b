"""Tables with several complex (map<blob,blob>) columns, CPU side: the
oracle, unchanged, is the reference for them, and the host schema resolver
counts the trailing map columns."""
import os
import subprocess

import pytest

from conftest import ORACLE, REPO
from multi_cpx_helpers import CASES, base_name, widen_tool, widened  # noqa: F401


@pytest.mark.parametrize("case", sorted(CASES))
def test_oracle_is_the_reference(widened, tmp_path, case):
    """Every widened input re-serializes byte-identically through the oracle
    (all components OK), and the oracle compacts the three of them, plain and
    purging. (Each input's mixed_del / del_only / partial counts are asserted
    positive where the inputs are built.)"""
    bases = widened[case]["bases"]
    for b in bases:
        r = subprocess.run([ORACLE, "roundtrip", b], capture_output=True, text=True)
        assert r.returncode == 0 and "FAIL" not in r.stdout and "OK" in r.stdout, (
            b, r.stdout + r.stderr)
    for tag, extra in (("plain", []), ("purge", ["gcbefore=2000000000", "now=2000000000"])):
        out = str(tmp_path / f"{tag}_{base_name(case, 90)}")
        r = subprocess.run([ORACLE, "compact", out, *bases, *extra],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        assert os.path.getsize(out + "-Data.db") > 0


def test_resolve_schema_counts_trailing_maps(widened, tmp_path):
    """resolve_schema on a widened Statistics.db gives n_cpx == 3 with two
    simple columns; a map before a simple column, a counter table with a
    map, another collection type, a map static and 62 + 2 columns all throw.
    Built with the address and undefined-behaviour sanitizers."""
    exe = str(tmp_path / "multi_cpx_schema_test")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(REPO, "tests/native/multi_cpx_schema_test.cpp"),
                    "-o", exe], check=True, capture_output=True)
    r = subprocess.run([exe, widened["a"]["bases"][0] + "-Statistics.db"],
                       capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout + r.stderr
