"""CPU tests of the Merkle-leaf validation entry point (gpuc_validate_merkle):
the host-only spec code of cassandra_amd/csrc/merkle_spec.h in a native test
built with plain g++ (no HIP), and every refusal the real library makes before
it probes a device: malformed leaf bounds and the job modes validation does
not take."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import ORACLE, REPO

SRC = os.path.join(REPO, "tests", "native", "merkle_spec_test.cpp")
UNSUPPORTED, NO_GPU = 3, 4


def test_merkle_spec_native(oracle_bin, tmp_path):
    """Lookup + host reducer against a linear-scan assignment on an oracle
    validate file, and the spec check on every malformed spec."""
    d = str(tmp_path)
    subprocess.run([ORACLE, "gen", d, "seed=5", "n=3", "rows=900", "vlen=100", "overlap=25",
                    "tomb=15", "pdel=2"], check=True, capture_output=True)
    ins = [f"{d}/oa-{g}-big" for g in (1, 2, 3)]
    vfile = f"{d}/v_cpu.bin"
    subprocess.run([ORACLE, "validate", vfile, *ins, "gcbefore=1900000000", "now=1900000000"],
                   check=True, capture_output=True)
    binp = str(tmp_path / "merkle_spec_test")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-o", binp, SRC],
                   check=True)
    r = subprocess.run([binp, vfile], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.splitlines()[-1].startswith("OK merkle_spec"), r.stdout
    assert len(re.findall(r"^layout ", r.stdout, re.M)) == 5, r.stdout
    assert "14 malformed specs refused" in r.stdout, r.stdout


@pytest.fixture(scope="module")
def ca(product_lib):
    import cassandra_amd as mod
    return mod


def _refused(ca, match, **kw):
    """The call must fail with GPUC_ERR_UNSUPPORTED and name `match`."""
    kw.setdefault("trees", None)
    with pytest.raises(ca.GpuCompactError) as ei:
        ca.validate_merkle(["/nonexistent/oa-1-big"], **kw)
    msg = str(ei.value)
    assert f"rc={UNSUPPORTED}:" in msg, msg
    assert match in msg, msg


# (n_trees, tree_left, leaf_begin, leaf_right) handed over unchecked, and what
# the message must name
BAD_SPECS = {
    "null_tree_left": ((2, None, [0, 2, 3], [10, 20, 40]), "tree_left"),
    "null_leaf_begin": ((2, [0, 30], None, [10, 20, 40]), "leaf_begin"),
    "null_leaf_right": ((2, [0, 30], [0, 2, 3], None), "leaf_right"),
    "no_trees": ((0, [0, 30], [0, 2, 3], [10, 20, 40]), "n_trees"),
    "begin_not_zero": ((2, [0, 30], [1, 2, 3], [10, 20, 40]), "leaf_begin[0]"),
    "empty_tree": ((2, [0, 30], [0, 2, 2], [10, 20, 40]), "tree 1"),
    "begin_decreasing": ((2, [0, 30], [0, 2, 1], [10, 20, 40]), "tree 1"),
    "first_leaf_not_above_left": ((2, [10, 30], [0, 2, 3], [10, 20, 40]), "leaf 0"),
    "first_leaf_of_tree_1": ((2, [0, 40], [0, 2, 3], [10, 20, 40]), "leaf 2"),
    "right_not_ascending": ((2, [0, 30], [0, 2, 3], [10, 10, 40]), "leaf 1"),
    "overlapping_trees": ((2, [0, 19], [0, 2, 3], [10, 20, 40]), "tree 1"),
    "unordered_trees": ((2, [30, 0], [0, 2, 3], [40, 50, 10]), "tree 1"),
    "too_many_leaves": ((1, [0], [0, 2 ** 31], [10]), str(2 ** 31)),
}


@pytest.mark.parametrize("name", sorted(BAD_SPECS))
def test_malformed_spec_refused(ca, name):
    raw, match = BAD_SPECS[name]
    _refused(ca, match, raw_spec=raw)


def test_null_spec_refused(ca):
    _refused(ca, "NULL", raw_spec=None)


GOOD_TREES = [(0, [10, 20]), (30, [40])]


@pytest.mark.parametrize("mode", [
    dict(n_output_shards=2),
    dict(max_output_bytes=1 << 20),
    dict(tombstone_sources=["/nonexistent/oa-2-big"]),
    dict(keep_ranges=[(0, 100)]),
], ids=["shards", "size_split", "tomb_sources", "keep_ranges"])
def test_rejected_job_modes(ca, mode):
    """Rejected as gpuc_validate rejects them, whatever the spec."""
    _refused(ca, "unsupported", trees=GOOD_TREES, **mode)


def test_well_formed_call_needs_a_gpu(ca):
    if ca.device_count() > 0:
        pytest.skip("GPU present; the no-GPU refusal is exercised on CPU boxes")
    with pytest.raises(ca.GpuCompactError, match=f"rc={NO_GPU}:"):
        ca.validate_merkle(["/nonexistent/oa-1-big"], GOOD_TREES)


def test_declared_and_exported(product_lib):
    hdr = open(os.path.join(REPO, "include", "gpucompact.h")).read()
    assert re.search(r"^int gpuc_validate_merkle\(const gpuc_job\* job, "
                     r"const gpuc_merkle_spec\* spec,", hdr, re.M)
    assert "typedef struct gpuc_merkle_spec {" in hdr
    lib = ctypes.CDLL(product_lib)
    assert hasattr(lib, "gpuc_validate_merkle")
