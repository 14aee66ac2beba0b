"""CPU side of the size-split (max_output_bytes) tests: the reference that
the GPU tests compare against is checked against itself and against vacuity,
and the C structs match the ctypes ones."""
import os
import subprocess

import chunk_helpers as ch
from conftest import REPO
from multi_cpx_helpers import widen_tool, widened  # noqa: F401  (fixtures)
from size_split_helpers import (CASES, est_on_disk, last_partition_offset, oracle_compact,
                                size_split_tool, split_ref)  # noqa: F401  (fixtures)


def _cinfo(base):
    with open(base + "-CompressionInfo.db", "rb") as f:
        _n, _o, chunk_len, _mc, data_len, offsets = ch.parse_compression_info(f.read())
    return chunk_len, data_len, offsets


def test_reference_is_consistent(split_ref, tmp_path):
    for case, ref in split_ref.items():
        outs, cap = ref["outputs"], ref["cap"]
        assert outs, case
        for a, b in zip(outs, outs[1:]):
            assert a["first_token"] <= a["last_token"] < b["first_token"], (case, a, b)
        assert outs[-1]["first_token"] <= outs[-1]["last_token"]
        assert sum(o["partitions"] for o in outs) == ref["r"]["partitions_out"], case
        for k, o in enumerate(outs):
            assert o["oracle"]["partitions_out"] == o["partitions"], (case, k)
            chunk_len, data_len, offsets = _cinfo(o["base"])
            size = os.path.getsize(o["base"] + "-Data.db")
            if k + 1 < len(outs):
                # the estimate only counts bytes that are in the file
                assert size > cap, (case, k, size)
                assert est_on_disk(offsets, chunk_len, data_len) > cap, (case, k)
            if o["partitions"] >= 2:
                if CASES[case].get("bti"):
                    # no Index.db: size the last partition as an output of its own
                    one = oracle_compact(str(tmp_path / f"da-{k}-bti"), ref["inputs"],
                                         [f"shard={o['last_token']}:{o['last_token']}"])
                    assert one["partitions_out"] == 1
                    before = data_len - _cinfo(str(tmp_path / f"da-{k}-bti"))[1]
                else:
                    before = last_partition_offset(o["base"])
                assert 0 < before < data_len
                assert est_on_disk(offsets, chunk_len, before) <= cap, (case, k, before)


def test_reference_is_not_vacuous(split_ref):
    for case, ref in split_ref.items():
        print(case, len(ref["outputs"]), [o["partitions"] for o in ref["outputs"]][:12])
        assert len(ref["outputs"]) >= ref["min_outputs"], (case, len(ref["outputs"]))
    assert len(split_ref["a_nocut"]["outputs"]) == 1
    b = split_ref["b"]
    assert any(o["partitions"] == 1 and os.path.getsize(o["base"] + "-Data.db") > b["cap"]
               for o in b["outputs"])
    assert split_ref["e_purge"]["r"]["partitions_out"] < split_ref["a"]["r"]["partitions_out"]
    assert split_ref["e_gc"]["r"]["partitions_out"] > 0
    # (g) restricts: fewer partitions than the unrestricted job
    assert 0 < split_ref["g"]["r"]["partitions_out"] < split_ref["a"]["r"]["partitions_out"]


PROBE = r"""
#include <stdio.h>
#include <stddef.h>
#include "gpucompact.h"
int main(void) {
    printf("%zu %zu %zu %zu\n", offsetof(gpuc_job, max_output_bytes), sizeof(gpuc_job),
           offsetof(gpuc_result, n_outputs), sizeof(gpuc_result));
    return 0;
}
"""


def test_abi_matches_ctypes(tmp_path):
    import cassandra_amd as ca
    src = tmp_path / "probe.c"
    src.write_text(PROBE)
    exe = str(tmp_path / "probe")
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), str(src), "-o", exe], check=True,
                   capture_output=True)
    got = [int(x) for x in subprocess.run([exe], check=True, capture_output=True,
                                          text=True).stdout.split()]
    assert got == [ca.GpucJob.max_output_bytes.offset, ctypes_sizeof(ca.GpucJob),
                   ca.GpucResult.n_outputs.offset, ctypes_sizeof(ca.GpucResult)]


def ctypes_sizeof(t):
    import ctypes
    return ctypes.sizeof(t)
