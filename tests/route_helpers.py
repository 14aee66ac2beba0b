"""Shared by the routed-output tests: the oracle runs and the per-output check.

The reference of every output is the oracle's compaction of the same inputs
restricted to that output's ranges (`ranges=`; the default output is
`invertranges=1` over the ranges of all other outputs), one oracle run per
output, compared byte for byte in every component file. An output the oracle
leaves empty must not be written at all."""
import glob
import json
import os
import struct
import subprocess

from conftest import ORACLE
from multi_cpx_helpers import BTI_COMPONENTS, COMPONENTS, assert_same_components


def gen(d, spec):
    os.makedirs(d, exist_ok=True)
    subprocess.run([ORACLE, "gen", d, *spec.split()], check=True, capture_output=True)
    kv = dict(a.split("=") for a in spec.split())
    stem = "da-{}-bti" if kv.get("bti") == "1" else "oa-{}-big"
    return [f"{d}/" + stem.format(g) for g in range(1, int(kv["n"]) + 1)]


def oracle_compact(out, inputs, *args):
    os.makedirs(os.path.dirname(out), exist_ok=True)
    r = subprocess.run([ORACLE, "compact", out, *inputs, *args], check=True,
                       capture_output=True, text=True)
    return json.loads(r.stdout.splitlines()[-1])


def kept_tokens(inputs, *args):
    """Sorted distinct tokens of the partitions a compaction keeps."""
    vfile = os.path.join(os.path.dirname(inputs[0]), "kept_tokens.bin")
    subprocess.run([ORACLE, "validate", vfile, *inputs, *args], check=True, capture_output=True)
    raw = open(vfile, "rb").read()
    return sorted({struct.unpack_from(">q", raw, o)[0] for o in range(0, len(raw), 40)})


def rs(ranges):
    return "ranges=" + ",".join(f"{lo}:{hi}" for lo, hi in ranges)


def route_and_check(ca, ins, d, ranges, default, n_out, oracle_ins=None, oracle_args=(),
                    bti=False, **job):
    """One routed call, one oracle run per output. Returns (result, oracle
    partition counts per output)."""
    stem = "da-{}-bti" if bti else "oa-{}-big"
    comps = (BTI_COMPONENTS if bti else COMPONENTS) + ["TOC.txt"]
    os.makedirs(f"{d}/gpu", exist_ok=True)
    bases = [f"{d}/gpu/" + stem.format(10 + o) for o in range(n_out)]
    r = ca.compact_routed(ins, bases, ranges, default, **job)
    assert len(r["outputs"]) == n_out
    want_parts = []
    for o in range(n_out):
        if o == default:
            others = [(lo, hi) for lo, hi, t in ranges if t != o]
            sel = [rs(others), "invertranges=1"] if others else []
        else:
            mine = [(lo, hi) for lo, hi, t in ranges if t == o]
            assert mine, f"output {o} has no range: the test's own table is wrong"
            sel = [rs(mine)]
        cpu = f"{d}/cpu/" + stem.format(10 + o)
        w = oracle_compact(cpu, oracle_ins or ins, *oracle_args, *sel)
        got = r["outputs"][o]
        want_parts.append(w["partitions_out"])
        if w["partitions_out"] == 0:
            assert got["written"] == 0 and got["partitions"] == 0, (o, got)
            assert not glob.glob(bases[o] + "-*"), f"output {o} is empty but has files"
            continue
        assert got["written"] == 1, (o, got)
        assert (got["partitions"], got["rows"]) == (w["partitions_out"], w["rows_out"]), (o, got, w)
        try:
            assert_same_components(bases[o], cpu, comps)
        except AssertionError as e:
            raise AssertionError(f"output {o}: {e}")
        assert got["compressed_bytes"] == os.path.getsize(bases[o] + "-Data.db")
        ca.verify(bases[o])
    written = [o for o in r["outputs"] if o["written"]]
    assert r["n_outputs"] == len(written)
    assert r["partitions_out"] == sum(want_parts)
    assert r["rows_out"] == sum(o["rows"] for o in written)
    assert r["output_compressed_bytes"] == sum(o["compressed_bytes"] for o in written)
    assert r["output_uncompressed_bytes"] == sum(o["uncompressed_bytes"] for o in written)
    return r, want_parts
